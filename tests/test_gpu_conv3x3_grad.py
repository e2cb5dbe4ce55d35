"""dc_op_conv3x3_grad and its weight-gradient kernel alone (include/densecap_debug_rpn.h) against the float64 autograd
restatement of tests/rpn_grad_rules.py.

Every tensor is held to max|dev - ref64| <= REL * max|ref64| and, per row (dw per output channel, dx per pixel), to
tests/grad_bars.py's bar: FACTOR times the worst row of the same rules evaluated in float32 on the CPU, computed here.  The
operands lie in one device block with NaN between them and the outputs in another between sentinels, so a read or a write one
element outside an operand shows."""
import ctypes as C

import numpy as np
import pytest

from tests import grad_bars as GB
from tests import rpn_grad_rules as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = F32(-7.25)
GAP = 64                           # floats between two buffers of a block (keeps every buffer 256-byte aligned)
INVALID, UNSUPPORTED = -1, -5

# (h, w, Cin, Cout): the 1x1 map has only the centre tap inside; single rows and columns; 2x2 and 3x3 (every pixel on the border
# / one interior pixel); Cin = 96, Cout = 160: 128-column tiles straddle taps and the last tile of both dimensions is partial;
# h * w = 15, 16, 17 and 33 sit around the staging step of 16 pixels
SHAPES = [(1, 1, 32, 32), (1, 5, 32, 32), (5, 1, 32, 32), (2, 2, 32, 32), (3, 3, 32, 32), (6, 8, 96, 160),
          (3, 5, 32, 32), (4, 4, 32, 32), (1, 17, 32, 32), (3, 11, 32, 32)]


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _block(parts, fill):
    """One float32 host array holding `parts` (name -> array or None) GAP floats apart, `fill` everywhere else; the offsets."""
    off, n = {}, GAP
    for k, a in parts.items():
        if a is not None:
            off[k] = n
            n += (a.size + GAP - 1) // GAP * GAP + GAP
    host = np.full(n, fill, F32)
    for k, o in off.items():
        host[o:o + parts[k].size] = parts[k].reshape(-1)
    return host, off


def _at(dev, off):
    return C.c_void_p(dev.ptr.value + 4 * off)


def run(ctx, x, w, dy, want=("dw", "db", "dx"), dims=None, hook_slices=None):
    """The call on CHW / OIHW numpy operands (any may be None).  Returns (rc, outputs in the rules' layouts); asserts that nothing
    outside the wanted outputs was written."""
    if dims is None:
        Cout, h, wd = dy.shape
        Cin = x.shape[0] if x is not None else w.shape[1]
        dims = (h, wd, Cin, Cout)
    h, wd, Cin, Cout = dims
    hwc = lambda a: None if a is None else np.ascontiguousarray(a.transpose(1, 2, 0))
    ins, ioff = _block({"x": hwc(x), "w": w, "dy": hwc(dy)}, np.nan)
    shapes = {"dw": (Cout, Cin, 3, 3), "db": (Cout,), "dx": (h, wd, Cin)}
    ok_shape = min(dims) > 0 and h * wd <= 65536
    outs0, ooff = _block({k: np.full(shapes[k] if ok_shape else (8,), SENTINEL, F32) for k in want}, SENTINEL)
    di, do = ctx.to_device(ins), ctx.to_device(outs0)
    pi = lambda k: _at(di, ioff[k]) if k in ioff else None
    po = lambda k: _at(do, ooff[k]) if k in ooff else None
    if hook_slices is None:
        rc = ctx.lib.dc_op_conv3x3_grad(ctx.h, pi("x"), pi("w"), pi("dy"), h, wd, Cin, Cout, po("dw"), po("db"), po("dx"))
    else:
        rc = ctx.lib.dc_debug_conv3x3_wgrad(ctx.h, pi("x"), pi("dy"), h, wd, Cin, Cout, hook_slices, po("dw"))
    got = do.numpy()
    if rc != 0:
        assert np.array_equal(_bits(got), _bits(outs0)), "a refused call wrote to its outputs"
        return rc, {}
    out, mask = {}, np.ones(got.size, bool)
    for k in want:
        n = int(np.prod(shapes[k]))
        out[k] = got[ooff[k]:ooff[k] + n].reshape(shapes[k]).copy()
        mask[ooff[k]:ooff[k] + n] = False
    assert np.array_equal(_bits(got[mask]), _bits(outs0[mask])), "a write outside the output buffers"
    if "dx" in out:
        out["dx"] = np.ascontiguousarray(out["dx"].transpose(2, 0, 1))
    return rc, out


def check(what, dev, ref64, ref32):
    """REL on every tensor, the per-row bars on dw and dx; prints each figure before it asserts."""
    figs, bad = [], []
    for k in dev:
        scale = float(np.abs(ref64[k]).max())
        err = float(np.abs(dev[k].astype(np.float64) - ref64[k]).max())
        assert np.isfinite(dev[k]).all(), (what, k)
        figs.append("%s max-norm %.2e" % (k, err / scale if scale > 0 else err))
        if err > R.REL * scale:
            bad.append((k, "max-norm", err / max(scale, 1e-300)))
        if k in ("dw", "dx"):
            bar = GB.FACTOR * GB.worst(GB.row_ratios(R.rows(k, ref32[k]), R.rows(k, ref64[k])))
            worst, rows = GB.check_rows(k, R.rows(k, dev[k]), R.rows(k, ref64[k]), bar)
            figs.append("%s rows %.2e (bar %.2e)" % (k, worst, bar))
            if rows:
                bad.append((k, "rows, bar %.3e" % bar, rows))
    print("conv3x3_grad %s: " % what + ", ".join(figs))
    assert not bad, (what, bad)


def refs(x, w, dy):
    return R.conv3x3_grad(x, w, dy), R.conv3x3_grad(x, w, dy, dtype="float32")


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_%dto%d" % s for s in SHAPES])
def test_conv3x3_grad_matches_the_rules(ctx, shape):
    h, w, Cin, Cout = shape
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed=h * 100 + w * 10 + Cin)
    rc, dev = run(ctx, x, wt, dy)
    assert rc == 0
    ref64, ref32 = refs(x, wt, dy)
    check("%dx%d %d->%d" % shape, dev, ref64, ref32)
    rc, again = run(ctx, x, wt, dy)
    assert rc == 0 and all(np.array_equal(_bits(dev[k]), _bits(again[k])) for k in R.TENSORS)


def test_model_size_map_takes_slices_of_its_own_accord(ctx):
    """38 x 45, 512 -> 256: the RPN's convolution at 720 x 600, where the weight gradient's pixels are shared by several slices
    without being told to.  The hook with slices = 0 is the same launch: the same bits."""
    from densecap_amd import ops
    h, w, Cin, Cout = 38, 45, 512, 256
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed=7)
    rc, dev = run(ctx, x, wt, dy)
    assert rc == 0
    ref64, ref32 = refs(x, wt, dy)
    check("38x45 512->256", dev, ref64, ref32)
    assert np.array_equal(_bits(dev["dw"]), _bits(ops.conv3x3_wgrad(ctx, x, dy, 0)))
    assert not np.array_equal(_bits(dev["dw"]), _bits(ops.conv3x3_wgrad(ctx, x, dy, 1)))        # (one slice adds in another order)
    got = ops.conv3x3_grad(ctx, x, wt, dy)
    assert all(np.array_equal(_bits(dev[k]), _bits(got[k])) for k in R.TENSORS)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_forced_slice_counts_agree_and_add_in_slice_order(ctx, S):
    """7 x 9 = 63 pixels.  S = 2, 3: slices of 32 pixels, the boundary inside map row 3, a last slice of 31 (S = 3: and an empty
    one); S = 4: slices of 16, the last of 15.  The result is the rules' within the bars, and bit for bit the fp32 sum, in slice
    order, of the partial results -- each the one-slice kernel on a dy that is zero outside the slice's pixels (the zero
    products leave an accumulator's bits alone, and a slice starts on a staging step, so the partial is the slice's own)."""
    h, w, Cin, Cout = 7, 9, 32, 32
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed=79)
    rc, dev = run(ctx, x, None, dy, want=("dw",), hook_slices=S)
    assert rc == 0
    ref64, ref32 = refs(x, wt, dy)
    check("7x9 S=%d" % S, dev, {"dw": ref64["dw"]}, {"dw": ref32["dw"]})
    per = ((h * w + S - 1) // S + 15) // 16 * 16
    want = None
    for z in range(S):
        part = np.zeros_like(dy).reshape(Cout, -1)
        part[:, z * per:(z + 1) * per] = dy.reshape(Cout, -1)[:, z * per:(z + 1) * per]
        rc, p = run(ctx, x, None, part.reshape(dy.shape), want=("dw",), hook_slices=1)
        assert rc == 0
        want = p["dw"] if want is None else (want + p["dw"]).astype(F32)
    assert np.array_equal(_bits(dev["dw"]), _bits(want))
    rc, again = run(ctx, x, None, dy, want=("dw",), hook_slices=S)
    assert rc == 0 and np.array_equal(_bits(dev["dw"]), _bits(again["dw"]))


@pytest.mark.parametrize("o,y0,x0", [(3, 0, 0), (17, 0, 3), (31, 2, 3), (0, 4, 5)], ids=["corner", "edge", "interior", "last"])
def test_one_hot_gradient_is_exact(ctx, o, y0, x0):
    """dy is 1 at one pixel and channel, x and w are small integers: dw's row o is the shifted patch of x, dx the weights of o
    around the pixel, db the one-hot vector, every other element +0.0 -- bit for bit."""
    h, w, Cin, Cout = 5, 6, 32, 32
    rng = np.random.default_rng(o + y0 + x0)
    x = rng.integers(-4, 5, (Cin, h, w)).astype(F32)
    wt = rng.integers(-4, 5, (Cout, Cin, 3, 3)).astype(F32)
    dy = np.zeros((Cout, h, w), F32)
    dy[o, y0, x0] = 1
    rc, dev = run(ctx, x, wt, dy)
    assert rc == 0
    dw, dx = R.one_hot_expected(x, wt, o, y0, x0)
    assert np.array_equal(_bits(dev["dw"]), _bits(dw))
    assert np.array_equal(_bits(dev["dx"]), _bits(dx))
    assert np.array_equal(_bits(dev["db"]), _bits(dy[:, y0, x0]))


def test_zero_gradient_gives_plus_zero_bits(ctx):
    h, w, Cin, Cout = 6, 8, 96, 160
    x, wt, _ = R.make_case(h, w, Cin, Cout, seed=3)
    rc, dev = run(ctx, x, wt, np.zeros((Cout, h, w), F32))
    assert rc == 0
    for k in R.TENSORS:
        assert not _bits(dev[k]).any(), k


def test_null_outputs_are_skipped(ctx):
    """Every subset of the outputs gives the bits of the full call; the inputs an absent output alone reads may be absent too."""
    h, w, Cin, Cout = 4, 5, 32, 64
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed=11)
    rc, full = run(ctx, x, wt, dy)
    assert rc == 0
    for want in (("dw",), ("db",), ("dx",), ("dw", "db"), ("dw", "dx"), ("db", "dx")):
        rc, got = run(ctx, x if "dw" in want else None, wt if "dx" in want else None, dy, want=want, dims=(h, w, Cin, Cout))
        assert rc == 0 and sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(_bits(got[k]), _bits(full[k])), (want, k)


def test_refusals_leave_the_outputs_alone(ctx):
    x, wt, dy = R.make_case(4, 5, 32, 32, seed=13)
    h, w = 4, 5
    for dims in ((h, w, 48, 32), (h, w, 32, 48), (0, w, 32, 32), (h, 0, 32, 32), (h, w, 0, 32), (h, w, 32, 0), (-1, w, 32, 32)):
        assert run(ctx, x, wt, dy, dims=dims)[0] == INVALID, dims
    assert run(ctx, x, wt, dy, dims=(257, 256, 32, 32))[0] == UNSUPPORTED            # h * w = 65792 pixels
    assert run(ctx, x, wt, dy, dims=(h, w, 32, 32 * 66))[0] == UNSUPPORTED            # dx: 2112 channels into the engine
    assert run(ctx, None, wt, dy, dims=(h, w, 32, 32))[0] == INVALID                  # dw without x
    assert run(ctx, x, None, dy, dims=(h, w, 32, 32))[0] == INVALID                   # dx without w
    assert run(ctx, x, wt, None, dims=(h, w, 32, 32))[0] == INVALID
    assert run(ctx, x, wt, dy, want=())[0] == INVALID                                 # nothing asked for
    for S in (-1, 65):
        assert run(ctx, x, None, dy, want=("dw",), hook_slices=S)[0] == INVALID
    assert run(ctx, x, None, dy, want=("dw",), dims=(257, 256, 32, 32), hook_slices=1)[0] == UNSUPPORTED
    rc, dev = run(ctx, x, wt, dy)                                                    # and the context still works
    assert rc == 0
    check("after refusals", dev, *refs(x, wt, dy))
