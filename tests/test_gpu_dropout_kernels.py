"""dc_op_dropout and dc_op_relu_dropout_grad (docs/SEMANTICS.md, "Dropout"), the two point-wise kernels of dropout.hip, bit for
bit against tests/dropout_rules.py.  NaN is compared as NaN, a dropped element as +0.0 bits.

The matrix lies in a device block between sentinels, as tests/test_gpu_cnn_kernels.py lays its blocks out; a thread of the forward
owns one run of four columns of one row and a workgroup 256 of them, so (2, 4096) and (257, 516) take more than one workgroup and
4095 / 4096 / 4097 columns sit around a whole number of runs; one float past a 256-byte boundary every access is scalar."""
import numpy as np
import pytest

from tests import dropout_rules as DR
from tests.test_gpu_conv3x3_grad import SENTINEL, _at, _bits, _block

pytestmark = pytest.mark.gpu

F32 = np.float32
HUGE = F32(3e38)
INVALID = -1
SHAPES = [(1, 1), (1, 3), (1, 5), (3, 7), (5, 4), (2, 4096), (257, 516), (1, 4095), (1, 4096), (1, 4097)]
PS = (0.0, 0.1, 0.5, 0.999)
SEED = 2 ** 33 + 12345
SPECIAL = np.array([-0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, 0.0], F32)
_words = {}


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()
    _words.clear()


def keep_of(rows, cols, layer, p, seed):
    """The rule's mask; the Philox words of a (shape, layer, seed) are drawn once for every p."""
    key = (rows, cols, layer, seed)
    if key not in _words:
        _words[key] = DR.words(rows, cols, layer, seed).astype(np.uint64)
    return _words[key] < np.uint64(DR.threshold(p))


def matrix(rows, cols, seed):
    """Normal values with -0.0, denormals, infinities, NaN and +0.0 on every eleventh place (and on the first)."""
    x = np.random.default_rng(seed).standard_normal(rows * cols).astype(F32)
    at = np.arange(0, x.size, 11)
    x[at] = SPECIAL[np.arange(len(at)) % len(SPECIAL)]
    return x.reshape(rows, cols)


def same(got, want):
    """Bit equality, NaN against NaN."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def run_dropout(ctx, x, layer, p, seed, off=0, dims=None):
    """The call on a (rows, cols) matrix placed `off` floats past a 256-byte boundary.  Returns (rc, the matrix after the call);
    asserts that nothing outside it was written, and nothing at all by a refused call."""
    rows, cols = x.shape if dims is None else dims
    io0, ooff = _block({"x": np.concatenate([np.full(off, SENTINEL, F32), x.reshape(-1)])}, SENTINEL)
    dev = ctx.to_device(io0)
    rc = ctx.lib.dc_op_dropout(ctx.h, _at(dev, ooff["x"] + off), rows, cols, layer, p, seed)
    got = dev.numpy()
    if rc != 0:
        assert np.array_equal(_bits(got), _bits(io0)), "a refused call wrote to x"
        return rc, None
    a = ooff["x"] + off
    outside = np.ones(got.size, bool)
    outside[a:a + x.size] = False
    assert np.array_equal(_bits(got[outside]), _bits(io0[outside])), "a write outside x"
    return rc, got[a:a + x.size].reshape(x.shape).copy()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_dropout_is_the_rule_bit_for_bit(ctx, shape):
    rows, cols = shape
    x = matrix(rows, cols, rows * 7 + cols)
    for off in (0, 1):
        for p in PS:
            rc, got = run_dropout(ctx, x, 1, p, SEED, off)
            assert rc == 0
            if p == 0.0:
                assert np.array_equal(_bits(got), _bits(x)), (off, "p = 0 is the identity, NaN payloads included")
                continue
            keep = keep_of(rows, cols, 1, p, SEED)
            assert same(got, DR.apply_mask(x, keep, p)), (off, p)
            assert not _bits(got[~keep]).any(), (off, p, "a dropped element is +0.0 bits, whatever it was")


def test_two_calls_agree_and_layers_and_seeds_differ(ctx):
    from densecap_amd import ops
    x = np.abs(matrix(65, 260, 3)) + F32(1)
    x[~np.isfinite(x)] = F32(1)
    a = run_dropout(ctx, x, 1, 0.5, SEED)[1]
    assert np.array_equal(_bits(a), _bits(run_dropout(ctx, x, 1, 0.5, SEED)[1]))
    assert np.array_equal(_bits(a), _bits(ops.dropout(ctx, x, 1, 0.5, SEED)))
    for layer, seed in ((2, SEED), (1, SEED ^ (1 << 40)), (1, SEED ^ 1), (0, SEED), (255, SEED)):
        b = run_dropout(ctx, x, layer, 0.5, seed)[1]
        assert np.array_equal(b > 0, keep_of(65, 260, layer, 0.5, seed)), (layer, seed)
        assert not np.array_equal(b > 0, a > 0), (layer, seed)
    frac = float((a > 0).mean())                         # (the rule's own fraction is checked on the CPU; this is bit equality)
    assert frac == float(keep_of(65, 260, 1, 0.5, SEED).mean())


def test_the_mask_does_not_depend_on_the_matrix_it_is_part_of(ctx):
    """The first rows and columns of a larger call: a pure function of (seed, layer, row, col, p)."""
    big = np.ones((9, 23), F32)
    a = run_dropout(ctx, big, 2, 0.1, 5)[1]
    b = run_dropout(ctx, np.ones((4, 7), F32), 2, 0.1, 5)[1]
    c = run_dropout(ctx, np.ones((4, 8), F32), 2, 0.1, 5, off=1)[1]
    assert np.array_equal(_bits(a[:4, :7]), _bits(b)) and np.array_equal(_bits(a[:4, :8]), _bits(c))
    assert np.array_equal(_bits(a), _bits(DR.dropout_forward(big, 2, 0.1, 5))) and _bits(a).any() and not _bits(a).all()


def run_grad(ctx, y, dy, p, off_y=0, off_dy=0, n=None):
    n = y.size if n is None else n
    pad = lambda a, o, fill: np.concatenate([np.full(o, fill, F32), a.reshape(-1)])
    ins, ioff = _block({"y": pad(y, off_y, HUGE)}, HUGE)
    io0, ooff = _block({"dy": pad(dy, off_dy, SENTINEL)}, SENTINEL)
    di, do = ctx.to_device(ins), ctx.to_device(io0)
    rc = ctx.lib.dc_op_relu_dropout_grad(ctx.h, _at(di, ioff["y"] + off_y), _at(do, ooff["dy"] + off_dy), n, p)
    got = do.numpy()
    if rc != 0:
        assert np.array_equal(_bits(got), _bits(io0)), "a refused call wrote to dy"
        return rc, None
    a = ooff["dy"] + off_dy
    outside = np.ones(got.size, bool)
    outside[a:a + n] = False
    assert np.array_equal(_bits(got[outside]), _bits(io0[outside])), "a write outside dy"
    return rc, got[a:a + n].copy()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_relu_dropout_grad_is_the_numpy_form(ctx, shape):
    from densecap_amd import ops
    n = shape[0] * shape[1]
    y = matrix(1, n, n + 1).reshape(-1)
    dy = matrix(1, n, n + 2).reshape(-1)[::-1].copy()
    for offs in ((0, 0), (1, 1), (1, 0), (0, 3)):
        for p in PS:
            rc, got = run_grad(ctx, y, dy, p, *offs)
            assert rc == 0
            want = DR.relu_dropout_grad(y, dy, p)
            assert same(got, want), (offs, p)
            assert not _bits(got[~(y > 0)]).any(), (offs, p)
            if p == 0.0:
                assert np.array_equal(_bits(got), _bits(ops.relu_grad(ctx, y, dy))), offs
    assert same(ops.relu_dropout_grad(ctx, y, dy, 0.1), DR.relu_dropout_grad(y, dy, 0.1))


def test_refusals_leave_the_buffers_alone(ctx):
    x = np.ones((4, 8), F32)
    for p in (np.nan, -0.1, 1.0, 1.5, np.inf, -np.inf):
        assert run_dropout(ctx, x, 1, p, 3)[0] == INVALID, p
        assert run_grad(ctx, x, x, p)[0] == INVALID, p
    for dims in ((0, 8), (-1, 8), (4, 0), (4, -8)):
        assert run_dropout(ctx, x, 1, 0.5, 3, dims=dims)[0] == INVALID, dims
        assert run_dropout(ctx, x, 1, 0.0, 3, dims=dims)[0] == INVALID, dims
    for layer in (-1, 256, 2 ** 20):
        assert run_dropout(ctx, x, layer, 0.5, 3)[0] == INVALID, layer
    for n in (0, -1, -2 ** 40):
        assert run_grad(ctx, x, x, 0.5, n=n)[0] == INVALID, n
    assert ctx.lib.dc_op_dropout(ctx.h, None, 4, 8, 1, 0.5, 3) == INVALID
    assert ctx.lib.dc_op_relu_dropout_grad(ctx.h, None, None, 8, 0.5) == INVALID
    rc, got = run_dropout(ctx, x, 1, 0.5, 3)                  # and the context still works
    assert rc == 0 and np.array_equal(_bits(got), _bits(DR.dropout_forward(x, 1, 0.5, 3)))
