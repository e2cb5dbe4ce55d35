"""dc_op_maxpool2x2_grad and dc_op_relu_grad, the two point-wise kernels of the CNN's backward, bit for bit against the selections
of tests/cnn_grad_rules.py.

The operands lie in one device block with a huge value between them (a stray read of the pooled map would win its window and
steal the gradient; a stray read of dpool would show in the output) and the output in another between sentinels, as
tests/test_gpu_conv3x3_grad.py lays its blocks out."""

import numpy as np
import pytest

from tests import cnn_grad_rules as CR
from tests.test_gpu_conv3x3_grad import SENTINEL, _at, _bits, _block

pytestmark = pytest.mark.gpu

F32 = np.float32
HUGE = F32(3e38)
INVALID = -1
# (n, H, W, C): a single element; single rows and columns; one full window; 3x3: every edge window clipped; 5x7 and 4x6 with
# C = 32 and C = 36 (not a multiple of 32); two images; 33x35x8: more than one workgroup (2448 threads)
POOL_SHAPES = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 4), (1, 2, 2, 4), (1, 3, 3, 4), (1, 5, 7, 32), (1, 4, 6, 36), (2, 5, 7, 8),
               (1, 33, 35, 8)]


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def run_pool(ctx, y, dpool, dims=None):
    """The call on (n, C, H, W) numpy operands.  Returns (rc, dy (n, C, H, W)); asserts that nothing outside dy was written."""
    (n, C_, H, W) = y.shape if dims is None else (dims[0], dims[3], dims[1], dims[2])         # dims: (n, H, W, C)
    hwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    ins, ioff = _block({"y": hwc(y), "g": hwc(dpool)}, HUGE)
    size = y.size if dims is None else max(8, abs(n * H * W * C_))       # (room for the shape even where it is to be refused)
    outs0, ooff = _block({"dy": np.full(size, SENTINEL, F32)}, SENTINEL)
    di, do = ctx.to_device(ins), ctx.to_device(outs0)
    rc = ctx.lib.dc_op_maxpool2x2_grad(ctx.h, _at(di, ioff["y"]), _at(di, ioff["g"]), n, H, W, C_, _at(do, ooff["dy"]))
    got = do.numpy()
    if rc != 0:
        assert np.array_equal(_bits(got), _bits(outs0)), "a refused call wrote to its output"
        return rc, None
    mask = np.ones(got.size, bool)
    mask[ooff["dy"]:ooff["dy"] + size] = False
    assert np.array_equal(_bits(got[mask]), _bits(outs0[mask])), "a write outside the output buffer"
    return rc, np.ascontiguousarray(got[ooff["dy"]:ooff["dy"] + size].reshape(n, H, W, C_).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["%dx%dx%dx%d" % s for s in POOL_SHAPES])
def test_pool_gradient_is_the_rules_selection(ctx, shape):
    n, H, W, C_ = shape
    y, g = CR.make_pool_case(C_, H, W, seed=H * 100 + W * 10 + C_, n=n)
    rc, dy = run_pool(ctx, y, g)
    assert rc == 0
    want = np.stack([CR.pool_relu_grad(y[m], g[m]) for m in range(n)])
    assert np.array_equal(_bits(dy), _bits(want))
    live = np.stack([CR.pool_relu_grad(y[m], np.ones_like(g[m])) for m in range(n)]) > 0
    assert not _bits(dy[~live]).any()                                   # everything the rule leaves out is +0.0, not -0.0
    from densecap_amd import ops
    assert np.array_equal(_bits(ops.maxpool2x2_grad(ctx, y, g)), _bits(want))


@pytest.mark.parametrize("place", range(4))
def test_positive_tie_goes_to_the_first_maximum(ctx, place):
    """Window (0, 0) of every channel holds its maximum at `place` and at every later place; the NaN of dpool lands on `place`
    alone.  A window of zeros, one of -0.0 and one of negatives (a map taken before the ReLU) give +0.0 everywhere."""
    y = np.zeros((1, 4, 4, 4), F32)
    win = np.full(4, 2, F32)
    win[:place] = 1
    y[0, :, 0:2, 0:2] = win.reshape(2, 2)
    y[0, :, 0:2, 2:4] = F32(-0.0)
    y[0, :, 2:4, 0:2] = np.array([[-1, -2], [-3, -0.5]], F32)
    g = np.arange(1, 17, dtype=F32).reshape(1, 4, 2, 2)
    g[0, :, 0, 0] = np.nan
    rc, dy = run_pool(ctx, y, g)
    assert rc == 0
    want = np.zeros_like(y)
    want[0, :, place // 2, place % 2] = np.nan
    assert np.array_equal(_bits(dy), _bits(want))
    assert np.array_equal(_bits(dy[0]), _bits(CR.pool_relu_grad(y[0], g[0])))


def run_relu(ctx, y, dy, off_y=0, off_dy=0, n=None):
    """The call on flat arrays placed off_y / off_dy floats past a 256-byte boundary.  Returns (rc, dy after the call)."""
    n = y.size if n is None else n
    pad = lambda a, o, fill: np.concatenate([np.full(o, fill, F32), a])
    ins, ioff = _block({"y": pad(y, off_y, HUGE)}, HUGE)
    io0, ooff = _block({"dy": pad(dy, off_dy, SENTINEL)}, SENTINEL)
    di, do = ctx.to_device(ins), ctx.to_device(io0)
    rc = ctx.lib.dc_op_relu_grad(ctx.h, _at(di, ioff["y"] + off_y), _at(do, ooff["dy"] + off_dy), n)
    got = do.numpy()
    if rc != 0:
        assert np.array_equal(_bits(got), _bits(io0)), "a refused call wrote to dy"
        return rc, None
    a = ooff["dy"] + off_dy
    mask = np.ones(got.size, bool)
    mask[a:a + n] = False
    assert np.array_equal(_bits(got[mask]), _bits(io0[mask])), "a write outside dy"
    return rc, got[a:a + n].copy()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 70001])
@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (1, 0), (0, 3)], ids=["aligned", "both+4B", "y+4B", "dy+12B"])
def test_relu_mask_is_the_rules_selection(ctx, n, offs):
    """+0.0, -0.0, the smallest denormals of both signs, a NaN in y (not > 0: dead), NaN and infinity in dy on live and dead
    places; n not a multiple of 4; either pointer 4 bytes off a 16-byte boundary."""
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n).astype(F32)
    dy = (rng.standard_normal(n) * 3).astype(F32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.nan, 1.0, -1.0, 2.0, -2.0], F32)
    gspec = np.array([1, 2, 3, 4, 5, 6, 7, np.nan, np.nan, np.inf, -np.inf], F32)
    k = min(n, special.size)
    y[n - k:] = special[:k]
    dy[n - k:] = gspec[:k]
    rc, got = run_relu(ctx, y, dy, *offs)
    assert rc == 0
    want = CR.relu_grad(y, dy)
    assert np.array_equal(_bits(got), _bits(want))
    if n == 1027 and offs == (0, 0):
        from densecap_amd import ops
        assert np.array_equal(_bits(ops.relu_grad(ctx, y, dy)), _bits(want))
        assert _bits(want[n - k:])[2] == _bits(gspec)[2] and not _bits(want[n - k:])[[0, 1, 3, 5, 6]].any()   # (the rule itself)


def test_refusals_leave_the_outputs_alone(ctx):
    y, g = CR.make_pool_case(8, 4, 6, seed=1)
    for dims in ((1, 4, 6, 6), (1, 4, 6, 2), (0, 4, 6, 8), (1, 0, 6, 8), (1, 4, 0, 8), (1, 4, 6, 0), (1, 4, 6, -4), (-1, 4, 6, 8)):
        assert run_pool(ctx, y, g, dims=dims)[0] == INVALID, dims
    a = np.ones(8, F32)
    for n in (0, -1, -2 ** 40):
        assert run_relu(ctx, a, a, n=n)[0] == INVALID, n
    assert ctx.lib.dc_op_relu_grad(ctx.h, None, None, 8) == INVALID
    big = ctx.to_device(np.full(3 * 256, SENTINEL, F32))                  # y, dpool, dy of a 2x2x4 map; one of them 4 bytes off
    for off in ((1, 64, 128), (0, 65, 128), (0, 64, 129)):
        assert ctx.lib.dc_op_maxpool2x2_grad(ctx.h, _at(big, off[0]), _at(big, off[1]), 1, 2, 2, 4, _at(big, off[2])) == INVALID, off
    assert np.array_equal(_bits(big.numpy()), _bits(np.full(3 * 256, SENTINEL, F32)))
    assert ctx.lib.dc_op_maxpool2x2_grad(ctx.h, None, None, 1, 4, 6, 8, None) == INVALID
    rc, dy = run_pool(ctx, y, g)                                          # and the context still works
    assert rc == 0 and np.array_equal(_bits(dy[0]), _bits(CR.pool_relu_grad(y[0], g[0])))
