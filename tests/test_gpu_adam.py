"""dc_op_adam (docs/SEMANTICS.md, "Training step") against the float32 restatement of tests/optim_rules.py, bit for bit over p, m
and v: every size class of the kernel (below one vector, one chunk of 4096 less / exactly / more, several chunks), every offset
from 16-byte alignment, zeros, denormals of both signs and values near FLT_MAX, the multi-segment launch of dc_train_step
against per-segment calls, and the refusals."""
import numpy as np
import pytest

from tests import optim_rules as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027, 65541)
OPTS = dict(learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)
FLT_MAX = np.finfo(F32).max
DENORM = np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1e-38], F32)


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _inputs(n, seed):
    """p, g, m, v (v >= 0) with the special values spread over them: zeros, +-denormals, values near FLT_MAX, and a stretch where
    g is zero under a non-zero m"""
    rng = np.random.RandomState(seed)
    p = rng.randn(n).astype(F32)
    g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(F32)
    m = (rng.randn(n) * 0.1).astype(F32)
    v = (rng.rand(n) * 10.0 ** rng.uniform(-12, 0, n)).astype(F32)
    special = np.concatenate([DENORM, [0.0, -0.0, FLT_MAX, -FLT_MAX, FLT_MAX / 2, 1e38]]).astype(F32)
    for k, arr in enumerate((p, g, m, v)):
        idx = rng.permutation(n)[:min(n, 2 * len(special))]
        vals = special[(np.arange(len(idx)) + 3 * k) % len(special)]
        arr[idx] = np.abs(vals) if arr is v else vals
    zero_g = rng.rand(n) < 0.1
    g[zero_g] = 0.0
    m[zero_g & (m == 0)] = F32(0.25)
    if n >= 16:                      # results that ARE denormal (a kernel that flushed them would give zeros): g = 0 under denormal m, v, p
        k = len(DENORM)
        g[:k] = 0.0; m[:k] = DENORM; v[:k] = np.abs(DENORM); p[:k] = DENORM[::-1]
    return p, g, m, v


def _same(name, got, want):
    """the same bits; where the rule gives a NaN (inf / inf next to FLT_MAX) a NaN, whose sign and payload IEEE 754 leaves open"""
    a, b = _bits(got), _bits(want)
    bad = np.flatnonzero((a != b) & ~(np.isnan(got) & np.isnan(want)))
    assert bad.size == 0, (name, int(bad[0]), float(got[bad[0]]), float(want[bad[0]]), int(bad.size))


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_adam_equals_the_restatement_bit_for_bit(ctx, offset, t, wd):
    from densecap_amd import ops
    for n in SIZES:
        p, g, m, v = _inputs(n, seed=n + 7 * t + offset)
        opts = dict(OPTS, weight_decay=wd)
        wp, wm, wv = R.adam_step32(p, g, m, v, t, **opts)
        gp, gm, gv, g_after, intact = ops.adam(ctx, p, g, m, v, t, offset=offset, **opts)
        _same("p n=%d" % n, gp, wp); _same("m n=%d" % n, gm, wm); _same("v n=%d" % n, gv, wv)
        assert np.array_equal(_bits(g_after), _bits(g)), "g changed (n = %d)" % n
        assert intact, "guard floats changed (n = %d)" % n


def test_buffers_at_different_offsets_take_the_scalar_path(ctx):
    """p, g, m, v each at another offset from 16-byte alignment: no common aligned element, the same bits."""
    import ctypes as C
    from densecap_amd import ops
    n, t = 1027, 3
    p, g, m, v = _inputs(n, seed=5)
    opts = dict(OPTS, weight_decay=1e-2)
    want = R.adam_step32(p, g, m, v, t, **opts)
    pad = F32(3.5)
    bufs = []
    for off, a in zip((0, 1, 2, 3), (p, g, m, v)):
        host = np.full(off + 4 + n + 4, pad, F32)
        host[off + 4:off + 4 + n] = a
        bufs.append((ctx.to_device(host), off + 4))
    at = lambda b: C.c_void_p(b[0].ptr.value + 4 * b[1])
    o = ops.train_opts(**opts)
    ops.check(ctx.h, ctx.lib.dc_op_adam(ctx.h, at(bufs[0]), at(bufs[1]), at(bufs[2]), at(bufs[3]), n, t, C.byref(o)), "dc_op_adam")
    outs = [b[0].numpy() for b in bufs]
    for k, (name, j) in enumerate((("p", 0), ("m", 2), ("v", 3))):
        lo = bufs[j][1]
        _same(name, outs[j][lo:lo + n], want[k])
    for (b, lo), h in zip(bufs, outs):
        assert (h[:lo] == pad).all() and (h[lo + n:] == pad).all()
    assert np.array_equal(_bits(outs[1][bufs[1][1]:bufs[1][1] + n]), _bits(g))


def test_multi_segment_launch_equals_per_segment_calls(ctx):
    from densecap_amd import ops
    sizes = [(1, 4, 7, 64, 4099)[i % 5] for i in range(21)]
    segs = [_inputs(n, seed=100 + i) for i, n in enumerate(sizes)]
    opts = dict(OPTS, weight_decay=1e-2)
    t = 4
    one = [ops.adam(ctx, *s, t, **opts)[:3] for s in segs]
    for grid in (0, 1, 3):                                   # the result does not depend on the grid
        many = ops.adam_multi(ctx, segs, t, grid=grid, **opts)
        for i, (a, b) in enumerate(zip(many, one)):
            for name, x, y in zip("pmv", a, b):
                _same("segment %d %s grid %d" % (i, name, grid), x, y)
    for i, (a, s) in enumerate(zip(one, segs)):
        for name, x, y in zip("pmv", a, R.adam_step32(*s, t, **opts)):
            _same("segment %d %s rule" % (i, name), x, y)


def test_two_identical_calls_give_identical_bits(ctx):
    from densecap_amd import ops
    p, g, m, v = _inputs(65541, seed=9)
    a = ops.adam(ctx, p, g, m, v, 2, weight_decay=1e-2, **OPTS)
    b = ops.adam(ctx, p, g, m, v, 2, weight_decay=1e-2, **OPTS)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("bad", [dict(learning_rate=-1e-5), dict(learning_rate=float("nan")), dict(learning_rate=float("inf")),
                                 dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(epsilon=0.0),
                                 dict(epsilon=-1e-8), dict(epsilon=float("nan")), dict(weight_decay=-1e-6),
                                 dict(weight_decay=float("inf"))])
def test_bad_options_are_refused_and_nothing_changes(ctx, bad):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    p, g, m, v = _inputs(257, seed=1)
    with pytest.raises(DenseCapError, match=r"\(-1\)"):
        ops.adam(ctx, p, g, m, v, 1, **dict(dict(OPTS, weight_decay=0.0), **bad))
    with pytest.raises(DenseCapError, match=r"\(-1\)"):
        ops.adam(ctx, p, g, m, v, 0, **OPTS)                 # t counts from 1
