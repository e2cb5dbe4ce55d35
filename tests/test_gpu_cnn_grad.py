"""dc_op_cnn_grad -- conv_net2's forward with kept activations and the backward through conv5_3 .. conv3_1 -- against
tests/cnn_grad_rules.py, teacher-forced on the device's own dumped activations and masked gradients.

Per shape one device call is checked five ways: the kept activations are the per-op forward's bits; every masked gradient is the
rules' selection, bit for bit, of the per-op dx of the layer behind it; every layer's dw, db and dx sit inside
tests/test_gpu_conv3x3_grad.check's bars against float64; the eighteen gradients and x sit inside the per-row bars that the
float32 evaluation of the same chain sets; a second call gives the same bits."""
import numpy as np
import pytest

from tests import cnn_grad_rules as CR
from tests import grad_bars as GB
from tests import rpn_grad_rules as R
from tests.test_gpu_conv3x3_grad import SENTINEL, _bits, check, refs, run

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID, STATE, UNSUPPORTED = -1, -3, -5


@pytest.fixture(scope="module")
def model():
    from densecap_amd import DenseCapModel
    m = DenseCapModel(CR.model_weights(), device=0)
    yield m
    m.ctx.close()


@pytest.fixture(scope="module")
def params():
    return CR.conv_params(CR.model_weights())


_calls = {}


def device_call(model, shape):
    """(x4, dfeat, the dumped result) of one shape: one device call per module, shared by the tests and left unchanged."""
    from densecap_amd import ops
    if shape not in _calls:
        x4, dfeat = CR.make_chain_case(*shape, seed=shape[0] * 10 + shape[1])
        _calls[shape] = (x4, dfeat, ops.cnn_grad(model.ctx, x4, dfeat, want_x=True, dump=True))
    return _calls[shape]


def kept(d):
    """(acts, prepool) as chain takes them, from a dumped result."""
    acts = {i: d["act%d" % i] for i in CR.CONVS}
    acts[13] = d["feat"]
    return acts, {i: d["prepool%d" % i] for i in CR.POOL_AFTER}


SHAPES = pytest.mark.parametrize("shape", CR.CHAIN_SHAPES, ids=["%dx%d" % s for s in CR.CHAIN_SHAPES])


@SHAPES
def test_kept_activations_are_the_per_op_forward(model, params, shape):
    from densecap_amd import ops
    w, b = params
    x4, _, d = device_call(model, shape)
    hw, (fh, fw) = CR.sizes(*shape)
    assert np.array_equal(_bits(d["act4"]), _bits(x4))
    for i in CR.CONVS:
        assert d["act%d" % i].shape == (CR.CHANNELS[i][0],) + hw[i]
        out = ops.conv3x3(model.ctx, d["act%d" % i][None], w[i], b[i], relu=True)
        if i in CR.POOL_AFTER:
            assert np.array_equal(_bits(out[0]), _bits(d["prepool%d" % i])), i
            out = ops.maxpool2x2_ceil(model.ctx, out)
        nxt = d["feat"] if i == 12 else d["act%d" % (i + 1)]
        assert np.array_equal(_bits(out[0]), _bits(nxt)), i
    assert d["feat"].shape == (512, fh, fw)


@SHAPES
def test_masks_pool_gradients_and_layers(model, params, shape):
    """From conv5_3 down: dy_i is the rules' selection of the gradient that reaches the layer -- dfeat, or the per-op dx of layer
    i + 1 on the dumped x and dy --, bit for bit; dw_i, db_i and that dx against float64 on the dumped operands."""
    from densecap_amd import ops
    w, _ = params
    _, dfeat, d = device_call(model, shape)
    acts, prepool = kept(d)
    g = dfeat
    for i in reversed(CR.CONVS):
        want = CR.pool_relu_grad(prepool[i], g) if i in CR.POOL_AFTER else CR.relu_grad(acts[i + 1], g)
        assert np.array_equal(_bits(d["dy%d" % i]), _bits(want)), i
        g = d["x"] if i == 4 else ops.conv3x3_grad(model.ctx, None, w[i], d["dy%d" % i], want=("dx",))["dx"]
        dev = {"dw": d["conv_w%d" % i], "db": d["conv_b%d" % i], "dx": g}
        check("%dx%d conv %d" % (shape + (i,)), dev, *refs(acts[i], w[i], d["dy%d" % i]))
    layer4 = ops.conv3x3_grad(model.ctx, acts[4], w[4], d["dy4"])
    assert all(np.array_equal(_bits(layer4[k]), _bits(v)) for k, v in (("dw", d["conv_w4"]), ("db", d["conv_b4"]), ("dx", d["x"])))


@SHAPES
def test_whole_chain_within_the_float32_chains_bars(model, params, shape):
    w, _ = params
    _, dfeat, d = device_call(model, shape)
    acts, prepool = kept(d)
    r64, r32 = CR.chain(acts, prepool, w, dfeat, "float64"), CR.chain(acts, prepool, w, dfeat, "float32")
    figs, bad = [], []
    rows = lambda k, a: a.reshape(a.shape[0], -1) if k != "x" else GB.rows_of("feat", a)
    for k in [n for i in CR.CONVS for n in ("conv_w%d" % i, "conv_b%d" % i)] + ["x"]:
        assert np.isfinite(d[k]).all(), k
        scale = float(np.abs(r64[k]).max())
        err = float(np.abs(d[k].astype(np.float64) - r64[k]).max())
        figs.append("%s %.1e" % (k, err / scale))
        if err > R.REL * scale:
            bad.append((k, "max-norm", err / scale))
        if not k.startswith("conv_b"):              # (bias vectors stay on the max-norm: tests/grad_bars.py says why)
            bar = GB.bar_from_float32(k, rows(k, r32[k]), rows(k, r64[k]))
            worst, over = GB.check_rows(k, rows(k, d[k]), rows(k, r64[k]), bar)
            figs.append("rows %.1e (bar %.1e)" % (worst, bar))
            if over:
                bad.append((k, "rows, bar %.3e" % bar, over))
    print("cnn_grad chain %dx%d: " % shape + ", ".join(figs))
    assert not bad, bad


@SHAPES
def test_two_calls_give_the_same_bits(model, shape):
    from densecap_amd import ops
    x4, dfeat, d = device_call(model, shape)
    again = ops.cnn_grad(model.ctx, x4, dfeat, want_x=True)
    assert sorted(again) == sorted(ops.CNN_GRAD_KEYS + ("x",))
    assert all(np.array_equal(_bits(again[k]), _bits(d[k])) for k in again)
    no_x = ops.cnn_grad(model.ctx, x4, dfeat, want_x=False)
    assert "x" not in no_x and all(np.array_equal(_bits(no_x[k]), _bits(d[k])) for k in no_x)
    fwd_ms, bwd_ms = ops.cnn_grad_ms(model.ctx)
    assert fwd_ms > 0 and bwd_ms > 0


def test_math_mode_does_not_reach_the_gradients(model):
    from densecap_amd import ops
    x4, dfeat, d = device_call(model, (5, 7))
    model.ctx.set_math_mode(1)
    try:
        got = ops.cnn_grad(model.ctx, x4, dfeat)
    finally:
        model.ctx.set_math_mode(0)
    assert all(np.array_equal(_bits(got[k]), _bits(d[k])) for k in got)


def test_single_layer_above_every_slice_threshold(model):
    """150 x 180 = 27000 pixels, conv3's map at 720 x 600, with 32 -> 32 channels: the weight gradient's slice count sits at its
    cap of 64 (two workgroups per CU over three tiles ask for more, and every slice still sums more than 64 pixels)."""
    h, w, Cin, Cout = 150, 180, 32, 32
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed=27)
    rc, dev = run(model.ctx, x, wt, dy)
    assert rc == 0
    check("150x180 32->32", dev, *refs(x, wt, dy))


def _call(ctx, x4, h4, w4, dfeat, bufs, want_x=True, null=None):
    from densecap_amd import _lib
    cg = _lib.DcCnnGrads()
    for j, i in enumerate(CR.CONVS):
        cg.conv_w[j] = bufs["conv_w%d" % i].ptr.value
        cg.conv_b[j] = bufs["conv_b%d" % i].ptr.value
    if null is not None:
        getattr(cg, null[0])[null[1]] = None
    cg.x = bufs["x"].ptr.value if want_x else None
    import ctypes as C
    return ctx.lib.dc_op_cnn_grad(ctx.h, x4.ptr if x4 is not None else None, h4, w4, dfeat.ptr if dfeat is not None else None,
                                  C.byref(cg), None)


def test_refusals_come_before_any_launch(model):
    """65537 pixels (1 x 65537) is refused in dc_op_conv3x3_grad's words; so are a null buffer and a non-positive size.  The
    output buffers, sized for the refused shape, keep their sentinels."""
    ctx = model.ctx
    h4, w4 = 1, 65537
    _, (fh, fw) = CR.sizes(h4, w4)
    shapes = {"x": (h4, w4, 128)}
    for i in CR.CONVS:
        shapes["conv_w%d" % i] = CR.CHANNELS[i][::-1] + (3, 3)
        shapes["conv_b%d" % i] = (CR.CHANNELS[i][1],)
    host = {k: np.full(s, SENTINEL, F32) for k, s in shapes.items()}
    bufs = {k: ctx.to_device(a) for k, a in host.items()}
    x4 = ctx.to_device(np.zeros((h4, w4, 128), F32)); dfeat = ctx.to_device(np.zeros((fh, fw, 512), F32))
    assert _call(ctx, x4, h4, w4, dfeat, bufs) == UNSUPPORTED
    msg = ctx.lib.dc_last_error(ctx.h).decode()
    assert msg.startswith("dc_op_cnn_grad: a map of 1 x 65537 pixels, more than the 65536 the kernels take"), msg
    assert _call(ctx, x4, w4, h4, dfeat, bufs, want_x=False) == UNSUPPORTED
    for args in ((0, 8), (8, 0), (-1, 8)):
        assert _call(ctx, x4, args[0], args[1], dfeat, bufs) == INVALID, args
    assert _call(ctx, None, 8, 8, dfeat, bufs) == INVALID
    assert _call(ctx, x4, 8, 8, None, bufs) == INVALID
    assert _call(ctx, x4, 8, 8, dfeat, bufs, null=("conv_w", 3)) == INVALID
    assert _call(ctx, x4, 8, 8, dfeat, bufs, null=("conv_b", 8)) == INVALID
    assert ctx.lib.dc_op_cnn_grad(ctx.h, x4.ptr, 8, 8, dfeat.ptr, None, None) == INVALID
    for k, b in bufs.items():
        assert np.array_equal(_bits(b.numpy()), _bits(host[k])), k
    from densecap_amd.ops import Context
    bare = Context(0)
    try:
        assert _call(bare, x4, 8, 8, dfeat, bufs) == STATE                # no weights loaded
    finally:
        bare.close()
