"""Clipping by the global gradient norm (docs/SEMANTICS.md, "Gradient clipping") against tests/clip_rules.py: the norm kernels on
exact seams (ones: sumsq is the element count; NaN guards on both sides), on random data within the bar the reduction's structure
gives, over 21 segments at three grids; the scale within 1 ulp of the rule's and the update bit for bit the restatement's WITH
the device's scale; then dc_train_step end to end on tests/test_gpu_train_step.py's tiny setup, in CNN mode 2, and the refusals."""
import math

import numpy as np
import pytest

from tests import clip_rules as K
from tests import optim_rules as R
from tests.test_gpu_adam import OPTS, SIZES, _inputs, _same
from tests.test_gpu_train_cnn import CNN, _grads_cnn
from tests.test_gpu_train_step import DECAY, FORCED, LOSS, _assert_weights, _bits, _model, _np, _step, setup  # noqa: F401 (setup: a fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
SEAM_SIZES = SIZES + (4095, 4096, 4097, 2 * 4096 + 5)
SEG_SIZES = [(1, 4, 7, 64, 4099)[i % 5] for i in range(21)]       # test_multi_segment_launch_equals_per_segment_calls'


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import Context
    c = Context(0)
    yield c
    c.close()


# ---- the norm kernels alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_ones_sum_to_the_element_count_at_every_seam(ctx, offset):
    """g = 1.0f: an over-read meets a NaN guard, a missed or doubled element changes the integer"""
    from densecap_amd import ops
    for n in SEAM_SIZES:
        sumsq, norm, scale = ops.grad_norm(ctx, np.ones(n, F32), float("inf"), offset=offset)
        assert sumsq == float(n), (n, offset, sumsq)
        assert norm == math.sqrt(float(n)) and scale == F32(1.0)


@pytest.mark.parametrize("offset", [0, 3])
def test_random_data_is_within_the_bar_and_repeats(ctx, offset):
    from densecap_amd import ops
    for n in SEAM_SIZES:
        g = K.trial_gradient(n, seed=n + offset)
        want = K.sumsq_ref([g])
        a = ops.grad_norm(ctx, g, 1.0, offset=offset)
        b = ops.grad_norm(ctx, g, 1.0, offset=offset)
        print("n = %d offset %d: sumsq off by %.2f units of 2^-53 (bar %d)" % (n, offset, abs(a[0] - want) / max(want, 1e-300) / K.U53,
                                                                               K.chain_length([n]) + 1))
        assert K.within_bar(a[0], want, [n]), (n, a[0], want)
        assert _bits(np.float64(a[0])) == _bits(np.float64(b[0])) and _bits(np.float64(a[1])) == _bits(np.float64(b[1]))
        assert _bits(F32(a[2])) == _bits(F32(b[2]))
        assert K.ulps32(a[2], K.scale_rule(want, 1.0)[0]) <= 1


def test_op_refusals(ctx):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    for bad in (-1.0, float("nan")):
        with pytest.raises(DenseCapError, match=r"\(-1\)"):
            ops.grad_norm(ctx, np.ones(5, F32), bad)
    with pytest.raises(DenseCapError, match=r"\(-1\)"):
        ops.grad_norm(ctx, np.zeros(0, F32), 1.0)                                      # n < 1
    assert ops.grad_norm(ctx, np.full(7, 2.0, F32), 0.0) == (28.0, math.sqrt(28.0), F32(1.0))     # 0: the norm alone


# ---- twenty-one segments -------------------------------------------------------------------------------------------------------------
def test_twenty_one_segments_at_three_grids(ctx):
    from densecap_amd import ops
    segs = [_inputs(n, seed=100 + i) for i, n in enumerate(SEG_SIZES)]
    ones = [(p, np.ones_like(g), m, v) for p, g, m, v in segs]
    opts = dict(OPTS, weight_decay=1e-2)
    runs = []
    for grid in (0, 1, 3):
        _, sumsq, _ = ops.adam_multi_clip(ctx, ones, 4, float("inf"), grid=grid, **opts)
        assert sumsq == float(sum(SEG_SIZES)), grid
        finite = [(p, K.trial_gradient(len(g), seed=7 + i), m, v) for i, (p, g, m, v) in enumerate(segs)]
        runs.append(ops.adam_multi_clip(ctx, finite, 4, 3.0, grid=grid, **opts))
    want = K.sumsq_ref([s[1] for s in finite])
    assert K.within_bar(runs[0][1], want, SEG_SIZES) and runs[0][2] < F32(1.0)
    for many, sumsq, scale in runs[1:]:
        assert _bits(np.float64(sumsq)) == _bits(np.float64(runs[0][1])) and _bits(F32(scale)) == _bits(F32(runs[0][2]))
        for i, (a, b) in enumerate(zip(many, runs[0][0])):
            for name, x, y in zip("pmv", a, b):
                assert np.array_equal(_bits(x), _bits(y)), (i, name)


# ---- scale and update through the hook -------------------------------------------------------------------------------------------------
def _hook_case(ctx, segs, t, wd, max_norm):
    """-> (device results, sumsq, scale, the rule's scale) for one call of the hook"""
    from densecap_amd import ops
    opts = dict(OPTS, weight_decay=wd)
    got, sumsq, scale = ops.adam_multi_clip(ctx, segs, t, max_norm, **opts)
    return got, sumsq, scale, opts


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("case", ["below", "above", "inf"])
def test_scale_and_update_are_the_rule_with_the_devices_scale(ctx, case, t, wd):
    from densecap_amd import ops
    segs = [(p, K.trial_gradient(len(g), seed=31 + i), m, v)
            for i, (p, g, m, v) in enumerate(_inputs(n, seed=40 + i) for i, n in enumerate((5, 257, 4097, 2 * 4096 + 5)))]
    sizes = [len(s[0]) for s in segs]
    want_sumsq = K.sumsq_ref([s[1] for s in segs])
    norm = math.sqrt(want_sumsq)
    max_norm = {"below": 2.0 * norm, "above": 0.37 * norm, "inf": float("inf")}[case]
    got, sumsq, scale, opts = _hook_case(ctx, segs, t, wd, max_norm)
    assert K.within_bar(sumsq, want_sumsq, sizes)
    rule = K.scale_rule(want_sumsq, max_norm)[0]
    assert K.ulps32(scale, rule) <= 1, (scale, rule)
    if case == "above":
        assert F32(0.36) < scale < F32(0.38)
    else:
        assert _bits(F32(scale)) == _bits(F32(1.0))
        plain = ops.adam_multi(ctx, segs, t, **opts)
        for i, (a, b) in enumerate(zip(got, plain)):
            for name, x, y in zip("pmv", a, b):
                assert np.array_equal(_bits(x), _bits(y)), (i, name)
    for i, ((p, g, m, v), res) in enumerate(zip(segs, got)):
        for name, x, y in zip("pmv", res, K.adam_step32_scaled(p, g, m, v, t, scale, **opts)):
            _same("segment %d %s" % (i, name), x, y)


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_gradient_is_reported_and_not_clipped(ctx, poison, t, wd):
    segs = [(p, K.trial_gradient(len(g), seed=51 + i), m, v)
            for i, (p, g, m, v) in enumerate(_inputs(n, seed=60 + i) for i, n in enumerate((64, 4099)))]
    segs[1][1][4098] = poison
    got, sumsq, scale, opts = _hook_case(ctx, segs, t, wd, 0.01)
    assert (math.isnan(sumsq) if np.isnan(poison) else sumsq == float("inf")), sumsq
    assert _bits(F32(scale)) == _bits(F32(1.0))
    for i, ((p, g, m, v), res) in enumerate(zip(segs, got)):
        for name, x, y in zip("pmv", res, R.adam_step32(p, g, m, v, t, **opts)):       # the unclipped rule's bits
            _same("segment %d %s" % (i, name), x, y)
    assert not np.isfinite(got[1][1][4098])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _scaled_rule_step(Wk, grads, t, scale, **opts):
    from densecap_amd.ops import WEIGHT_KEYS
    out = {}
    for k in WEIGHT_KEYS:
        p = _np(Wk[k])
        z = np.zeros(p.size, F32)
        out[k] = K.adam_step32_scaled(p.reshape(-1), _np(grads[k]).reshape(-1), z, z, t, scale, **opts)[0].reshape(p.shape)
    return out


def _device_sizes(grads, cnn=False):
    """the segment sizes of the step's table(s): 17 for the 21 tensors (the two RPN heads and the five recognition heads are
    fused), then the CNN's 18"""
    n = lambda *ks: sum(_np(grads[k]).size for k in ks)
    out = [n("rpn_conv_w"), n("rpn_conv_b"), n("rpn_box_w", "rpn_score_w"), n("rpn_box_b", "rpn_score_b"), n("fc6_w"), n("fc6_b"),
           n("fc7_w"), n("fc7_b"), n("obj_w", "boxreg_w"), n("obj_b", "boxreg_b"), n("lm_enc_w"), n("lm_enc_b"), n("lm_emb"),
           n("lstm_w"), n("lstm_b"), n("lm_out_w"), n("lm_out_b")]
    if cnn:
        out += [n("conv_%s%d" % (wb, i)) for i in CNN for wb in "wb"]
    return out


def _norm_bar(sizes):
    """relative, of the device's norm against sqrt(fsum) in double: half the sumsq bar through the root, the root's own rounding
    on both sides and the second-order term"""
    return ((K.chain_length(sizes) + 1) / 2.0 + 3.0) * K.U53


def test_off_is_the_step_of_a_context_that_never_heard_of_it(setup):
    W, img, gt, lab, _g, want = setup
    got = []
    for tell in (False, True):
        m = _model(W)
        try:
            m.train_begin(weight_decay=1e-6)
            if tell:
                m.train_set_grad_clip(0)
            res = _step(m, img, gt, lab)
            assert "grad_norm" not in res and "grad_scale" not in res
            got.append((res, m.get_weights()))
        finally:
            m.ctx.close()
    assert sorted(got[0][0]) == sorted(got[1][0])
    _assert_weights(got[1][1], got[0][1], "clip 0")
    _assert_weights(got[1][1], want, "clip 0 against the rule")


def test_on_clips_all_21_tensors_with_the_reported_scale(setup):
    from densecap_amd.ops import WEIGHT_KEYS
    W, img, gt, lab, grads, _want = setup
    twin = _model(W)
    try:
        twin.train_begin(weight_decay=1e-6)
        twin.train_set_grad_clip(float("inf"))                                       # log only
        log = _step(twin, img, gt, lab)
        logged = twin.get_weights()
    finally:
        twin.ctx.close()
    gs = [_np(grads[k]).reshape(-1) for k in WEIGHT_KEYS]
    sizes = _device_sizes(grads)
    assert sum(sizes) == sum(len(g) for g in gs)
    ss = K.sumsq_ref(gs)
    ref = math.sqrt(ss)
    assert log["grad_scale"] == 1.0 and abs(log["grad_norm"] - ref) <= _norm_bar(sizes) * ref, (log["grad_norm"], ref)
    _assert_weights(logged, setup[5], "log only is the unclipped step")
    m = _model(W)
    try:
        m.train_begin(weight_decay=1e-6)
        m.train_set_grad_clip(0.5 * log["grad_norm"])
        res = _step(m, img, gt, lab)
        got = m.get_weights()
    finally:
        m.ctx.close()
    print("grad_norm %.17g (fsum's %.17g), scale %r" % (res["grad_norm"], ref, res["grad_scale"]))
    assert _bits(np.float64(res["grad_norm"])) == _bits(np.float64(log["grad_norm"]))
    assert abs(res["grad_norm"] - ref) <= _norm_bar(sizes) * ref
    scale = F32(res["grad_scale"])
    assert K.ulps32(scale, K.scale_rule(ss, 0.5 * log["grad_norm"])[0]) <= 1 and F32(0.49) < scale < F32(0.51)
    for k in ("total_loss", "num_pos", "num_neg"):
        assert res[k] == grads[k], k
    _assert_weights(got, _scaled_rule_step(W, grads, 1, scale, **R.DEFAULTS), "clipped step")


def test_cnn_mode_2_has_one_norm_over_both_tables(setup):
    from densecap_amd.ops import WEIGHT_KEYS
    W, img, gt, lab, _g, _w = setup
    grads = _grads_cnn(W, img, gt, lab)
    cnn_keys = ["conv_%s%d" % (wb, i) for i in CNN for wb in "wb"]
    gs = [_np(grads[k]).reshape(-1) for k in list(WEIGHT_KEYS) + cnn_keys]
    sizes = _device_sizes(grads, cnn=True)
    assert sum(sizes) == sum(len(g) for g in gs)
    ss = K.sumsq_ref(gs)
    ref = math.sqrt(ss)
    only21 = math.sqrt(K.sumsq_ref(gs[:21]))
    assert ref > only21 * (1 + 1e-9)                                                   # the CNN's share is visible in the norm
    m = _model(W)
    try:
        m.train_begin(weight_decay=1e-6)
        m.train_set_cnn(2)
        m.train_set_grad_clip(0.25 * ref)
        res = _step(m, img, gt, lab)
        got = m.get_weights()
    finally:
        m.ctx.close()
    assert abs(res["grad_norm"] - ref) <= _norm_bar(sizes) * ref, (res["grad_norm"], ref, only21)
    scale = F32(res["grad_scale"])
    assert K.ulps32(scale, K.scale_rule(ss, 0.25 * ref)[0]) <= 1
    _assert_weights(got, _scaled_rule_step(W, grads, 1, scale, **R.DEFAULTS), "the 21 tensors")
    for i in CNN:
        for key in ("conv_w", "conv_b"):
            p = _np(W[key][i])
            z = np.zeros(p.size, F32)
            want = K.adam_step32_scaled(p.reshape(-1), _np(grads["%s%d" % (key, i)]).reshape(-1), z, z, 1, scale, **R.DEFAULTS)[0]
            assert np.array_equal(_bits(_np(got[key][i]).reshape(-1)), _bits(want)), (key, i)


def test_mode_1_leaves_the_cnn_out_of_the_norm(setup):
    from densecap_amd.ops import WEIGHT_KEYS
    W, img, gt, lab, grads, _w = setup
    m = _model(W)
    try:
        m.train_begin(weight_decay=1e-6)
        m.train_set_cnn(1)
        m.train_set_grad_clip(float("inf"))
        res = _step(m, img, gt, lab)
    finally:
        m.ctx.close()
    gs = [_np(grads[k]).reshape(-1) for k in WEIGHT_KEYS]
    ref = math.sqrt(K.sumsq_ref(gs))
    assert abs(res["grad_norm"] - ref) <= _norm_bar(_device_sizes(grads)) * ref


def test_refusals_and_the_kept_record(setup):
    import ctypes as C
    from densecap_amd._lib import DenseCapError
    W, img, gt, lab, _g, _w = setup
    m = _model(W)

    def record():
        norm, scale = C.c_double(0.0), C.c_float(0.0)
        return m.lib.dc_train_grad_norm(m.ctx.h, C.byref(norm), C.byref(scale)), norm.value, scale.value

    try:
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_set_grad_clip(1.0)                                                # before begin
        assert record()[0] == -3
        m.train_begin(weight_decay=1e-6)
        for bad in (-1.0, float("nan")):
            with pytest.raises(DenseCapError, match=r"\(-1\)"):
                m.train_set_grad_clip(bad)
        assert record()[0] == -3                                                      # no clipped step yet
        _step(m, img, gt, lab)                                                        # an unclipped step leaves no record
        assert record()[0] == -3
        m.train_set_grad_clip(1e-3)
        res = _step(m, img, gt, lab)
        rc, norm, scale = record()
        assert rc == 0 and norm == res["grad_norm"] > 1e-3 and scale == res["grad_scale"] < 1.0
        bad_gt = gt.copy(); bad_gt[1, 2] = 0.0
        with pytest.raises(DenseCapError):
            m.train_step(img, bad_gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
        assert record() == (rc, norm, scale)                                          # a refused step keeps the record
        m.train_end()
        assert record()[0] == -3
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_set_grad_clip(1.0)                                                # after end
        m.train_begin()
        assert record()[0] == -3                                                      # begin starts without a record, clipping off
        assert "grad_norm" not in _step(m, img, gt, lab)
    finally:
        m.ctx.close()
