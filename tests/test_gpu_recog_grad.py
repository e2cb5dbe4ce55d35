"""dc_op_recog_grad (docs/SEMANTICS.md, "Recognition-net gradients") and its kernels alone (the hooks of
include/densecap_debug_recog.h) against the float64 autograd restatement of tests/recog_grad_rules.py.

Largest observed max|dev - ref64| / max|ref64| per tensor and case (MI355X; the bar is 1e-4), and the worst per-row ratio of the
2-D tensors beside the bar it was held to (tests/grad_bars.py): see DESIGN.md §17."""
import ctypes as C

import numpy as np
import pytest

from tests import grad_bars as GB
from tests import recog_grad_rules as R

pytestmark = pytest.mark.gpu

REL = 1e-4                     # tests/parity.py's continuous-stage bar
F32 = np.float32
IMG, MAP = (96, 128), (6, 8)   # image (H, W); its feature map (h, w)
# case -> (weights, n, num_pos, masked rows, rows on SmoothL1's linear branch, a gradient g of the positive codes?)
CASES = {"minimal_1_0": ("minimal", 1, 0, (), (), False), "minimal_1_1": ("minimal", 1, 1, (), (), True),
         "minimal_5_2": ("minimal", 5, 2, (0,), (1,), True), "minimal_5_2_no_g": ("minimal", 5, 2, (0,), (1,), False),
         "minimal_70": ("minimal", 70, 33, (), (2,), True), "minimal_256": ("minimal", 256, 128, (5,), (7,), True),
         "odd32_5_2": ("odd32", 5, 2, (0,), (1,), True), "odd32_70": ("odd32", 70, 20, (), (), False),
         "default_3_2": ("default", 3, 2, (), (1,), True)}
_models, _runs = {}, {}


def _weights(name):
    from densecap_amd.weights import make_synthetic_weights
    from tests.test_gpu_dims import set_weights
    return make_synthetic_weights(seed=21, vocab_size=200, seq_length=15) if name == "default" else set_weights(name)


def _model(name):
    """One model per weight set for the whole module."""
    if name not in _models:
        from densecap_amd import DenseCapModel
        W = _weights(name)
        _models[name] = (DenseCapModel(W, device=0), W)
    return _models[name]


def _run(case):
    """(model, W, inputs, device result, float64 reference) of a case, computed once."""
    if case not in _runs:
        from densecap_amd import ops
        name, n, np_, masked, far, with_g = CASES[case]
        m, W = _model(name)
        rng = np.random.default_rng(300 + n * 8 + np_)
        feat, boxes, targets = R.draw_case(W, rng, n, np_, IMG[0], IMG[1], MAP[0], MAP[1], masked_rows=masked, far_rows=far, outside=0.2)
        g = (rng.standard_normal((np_, m.fc_dim)) * 1e-3).astype(F32) if with_g and np_ else None
        dev = ops.recog_grad(m.ctx, feat, boxes, np_, targets, IMG[0], IMG[1], dcodes=g)
        _runs[case] = (m, W, (feat, boxes, targets, g), dev, R.recog_grad(W, feat, boxes, np_, targets, g, IMG[0], IMG[1]))
    return _runs[case]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m, _ in _models.values():
        m.ctx.close()
    _models.clear(); _runs.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ratio(dev, ref):
    if ref.size == 0:
        return 0.0
    scale = np.abs(ref).max()
    return float(np.abs(dev - ref).max() / scale) if scale else float(np.abs(dev).max())


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    return _model("minimal")[0].ctx


@pytest.mark.parametrize("n,np_", [(1, 0), (1, 1), (5, 2), (70, 33), (1024, 512)])
def test_end_crit_grad_alone(ctx, n, np_):
    from densecap_amd import ops
    rng = np.random.default_rng(n + np_)
    obj = (rng.standard_normal(n) * 4).astype(F32)
    anchors = np.stack([rng.uniform(20, 100, n), rng.uniform(20, 80, n), rng.uniform(10, 60, n), rng.uniform(10, 60, n)], 1).astype(F32)
    targets = (anchors[:np_] * (1 + 0.2 * rng.uniform(-1, 1, (np_, 4)))).astype(F32)
    trans = (rng.standard_normal((n, 4)) * 0.8).astype(F32)
    if np_ >= 2:
        targets[0, 1] = anchors[0, 1] - 11.0 * anchors[0, 3]                      # masked
        trans[1] = [3.0, -3.0, 0.2, -0.1]                                         # both SmoothL1 branches
    ref = R.end_crit_grad(obj, trans, anchors, targets, np_, 0.1, 0.25)
    dev = ops.end_crit_grad(ctx, obj, trans, anchors, targets, np_, 0.1, 0.25)
    assert dev[3] == ref[3] == (1 if np_ >= 2 else 0)
    for what, d, r in zip(("dobj", "dtrans", "danchor"), dev, ref):
        assert d.shape == r.shape and _ratio(d, r) <= REL, (what, _ratio(d, r))
    if np_ >= 2:
        assert not dev[1][0].any() and not dev[2][0].any()                        # the masked row gives nothing


@pytest.mark.parametrize("n,np_,D,with_g", [(1, 0, 256, False), (1, 1, 256, True), (5, 2, 768, True), (70, 33, 256, False), (256, 128, 4096, True)])
def test_heads_bwd_alone(ctx, n, np_, D, with_g):
    from densecap_amd import ops
    rng = np.random.default_rng(n * 3 + D)
    codes, w5 = rng.standard_normal((n, D)).astype(F32), rng.standard_normal((5, D)).astype(F32)
    dobj, dtrans = rng.standard_normal(n).astype(F32), rng.standard_normal((np_, 4)).astype(F32)
    g = rng.standard_normal((np_, D)).astype(F32) if with_g else None
    dc, dw, db = ops.heads_bwd(ctx, codes, w5, dobj, dtrans, g)
    c64, w64 = codes.astype(np.float64), w5.astype(np.float64)
    dh = np.zeros((n, 5))
    dh[:, 0] = dobj
    dh[:np_, 1:] = dtrans
    rc = dh @ w64
    if with_g:
        rc[:np_] += g
    for what, d, r in (("dcodes", dc, rc), ("dw5", dw, dh.T @ c64), ("db5", db, dh.sum(0))):
        assert d.shape == r.shape and _ratio(d, r) <= REL, (what, _ratio(d, r))


@pytest.mark.parametrize("N,Cc,HW", [(1, 64, 1), (3, 128, 49), (5, 512, 49), (2, 64, 64)])
def test_permute_fc6_back_inverts_the_load_time_permutation(ctx, N, Cc, HW):
    from densecap_amd import ops
    x = np.random.default_rng(N).standard_normal((N, Cc * HW)).astype(F32)                  # k = c * HW + p
    perm = np.ascontiguousarray(x.reshape(N, Cc, HW).transpose(0, 2, 1)).reshape(N, -1)     # k' = p * C + c (permute_fc6)
    assert np.array_equal(_bits(ops.permute_fc6_back(ctx, perm, Cc, HW)), _bits(x))


# ---- the whole call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_the_float64_restatement(case):
    """All ten tensors: max|dev - ref64| <= 1e-4 max|ref64|; the two losses within 1e-6 relative."""
    m, W, inp, dev, ref = _run(case)
    ratios = {k: _ratio(dev[k], ref[k]) for k in R.TENSORS}
    print("recog_grad %s: " % case + ", ".join("%s %.2e" % kv for kv in ratios.items()))
    for k in R.TENSORS:
        assert dev[k].shape == ref[k].shape and dev[k].dtype == F32, k
        assert ratios[k] <= REL, (k, ratios[k])
    for k in ("end_objectness_loss", "end_box_reg_loss"):
        assert abs(dev[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, dev[k], ref[k])
    assert dev["masked_end"] == ref["masked_end"] == len(CASES[case][3])


@pytest.mark.parametrize("case", list(CASES))
def test_every_row_matches_the_float64_restatement_at_the_float32_evaluations_bar(case):
    """fc6_w, fc7_w and boxreg_w row by row, feat pixel by pixel over its 512 channels, roi_boxes box by box
    (tests/grad_bars.py): every row within 8 x the float32 evaluation's worst per-row ratio of ITS OWN largest entry, and the
    rows whose reference is exactly zero (ReLU-dead rows, untouched pixels) all +0.0 bits."""
    import torch
    m, W, (feat, boxes, targets, g), dev, ref = _run(case)
    ref32 = R.recog_grad(W, feat, boxes, CASES[case][2], targets, g, IMG[0], IMG[1], dtype=torch.float32)
    GB.assert_rows("recog_grad " + case, GB.RECOG_ROW_TENSORS, dev, ref, ref32)


def test_no_positive_row_means_no_box_terms():
    m, W, inp, dev, ref = _run("minimal_1_0")
    assert dev["end_box_reg_loss"] == 0.0 and not dev["boxreg_w"].any() and not dev["boxreg_b"].any()


def test_the_codes_gradient_is_added():
    a, b = _run("minimal_5_2")[3], _run("minimal_5_2_no_g")[3]
    assert a["end_objectness_loss"] == b["end_objectness_loss"] and a["end_box_reg_loss"] == b["end_box_reg_loss"]
    assert not np.array_equal(a["fc7_w"], b["fc7_w"])
    assert np.array_equal(_bits(a["obj_w"]), _bits(b["obj_w"])) and np.array_equal(_bits(a["boxreg_b"]), _bits(b["boxreg_b"]))


@pytest.mark.parametrize("case", ["minimal_5_2", "minimal_256", "odd32_70"])
def test_two_calls_give_identical_bits(case):
    from densecap_amd import ops
    m, W, (feat, boxes, targets, g), dev, ref = _run(case)
    again = ops.recog_grad(m.ctx, feat, boxes, CASES[case][2], targets, IMG[0], IMG[1], dcodes=g)
    for k in R.TENSORS:
        assert np.array_equal(_bits(again[k]), _bits(dev[k])), k
    assert again["end_objectness_loss"] == dev["end_objectness_loss"] and again["end_box_reg_loss"] == dev["end_box_reg_loss"]


def test_losses_are_forward_losses_numbers_for_the_same_rows():
    """The forward half goes through dc_forward_losses' own calls, and loss_terms skips the terms an op gives no inputs for: on
    dc_forward_losses' sampled rows (dump) and feature map the two end losses and their masked count are its bits, and so are
    dc_op_rpn_grad's two mid losses and theirs.  In the second case every positive row is masked in both box terms: the ground-truth
    boxes are 1e5 times as tall, as wide or both as any anchor, thresholds 0 / 0 (every input that overlaps anything is positive)."""
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, W = _model("minimal")
    img = make_synthetic_image(IMG[0], IMG[1], 3)
    lab = np.ones((3, 1), np.int32)
    for masked in (False, True):
        gt = R.draw_boxes(np.random.default_rng(4), 3, IMG[0], IMG[1], MAP[0], MAP[1])
        opts = dict(batch_size=16)
        if masked:
            gt[:] = [[IMG[1] / 2, IMG[0] / 2, 40, 724e5], [IMG[1] / 2, IMG[0] / 2, 724e5, 40], [IMG[1] / 2, IMG[0] / 2, 724e5, 724e5]]
            opts.update(high_thresh=0.0, low_thresh=0.0)
        fl = m.forward_losses(img, gt, lab, dump=True, **opts)
        n = fl["num_pos"] + fl["num_neg"]
        feat, boxes = np.zeros((MAP[0], MAP[1], 512), F32), np.zeros((n, 4), F32)
        assert m.ctx.lib.dc_debug_fetch(m.ctx.h, b"feat_hwc", feat.ctypes.data, feat.nbytes) == feat.size
        assert m.ctx.lib.dc_debug_fetch(m.ctx.h, b"loss_roi_boxes", boxes.ctypes.data, boxes.nbytes) == boxes.size
        feat = feat.transpose(2, 0, 1)
        rg = ops.recog_grad(m.ctx, feat, boxes[:n], fl["num_pos"], gt[fl["pos_target_idx"]], IMG[0], IMG[1], **opts)
        assert rg["end_objectness_loss"] == fl["end_objectness_loss"] and rg["end_box_reg_loss"] == fl["end_box_reg_loss"]
        assert rg["masked_end"] == fl["masked_end"]
        pg = ops.rpn_grad(m.ctx, feat, fl["pos_input_idx"], fl["pos_target_idx"], fl["neg_input_idx"], gt, IMG[0], IMG[1], **opts)
        assert pg["mid_objectness_loss"] == fl["mid_objectness_loss"] and pg["mid_box_reg_loss"] == fl["mid_box_reg_loss"]
        assert pg["masked_mid"] == fl["masked_mid"]
        assert (fl["masked_mid"] >= 1 and fl["masked_end"] >= 1) == masked and fl["num_pos"] >= 1


def test_refusals_come_before_any_launch():
    from densecap_amd import ops, _lib
    m, W, (feat, boxes, targets, g), dev, ref = _run("minimal_5_2")
    with pytest.raises(_lib.DenseCapError, match="n must be in 1..1024"):
        ops.recog_grad(m.ctx, feat, np.zeros((1025, 4), F32), 0, None, IMG[0], IMG[1], batch_size=1024)
    with pytest.raises(_lib.DenseCapError, match="n must be in 1..1024"):
        ops.recog_grad(m.ctx, feat, np.zeros((0, 4), F32), 0, None, IMG[0], IMG[1])
    with pytest.raises(_lib.DenseCapError, match="num_pos"):
        ops.recog_grad(m.ctx, feat, boxes, 6, np.zeros((6, 4), F32), IMG[0], IMG[1])
    with pytest.raises(_lib.DenseCapError, match="batch_size"):
        ops.recog_grad(m.ctx, feat, boxes, 2, targets, IMG[0], IMG[1], batch_size=4)
    fd, bd, td = (m.ctx.to_device(a) for a in (np.ascontiguousarray(feat.transpose(1, 2, 0)), boxes, targets))
    lo, lb, me = C.c_double(0), C.c_double(0), C.c_int32(0)
    empty = _lib.DcRecogGrads()                                                   # every buffer null
    rc = m.ctx.lib.dc_op_recog_grad(m.ctx.h, fd.ptr, MAP[0], MAP[1], bd.ptr, 5, 2, td.ptr, None, IMG[0], IMG[1], None,
                                    C.byref(empty), C.byref(lo), C.byref(lb), C.byref(me))
    assert rc == -1                                                               # DC_E_INVALID
    assert np.array_equal(_bits(ops.recog_grad(m.ctx, feat, boxes, 2, targets, IMG[0], IMG[1], dcodes=g)["fc6_w"]), _bits(dev["fc6_w"]))


def test_settings_and_weights_survive_the_call():
    """Identical bits under dc_set_math_mode(1); forward_test gives the same outputs before and after a gradient call."""
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, W, (feat, boxes, targets, g), dev, ref = _run("odd32_5_2")
    img = make_synthetic_image(224, 288, 2)
    before = m.forward_raw(img)
    m.ctx.set_math_mode(1)
    try:
        mixed_before = m.forward_raw(img)
        again = ops.recog_grad(m.ctx, feat, boxes, 2, targets, IMG[0], IMG[1], dcodes=g)
        mixed_after = m.forward_raw(img)
    finally:
        m.ctx.set_math_mode(0)
    after = m.forward_raw(img)
    for k in R.TENSORS:
        assert np.array_equal(_bits(again[k]), _bits(dev[k])), k
    for a, b in ((before, after), (mixed_before, mixed_after)):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_stage_split_is_reported():
    from densecap_amd import ops
    m = _run("minimal_256")[0]
    ms = ops.recog_grad_stage_ms(m.ctx)
    assert set(ms) == {"heads_fc", "dpool", "roi_scatter", "roi_boxes"} and all(v > 0 for v in ms.values())
