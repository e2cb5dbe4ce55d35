"""Dropout inside the training calls (docs/SEMANTICS.md, "Dropout") on the 96 x 128 image and the "minimal" weights of
tests/test_gpu_loss_gradients.py, with forced sampler lists where the row count must be fixed.

Layer 1 is pinned bit for bit: fc6's forward does not depend on Dropout, so "loss_fc6_out" at p = 0.5 is where(mask1, 2 * the
p = 0 activation, +0.0).  Everything downstream is held to tests/dropout_rules.py's float64 restatement, fed with the rule's masks,
under tests/grad_bars.py's per-row rule at its own bar; scalars and the tensors that rule does not take (biases, obj_w) at the bars
the recognition and language-model gradient tests already use (1e-6 relative for a loss, 1e-4 of a tensor's largest entry)."""
import numpy as np
import pytest

from tests import dropout_rules as DR
from tests import grad_bars as GB
from tests import lm_grad_rules as G
from tests import optim_rules as OR
from tests import recog_grad_rules as R

pytestmark = pytest.mark.gpu

REL = 1e-4
F32 = np.float32
H, WD, MAP = 96, 128, (6, 8)
OPTS = dict(batch_size=16, seed=3, remove_outbounds=0)
FORCED = dict(forced_pos=[1, 0], forced_neg=[2, 0, 2, 1])
DECAY = 5e-5
LOSS_KEYS = ("mid_objectness_loss", "mid_box_reg_loss", "end_objectness_loss", "end_box_reg_loss", "captioning_loss", "total_loss")
MAX_NORM_TENSORS = ("fc6_b", "fc7_b", "obj_w", "obj_b", "boxreg_b")       # (the 2-D ones go row by row)
_cases = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _model(W, p=None):
    from densecap_amd import DenseCapModel
    m = DenseCapModel(W, device=0)
    if p is not None:
        m.set_dropout(p)
    return m


@pytest.fixture(scope="module")
def run():
    """The model, its weights and inputs, and one dc_loss_gradients call at p = 0 with the activations it left."""
    from densecap_amd.weights import make_synthetic_image
    from tests.test_gpu_dims import set_weights
    W = set_weights("minimal")
    m = _model(W)
    img = make_synthetic_image(H, WD, 6)
    A = m.num_anchors * MAP[0] * MAP[1]
    m.forward_losses(img, np.array([[60, 50, 60, 40]], F32), np.ones((1, 1), np.int32), **OPTS)
    boxes = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
    big = np.nonzero((boxes[:, 2] > 20) & (boxes[:, 3] > 20))[0]
    pick = big[np.linspace(0, len(big) - 1, 4).astype(int)]
    gt = (boxes[pick] + np.array([[1, -1, 0, 0], [2, 1, 0, 0], [-1, 2, 0, 0], [0, 1, 1, 0]], F32)).astype(F32)
    lab = G.draw_labels(4, m.seq_length, m.vocab_size, np.random.default_rng(11))
    assert m.dropout == 0.0
    base = m.loss_gradients(img, gt, lab, dump=True, **FORCED, **OPTS)
    n = base["num_pos"] + base["num_neg"]
    assert (base["num_pos"], base["num_neg"]) == (2, 4)
    kept = dict(feat=m.debug_fetch("feat_hwc", (MAP[0], MAP[1], 512))[0].transpose(2, 0, 1).copy(),
                roi_boxes=m.debug_fetch("loss_roi_boxes", (n, 4))[0].copy(), fc6_out=m.debug_fetch("loss_fc6_out", (n, m.fc_dim))[0].copy(),
                codes=m.debug_fetch("loss_codes", (n, m.fc_dim))[0].copy())
    yield m, W, img, gt, lab, base, kept
    m.ctx.close()
    _cases.clear()


def _case(run, p):
    """dc_loss_gradients at p on the fixture's rows, what it left, the rule's masks and the restatement in float64 and float32;
    computed once.  The context is back at p = 0 afterwards."""
    import torch
    if p not in _cases:
        m, W, img, gt, lab, base, kept = run
        m.set_dropout(p)
        try:
            assert m.dropout == float(F32(p))
            res = m.loss_gradients(img, gt, lab, dump=True, **FORCED, **OPTS)
            n, D = res["num_pos"] + res["num_neg"], m.fc_dim
            left = dict(fc6_out=m.debug_fetch("loss_fc6_out", (n, D))[0].copy(), codes=m.debug_fetch("loss_codes", (n, D))[0].copy(),
                        roi_boxes=m.debug_fetch("loss_roi_boxes", (n, 4))[0].copy())
        finally:
            m.set_dropout(0.0)
        m1, m2 = DR.masks_for(n, D, p, OPTS["seed"])
        args = (W, kept["feat"], kept["roi_boxes"], res["num_pos"], gt[res["pos_target_idx"]], res["codes"], H, WD, m1, m2, p)
        _cases[p] = (res, left, m1, m2, DR.recog_grad(*args), DR.recog_grad(*args, dtype=torch.float32))
    return _cases[p]


def test_p_0_after_p_05_is_a_context_that_never_set_it(run):
    m, W, img, gt, lab, base, kept = run
    m2 = _model(W)
    try:
        want = m2.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **FORCED, **OPTS)
    finally:
        m2.ctx.close()
    m.set_dropout(0.5)
    dropped = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **FORCED, **OPTS)
    m.set_dropout(0)
    got = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **FORCED, **OPTS)
    assert dropped["end_objectness_loss"] != want["end_objectness_loss"]
    for k, v in want.items():
        a, b = np.asarray(got[k]), np.asarray(v)
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    for k in LOSS_KEYS:
        assert _bits(np.float64(got[k])) == _bits(np.float64(base[k])), k


def test_fc6_mask_at_p_05_is_the_rule_bit_for_bit(run):
    res, left, m1, m2, ref, ref32 = _case(run, 0.5)
    kept = run[6]
    want = np.where(m1, kept["fc6_out"] * F32(2), F32(0.0)).astype(F32)
    assert np.array_equal(_bits(left["fc6_out"]), _bits(want))
    assert (kept["fc6_out"][~m1] > 0).any() and (left["fc6_out"] > 0).any()                   # the mask dropped something alive
    assert np.array_equal(_bits(left["roi_boxes"]), _bits(kept["roi_boxes"]))


def test_codes_at_p_05_are_plus_zero_where_mask_2_drops(run):
    res, left, m1, m2, ref, ref32 = _case(run, 0.5)
    assert not _bits(left["codes"][~m2]).any()
    assert (left["codes"][m2] > 0).any() and not np.array_equal(m1, m2)


def _check_against_the_restatement(run, p):
    m, W, img, gt, lab, base, kept = run
    res, left, m1, m2, ref, ref32 = _case(run, p)
    np_ = res["num_pos"]
    what = "loss_gradients p = %g" % p
    # ---- the dropped codes, the recognition gradients row by row ----
    dev = dict(res, codes_fwd=left["codes"], feat=res["feat"])
    tensors = ("codes_fwd",) + GB.RECOG_ROW_TENSORS
    assert not DR.row_failures(what, dev, ref, ref32, tensors)
    for k in MAX_NORM_TENSORS:
        ratio = float(np.abs(res[k] - ref[k]).max() / np.abs(ref[k]).max())
        print("%s: %s %.2e" % (what, k, ratio))
        assert res[k].shape == ref[k].shape and ratio <= REL, (k, ratio)
    # ---- the losses ----
    for k in ("end_objectness_loss", "end_box_reg_loss"):
        print("%s: %s %.3e" % (what, k, abs(res[k] - ref[k]) / abs(ref[k])))
        assert abs(res[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, res[k], ref[k])
        assert res[k] != base[k], k
    # ---- the language model reads the dropped codes: its loss and lm_enc_w against lm_grad_rules on them ----
    import torch
    largs = (W, left["codes"][:np_], lab[res["pos_target_idx"]])
    l64, l32 = G.lm_grad(*largs), G.lm_grad(*largs, dtype=torch.float32)
    print("%s: captioning_loss %.3e" % (what, abs(res["captioning_loss"] - l64["loss"]) / abs(l64["loss"])))
    assert abs(res["captioning_loss"] - l64["loss"]) <= 1e-6 * abs(l64["loss"])
    assert not DR.row_failures(what + " lm", res, l64, l32, ("lm_enc_w",))
    # ---- dead rows: no sampled row alive and kept in that unit ----
    dead7, dead6 = ~(left["codes"] > 0).any(0), ~(left["fc6_out"] > 0).any(0)
    assert dead7.any() and dead6.any() and not dead7.all() and not dead6.all()
    assert not _bits(res["fc7_w"][dead7]).any() and not _bits(res["fc6_w"][dead6]).any()
    assert res["fc7_w"][~dead7].any(1).all()


def test_losses_and_gradients_match_the_restatement_at_p_05(run):
    _check_against_the_restatement(run, 0.5)


def test_losses_and_gradients_match_the_restatement_at_p_01(run):
    """The scale 1 / (1 - 0.1f) is inexact in float32: fc6's output against the numpy form, the rest as at p = 0.5."""
    res, left, m1, m2, ref, ref32 = _case(run, 0.1)
    assert np.array_equal(_bits(left["fc6_out"]), _bits(DR.apply_mask(run[6]["fc6_out"], m1, 0.1)))
    assert not _bits(left["codes"][~m2]).any()
    _check_against_the_restatement(run, 0.1)


@pytest.mark.parametrize("name,n,np_", [("minimal", 1, 1), ("minimal", 5, 2), ("minimal", 70, 33), ("odd32", 5, 2)])
def test_recog_grad_on_caller_rows(run, name, n, np_):
    """dc_op_recog_grad at p = 0.5 on generated rows; odd32: fc_dim = 768, a dimension set of tests/test_gpu_dims.py's family."""
    import torch
    from densecap_amd import ops
    from tests.test_gpu_dims import set_weights
    own = name != "minimal"
    m, W = (_model(set_weights(name)), set_weights(name)) if own else (run[0], run[1])
    try:
        rng = np.random.default_rng(500 + n * 8 + np_)
        feat, boxes, targets = R.draw_case(W, rng, n, np_, H, WD, MAP[0], MAP[1], far_rows=(1,) if np_ > 1 else (), outside=0.2)
        g = (rng.standard_normal((np_, m.fc_dim)) * 1e-3).astype(F32)
        m.set_dropout(0.5)
        dev = ops.recog_grad(m.ctx, feat, boxes, np_, targets, H, WD, dcodes=g, seed=9, batch_size=256)
        again = ops.recog_grad(m.ctx, feat, boxes, np_, targets, H, WD, dcodes=g, seed=9, batch_size=256)
        other = ops.recog_grad(m.ctx, feat, boxes, np_, targets, H, WD, dcodes=g, seed=10, batch_size=256)
    finally:
        m.set_dropout(0.0)
        if own:
            m.ctx.close()
    m1, m2 = DR.masks_for(n, m.fc_dim, 0.5, 9)
    args = (W, feat, boxes, np_, targets, g, H, WD, m1, m2, 0.5)
    ref, ref32 = DR.recog_grad(*args), DR.recog_grad(*args, dtype=torch.float32)
    assert not DR.row_failures("recog_grad %s n = %d" % (name, n), dev, ref, ref32)
    for k in MAX_NORM_TENSORS:
        assert float(np.abs(dev[k] - ref[k]).max()) <= REL * float(np.abs(ref[k]).max()), k
    for k in ("end_objectness_loss", "end_box_reg_loss"):
        assert abs(dev[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, dev[k], ref[k])
    for k in R.TENSORS:
        assert np.array_equal(_bits(again[k]), _bits(dev[k])), k
    assert other["end_objectness_loss"] != dev["end_objectness_loss"]


def test_masks_follow_the_seed(run):
    m, W, img, gt, lab, base, kept = run
    m.set_dropout(0.5)
    try:
        a = m.forward_losses(img, gt, lab, **FORCED, **OPTS)
        b = m.forward_losses(img, gt, lab, **FORCED, **OPTS)
        c = m.forward_losses(img, gt, lab, **FORCED, **dict(OPTS, seed=OPTS["seed"] + 2 ** 32))
    finally:
        m.set_dropout(0.0)
    for k in LOSS_KEYS:
        assert _bits(np.float64(a[k])) == _bits(np.float64(b[k])), k
        assert _bits(np.float64(a[k])) == _bits(np.float64(_case(run, 0.5)[0][k])), k      # dc_loss_gradients' forward is this one
    for k in ("mid_objectness_loss", "mid_box_reg_loss"):                                   # forced lists: the same rows, other masks
        assert a[k] == c[k], k
    for k in ("end_objectness_loss", "end_box_reg_loss", "captioning_loss"):
        assert a[k] != c[k], k


def _rule_step(Wk, grads, mom, t, **opts):
    from densecap_amd.ops import WEIGHT_KEYS
    as32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=F32)
    out = {}
    for k in WEIGHT_KEYS:
        p = as32(Wk[k])
        mm, vv = mom.get(k, (np.zeros(p.size, F32), np.zeros(p.size, F32)))
        pn, mn, vn = OR.adam_step32(p.reshape(-1), as32(grads[k]).reshape(-1), mm, vv, t, **opts)
        out[k] = pn.reshape(p.shape)
        mom[k] = (mn, vn)
    return out


def test_two_train_steps_at_p_05_are_the_rule_on_the_devices_own_gradients(run):
    from densecap_amd.ops import WEIGHT_KEYS
    _m, W, img, gt, lab, base, kept = run
    fast = dict(learning_rate=1e-3, weight_decay=1e-2)
    as32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=F32)
    m = _model(W, 0.5)
    try:
        m.train_begin(**fast)
        Wk, mom = W, {}
        for t in (1, 2):
            m0 = _model(Wk, 0.5)                  # a fresh context with step t-1's exported weights and the same p
            try:
                grads = m0.forward_backward(img, gt, lab, box_reg_decay=DECAY, **FORCED, **dict(OPTS, seed=OPTS["seed"] + t))
            finally:
                m0.ctx.close()
            want = _rule_step(Wk, grads, mom, t, **dict(OR.DEFAULTS, **fast))
            res = m.train_step(img, gt, lab, box_reg_decay=DECAY, **FORCED, **dict(OPTS, seed=OPTS["seed"] + t))
            for k in LOSS_KEYS:
                assert _bits(np.float64(res[k])) == _bits(np.float64(grads[k])), (t, k)
            Wk = m.get_weights()
            for k in WEIGHT_KEYS:
                assert np.array_equal(_bits(as32(Wk[k]).reshape(-1)), _bits(as32(want[k]).reshape(-1))), (t, k)
        assert m.dropout == 0.5
        trained = m.forward_losses(img, gt, lab, **FORCED, **OPTS)
        m.train_end()
    finally:
        m.ctx.close()
    m0 = _model(Wk, 0.5)
    try:
        fresh = m0.forward_losses(img, gt, lab, **FORCED, **OPTS)
    finally:
        m0.ctx.close()
    for k in LOSS_KEYS:
        assert _bits(np.float64(trained[k])) == _bits(np.float64(fresh[k])), k
    assert trained["end_objectness_loss"] != base["end_objectness_loss"]


def test_inference_never_drops(run):
    m, W, img, gt, lab, base, kept = run
    q = np.array([[1], [3]], np.int32)
    before = (m.forward_raw(img), m.scoreCaptions(img, q))
    m.set_dropout(0.5)
    try:
        after = (m.forward_raw(img), m.scoreCaptions(img, q))
    finally:
        m.set_dropout(0.0)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.tobytes() == y.tobytes()


def test_the_setting_is_checked(run):
    from densecap_amd import _lib
    m = run[0]
    for bad in (np.nan, -0.1, 1.0, 2.0, np.inf):
        with pytest.raises(_lib.DenseCapError, match="dc_set_dropout"):
            m.set_dropout(bad)
        assert m.dropout == 0.0
    tiny = float(np.nextafter(F32(0), F32(1)))
    assert m.set_dropout(tiny).dropout == tiny and m.set_dropout(0.0).dropout == 0.0
