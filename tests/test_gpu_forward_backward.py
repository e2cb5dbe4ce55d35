"""dc_forward_backward end to end on a 96 x 128 image at the "minimal" dimensions of tests/test_gpu_dims.py: its losses, lists,
recognition and language-model gradients are dc_loss_gradients' bits, its RPN gradients dc_op_rpn_grad's bits on what the forward
left and the float64 restatement's (tests/rpn_grad_rules.py) within the bars, feat is feat_roi + feat_rpn as one fp32 add, and a
step against the RPN gradients lowers the float64 loss as first order predicts (docs/SEMANTICS.md, "RPN gradients")."""
import os
import re

import numpy as np
import pytest

from tests import lm_grad_rules as G
from tests import loss_rules as LR
from tests import recog_grad_rules as RR
from tests import rpn_grad_rules as R
from tests.test_gpu_rpn_grad import check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
H, WD, MAP = 96, 128, (6, 8)
OPTS = dict(batch_size=16, seed=3, remove_outbounds=0)
DECAY = 5e-5
COUNTS = ("num_pos", "num_neg", "total_pos", "total_neg", "masked_mid", "masked_end", "flags")
LISTS = ("pos_input_idx", "pos_target_idx", "neg_input_idx")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def run():
    """The model, its weights, the inputs (ground truth made of RPN boxes, as tests/test_gpu_loss_gradients.py makes its own), one
    dc_forward_backward call and the feature map it ran on."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image
    from tests.test_gpu_dims import set_weights
    W = set_weights("minimal")
    m = DenseCapModel(W, device=0)
    img = make_synthetic_image(H, WD, 6)
    A = m.num_anchors * MAP[0] * MAP[1]
    rng = np.random.default_rng(11)
    m.forward_losses(img, np.array([[60, 50, 60, 40]], F32), np.ones((1, 1), np.int32), **OPTS)
    boxes = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
    big = np.nonzero((boxes[:, 2] > 20) & (boxes[:, 3] > 20))[0]
    pick = big[np.linspace(0, len(big) - 1, 4).astype(int)]
    gt = (boxes[pick] + np.array([[1, -1, 0, 0], [2, 1, 0, 0], [-1, 2, 0, 0], [0, 1, 1, 0]], F32)).astype(F32)
    lab = G.draw_labels(4, m.seq_length, m.vocab_size, rng)
    res = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **OPTS)
    feat = m.debug_fetch("feat_hwc", (MAP[0], MAP[1], 512))[0].transpose(2, 0, 1).copy()
    yield m, W, img, gt, lab, res, feat
    m.ctx.close()


def test_everything_loss_gradients_returns_is_its_bits(run):
    m, W, img, gt, lab, res, feat = run
    lg = m.loss_gradients(img, gt, lab, dump=True, **OPTS)
    assert res["num_pos"] >= 2 and res["num_neg"] >= 1
    for k in LR.LOSS_KEYS:
        assert _bits(np.float64(res[k])) == _bits(np.float64(lg[k])), k
    for k in COUNTS:
        assert res[k] == lg[k], k
    for k in LISTS:
        assert np.array_equal(res[k], lg[k]), k
    for k in RR.TENSORS + G.TENSORS:
        assert np.array_equal(_bits(res["feat_roi" if k == "feat" else k]), _bits(lg[k])), k


def _rpn_args(res, gt):
    return res["pos_input_idx"], res["pos_target_idx"], res["neg_input_idx"], gt


def test_rpn_gradients_are_rpn_grads_bits_and_the_rules(run):
    from densecap_amd import ops
    m, W, img, gt, lab, res, feat = run
    pi, pt, ni, _ = _rpn_args(res, gt)
    droi = res["roi_boxes"]
    want = ops.rpn_grad(m.ctx, feat, pi, pt, ni, gt, H, WD, droi_boxes=droi, box_reg_decay=DECAY, **OPTS)
    for k in R.RPN_PARAMS:
        assert np.array_equal(_bits(res[k]), _bits(want[k])), k
    assert np.array_equal(_bits(res["feat_rpn"]), _bits(want["feat"]))
    assert want["mid_objectness_loss"] == res["mid_objectness_loss"] and want["mid_box_reg_loss"] == res["mid_box_reg_loss"]
    assert want["masked_mid"] == res["masked_mid"]
    dev = dict({k: res[k] for k in R.RPN_PARAMS}, feat=res["feat_rpn"])
    check("forward_backward", dev, R.rpn_grad(W, feat, pi, pt, ni, gt, droi, DECAY), R.rpn_grad(W, feat, pi, pt, ni, gt, droi, DECAY, dtype="float32"))


def test_feat_is_one_fp32_add_of_its_two_shares(run):
    m, W, img, gt, lab, res, feat = run
    assert res["feat"].shape == res["feat_roi"].shape == res["feat_rpn"].shape == (512,) + MAP
    assert np.array_equal(_bits(res["feat"]), _bits((res["feat_roi"] + res["feat_rpn"]).astype(F32)))
    assert res["feat_roi"].any() and res["feat_rpn"].any()


def test_forced_lists_with_a_duplicate_negative_match_the_rules(run):
    m, W, img, gt, lab, res, feat = run
    forced = dict(forced_pos=[1, 0], forced_neg=[2, 0, 2, 1])
    a = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **forced, **OPTS)
    b = m.loss_gradients(img, gt, lab, dump=True, **forced, **OPTS)
    assert (a["num_pos"], a["num_neg"]) == (2, 4) and a["neg_input_idx"][0] == a["neg_input_idx"][2]
    for k in LR.LOSS_KEYS:
        assert _bits(np.float64(a[k])) == _bits(np.float64(b[k])), k
    for k in RR.TENSORS + G.TENSORS:
        assert np.array_equal(_bits(a["feat_roi" if k == "feat" else k]), _bits(b[k])), k
    pi, pt, ni, _ = _rpn_args(a, gt)
    dev = dict({k: a[k] for k in R.RPN_PARAMS}, feat=a["feat_rpn"])
    args = (W, feat, pi, pt, ni, gt, a["roi_boxes"], DECAY)
    check("forward_backward forced", dev, R.rpn_grad(*args), R.rpn_grad(*args, dtype="float32"))
    assert np.array_equal(_bits(a["feat"]), _bits((a["feat_roi"] + a["feat_rpn"]).astype(F32)))


def test_two_calls_give_identical_bits(run):
    m, W, img, gt, lab, res, feat = run
    again = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **OPTS)
    for k in R.RPN_PARAMS + ("feat", "feat_rpn", "feat_roi"):
        assert np.array_equal(_bits(again[k]), _bits(res[k])), k


def test_a_gradient_step_lowers_the_float64_loss_as_first_order_predicts(run):
    """W' = W - eta g on the six RPN tensors, g the DEVICE's gradient, the lists held: the float64 restated loss mid_objectness +
    mid_box_reg + 0.5 decay |trans|^2 + <droi, boxes> drops by eta |g|^2 within 10 %.  eta is halved until the restatement itself,
    stepped along its own gradient, is first-order to 5 % (as tests/test_gpu_loss_gradients.py judges its own step)."""
    import torch
    m, W, img, gt, lab, res, feat = run
    pi, pt, ni, _ = _rpn_args(res, gt)
    assert len(set(pi.tolist()) | set(ni.tolist())) == len(pi) + len(ni)          # no input row twice: the rules are a gradient
    droi = res["roi_boxes"]
    ref = R.rpn_grad(W, feat, pi, pt, ni, gt, droi, DECAY)

    def loss(grads, eta):
        leaves = {k: torch.as_tensor(np.asarray(W[k], np.float64)) - eta * torch.as_tensor(np.asarray(grads[k], np.float64)).reshape(tuple(W[k].shape))
                  for k in R.RPN_PARAMS}
        leaves["feat"] = torch.as_tensor(feat.astype(np.float64))
        with torch.no_grad():
            return R.rpn_loss(W, feat, pi, pt, ni, gt, droi, DECAY, opts=None, leaves=leaves)
    base, (mo, mb, masked) = loss(ref, 0.0)
    base = float(base)
    assert mo == pytest.approx(res["mid_objectness_loss"], rel=1e-5) and mb == pytest.approx(res["mid_box_reg_loss"], rel=1e-5)
    g2 = sum(float((ref[k] ** 2).sum()) for k in R.RPN_PARAMS)
    eta = 0.02 / np.sqrt(g2)
    for _ in range(12):
        drop = base - float(loss(ref, eta)[0])
        if abs(drop - eta * g2) <= 0.05 * eta * g2:
            break
        eta *= 0.5
    assert drop > 0 and abs(drop - eta * g2) <= 0.05 * eta * g2
    dg2 = sum(float((res[k].astype(np.float64) ** 2).sum()) for k in R.RPN_PARAMS)
    got = base - float(loss(res, eta)[0])
    print("descent: eta %.3e, predicted drop %.6e, observed drop %.6e" % (eta, eta * dg2, got))
    assert got > 0 and abs(got - eta * dg2) <= 0.10 * eta * dg2


def test_shapes_and_the_lua_key_list():
    """The Lua wrapper names the RPN tensors as the Python one does, by text."""
    from densecap_amd import ops
    lua = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    body = lua[lua.index("function Model:forward_backward"):]
    body = body[:body.index("\nend\n")]
    names = re.search(r"local pnames = \{(.*?)\}", body).group(1)
    assert tuple(re.findall(r"'(\w+)'", names)) == ops.RPN_GRAD_KEYS
    for k in ops.RECOG_GRAD_KEYS + ops.LM_GRAD_KEYS:
        assert "'%s'" % k in body, k
    assert "feat_roi" in body and "dc_forward_backward" in body and "box_reg_decay" in body
