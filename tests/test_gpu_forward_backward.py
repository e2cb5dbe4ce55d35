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


def _assert_same_result(a, b):
    """Every key of two result dicts: arrays by dtype, shape and bytes, scalars by value."""
    assert set(a) == set(b)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and v.shape == b[k].shape and v.tobytes() == b[k].tobytes(), k
        else:
            assert _bits(np.float64(v)) == _bits(np.float64(b[k])), k


def test_the_forward_record_is_per_call(run):
    """A training forward at another size (another map, another A) and a test forward in between leave nothing behind."""
    from densecap_amd.weights import make_synthetic_image
    m, W, img, gt, lab, res, feat = run
    m.forward_losses(make_synthetic_image(64, 96, 2), np.array([[40, 30, 30, 24]], F32), np.ones((1, 1), np.int32), **OPTS)
    m.forward_test(img)
    _assert_same_result(m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **OPTS), res)


def fetch_loss_names(m, num_pos, num_neg):
    """Every "loss_*" array of dc_debug_fetch, and loss_stage_ms."""
    A, n = m.num_anchors * MAP[0] * MAP[1], num_pos + num_neg
    shapes = {"loss_rpn_boxes": (A, 4), "loss_rpn_anchors": (A, 4), "loss_rpn_trans": (A, 4), "loss_rpn_scores": (A, 2), "loss_obj": (n,),
              "loss_final_trans": (n, 4), "loss_roi_boxes": (n, 4), "loss_codes": (n, m.fc_dim)}
    out = {}
    for k, s in shapes.items():
        out[k], count = m.debug_fetch(k, s)
        assert count == int(np.prod(s)), k
    out["loss_rowlik"], count = m.debug_fetch("loss_rowlik", (num_pos,), np.float64)
    assert count == num_pos
    out["loss_stage_ms"], count = m.debug_fetch("loss_stage_ms", (5,))
    assert count == 5
    return out


def test_the_fetch_names_hold_the_same_bits_after_every_entry_point(run):
    m, W, img, gt, lab, res, feat = run
    first = None
    for call in (m.forward_losses, m.loss_gradients, m.forward_backward):
        r = call(img, gt, lab, **OPTS)
        got = fetch_loss_names(m, r["num_pos"], r["num_neg"])
        ms = got.pop("loss_stage_ms")
        assert ms.shape == (5,) and np.isfinite(ms).all() and (ms >= 0).all(), call.__name__
        first = first or got
        for k in got:
            assert got[k].size > 0 and got[k].tobytes() == first[k].tobytes(), (call.__name__, k)


def test_no_sampled_row_means_zero_gradients_and_forward_losses_numbers(run):
    """Both forced lists empty, box_reg_decay = 0 (the decay term is decay * trans on every RPN row, sampled or not: it alone
    would be left in the RPN's gradients)."""
    m, W, img, gt, lab, res, feat = run
    empty = dict(forced_pos=[], forced_neg=[])
    a = m.forward_backward(img, gt, lab, box_reg_decay=0.0, dump=True, **empty, **OPTS)
    fl = m.forward_losses(img, gt, lab, **empty, **OPTS)
    assert a["num_pos"] == a["num_neg"] == 0
    for k in RR.TENSORS + G.TENSORS + R.RPN_PARAMS + ("feat", "feat_roi", "feat_rpn"):
        assert (a[k] == 0).all(), k
    for k in LR.LOSS_KEYS:
        assert _bits(np.float64(a[k])) == _bits(np.float64(fl[k])), k


SENTINEL = np.float32(-7.5)
# the refusals of dc_forward_backward's own arguments and of the calls it used to nest: what, the error code
FB_REFUSALS = (("decay", -1), ("gt_w0", -1), ("G0", -5), ("G513", -5))


def forward_backward_refusals(m, img, gt, lab):
    """dc_forward_backward with one bad argument at a time on sentinel-filled outputs: ({what: code}, every output buffer still
    holds the sentinel)."""
    import ctypes as C
    from densecap_amd import _lib, ops
    ctx, k, Rh, D, E, Hd, V = m.ctx, m.num_anchors, m.ctx.lm_dims["R"], m.fc_dim, m.ctx.lm_dims["E"], m.ctx.lm_dims["Hd"], m.vocab_size
    h, w = MAP
    cap = OPTS["batch_size"]
    shapes = [{"fc6_w": (D, 512 * 49), "fc6_b": (D,), "fc7_w": (D, D), "fc7_b": (D,), "obj_w": (1, D), "obj_b": (1,), "boxreg_w": (4, D),
               "boxreg_b": (4,), "feat": (h, w, 512), "roi_boxes": (cap, 4)},
              {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
               "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (cap, D)},
              {"rpn_conv_w": (Rh, 512, 3, 3), "rpn_conv_b": (Rh,), "rpn_box_w": (4 * k, Rh), "rpn_box_b": (4 * k,),
               "rpn_score_w": (2 * k, Rh), "rpn_score_b": (2 * k,), "feat": (h, w, 512)}]
    bufs = [{n: ctx.to_device(np.full(s, SENTINEL, F32)) for n, s in sh.items()} for sh in shapes]
    rg, lg, pg = (T(**{n: b.ptr for n, b in bs.items()}) for T, bs in zip((_lib.DcRecogGrads, _lib.DcLmGrads, _lib.DcRpnGrads), bufs))
    o = ops.loss_opts(**OPTS)
    img = np.ascontiguousarray(img, F32)
    lab513 = np.ones((513, lab.shape[1]), np.int32)
    gt513 = np.tile(gt, (130, 1))[:513].copy()
    bad_gt = gt.copy()
    bad_gt[1, 2] = 0.0

    def call(g=gt, labels=lab, G=len(gt), decay=DECAY):
        out = _lib.DcLosses()
        g, labels = np.ascontiguousarray(g, F32), np.ascontiguousarray(labels, np.int32)
        return ctx.lib.dc_forward_backward(ctx.h, img.ctypes.data, H, WD, 0, g.ctypes.data, labels.ctypes.data, G, labels.shape[1],
                                           C.byref(o), None, C.byref(out), None, C.byref(rg), C.byref(lg), float(decay), C.byref(pg))
    codes = {"decay": call(decay=-1e-3), "gt_w0": call(g=bad_gt), "G0": call(G=0), "G513": call(g=gt513, labels=lab513, G=513)}
    untouched = all(np.array_equal(_bits(b.numpy()), _bits(np.full(sh[n], SENTINEL, F32)))
                    for sh, bs in zip(shapes, bufs) for n, b in bs.items())
    return codes, untouched


def test_refusals_of_the_outer_call_come_before_any_launch_and_leave_the_outputs_alone(run):
    m, W, img, gt, lab, res, feat = run
    codes, untouched = forward_backward_refusals(m, img, gt, lab)
    assert codes == dict(FB_REFUSALS) and untouched
    _assert_same_result(m.forward_backward(img, gt, lab, box_reg_decay=DECAY, dump=True, **OPTS), res)     # the context works on


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
