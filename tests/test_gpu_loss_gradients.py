"""dc_loss_gradients end to end on a 96 x 128 image at the "minimal" dimensions of tests/test_gpu_dims.py: its losses are
dc_forward_losses' bits, its language-model gradients dc_op_lm_grad's bits, its recognition gradients the float64 restatement's
(tests/recog_grad_rules.py) on the rows the sampler drew, and a step against them lowers the float64 loss as first order predicts
(docs/SEMANTICS.md, "Recognition-net gradients"; the figures are recorded in DESIGN.md §17)."""
import numpy as np
import pytest

from tests import grad_bars as GB
from tests import lm_grad_rules as G
from tests import loss_rules as LR
from tests import recog_grad_rules as R

pytestmark = pytest.mark.gpu

REL = 1e-4
F32 = np.float32
H, WD, MAP = 96, 128, (6, 8)
OPTS = dict(batch_size=16, seed=3, remove_outbounds=0)
COUNTS = ("num_pos", "num_neg", "total_pos", "total_neg", "masked_mid", "masked_end", "flags")
LISTS = ("pos_input_idx", "pos_target_idx", "neg_input_idx")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def run():
    """The model, its weights, the inputs, and one dc_loss_gradients call with what it left in the context."""
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
    res = m.loss_gradients(img, gt, lab, dump=True, **OPTS)
    n = res["num_pos"] + res["num_neg"]
    kept = dict(feat=m.debug_fetch("feat_hwc", (MAP[0], MAP[1], 512))[0].transpose(2, 0, 1).copy(),
                roi_boxes=m.debug_fetch("loss_roi_boxes", (n, 4))[0].copy(), codes=m.debug_fetch("loss_codes", (n, m.fc_dim))[0].copy())
    yield m, W, img, gt, lab, res, kept
    m.ctx.close()


def test_losses_are_forward_losses_bits_with_and_without_forced_lists(run):
    m, W, img, gt, lab, res, kept = run
    fl = m.forward_losses(img, gt, lab, dump=True, **OPTS)
    assert res["num_pos"] >= 2 and res["num_neg"] >= 1
    for k in LR.LOSS_KEYS:
        assert _bits(np.float64(res[k])) == _bits(np.float64(fl[k])), k
    for k in COUNTS:
        assert res[k] == fl[k], k
    for k in LISTS:
        assert np.array_equal(res[k], fl[k]), k
    forced = dict(forced_pos=[1, 0], forced_neg=[2, 0, 1])
    a, b = m.loss_gradients(img, gt, lab, dump=True, **forced, **OPTS), m.forward_losses(img, gt, lab, dump=True, **forced, **OPTS)
    assert (a["num_pos"], a["num_neg"]) == (2, 3)
    for k in LR.LOSS_KEYS:
        assert _bits(np.float64(a[k])) == _bits(np.float64(b[k])), k
    for k in LISTS:
        assert np.array_equal(a[k], b[k]), k
    assert a["roi_boxes"].shape == (5, 4) and a["codes"].shape == (2, m.fc_dim)


def test_language_model_gradients_are_lm_grads_bits(run):
    from densecap_amd import ops
    m, W, img, gt, lab, res, kept = run
    np_ = res["num_pos"]
    want = ops.lm_grad(m.ctx, kept["codes"][:np_], lab[res["pos_target_idx"]], weight=1.0)
    for k in G.TENSORS:
        assert np.array_equal(_bits(res[k]), _bits(want[k])), k
    assert want["loss"] == res["captioning_loss"]


def test_recognition_gradients_match_the_rules_on_the_sampled_rows(run):
    m, W, img, gt, lab, res, kept = run
    np_ = res["num_pos"]
    # The rows are the sampler's, not a generator's, so R.EDGE is not enforced (of 16 x 98 coordinates a few lie within 1e-3 px
    # of an integer by chance).  Floors cannot disagree -- the restatement floors the device's own float32 coordinates -- and both
    # sides hold the floor constant; only a coordinate ON an integer leaves the derivative one-sided.  Say so if it happens.
    assert (R.edge_distance(kept["roi_boxes"], H, WD, MAP[0], MAP[1], 7, 7) > 1e-6).all(), "a sampled row has a sampling coordinate on an integer"
    ref = R.recog_grad(W, kept["feat"], kept["roi_boxes"], np_, gt[res["pos_target_idx"]], res["codes"], H, WD)
    ratios = {k: float(np.abs(res[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in R.TENSORS}
    print("loss_gradients (n %d, num_pos %d): " % (len(kept["roi_boxes"]), np_) + ", ".join("%s %.2e" % kv for kv in ratios.items()))
    for k in R.TENSORS:
        assert res[k].shape == ref[k].shape and ratios[k] <= REL, (k, ratios[k])
    for k in ("end_objectness_loss", "end_box_reg_loss"):
        assert abs(res[k] - ref[k]) <= 1e-6 * abs(ref[k]), k


def test_every_row_matches_the_rules_at_the_float32_evaluations_bar(run):
    """The 2-D tensors of both backward passes row by row (tests/grad_bars.py), on the rows the sampler drew: the recognition
    net's against R.recog_grad with the device's own codes gradient, the language model's against G.lm_grad on the kept codes.
    Every row within 8 x the float32 evaluation's worst per-row ratio of its own largest entry; zero reference rows +0.0."""
    import torch
    m, W, img, gt, lab, res, kept = run
    np_ = res["num_pos"]
    args = (W, kept["feat"], kept["roi_boxes"], np_, gt[res["pos_target_idx"]], res["codes"], H, WD)
    GB.assert_rows("loss_gradients recog", GB.RECOG_ROW_TENSORS, res, R.recog_grad(*args), R.recog_grad(*args, dtype=torch.float32))
    largs = (W, kept["codes"][:np_], lab[res["pos_target_idx"]])
    GB.assert_rows("loss_gradients lm", GB.LM_ROW_TENSORS, res, G.lm_grad(*largs), G.lm_grad(*largs, dtype=torch.float32))


def test_two_calls_give_identical_bits(run):
    m, W, img, gt, lab, res, kept = run
    again = m.loss_gradients(img, gt, lab, dump=True, **OPTS)
    for k in R.TENSORS + G.TENSORS:
        assert np.array_equal(_bits(again[k]), _bits(res[k])), k


def test_a_gradient_step_lowers_the_float64_loss_as_first_order_predicts(run):
    """W' = W - eta g on fc7 and the two heads, g the DEVICE's gradient; the float64 loss end_objectness + end_box_reg + captioning
    of the sampled rows drops by eta |g|^2 within 10 %.  eta is halved until the restatement itself, stepped along its own
    gradient, is first-order to 5 %."""
    import torch
    m, W, img, gt, lab, res, kept = run
    np_ = res["num_pos"]
    keys = ("fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b")
    rows_lab = lab[res["pos_target_idx"]]
    ref = R.recog_grad(W, kept["feat"], kept["roi_boxes"], np_, gt[res["pos_target_idx"]], res["codes"], H, WD)
    f, b = torch.tensor(kept["feat"].astype(np.float64)), torch.tensor(kept["roi_boxes"].astype(np.float64))
    t = torch.tensor(gt[res["pos_target_idx"]].astype(np.float64))
    PL = {k: torch.tensor(np.asarray(W[k], F32).astype(np.float64)) for k in G.PARAMS}

    def loss(grads, eta):
        with torch.no_grad():
            P = R._torch_params(W, torch.float64, requires_grad=False)
            for k in keys:
                P[k] = P[k] - eta * torch.tensor(np.asarray(grads[k], np.float64)).reshape(P[k].shape)
            out = R.forward(P, f, b, np_, t, None, H, WD)
            return float(out["total"]) + float(G.forward(PL, out["codes"][:np_], rows_lab, 1.0)[0])
    base = loss(ref, 0.0)
    assert base == pytest.approx(res["end_objectness_loss"] + res["end_box_reg_loss"] + res["captioning_loss"], rel=1e-5)
    g2 = sum(float((ref[k] ** 2).sum()) for k in keys)
    eta = 0.02 / np.sqrt(g2)
    for _ in range(12):
        drop = base - loss(ref, eta)
        if abs(drop - eta * g2) <= 0.05 * eta * g2:
            break
        eta *= 0.5
    assert drop > 0 and abs(drop - eta * g2) <= 0.05 * eta * g2
    dg2 = sum(float((res[k].astype(np.float64) ** 2).sum()) for k in keys)
    got = base - loss(res, eta)
    print("descent: eta %.3e, predicted drop %.6e, observed drop %.6e" % (eta, eta * dg2, got))
    assert got > 0 and abs(got - eta * dg2) <= 0.10 * eta * dg2


def test_model_loss_gradients_shapes_and_layouts(run):
    m, W, img, gt, lab, res, kept = run
    D, n, np_ = m.fc_dim, res["num_pos"] + res["num_neg"], res["num_pos"]
    shapes = dict(fc6_w=(D, 512 * 49), fc6_b=(D,), fc7_w=(D, D), fc7_b=(D,), obj_w=(1, D), obj_b=(1,), boxreg_w=(4, D), boxreg_b=(4,),
                  feat=(512,) + MAP, roi_boxes=(n, 4), codes=(np_, D))
    for k, s in shapes.items():
        assert res[k].shape == s and res[k].dtype == F32, k
    for k in G.PARAMS:
        assert res[k].shape == tuple(W[k].shape), k
    assert set(LR.LOSS_KEYS) | set(COUNTS) | set(LISTS) <= set(res)
    from densecap_amd import ops
    assert ops.feature_size(m.ctx, H, WD) == MAP and ops.feature_size(m.ctx, 600, 720) == (38, 45)


def test_the_loaded_weights_are_unchanged(run):
    m, W, img, gt, lab, res, kept = run
    before = m.forward_raw(img)
    m.loss_gradients(img, gt, lab, **OPTS)
    for x, y in zip(before, m.forward_raw(img)):
        assert np.array_equal(np.asarray(x), np.asarray(y))
