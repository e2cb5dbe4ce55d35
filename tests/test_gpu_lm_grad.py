"""dc_op_lm_grad (docs/SEMANTICS.md, "Language-model gradients") against the float64 autograd restatement
(tests/lm_grad_rules.py), through ops.lm_grad and the model's public methods.

Largest observed max|dev - ref64| / max|ref64| per tensor and case (MI355X; the bar is 1e-4), and the worst per-row ratio of the
2-D tensors beside the bar it was held to (tests/grad_bars.py): see DESIGN.md §16."""
import numpy as np
import pytest

from tests import grad_bars as GB
from tests import lm_grad_rules as G

pytestmark = pytest.mark.gpu

REL = 1e-4                     # tests/parity.py's continuous-stage bar
# (weights, n, L): the sets of tests/test_gpu_dims.py, and the default dimensions with a 200-word vocabulary
CASES = {"minimal_1x1": ("minimal", 1, 1), "minimal_3x1": ("minimal", 3, 1), "odd32_5x3": ("odd32", 5, 3),
         "e_lt_h_70x9": ("e_lt_h", 70, 9), "default_7x15": ("default", 7, 15)}
# The vocabularies and sizes of the product and of the op's limits.  "ckpt_vocab" is the checkpoint's V = 10,497 (V + 1 = 82 * 128
# + 2: the last tile of the lm_out_w gradient has two live columns, lda = V1pad = 10,560 > N, dH = dlogits . Wout is a split-K
# shape of 330 K tiles) at fc_dim = 256; big_vocab (V = 20,000) and e_gt_h (E > Hd) are tests/test_gpu_dims.py's sets; n = 1024
# and L = 64 are the largest the op admits (L is bounded by the op, not by the model's seq_length).  A fourth entry fixes the
# labels: "empty" (every caption empty: one projection step) or "full" (every caption full width).
NEW_CASES = {"ckpt_vocab_3x2": ("ckpt_vocab", 3, 2), "ckpt_vocab_70x9": ("ckpt_vocab", 70, 9), "big_vocab_5x4": ("big_vocab", 5, 4),
             "e_gt_h_5x5": ("e_gt_h", 5, 5), "minimal_1024x1": ("minimal", 1024, 1), "minimal_3x64": ("minimal", 3, 64),
             "odd32_4x3_empty": ("odd32", 4, 3, "empty"), "odd32_4x3_full": ("odd32", 4, 3, "full")}
CASES.update(NEW_CASES)
_models, _runs, _wcache = {}, {}, {}


def _weights(name):
    from densecap_amd.weights import make_synthetic_weights
    from tests.test_gpu_dims import set_weights
    if name not in _wcache:
        if name == "default":
            _wcache[name] = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
        elif name == "ckpt_vocab":
            _wcache[name] = make_synthetic_weights(seed=21, vocab_size=10497, seq_length=15, fc_dim=256)
        else:
            _wcache[name] = set_weights(name)
    return _wcache[name]


def case_inputs(case):
    """(W, codes, labels) of a case: from the weights' shapes alone, so that the CPU tests can form them too."""
    name, n, L = CASES[case][:3]
    W = _weights(name)
    D, V = int(W["lm_enc_w"].shape[1]), int(W["lm_out_w"].shape[0]) - 1
    rng = np.random.default_rng(100 + n * 64 + L)
    codes, lab = G.draw_codes(n, D, rng), G.draw_labels(n, L, V, rng)
    mode = CASES[case][3] if len(CASES[case]) > 3 else None
    if mode == "empty":
        lab[:] = 0
    elif mode == "full":
        lab = np.where(lab == 0, rng.integers(1, V + 1, lab.shape), lab).astype(np.int32)
    return W, codes, lab


def _model(name):
    """One model per weight set for the whole module."""
    if name not in _models:
        from densecap_amd import DenseCapModel
        W = _weights(name)
        _models[name] = (DenseCapModel(W, device=0), W)
    return _models[name]


def _run(case):
    """(model, W, codes, labels, device result, float64 reference) of a case, computed once."""
    if case not in _runs:
        m, W = _model(CASES[case][0])
        _, codes, lab = case_inputs(case)
        assert codes.shape[1] == m.fc_dim and lab.max(initial=0) <= m.vocab_size
        _runs[case] = (m, W, codes, lab, m.lm_gradients(codes, lab), G.lm_grad(W, codes, lab))
    return _runs[case]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m, _ in _models.values():
        m.ctx.close()
    _models.clear(); _runs.clear(); _wcache.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in G.TENSORS) and a["loss"] == b["loss"] and \
        np.array_equal(_bits(a["rowlik"]), _bits(b["rowlik"]))


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_the_float64_restatement(case):
    """Every tensor: max|dev - ref64| <= 1e-4 max|ref64|; the loss within 1e-6 relative."""
    m, W, codes, lab, dev, ref = _run(case)
    ratios = {k: float(np.abs(dev[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in G.TENSORS}
    print("lm_grad %s: " % case + ", ".join("%s %.2e" % kv for kv in ratios.items()) +
          ", loss %.2e" % (abs(dev["loss"] - ref["loss"]) / abs(ref["loss"])))
    for k in G.TENSORS:
        assert dev[k].shape == ref[k].shape and dev[k].dtype == np.float32, k
        assert ratios[k] <= REL, (k, ratios[k])
    assert abs(dev["loss"] - ref["loss"]) <= 1e-6 * abs(ref["loss"])


@pytest.mark.parametrize("case", list(CASES))
def test_every_row_matches_the_float64_restatement_at_the_float32_evaluations_bar(case):
    """The five 2-D tensors row by row (tests/grad_bars.py): every row within 8 x the float32 evaluation's worst per-row ratio of
    ITS OWN largest entry, and the rows whose reference is exactly zero all +0.0 bits."""
    import torch
    m, W, codes, lab, dev, ref = _run(case)
    GB.assert_rows("lm_grad " + case, GB.LM_ROW_TENSORS, dev, ref, G.lm_grad(W, codes, lab, dtype=torch.float32))


def _paired_scores(ctx, codes, lab, block=128):
    """lm_score of code i against caption i, in blocks (a row's number does not depend on the rows scored beside it)."""
    from densecap_amd import ops
    return np.concatenate([np.diag(ops.lm_score(ctx, codes[i:i + block], lab[i:i + block])) for i in range(0, len(codes), block)])


@pytest.mark.parametrize("case", list(CASES))
def test_rowlik_is_lm_scores_number_bit_for_bit(case):
    m, W, codes, lab, dev, ref = _run(case)
    want = _paired_scores(m.ctx, codes, lab).astype(np.float32)
    assert np.array_equal(_bits(dev["rowlik"].astype(np.float32)), _bits(want))
    assert dev["loss"] == pytest.approx(-dev["rowlik"].sum() / (lab.shape[0] * (lab.shape[1] + 2)), rel=1e-14)


@pytest.mark.parametrize("case", list(CASES))
def test_never_fed_embedding_rows_are_zero_and_two_calls_agree_bitwise(case):
    m, W, codes, lab, dev, ref = _run(case)
    fed = G.fed_rows(lab, m.vocab_size)
    rest = np.array(sorted(set(range(m.vocab_size + 2)) - set(fed)))
    assert m.vocab_size + 1 in rest and not _bits(dev["lm_emb"][rest]).any()       # +0.0, the NULL row included
    assert all(dev["lm_emb"][r].any() for r in fed)
    assert _same(dev, m.lm_gradients(codes, lab))


def test_weight_scales_the_gradients_and_codes_may_be_left_out():
    from densecap_amd import ops
    m, W, codes, lab, dev, ref = _run("odd32_5x3")
    half = ops.lm_grad(m.ctx, codes, lab, weight=0.5, want_codes=False)
    assert "codes" not in half and half["loss"] == 0.5 * dev["loss"]
    for k in G.PARAMS:                                                             # a power of two scales exactly
        assert np.array_equal(_bits(half[k]), _bits(dev[k] * np.float32(0.5))), k
    assert np.array_equal(half["rowlik"], dev["rowlik"])


def test_settings_do_not_change_the_result_and_survive_the_call():
    """Identical bits under dc_set_math_mode(1), dc_set_lanes(1) and dc_set_beam_size(3); forward_test under those settings gives
    the same outputs before and after a gradient call (and not the default settings' outputs: they were really in force)."""
    from densecap_amd.weights import make_synthetic_image
    m, W, codes, lab, dev, ref = _run("odd32_5x3")
    img = make_synthetic_image(224, 288, 2)
    plain = m.forward_raw(img)
    try:
        m.setMathMode(1); m.setLanes(1); m.setBeamSize(3)
        before = m.forward_raw(img)
        assert _same(dev, m.lm_gradients(codes, lab))
        after = m.forward_raw(img)
    finally:
        m.setMathMode(0); m.setLanes(3); m.setBeamSize(0)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert not all(np.array_equal(a, b) for a, b in zip(plain, before))
    for a, b in zip(plain, m.forward_raw(img)):                                    # and the weights are what they were
        assert np.array_equal(a, b)


def test_refusals_enqueue_nothing():
    import ctypes as C
    from densecap_amd import _lib, ops
    m, W, codes, lab, dev, ref = _run("minimal_3x1")
    V, D = m.vocab_size, m.fc_dim
    ok = lambda n, L: (np.zeros((n, D), np.float32), np.ones((n, L), np.int32))
    bad = [ok(1025, 1), ok(2, 65), (codes, np.full_like(lab, V + 1)), (codes, np.full_like(lab, -1))]
    two = np.zeros((3, 2), np.int32); two[0] = [0, 1]                              # a word after a zero
    bad.append((codes, two))
    for x, l in bad:
        with pytest.raises(_lib.DenseCapError, match=r"\(-"):
            ops.lm_grad(m.ctx, x, l)
    for w in (np.inf, -np.inf, np.nan):
        with pytest.raises(_lib.DenseCapError, match="finite"):
            ops.lm_grad(m.ctx, codes, lab, weight=w)
    # n = 0 and L = 0 straight through the ABI (the wrapper cannot shape them)
    g = _lib.DcLmGrads(**{k: 1 for k in G.TENSORS})
    loss = C.c_double()
    one = np.ones(1, np.int32)
    for n, L in ((0, 1), (1, 0)):
        assert m.lib.dc_op_lm_grad(m.ctx.h, 1, n, one.ctypes.data, L, 1.0, C.byref(g), C.byref(loss), None) == -1
    assert _same(dev, m.lm_gradients(codes, lab))                                  # the context is as it was


def test_a_gradient_step_lowers_the_loss_as_first_order_predicts():
    """e_lt_h, n = 70: W' = W - eta g on the seven tensors, a second model from W'; its loss drops by eta |g|^2 within 10 %.  eta is
    chosen so that the restatement's own second-order term stays below 5 % -- checked on the CPU first."""
    import torch
    from densecap_amd import DenseCapModel
    m, W, codes, lab, dev, ref = _run("e_lt_h_70x9")
    g2 = sum(float((ref[k] ** 2).sum()) for k in G.PARAMS)
    eta = 0.02 / np.sqrt(g2)

    def stepped(grads, e):
        W2 = dict(W)
        for k in G.PARAMS:
            W2[k] = (W[k].double() - e * torch.from_numpy(np.asarray(grads[k], np.float64))).float().reshape(W[k].shape)
        return W2

    for _ in range(8):                                   # halve eta until the restatement is first-order to 5 %
        drop = ref["loss"] - G.loss_only(stepped(ref, eta), codes, lab)
        if abs(drop - eta * g2) <= 0.05 * eta * g2:
            break
        eta *= 0.5
    assert abs(drop - eta * g2) <= 0.05 * eta * g2 and drop > 0
    m2 = DenseCapModel(stepped(dev, eta), device=0)
    try:
        loss2 = m2.lm_gradients(codes, lab)["loss"]
    finally:
        m2.ctx.close()
    dg2 = sum(float((dev[k].astype(np.float64) ** 2).sum()) for k in G.PARAMS)
    got = dev["loss"] - loss2
    print("descent: eta %.3e, predicted drop %.6e, device drop %.6e" % (eta, eta * dg2, got))
    assert got > 0 and abs(got - eta * dg2) <= 0.10 * eta * dg2


def test_caption_gradients_is_lm_gradients_on_the_boxes_codes():
    from densecap_amd.weights import make_synthetic_image
    m, W, codes, lab, dev, ref = _run("odd32_5x3")
    img = make_synthetic_image(224, 320, 4)
    boxes = np.array([[60, 50, 80, 60], [200, 120, 100, 90], [160, 112, 300, 200], [40, 180, 50, 40]], np.float32)
    labels = G.draw_labels(4, 3, m.vocab_size, np.random.default_rng(12))
    saved = m.opt["final_nms_thresh"]
    m.opt["final_nms_thresh"] = 0.0
    try:
        (_b, feats, src), = m.extractFeatures_boxes([img], [boxes])
    finally:
        m.opt["final_nms_thresh"] = saved
    assert list(src) == [0, 1, 2, 3]
    a, b = m.caption_gradients(img, boxes, labels), m.lm_gradients(feats, labels)
    assert _same(a, b) and a["codes"].shape == (4, m.fc_dim) and a["codes"].any()
    assert m.opt["final_nms_thresh"] == saved
