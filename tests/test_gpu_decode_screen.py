"""The screened greedy decode step (dc_debug_set "decode_screen" = 1: bf16 screen of the vocabulary + exact fp32 re-scoring of
the columns that can still win) against the fused fp32 step (0): the same tokens and the same LSTM state, bit
for bit -- on random codes, on ties and near-ties, on rows that must fall back to the exact scan, at other model dimensions,
and end to end.  The selection rule and its bound are restated in tests/decode_screen_rules.py.

A device-side row count below the launch's rows (n_dev) reaches the language model only through the packed survivor decode,
i.e. the captions-after-final-NMS order of the end-to-end test: 64 proposals are launched, the final NMS keeps fewer (asserted),
and the live rows' LSTM state is compared as well as the outputs.

The shipped default (-1) chooses the route per launch from its row count, from SCREEN_MIN_ROWS rows on; which route ran is read
back through dc_debug_fetch "decode_screen_routes".  A single-image forward at one lane cuts its rows into two parts on two
streams, and between 769 and 911 rows the first part is screened and the second is not: both run at once on one buffer.

The dimension sets come from tests/test_gpu_dims.py and tests/test_gpu_decode_screen_kernels.py (lds_last / lds_out: the last
vocabulary the row tail's LDS rule admits and the first it declines); that module tests the kernels underneath one at a time."""
import math

import numpy as np
import pytest
import torch

from tests import decode_screen_rules as R

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 129, 300)
SCREEN_MIN_ROWS = 400           # kScreenMinRows of densecap.hip: the rule of decode_screen = -1


def _routes(m):
    """(parts, mask of the screened ones) of the greedy decode enqueued last."""
    return tuple(int(x) for x in m.debug_fetch("decode_screen_routes", (2,), np.int32)[0])


def _lm_state(m, rows):
    Hd = m._test_W["lstm_w"].shape[1] // 4
    return [m.debug_fetch(k, (rows, Hd))[0].view(np.uint32) for k in ("lm_h", "lm_c")]


def _set(m, name, v):
    from densecap_amd._lib import check
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, name.encode(), int(v)), "dc_debug_set(%s)" % name)


def _decode(m, codes, route):
    """dc_op_lm_sample on the route: tokens (n, T), final h and c (n, Hd) as uint32 bit patterns."""
    from tests.test_gpu_sample import _greedy
    _set(m, "decode_screen", route); _set(m, "lm_op_keep", 1)
    try:
        tok = _greedy(m, np.ascontiguousarray(codes, np.float32))
        Hd = m._test_W["lstm_w"].shape[1] // 4
        h = m.debug_fetch("lm_op_h", (len(codes), Hd))[0].view(np.uint32)
        c = m.debug_fetch("lm_op_c", (len(codes), Hd))[0].view(np.uint32)
    finally:
        _set(m, "decode_screen", -1); _set(m, "lm_op_keep", 0)
    return tok, h, c


def _kept(m, n):
    """What the screened dc_op_lm_sample just kept: candidate counts (n, T), last step's scores (n, V1) fp16, winners' logits."""
    T, V1 = m.seq_length, m.vocab_size + 1
    V1pad = (V1 + 63) // 64 * 64
    cand = m.debug_fetch("lm_op_cand", (n, T), np.int32)[0]
    sc = m.debug_fetch("lm_op_scores", (n, V1pad), np.float16)[0][:, :V1]
    best = m.debug_fetch("lm_op_best", (n,))[0]
    return cand, sc, best


def _same(m, codes, what=""):
    t0, h0, c0 = _decode(m, codes, 0)
    t1, h1, c1 = _decode(m, codes, 1)
    np.testing.assert_array_equal(t1, t0, err_msg=what)
    np.testing.assert_array_equal(h1, h0, err_msg=what)
    np.testing.assert_array_equal(c1, c0, err_msg=what)
    return t1


def _codes(n, D, seed):
    return np.maximum(np.random.default_rng(seed).standard_normal((n, D)), 0).astype(np.float32)


def _model(W):
    from densecap_amd import DenseCapModel
    m = DenseCapModel(W, device=0)
    m._test_W = W
    return m


@pytest.fixture(scope="module")
def weights():
    from densecap_amd.weights import make_synthetic_weights
    return make_synthetic_weights(seed=1234)


@pytest.fixture(scope="module")
def model(weights):
    m = _model(weights)
    yield m
    m.ctx.close()


# ---- token and state identity ------------------------------------------------------------------------------------------------
def test_tokens_and_state_identical_at_row_counts(model):
    codes = _codes(max(ROW_COUNTS), 4096, 21)
    for n in ROW_COUNTS:
        tok = _same(model, codes[:n], "rows=%d" % n)
        cand = _kept(model, n)[0]
        assert tok.min() >= 1 and cand.min() >= 1 and cand.max() <= R.MAX_CAND, (n, cand.min(), cand.max())


@pytest.mark.parametrize("name", ["e_gt_h", "odd32"])
def test_tokens_and_state_identical_at_other_dimensions(name):
    """e_gt_h: V + 1 = 1501 is no multiple of 64 (nor of the screen's 128-column tile), Hd = 256; odd32: Hd = 1056, an odd
    multiple of 32 (the bf16 rows are padded to 1088), V + 1 = 71 inside one tile, three passes of the LSTM row tail."""
    from tests.test_gpu_dims import SETS, set_weights
    W = set_weights(name)
    m = _model(W)
    try:
        codes = _codes(129, SETS[name]["D"], 4)
        for n in (1, 65, 129):
            _same(m, codes[:n], "%s rows=%d" % (name, n))
    finally:
        m.ctx.close()


def _set_model(name):
    """(model, fc_dim) of a set of tests/test_gpu_decode_screen_kernels.py: the five of test_gpu_dims.py, lds_last, lds_out."""
    from tests.test_gpu_decode_screen_kernels import screen_set_weights
    W = screen_set_weights(name)
    return _model(W), W["lm_enc_w"].shape[1]


@pytest.mark.parametrize("name,rows", [("minimal", (1, 129)), ("e_lt_h", (1, 129)), ("big_vocab", (1, 129)), ("lds_last", (1, 129)),
                                       ("e_gt_h", (1025,))])
def test_tokens_and_state_identical_on_every_dimension_set(name, rows):
    """The sets the route had never run at: minimal (Kp = 64: one K step of the screen, V + 1 = 6), e_lt_h (Hd = 768: twelve
    K steps, two tail passes), big_vocab (five outer rounds of the tail's first pass, 40 KB of upper ends in LDS), lds_last (the
    largest vocabulary the row tail's LDS rule admits at Hd = 512: 64 KiB of dynamic LDS beside the kernel's static LDS) -- and
    e_gt_h at 1025 rows: nine row tiles, two per XCD with seven slots empty."""
    m, D = _set_model(name)
    try:
        codes = _codes(max(rows), D, 4)
        for n in rows:
            _same(m, codes[:n], "%s rows=%d" % (name, n))
            assert _routes(m) == (1, 1), (name, n, _routes(m))
            cand = _kept(m, n)[0]
            assert cand.min() >= 1, (name, n, cand.min())
    finally:
        m.ctx.close()


def test_route_declined_past_the_lds_rule():
    """lds_out: one more 64-column group of vocabulary than lds_last and the row tail's LDS no longer fits.  The loader admits
    the model, so nothing may fail later: decode_screen = 1 and the default rule at 400 rows both decode on the fused step."""
    m, D = _set_model("lds_out")
    try:
        codes = _codes(SCREEN_MIN_ROWS, D, 4)
        t0 = _decode(m, codes[:65], 0)
        t1 = _decode(m, codes[:65], 1)
        assert _routes(m) == (1, 0)
        for x, y in zip(t1, t0):
            np.testing.assert_array_equal(x, y)
        tok = _decode(m, codes, -1)[0]
        assert _routes(m) == (1, 0)
        assert tok.shape == (SCREEN_MIN_ROWS, m.seq_length) and tok.min() >= 1
    finally:
        m.ctx.close()


def test_default_rule_by_row_count(model):
    """decode_screen = -1: 399 rows take the fused step, 400 the screened one; the same tokens and state as route 0 at both."""
    codes = _codes(SCREEN_MIN_ROWS, 4096, 5)
    for n, screened in ((SCREEN_MIN_ROWS - 1, 0), (SCREEN_MIN_ROWS, 1)):
        t0, h0, c0 = _decode(model, codes[:n], 0)
        assert _routes(model) == (1, 0)
        t, h, c = _decode(model, codes[:n], -1)
        assert _routes(model) == (1, screened), (n, _routes(model))
        np.testing.assert_array_equal(t, t0)
        np.testing.assert_array_equal(h, h0)
        np.testing.assert_array_equal(c, c0)


def test_default_rule_mixed_routes_on_two_streams(model):
    """800 proposals at one lane: parts of 512 rows (screened under -1) and 288 rows (fused) advance at the same time on two
    streams and share the lane's buffers.  Outputs and the LSTM state of every live row against route 0, bit for bit."""
    from densecap_amd.weights import make_synthetic_image
    P = 800
    img = np.ascontiguousarray(make_synthetic_image(480, 640, 11), np.float32)
    model.setTestArgs(rpn_nms_thresh=0.9, final_nms_thresh=0.3, num_proposals=P)
    model.setLanes(1)
    try:
        got = {}
        for route in (0, -1):
            _set(model, "decode_screen", route)
            outs = model.forward_raw(img)
            got[route] = (outs, _lm_state(model, P), _routes(model))
        live = int(model.debug_fetch("rpn_nms_count", (1,), np.int32)[0][0])
        print("live rows %d of %d, routes %s" % (live, P, got[-1][2]))
        assert live > 512 + 64, "the second part has too few live rows: the case tests little"
        assert got[0][2] == (2, 0b00) and got[-1][2] == (2, 0b01), (got[0][2], got[-1][2])
        assert len(got[0][0][0]) > 0
        for x, y in zip(got[-1][0], got[0][0]):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(got[-1][1], got[0][1]):
            np.testing.assert_array_equal(x[:live], y[:live])
    finally:
        model.setLanes(3); model.setTestArgs()
        _set(model, "decode_screen", -1)


# ---- ties and near-ties ------------------------------------------------------------------------------------------------------
def test_ties_and_one_ulp_biases(weights, model):
    """The words the rows choose get a duplicate -- the same weight row and bias at a HIGHER and at a LOWER index (the lower one
    must win, at every step it comes up) -- and other chosen words a twin whose bias is one ulp above / below."""
    codes = _codes(130, 4096, 8)
    base = _decode(model, codes, 0)[0]
    words = [int(w) - 1 for w in np.unique(base[:, 0])][:40]             # columns some row chooses at the first step
    W = dict(weights)
    ow, ob = weights["lm_out_w"].clone(), weights["lm_out_b"].clone()
    V1 = ow.shape[0]
    free = [j for j in range(V1 - 1) if j not in set(words)]
    twins = [free[i] if i % 2 else free[-1 - i] for i in range(len(words))]     # distinct; low and high indices
    for i, (col, twin) in enumerate(zip(words, twins)):
        ow[twin] = ow[col]
        kind = i % 4
        ob[twin] = ob[col] if kind < 2 else torch.nextafter(ob[col], torch.tensor(math.inf if kind == 2 else -math.inf))
    W["lm_out_w"], W["lm_out_b"] = ow, ob
    m = _model(W)
    try:
        tok = _same(m, codes, "duplicated rows / one-ulp biases")
        dup = {}
        for i, (col, twin) in enumerate(zip(words, twins)):
            if i % 4 < 2:
                dup[max(col, twin) + 1] = min(col, twin) + 1
        assert not np.isin(tok, list(dup)).any(), "the higher index of a tied pair was chosen"
        assert np.isin(tok, list(dup.values())).any(), "no tied pair came up: the case tests nothing"
    finally:
        m.ctx.close()


# ---- fallback ----------------------------------------------------------------------------------------------------------------
def test_fallback_all_equal_columns(weights):
    """Every column the same weight row and bias: every column is a candidate at every step, every row scans exactly, word 1."""
    W = dict(weights)
    W["lm_out_w"] = weights["lm_out_w"][:1].repeat(weights["lm_out_w"].shape[0], 1)
    W["lm_out_b"] = torch.full_like(weights["lm_out_b"], 0.125)
    m = _model(W)
    try:
        codes = _codes(65, 4096, 2)
        tok = _same(m, codes, "all-equal columns")
        cand = _kept(m, 65)[0]
        assert (tok == 1).all() and (cand == W["lm_out_w"].shape[0]).all()
    finally:
        m.ctx.close()


def test_fallback_non_finite_rows(model):
    """An Inf among a row's codes makes its state and every score NaN (docs/SEMANTICS.md): those rows, and only those, take the
    exact scan (candidate count -1) at every step and have no word; every other row is as without them."""
    codes = _codes(70, 4096, 6)
    bad = [0, 33, 64, 69]
    for r in bad:
        codes[r, 5 + r] = np.inf
    tok = _same(model, codes, "non-finite rows")
    cand = _kept(model, 70)[0]
    fell = (cand < 0) | (cand > R.MAX_CAND)
    assert fell[bad].all() and not np.delete(fell, bad, axis=0).any()
    assert (tok[bad] == 0).all() and (np.delete(tok, bad, axis=0) >= 1).all()
    clean = np.delete(codes, bad, axis=0)
    np.testing.assert_array_equal(np.delete(tok, bad, axis=0), _decode(model, clean, 1)[0])


# ---- the bound on the device -------------------------------------------------------------------------------------------------
def test_bound_and_rescored_value_on_the_device(weights, model):
    """The last step's stored scores against the full fp32 logits of the same h (dc_op_linear: the fp32 MFMA family, whose K
    order the re-scoring restates): |s - z| <= b everywhere, and the re-scored winner's logit IS the GEMM's row maximum."""
    from densecap_amd import ops
    n = 129
    codes = _codes(n, 4096, 13)
    tok, h, _ = _decode(model, codes, 1)
    cand, sc, best = _kept(model, n)
    h = h.view(np.float32)
    z = ops.linear(model.ctx, h, weights["lm_out_w"].numpy(), weights["lm_out_b"].numpy())
    s = torch.from_numpy(sc.astype(np.float32))
    ht = torch.from_numpy(h.copy())
    b = R.bounds(s, R.h_norms_up(ht), R.row_norms_up(weights["lm_out_w"]), R.bound_c(h.shape[1]))
    ratio = (np.abs(sc.astype(np.float64) - z.astype(np.float64)) / b.double().numpy()).max()
    print("max |s - z| / b on the device: %.4f; candidates of the last step: mean %.2f max %d" % (ratio, cand[:, -1].mean(), cand[:, -1].max()))
    assert ratio <= 1.0
    np.testing.assert_array_equal(best.view(np.uint32), z.max(1).view(np.uint32))
    np.testing.assert_array_equal(tok[:, -1], z.argmax(1) + 1)


def test_subnormal_logits(weights):
    """Wout scaled by 2^-120, no bias: products and partial sums of the fp32 chain are subnormal, the fp16 scores are all zero,
    so every row scans every column exactly -- the scalar fmaf chain of the re-scoring against the MFMA chain of the fused step
    (tokens) and of the full-logits GEMM (the winner's value, bit for bit)."""
    from densecap_amd import ops
    W = dict(weights)
    W["lm_out_w"] = weights["lm_out_w"] * 2.0 ** -120
    W["lm_out_b"] = torch.zeros_like(weights["lm_out_b"])
    m = _model(W)
    try:
        n = 65
        codes = _codes(n, 4096, 17)
        tok = _same(m, codes, "subnormal logits")
        _, h, _ = _decode(m, codes, 1)
        cand, _, best = _kept(m, n)
        assert (cand == W["lm_out_w"].shape[0]).all()
        z = ops.linear(m.ctx, h.view(np.float32), W["lm_out_w"].numpy(), None)
        assert (np.abs(z) < 2.0 ** -126).any() and (z != 0).any()
        np.testing.assert_array_equal(best.view(np.uint32), z.max(1).view(np.uint32))
        np.testing.assert_array_equal(tok[:, -1], z.argmax(1) + 1)
    finally:
        m.ctx.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 1], ids=["lanes2", "lanes1"])
@pytest.mark.parametrize("order", [False, True], ids=["reference_order", "captions_after_nms"])
def test_forward_identical(model, order, lanes):
    from densecap_amd.weights import make_synthetic_image
    img = np.ascontiguousarray(make_synthetic_image(240, 320, 7), np.float32)
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=64)
    model.setLanes(lanes); model.setCaptionOrder(order)
    try:
        outs, state = {}, {}
        for route in (0, 1):
            _set(model, "decode_screen", route)
            outs[route] = model.forward_raw(img)
            state[route] = _lm_state(model, 64)
            if route == 1:
                cand = model.debug_fetch("decode_screen_cand", (64, model.seq_length), np.int32)[0]
                live = len(outs[1][0]) if order else int(model.debug_fetch("rpn_nms_count", (1,), np.int32)[0][0])
                assert (cand[:live] >= 1).all() and (cand[:live] <= R.MAX_CAND).all()
                if order:                                # the device-side row count is below the 64 rows of the launch
                    assert 0 < live < 64, live
                for x, y in zip(state[1], state[0]):     # row = RoI (reference order) or final rank (captions after NMS)
                    np.testing.assert_array_equal(x[:live], y[:live])
        assert len(outs[0][0]) > 0
        for x, y in zip(outs[1], outs[0]):
            np.testing.assert_array_equal(x, y)
        if lanes == 2 and not order:                     # once graph-replayed: captured, then relaunched
            model.setGraphReplay(True)
            for _ in range(3):
                for x, y in zip(model.forward_raw(img), outs[0]):
                    np.testing.assert_array_equal(x, y)
            assert model.debug_fetch("graph_launches", (1,), np.int32)[0][0] >= 1
    finally:
        model.setGraphReplay(False); model.setLanes(3); model.setCaptionOrder(False); model.setTestArgs()
        _set(model, "decode_screen", -1)


def test_packed_survivor_decode_on_the_xcd_map(model):
    """A group of four images at 300 proposals, captions after the final NMS: ONE decode launch of 1200 rows (ten row tiles, two
    per XCD, six slots empty) with a device-side row count below that.  The default rule screens it; outputs of every image and
    the LSTM state of the live rows of the first 300 against route 0, bit for bit.
    (Last in the module: a lane keeps its group capacity for an image size, and "decode_screen_cand" is sized by it.)"""
    from densecap_amd.weights import make_synthetic_image
    P, G = 300, 4
    imgs = np.stack([np.ascontiguousarray(make_synthetic_image(240, 320, 30 + i), np.float32) for i in range(G)])
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.5, num_proposals=P)
    model.setLanes(2); model.setGroup(G); model.setCaptionOrder(True)
    try:
        got = {}
        for route in (0, -1):
            _set(model, "decode_screen", route)
            outs = model.forward_batch(imgs)
            surv = int(model.debug_fetch("survivor_rows", (1,), np.int32)[0][0])
            got[route] = (outs, _lm_state(model, P), _routes(model), surv)
        surv = got[0][3]
        print("survivor rows %d of %d launched, routes %s" % (surv, G * P, got[-1][2]))
        assert got[-1][3] == surv and 128 < surv < G * P, surv
        assert got[0][2] == (1, 0) and got[-1][2] == (1, 1), (got[0][2], got[-1][2])
        assert len(got[0][0]) == G and sum(len(o[0]) for o in got[0][0]) == surv
        for a, b in zip(got[-1][0], got[0][0]):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        live = min(P, surv)
        for x, y in zip(got[-1][1], got[0][1]):
            np.testing.assert_array_equal(x[:live], y[:live])
    finally:
        model.setLanes(3); model.setGroup(0); model.setCaptionOrder(False); model.setTestArgs()
        _set(model, "decode_screen", -1)
