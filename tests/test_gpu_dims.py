"""The GPU path at model dimensions other than the defaults (docs/SEMANTICS.md, "Supported model dimensions").

dc_load_weights admits a family of architectures -- num_anchors >= 1, rpn_hidden, enc_size, rnn_size multiples of 32, fc_dim a
multiple of 256, any vocabulary and sequence length -- and every other GPU module runs one point of it (R = 256, E = Hd = 512,
D = 4096, k = 12 with the default anchor table).  Here five other points go through every entry point against the CPU oracle
and the CPU restatements, with the rules and constants of the modules that test the default point (imported, not copied):

  minimal    the smallest model the loader admits; T = 1 (the first step is the last), N = 6k = 6, END is frequent
  e_lt_h     E < Hd; Hd = 768: two passes of the LSTM row tail, the second half full
  e_gt_h     E > Hd; R = 512; twelve anchors of other sizes than the default table (the values come from the weights)
  odd32      every K an odd multiple of 32 (R = 96, E = 544, Hd = 1056, D = 768): three tail passes, the last with 32 units
  big_vocab  V = 20000: an 80 KB LDS row in the beam top-k kernel, V1pad and the log-sum-exp slot count far from the others

A set the loader admits must never fail later: every call below goes through _lib.check, which raises on any code but DC_OK."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT = np.array([[45, 90], [90, 45], [64, 64], [90, 180], [180, 90], [128, 128], [181, 362], [362, 181], [256, 256],
                    [362, 724], [724, 362], [512, 512]], np.float32).T.copy()
# e_gt_h: twelve anchors, none of them a size of the default table (what `anchor_scale` = 0.6 makes of it, plus a pixel)
OTHER12 = (DEFAULT * np.float32(0.6) + np.float32(1)).astype(np.float32)
EXTRA3 = np.array([[32, 32], [48, 96], [96, 48]], np.float32).T
SETS = {
    #            R        E        Hd        D        V        T     anchors (2, k)                               beam
    "minimal": dict(R=32, E=32, Hd=32, D=256, V=5, T=1, anchors=np.array([[96], [80]], np.float32), beam=2),
    "e_lt_h": dict(R=128, E=256, Hd=768, D=512, V=777, T=9, anchors=DEFAULT[:, :9].copy(), beam=3),
    "e_gt_h": dict(R=512, E=768, Hd=256, D=1024, V=1500, T=5, anchors=OTHER12, beam=3),
    "odd32": dict(R=96, E=544, Hd=1056, D=768, V=70, T=3, anchors=DEFAULT[:, [0, 2, 3, 5, 8]].copy(), beam=3),
    "big_vocab": dict(R=256, E=512, Hd=512, D=256, V=20000, T=4, anchors=np.concatenate([DEFAULT, EXTRA3], 1), beam=3),
}
IDS = list(SETS)
BIG_IMAGE_SET = "odd32"            # the one set that also runs 600x720 / 300 proposals
ENTRY_POINT_SET = "odd32"          # the one set of (g)
GREEDY_EXCUSED_CAP = 6             # 2 % of 300 rows
BEAM_EXCUSED_CAP = 7               # 10 % of 70 rows
SAMPLE_ROWS = 300                  # regions of (d), as in test_gpu_sample.py


def set_weights(name):
    from densecap_amd.weights import make_synthetic_weights
    s = SETS[name]
    return make_synthetic_weights(seed=11, vocab_size=s["V"], seq_length=s["T"], rpn_hidden=s["R"], enc_size=s["E"],
                                  rnn_size=s["Hd"], fc_dim=s["D"], anchors=s["anchors"])


@pytest.fixture(scope="module", params=IDS)
def dims(request):
    """(model, weights, spec, name) of one set: one module-scoped model per set."""
    from densecap_amd import DenseCapModel
    W = set_weights(request.param)
    m = DenseCapModel(W, device=0)
    s = SETS[request.param]
    assert (m.num_anchors, m.fc_dim, m.vocab_size, m.seq_length) == (s["anchors"].shape[1], s["D"], s["V"], s["T"])
    yield m, W, s, request.param
    m.ctx.close()


@pytest.fixture
def knobs(dims):
    """The set's model with the scheduling knobs back at their defaults after the test."""
    yield dims
    m = dims[0]
    m.setGraphReplay(False); m.setBeamSize(0); m.setCaptionOrder(False); m.setLanes(3); m.setGroup(0); m.setMathMode(0)
    m.setTestArgs()


def _greedy(m, codes):
    from tests.test_gpu_sample import _greedy as greedy
    return greedy(m, np.ascontiguousarray(codes, np.float32))


def _oracle_codes(n, D, seed):
    return np.maximum(np.random.default_rng(seed).standard_normal((n, D)), 0).astype(np.float32)


# ---- a. the forward against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 1], ids=["lanes2", "lanes1"])
@pytest.mark.parametrize("order", [False, True], ids=["reference_order", "captions_after_nms"])
def test_forward_matches_the_oracle(knobs, order, lanes):
    """parity.strict_check at 224x288 / 100 proposals in both caption orders, with two lanes and in single-image mode (stream-K
    and tail plans)."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    m, W, s, name = knobs
    m.setLanes(lanes); m.setCaptionOrder(order)
    r = parity.strict_check(m, W, make_synthetic_image(224, 288, 3), 100)
    print(name, {k: v for k, v in r.items() if not isinstance(v, list)})
    assert r["K"] > 0 and r["matched"] == r["K_oracle"]


@pytest.mark.parametrize("lanes", [2, 1], ids=["lanes2", "lanes1"])
def test_forward_matches_the_oracle_600x720_300_proposals(lanes):
    """One set (odd32) at 600x720 / 300 proposals."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    W = set_weights(BIG_IMAGE_SET)
    m = DenseCapModel(W, device=0)
    try:
        m.setLanes(lanes)
        r = parity.strict_check(m, W, make_synthetic_image(600, 720, 0), 300)
        print({k: v for k, v in r.items() if not isinstance(v, list)})
        assert r["K"] > 0 and r["matched"] == r["K_oracle"]
    finally:
        m.ctx.close()


# ---- b. greedy decode, teacher-forced on the oracle's codes ------------------------------------------------------------------
def _greedy_rows_against_the_oracle(m, W, s, codes):
    """The rule of test_gpu_e2e.py::test_lm_sample_teacher_forced: identical token rows, or the oracle's own top-2 logit margin
    at the first differing step is below 1e-4 relative to max(1, |top|).  Returns (device rows, oracle rows, rows excused)."""
    import torch
    from oracle import densecap_oracle as O
    oseq, logits = O.lm_sample(torch.from_numpy(codes), W, s["T"], return_logits=True)
    seq = _greedy(m, codes)
    assert seq.shape == oseq.shape == (len(codes), s["T"])
    bad_rows = np.nonzero((seq != oseq).any(axis=1))[0]
    for r in bad_rows:
        t = int(np.nonzero(seq[r] != oseq[r])[0][0])
        top2 = torch.topk(logits[t][r], 2).values
        margin = float(top2[0] - top2[1]) / max(1.0, float(top2[0].abs()))
        assert margin < 1e-4, "row %d step %d diverged with margin %g (device %s, oracle %s)" % (r, t, margin, seq[r], oseq[r])
    assert seq.min() >= 1 and seq.max() <= s["V"] + 1
    return seq, oseq, len(bad_rows)


def test_greedy_decode_teacher_forced(knobs):
    """dc_op_lm_sample on 300 oracle codes, and on 1, 63, 64 and 65 rows.  At most 2 % of the rows may be excused by a near-tie:
    on the oracle alone 0 / 2 / 0 / 0 / 4 of the 300 rows of the five sets (rows 57, 79 of e_lt_h; 47, 79, 100, 261 of
    big_vocab) have a top-2 margin below 1e-4 at ANY step, so the inputs stay inside the cap without the device's help -- and at
    most one of the first 65 rows does.  The oracle has END in 23 of the 300 rows of `minimal`.  (Counted on the CPU with these
    seeds; recount before changing one.)"""
    from tests import parity
    m, W, s, name = knobs
    parity.oracle_threads()
    codes = _oracle_codes(300, s["D"], 0)
    seq, oseq, excused = _greedy_rows_against_the_oracle(m, W, s, codes)
    print("%s: greedy decode excused %d of 300 rows" % (name, excused))
    assert excused <= GREEDY_EXCUSED_CAP
    if name == "minimal":
        assert (seq == s["V"] + 1).any(), "END never occurs (the oracle has it in 23 of 300 rows)"
        assert (oseq == s["V"] + 1).any()
    for n in (1, 63, 64, 65):
        _, _, ex = _greedy_rows_against_the_oracle(m, W, s, codes[:n])
        assert ex <= (0 if n == 1 else 1)


# ---- c. the LSTM state as numbers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 1], ids=["lanes2", "lanes1"])
def test_lstm_state_matches_the_oracle(knobs, lanes):
    """After a forward in the reference caption order: lm_enc, lm_h, lm_c of the RoI rows against the oracle's encoder output
    and final state on the device's own codes -- the rows whose tokens are identical (at least 90 % of them), within parity.REL."""
    import torch
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    from tests import parity
    m, W, s, name = knobs
    parity.oracle_threads()
    P = 100
    m.setLanes(lanes); m.setCaptionOrder(False)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    out = m.forward_raw(make_synthetic_image(224, 288, 3))
    assert len(out[0]) > 0
    B = int(m.debug_fetch("rpn_nms_count", (1,), np.int32)[0][0])
    assert 0 < B <= P
    codes = m.debug_fetch("codes", (P, s["D"]))[0][:B]
    seq = m.debug_fetch("seq", (P, s["T"]), np.int32)[0][:B]
    oseq, state = O.lm_sample(torch.from_numpy(np.ascontiguousarray(codes)), W, s["T"], return_state=True)
    same = (seq == oseq).all(axis=1)
    print("%s lanes=%d: %d of %d rows have identical tokens" % (name, lanes, int(same.sum()), B))
    assert same.sum() >= 0.9 * B
    for buf, width, key in (("lm_enc", s["E"], "enc"), ("lm_h", s["Hd"], "h"), ("lm_c", s["Hd"], "c")):
        dev = m.debug_fetch(buf, (P, width))[0][:B]
        err = parity.rel_err(dev[same], state[key][same])
        print("%s lanes=%d: %s relative error %.3g" % (name, lanes, buf, err))
        assert err <= parity.REL, "%s: relative error %.3g" % (buf, err)


# ---- d. scorer and sampler ---------------------------------------------------------------------------------------------------
def _queries(V, T, rng, n=40):
    """The pattern of test_gpu_score.py::_queries sized to this V and T: lengths 0..T, the ids 1 and V, repeated words."""
    q = np.zeros((n, T), np.int32)
    for i in range(n):
        L = i % (T + 1)
        q[i, :L] = rng.integers(1, V + 1, L)
    w = min(7, V)
    for row, words in ((1, [1]), (2, [V, V]), (3, [1, V, 1]), (4, [w, w, w, w])):
        q[row] = 0
        q[row, :min(T, len(words))] = words[:T]
    return q


def test_scorer_matches_restatement(knobs):
    from densecap_amd import ops
    from tests import score_restatement
    from tests.test_gpu_score import _codes
    m, W, s, name = knobs
    assert 1 <= s["T"] <= 64
    q = _queries(s["V"], s["T"], np.random.default_rng(0))
    codes = _codes(300, s["D"], 1)
    got = ops.lm_score(m.ctx, codes, q)
    ref = score_restatement.lm_score(codes, W, q)
    assert got.shape == (300, len(q)) and np.isfinite(got).all()
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
    print("%s: scorer max relative error %.3g" % (name, rel.max()))
    assert rel.max() < 1e-4, rel.max()


def test_sampler_matches_restatement_and_the_scorer(knobs):
    """test_gpu_sample.py::test_words_and_logprob_match_restatement at temperature 1.0 with that file's rule and constants."""
    from densecap_amd import ops
    from tests import sample_restatement as R
    from tests.test_gpu_sample import NOISE, STAGE, _codes, _decisions
    m, W, s, name = knobs
    end, T, n = s["V"] + 1, s["T"], SAMPLE_ROWS
    codes = _codes(n, s["D"], 1)
    dev, lp = ops.lm_sample_n(m.ctx, codes, 8, temperature=1.0, seed=7)
    assert dev.shape == (n, 8, T) and lp.shape == (n, 8)
    ref = R.lm_sample_n(codes, W, 8, temperature=1.0, seed=7, forced=dev)
    margin = 2 * (STAGE / 1.0 + NOISE)
    total, needed = _decisions(dev, ref, margin, end)
    print("%s: %d of %d decisions needed the margin %.3g" % (name, needed, total, margin))
    assert needed <= 0.01 * total
    np.testing.assert_array_equal(ref["samples"], dev)
    rel = np.abs(lp - ref["logprob"]) / np.maximum(np.abs(ref["logprob"]), 1e-3)
    print("%s: max relative error of logprob %.3g" % (name, rel.max()))
    assert rel.max() < 1e-4, rel.max()
    # every draw that contains END: logprob IS the scorer's number for that caption on that region
    rows = [(i, d) for i in range(n) for d in range(8) if (dev[i, d] == end).any()]
    print("%s: %d of %d draws contain END" % (name, len(rows), n * 8))
    if name == "minimal":
        assert len(rows) >= 1
    if rows:
        q = np.zeros((len(rows), T), np.int32)
        for k, (i, d) in enumerate(rows):
            q[k] = np.where(dev[i, d] == end, 0, dev[i, d])
        ll = ops.lm_score(m.ctx, codes, q)
        np.testing.assert_array_equal(lp[[i for i, _ in rows], [d for _, d in rows]], ll[[i for i, _ in rows], np.arange(len(rows))])


# ---- e. beam search ----------------------------------------------------------------------------------------------------------
def test_beamsearch_teacher_forced(knobs):
    """The rule of test_gpu_e2e.py::test_beamsearch_teacher_forced at beam 3 (minimal: 2, V + 1 = 6) on 70 oracle codes with the
    chunk loop walked: identical rows, or the oracle's own selection margin is below 1e-4.  At most 10 % of the rows may be
    excused: on the oracle alone 0 / 6 / 0 / 2 / 2 of the 70 rows of the five sets have such a margin (counted on the CPU with
    these seeds).  big_vocab is the set whose top-k row (80 KB) needs the raised dynamic-LDS limit."""
    import torch
    from densecap_amd._lib import check
    from oracle import densecap_oracle as O
    from tests import parity
    m, W, s, name = knobs
    parity.oracle_threads()
    beam, n, T = s["beam"], 70, s["T"]
    ctx = m.ctx
    check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"beam_chunk_floats", 1), "dc_debug_set")
    codes = _oracle_codes(n, s["D"], 0)
    oseq, margins = O.lm_beamsearch(torch.from_numpy(codes), W, T, beam, return_margins=True)
    print("%s: the oracle alone has %d of %d rows with a margin below 1e-4" % (name, int((margins < 1e-4).sum()), n))
    m.setBeamSize(beam)
    seq = _greedy(m, codes)
    bad = np.nonzero((seq != oseq).any(axis=1))[0]
    for r in bad:
        assert margins[r] < 1e-4, "row %d differs (hip %s oracle %s) with oracle margin %g" % (r, seq[r], oseq[r], margins[r])
    print("%s: beam %d excused %d of %d rows" % (name, beam, len(bad), n))
    assert len(bad) <= BEAM_EXCUSED_CAP
    assert seq.min() >= 1 and seq.max() <= s["V"] + 1


def test_beam_is_refused_on_the_host_for_a_vocabulary_beyond_the_lds_row():
    """V + 1 = 45001 floats do not fit the top-k kernel's LDS row: dc_set_beam_size answers on the host, from the device's
    attribute, before anything is launched -- and the greedy decode of that model still works afterwards."""
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import DenseCapError
    from densecap_amd.weights import make_synthetic_weights
    s = dict(SETS["minimal"], V=45000, T=2)
    W = make_synthetic_weights(seed=11, vocab_size=s["V"], seq_length=s["T"], rpn_hidden=s["R"], enc_size=s["E"],
                               rnn_size=s["Hd"], fc_dim=s["D"], anchors=s["anchors"])
    m = DenseCapModel(W, device=0)
    try:
        m.mfma_profile(reset=1)                               # count the contraction launches from here on
        before = m.mfma_profile()["launches"]
        with pytest.raises(DenseCapError) as e:
            m.setBeamSize(2)
        assert "(-5)" in str(e.value) and "does not fit the top-k kernel's LDS row" in str(e.value)   # DC_E_UNSUPPORTED
        assert before == 0 and m.mfma_profile()["launches"] == before, "the refusal launched a contraction"
        _, _, excused = _greedy_rows_against_the_oracle(m, W, s, _oracle_codes(64, s["D"], 0))
        assert excused <= 1
        assert m.mfma_profile(reset=-1)["launches"] > 0       # the counter was live: the greedy decode shows in it
    finally:
        m.ctx.close()


# ---- f. split-bf16 mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("everywhere", [False, True])
def test_split_mode_passes_the_strict_check_and_fp32_bits_return(knobs, everywhere):
    """test_gpu_bf3.py::test_forward_split_mode_passes_the_strict_check_small per set, then the fp32 bits after mode 0."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    from tests.test_gpu_bf3 import _split_mode
    m, W, s, name = knobs
    img = make_synthetic_image(224, 288, 3)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
    fp32 = m.forward_raw(img)
    with _split_mode(m.ctx, everywhere=everywhere):
        r = parity.strict_check(m, W, img, 100)
    print(name, everywhere, {k: v for k, v in r.items() if not isinstance(v, list)})
    assert r["K"] > 0 and r["matched"] > 0 and r["trunk_rel_err"] < 1e-5
    again = m.forward_raw(img)
    for x, y in zip(again, fp32):
        np.testing.assert_array_equal(x, y)


# ---- g. the other entry points, one set ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entry_model():
    from densecap_amd import DenseCapModel
    W = set_weights(ENTRY_POINT_SET)
    m = DenseCapModel(W, device=0)
    yield m, W, SETS[ENTRY_POINT_SET]
    m.ctx.close()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("order", [0, 1])
def test_forward_boxes_round_trip_is_bitwise(entry_model, order, lanes):
    from tests.test_gpu_boxes import _round_trip
    m, W, s = entry_model
    try:
        _round_trip(m, 224, 288, 100, order, lanes)
    finally:
        m.setGraphReplay(False); m.setCaptionOrder(False); m.setLanes(3); m.setTestArgs()


def test_extract_features_rows_are_the_codes_of_the_kept_boxes(entry_model):
    from densecap_amd.weights import make_synthetic_image
    m, W, s = entry_model
    P = 100
    img = make_synthetic_image(224, 288, 3)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    b, sc, _ = m.forward_raw(img)
    K = len(b)
    assert K > 0
    codes = m.debug_fetch("codes", (P, s["D"]))[0]
    idx = m.debug_fetch("final_nms_idx", (P,), np.int32)[0][:K]
    fb, ff = m.extractFeatures(img)
    np.testing.assert_array_equal(fb, b)
    assert ff.shape == (K, s["D"])
    np.testing.assert_array_equal(ff, codes[idx])


def test_graph_replayed_forward_equals_the_eager_one(entry_model):
    from densecap_amd.weights import make_synthetic_image
    m, W, s = entry_model
    imgs = [make_synthetic_image(224, 288, 300 + i) for i in range(4)]
    try:
        m.setLanes(1)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
        eager = [m.forward_raw(im) for im in imgs]
        launches0 = int(m.debug_fetch("graph_launches", (1,), np.int32)[0][0])
        m.setGraphReplay(True)
        replay = [m.forward_raw(im) for im in imgs]
        assert int(m.debug_fetch("graph_launches", (1,), np.int32)[0][0]) - launches0 == len(imgs) - 1
        for a, b in zip(eager, replay):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        assert len(eager[0][0]) > 0
    finally:
        m.setGraphReplay(False); m.setLanes(3); m.setTestArgs()


# ---- h. the door ---------------------------------------------------------------------------------------------------------
REFUSED = [("rnn_size", 48), ("enc_size", 16), ("fc_dim", 384), ("rpn_hidden", 40), ("num_anchors", 0)]


def test_the_loader_refuses_other_dimensions_and_the_context_stays_usable():
    """dc_load_weights checks the dimension fields before it reads a pointer: each refused value returns DC_E_INVALID with a
    message that names the field, and the same context then loads a valid model and runs it."""
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import DcWeights
    from densecap_amd.ops import Context
    from densecap_amd.weights import make_synthetic_image
    ctx = Context(0)
    try:
        good = dict(num_anchors=1, rpn_hidden=32, vocab_size=5, seq_length=1, enc_size=32, rnn_size=32, fc_dim=256)
        for field, value in REFUSED:
            w = DcWeights()                                   # null tensors: the refusal must come before any of them is read
            for k, v in dict(good, **{field: value}).items():
                setattr(w, k, v)
            rc = ctx.lib.dc_load_weights(ctx.h, C.byref(w))
            msg = (ctx.lib.dc_last_error(ctx.h) or b"").decode()
            assert rc == -1, (field, value, rc)               # DC_E_INVALID
            assert "dc_load_weights" in msg and field in msg, (field, msg)
        W = set_weights("minimal")
        m = DenseCapModel(W, ctx=ctx)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
        boxes, scores, tokens = m.forward_raw(make_synthetic_image(160, 224, 1))
        assert len(boxes) > 0 and tokens.shape == (len(boxes), 1)
    finally:
        ctx.close()
