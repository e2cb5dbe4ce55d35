"""The standard beam search on the GPU (dc_beam_captions / dc_op_lm_beam_n; docs/SEMANTICS.md, "Standard beam search"), kernel by
kernel and step by step against tests/beam_std_rules.py (checked without a GPU in tests/test_beam_std_cpu.py).

  a. beam_std_merge_kernel against std_merge_ref, bit for bit, on hand-made inputs (multiples of 0.25: exact sums, ties
     everywhere): no / every / every other / only the best / only the worst parent finished, every sum equal, a finished parent
     that ties a live candidate, a proposal whose sums are all NaN.
  b. beam_std_finish_kernel: alpha 0 is the input order bit for bit; alpha > 0 passes the rank-wise rule (check_finish); equal
     scores, a NaN lp, len 1 and len T.
  c. every step of every proposal teacher-forced on std_walk's trajectory through dc_debug_beam_std_start / _step: lists by
     beam_rules.check_lists at parity.TOKEN_TOL, the merge on its own inputs bit for bit, the state by beam_rules.check_gather;
     the start state's h is the START step's h, not its c.
  d. ops.lm_beam_n end to end: the chained hooks end in the same bits, finished rows score what dc_op_lm_score says, the row
     format, the invariances (other rows, n_best, chunking, repeat, dc_set_beam_size and the math mode).
  e. the whole image, other model dimensions, the full vocabulary at B = 32, refusals, rows without a word, the CLI.

Nothing in this module excuses a row, a step or a rank, except the greedy comparison (B = 1), which excuses the rows the ORACLE
calls a near tie and asserts there are at most 2 of them.
"""
import ctypes as C
import json

import numpy as np
import pytest

from tests import beam_rules as R
from tests import beam_std_rules as S
from tests import parity

pytestmark = pytest.mark.gpu
V, T, N = S.FIX_V, S.FIX_T, S.FIX_N
END = V + 1
STAGE = 1e-4                     # the scorer's bound (docs/SEMANTICS.md, "Scoring captions")


@pytest.fixture(scope="module")
def model():
    """The fixture's model.  One small forward first, so that the ctx's fault word exists and reads 0 from then on."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image
    parity.oracle_threads()
    W, codes = S.fixture()
    m = DenseCapModel(W, device=0)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    m.forward_raw(make_synthetic_image(96, 128, 0))
    assert _fault_word(m) == 0
    yield m, W, codes
    m.ctx.close()


def _fault_word(m):
    return int(m.debug_fetch("fault_word", (1,), np.int32)[0][0])


def _hd(W):
    return W["lstm_w"].shape[1] // 4


# ---- a. the merge kernel -------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "alternating", "best", "worst")


def _fin_pattern(pattern, nprop, beam):
    fin = np.zeros((nprop, beam), np.uint8)
    if pattern == "all":
        fin[:] = 1
    elif pattern == "alternating":
        fin[:, 1::2] = 1
        fin[1::2] ^= 1 if beam > 1 else 0                             # odd proposals: the other half
    elif pattern == "best":
        fin[:, 0] = 1
    elif pattern == "worst":
        fin[:, -1] = 1
    return fin


def _merge_case(nprop, beam, t, pattern, seed):
    """Inputs of a merge at column t on multiples of 0.25.  Finished parents hold END in a column below t, zeros after it, and
    the lists the top-k kernel makes for them (zeros / 1..beam); live lists hold END now and then, at any rank."""
    rng = np.random.default_rng(seed)
    fin = _fin_pattern(pattern, nprop, beam)
    beam_lp = -np.sort(rng.integers(0, 12, (nprop, beam)), axis=1).astype(np.float32) * np.float32(0.25)
    beams = np.zeros((nprop, beam, T), np.int32)
    beams[:, :, :t] = rng.integers(1, END, (nprop, beam, t))
    length = np.full((nprop, beam), t, np.int32)
    for p, b in np.argwhere(fin):
        e = int(rng.integers(0, t))
        beams[p, b, e] = END
        beams[p, b, e + 1:] = 0
        length[p, b] = e + 1
    top_lp = -np.sort(rng.integers(0, 8, (nprop, beam, beam)), axis=2).astype(np.float32) * np.float32(0.25)
    top_idx = np.stack([np.stack([rng.permutation(END - 1)[:beam] + 1 for _ in range(beam)]) for _ in range(nprop)]).astype(np.int32)
    for p, b in np.argwhere(rng.random((nprop, beam)) < 0.5):
        top_idx[p, b, rng.integers(0, beam)] = END
    f = fin.astype(bool)
    top_lp[f] = 0
    top_idx[f] = np.arange(1, beam + 1)
    return top_lp, top_idx, beam_lp, beams, length, fin


def _merge_checked(ctx, case, t, what):
    from densecap_amd import ops
    top_lp, top_idx, beam_lp, beams, length, fin = case
    out = ops.beam_std_merge(ctx, top_lp, top_idx, beam_lp, beams, length, fin, t, END)
    R.check_same(out, S.std_merge_ref(top_lp, top_idx, beam_lp, beams, length, fin, t, END), what)
    return out


@pytest.mark.parametrize("beam", [1, 2, 5, 32])
def test_merge_is_the_restatement_bit_for_bit(model, beam):
    ctx = model[0].ctx
    for t in (1, T - 1):
        for k, pattern in enumerate(PATTERNS):
            case = _merge_case(7, beam, t, pattern, 1000 * beam + 10 * t + k)
            out = _merge_checked(ctx, case, t, "merge beam %d t %d fin %s" % (beam, t, pattern))
            fin = case[5].astype(bool)
            pf = np.take_along_axis(fin, out["parent"].astype(np.int64), 1)
            if pattern == "all":                                      # nothing moves: every hypothesis is its own single candidate
                assert (out["beams"][:, :, t] == 0).all() and out["fin"].all()
                assert (out["len"] == np.take_along_axis(case[4], out["parent"].astype(np.int64), 1)).all()
                assert sorted(out["parent"][0].tolist()) == list(range(beam))
            if pattern == "none":
                assert (out["beams"][:, :, t] >= 1).all() and (out["len"] == t + 1).all()
            for p in range(7):                                        # a finished parent is selected at most once
                chosen = out["parent"][p][pf[p]]
                assert len(set(chosen.tolist())) == len(chosen)
    # every sum equal: the picks are flat 0..beam-1, whatever is finished (a finished parent's single candidate is (b, 0))
    top_lp = np.zeros((7, beam, beam), np.float32); beam_lp = np.full((7, beam), -1.25, np.float32)
    top_idx = np.tile(np.arange(1, beam + 1, dtype=np.int32), (7, beam, 1))
    beams = np.zeros((7, beam, T), np.int32); beams[:, :, 0] = 3
    length = np.ones((7, beam), np.int32)
    out = _merge_checked(ctx, (top_lp, top_idx, beam_lp, beams, length, np.zeros((7, beam), np.uint8)), 1, "flat merge")
    assert (out["parent"] == 0).all() and (out["tok"] == np.arange(1, beam + 1)).all()
    if beam > 1:
        fin = _fin_pattern("best", 7, beam)
        fb = beams.copy(); fb[:, 0, 0] = END
        out = _merge_checked(ctx, (top_lp, top_idx, beam_lp, fb, length, fin), 1, "flat merge, the best finished")
        assert (out["parent"][:, 0] == 0).all() and (out["parent"][:, 1:] == 1).all() and (out["fin"][:, 0] == 1).all()
        # a finished parent's lp ties a live candidate: parent 0 live at -1 with lists of -1 (sums -2 at flat 0..), parent 1
        # finished at -2 (flat `beam`): the live candidates of parent 0 come first, then the finished one, once
        beam_lp = np.full((7, beam), -3.0, np.float32); beam_lp[:, 0] = -1; beam_lp[:, 1] = -2
        fin = np.zeros((7, beam), np.uint8); fin[:, 1] = 1
        fb = beams.copy(); fb[:, 1, 0] = END
        out = _merge_checked(ctx, (top_lp - 1, top_idx, beam_lp, fb, length, fin), 1, "a finished parent ties a live candidate")
        assert (out["parent"] == 0).all()
        beam_lp[:, 1] = -1.5                                          # and ahead of them when it is better
        out = _merge_checked(ctx, (top_lp - 1, top_idx, beam_lp, fb, length, fin), 1, "a finished parent ahead")
        assert (out["parent"][:, 0] == 1).all() and (out["beam_lp"][:, 0] == -1.5).all() and (out["parent"][:, 1:] == 0).all()
    # one proposal whose sums are all NaN: no word
    case = list(_merge_case(7, beam, 1, "none", 77 + beam))
    case[0][3] = np.nan; case[2][3] = np.nan
    out = _merge_checked(ctx, tuple(case), 1, "a proposal of NaNs")
    assert np.isnan(out["beam_lp"][3]).all() and (out["tok"][3] == S.FEED_WORD).all() and out["fin"][3].all()
    assert (out["beams"][3, :, 1] == 0).all() and out["parent"][3].tolist() == list(range(beam))
    assert _fault_word(model[0]) == 0


# ---- b. the finish kernel ------------------------------------------------------------------------------------------------------
def _finish_case(nprop, beam, seed):
    """beam_lp descending (the merge's order), lengths 1..T with both ends present, rows that hold `len` words; where the beam is
    wide enough: two hypotheses with equal lp and len, a NaN lp in the last place of proposal 1."""
    rng = np.random.default_rng(seed)
    lp = -np.sort(rng.random((nprop, beam)).astype(np.float32) * 12, axis=1)
    length = rng.integers(1, T + 1, (nprop, beam)).astype(np.int32)
    length[0, 0] = 1
    length[0, -1] = T
    if beam >= 5:
        lp[2, 3] = lp[2, 2]; length[2, 3] = length[2, 2]
        lp[3, :] = np.float32(-6); length[3] = np.arange(beam) % T + 1        # equal lp, scores differ by length only
    if beam > 1:
        lp[1, -1] = np.nan
    beams = np.zeros((nprop, beam, T), np.int32)
    for p in range(nprop):
        for b in range(beam):
            beams[p, b, :length[p, b]] = rng.integers(1, END, length[p, b])
            if length[p, b] < T or rng.random() < 0.5:
                beams[p, b, length[p, b] - 1] = END
    return lp, beams, length


@pytest.mark.parametrize("beam", [1, 5, 32])
def test_finish_kernel(model, beam):
    from densecap_amd import ops
    ctx = model[0].ctx
    lp, beams, length = _finish_case(7, beam, beam)
    for n_best in sorted({1, beam}):
        caps, out = ops.beam_std_finish(ctx, lp, beams, length, n_best, 0.0)
        S.check_finish(caps, out, lp, beams, length, n_best, 0.0, "finish beam %d n_best %d alpha 0" % (beam, n_best))
        assert (caps[0] == beams[0, :n_best]).all()
    worst = 0.0
    for a in (0.5, 1.0, 2.0):
        for n_best in sorted({1, min(2, beam), beam}):
            caps, out = ops.beam_std_finish(ctx, lp, beams, length, n_best, a)
            worst = max(worst, S.check_finish(caps, out, lp, beams, length, n_best, a,
                                              "finish beam %d n_best %d alpha %g" % (beam, n_best, a)))
            if beam > 1 and n_best == beam:
                assert np.isnan(out[1, -1]) and (caps[1, -1] == 0).all() and not np.isnan(out[1, :-1]).any()
            if beam >= 5 and n_best == beam:
                r = [i for i in range(beam) if (caps[2, i] == beams[2, 2]).all()][0]       # equal scores: hypothesis order
                assert (caps[2, r + 1] == beams[2, 3]).all()
                assert (caps[3, 0] == beams[3, length[3].argmax()]).all()                   # lp -6: the longest first
    print("finish beam %d: worst relative score distance from the rank's %.3g (bound %.3g)" % (beam, worst, S.RANK_REL))


# ---- c. every step, teacher-forced on std_walk's trajectory ----------------------------------------------------------------------
def _teacher_forced(m, W, codes, beam, T_, V_, walk, name):
    from densecap_amd import ops
    Hd = _hd(W)
    end = V_ + 1
    tol = parity.TOKEN_TOL
    state, top_lp, top_idx = ops.beam_std_start(m.ctx, codes, beam, Hd, T_)
    what = "%s beam %d start" % (name, beam)
    wv, ws, lists = S.check_start(state, top_lp, top_idx, walk, T_, end, tol, parity.REL, what)
    assert (state["h"].view(np.uint32) != state["c"].view(np.uint32)).any(), "%s: h rows are the cell rows" % what
    for t in range(1, T_):
        st = walk["steps"][t]
        fed = st["state"]                                            # always the reference's, never the device's
        out, top_lp, top_idx = ops.beam_std_step(m.ctx, fed, t)
        v, s, k = S.check_step(out, top_lp, top_idx, fed, st, t, end, tol, parity.REL, "%s beam %d step %d" % (name, beam, t))
        wv, ws, lists = max(wv, v), max(ws, s), lists + k
    print("%s beam %d: %d proposals x %d steps, %d live lists, worst value difference %.3g, worst rank slack %.3g; "
          "excused 0 rows, 0 steps, 0 ranks" % (name, beam, len(codes), T_, lists, wv, ws))
    return lists


@pytest.mark.parametrize("beam", [1, 4, 8])
def test_every_step_teacher_forced(model, beam):
    m, W, codes = model
    lists = _teacher_forced(m, W, codes, beam, T, V, S.fixture_walk(beam), "fixture")
    assert lists >= N * (1 + beam)
    assert _fault_word(m) == 0


# ---- d. end to end ---------------------------------------------------------------------------------------------------------------
def _chained(m, W, codes, beam, T_):
    """dc_debug_beam_std_start and T - 1 dc_debug_beam_std_step calls on the device's own outputs: the last state."""
    from densecap_amd import ops
    state, _, _ = ops.beam_std_start(m.ctx, codes, beam, _hd(W), T_)
    for t in range(1, T_):
        state, _, _ = ops.beam_std_step(m.ctx, state, t)
    return state


def _row_format(caps, end):
    assert caps.min() >= 0 and caps.max() <= end, (caps.min(), caps.max())
    flat = caps.reshape(-1, caps.shape[-1])
    after = np.cumsum(flat == end, axis=1) - (flat == end)             # > 0 strictly after the first END
    assert (flat[after > 0] == 0).all(), "a word after END"
    gap = np.cumsum(flat == 0, axis=1)
    assert (flat[gap > 0] == 0).all(), "a word after a zero"
    ended = (flat == end).any(axis=1)
    assert ((flat != 0).all(axis=1) | ended | (flat == 0).all(axis=1)).all(), "a row stops without END"
    return ended.reshape(caps.shape[:-1])


@pytest.mark.parametrize("beam,alpha", [(4, 0.0), (8, 0.0), (4, 0.7)])
def test_lm_beam_n_end_to_end(model, beam, alpha):
    from densecap_amd import ops
    m, W, codes = model
    caps, lp = ops.lm_beam_n(m.ctx, codes, beam, None, alpha)
    assert caps.shape == (N, beam, T) and lp.shape == (N, beam) and caps.dtype == np.int32 and lp.dtype == np.float32
    last = _chained(m, W, codes, beam, T)
    want = ops.beam_std_finish(m.ctx, last["beam_lp"], last["beams"], last["len"], beam, alpha)
    R.check_same(dict(captions=caps, logprob=lp), dict(captions=want[0], logprob=want[1]), "chained hooks beam %d" % beam)
    S.check_finish(caps, lp, last["beam_lp"], last["beams"], last["len"], beam, alpha, "ranking beam %d alpha %g" % (beam, alpha))
    ended = _row_format(caps, END)
    assert np.isfinite(lp).all()
    if alpha == 0:
        assert (np.diff(lp.astype(np.float64), axis=1) <= 0).all()
        assert (ended == last["fin"].astype(bool)).all()
    # every finished row: its logprob is the scorer's for that caption on that code
    q = np.where(caps == END, 0, caps).reshape(N * beam, T)
    score = ops.lm_score(m.ctx, codes, q).reshape(N, N, beam)[np.arange(N), np.arange(N)]
    d = np.abs(lp.astype(np.float64) - score)[ended]
    assert ended.sum() >= 24 and (~ended).sum() >= 5                  # the fixture's conditions (test_beam_std_cpu.py)
    print("beam %d alpha %g: %d finished rows, worst |logprob - dc_op_lm_score| %.3g (bound %.3g)" % (beam, alpha, ended.sum(), d.max(), STAGE))
    assert d.max() <= STAGE
    ref_caps, _ = S.std_search(S.fixture_walk(beam), beam, alpha)
    print("  proposals whose captions are the reference's: %d of %d" % (sum((caps[i] == ref_caps[i]).all() for i in range(N)), N))
    assert _fault_word(m) == 0


def test_width_one_is_the_greedy_decode(model):
    import torch
    from densecap_amd import ops
    from oracle import densecap_oracle as O
    from tests.test_gpu_sample import _greedy
    m, W, codes = model
    m.setBeamSize(0)
    seq = _greedy(m, codes)
    caps, lp = ops.lm_beam_n(m.ctx, codes, 1, 1, 0.0)
    oseq, logits = O.lm_sample(torch.from_numpy(codes), W, T, return_logits=True)
    excused = 0
    for i in range(N):
        e = np.nonzero(oseq[i] == END)[0]
        n = e[0] + 1 if len(e) else T
        gap = min(float(np.diff(np.sort(logits[t][i].numpy().astype(np.float64))[-2:])[0]) for t in range(n))
        if gap <= 2 * parity.TOKEN_TOL:
            excused += 1
            continue
        e = np.nonzero(seq[i] == END)[0]
        n = e[0] + 1 if len(e) else T
        np.testing.assert_array_equal(caps[i, 0, :n], seq[i, :n], err_msg="row %d" % i)
        assert (caps[i, 0, n:] == 0).all()
    print("B = 1 against dc_op_lm_sample: %d of %d rows excused by the oracle's own near tie" % (excused, N))
    assert excused <= 2


def test_invariances_bit_for_bit(model):
    from densecap_amd import ops
    from densecap_amd._lib import check
    m, W, codes = model
    B, a = 4, 0.7
    caps, lp = ops.lm_beam_n(m.ctx, codes, B, None, a)
    same = lambda got, what: R.check_same(dict(captions=got[0], logprob=got[1]), dict(captions=caps, logprob=lp), what)
    same(ops.lm_beam_n(m.ctx, codes, B, None, a), "a second call")
    sub = ops.lm_beam_n(m.ctx, codes[3:7], B, None, a)
    R.check_same(dict(captions=sub[0], logprob=sub[1]), dict(captions=caps[3:7], logprob=lp[3:7]), "rows 3..6 alone")
    two = ops.lm_beam_n(m.ctx, codes, B, 2, a)
    R.check_same(dict(captions=two[0], logprob=two[1]), dict(captions=caps[:, :2], logprob=lp[:, :2]), "n_best 2")
    try:
        m.setBeamSize(3)
        same(ops.lm_beam_n(m.ctx, codes, B, None, a), "under dc_set_beam_size(3)")
        m.setBeamSize(0)
        m.setMathMode(1)
        same(ops.lm_beam_n(m.ctx, codes, B, None, a), "under math mode 1")
    finally:
        m.setBeamSize(0)
        m.setMathMode(0)
    # the chunk loop: chunks hold at least 64 proposals, so 130 rows (the fixture's codes and variations of them) make three
    big = np.concatenate([codes * np.float32(s) for s in (1.0, 0.5, 1.5, 0.75, 1.25, 2.0)])[:130]
    whole = ops.lm_beam_n(m.ctx, big, B, None, a)
    R.check_same(dict(captions=whole[0][:N], logprob=whole[1][:N]), dict(captions=caps, logprob=lp), "the first 24 of 130 rows")
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"beam_chunk_floats", 1), "dc_debug_set")
    try:
        parts = ops.lm_beam_n(m.ctx, big, B, None, a)
    finally:
        check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"beam_chunk_floats", 1 << 28), "dc_debug_set")
    R.check_same(dict(captions=parts[0], logprob=parts[1]), dict(captions=whole[0], logprob=whole[1]), "three chunks")
    assert _fault_word(m) == 0


def test_two_searches_share_one_scratch():
    """Both searches grow and reuse the lane's one beam scratch: on a ctx whose scratch does not exist yet, the standard search at
    width 4 and the reference rule at width 3 give the same bits before and after the other search, a wider and a narrower run
    have carved the scratch again or run on a corner of it."""
    from densecap_amd import DenseCapModel, ops
    from densecap_amd.weights import make_synthetic_image
    from tests.test_gpu_sample import _greedy
    W, codes = S.fixture()
    m = DenseCapModel(W, device=0)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    a = 0.7
    std = lambda x, B: dict(zip(("captions", "logprob"), ops.lm_beam_n(m.ctx, x, B, None, a)))

    def ref(B):
        m.setBeamSize(B)
        try:
            return _greedy(m, codes)
        finally:
            m.setBeamSize(0)

    try:
        m.forward_raw(make_synthetic_image(96, 128, 0))               # the fault word exists from here on
        A = std(codes, 4)
        R3 = ref(3)
        assert R3.shape == (N, T) and (R3 != R3[0]).any()
        ref(8)                                                        # the width grows: carved again
        R.check_same(std(codes, 4), A, "width 4 after the reference rule at 8")
        wide = std(codes, 32)                                         # ... and again
        np.testing.assert_array_equal(ref(3), R3)
        two = std(codes[3:7], 2)                                      # rows, chunk and width shrink: the same carve
        R.check_same(two, {k: v[3:7] for k, v in std(codes, 2).items()}, "width 2, rows 3..6 alone")
        R.check_same(std(codes, 4), A, "width 4 at the end")
        assert wide["captions"].shape == (N, 32, T) and _row_format(A["captions"], END).any()
        assert _fault_word(m) == 0
    finally:
        m.setBeamSize(0)
        m.ctx.close()


# ---- e. the whole image, other shapes, refusals, the CLI -------------------------------------------------------------------------
def test_whole_image(model):
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, W, _ = model
    img = np.ascontiguousarray(make_synthetic_image(320, 480, 3), np.float32)
    b0, s0, t0 = m.forward_raw(img)
    boxes, scores, tokens, caps, lp = m.beamCaptions(img, 4, 2, 0.7)
    K = len(b0)
    assert K > 0 and caps.shape == (K, 2, T) and lp.shape == (K, 2)
    np.testing.assert_array_equal(boxes, b0)
    np.testing.assert_array_equal(scores, s0)
    np.testing.assert_array_equal(tokens, t0)
    fb, feats = m.extractFeatures(img)
    np.testing.assert_array_equal(fb, b0)
    want = ops.lm_beam_n(m.ctx, feats, 4, 2, 0.7)
    R.check_same(dict(captions=caps, logprob=lp), dict(captions=want[0], logprob=want[1]), "beamCaptions against lm_beam_n")
    _row_format(caps, END)
    b1, s1, none, c1, l1 = m.beamCaptions(img, 4, 2, 0.7, want_tokens=False)
    assert none is None
    np.testing.assert_array_equal(b1, b0)
    R.check_same(dict(captions=c1, logprob=l1), dict(captions=caps, logprob=lp), "want_tokens=False")
    assert len(m.decodeSequence(caps[:, 0])) == K
    assert _fault_word(m) == 0


def test_other_dimensions_teacher_forced():
    """One set of the family tests/test_gpu_dims.py covers (E = 256 < rnn_size = 768, fc_dim 512, V = 777, T = 9), built the way
    that file builds its weights: every step at B = 3 on 8 codes."""
    from densecap_amd import DenseCapModel
    from tests.test_gpu_dims import SETS, _oracle_codes, set_weights
    parity.oracle_threads()
    s = SETS["e_lt_h"]
    W = set_weights("e_lt_h")
    codes = _oracle_codes(8, s["D"], 0)
    walk = S.std_walk(codes, W, s["T"], 3)
    m = DenseCapModel(W, device=0)
    try:
        assert _teacher_forced(m, W, codes, 3, s["T"], s["V"], walk, "e_lt_h") >= 8
    finally:
        m.ctx.close()


def test_full_vocabulary_widest_beam():
    """V = 10497, B = 32, n_best = 32, alpha 1 on 4 codes: the 1024-candidate merge and the widest lists, every step
    teacher-forced on std_walk, the final ranking rank-wise on the device's own last state."""
    from densecap_amd import DenseCapModel, ops
    from densecap_amd.weights import make_synthetic_weights
    parity.oracle_threads()
    Vf, Tf, B = 10497, 15, 32
    W = make_synthetic_weights(seed=1234, vocab_size=Vf, seq_length=Tf)
    codes = (np.random.default_rng(7).standard_normal((4, 4096)) * 2).astype(np.float32)
    walk = S.std_walk(codes, W, Tf, B)
    m = DenseCapModel(W, device=0)
    try:
        assert _teacher_forced(m, W, codes, B, Tf, Vf, walk, "full vocabulary") >= 4 * (1 + B)
        caps, lp = ops.lm_beam_n(m.ctx, codes, B, B, 1.0)
        last = _chained(m, W, codes, B, Tf)
        S.check_finish(caps, lp, last["beam_lp"], last["beams"], last["len"], B, 1.0, "full vocabulary ranking")
        _row_format(caps, Vf + 1)
        ref = walk["final"]
        S.check_finish(*S.std_search(walk, B, 1.0), ref["beam_lp"], ref["beams"], ref["len"], B, 1.0, "the reference's own ranking")
    finally:
        m.ctx.close()


def test_refusals_and_rows_without_a_word(model):
    from densecap_amd import _lib, ops
    from densecap_amd._lib import DenseCapError, check
    m, W, codes = model
    ctx = m.ctx
    xd = ctx.to_device(codes[:2])
    cap = ctx.to_device(np.full((2, 32, T), -7, np.int32)); lp = ctx.to_device(np.full((2, 32), 7.0, np.float32))
    bad = [(0, 1, 0.0), (33, 1, 0.0), (-1, 1, 0.0), (4, 0, 0.0), (4, 5, 0.0), (4, -1, 0.0), (4, 2, -0.1), (4, 2, 2.5),
           (4, 2, float("nan")), (4, 2, float("inf"))]
    for b, n, a in bad:
        o = _lib.DcBeamOpts(b, n, a)
        rc = ctx.lib.dc_op_lm_beam_n(ctx.h, xd.ptr, 2, C.byref(o), cap.ptr, lp.ptr)
        assert rc == -1, ((b, n, a), rc)                              # DC_E_INVALID
        with pytest.raises(DenseCapError):
            check(ctx.h, rc, "dc_op_lm_beam_n")
        assert (cap.numpy() == -7).all() and (lp.numpy() == 7.0).all()
    img = np.zeros((3, 96, 128), np.float32)
    r, r_boxes, r_scores, r_tokens = m._new_result(m._capacity(96, 128))      # (the arrays r points into stay alive)
    host_c = np.full((r.capacity, 2, T), -7, np.int32); host_l = np.full((r.capacity, 2), 7.0, np.float32)
    o = _lib.DcBeamOpts(40, 2, 0.0)
    assert ctx.lib.dc_beam_captions(ctx.h, img.ctypes.data, 96, 128, 0, C.byref(o), C.byref(r), host_c.ctypes.data,
                                    host_l.ctypes.data) == -1
    assert (host_c == -7).all() and (host_l == 7.0).all()
    # the ctx is usable afterwards, and a non-finite code gives its row no word while the others do not notice
    six = codes[:6].copy()
    clean = ops.lm_beam_n(ctx, np.delete(six, 2, axis=0), 4, None, 0.7)
    six[2, 100] = np.inf
    caps, out = ops.lm_beam_n(ctx, six, 4, None, 0.7)                 # _lib.check: any code but DC_OK raises
    assert (caps[2] == 0).all() and np.isnan(out[2]).all()
    keep = [0, 1, 3, 4, 5]
    R.check_same(dict(captions=caps[keep], logprob=out[keep]), dict(captions=clean[0], logprob=clean[1]), "rows beside the bad one")
    assert caps.min() >= 0 and caps.max() <= END
    assert _fault_word(m) == 0
    again = ops.lm_beam_n(ctx, np.delete(codes[:6], 2, axis=0), 4, None, 0.7)
    R.check_same(dict(captions=again[0], logprob=again[1]), dict(captions=clean[0], logprob=clean[1]), "a clean call afterwards")


def test_cli(tmp_path):
    """run_model in this process on two synthetic images: with -num_beams the file gains beam_captions / beam_logprobs of the
    right shapes; without it no new key appears anywhere in the file, and the boxes, scores and captions are the same."""
    from PIL import Image
    from densecap_amd import run_model
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(120, 160), (140, 100)]):
        rgb = (np.random.default_rng(i).random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(d / ("im%d.png" % i)))
    common = ["-input_dir", str(d), "-synthetic_weights", "1", "-num_proposals", "50", "-image_size", "160"]
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "plain")]) == 0
    text = open(tmp_path / "plain" / "results.json").read()
    for key in ("beam_captions", "beam_logprobs", "num_beams", "n_best", "length_alpha"):
        assert key not in text, key
    plain = json.loads(text)
    assert len(plain["results"]) == 2 and all(set(e) == {"boxes", "scores", "captions", "img_name"} for e in plain["results"])
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "beam"), "-num_beams", "3", "-n_best", "2",
                                    "-length_alpha", "0.7"]) == 0
    res = json.load(open(tmp_path / "beam" / "results.json"))
    assert (res["opt"]["num_beams"], res["opt"]["n_best"], res["opt"]["length_alpha"]) == (3, 2, 0.7)
    assert "num_samples" not in res["opt"]
    for e, p in zip(res["results"], plain["results"]):
        assert {k: e[k] for k in p} == p
        K = len(e["boxes"])
        assert K > 0 and len(e["beam_captions"]) == K and len(e["beam_logprobs"]) == K
        assert all(len(c) == 2 and all(isinstance(s, str) for s in c) for c in e["beam_captions"])
        assert all(len(l) == 2 and all(isinstance(v, float) for v in l) for l in e["beam_logprobs"])
