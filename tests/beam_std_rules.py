"""The standard beam search step by step (test infrastructure for tests/test_beam_std_cpu.py and tests/test_gpu_beam_std.py).

docs/SEMANTICS.md, "Standard beam search", restated on numpy arrays for all proposals at once in the layout of the device
(rows = proposal x hypothesis), with the oracle's own lstm_step / _log_softmax_thnn and beam_rules.topk_ref for the lists:

  std_init_ref    the first expansion: the B best words, len 1, columns 1.. hold 0
  std_merge_ref   fp32 sums under live parents, ONE candidate (b, 0) with lp[b] itself under a finished one, stable order (lower
                  flat index first), NaN never a candidate; a rank without a candidate keeps its own row, NaN, no word, finished
  std_finish_ref  lp / pen[len] with one fp32 division, pen tabulated as (float)pow(l, a); a == 0: the order of the input
  std_walk        the whole trajectory in fp32, every step recorded as beam_rules.oracle_walk records it

and the rules a device must meet, written once: lists by beam_rules.check_lists at parity.TOKEN_TOL, a merge or finish fed its own
inputs bit for bit (beam_rules.check_same), the ranking under a > 0 rank-wise (check_finish).  Nothing here skips a row, a step or
a rank.

The fixture (shared by both test files): make_synthetic_weights(seed=21, vocab_size=200, seq_length=15) with the END bias raised by
1.0 -- without it almost no hypothesis ever finishes and the new rules go untested -- and 24 codes of scale 2.
"""
import numpy as np

from tests import beam_rules as R

F32 = np.float32
FEED_WORD = 1                     # kFeedWord of beam.hip: the valid id a row without a word feeds to the next step
RANK_REL = 2.0 ** -22             # two correct implementations round the table entry and the quotient once each: 2 x 2^-23

FIX_V, FIX_T, FIX_N = 200, 15, 24


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
_FIXTURE = {}


def fixture():
    """(weights, codes (24, 4096) float32) of the module docstring, made once."""
    if not _FIXTURE:
        from densecap_amd.weights import make_synthetic_weights
        W = make_synthetic_weights(seed=21, vocab_size=FIX_V, seq_length=FIX_T)
        W["lm_out_b"][FIX_V] += 1.0                                   # END = V + 1, 1-based: row V of the output layer
        codes = (np.random.default_rng(5).standard_normal((FIX_N, 4096)) * 2).astype(F32)
        _FIXTURE["v"] = (W, codes)
    return _FIXTURE["v"]


_WALKS = {}


def fixture_walk(beam):
    """std_walk of the fixture at a beam width, computed once and left unchanged."""
    if beam not in _WALKS:
        W, codes = fixture()
        _WALKS[beam] = std_walk(codes, W, FIX_T, beam)
    return _WALKS[beam]


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def std_init_ref(top_lp, top_idx, T, END):
    """The first expansion from the first step's lists (nprop, beam): dict(beam_lp, beams, len, parent, tok, fin)."""
    top_idx = np.asarray(top_idx, np.int32)
    nprop, beam = top_idx.shape
    none = (top_idx < 1) | (top_idx > END)
    w = np.where(none, 0, top_idx).astype(np.int32)
    beams = np.zeros((nprop, beam, T), np.int32)
    beams[:, :, 0] = w
    return dict(beam_lp=np.asarray(top_lp, F32).copy(), beams=beams, len=(~none).astype(np.int32),
                parent=np.zeros((nprop, beam), np.int32), tok=np.where(none, FEED_WORD, w).astype(np.int32),
                fin=(none | (w == END)).astype(np.uint8))


def std_merge_ref(top_lp, top_idx, beam_lp, beams, length, fin, t, END, flood=False):
    """The merge of step t: top_lp / top_idx (nprop, beam, beam), beam_lp, length, fin (nprop, beam), beams (nprop, beam, T) ->
    dict(beam_lp, beams, len, parent, tok, fin).  flood=True is the WRONG rule the definition replaces (a finished parent
    contributes all its `beam` candidates): for the tests that show the rule has teeth."""
    top_lp = np.asarray(top_lp, F32); beam_lp = np.asarray(beam_lp, F32)
    top_idx = np.asarray(top_idx, np.int32); beams = np.asarray(beams, np.int32)
    length = np.asarray(length, np.int32); pf = np.asarray(fin).astype(bool)
    nprop, beam, T = beams.shape
    nc = beam * beam
    cand = np.where(pf[:, :, None], beam_lp[:, :, None], (top_lp + beam_lp[:, :, None]).astype(F32)).astype(F32)
    valid = ~pf[:, :, None] | (np.arange(beam)[None, None, :] == 0) | bool(flood)
    cand = cand.reshape(nprop, nc)
    valid = valid.reshape(nprop, nc) & ~np.isnan(cand)
    flat_ix = np.broadcast_to(np.arange(nc), (nprop, nc))
    neg = np.where(valid, -cand.astype(np.float64), 0.0)
    order = np.lexsort((flat_ix, neg, ~valid), axis=-1)[:, :beam]            # valid first, higher sum first, lower index first
    picked = np.take_along_axis(valid, order, 1)
    q_ix = np.broadcast_to(np.arange(beam), (nprop, beam))
    parent = np.where(picked, order // beam, q_ix).astype(np.int32)
    set_aside = ~picked | np.take_along_axis(pf, parent.astype(np.int64), 1)
    w0 = np.where(set_aside, 0, np.take_along_axis(top_idx.reshape(nprop, nc), order, 1))
    none = (w0 < 1) | (w0 > END)
    w = np.where(none, 0, w0).astype(np.int32)
    new = np.take_along_axis(beams, parent[:, :, None].astype(np.int64), 1).copy()
    new[:, :, t] = w
    lp = np.where(picked, np.take_along_axis(cand, order, 1), F32(np.nan)).astype(F32)
    return dict(beam_lp=lp, beams=new, len=(np.take_along_axis(length, parent.astype(np.int64), 1) + ~none).astype(np.int32),
                parent=parent, tok=np.where(none, FEED_WORD, w).astype(np.int32), fin=(none | (w == END)).astype(np.uint8))


def pen_table(T, alpha):
    """pen[l] = (float)pow((double)l, (double)alpha) for l = 0..T, pen[0] = 1."""
    pen = np.ones(T + 1, F32)
    pen[1:] = np.power(np.arange(1, T + 1, dtype=np.float64), float(F32(alpha))).astype(F32)
    return pen


def std_scores(beam_lp, length, T, alpha):
    """The ranking score of every hypothesis: lp itself at alpha 0, else the fp32 quotient lp / pen[len]."""
    lp = np.asarray(beam_lp, F32)
    if float(alpha) == 0.0:
        return lp.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return (lp / pen_table(T, alpha)[np.clip(np.asarray(length), 0, T)]).astype(F32)


def std_order(scores, alpha):
    """The final order of every proposal's hypotheses: at alpha 0 the input's; else descending score, equal scores in
    hypothesis order, NaN last in hypothesis order."""
    nprop, beam = scores.shape
    ix = np.broadcast_to(np.arange(beam), (nprop, beam))
    if float(alpha) == 0.0:
        return ix.copy()
    nan = np.isnan(scores)
    return np.lexsort((ix, np.where(nan, 0.0, -scores.astype(np.float64)), nan), axis=-1)


def std_finish_ref(beam_lp, beams, length, n_best, alpha):
    """The final ranking: (captions (nprop, n_best, T) int32, logprob (nprop, n_best) float32)."""
    beam_lp = np.asarray(beam_lp, F32); beams = np.asarray(beams, np.int32)
    T = beams.shape[2]
    order = std_order(std_scores(beam_lp, length, T, alpha), alpha)[:, :n_best]
    lp = np.take_along_axis(beam_lp, order, 1)
    caps = np.take_along_axis(beams, order[:, :, None], 1).copy()
    caps[np.isnan(lp)] = 0
    return caps, lp


def _lm_rows(Wt, tok, h, c):
    """One LSTM step of rows on their words and the log-probabilities after it, with the oracle's functions."""
    import torch
    from oracle import densecap_oracle as O
    Hd = Wt["lstm_w"].shape[1] // 4
    D = Wt["lstm_w"].shape[0] - Hd
    Wx = Wt["lstm_w"][:D]; Wh = Wt["lstm_w"][D:]
    words = torch.from_numpy(np.asarray(tok, np.int64))
    h2, c2 = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][words - 1] @ Wx, torch.from_numpy(np.ascontiguousarray(h, F32)),
                         torch.from_numpy(np.ascontiguousarray(c, F32)), Wh)
    lp = O._log_softmax_thnn((h2 @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy())
    return h2.numpy(), c2.numpy(), lp


def std_walk(codes, Wt, T, beam, variant=None):
    """The standard search on codes (N, fc_dim) in fp32.  Returns dict(
      lp0 (N, V1)   log-probabilities of the first step;  h0, c0 (N, Hd) the state of the START step,
      first         the state iteration t = 1 reads: dict(h, c, beam_lp, beams, len, tok, parent, fin), (N, beam, ...),
      steps         {t: dict(state=<what iteration t reads>, lp (N, beam, V1) unmasked log-probabilities of the step, top_lp,
                     top_idx (N, beam, beam) the lists under the finished mask, h_post, c_post (N, beam, Hd) the LSTM state after
                     the step, before the re-indexing, next=<what iteration t + 1 reads>)},
      final         the last state).
    variant: None, or one of three WRONG searches for the tests that show the rules have teeth -- "h_from_c" (the hidden state
    of every hypothesis starts from the cell state), "flood" (a finished parent contributes all its candidates), "ones"
    (columns without a word hold 1)."""
    import torch
    from oracle import densecap_oracle as O
    assert variant in (None, "h_from_c", "flood", "ones")
    codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=F32))
    N = codes.shape[0]
    Hd = Wt["lstm_w"].shape[1] // 4
    D = Wt["lstm_w"].shape[0] - Hd
    Wx = Wt["lstm_w"][:D]; Wh = Wt["lstm_w"][D:]
    V1 = Wt["lm_out_w"].shape[0]
    END = V1
    enc = torch.relu(codes @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"])
    h, c = O.lstm_step(Wt["lstm_b"] + enc @ Wx, torch.zeros(N, Hd), torch.zeros(N, Hd), Wh)
    h0, c0, lp0 = _lm_rows(Wt, np.full(N, V1), h.numpy(), c.numpy())
    top_lp, order = O._topk_sorted(lp0, beam)
    state = std_init_ref(top_lp, (order + 1).astype(np.int32), T, END)
    if variant == "ones":
        state["beams"][:, :, 1:] = 1
    state["c"] = np.repeat(c0[:, None, :], beam, axis=1)
    state["h"] = state["c"].copy() if variant == "h_from_c" else np.repeat(h0[:, None, :], beam, axis=1)
    out = dict(lp0=lp0, h0=h0, c0=c0, first=state, steps={})
    for t in range(1, T):
        h_post, c_post, lp = _lm_rows(Wt, state["tok"].reshape(-1), state["h"].reshape(N * beam, Hd), state["c"].reshape(N * beam, Hd))
        masked = lp * (1 - state["fin"].reshape(-1).astype(F32))[:, None]
        tl, order = O._topk_sorted(masked, beam)
        tl = (tl.astype(F32) + F32(0)).reshape(N, beam, beam)                 # + 0: the -0 of lp * 0 is the device's +0
        ti = (order + 1).astype(np.int32).reshape(N, beam, beam)
        nxt = std_merge_ref(tl, ti, state["beam_lp"], state["beams"], state["len"], state["fin"], t, END, flood=variant == "flood")
        h_post = h_post.reshape(N, beam, Hd); c_post = c_post.reshape(N, beam, Hd)
        par = nxt["parent"][:, :, None].astype(np.int64)
        nxt["h"] = np.take_along_axis(h_post, par, 1)
        nxt["c"] = np.take_along_axis(c_post, par, 1)
        out["steps"][t] = dict(state=state, lp=lp.reshape(N, beam, V1), top_lp=tl, top_idx=ti, h_post=h_post, c_post=c_post, next=nxt)
        state = nxt
    out["final"] = state
    return out


def std_search(walk, n_best, alpha):
    """(captions, logprob) of a walk: std_finish_ref of its last state."""
    f = walk["final"]
    return std_finish_ref(f["beam_lp"], f["beams"], f["len"], n_best, alpha)


# ---- the rules -----------------------------------------------------------------------------------------------------------------
MERGE_OUT = ("beam_lp", "beams", "len", "parent", "tok", "fin")


def check_start(state, top_lp, top_idx, walk, T, END, tol, rel, what=""):
    """The start of a search against a walk: the first lists rank-wise, the first expansion bit for bit on its own lists, every
    hypothesis's h within `rel` of the START step's h (NOT its c) and its c of the START step's c, rows of a proposal bit-equal."""
    from tests import parity
    v, s, n = R.check_lists(top_lp, top_idx, walk["lp0"], None, tol, what)
    R.check_same({k: state[k] for k in MERGE_OUT}, std_init_ref(top_lp, top_idx, T, END), what)
    R.check_gather(state["h"], state["c"], state["parent"], walk["h0"][:, None, :], walk["c0"][:, None, :], rel, what)
    far = parity.row_rel_err(walk["h0"], walk["c0"])
    assert far > 100 * rel, "%s: the START step's h and c are too close (%.3g) to tell a state seeded from c" % (what, far)
    return v, s, n


def check_step(out, top_lp, top_idx, fed, st, t, END, tol, rel, what=""):
    """One step fed `fed` (a walk's state) against that walk's step `st`: the lists rank-wise against the walk's
    log-probabilities, the merge bit for bit on the step's own lists, the re-indexed state within `rel` at the step's own parents.
    Returns (worst value difference, worst rank slack, live lists)."""
    nb = top_idx.shape[0] * top_idx.shape[1]
    beam = top_idx.shape[2]
    v, s, n = R.check_lists(top_lp.reshape(nb, beam), top_idx.reshape(nb, beam), st["lp"], fed["fin"], tol, what)
    R.check_same({k: out[k] for k in MERGE_OUT},
                 std_merge_ref(top_lp, top_idx, fed["beam_lp"], fed["beams"], fed["len"], fed["fin"], t, END), what)
    R.check_gather(out["h"], out["c"], out["parent"], st["h_post"], st["c_post"], rel, what)
    return v, s, n


def check_finish(caps, logprob, beam_lp, beams, length, n_best, alpha, what=""):
    """The final ranking of a device against its own inputs.  alpha == 0: std_finish_ref bit for bit.  alpha > 0, rank-wise: every
    output is one of the proposal's hypotheses (its row -- zeros under a NaN lp -- and its lp bits), none used twice, and scores, by
    the reference's table, within 2^-22 relative of the score that belongs at its rank (NaN where that is NaN)."""
    beam_lp = np.asarray(beam_lp, F32); beams = np.asarray(beams, np.int32); length = np.asarray(length, np.int32)
    nprop, beam, T = beams.shape
    assert caps.shape == (nprop, n_best, T) and caps.dtype == np.int32 and logprob.shape == (nprop, n_best) and logprob.dtype == F32
    want_caps, want_lp = std_finish_ref(beam_lp, beams, length, n_best, alpha)
    if float(alpha) == 0.0:
        R.check_same(dict(captions=caps, logprob=logprob), dict(captions=want_caps, logprob=want_lp), what)
        return 0.0
    sc = std_scores(beam_lp, length, T, alpha)
    ranked = np.take_along_axis(sc, std_order(sc, alpha), 1)
    rows = np.where(np.isnan(beam_lp)[:, :, None], 0, beams)
    worst = 0.0
    for p in range(nprop):
        used = np.zeros(beam, bool)
        for r in range(n_best):
            same = (beam_lp[p].view(np.uint32) == logprob[p, r].view(np.uint32)) & (rows[p] == caps[p, r]).all(axis=1) & ~used
            assert same.any(), "%s: proposal %d rank %d: (%r, %s) is not a hypothesis of the proposal (or is used twice)" % (
                what, p, r, logprob[p, r], caps[p, r].tolist())
            # among bit-equal twins the one whose score is nearest the rank's
            cands = np.nonzero(same)[0]
            want = ranked[p, r]
            if np.isnan(want):
                b = cands[np.isnan(sc[p, cands])][:1]
                assert len(b), "%s: proposal %d rank %d: a number where the rank holds NaN" % (what, p, r)
                used[b[0]] = True
                continue
            ok = cands[~np.isnan(sc[p, cands])]
            assert len(ok), "%s: proposal %d rank %d: NaN where the rank holds %r" % (what, p, r, want)
            err = np.abs(sc[p, ok].astype(np.float64) - float(want))
            b = ok[int(np.argmin(err))]
            used[b] = True
            bound = RANK_REL * abs(float(want))
            assert err.min() <= bound, "%s: proposal %d rank %d: hypothesis %d scores %.9g, the rank holds %.9g (off by %.3g > %.3g)" % (
                what, p, r, b, sc[p, b], want, err.min(), bound)
            worst = max(worst, float(err.min() / max(abs(float(want)), 1e-30)))
    return worst
