"""The beam search step by step (test infrastructure for tests/test_gpu_beam.py and tests/test_beam_rules_cpu.py).

LM:beamsearch (LanguageModel.lua:170-290) is a loop of four row operations between two GEMMs.  Here each of them is restated on
numpy arrays for ALL proposals at once, in the layout of the device (rows = proposal x beam), so that a kernel or a whole step
can be compared with it on its own:

  topk_ref    LogSoftMax (oracle._log_softmax_thnn) + stable top-k, lower index first, with the finished mask
  init_ref    the first expansion
  merge_ref   fp32 top_lp + beam_lp, stable top-`beam`, parent = flat // beam, beams re-indexed with column t set
  oracle_walk the oracle's own trajectory, every step recorded: chained, the restatements ARE oracle.lm_beamsearch (asserted in
              test_beam_rules_cpu.py), so a step checked against them is checked against the oracle

and the rule a device step must meet is written once (check_lists / check_merge / check_gather).  The rule is rank-wise, so it
needs no excuse for a near tie: a list passes if every entry is, by the oracle's own numbers, within 2 x TOKEN_TOL of the entry
that belongs at its rank -- either order of a near tie passes, a wrong pick does not.  Nothing here skips a row, a step or a rank.
"""
import numpy as np

F32 = np.float32


# ---- the restatements --------------------------------------------------------------------------------------------------------
def topk_ref(logits, k, finished=None):
    """(top_lp (rows, k) float32, top_idx (rows, k) int32 1-based, lp (rows, V1) float32) of logits (rows, V1): THNN's LogSoftMax,
    finished rows multiplied by 0 (LanguageModel.lua:243-247), torch.topk with the lower index first among equal values."""
    from oracle import densecap_oracle as O
    lp = O._log_softmax_thnn(np.asarray(logits, F32))
    masked = lp
    if finished is not None:
        masked = lp * (1 - np.asarray(finished, F32))[:, None]
    top_lp, order = O._topk_sorted(masked, k)
    return top_lp.astype(F32) + F32(0), (order + 1).astype(np.int32), lp       # + 0: the -0 of lp * 0 is the device's +0


def init_ref(top_lp, top_idx, T, END):
    """The first expansion (:207-214) from the first step's lists (nprop, beam): dict(beam_lp, beams, parent, tok, fin)."""
    nprop, beam = top_idx.shape
    beams = np.ones((nprop, beam, T), np.int32)
    beams[:, :, 0] = top_idx
    return dict(beam_lp=np.asarray(top_lp, F32).copy(), beams=beams, parent=np.zeros((nprop, beam), np.int32),
                tok=np.asarray(top_idx, np.int32).copy(), fin=(top_idx == END).astype(np.uint8))


def merge_ref(top_lp, top_idx, beam_lp, beams, t, END):
    """The merge of step t (:249-264): top_lp / top_idx (nprop, beam, beam), beam_lp (nprop, beam), beams (nprop, beam, T) ->
    dict(beam_lp, beams, parent, tok, fin).  Sums in fp32, stable order: the lower flat index first among equal sums."""
    top_lp = np.asarray(top_lp, F32); beam_lp = np.asarray(beam_lp, F32)
    nprop, beam, T = beams.shape
    cand = (top_lp + beam_lp[:, :, None]).astype(F32).reshape(nprop, beam * beam)
    flat = np.argsort(-cand.astype(np.float64), axis=1, kind="stable")[:, :beam]
    parent = (flat // beam).astype(np.int32)
    word = np.take_along_axis(np.asarray(top_idx, np.int32).reshape(nprop, beam * beam), flat, 1)
    new = np.take_along_axis(np.asarray(beams, np.int32), parent[:, :, None], 1).copy()
    new[:, :, t] = word
    return dict(beam_lp=np.take_along_axis(cand, flat, 1), beams=new, parent=parent, tok=word.astype(np.int32),
                fin=(new == END).any(axis=2).astype(np.uint8))


# ---- the oracle's trajectory ---------------------------------------------------------------------------------------------------
def oracle_walk(codes, Wt, T, beam):
    """The oracle's beam search on codes (N, fc_dim), proposal by proposal with the oracle's own functions (lstm_step,
    _log_softmax_thnn) and the restatements above for the row operations.  Returns dict(
      lp0 (N, V1)              log-probabilities of the first step,   c0 (N, Hd) the cell state of the START step,
      first                    the state the iteration t = 1 reads: dict(h, c, beam_lp, beams, tok, parent, fin), (N, beam, ...),
      steps                    {t: dict(state=<what iteration t reads>, lp (N, beam, V1) unmasked log-probabilities of the step,
                                        h_post, c_post (N, beam, Hd) the LSTM state after the step, before the re-indexing,
                                        next=<what iteration t + 1 reads>)},
      seq (N, T)               beams[:, 0] of the last state).
    All fp32, exactly the numbers oracle.lm_beamsearch goes through."""
    import torch
    from oracle import densecap_oracle as O
    codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=F32))
    N = codes.shape[0]
    Hd = Wt["lstm_w"].shape[1] // 4
    D = Wt["lstm_w"].shape[0] - Hd
    Wx = Wt["lstm_w"][:D]; Wh = Wt["lstm_w"][D:]
    V1 = Wt["lm_out_w"].shape[0]
    END = V1
    lp0 = np.zeros((N, V1), F32); c0 = np.zeros((N, Hd), F32)
    for i in range(N):
        enc = torch.relu(codes[i:i + 1] @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"])
        h = torch.zeros(1, Hd); c = torch.zeros(1, Hd)
        h, c = O.lstm_step(Wt["lstm_b"] + enc @ Wx, h, c, Wh)
        start = torch.full((1,), V1, dtype=torch.int64)
        h, c = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][start - 1] @ Wx, h, c, Wh)
        lp0[i] = O._log_softmax_thnn((h @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy())[0]
        c0[i] = c.numpy()[0]
    top_lp, order = O._topk_sorted(lp0, beam)
    state = init_ref(top_lp, (order + 1).astype(np.int32), T, END)
    state["c"] = np.repeat(c0[:, None, :], beam, axis=1)
    state["h"] = state["c"].copy()                                            # :221-226: h starts from the CELL state
    out = dict(lp0=lp0, c0=c0, first=state, steps={})
    for t in range(1, T):
        lp = np.zeros((N, beam, V1), F32)
        h_post = np.zeros((N, beam, Hd), F32); c_post = np.zeros((N, beam, Hd), F32)
        for i in range(N):
            words = torch.from_numpy(state["tok"][i].astype(np.int64))
            h, c = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][words - 1] @ Wx, torch.from_numpy(state["h"][i]),
                               torch.from_numpy(state["c"][i]), Wh)
            lp[i] = O._log_softmax_thnn((h @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy())
            h_post[i] = h.numpy(); c_post[i] = c.numpy()
        masked = lp * (1 - state["fin"].astype(F32))[:, :, None]
        tl, order = O._topk_sorted(masked, beam)
        nxt = merge_ref(tl.astype(F32) + F32(0), (order + 1).astype(np.int32), state["beam_lp"], state["beams"], t, END)
        nxt["h"] = np.take_along_axis(h_post, nxt["parent"][:, :, None].astype(np.int64), 1)
        nxt["c"] = np.take_along_axis(c_post, nxt["parent"][:, :, None].astype(np.int64), 1)
        out["steps"][t] = dict(state=state, lp=lp, h_post=h_post, c_post=c_post, next=nxt)
        state = nxt
    out["seq"] = state["beams"][:, 0].astype(np.int64)
    return out


def float64_step(state, Wt, beam):
    """One step recomputed in float64 from the fp32 state (the stand-in for a device in test_beam_rules_cpu.py: another
    arithmetic on the same inputs): (top_lp (N, beam, beam) float32, top_idx int32, h_post, c_post float32)."""
    Hd = Wt["lstm_w"].shape[1] // 4
    D = Wt["lstm_w"].shape[0] - Hd
    w = {k: Wt[k].numpy().astype(np.float64) for k in ("lstm_w", "lstm_b", "lm_emb", "lm_out_w", "lm_out_b")}
    N = state["h"].shape[0]
    h = state["h"].reshape(N * beam, Hd).astype(np.float64); c = state["c"].reshape(N * beam, Hd).astype(np.float64)
    g = w["lstm_b"] + w["lm_emb"][state["tok"].reshape(-1) - 1] @ w["lstm_w"][:D] + h @ w["lstm_w"][D:]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    c2 = sig(g[:, Hd:2 * Hd]) * c + sig(g[:, :Hd]) * np.tanh(g[:, 3 * Hd:])
    h2 = sig(g[:, 2 * Hd:3 * Hd]) * np.tanh(c2)
    x = h2 @ w["lm_out_w"].T + w["lm_out_b"]
    mx = x.max(axis=1, keepdims=True)
    lp = (x - (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))).astype(F32)
    lp = lp * (1 - state["fin"].reshape(-1).astype(F32))[:, None]
    order = np.argsort(-lp.astype(np.float64), axis=1, kind="stable")[:, :beam]
    top_lp = np.take_along_axis(lp, order, 1) + F32(0)
    return (top_lp.reshape(N, beam, beam), (order + 1).astype(np.int32).reshape(N, beam, beam),
            h2.astype(F32).reshape(N, beam, Hd), c2.astype(F32).reshape(N, beam, Hd))


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def check_lists(top_lp, top_idx, lp_oracle, fin, tol, what=""):
    """The top-k lists of one step, (rows, k), against the oracle's log-probabilities (rows, V1) of the same rows:
    finished rows   k zeros, indices 1..k, exactly;
    live rows       indices distinct and in [1, V1]; values non-increasing, equal values in ascending index;
                    |top_lp[q] - lp_oracle[top_idx[q]]| <= tol;  lp_oracle[top_idx[q]] >= (q-th largest of lp_oracle) - 2 tol.
    Every row, every rank.  Returns (worst value difference, worst rank slack, live lists checked)."""
    top_lp = np.asarray(top_lp); top_idx = np.asarray(top_idx)
    rows, k = top_idx.shape
    lp_oracle = np.asarray(lp_oracle, F32).reshape(rows, -1)
    V1 = lp_oracle.shape[1]
    fin = np.zeros(rows, bool) if fin is None else np.asarray(fin).reshape(rows).astype(bool)
    assert top_lp.shape == (rows, k) and top_lp.dtype == F32
    f = np.nonzero(fin)[0]
    assert (top_lp[f] == 0).all(), "%s: a finished row has a non-zero log-probability (rows %s)" % (
        what, f[(top_lp[f] != 0).any(axis=1)][:5].tolist())
    assert (top_idx[f] == np.arange(1, k + 1)).all(), "%s: a finished row's indices are not 1..k (rows %s)" % (
        what, f[(top_idx[f] != np.arange(1, k + 1)).any(axis=1)][:5].tolist())
    live = np.nonzero(~fin)[0]
    if len(live) == 0:
        return 0.0, 0.0, 0
    v, ix, lo = top_lp[live], top_idx[live].astype(np.int64), lp_oracle[live]
    assert not np.isnan(v).any(), "%s: NaN in a live list" % what
    assert ix.min() >= 1 and ix.max() <= V1, "%s: index outside [1, %d]: %d .. %d" % (what, V1, ix.min(), ix.max())
    srt = np.sort(ix, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "%s: an index appears twice in a list (rows %s)" % (
        what, live[(srt[:, 1:] == srt[:, :-1]).any(axis=1)][:5].tolist())
    d = np.diff(v.astype(np.float64), axis=1)
    assert (d <= 0).all(), "%s: values increase within a list (rows %s)" % (what, live[(d > 0).any(axis=1)][:5].tolist())
    tie_bad = (d == 0) & (np.diff(ix, axis=1) <= 0)
    assert not tie_bad.any(), "%s: equal values are not in ascending index (rows %s)" % (what, live[tie_bad.any(axis=1)][:5].tolist())
    at = np.take_along_axis(lo, ix - 1, 1).astype(np.float64)
    val = np.abs(v.astype(np.float64) - at)
    kth = -np.sort(-lo.astype(np.float64), axis=1)[:, :k]
    slack = kth - at
    r, q = np.unravel_index(int(np.argmax(val)), val.shape)
    assert val.max() <= tol, "%s: row %d rank %d: value %.9g, the oracle has %.9g at word %d (difference %.3g > %.3g)" % (
        what, live[r], q, v[r, q], at[r, q], ix[r, q], val[r, q], tol)
    r, q = np.unravel_index(int(np.argmax(slack)), slack.shape)
    assert slack.max() <= 2 * tol, "%s: row %d rank %d: word %d has %.9g by the oracle, the entry of that rank %.9g (%.3g > %.3g)" % (
        what, live[r], q, ix[r, q], at[r, q], kth[r, q], slack[r, q], 2 * tol)
    return float(val.max()), float(max(slack.max(), 0.0)), len(live)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def check_same(got, want, what=""):
    """Every array of `want` bit for bit (fp32 compared as words: no tolerance, -0 is not +0)."""
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: %s has shape %s %s, expected %s %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.argwhere(_bits(g) != _bits(w))
        assert len(bad) == 0, "%s: %s differs at %d places, first %s: %r, expected %r" % (
            what, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def check_merge(out, top_lp, top_idx, beam_lp, beams, t, END, what=""):
    """beam_lp, beams, parent, tok, fin of a merge are merge_ref of its own inputs, bit for bit."""
    check_same(out, merge_ref(top_lp, top_idx, beam_lp, beams, t, END), what)


def check_gather(h, c, parent, h_post, c_post, rel, what=""):
    """The re-indexed state (N, beam, Hd): rows of a proposal with the same parent are bit-equal, and every row is within `rel`
    (parity.row_rel_err) of the oracle's post-step state of its parent.  Returns the two errors."""
    from tests import parity
    N, beam, Hd = h.shape
    parent = np.asarray(parent, np.int64)
    assert parent.min() >= 0 and parent.max() < h_post.shape[1], "%s: parent outside [0, %d)" % (what, h_post.shape[1])
    first = np.argmax(parent[:, :, None] == parent[:, None, :], axis=2)          # the first row with the same parent
    for name, a in (("h", h), ("c", c)):
        twin = np.take_along_axis(a, first[:, :, None], 1)
        assert (_bits(a) == _bits(twin)).all(), "%s: %s rows with the same parent differ" % (what, name)
    eh = parity.row_rel_err(h.reshape(N * beam, Hd), np.take_along_axis(h_post, parent[:, :, None], 1).reshape(N * beam, Hd))
    ec = parity.row_rel_err(c.reshape(N * beam, Hd), np.take_along_axis(c_post, parent[:, :, None], 1).reshape(N * beam, Hd))
    assert eh <= rel and ec <= rel, "%s: state after the step: h %.3g, c %.3g against the oracle's (bound %.3g)" % (what, eh, ec, rel)
    return eh, ec
