"""Truncated caption sampling (docs/SEMANTICS.md, "Truncation: top-k and nucleus") restated on the CPU in float64, and the
decision rule the GPU tests hold the device to.  Built on tests/sample_restatement.py (Philox, Gumbel, the LSTM pieces).
Used by tests/test_sample_trunc_cpu.py, tests/test_gpu_sample_trunc_kernel.py and tests/test_gpu_sample_trunc.py."""
import numpy as np

from tests import sample_restatement as R

STAGE = 1e-4          # the project's bound for a continuous stage against the oracle (tests/parity.py::strict_check)
NOISE = 1e-5          # the bound of the device's g against float64 (tests/test_gpu_sample.py::test_noise_function)
BAND = 1e-9           # a nucleus cut may differ from the float64 one only where some |C_j - p Z| <= BAND * Z


def inv_temperature(temperature):
    """1 / temperature as the device forms it: one fp32 division."""
    return np.float64(np.float32(1.0) / np.float32(temperature))


def scaled(x, temperature):
    """y = x * (1 / temperature): the fp32 product, as float64."""
    return (np.asarray(x, np.float32) * np.float32(inv_temperature(temperature))).astype(np.float64)


def rank_order(x):
    """Candidate columns (a NaN is never one) by x descending, the lower column first among equal values."""
    x = np.asarray(x, np.float32)
    cand = np.nonzero(~np.isnan(x))[0]
    return cand[np.argsort(-x[cand].astype(np.float64), kind="stable")]


def kept_set(x, temperature, top_k=0, top_p=1.0, detail=False):
    """The kept columns of one row in rank order, exactly as defined, or None for a row without a word (no candidate, or a
    first-ranked score -- raw or scaled -- that is not finite).  detail: (kept, order, C, Z, p) with C the float64 cumulative
    masses of the top-k survivors in rank order."""
    x = np.asarray(x, np.float32)
    order = rank_order(x)
    if len(order) == 0 or not np.isfinite(x[order[0]]):
        return (None, order, None, None, None) if detail else None
    y = scaled(x, temperature)
    if not np.isfinite(y[order[0]]):
        return (None, order, None, None, None) if detail else None
    K = min(int(top_k), len(order)) if top_k else len(order)
    surv = order[:K]
    with np.errstate(over="ignore"):
        q = np.exp(y[surv] - y[surv[0]])
    C = np.cumsum(q)                        # float64, rank order
    Z = C[-1]
    p = np.float64(np.float32(top_p))
    m = K if p >= 1.0 else int(np.argmax(C >= p * Z)) + 1        # the smallest j with C_j >= p Z (C_K = Z: one exists)
    kept = surv[:m]
    return (kept, order, C, Z, p) if detail else kept


def log_softmax_at(x, col):
    """LogSoftMax over the candidates of the row at `col`, in float64 (a row without a NaN: nn.LogSoftMax)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    c = x[~np.isnan(x)]
    return x[col] - (c.max() + np.log(np.exp(c - c.max()).sum()))


def log_q_at(x, temperature, kept, col):
    """log-probability of `col` under the distribution over `kept` at the temperature, in float64."""
    y = scaled(x, temperature)
    top = y[kept].max()
    return (y[col] - top) - np.log(np.exp(y[kept] - top).sum())


def wide_narrow(x, temperature, top_k, top_p, delta):
    """(wide, narrow) boolean masks over the columns: kept under SOME / under EVERY perturbation of the scores within delta
    (masses then move by the relative eps = 2 delta / temperature; two scores compare differently only within 2 delta)."""
    x = np.asarray(x, np.float32)
    xs = x.astype(np.float64)
    V1 = len(xs)
    cand = ~np.isnan(xs)
    kept, order, C, Z, p = kept_set(x, temperature, top_k, top_p, detail=True)
    if kept is None:
        return np.zeros(V1, bool), np.zeros(V1, bool)
    eps = 2.0 * delta / temperature
    nc = len(order)
    K = min(int(top_k), nc) if top_k else nc
    xo = xs[order]                                        # descending
    asc = xo[::-1]
    # per column: how many OTHER candidates are certainly ahead (x_u > x_v + 2 delta) / possibly ahead (x_u >= x_v - 2 delta)
    certain = nc - np.searchsorted(asc, xs + 2 * delta, side="right")
    possible = nc - np.searchsorted(asc, xs - 2 * delta, side="left") - 1
    if delta == 0.0:                                      # exact scores: the rank itself, ties by the lower column
        rank = np.empty(V1, np.int64); rank[order] = np.arange(nc)
        certain = possible = np.where(cand, rank, nc)
    wide_k = cand & (certain < K)
    narrow_k = cand & (possible < K)
    if np.float64(np.float32(top_p)) >= 1.0:
        return wide_k, narrow_k
    y = scaled(x, temperature)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.where(cand, np.exp(y - y[order[0]]), 0.0)
    qo = q[order]
    pre = np.concatenate([[0.0], np.cumsum(qo)])          # pre[j] = mass of the first j ranks
    exact_k = np.zeros(V1, bool); exact_k[order[:K]] = True
    z_hi = (Z + q[wide_k & ~exact_k].sum()) * (1 + eps)
    z_lo = (Z - q[exact_k & ~narrow_k].sum()) * (1 - eps)
    before_lo = pre[np.minimum(certain, K)] * (1 - eps)   # the mass that is ahead of the column whatever the perturbation
    # `possible` counts others with x_u >= x_v - 2 delta: the first possible + 1 ranks hold them and the column itself
    before_hi = (pre[np.minimum(possible + 1, nc)] - q) * (1 + eps)
    if delta == 0.0:
        before_lo = before_hi = pre[np.minimum(certain, nc)]
        z_hi = z_lo = Z
        wide_p = narrow_p = before_lo < p * Z
    else:
        wide_p = before_lo < p * z_hi
        narrow_p = before_hi < p * z_lo
    return wide_k & wide_p, narrow_k & narrow_p & cand


def decide(x, pert, word, temperature, top_k, top_p, delta=2 * STAGE, margin=None):
    """The decision rule for a device word (1-based) on a row whose restated scores are x and perturbed scores pert:
    returns (ok, why).  The word must lie in the wide kept set -- nothing excuses one outside -- and its perturbed score
    must be within `margin` of the best over the narrow set."""
    if margin is None:
        margin = 2 * (STAGE / temperature + NOISE)
    wide, narrow = wide_narrow(x, temperature, top_k, top_p, delta)
    d = int(word) - 1
    if d < 0 or d >= len(wide) or not wide[d]:
        return False, "outside the wide kept set"
    if narrow.any() and pert[narrow].max() - pert[d] > margin:
        return False, "perturbed score %.6g below the best of the narrow set by more than %.3g" % (pert[narrow].max() - pert[d], margin)
    return True, ""


def lm_sample_n_trunc(codes, Wt, num_samples, temperature=1.0, seed=0, top_k=0, top_p=1.0, row_ids=None, forced=None, steps=None,
                      chooser=None):
    """tests/sample_restatement.py::lm_sample_n with truncation: codes (n, D) -> dict of
      choice (n, S, T): 1 + argmax of the perturbed scores over the kept set (lower column on ties; 0 = no word),
      samples (n, S, T) int32, logprob / sample_logprob (n, S) float64 (sums over t <= t_end in step order),
      scores (n, S, T, V1) float32 and pert (n, S, T, V1) float64: every step's scores and perturbed scores.
    forced (n, S, T): the words fed (teacher forcing); chooser(x, pert, kept) -> column: another choice rule (the CPU tests'
    wrong samplers)."""
    import torch
    from oracle import densecap_oracle as O
    codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float32))
    n, S = codes.shape[0], int(num_samples)
    Hd = Wt["lstm_w"].shape[1] // 4
    E = Wt["lstm_w"].shape[0] - Hd
    Wx, Wh = Wt["lstm_w"][:E], Wt["lstm_w"][E:]
    V1 = Wt["lm_out_w"].shape[0]
    T = int(steps or Wt["seq_length"])
    rid = np.arange(n) if row_ids is None else np.asarray(row_ids)
    codes = codes.repeat(S, 1)                 # rows: s * n + i, as the device packs them
    Rn = n * S
    enc = torch.relu(codes @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"])
    h, c = O.lstm_step(Wt["lstm_b"] + enc @ Wx, torch.zeros(Rn, Hd), torch.zeros(Rn, Hd), Wh)
    h, c = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][V1 - 1][None] @ Wx, h, c, Wh)
    xg_rows = {}

    def x_gates(words):
        for y in np.unique(words):
            if int(y) not in xg_rows:
                xg_rows[int(y)] = Wt["lstm_b"] + Wt["lm_emb"][int(y) - 1][None] @ Wx
        return torch.cat([xg_rows[int(y)] for y in words], 0)
    rr = np.tile(rid, S)[:, None]
    ss = np.repeat(np.arange(S), n)[:, None]
    vv = np.arange(V1)[None, :]
    inv_t = inv_temperature(temperature)
    choice = np.zeros((Rn, T), np.int64); fed = np.zeros((Rn, T), np.int64)
    lp = np.zeros((Rn, T)); lq = np.zeros((Rn, T))
    all_scores = np.zeros((Rn, T, V1), np.float32); all_pert = np.zeros((Rn, T, V1))
    fz = None if forced is None else np.asarray(forced).transpose(1, 0, 2).reshape(Rn, -1)
    for t in range(1, T + 1):
        scores = (h @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy()
        pert = scaled(scores, temperature) + R.gumbel(R.noise_bits(seed, ss, rr, t, vv))
        all_scores[:, t - 1] = scores; all_pert[:, t - 1] = pert
        for i in range(Rn):
            kept = kept_set(scores[i], temperature, top_k, top_p)
            if chooser is not None:
                col = chooser(scores[i], pert[i], kept)
            else:
                ks = np.sort(kept)
                col = int(ks[np.argmax(pert[i, ks])])            # first maximum in column order
            choice[i, t - 1] = col + 1
            f = col + 1 if fz is None or fz[i, t - 1] <= 0 else int(fz[i, t - 1])
            fed[i, t - 1] = f
            lp[i, t - 1] = log_softmax_at(scores[i], f - 1)
            lq[i, t - 1] = log_q_at(scores[i], temperature, kept, f - 1)
        if t < T:
            h, c = O.lstm_step(x_gates(fed[:, t - 1]), h, c, Wh)
    samples = np.zeros((Rn, T), np.int32); logprob = np.zeros(Rn); slogprob = np.zeros(Rn)
    for i in range(Rn):
        ends = np.nonzero(fed[i] == V1)[0]
        te = int(ends[0]) + 1 if len(ends) else T
        samples[i, :te] = fed[i, :te]
        for t in range(te):                      # one double sum per row in step order
            logprob[i] += lp[i, t]
            slogprob[i] += lq[i, t]
    back = lambda a: a.reshape((S, n) + a.shape[1:]).swapaxes(0, 1)
    return dict(choice=back(choice), samples=back(samples), logprob=logprob.reshape(S, n).T.copy(),
                sample_logprob=slogprob.reshape(S, n).T.copy(), scores=back(all_scores), pert=back(all_pert))


def check_words(dev, ref, temperature, top_k, top_p, end, delta=2 * STAGE):
    """Every device word up to its row's end against the restatement `ref` that was fed the device's words: asserts the
    decision rule, returns (decisions, decisions whose word is not the restatement's own choice)."""
    total = needed = 0
    n, S, T = dev.shape
    for i in range(n):
        for s in range(S):
            e = np.nonzero(dev[i, s] == end)[0]
            te = int(e[0]) + 1 if len(e) else T
            total += te
            for t in range(te):
                if dev[i, s, t] == ref["choice"][i, s, t]:
                    continue
                needed += 1
                ok, why = decide(ref["scores"][i, s, t], ref["pert"][i, s, t], dev[i, s, t], temperature, top_k, top_p, delta)
                assert ok, (i, s, t, int(dev[i, s, t]), int(ref["choice"][i, s, t]), why)
    return total, needed


# ---- the reference of the kernel test: one row's cut, and where a nucleus cut may be excused ----------------------------------
def row_reference(x, temperature, top_k, top_p):
    """dict(kept = count or -1, theta = raw score of the last kept rank, cols = kept columns in rank order, band = (lo, hi):
    the kept counts a device may report -- more than one only where some |C_j - p Z| <= BAND * Z)."""
    kept, order, C, Z, p = kept_set(x, temperature, top_k, top_p, detail=True)
    if kept is None:
        return dict(kept=-1, theta=np.nan, cols=None, band=(-1, -1), order=order)
    m = len(kept)
    lo = hi = m
    if p < 1.0:
        near = np.nonzero(np.abs(C - p * Z) <= BAND * Z)[0]           # ranks (0-based) whose cumulative mass sits in the band
        if len(near):
            lo, hi = min(m, int(near.min()) + 1), max(m, int(near.max()) + 2)
            hi = min(hi, len(C))
    return dict(kept=m, theta=np.float32(x[kept[-1]]), cols=kept, band=(lo, hi), order=order)
