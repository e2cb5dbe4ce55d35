"""The caption sampling definition (docs/SEMANTICS.md, "Sampling captions") restated on the CPU from the oracle's own pieces:
O.lstm_step for the LSTM and O._log_softmax_thnn for the log-probabilities, Philox4x32-10 and the Gumbel transform in numpy
(float64).  Used by tests/test_sample_captions_cpu.py and tests/test_gpu_sample.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The Random123 function on broadcastable uint32 counters and python-int keys -> four uint32 arrays."""
    c0, c1, c2, c3 = [np.asarray(c).astype(np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def noise_bits(seed, s, r, t, v):
    """bits of (seed, draw s, region row r, step t (1-based), column v (0-based)): word v & 3 of the call with counter
    (v >> 2, t, r, s) and key (seed & 0xffffffff, seed >> 32)."""
    s, r, t, v = np.broadcast_arrays(np.asarray(s, np.uint32), np.asarray(r, np.uint32), np.asarray(t, np.uint32),
                                     np.asarray(v, np.uint32))
    w = philox4x32_10(v >> np.uint32(2), t, r, s, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.choose(v & np.uint32(3), w)


def uniform(bits):
    """u = ((bits >> 9) + 0.5) * 2^-23 in float64 (the value is exact in fp32 too)."""
    return ((np.asarray(bits, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(bits):
    """g = -log(-log(u)) in float64, the inner logarithm as log1p(-(1 - u))."""
    u = uniform(bits)
    return -np.log(-np.log1p(-(1.0 - u)))


def lm_sample_n(codes, Wt, num_samples, temperature=1.0, seed=0, row_ids=None, forced=None, steps=None):
    """codes (n, D) float32 -> dict of
      choice  (n, S, T) int: the restatement's word at every step (1 + argmax of the perturbed scores, lower column on ties),
      samples (n, S, T) int32: the output rows (the words fed, up to and including the first END, zeros after it),
      logprob (n, S) float64: sum over t <= t_end of LogSoftMax(scores_t)[word fed at t],
      gap     (n, S, T): best minus second-best perturbed score of every decision,
      best    (n, S, T): the best perturbed score,  fed_score (n, S, T): the perturbed score of the word fed.
    The words fed to the LSTM are the restatement's own, or `forced` (n, S, T) (teacher forcing: a departure cannot cascade).
    temperature 0: no noise, no scaling.  steps: stop after that many steps (default T = all of them)."""
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
    # rows: s * n + i, as the device packs them.  The state before step 1 does not depend on s; it is still computed on all
    # n * S rows, and a word's input gates as the one-row product score_restatement.lm_score forms, so that every matrix
    # product here has the shape it has there on the same rows: the two restatements then agree bit for bit.
    codes = codes.repeat(S, 1)
    R = n * S
    enc = torch.relu(codes @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"])
    h, c = O.lstm_step(Wt["lstm_b"] + enc @ Wx, torch.zeros(R, Hd), torch.zeros(R, Hd), Wh)    # image step
    h, c = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][V1 - 1][None] @ Wx, h, c, Wh)              # START (id V+1)
    xg_rows = {}

    def x_gates(words):
        for y in np.unique(words):
            if int(y) not in xg_rows:
                xg_rows[int(y)] = Wt["lstm_b"] + Wt["lm_emb"][int(y) - 1][None] @ Wx
        return torch.cat([xg_rows[int(y)] for y in words], 0)
    rr = np.tile(rid, S)[:, None]
    ss = np.repeat(np.arange(S), n)[:, None]
    vv = np.arange(V1)[None, :]
    inv_t = np.float64(np.float32(1.0) / np.float32(temperature)) if temperature != 0 else None
    choice = np.zeros((R, T), np.int64); gap = np.zeros((R, T)); best = np.zeros((R, T)); fed_score = np.zeros((R, T))
    fed = np.zeros((R, T), np.int64); lp_fed = np.zeros((R, T))
    fz = None if forced is None else np.asarray(forced).transpose(1, 0, 2).reshape(R, -1)
    for t in range(1, T + 1):
        scores = (h @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy()
        pert = scores.astype(np.float64)
        if inv_t is not None:
            pert = pert * inv_t + gumbel(noise_bits(seed, ss, rr, t, vv))
        order = np.argsort(-pert, axis=1, kind="stable")[:, :2]
        tok = order[:, 0] + 1
        rows = np.arange(R)
        choice[:, t - 1] = tok
        best[:, t - 1] = pert[rows, order[:, 0]]
        gap[:, t - 1] = pert[rows, order[:, 0]] - pert[rows, order[:, 1]]
        f = tok if fz is None else np.where(fz[:, t - 1] > 0, fz[:, t - 1], tok)     # past a forced row's END: its own word
        fed[:, t - 1] = f
        fed_score[:, t - 1] = pert[rows, f - 1]
        lp_fed[:, t - 1] = O._log_softmax_thnn(scores)[rows, f - 1].astype(np.float64)
        if t < T:
            h, c = O.lstm_step(x_gates(f), h, c, Wh)
    samples = np.zeros((R, T), np.int32); logprob = np.zeros(R)
    for i in range(R):
        ends = np.nonzero(fed[i] == V1)[0]
        te = int(ends[0]) + 1 if len(ends) else T
        samples[i, :te] = fed[i, :te]
        for t in range(te):                      # one double sum per row in step order
            logprob[i] += lp_fed[i, t]
    back = lambda a: a.reshape(S, n, -1).transpose(1, 0, 2)
    return dict(choice=back(choice), samples=back(samples), logprob=logprob.reshape(S, n).T.copy(), gap=back(gap),
                best=back(best), fed_score=back(fed_score))
