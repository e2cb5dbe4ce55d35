"""The rules of the classic decode step in plain numpy: what the step GEMM's three row epilogues (mfma_gemm.hip, v2_tile<.., AMAX,
BF3, LSE>) must write for an array z of fp32 logits, and what the three row tails (elementwise.hip: lstm_step_tail_kernel,
lse_step_tail_kernel, sample_step_tail_kernel) must make of such partials.  tests/test_step_rules_cpu.py holds the rules against
wrong variants; tests/test_gpu_step_gemm.py and tests/test_gpu_step_tails.py hold the kernels against the rules.

Layout: the columns of a row fall into 32-column slots, two per 64-column tile; slot s covers columns [32 s, 32 s + 32), of which
only those below `an` (the real vocabulary) count.  Selections are exact (bit for bit on z); sums are float64.

Entries (docs/SEMANTICS.md, "Rows without a word"): an entry needs v > -inf, so a NaN and a -inf are never entries, a slot without
an entry holds the sentinel column NO_COL, a sentinel is never an entry of the row, and a row without an entry has no word: id 0."""
import numpy as np

NO_COL = 0x7fffffff
NEG_INF = np.float32(-np.inf)


def slots_of(columns):
    """32-column slots of an epilogue over `columns` columns: two for every 64-column tile, whole tiles."""
    return 2 * ((int(columns) + 63) // 64)


def slotted(z, an, slots):
    """z (M, >= an) -> (M, slots, 32) float32: the real columns in their slots, -inf everywhere else."""
    z = np.asarray(z, np.float32)
    p = np.full((z.shape[0], slots * 32), NEG_INF, np.float32)
    p[:, :an] = z[:, :an]
    return p.reshape(z.shape[0], slots, 32)


def _first_max(score, value=None):
    """score (M, S, 32): per (row, slot) the first maximum among the entries (score > -inf; NaN is none) -> (best score, column
    or NO_COL, value at that column); without an entry (-inf, NO_COL, -inf)."""
    ok = score > NEG_INF
    w = np.where(ok, score, NEG_INF)
    j = w.argmax(2)                                           # numpy's argmax returns the FIRST maximum
    has = ok.any(2)
    best = np.where(has, np.take_along_axis(w, j[..., None], 2)[..., 0], NEG_INF).astype(np.float32)
    col = np.where(has, 32 * np.arange(score.shape[1])[None, :] + j, NO_COL).astype(np.int32)
    val = None
    if value is not None:
        val = np.where(has, np.take_along_axis(value, j[..., None], 2)[..., 0], NEG_INF).astype(np.float32)
    return best, col, val


def argmax_partials(z, an, slots):
    """Arg-max partial: (val (M, slots) float32, col (M, slots) int32)."""
    best, col, _ = _first_max(slotted(z, an, slots))
    return best, col


def lse_partials(z, an, slots):
    """Log-sum-exp partial: (max (M, slots) float32, sum exp(v - max) (M, slots) float64), the -inf entries left out; a slot
    without a maximum gives (-inf, 0).  (A NaN is no maximum but does poison its slot's sum.)"""
    p = slotted(z, an, slots)
    mx = np.where(p > NEG_INF, p, NEG_INF).max(2).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(p != NEG_INF, np.exp(p.astype(np.float64) - mx.astype(np.float64)[..., None]), 0.0)
    s = np.where(mx > NEG_INF, e.sum(2), 0.0)
    return mx, s


# Units in the last place granted to the hardware exponential in lse_sum_bound.  The ROCm documentation installed with the compiler
# states none for __expf, so it was measured once on an MI355X: the smallest integer at which the worst err / bound over the fixed
# seeds of tests/test_gpu_step_gemm.py is at most 0.5.  That already holds at 0 (worst 0.191; 0.186 at 1, 0.181 at 2): the 33
# units granted to the additions leave the exponential's own error no room to show.
U_EXP = 0


def lse_sum_bound(z, an, slots, u):
    """How far an fp32 evaluation of a slot's sum may be from lse_partials': per term e = exp(v - max), relative
    (2 |v - max| + u + 1) 2^-24 -- the rounded subtraction and the rounded product with log2(e) inside the fast exponential each
    move the exponent's argument by up to 2^-24 |v - max| (relative to e: the same figure), the hardware exponential is good to
    u units and one more for its result's rounding -- and 33 2^-24 of the sum for the 32 fp32 additions (the terms are
    positive) and the final one between the lane halves.  (M, slots) float64."""
    p = slotted(z, an, slots).astype(np.float64)
    mx = np.where(p > -np.inf, p, -np.inf).max(2)
    with np.errstate(invalid="ignore"):
        d = np.where(p > -np.inf, p - mx[..., None], -np.inf)
        e = np.where(p > -np.inf, np.exp(d), 0.0)
        per = np.where(p > -np.inf, e * (2 * np.abs(d) + u + 1), 0.0)
    return (per.sum(2) + 33 * e.sum(2)) * 2.0 ** -24


def target_logit(z, tgt):
    """z[row, tgt - 1]: the target's biased logit (tgt 1-based)."""
    z = np.asarray(z, np.float32)
    return z[np.arange(z.shape[0]), np.asarray(tgt, np.int64) - 1]


def gumbel_f64(bits):
    """The float64 Gumbel of tests/sample_restatement.py rounded to fp32: what stands in for the device's table without a GPU."""
    from tests import sample_restatement as R
    return R.gumbel(bits).astype(np.float32)


def perturbed(z, an, slots, keys, t, seed, inv_temp, gumbel=gumbel_f64, bits=None):
    """fp32(fp32(v * inv_temp) + g) in the slotted layout; inv_temp == 0: v itself (no noise, no scaling).  g = gumbel(bits) with
    the counter layout of tests/sample_restatement.py: word n & 3 of the call at (n >> 2, t, r, s), (r, s) = keys[row]."""
    from tests import sample_restatement as R
    p = slotted(z, an, slots)
    if float(inv_temp) == 0.0:
        return p
    keys = np.asarray(keys, np.int64)
    M = p.shape[0]
    n = np.arange(slots * 32)[None, :]
    b = (bits or R.noise_bits)(seed, keys[:, 1:2], keys[:, 0:1], t, n)
    g = np.asarray(gumbel(b), np.float32).reshape(M, slots, 32)
    with np.errstate(invalid="ignore", over="ignore"):
        pv = (p * np.float32(inv_temp)).astype(np.float32) + g
    return np.where(np.arange(slots * 32).reshape(1, slots, 32) < an, pv, NEG_INF).astype(np.float32)


def sample_partials(z, an, slots, keys, t, seed, inv_temp, gumbel=gumbel_f64, bits=None):
    """Sampling partial: (max, sum) as lse_partials, then the best perturbed entry (score, col, v), first maximum on ties."""
    mx, s = lse_partials(z, an, slots)
    score, col, v = _first_max(perturbed(z, an, slots, keys, t, seed, inv_temp, gumbel, bits), slotted(z, an, slots))
    return mx, s, score, col, v


def row_merge(val, col):
    """The best entry over a row's slots, the lower column on equal values; a sentinel is never an entry.  val, col (M, slots)
    -> (tok (M,) int: column + 1, 0 = no entry; slot (M,) int: the winning slot, -1 = none).  The epilogue's columns ascend with
    the slot, and so must a caller's."""
    val = np.asarray(val, np.float32)
    col = np.asarray(col, np.int64)
    M = val.shape[0]
    tok = np.zeros(M, np.int64)
    slot = np.full(M, -1, np.int64)
    for m in range(M):
        ent = np.nonzero(col[m] != NO_COL)[0]
        if len(ent) == 0:
            continue
        top = val[m, ent].max()
        tied = ent[val[m, ent] == top]
        s = tied[np.argmin(col[m, tied])]
        tok[m], slot[m] = col[m, s] + 1, s
    return tok, slot


def lse_rows(mx, s):
    """Row log-sum-exp from the partials in float64: M + log(sum_s s_s exp(mx_s - M)), M the largest max; empty slots left out."""
    mx = np.asarray(mx, np.float64)
    s = np.asarray(s, np.float64)
    top = mx.max(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = np.where(mx > -np.inf, s * np.exp(mx - top[:, None]), 0.0).sum(1)
        return top + np.log(tot)


def lstm_update(x, gates_pre, c, zero_c=False):
    """(x + gates_pre), gate order i, f, o, g; c' = f c + i g, h' = o tanh(c') in float64.  x None (or a row of it all None): a row
    without a word adds nothing.  x, gates_pre (n, 4 Hd); c (n, Hd) -> (c', h')."""
    g = np.asarray(gates_pre, np.float64)
    if x is not None:
        g = np.asarray(x, np.float64) + g
    Hd = g.shape[1] // 4
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    i, f, o, gg = (g[:, k * Hd:(k + 1) * Hd] for k in range(4))
    c0 = np.zeros_like(i) if zero_c else np.asarray(c, np.float64)
    c1 = sig(f) * c0 + sig(i) * np.tanh(gg)
    return c1, sig(o) * np.tanh(c1)


def xg_rows_of(xg, tok):
    """The rows of xg the words select, zeros for a row without a word (tok 0)."""
    xg = np.asarray(xg)
    tok = np.asarray(tok, np.int64)
    return np.where((tok > 0)[:, None], xg[np.maximum(tok, 1) - 1], 0.0)


# ---- crafted operands both test modules use ----------------------------------------------------------------------------------------
TIE_SETS = {"c0_1": (0, 1), "c3_4": (3, 4), "c7_8": (7, 8), "c31_32": (31, 32), "c63_64": (63, 64), "c0_2048": (0, 2048),
            "c5_8197": (5, 8197), "c3_4_64": (3, 4, 64)}
# which seam of the first-maximum rule a tie sits on: 1 a lane's registers, 2 the two lane halves (interleaved 4-column runs), 3 the
# two slots of a tile, 4 tiles, 5 a tail thread's slots s and s + 256, 6 the tail's four waves (slot s belongs to thread s mod 256,
# wave (s mod 256) // 64)
TIE_SEAMS = {"c0_1": "seam1", "c3_4": "seam2", "c7_8": "seam2", "c31_32": "seam3", "c63_64": "seam4", "c0_2048": "seam6",
             "c5_8197": "seam5", "c3_4_64": "seam2_4"}


def tie_operands(cols, M, V1, K, seed, rows_extra=0):
    """A (M, K), W (V1 + rows_extra, K), bias: uniform in (-1, 1), the W rows of `cols` identical and their bias 64 -- the tied
    columns are every row's maximum, exactly equal whatever the arithmetic."""
    rng = np.random.default_rng(seed)
    A = (rng.random((M, K), dtype=np.float32) * 2 - 1).astype(np.float32)
    W = (rng.random((V1 + rows_extra, K), dtype=np.float32) * 2 - 1).astype(np.float32)
    bias = (rng.random(V1 + rows_extra, dtype=np.float32) * 2 - 1).astype(np.float32)
    for c in cols[1:]:
        W[c] = W[cols[0]]
    bias[list(cols)] = 64.0
    return A, W, bias


def host_logits(A, W, bias):
    """A stand-in for the device's z where there is no device: the float64 product rounded once."""
    return (np.asarray(A, np.float64) @ np.asarray(W, np.float64).T + np.asarray(bias, np.float64)).astype(np.float32)
