"""The kernels of the screened greedy decode step one at a time, through dc_debug_screen_scores and
dc_debug_rescore_tail (include/densecap_debug.h): the launchers the decode calls, on the loaded weights.

tests/test_gpu_decode_screen.py pins what the route is for -- tokens and LSTM state bit-identical to the fused step -- but the row
tail re-scores its candidates exactly, so a wrong score changes a token only once it leaves the proven bound b, and the device's
scores sit at 0.066 of b.  Here the scores are held to R.score_tol, the error model of the proof with the exact sum of magnitudes
(about 75 times finer than b), one-hot rows pin every (k, column) of the screen bit for bit, the operands hb / hnorm are compared
with their definitions, and the tail's selection is driven with crafted scores to its edges: exactly 64 and 65 candidates, the
chunks of 8 staged rows, the edge of the bound, non-finite scores.

Models come from make_synthetic_weights at fc_dim 256 (no forward runs here; h is supplied directly): the default language-model
dimensions, the five sets of tests/test_gpu_dims.py, and two at the edge of the row tail's LDS rule (Hd 512, E 32, R 32, T 2):
  lds_last   V = 31743: V1pad = 31744, the tail's dynamic LDS is exactly 64 KiB -- the last vocabulary the route takes
  lds_out    V = 31744: V1pad = 31808, the route is declined (both hooks refuse with DC_E_UNSUPPORTED)."""
import numpy as np
import pytest
import torch

from tests import decode_screen_rules as R

pytestmark = pytest.mark.gpu

LDS_SETS = {"lds_last": 31743, "lds_out": 31744}
NAMES = ["default", "minimal", "e_lt_h", "e_gt_h", "odd32", "big_vocab", "lds_last", "lds_out"]
ROWS = (1, 127, 128, 129)
XCD_ROWS = {"minimal": (897, 1025), "e_gt_h": (897, 1025)}     # 8 and 9 row tiles: each XCD owns one / two, seven slots empty
FP16_EDGE = 65520.0                                            # halfway between the largest fp16 and 2^16: from here on, inf
FILL = 0xA5


def screen_set_weights(name):
    """The weights of a set of this module (test_gpu_decode_screen.py loads the lds_* sets through it as well)."""
    from densecap_amd.weights import make_synthetic_weights
    from tests.test_gpu_dims import SETS, set_weights
    if name == "default":
        return make_synthetic_weights(seed=1234, fc_dim=256)
    if name in LDS_SETS:
        return make_synthetic_weights(seed=11, vocab_size=LDS_SETS[name], seq_length=2, rpn_hidden=32, enc_size=32, rnn_size=512,
                                      fc_dim=256)
    assert name in SETS
    return set_weights(name)


class _Set:
    """One loaded model and what the tests share about it (computed once, never modified)."""

    def __init__(self, name):
        from densecap_amd import DenseCapModel
        self.name = name
        self.W = screen_set_weights(name)
        self.m = DenseCapModel(self.W, device=0)
        self.ctx = self.m.ctx
        self.w, self.bias = self.W["lm_out_w"], self.W["lm_out_b"]
        self.V1, self.Hd = self.w.shape
        self.V = self.V1 - 1
        self.Kp, self.V1pad = (self.Hd + 63) // 64 * 64, (self.V1 + 63) // 64 * 64
        self._cache = {}

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def wn(self):
        return self.cached("wn", lambda: R.row_norms_up(self.w))

    def logits(self, h):
        """The fp32 logits of the fused step's family for rows h (dc_op_linear), as the route tests take them."""
        from densecap_amd import ops
        return ops.linear(self.ctx, h, self.w.numpy(), self.bias.numpy())


_LOADED = {}


def _get(name):
    """The set's model, loaded at its first use and kept to the end of the module (eight small models at most)."""
    if name not in _LOADED:
        _LOADED[name] = _Set(name)
    return _LOADED[name]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for s in _LOADED.values():
        s.ctx.close()
    _LOADED.clear()


ROUTE_SETS = [n for n in NAMES if n != "lds_out"]


def _uniform(n, Hd, seed):
    return (np.random.default_rng(seed).random((n, Hd), dtype=np.float32) * 2 - 1).astype(np.float32)


def _untouched(a, what):
    assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all(), "%s was written" % what


# ---- the hooks refuse where the route does not exist ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds_out"])
def test_hooks_refuse_where_the_route_is_declined(name):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    sset = _get(name)
    h = _uniform(2, sset.Hd, 1)
    with pytest.raises(DenseCapError, match=r"\(-5\)"):
        ops.screen_scores(sset.ctx, h, sset.V)
    with pytest.raises(DenseCapError, match=r"\(-5\)"):
        ops.rescore_tail(sset.ctx, np.zeros((2, sset.V1pad), np.float16), h, np.ones(2, np.float32))


def test_hooks_refuse_without_weights():
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    ctx = ops.Context(0)
    try:
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            ops.screen_scores(ctx, _uniform(2, 64, 1), 63)
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            ops.rescore_tail(ctx, np.zeros((2, 64), np.float16), _uniform(2, 64, 1), np.ones(2, np.float32))
    finally:
        ctx.close()


# ---- the screen against the float64 reference ----------------------------------------------------------------------------------
def _screen_inputs(s):
    """(h, ref, tol): uniform rows in (-1, 1) with five special rows at 1..5 -- zeros, +-1, 2^-70, and 2^10 doubled until a
    reference score of that row is past the fp16 range by more than its tolerance -- and their float64 scores and tolerances."""
    def make():
        n = max(ROWS + XCD_ROWS.get(s.name, ()))
        h = _uniform(n, s.Hd, 40)
        rng = np.random.default_rng(41)
        h[1] = 0
        h[2] = rng.integers(0, 2, s.Hd) * 2.0 - 1.0
        h[3] = 2.0 ** -70
        big = None
        for p in range(10, 40):
            row = torch.full((1, s.Hd), 2.0 ** p)
            r, t = R.scores_ref64(row, s.w, s.bias), R.score_tol(row, s.w, s.bias, s.Hd)
            if ((r.abs() - t) > FP16_EDGE).any():
                big = p
                break
        assert big is not None
        h[4] = 2.0 ** big
        h[5] = -h[4]
        ht = torch.from_numpy(h)
        return h, R.scores_ref64(ht, s.w, s.bias).numpy(), R.score_tol(ht, s.w, s.bias, s.Hd).numpy()
    return s.cached("screen_inputs", make)


def _check_scores(s, sc, ref, tol, live, what):
    """sc (rows, V1pad) fp16 against ref / tol (>= live rows, V1): every real column of every live row.  A reference value past
    the fp16 range by more than the tolerance must be that inf; an inf must be within the tolerance of the range's end; every
    other score within the tolerance.  Returns the worst err / tol over the finite scores."""
    dev = sc[:live, :s.V1].astype(np.float64)
    ref, tol = ref[:live], tol[:live]
    assert not np.isnan(dev).any(), what
    inf = np.isinf(dev)
    must = np.abs(ref) - tol > FP16_EDGE
    assert inf[must].all(), "%s: a score past the fp16 range is finite" % what
    assert (np.sign(dev[inf]) == np.sign(ref[inf])).all() and (np.abs(ref[inf]) + tol[inf] >= FP16_EDGE).all(), what
    ratio = np.abs(dev[~inf] - ref[~inf]) / tol[~inf]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "%s: err/tol %.3f at %d elements" % (what, worst, int((ratio > 1).sum()))
    return worst, int(must.sum())


@pytest.mark.parametrize("name", ROUTE_SETS)
def test_screen_scores_against_the_reference(name):
    """|s_dev - ref| <= R.score_tol at 1, 127, 128 and 129 rows (one tile, its last row, two tiles), at 897 and 1025 rows where
    the XCD map owns the row tiles, and at 1025 rows with a device-side count of 900; hb and hnorm of the same launches against
    their definitions; guard rows and rows past the count keep the caller's bytes."""
    from densecap_amd import ops
    s = _get(name)
    h, ref, tol = _screen_inputs(s)
    hb_ref = R.bf16_rne_bits(h)
    norm = np.sqrt((h.astype(np.float64) ** 2).sum(1))
    cases = [(n, None) for n in ROWS + XCD_ROWS.get(s.name, ())] + ([(1025, 900)] if s.name == "e_gt_h" else [])
    worst, infs = 0.0, 0
    for n, n_dev in cases:
        what = "%s rows=%d count=%s" % (s.name, n, n_dev)
        hb, hn, sc = ops.screen_scores(s.ctx, h[:n], s.V, n_dev=n_dev)
        live = n if n_dev is None else min(n, n_dev)
        w, k = _check_scores(s, sc, ref, tol, live, what)
        worst, infs = max(worst, w), max(infs, k)
        np.testing.assert_array_equal(hb[:live, :s.Hd], hb_ref[:live], err_msg=what)
        assert not hb[:live, s.Hd:].any(), what
        assert (hn[:live] >= norm[:live]).all() and (hn[:live] <= 1.002 * norm[:live]).all(), what
        for a, name in ((hb, "hb"), (hn, "hnorm"), (sc, "scores")):
            _untouched(a[live:], "%s: %s past row %d" % (what, name, live))
    assert infs > 0, "no score left the fp16 range: the case tests nothing"
    print("SCREEN_STAT set=%s worst_err_over_tol=%.4f rows=%s" % (s.name, worst, [c[0] for c in cases]))


@pytest.mark.parametrize("name", ["minimal", "default", "e_lt_h", "odd32"])
def test_one_hot_rows_bit_for_bit(name):
    """h = e_k for every k < Hd (Hd rows): the score of column j is exactly fp16(fp32(bias_j + bf16(w_jk))) -- one exact product
    and zeros in the MFMA chain, one fp32 addition, one rounding.  A wrong LDS swizzle, k-to-lane map or register set of the
    three-deep ring, or a padded column Hd..Kp that is not zero, moves a whole (k, column) pattern.  1, 8, 12 and 17 K steps."""
    from densecap_amd import ops
    s = _get(name)
    h = np.eye(s.Hd, dtype=np.float32)
    _, _, sc = ops.screen_scores(s.ctx, h, s.V)
    wb = R.bf16_values(s.w).float().numpy()                                   # (V1, Hd)
    want = (wb.T + s.bias.numpy()[None, :]).astype(np.float32).astype(np.float16)
    np.testing.assert_array_equal(sc[:s.Hd, :s.V1].view(np.uint16), want.view(np.uint16))
    _untouched(sc[s.Hd:], "guard rows")


# ---- the operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROUTE_SETS)
def test_operands_on_ties_and_specials(name):
    """hb = bf16(h) by round to nearest even on constructed ties (both directions, the carry into the exponent and into inf)
    and their neighbours, -0, inf and NaN (a NaN stays a NaN); an fp32 subnormal may be rounded or flushed to a zero of its
    sign ("Subnormal operands").  hnorm: fp64 |h| <= hnorm <= 1.002 |h| (the kernel's factor 1.001 and a
    rounding error below 1e-4); not finite for a row with an inf or a NaN."""
    from densecap_amd import ops
    s = _get(name)
    rng = np.random.default_rng(50)
    Hd = s.Hd
    hi = rng.integers(0x3000, 0x4800, (8, Hd)).astype(np.uint32)              # 2^-31 .. 2^17, either parity of the kept pattern
    hi |= rng.integers(0, 2, (8, Hd)).astype(np.uint32) << 15                 # either sign
    low = np.array([0x8000, 0x8000, 0x7fff, 0x8001, 0x0001, 0xffff, 0x8000, 0x4000], np.uint32)[:, None]
    bits = (hi << 16) | low
    bits[6, :] = (bits[6, :] & 0x80000000) | (0x3fff << 16) | 0x8000            # a tie whose carry runs into the exponent
    rows = [bits.view(np.float32)]
    sub = rng.integers(1, 0x00800000, (1, Hd)).astype(np.uint32) | (rng.integers(0, 2, (1, Hd)).astype(np.uint32) << 31)
    rows.append(sub.view(np.float32))                                         # 8: fp32 subnormals
    z = _uniform(1, Hd, 51); z[0, ::2] = -0.0; z[0, 1::4] = 0.0; rows.append(z)   # 9: signed zeros
    big = np.full((1, Hd), 0x7f7f8000, np.uint32).view(np.float32).copy(); big[0, 1::2] = np.float32(-3.0e38); rows.append(big)  # 10
    for v in (np.inf, -np.inf, np.nan):                                       # 11, 12, 13
        r = _uniform(1, Hd, 52); r[0, Hd // 2 + 3] = v; rows.append(r)
    h = np.ascontiguousarray(np.concatenate(rows, 0), np.float32)
    n = len(h)
    hb, hn, _ = ops.screen_scores(s.ctx, h, s.V)
    want = R.bf16_rne_bits(h)
    nan = np.isnan(h)
    subn = (np.abs(h) < 2.0 ** -126) & (h != 0)
    exact = ~nan & ~subn
    got = hb[:n, :Hd]
    np.testing.assert_array_equal(got[exact], want[exact])
    assert ((got[nan] & 0x7fff) > 0x7f80).all()
    flushed = (h.view(np.uint32)[subn] >> 16 & 0x8000).astype(np.uint16)
    assert ((got[subn] == want[subn]) | (got[subn] == flushed)).all()
    assert not hb[:n, Hd:].any()
    fin = [0, 1, 2, 3, 4, 5, 6, 7, 9]                     # (row 8: squares of fp32 subnormals underflow, DESIGN.md §4.1c covers it)
    norm = np.sqrt((h[fin].astype(np.float64) ** 2).sum(1))
    assert (hn[fin] >= norm).all() and (hn[fin] <= 1.002 * norm).all(), (hn[fin] / norm)
    assert not np.isfinite(hn[10:n]).any()
    for a in (hb, hn):
        _untouched(a[n:], "guard rows")


# ---- the tail on the device's own scores ------------------------------------------------------------------------------------------
def _tail_inputs(s, n=300):
    """(h, hb, hnorm, scores, z) of n uniform rows: the screen's outputs as the device wrote them and the fp32 logits."""
    def make():
        from densecap_amd import ops
        h = _uniform(n, s.Hd, 60)
        hb, hn, sc = ops.screen_scores(s.ctx, h, s.V, guard_rows=0)
        return h, hb, hn, sc, s.logits(h)
    return s.cached(("tail_inputs", n), make)


@pytest.mark.parametrize("name", ["default", "big_vocab"])
def test_tail_on_the_devices_scores(name):
    """Last-step mode on 300 rows: the token is the first arg-max of the fp32 logits, the winner's value is the row maximum bit
    for bit, the candidate count lies in R.cand_bracket of the device's scores, which is exact on >= 95 % of the rows."""
    from densecap_amd import ops
    s = _get(name)
    h, hb, hn, sc, z = _tail_inputs(s)
    n = len(h)
    o = ops.rescore_tail(s.ctx, sc, h, hn)
    np.testing.assert_array_equal(o["tok"][:n], z.argmax(1) + 1)
    np.testing.assert_array_equal(o["best"][:n].view(np.uint32), z.max(1).view(np.uint32))
    st = torch.from_numpy(sc[:, :s.V1].astype(np.float32))
    lo, hi = R.cand_bracket(st, R.h_norms_up(torch.from_numpy(h)), s.wn(), R.bound_c(s.Hd))
    cand = o["cand"][:n]
    assert (cand >= lo.numpy()).all() and (cand <= hi.numpy()).all(), (cand, lo, hi)
    exact = float((lo == hi).double().mean())
    print("TAIL_STAT set=%s bracket_exact_share=%.4f widest_gap=%d cand_mean=%.2f cand_max=%d" %
          (s.name, exact, int((hi - lo).max()), cand.mean(), cand.max()))
    assert exact >= 0.95
    for k in ("tok", "cand", "best"):
        _untouched(o[k][n:], "guard rows of %s" % k)


@pytest.mark.parametrize("name", ["default"])
def test_tail_at_the_edge_of_the_bound(name):
    """Scores as wrong as the bound allows, against the winner: its score 0.99 b below its fp32 logit, the eight runners-up
    0.99 b above theirs, every other column at fp16(z).  Rows where |s - z| <= b(s) no longer holds on the host after the
    rounding to fp16 are left out (at most 5 %); on all others the token is still the fp32 arg-max."""
    from densecap_amd import ops
    s = _get(name)
    h, hb, hn, sc, z = _tail_inputs(s)
    n = len(h)
    zt = torch.from_numpy(z)
    hnt, c = torch.from_numpy(hn[:n]), R.bound_c(s.Hd)
    b0 = R.bounds(zt.half(), hnt, s.wn(), c)
    order = torch.sort(zt, dim=1, descending=True, stable=True).indices
    rows = torch.arange(n)[:, None]
    crafted = zt.clone()
    crafted[rows, order[:, :1]] -= 0.99 * b0[rows, order[:, :1]]
    crafted[rows, order[:, 1:9]] += 0.99 * b0[rows, order[:, 1:9]]
    sh = crafted.half()
    ok = ((sh.double() - zt.double()).abs() <= R.bounds(sh, hnt, s.wn(), c).double()).all(1).numpy()
    assert ok.mean() >= 0.95, ok.mean()
    scores = np.zeros((n, s.V1pad), np.float16)
    scores[:, :s.V1] = sh.numpy()
    o = ops.rescore_tail(s.ctx, scores, h, hn[:n])
    np.testing.assert_array_equal(o["tok"][:n][ok], (z.argmax(1) + 1)[ok])
    assert (o["cand"][:n][ok] >= 1).all()
    print("edge of the bound: %d of %d rows kept, candidates mean %.1f max %d" % (ok.sum(), n, o["cand"][:n][ok].mean(), o["cand"][:n][ok].max()))


@pytest.mark.parametrize("k", [1, 8, 9, 64, 65, "all"])
@pytest.mark.parametrize("name", ["default", "odd32"])
def test_candidate_counts(name, k):
    """k columns at 8.0, every other at -8.0, the k columns chosen without the row's fp32 arg-max: the count must be k.  Up to
    64 the token is the best exact logit among the k (the lower column on ties), from 65 on the row scans every column and the
    token is the global arg-max -- which the scores, breaking the bound on purpose, rule out.  8 / 9: one and two chunks of
    staged weight rows; 64 / 65: the last slot of the candidate list and the first count past it."""
    from densecap_amd import ops
    s = _get(name)
    h, hb, hn, sc, z = _tail_inputs(s, 64)
    n = len(h)
    kk = s.V1 if k == "all" else k
    top = z.argmax(1)
    rng = np.random.default_rng(70 + kk % 1000)
    scores = np.full((n, s.V1pad), -8.0, np.float16)
    want = np.empty(n, np.int64)
    for r in range(n):
        if kk == s.V1:
            cols = np.arange(s.V1)
        else:
            pool = np.delete(np.arange(s.V1), top[r])
            cols = np.sort(rng.choice(pool, kk, replace=False))
            if r % 4 == 0:
                cols[-1] = pool[-1]                                           # the last real column (or the one before the winner)
                cols = np.unique(cols)
                while len(cols) < kk:
                    cols = np.unique(np.append(cols, rng.choice(pool)))
        scores[r, cols] = 8.0
        want[r] = (top[r] if kk > R.MAX_CAND else cols[np.argmax(z[r, cols])]) + 1
    o = ops.rescore_tail(s.ctx, scores, h, hn[:n])
    np.testing.assert_array_equal(o["cand"][:n], kk)
    np.testing.assert_array_equal(o["tok"][:n], want)


@pytest.mark.parametrize("name", ["default", "odd32"])
def test_candidate_at_equality(name):
    """The rule is s_j + b_j >= L, with equality: a column whose upper end IS L.  h = 0, so b = 2^-10 |s| + 2^-24 and the logits
    are the biases.  Column A at 2^-14: L = 2^-14 - 2^-23 = 1022 x 2^-24, exactly.  Column B at 1018 x 2^-24 (an fp16
    subnormal): s + b = 1019.994 x 2^-24, moved up by 2^-10 of itself + 2^-24 to 1021.99 x 2^-24, which rounds to the fp16
    1022 x 2^-24 = L -- every step is exact in fp32 or a quarter of a unit from a rounding boundary.  Every other column at -8.
    Two candidates, and B, given the larger bias, is the word; a strict comparison would leave A alone."""
    from densecap_amd import ops
    s = _get(name)
    n = 8
    h, hn = np.zeros((n, s.Hd), np.float32), np.zeros(n, np.float32)
    bias = s.bias.numpy()
    rng = np.random.default_rng(90)
    scores = np.full((n, s.V1pad), -8.0, np.float16)
    want = np.empty(n, np.int64)
    for r in range(n):
        a, b = rng.choice(s.V1, 2, replace=False)
        if r == 0:
            a, b = 0, s.V1 - 1
        if bias[b] <= bias[a]:
            a, b = b, a
        scores[r, a], scores[r, b] = np.float16(2.0 ** -14), np.float16(1018 * 2.0 ** -24)
        want[r] = b + 1
    st = torch.from_numpy(scores[:, :s.V1].astype(np.float32))
    bt = R.bounds(st, torch.from_numpy(hn), s.wn(), R.bound_c(s.Hd))
    mask, full = R.candidates(st, bt)
    assert (mask.sum(1) == 2).all() and not full.any()
    assert float((st - bt).max()) == 1022 * 2.0 ** -24                       # L, and the upper end of B equals it
    o = ops.rescore_tail(s.ctx, scores, h, hn)
    np.testing.assert_array_equal(o["cand"][:n], 2)
    np.testing.assert_array_equal(o["tok"][:n], want)
    np.testing.assert_array_equal(o["best"][:n], bias[want - 1])


@pytest.mark.parametrize("name", ["default", "odd32"])
def test_non_finite_scores(name):
    """A +inf, a -inf or a NaN among a row's scores (first, middle and last real column), or an infinite hnorm: the candidate
    count reads -1 and the token is the global arg-max; the rows between them are not affected."""
    from densecap_amd import ops
    s = _get(name)
    h, hb, hn, sc, z = _tail_inputs(s, 64)
    n = len(h)
    scores, hnorm = sc[:n].copy(), hn[:n].copy()
    bad = []
    for i, v in enumerate((np.inf, -np.inf, np.nan)):
        for j, col in enumerate((0, s.V1 // 2, s.V1 - 1)):
            r = 2 * (3 * i + j)
            scores[r, col] = v
            bad.append(r)
    hnorm[40] = np.inf; bad.append(40)
    hnorm[42] = np.nan; bad.append(42)
    o = ops.rescore_tail(s.ctx, scores, h, hnorm)
    good = np.setdiff1d(np.arange(n), bad)
    assert (o["cand"][bad] == -1).all() and (o["cand"][good] >= 1).all()
    np.testing.assert_array_equal(o["tok"][:n], z.argmax(1) + 1)
    np.testing.assert_array_equal(o["best"][:n].view(np.uint32), z.max(1).view(np.uint32))


# ---- the tail with the LSTM update -----------------------------------------------------------------------------------------------
def tail_update_tol(t, cmax):
    """(tol_c, tol_h): how far the device's c' and h' of tail_update (common.h) may be from the float64 cell when every gate
    pre-activation is off by at most t and |c| <= cmax.  Sigmoid and tanh move by at most a quarter of / exactly what their
    argument moves by, so c' = f c + i g moves by at most (cmax / 4 + 1 / 4 + 1) t and h' = o tanh(c') by t / 4 more; 2e-6 for the
    roundings and the device's exp of values <= 1.  (tests/test_gpu_step_tails.py holds the other tails to the same model.)"""
    tol_c = (cmax / 4 + 1.25) * t + 2e-6
    return tol_c, tol_c + t / 4 + 2e-6


@pytest.mark.parametrize("name", ["default", "e_lt_h", "odd32"])
def test_tail_with_gates_writes_the_next_operands(name):
    """With gates the tail also takes the LSTM step and writes the next screen's operands: hb = bf16 of the h it wrote, bit for
    bit, zero up to Kp, and hnorm in the range of the operand kernel.  1, 2 and 3 passes of the row tail (Hd 512, 768, 1056);
    70 rows, the last 20 past a device-side count: those keep the caller's bytes.  The selection is that of the last-step
    mode, and the caller's inputs are not modified."""
    from densecap_amd import ops
    s = _get(name)
    n, live = 70, 50
    h, hb, hn, sc, z = _tail_inputs(s, n)
    rng = np.random.default_rng(80)
    c = (rng.standard_normal((n, s.Hd)) * 0.5).astype(np.float32)
    gates = rng.standard_normal((n, 4 * s.Hd)).astype(np.float32)
    o = ops.rescore_tail(s.ctx, sc, h, hn[:n], c=c, gates_pre=gates, n_dev=live)
    sel = ops.rescore_tail(s.ctx, sc, h, hn[:n])
    for k in ("tok", "cand", "best"):
        np.testing.assert_array_equal(o[k][:live].view(np.uint32), sel[k][:live].view(np.uint32))
    h1, c1 = o["h"][:live], o["c"][:live]
    assert np.isfinite(h1).all() and np.isfinite(c1).all() and (np.abs(h1) <= 1).all() and (h1 != h[:live]).any()
    np.testing.assert_array_equal(o["hb"][:live, :s.Hd], R.bf16_rne_bits(h1))
    assert not o["hb"][:live, s.Hd:].any()
    norm = np.sqrt((h1.astype(np.float64) ** 2).sum(1))
    assert (o["hnorm"][:live] >= norm).all() and (o["hnorm"][:live] <= 1.002 * norm).all()
    for k, a in o.items():
        _untouched(a[live:], "%s past the device-side count" % k)
    # the LSTM update itself against float64 (the route tests hold it bit for bit against the fused step).  The word's gate row
    # xg = b + emb.Wx is an fp32 chain of E terms: off by at most (E + 2) 2^-24 of its sum of magnitudes, t at worst; from there
    # tail_update_tol.
    W = s.W
    E = W["lstm_w"].shape[0] - s.Hd
    tok = torch.from_numpy(o["tok"][:live].astype(np.int64))
    emb, wx = W["lm_emb"][tok - 1].double(), W["lstm_w"][:E].double()
    pre = (W["lstm_b"].double() + emb @ wx) + torch.from_numpy(gates[:live]).double()
    t = float(((E + 2) * 2.0 ** -24 * (W["lstm_b"].double().abs() + emb.abs() @ wx.abs() + torch.from_numpy(gates[:live]).double().abs())).max())
    i, f, og, g = pre.split(s.Hd, 1)
    c_ref = torch.sigmoid(f) * torch.from_numpy(c[:live]).double() + torch.sigmoid(i) * torch.tanh(g)
    h_ref = torch.sigmoid(og) * torch.tanh(c_ref)
    tol_c, tol_h = tail_update_tol(t, float(np.abs(c).max()))
    assert np.abs(c1 - c_ref.numpy()).max() <= tol_c and np.abs(h1 - h_ref.numpy()).max() <= tol_h
