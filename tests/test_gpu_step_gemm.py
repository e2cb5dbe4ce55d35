"""The step GEMM's three row epilogues -- arg-max, log-sum-exp, Gumbel sampling (mfma_gemm.hip, v2_tile<.., AMAX, BF3, LSE>) -- run
alone on crafted operands through dc_debug_step_gemm (include/densecap_debug_step.h), with and without the decode's column prefix
and its device-side row count.

An output element's K order does not depend on the tile shape in the v2 family, so the plain-store run of the same operands gives
the fp32 logits z the epilogues saw.  z is held to the float64 product at test_linear_matches_fp64's 2e-5 tensor bar; everything
else is then bit for bit a selection over z by tests/step_rules.py, except the slot sums of the log-sum-exp, which are held to the
float64 sum under step_rules.lse_sum_bound.  Whole-model tests cannot see a padding column in a sum (1e-5 relative on a caption's
log-likelihood against a 1e-4 bar), an `an` one too long, or a first-maximum slip at a seam nobody ties on; these can.

Every run repeats on both tile routes (force_cfg 2: 128x64 through the mixed launch, 3: 64x64), the 128x64 route also at ring
depths 2 and 3 and with the tile walk switched on: all must write identical bytes, guard rows and unused columns included.  The
walk switch changes a launch only where there are more tiles than workgroup slots, which none of the small cases has (393 tiles
at most against 512 slots): there it pins that the switch is inert.  A workgroup really walks several tiles on the 2048 x 6144
operands alone -- rows_case, test_device_row_count and test_sampling_as_a_tile_walk, all three epilogues."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from tests import step_rules as S

pytestmark = pytest.mark.gpu

FILL = 0xA5
VARIANTS = [("cfg3", dict(force_cfg=3)), ("cfg2", dict(force_cfg=2)), ("cfg2_ring2", dict(force_cfg=2, v2_stages=2)),
            ("cfg2_ring3", dict(force_cfg=2, v2_stages=3)), ("cfg2_walk", dict(force_cfg=2, walk=1)), ("planned", dict())]
ROUTES = VARIANTS[:2]
U_EXP = S.U_EXP             # units granted to the hardware exponential: measured, see step_rules.U_EXP and test_table


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gumbel(ctx):
    """The device's own g for every 23-bit index, as tests/test_gpu_sample.py takes it (held there to float64 within 1e-5)."""
    g = np.empty(1 << 23, np.float32)
    assert ctx.lib.dc_debug_fetch(ctx.h, b"sample_gumbel@0", g.ctypes.data, g.nbytes) == 1 << 23
    return lambda bits: g[np.asarray(bits, np.uint32) >> np.uint32(9)]


@contextmanager
def knobs(ctx, **kw):
    from densecap_amd._lib import check
    try:
        for k in ("force_cfg", "v2_stages", "walk"):
            check(ctx.h, ctx.lib.dc_debug_set(ctx.h, k.encode(), int(kw.get(k, 0))), "dc_debug_set")
        yield
    finally:
        for k in ("force_cfg", "v2_stages", "walk"):
            ctx.lib.dc_debug_set(ctx.h, k.encode(), 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _untouched(a, what):
    assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all(), "%s was written" % what


def _plan(M, N, K, amax):
    from densecap_amd import _lib
    o = (C.c_int32 * 8)()
    assert _lib.lib().dc_debug_plan_gemm(M, N, K, 0, 0, amax, 0, o) == 0
    return list(o)


ROUTE_V2_128x64 = 1


class Operands:
    """A (M, K), W = [V1 real rows; zero rows up to cols = V1 rounded up to 64; G further rows], bias (cols + G; read below V1
    only), uploaded once.  A run without the prefix is the same W read for N = V1 rows."""

    def __init__(self, ctx, M, V1, G, K, seed, A=None, W=None, bias=None):
        rng = np.random.default_rng(seed)
        self.ctx, self.M, self.V1, self.G, self.K = ctx, M, V1, G, K
        self.cols = (V1 + 63) // 64 * 64
        self.N = self.cols + G
        u = lambda *s: (rng.random(s, dtype=np.float32) * 2 - 1).astype(np.float32)
        self.A = u(M, K) if A is None else A
        self.W, self.bias = u(self.N, K), u(self.N)
        self.W[V1:self.cols] = 0
        self.bias[V1:] = 0
        if W is not None:
            self.W[:V1] = W[:V1]
        if bias is not None:
            self.bias[:V1] = bias[:V1]
        self.upload()

    def upload(self):
        self.Ad, self.Wd, self.bd = (self.ctx.to_device(a) for a in (self.A, self.W, self.bias))
        self.Wraw = self.ctx.to_device(self.W[self.cols:]) if self.G else None
        self._z = self._raw = None

    def z(self):
        """The fp32 logits of the real columns: the plain-store run (64x64 tiles), the same under every variant."""
        from densecap_amd import ops
        if self._z is None:
            outs = []
            for name, kw in VARIANTS:
                with knobs(self.ctx, **kw):
                    o = ops.step_gemm(self.ctx, self.Ad, self.Wd, self.bd, ops.STEP_STORE, self.M, self.V1, self.K)
                _untouched(o["C"][self.M:], "store guard rows (%s)" % name)
                outs.append(o["C"][:self.M])
                _same(outs[0], outs[-1], "store route %s" % name)
            self._z = outs[0]
        return self._z

    def raw(self):
        """The product of the G columns behind the prefix, no bias: its own plain-store run."""
        from densecap_amd import ops
        if self._raw is None:
            with knobs(self.ctx, force_cfg=3):
                self._raw = ops.step_gemm(self.ctx, self.Ad, self.Wraw, None, ops.STEP_STORE, self.M, self.G, self.K)["C"][:self.M]
        return self._raw

    def run(self, epi, prefix, variants=VARIANTS, extra_ld=3, **kw):
        """The epilogue under every variant, asserted byte-identical (outputs, guard rows, unused columns); returns one."""
        from densecap_amd import ops
        ld = ops.step_part_ld(epi, self.cols if prefix else self.V1) + extra_ld
        shape = dict(N=self.N, amax_cols=self.cols, amax_n=self.V1) if prefix else dict(N=self.V1)
        first = None
        for name, k in variants:
            with knobs(self.ctx, **k):
                o = ops.step_gemm(self.ctx, self.Ad, self.Wd, self.bd, epi, self.M, K=self.K, part_ld=ld, **shape, **kw)
            if first is None:
                first = o
            for key in first:
                if key != "rc":
                    _same(first[key], o[key], "%s under %s" % (key, name))
        return first


def _check_argmax(o, z, V1, slots, live=None):
    live = z.shape[0] if live is None else live
    val, col = S.argmax_partials(z[:live], V1, slots)
    _same(o["part"][:live, :slots], val, "arg-max values")
    np.testing.assert_array_equal(o["idx"][:live, :slots], col)
    for k in ("part", "idx"):
        _untouched(o[k][live:], "%s past row %d" % (k, live))
        _untouched(o[k][:, slots:], "%s past slot %d" % (k, slots))


def _check_lse(o, z, V1, slots, tgt, what):
    M = z.shape[0]
    mx, s = S.lse_partials(z, V1, slots)
    p = o["part"]
    _same(p[:M, 0:2 * slots:2], mx, "slot maxima")
    _same(p[:M, -1], S.target_logit(z, tgt), "target logit")
    dev = p[:M, 1:2 * slots:2].astype(np.float64)
    ok = np.isfinite(s)
    np.testing.assert_array_equal(np.isfinite(dev), ok)
    assert (dev[~ok & ~np.isnan(s)] == s[~ok & ~np.isnan(s)]).all() and np.isnan(dev[np.isnan(s)]).all()
    bound = S.lse_sum_bound(z, V1, slots, U_EXP)
    live = ok & (mx > -np.inf)
    assert (dev[ok & ~live] == 0).all(), "an empty slot's sum is not zero"
    ratio = float((np.abs(dev - s)[live] / bound[live]).max()) if live.any() else 0.0
    at = lambda u: float((np.abs(dev - s)[live] / S.lse_sum_bound(z, V1, slots, u)[live]).max()) if live.any() else 0.0
    print("LSE_STAT %s worst err/bound %.3f (u = %d); at u = 0 .. 4: %s" % (what, ratio, U_EXP, " ".join("%.3f" % at(u) for u in range(5))))
    assert ratio <= 1.0, (what, ratio)
    _untouched(p[M:], "lse guard rows")
    _untouched(p[:, 2 * slots:-1], "lse unused columns")
    return ratio


def _check_sample(o, want, lse=None):
    """want = S.sample_partials(..) of the run (computed once by the caller: the prefix does not change it)."""
    mx, s, score, col, v = want
    M, slots = mx.shape
    p = o["part"][:M, :5 * slots].reshape(M, slots, 5)
    _same(p[..., 0], mx, "sampling: slot maxima")
    if lse is not None:                                       # the first two floats are the LSE partial bit for bit
        _same(p[..., 0], lse["part"][:M, 0:2 * slots:2], "sampling max vs the LSE epilogue's")
        _same(p[..., 1], lse["part"][:M, 1:2 * slots:2], "sampling sum vs the LSE epilogue's")
    _same(p[..., 2], score, "best perturbed score")
    np.testing.assert_array_equal(_bits(p[..., 3]).view(np.int32), col)
    _same(p[..., 4], v, "logit of the best entry")
    _untouched(o["part"][M:], "sampling guard rows")
    _untouched(o["part"][:, 5 * slots:], "sampling unused columns")


def _keys(M, seed):
    rng = np.random.default_rng(seed)
    k = np.stack([rng.integers(0, 7000, M), rng.integers(0, 256, M)], 1).astype(np.int32)
    k[0] = [2 ** 31 - 1, 255]
    return k


def _targets(M, V1):
    """First column, last real column, and the second lane half (columns 4..7), row by row."""
    return np.array([(1, V1, min(5, V1), min(8, V1))[m % 4] for m in range(M)], np.int32)


# ---- the table ------------------------------------------------------------------------------------------------------------------
#        M    V1    G   K
TABLE = [(1, 1, 64, 32), (31, 31, 96, 96), (33, 32, 64, 32), (64, 33, 96, 96), (65, 63, 64, 32), (127, 64, 96, 96),
         (128, 65, 64, 32), (129, 97, 96, 96), (300, 33, 64, 32), (33, 8257, 96, 96), (300, 8257, 64, 32), (1, 97, 96, 96)]


@pytest.mark.parametrize("case", TABLE, ids=["M%d_V%d_G%d_K%d" % c for c in TABLE])
def test_table(ctx, gumbel, case):
    """One (M, V1, G) of the table, without the prefix (N = V1) and with it (amax_cols = V1 rounded up to 64, G raw columns):
    z against float64, then arg-max, log-sum-exp (targets in the first column, the last real one and the second lane half) and
    sampling at 1 / temperature 0 and 1 against the rules on z; the raw half is the bias-free product bit for bit.
    Measured on an MI355X over the whole module (28 runs of the LSE epilogue): the worst slot-sum err / bound is 0.191 at
    u = 0 (M129_V97_G96_K96), 0.186 at u = 1 and 0.181 at u = 2; u = 0 is the smallest integer that keeps it at or below 0.5."""
    from densecap_amd import ops
    M, V1, G, K = case
    op = Operands(ctx, M, V1, G, K, seed=M * 10007 + V1)
    z = op.z()
    ref = op.A.astype(np.float64) @ op.W[:V1].astype(np.float64).T + op.bias[:V1]
    assert np.abs(z - ref).max() <= 2e-5 * np.abs(ref).max()
    if (M, V1) == (300, 8257):                                 # the planned launch of this shape is the mixed one
        assert _plan(M, op.N, K, 1)[1] == ROUTE_V2_128x64 and _plan(M, V1, K, 1)[1] == ROUTE_V2_128x64
    slots = S.slots_of(V1)
    keys, tgt = _keys(M, V1), _targets(M, V1)
    want0 = S.sample_partials(z, V1, slots, keys, 1, 5, 0.0, gumbel)
    want1 = S.sample_partials(z, V1, slots, keys, 3, (7 << 32) | 11, 1.0, gumbel)
    for prefix in (False, True):
        what = "%s prefix=%d" % (case, prefix)
        o = op.run(ops.STEP_ARGMAX, prefix)
        _check_argmax(o, z, V1, slots)
        lse = op.run(ops.STEP_LSE, prefix, rowidx=tgt)
        _check_lse(lse, z, V1, slots, tgt, what)
        s0 = op.run(ops.STEP_SAMPLE, prefix, rowidx=keys, t=1, seed=5, inv_temp=0.0)
        _check_sample(s0, want0, lse=lse)
        p0 = s0["part"][:M, :5 * slots].reshape(M, slots, 5)
        _same(p0[..., 2], o["part"][:M, :slots], "inv_temp 0: score vs the arg-max epilogue's")
        _same(p0[..., 4], o["part"][:M, :slots], "inv_temp 0: logit vs the arg-max epilogue's")
        np.testing.assert_array_equal(_bits(p0[..., 3]).view(np.int32), o["idx"][:M, :slots])
        s1 = op.run(ops.STEP_SAMPLE, prefix, variants=ROUTES, rowidx=keys, t=3, seed=(7 << 32) | 11, inv_temp=1.0)
        _check_sample(s1, want1, lse=lse)
        if prefix:
            for out in (o, lse, s0, s1):
                _same(out["C"][:M, :G], op.raw(), "raw half")
                _untouched(out["C"][M:], "raw half guard rows")


# ---- ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.TIE_SETS), ids=["%s-%s" % (S.TIE_SEAMS[n], n) for n in S.TIE_SETS])
def test_first_maximum_on_ties(ctx, gumbel, name):
    """Identical W rows with identical large bias: the tied columns are every row's maximum, exactly.  The lower column wins at
    every seam: inside a lane's registers (0, 1), between the lane halves' interleaved runs (3, 4), (7, 8), between a tile's two
    slots (31, 32), between tiles (63, 64), between the tail's waves (0, 2048: slots 0 and 64), between a tail thread's slots
    s and s + 256 (5, 8197), and three ways (3, 4, 64).  Partials by the rules, then both tails on the device's partials."""
    from densecap_amd import ops
    cols = S.TIE_SETS[name]
    M, K, V1 = 33, 32, max(cols) + 40
    A, W, bias = S.tie_operands(cols, M, V1, K, seed=len(name) + V1)
    op = Operands(ctx, M, V1, 64, K, seed=1, A=A, W=W, bias=bias)
    z = op.z()
    assert all((z[:, c] == z[:, cols[0]]).all() for c in cols) and (z.argmax(1) == cols[0]).all()
    assert (np.delete(z, list(cols), 1).max(1) < z[:, cols[0]]).all()
    slots = S.slots_of(V1)
    keys = _keys(M, 3)
    want0 = S.sample_partials(z, V1, slots, keys, 1, 0, 0.0, gumbel)
    Hd = 32
    rng = np.random.default_rng(4)
    xg = rng.standard_normal((V1, 4 * Hd)).astype(np.float32)
    for prefix in (False, True):
        o = op.run(ops.STEP_ARGMAX, prefix, variants=ROUTES, extra_ld=0)
        _check_argmax(o, z, V1, slots)
        tok, _ = S.row_merge(o["part"][:M, :slots], o["idx"][:M, :slots])
        assert (tok == cols[0] + 1).all()
        t = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, M, Hd, part=o["part"][:M], idx=o["idx"][:M], nslots=slots, ld=slots, xg=xg)
        np.testing.assert_array_equal(t["seq"][:, 0], cols[0] + 1)
        s0 = op.run(ops.STEP_SAMPLE, prefix, variants=ROUTES, extra_ld=0, rowidx=keys, t=1, seed=0, inv_temp=0.0)
        _check_sample(s0, want0)
        t = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, M, Hd, part=s0["part"][:M], nslots=slots, ld=5 * slots, xg=xg, end_tok=V1,
                          acc=np.zeros(M), fin=np.zeros(M, np.uint8))
        np.testing.assert_array_equal(t["seq"][:, 0], cols[0] + 1)
        assert not t["fin"].any()


# ---- padding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1e30, np.nan, np.inf], ids=["pad_1e30", "pad_nan", "pad_inf"])
def test_padding_columns_do_not_exist(ctx, value):
    """Prefix mode with W rows and bias in [amax_n, amax_cols) poisoned: partials and the raw half equal the zero-padding run
    byte for byte, for all three epilogues.  An `an` one too long, or a mask off by one, lets the poison in."""
    from densecap_amd import ops
    M, V1, G, K = 65, 97, 64, 32
    clean = Operands(ctx, M, V1, G, K, seed=77)
    bad = Operands(ctx, M, V1, G, K, seed=77)
    bad.W[V1:bad.cols] = value
    bad.bias[V1:bad.cols] = value
    bad.upload()
    keys, tgt = _keys(M, 5), _targets(M, V1)
    runs = [(ops.STEP_ARGMAX, {}), (ops.STEP_LSE, dict(rowidx=tgt)), (ops.STEP_SAMPLE, dict(rowidx=keys, t=2, seed=9, inv_temp=0.0)),
            (ops.STEP_SAMPLE, dict(rowidx=keys, t=2, seed=9, inv_temp=1.0))]
    for epi, kw in runs:
        a, b = clean.run(epi, True, **kw), bad.run(epi, True, **kw)
        for key in a:
            if key != "rc":
                _same(a[key], b[key], "epilogue %d: %s" % (epi, key))


# ---- specials --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["neginf_slot", "nan_column", "nan_row"])
def test_specials(ctx, gumbel, kind):
    """docs/SEMANTICS.md: an entry needs v > -inf, a NaN never wins, a row without an entry has no word.  A slot whose bias is all
    -inf is empty -- (-inf, sentinel), (-inf, 0) -- and its row's word comes from the other slots; a NaN column among numbers
    is passed over; an all-NaN row (a NaN in its h) has sentinels in every slot, and both tails write word 0 for it."""
    from densecap_amd import ops
    M, V1, G, K = 33, 97, 64, 32
    op = Operands(ctx, M, V1, G, K, seed=55)
    if kind == "neginf_slot":
        op.bias[32:64] = -np.inf
    elif kind == "nan_column":
        op.bias[40] = np.nan
    else:
        op.A[7, 3] = np.nan
    op.upload()
    z = op.z()
    slots = S.slots_of(V1)
    keys, tgt = _keys(M, 6), _targets(M, V1)
    Hd = 32
    xg = np.random.default_rng(8).standard_normal((V1, 4 * Hd)).astype(np.float32)
    want = np.where(np.isnan(z).all(1), 0, np.nanargmax(np.where(np.isnan(z).all(1)[:, None], 0, z), 1) + 1)
    for prefix in (False, True):
        o = op.run(ops.STEP_ARGMAX, prefix, variants=ROUTES)
        _check_argmax(o, z, V1, slots)
        if kind == "neginf_slot":
            assert (o["idx"][:M, 1] == S.NO_COL).all() and np.isneginf(o["part"][:M, 1]).all()
        if kind == "nan_column":
            assert (o["idx"][:M, :slots] != 40).all()
        if kind == "nan_row":
            assert (o["idx"][7, :slots] == S.NO_COL).all()
        t = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, M, Hd, part=o["part"][:M, :slots], idx=o["idx"][:M, :slots], nslots=slots,
                          ld=slots, xg=xg)
        np.testing.assert_array_equal(t["seq"][:, 0], want)
        if kind != "nan_column":                                # (a NaN column poisons its slot's sum: out of the rules' scope)
            lse = op.run(ops.STEP_LSE, prefix, variants=ROUTES, rowidx=tgt)
            _check_lse(lse, z, V1, slots, tgt, "%s prefix=%d" % (kind, prefix))
        for inv_temp in (0.0, 1.0):
            s = op.run(ops.STEP_SAMPLE, prefix, variants=ROUTES, extra_ld=0, rowidx=keys, t=2, seed=3, inv_temp=inv_temp)
            mx, _, score, col, v = S.sample_partials(z, V1, slots, keys, 2, 3, inv_temp, gumbel)
            p = s["part"][:M].reshape(M, slots, 5)
            _same(p[..., 0], mx, "maxima")
            _same(p[..., 2], score, "scores")
            np.testing.assert_array_equal(_bits(p[..., 3]).view(np.int32), col)
            _same(p[..., 4], v, "logits")
            if inv_temp == 0.0:
                t = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, M, Hd, part=s["part"][:M], nslots=slots, ld=5 * slots, xg=xg,
                                  end_tok=V1, acc=np.zeros(M), fin=np.zeros(M, np.uint8))
                np.testing.assert_array_equal(t["seq"][:, 0], want)
                np.testing.assert_array_equal(t["fin"] != 0, (want == 0) | (want == V1))
                assert np.isnan(t["acc"][want == 0]).all()


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_temp", [1.0, 0.5, 100.0], ids=["inv_temp_1", "inv_temp_0.5", "inv_temp_100"])
def test_sampling_entries(ctx, gumbel, inv_temp):
    """amax_n not a multiple of 4 (97 and 8257: the last run of four columns holds one real column and three the noise must not
    reach): the best perturbed entry of every slot is the rule's, fp32(fp32(v inv_temp) + g) with the device's own g, bit for
    bit, at 1 / temperature 1, 0.5 and 100."""
    from densecap_amd import ops
    for M, V1, K in ((65, 97, 32), (33, 8257, 96)):
        op = Operands(ctx, M, V1, 64, K, seed=V1 + int(inv_temp * 10))
        z = op.z()
        keys = _keys(M, V1)
        for t, seed in ((1, 0), (15, 2 ** 64 - 1)):
            want = S.sample_partials(z, V1, S.slots_of(V1), keys, t, seed, inv_temp, gumbel)
            for prefix in (False, True):
                _check_sample(op.run(ops.STEP_SAMPLE, prefix, variants=ROUTES, rowidx=keys, t=t, seed=seed, inv_temp=inv_temp), want)


# ---- the device-side row count ---------------------------------------------------------------------------------------------------
ROWS_M, ROWS_N, ROWS_K = 2048, 6144, 32
COUNTS = [0, 1, 64, 65, 128] + list(range(256, 2049, 128)) + [1151, 1153, 1663, 1665, 1791, 1793]


@pytest.fixture(scope="module")
def rows_case(ctx):
    """2048 x 6144 x 32: 1536 tiles of 128x64, two full rounds of the 768 slots the planner picks (ring depth 2).  The operands
    stay on the device; the runs without a count are the reference of every count, themselves held to the rules once."""
    from densecap_amd import ops
    plan = _plan(ROWS_M, ROWS_N, ROWS_K, 1)
    assert plan[1] == ROUTE_V2_128x64 and plan[2] == 2, plan       # the mixed launch, or the sweep tests something else
    op = Operands(ctx, ROWS_M, ROWS_N, 0, ROWS_K, seed=2048)
    tgt = _targets(ROWS_M, ROWS_N)
    td = ctx.to_device(tgt)
    with knobs(ctx, force_cfg=3):
        z = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_STORE, ROWS_M, ROWS_N, ROWS_K, guard_rows=0)["C"]
    base = {}
    slots = S.slots_of(ROWS_N)
    for walk in (0, 1):
        with knobs(ctx, walk=walk):
            a = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_ARGMAX, ROWS_M, ROWS_N, ROWS_K, guard_rows=0)
            l = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_LSE, ROWS_M, ROWS_N, ROWS_K, rowidx=td, guard_rows=0)
        if walk == 0:
            base = dict(argmax=a, lse=l, z=z)
            _check_argmax(a, z, ROWS_N, slots)
            _same(l["part"][:, 0:2 * slots:2], S.lse_partials(z, ROWS_N, slots)[0], "slot maxima")
            _same(l["part"][:, -1], S.target_logit(z, tgt), "target logits")
        else:
            for k in ("part", "idx"):
                _same(a[k], base["argmax"][k], "arg-max, tile walk")
            _same(l["part"], base["lse"]["part"], "lse, tile walk")
    return op, td, base


@pytest.mark.parametrize("count", COUNTS, ids=["count%d" % c for c in COUNTS])
def test_device_row_count(ctx, rows_case, count):
    """*m_dev = count on the mixed launch, which rebuilds its tile map on the device for the live row tiles: rows below the count
    equal the run without a count bit for bit, rows from the count on keep the caller's bytes -- arg-max and log-sum-exp, one
    workgroup per tile and as a tile walk.  At 13 and 14 live row tiles (counts 1537 .. 1792) the rebuilt map wants a split last
    round that does not fit the grid the host sized (768 + 2 x 480 or 2 x 576 workgroups against 1536): the kernel then runs every
    live tile whole, one per workgroup -- without the tile walk having been asked for."""
    from densecap_amd import ops
    op, td, base = rows_case
    live = min(count, ROWS_M)
    for walk in (0, 1):
        with knobs(ctx, walk=walk):
            a = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_ARGMAX, ROWS_M, ROWS_N, ROWS_K, m_dev=count, guard_rows=0)
            l = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_LSE, ROWS_M, ROWS_N, ROWS_K, rowidx=td, m_dev=count, guard_rows=0)
        for got, ref, keys in ((a, base["argmax"], ("part", "idx")), (l, base["lse"], ("part",))):
            for k in keys:
                _same(got[k][:live], ref[k][:live], "%s below the count (walk %d)" % (k, walk))
                _untouched(got[k][live:], "%s from row %d on (walk %d)" % (k, live, walk))


def test_sampling_as_a_tile_walk(ctx, gumbel, rows_case):
    """The only operands of this module with more tiles than slots (1536 against 768): with dc_debug_set "walk" a workgroup
    runs two tiles, and the sampling epilogue must write the bytes it writes with one workgroup per tile; the first 130 rows
    (two row tiles) are also held to the rules."""
    from densecap_amd import ops
    op, _, base = rows_case
    keys = _keys(ROWS_M, 4)
    kd = ctx.to_device(keys)
    runs = []
    for walk in (0, 1):
        with knobs(ctx, walk=walk):
            runs.append(ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_SAMPLE, ROWS_M, ROWS_N, ROWS_K, rowidx=kd, t=2, seed=17,
                                      inv_temp=1.0, guard_rows=0))
    _same(runs[0]["part"], runs[1]["part"], "sampling, tile walk")
    n = 130
    want = S.sample_partials(base["z"][:n], ROWS_N, S.slots_of(ROWS_N), keys[:n], 2, 17, 1.0, gumbel)
    _check_sample(dict(part=runs[1]["part"][:n]), want)


def test_sampling_refuses_a_row_count(ctx, rows_case):
    from densecap_amd import ops
    op, td, _ = rows_case
    keys = ctx.to_device(_keys(ROWS_M, 1))
    o = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, ops.STEP_SAMPLE, ROWS_M, ROWS_N, ROWS_K, rowidx=keys, t=1, seed=1, inv_temp=1.0,
                      m_dev=100, raise_errors=False)
    assert o["rc"] < 0
    _untouched(o["part"], "partials of a refused launch")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSALS = ["amax_cols_not_64", "amax_n_past_amax_cols", "part_ld_argmax", "part_ld_lse", "part_ld_sample"]


@pytest.mark.parametrize("which", REFUSALS)
def test_refusals_write_nothing(ctx, which):
    """amax_cols not a multiple of 64, amax_n > amax_cols, and a part_ld one below each epilogue's documented minimum: an error
    code on both tile routes, and every output byte as the caller left it."""
    from densecap_amd import ops
    M, V1, G, K = 33, 97, 64, 32
    op = Operands(ctx, M, V1, G, K, seed=91)
    keys, tgt = _keys(M, 2), _targets(M, V1)
    per_epi = {ops.STEP_ARGMAX: {}, ops.STEP_LSE: dict(rowidx=tgt), ops.STEP_SAMPLE: dict(rowidx=keys, t=1, seed=1, inv_temp=1.0)}
    if which == "amax_cols_not_64":
        # a misaligned prefix that breaks no other rule: 160 <= N = 192, amax_n = 97 <= 160, partials sized for all of N
        assert V1 <= op.cols + 32 <= op.N
        runs = [(e, dict(N=op.N, amax_cols=op.cols + 32, amax_n=V1, part_ld=ops.step_part_ld(e, op.N))) for e in per_epi]
    elif which == "amax_n_past_amax_cols":
        runs = [(e, dict(N=op.N, amax_cols=op.cols, amax_n=op.cols + 1, part_ld=ops.step_part_ld(e, op.cols))) for e in per_epi]
    else:
        e = dict(part_ld_argmax=ops.STEP_ARGMAX, part_ld_lse=ops.STEP_LSE, part_ld_sample=ops.STEP_SAMPLE)[which]
        runs = [(e, dict(N=op.N, amax_cols=op.cols, amax_n=V1, part_ld=ops.step_part_ld(e, op.cols) - 1)),
                (e, dict(N=V1, part_ld=ops.step_part_ld(e, V1) - 1))]
    for name, kw in ROUTES:
        for e, shape in runs:
            with knobs(ctx, **kw):
                o = ops.step_gemm(ctx, op.Ad, op.Wd, op.bd, e, M, K=K, raise_errors=False, **shape, **per_epi[e])
            assert o["rc"] < 0, (which, name, e)
            for key in o:
                if key != "rc":
                    _untouched(o[key], "%s of a refused launch (%s)" % (key, name))
