"""The three row tails of the classic decode step (elementwise.hip: lstm_step_tail_kernel, lse_step_tail_kernel,
sample_step_tail_kernel), one launch each on crafted partials through dc_debug_step_tail (include/densecap_debug_step.h).

The GEMM tests (tests/test_gpu_step_gemm.py) hold what the epilogues write; here the partials are the test's own, so that the
tails meet what a model's weights never give them: sentinel slots before, between and after real ones, rows of sentinels only,
equal values in the two slots of one thread (s, s + 256) and in slots of two waves (s, s + 64), finished rows, rows that draw END,
a winning column past the vocabulary.  Words and flags are exact by tests/step_rules.py; the double sums are held to
(nslots + 8) 2^-52 (|logit| + |lse|); c' and h' to the float64 cell under the error model of tail_update that
tests/test_gpu_decode_screen_kernels.py derives.

Hd 32, 512, 544, 1056: part of a pass of the 512 hidden units a workgroup takes at a time, exactly one, a second pass of 32, three
passes.  nslots 1, 2, 255, 256, 257, 513: below, at and past one slot per thread, and a third round of 256."""
import numpy as np
import pytest

from tests import step_rules as S
from tests.test_gpu_decode_screen_kernels import tail_update_tol

pytestmark = pytest.mark.gpu

FILL = 0xA5
#        Hd   nslots
PAIRS = [(32, 1), (512, 2), (544, 255), (1056, 256), (32, 257), (544, 513), (512, 256), (1056, 2)]
IDS = ["Hd%d_slots%d" % p for p in PAIRS]
N = 14                       # rows of a launch
T, TPOS = 3, 1


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


def _untouched(a, what):
    assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all(), "%s was written" % what


def _state(n, Hd, xg_rows, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(xg=f(xg_rows, 4 * Hd), gates=f(n, 4 * Hd), c=(f(n, Hd) * 0.5).astype(np.float32), h=f(n, Hd))


def _check_state(got, st, tok, stepped, what, zero_c=False):
    """c', h' of the rows in `stepped` against the float64 cell with the words' xg rows; every other row keeps its bytes.  The
    one rounded addition x + gates_pre moves a pre-activation by at most 2^-24 of the sum of magnitudes: t."""
    x = S.xg_rows_of(st["xg"], tok)
    c1, h1 = S.lstm_update(x, st["gates"], st["c"], zero_c=zero_c)
    t = float(2.0 ** -24 * (np.abs(x) + np.abs(st["gates"])).max())
    tol_c, tol_h = tail_update_tol(t, float(np.abs(st["c"]).max()))
    rows = np.asarray(stepped, bool)
    ec, eh = np.abs(got["c"] - c1)[rows].max(initial=0.0), np.abs(got["h"] - h1)[rows].max(initial=0.0)
    print("STATE_STAT %s: err_c / tol %.3f, err_h / tol %.3f" % (what, ec / tol_c, eh / tol_h))
    assert ec <= tol_c and eh <= tol_h, (what, ec, tol_c, eh, tol_h)
    np.testing.assert_array_equal(got["c"][~rows].view(np.uint32), st["c"][~rows].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(got["h"][~rows].view(np.uint32), st["h"][~rows].view(np.uint32), err_msg=what)
    if rows.any() and st["c"].shape[1] >= 32:
        assert (got["h"][rows] != st["h"][rows]).any()


def _tie_slots(nslots):
    """Where rows 5 and 6 of _entries hold their equal values: two slots of one tail thread (s, s + 256) where there are that
    many, the last two otherwise; two slots 64 apart (two waves), the first and the last otherwise."""
    five = (3, 259) if nslots > 259 else (0, 256) if nslots > 256 else (max(nslots - 2, 0), nslots - 1)
    six = (5, 69) if nslots > 69 else (0, nslots - 1)
    return five, six


def _entries(nslots, seed, spread=2):
    """(val (N, nslots) float32, col (N, nslots) int32) of rows crafted for the merge; columns ascend with the slot as the
    epilogue's do: slot s holds column spread * s or spread * s + 1.
      0 random            1 sentinels before      2 sentinels between     3 sentinels after       4 sentinels only
      5 equal values in slots s, s + 256 (the last two slots below 257)   6 equal values in s, s + 64 (or 0, last)
      7 every value equal 8 the maximum in the last slot                  9 .. random"""
    rng = np.random.default_rng(seed)
    val = rng.standard_normal((N, nslots)).astype(np.float32)
    col = (spread * np.arange(nslots)[None, :] + rng.integers(0, 2, (N, nslots))).astype(np.int32)
    half = (nslots + 1) // 2
    gone = np.zeros((N, nslots), bool)
    gone[1, :nslots - half] = True
    gone[2, 1::2] = True
    gone[3, half:] = True
    gone[4, :] = True
    for row, (a, b) in zip((5, 6), _tie_slots(nslots)):
        val[row, a] = val[row, b] = 9.0
    val[7, :] = 0.25
    val[8, nslots - 1] = 9.0
    val[gone] = -np.inf
    col[gone] = S.NO_COL
    return val, col


# ---- greedy ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_greedy_tail(ctx, pair):
    """tok = 1 + the column of the best entry, the lower column on equal values (rows 5 - 7: slots of one thread, of two waves,
    of every thread), sentinels never; a row of sentinels writes 0 and steps without an xg row; rows from the device-side count
    on keep seq, c and h; with gates_pre null only seq is written."""
    from densecap_amd import ops
    Hd, nslots = pair
    val, col = _entries(nslots, seed=Hd + nslots)
    xg_rows = 2 * nslots
    st = _state(N, Hd, xg_rows, seed=nslots)
    want, slot = S.row_merge(val, col)
    assert want[4] == 0 and (want[[0, 1, 2, 3, 5, 6, 7, 8]] > 0).all() and want[7] == col[7, 0] + 1 and slot[8] == nslots - 1
    assert (slot[5], slot[6]) == tuple(a for a, _ in _tie_slots(nslots))
    live = N - 3
    kw = dict(part=val, idx=col, nslots=nslots, ld=nslots, T=T, t=TPOS)
    o = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, xg=st["xg"], gates_pre=st["gates"], c=st["c"], h=st["h"], n_dev=live, **kw)
    np.testing.assert_array_equal(o["seq"][:live, TPOS], want[:live])
    _untouched(o["seq"][live:], "seq from the count on")
    _untouched(o["seq"][:, [0, 2]], "seq at other steps")
    _check_state(o, st, want, np.arange(N) < live, "greedy %s" % (pair,))
    sel = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, xg=st["xg"], c=st["c"], h=st["h"], **kw)
    np.testing.assert_array_equal(sel["seq"][:, TPOS], want)
    _check_state(sel, st, want, np.zeros(N, bool), "greedy, selection only")
    # a wider row stride than slots: the words do not change, what lies between is not read as an entry
    ld = nslots + 5
    wide_v = np.full((N, ld), 99.0, np.float32); wide_v[:, :nslots] = val
    wide_c = np.zeros((N, ld), np.int32); wide_c[:, :nslots] = col
    w = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, part=wide_v, idx=wide_c, nslots=nslots, ld=ld, xg=st["xg"], T=T, t=TPOS)
    np.testing.assert_array_equal(w["seq"][:, TPOS], want)


@pytest.mark.parametrize("zero_c", [0, 1], ids=["keep_c", "zero_c"])
@pytest.mark.parametrize("Hd", [32, 512, 544, 1056])
def test_greedy_tail_fixed_word(ctx, Hd, zero_c):
    """No partials: fixed_tok is the word of every row (the START step) -- the last row of xg, the first, and 0 = no row of xg
    (the image step) -- from the caller's c or from c = 0; seq is not written."""
    from densecap_amd import ops
    st = _state(N, Hd, 7, seed=Hd)
    for tok in (7, 1, 0):
        o = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, xg=st["xg"], gates_pre=st["gates"], c=st["c"], h=st["h"], zero_c=zero_c,
                          fixed_tok=tok, T=T, t=TPOS)
        _untouched(o["seq"], "seq")
        _check_state(o, st, np.full(N, tok), np.ones(N, bool), "fixed_tok %d zero_c %d Hd %d" % (tok, zero_c, Hd), zero_c=bool(zero_c))


def test_hook_refuses_what_would_become_an_address(ctx):
    """A column, a target or a fixed word outside the xg table is refused before any launch: the greedy tail does not bound its
    column itself (include/densecap_debug_step.h), and nothing here may make a kernel read out of bounds."""
    from densecap_amd import ops
    Hd, nslots = 32, 4
    st = _state(N, Hd, 8, seed=1)
    val, col = _entries(nslots, seed=2)
    common = dict(xg=st["xg"], gates_pre=st["gates"], c=st["c"], h=st["h"], T=T, t=TPOS, raise_errors=False)
    for bad in (8, -1, 2 ** 31 - 2):
        c2 = col.copy(); c2[9, 2] = bad
        o = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, part=val, idx=c2, nslots=nslots, ld=nslots, **common)
        assert o["rc"] == -1, bad
        _untouched(o["seq"], "seq of a refused launch")
        np.testing.assert_array_equal(o["c"], st["c"]); np.testing.assert_array_equal(o["h"], st["h"])
        p = np.zeros((N, 5 * nslots), np.float32)
        p.view(np.int32)[:, 3::5] = c2
        o = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, N, Hd, part=p, nslots=nslots, ld=5 * nslots, end_tok=8, acc=np.zeros(N),
                          fin=np.zeros(N, np.uint8), **common)
        assert o["rc"] == -1 and not o["fin"].any() and not o["acc"].any(), bad
    for bad in (0, 9, -3):
        tgt = np.ones(N, np.int32); tgt[3] = bad
        o = ops.step_tail(ctx, ops.STEP_TAIL_SCORE, N, Hd, part=np.zeros((N, 2 * nslots + 1), np.float32), nslots=nslots,
                          ld=2 * nslots + 1, tgt=tgt, end_tok=100, acc=np.zeros(N), **common)
        assert o["rc"] == -1 and not o["acc"].any(), bad
    for bad in (9, -1):
        o = ops.step_tail(ctx, ops.STEP_TAIL_GREEDY, N, Hd, fixed_tok=bad, **common)
        assert o["rc"] == -1, bad
    o = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, N, Hd, part=np.zeros((N, 5 * nslots), np.float32), nslots=nslots, ld=5 * nslots,
                      end_tok=9, acc=np.zeros(N), fin=np.zeros(N, np.uint8), **common)
    assert o["rc"] == -1


# ---- scoring ---------------------------------------------------------------------------------------------------------------------
def _lse_parts(nslots, seed):
    """(mx (N, nslots) float32, sum (N, nslots) float32): maxima spread over a dozen units, sums in [1, 32), empty slots (-inf, 0)
    as _entries places its sentinels (row 4: every slot but the first)."""
    rng = np.random.default_rng(seed)
    mx = (rng.standard_normal((N, nslots)) * 4).astype(np.float32)
    sm = (1 + 31 * rng.random((N, nslots))).astype(np.float32)
    gone = _entries(nslots, seed)[1] == S.NO_COL
    gone[4, 0] = False
    mx[gone], sm[gone] = -np.inf, 0.0
    return mx, sm


def _acc_check(got, acc0, logit, lse, rows, nslots, what):
    """acc = acc0 + (logit - lse) on `rows`: the device's double exp / log and the order of at most nslots double additions, so
    (nslots + 8) 2^-52 (|logit| + |lse|), for every row: the odd rows start from a non-zero acc0, and the rule adds its term to
    acc0 in double as the device does (one rounded addition on either side), so they are held to the same bar."""
    want = acc0 + (logit.astype(np.float64) - lse)
    bar = (nslots + 8) * 2.0 ** -52 * (np.abs(logit.astype(np.float64)) + np.abs(lse))
    ratio = float((np.abs(got - want)[rows] / bar[rows]).max())
    print("ACC_STAT %s: worst err / bar %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_scoring_tail(ctx, pair):
    """acc[m] += target logit - lse in double against the rule; a row whose target is end_tok adds its term and keeps c, h;
    every other row steps with its target's xg row; with gates_pre null (the last step) the sums are the same and no row steps."""
    from densecap_amd import ops
    Hd, nslots = pair
    mx, sm = _lse_parts(nslots, seed=Hd + nslots)
    ld = 2 * nslots + 1
    rng = np.random.default_rng(nslots)
    part = np.zeros((N, ld), np.float32)
    part[:, 0:2 * nslots:2], part[:, 1:2 * nslots:2] = mx, sm
    part[:, -1] = (rng.standard_normal(N) * 3).astype(np.float32)
    xg_rows = 9
    end_tok = xg_rows
    st = _state(N, Hd, xg_rows, seed=nslots + 1)
    tgt = rng.integers(1, xg_rows, N).astype(np.int32)
    tgt[[2, 6]] = end_tok
    tgt[0], tgt[1] = 1, xg_rows - 1
    acc0 = np.where(np.arange(N) % 2, rng.standard_normal(N) * 40, 0.0)
    lse = S.lse_rows(mx, sm.astype(np.float64))
    kw = dict(part=part, nslots=nslots, ld=ld, xg=st["xg"], c=st["c"], h=st["h"], tgt=tgt, end_tok=end_tok, acc=acc0)
    o = ops.step_tail(ctx, ops.STEP_TAIL_SCORE, N, Hd, gates_pre=st["gates"], **kw)
    _acc_check(o["acc"], acc0, part[:, -1], lse, np.ones(N, bool), nslots, "scoring %s" % (pair,))
    _check_state(o, st, tgt, tgt != end_tok, "scoring %s" % (pair,))
    last = ops.step_tail(ctx, ops.STEP_TAIL_SCORE, N, Hd, **kw)
    np.testing.assert_array_equal(last["acc"].view(np.uint64), o["acc"].view(np.uint64))
    _check_state(last, st, tgt, np.zeros(N, bool), "scoring, last step")


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_sampling_tail(ctx, pair):
    """The word is the best perturbed entry over the slots (rows as in _entries); its term is the ENTRY'S OWN logit minus lse,
    not its score and not the slot maximum.  Row 9 is finished: it writes 0 and adds nothing but still steps with the word
    drawn.  Row 4 has no entry: NaN in acc, finished, word 0, a step without an xg row.  Row 10's winner sits at column
    end_tok, row 11's one past it: no entry either.  Row 12 draws END (column end_tok - 1): its term counts and it is finished."""
    from densecap_amd import ops
    Hd, nslots = pair
    score, col = _entries(nslots, seed=Hd + nslots + 7, spread=3)
    mx, sm = _lse_parts(nslots, seed=Hd + nslots + 7)
    rng = np.random.default_rng(nslots + 3)
    logit = (rng.standard_normal((N, nslots)) * 3).astype(np.float32)
    end_tok = 3 * nslots + 4
    xg_rows = end_tok + 3
    last = nslots - 1
    for row, c in ((10, end_tok), (11, end_tok + 1), (12, end_tok - 1)):
        score[row, last], col[row, last] = 50.0, c
    gone = col == S.NO_COL
    logit[gone] = -np.inf
    part = np.zeros((N, 5 * nslots), np.float32)
    part[:, 0::5], part[:, 1::5], part[:, 2::5], part[:, 4::5] = mx, sm, score, logit
    part.view(np.int32)[:, 3::5] = col
    fin0 = np.zeros(N, np.uint8)
    fin0[9] = 1
    acc0 = np.where(np.arange(N) % 2, rng.standard_normal(N) * 40, 0.0)
    st = _state(N, Hd, xg_rows, seed=nslots + 2)
    tok, slot = S.row_merge(score, col)
    none = (tok == 0) | (tok > end_tok)
    assert none[[4, 10, 11]].all() and none.sum() == 3 and tok[12] == end_tok
    word = np.where(none, 0, tok)
    lse = S.lse_rows(mx, sm.astype(np.float64))
    kw = dict(part=part, nslots=nslots, ld=5 * nslots, xg=st["xg"], c=st["c"], h=st["h"], end_tok=end_tok, acc=acc0, fin=fin0, T=T,
              t=TPOS)
    o = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, N, Hd, gates_pre=st["gates"], **kw)
    done = fin0 != 0
    np.testing.assert_array_equal(o["seq"][:, TPOS], np.where(done, 0, word))
    _untouched(o["seq"][:, [0, 2]], "seq at other steps")
    np.testing.assert_array_equal(o["fin"] != 0, done | none | (word == end_tok))
    assert np.isnan(o["acc"][none & ~done]).all()
    np.testing.assert_array_equal(o["acc"][done].view(np.uint64), acc0[done].view(np.uint64))
    adds = ~done & ~none
    own = logit[np.arange(N), np.maximum(slot, 0)]
    assert (own[adds] != score[np.arange(N), np.maximum(slot, 0)][adds]).all()
    _acc_check(o["acc"], acc0, own, lse, adds, nslots, "sampling %s" % (pair,))
    _check_state(o, st, word, np.ones(N, bool), "sampling %s" % (pair,))
    sel = ops.step_tail(ctx, ops.STEP_TAIL_SAMPLE, N, Hd, **kw)
    np.testing.assert_array_equal(sel["seq"], o["seq"])
    np.testing.assert_array_equal(sel["acc"].view(np.uint64), o["acc"].view(np.uint64))
    _check_state(sel, st, word, np.zeros(N, bool), "sampling, last step")
