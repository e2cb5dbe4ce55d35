"""The multi-order NMS on the GPU (dc_op_nms_multi): every comparison is exact list equality with the reference of
tests/nms_multi_rules.py -- per column, the oracle's box_utils.nms on the column's candidates."""
import ctypes as C

import numpy as np
import pytest

from tests import nms_multi_rules as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _check(ctx, boxes, scores, thresh, M, valid=None, what=""):
    from densecap_amd import ops
    picks, counts = ops.nms_multi(ctx, boxes, scores, thresh, M, valid)
    Q = scores.shape[1] if scores.ndim == 2 else 1
    assert picks.shape == (Q, M) and counts.shape == (Q,) and picks.dtype == np.int32
    got = R.as_lists(picks, counts)                                    # (checks the -1 padding)
    diff = R.first_difference(got, R.nms_multi_ref(boxes, scores, thresh, M, valid))
    assert diff is None, "%s: %s" % (what, diff)
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000, 4096])
def test_sweep(ctx, n):
    """Every n x Q x M of the sweep, each on clusters of 8 and on clusters of 100 boxes; the score columns hold independent,
    rounded (tied), copied and constant columns (nms_multi_rules.score_columns)."""
    rng = np.random.default_rng(n)
    sets = ((8, R.clustered_boxes(rng, n, 8)), (100, R.clustered_boxes(rng, n, 100)))
    for Q in (1, 3, 70):
        s = R.score_columns(rng, n, Q)
        for M in sorted({1, 7, n}):
            for per, b in sets:
                got = _check(ctx, b, s, 0.5, M, what="n=%d Q=%d M=%d clusters of %d" % (n, Q, M, per))
                if Q >= 4:
                    assert got[2] == got[0]                            # the copied column gives identical rows
                if Q >= 3 and M == n:
                    assert got[Q - 1] == sorted(got[Q - 1])            # the constant column: index order


@pytest.mark.parametrize("n", [65, 1000])
def test_box_sets(ctx, n):
    rng = np.random.default_rng(100 + n)
    s = R.score_columns(rng, n, 5)
    got = _check(ctx, R.identical_boxes(n), s, 0.5, 7, what="identical")
    assert [len(g) for g in got] == [1] * 5 and got[4] == [0]
    got = _check(ctx, R.disjoint_boxes(n), s, 0.5, n, what="disjoint")
    for q in range(5):                                                 # the picks are the sorted order itself
        assert got[q] == np.lexsort((np.arange(n), -s[:, q].astype(np.float64))).tolist()
    for per in (8, 100):
        b = R.with_non_finite(rng, R.clustered_boxes(rng, n, per), 6)
        _check(ctx, b, s, 0.4, n, what="non-finite coordinates, clusters of %d" % per)
        _check(ctx, b, s, 0.4, 7, what="non-finite coordinates, clusters of %d, M = 7" % per)


@pytest.mark.parametrize("M", [64, 128, 63, 65])
def test_pick_budget_met_at_the_end_of_a_chunk(ctx, M):
    """Disjoint boxes: every position of the order is a pick, so pick M is position M - 1 -- with M = 64 / 128 the last row
    of the first / second 64-row chunk of the walk, where the budget test and the chunk hand-off meet."""
    n = 130
    s = R.score_columns(np.random.default_rng(7), n, 3)
    got = _check(ctx, R.disjoint_boxes(n), s, 0.5, M, what="M=%d" % M)
    assert [len(g) for g in got] == [M] * 3


def test_special_scores(ctx):
    n = 300
    rng = np.random.default_rng(11)
    b = R.clustered_boxes(rng, n, 8)
    s = R.score_columns(rng, n, 6)
    s[rng.choice(n, 60, replace=False), 0] = np.nan                    # NaN in some columns only
    s[rng.choice(n, 7, replace=False), 3] = np.nan
    s[rng.choice(n, 9, replace=False), 3] = np.inf
    s[rng.choice(n, 9, replace=False), 3] = -np.inf
    s[:, 4] = np.where(rng.uniform(0, 1, n) < 0.5, 0.0, -0.0)          # -0 == +0: index order
    s[rng.choice(n, 20, replace=False), 4] = 1.0
    s[rng.choice(n, 20, replace=False), 4] = -1.0
    for M in (7, n):
        got = _check(ctx, b, s, 0.3, M, what="special scores, M=%d" % M)
    for q in (0, 3):
        assert not any(np.isnan(s[i, q]) for i in got[q])
    # a NaN row neither leads nor suppresses
    one = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [100, 100, 110, 110]], np.float32)
    sc = np.array([[np.nan], [0.5], [0.9]], np.float32)
    assert _check(ctx, one, sc, 0.3, 3, what="NaN twin") == [[2, 1]]


@pytest.mark.parametrize("n", [130, 1000])
def test_validity(ctx, n):
    rng = np.random.default_rng(13 + n)
    b = R.clustered_boxes(rng, n, 8)
    s = R.score_columns(rng, n, 4)
    s[:, 1] = np.nan                                                   # a column that is all NaN
    s[rng.choice(n, 30, replace=False), 0] = np.nan
    valid = (rng.uniform(0, 1, n) < 0.5).astype(np.uint8)
    for M in (7, n):
        got = _check(ctx, b, s, 0.3, M, valid, what="valid mask, M=%d" % M)
        assert got[1] == [] and all(valid[i] for g in got for i in g)
    got = _check(ctx, b, s, 0.3, 7, np.zeros((n,), np.uint8), what="all rows invalid")
    assert got == [[], [], [], []]
    # a valid mask of ones is no mask
    assert _check(ctx, b, s, 0.3, n, np.ones((n,), np.uint8), what="all valid") == _check(ctx, b, s, 0.3, n, what="no mask")


def test_a_column_does_not_depend_on_the_others(ctx):
    from densecap_amd import ops
    n, Q = 1000, 70
    rng = np.random.default_rng(17)
    b = R.clustered_boxes(rng, n, 100)
    s = R.score_columns(rng, n, Q)
    s[rng.choice(n, 50, replace=False), 5] = np.nan
    for M in (7, n):
        picks, counts = ops.nms_multi(ctx, b, s, 0.5, M)
        for q in (0, 1, 5, 33, 69):
            p1, c1 = ops.nms_multi(ctx, b, np.ascontiguousarray(s[:, q:q + 1]), 0.5, M)
            assert c1[0] == counts[q] and np.array_equal(p1[0], picks[q]), q
        perm = rng.permutation(Q)
        pp, cp = ops.nms_multi(ctx, b, np.ascontiguousarray(s[:, perm]), 0.5, M)
        assert np.array_equal(cp, counts[perm]) and np.array_equal(pp, picks[perm])


@pytest.mark.parametrize("n,per,thr,maxb", [(1000, 8, 0.3, None), (4096, 100, 0.5, None), (2000, 8, 0.7, 300), (130, 10, 0.5, 5)])
def test_equals_the_single_order_nms_on_a_clean_column(ctx, n, per, thr, maxb):
    from densecap_amd import ops
    rng = np.random.default_rng(n)
    b = R.clustered_boxes(rng, n, per)
    s = R.score_columns(rng, n, 3)
    M = n if maxb is None else maxb
    got = R.as_lists(*ops.nms_multi(ctx, b, s, thr, M))
    for q in range(3):
        assert got[q] == ops.nms(ctx, np.concatenate([b, s[:, q:q + 1]], 1), thr, maxb).tolist(), q


def test_refusals_leave_the_ctx_usable(ctx):
    from densecap_amd import ops
    rng = np.random.default_rng(19)
    n = 4097
    b = ctx.to_device(R.clustered_boxes(rng, n, 8)); s = ctx.to_device(R.score_columns(rng, n, 2))
    picks = ctx.empty((2, 4096), np.int32); cnt = ctx.empty((2,), np.int32)
    call = lambda n_, Q, M, bp=b, sp=s, pp=picks, cp=cnt: ctx.lib.dc_op_nms_multi(
        ctx.h, bp.ptr if bp else None, sp.ptr if sp else None, None, n_, Q, C.c_float(0.5), M, pp.ptr if pp else None,
        cp.ptr if cp else None)
    DC_E_INVALID, DC_E_UNSUPPORTED = -1, -5
    assert call(4097, 2, 7) == DC_E_UNSUPPORTED and b"4096" in ctx.lib.dc_last_error(ctx.h)
    for n_, Q, M in ((100, 2, 0), (100, 2, -1), (100, 2, 4097), (100, 0, 7), (100, -3, 7), (0, 2, 7), (-1, 2, 7)):
        assert call(n_, Q, M) == DC_E_INVALID, (n_, Q, M)
    assert call(100, 2, 7, bp=None) == DC_E_INVALID and call(100, 2, 7, sp=None) == DC_E_INVALID
    assert call(100, 2, 7, pp=None) == DC_E_INVALID and call(100, 2, 7, cp=None) == DC_E_INVALID
    with pytest.raises(Exception, match="dc_op_nms_multi"):
        ops.nms_multi(ctx, R.clustered_boxes(rng, 4097, 8), R.score_columns(rng, 4097, 1), 0.5, 7)
    assert call(4096, 2, 4096) == 0                                    # the largest call, on the buffers of the refused one
    _check(ctx, R.clustered_boxes(rng, 200, 8), R.score_columns(rng, 200, 3), 0.5, 7, what="after the refusals")
