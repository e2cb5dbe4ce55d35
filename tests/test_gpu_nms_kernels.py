"""The single-order NMS (launch_nms: nms_hist_kernel .. nms_scan_band_kernel) and the multi-order one on crafted operands, through
the hooks of include/densecap_debug_nms.h.

The cases are those of tests/nms_rules.py: each reaches a named path by construction (tests/test_nms_rules_cpu.py asserts that it
does, and that its expected picks are the oracle's).  Every case runs on both scans (dc_debug_set "nms_band" 0 and 1) and is held
to list equality: picks, count, the workspace's sorted order and nvalid, and the sentinel in every output entry past the count and
in every guard row.  No model and no weights."""
import numpy as np
import pytest

from tests import nms_multi_rules as M
from tests import nms_rules as R

pytestmark = pytest.mark.gpu

DC_E_INVALID, DC_E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


def _last_error(ctx):
    msg = ctx.lib.dc_last_error(ctx.h)
    return msg.decode() if msg else ""


def _on_both_scans(ctx, fn):
    """fn(scan name) with the chunk scan, then with the band scan (the default, restored whatever happens)"""
    from densecap_amd._lib import check
    try:
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"nms_band", 0), "dc_debug_set")
        fn("chunk scan")
    finally:
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"nms_band", 1), "dc_debug_set")
    fn("band scan")


def _run(ctx, case, what, n_dev=None, ws_rows=None, order=None):
    """one call on the current scan; picks, count, order[:nvalid], nvalid and every sentinel must be exactly the case's"""
    from densecap_amd import ops
    n = len(case.boxes5)
    cap = n if case.max_boxes is None else min(n, case.max_boxes)
    res = ops.nms_debug(ctx, case.boxes5, case.thresh, case.max_boxes, case.valid, n_dev, ws_rows)
    if order is None:
        order = R.sorted_order(case.boxes5[:, 4], case.valid, n_dev)
    diff = R.first_difference(res, case.expected, order, n, cap)
    assert diff is None, "%s: %s" % (what, diff)
    return res


def _check(ctx, case, name, n_dev=None, ws_rows=None):
    order = R.sorted_order(case.boxes5[:, 4], case.valid, n_dev)
    _on_both_scans(ctx, lambda scan: _run(ctx, case, "%s, %s" % (name, scan), n_dev, ws_rows, order))


# ---- the sort: disjoint boxes, no budget -- the picks are the sorted order ------------------------------------------------------------
@pytest.mark.parametrize("name", R.sort_names())
def test_sort(ctx, name):
    case = R.sort_build(name)
    assert case.expected == R.sorted_order(case.boxes5[:, 4], case.valid)
    _check(ctx, case, name)


# ---- the scan of one window -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SCAN))
def test_scan_one_window(ctx, name):
    case = R.scan_build(name)
    assert len(case.boxes5) <= R.WIN0
    _check(ctx, case, name)


# ---- the window ladder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.WINDOWS))
def test_windows(ctx, name):
    _check(ctx, R.window_build(name), name)


@pytest.mark.parametrize("n", [4097, 16386])
def test_staircase_across_windows(ctx, n):
    """one dependency chain from the first row to the last, through every border"""
    b5, exp, facts = R.staircase(n, n)
    for mb in (None, 2000):
        _check(ctx, R.Case(b5, 0.5, mb, None, exp[:mb], facts), "staircase %d, max_boxes %s" % (n, mb))


# ---- the budget --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disjoint", "staircase"])
@pytest.mark.parametrize("max_boxes", R.BUDGETS)
def test_budget(ctx, kind, max_boxes):
    """the count is exactly the budget (or every pick there is) and windows after the one that meets it add nothing"""
    case = R.budget_build(kind, max_boxes)
    assert len(case.expected) == min(max_boxes, case.facts["uncut"])
    _check(ctx, case, "%s, max_boxes %d" % (kind, max_boxes))


# ---- the device-side row count -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev", R.DEV_COUNTS)
def test_device_count(ctx, n_dev):
    """the final NMS's form (n_dev, no valid bytes, max_boxes -1) and the three forms next to it; the rows past the count hold NaN
    boxes, +inf scores and valid = 1, and must not show"""
    for with_valid in (False, True):
        for mb in (None, 20):
            case = R.device_count_build(n_dev, with_valid, mb, seed=3 * int(with_valid) + (mb or 0))
            _check(ctx, case, "n_dev %d, valid %s, max_boxes %s" % (n_dev, with_valid, mb), n_dev=n_dev)


def test_device_count_across_windows(ctx):
    """a count inside window 1 of a list that would have three: the host launches every window, the device closes the run early"""
    n, n_dev = 37000, 4096 + 700
    rng = np.random.default_rng(5)
    b5, _ = R.poison_tail(R.clustered_boxes5(rng, n, 40), None, n_dev)
    for mb in (None, 3000):
        case = R.Case(b5, 0.5, mb, None, R.reference(b5, 0.5, mb, None, n_dev), {})
        _check(ctx, case, "n_dev %d of %d, max_boxes %s" % (n_dev, n, mb), n_dev=n_dev)


# ---- the workspace of a larger call --------------------------------------------------------------------------------------------------------
def test_workspace_reuse_after_a_larger_call(ctx):
    """The forward's final NMS runs on 1000 rows with a device count in the workspace bound for, and last used by, the 20,520-row
    RPN NMS: the mask, the near band and the bucket pairs of the larger call are where the smaller one's will be."""
    big_n, n, n_dev = 20520, 1000, 300

    def body(scan):
        first = None
        for rep in range(3):
            rng = np.random.default_rng(100 + rep)
            big5 = R.clustered_boxes5(rng, big_n, 25, scores=np.round(rng.uniform(0, 1, big_n), 3))
            big = R.Case(big5, 0.7, 1000, None, R.reference(big5, 0.7, 1000), {})
            _run(ctx, big, "the 20,520-row call, round %d, %s" % (rep, scan), ws_rows=big_n)
            b5, _ = R.poison_tail(R.clustered_boxes5(rng, n, 8), None, n_dev)
            small = R.Case(b5, 0.3, None, None, R.reference(b5, 0.3, None, None, n_dev), {})
            res = _run(ctx, small, "the 1000-row call, round %d, %s" % (rep, scan), n_dev=n_dev, ws_rows=big_n)
            if rep == 0:
                first = (small, res)
        again = _run(ctx, first[0], "round 0 again, %s" % scan, n_dev=n_dev, ws_rows=big_n)
        for k in ("picks", "count", "nvalid"):
            assert np.array_equal(again[k], first[1][k]), k
        assert np.array_equal(again["order"][:n_dev], first[1]["order"][:n_dev])
    _on_both_scans(ctx, body)


# ---- the multi-order NMS under a device count ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev", [0, 1, 64, 299, 300, 305, -3])
def test_nms_multi_device_count(ctx, n_dev):
    from densecap_amd import ops
    n, Q, g = 300, 3, 2
    live = R.live_rows(n, n_dev)
    rng = np.random.default_rng(7)
    b = M.clustered_boxes(rng, n, 8)
    s = M.score_columns(rng, n, Q)
    for valid in (None, (rng.uniform(0, 1, n) < 0.7).astype(np.uint8)):
        bp, sp = b.copy(), s.copy()
        bp[live:] = np.nan
        sp[live:] = np.inf
        vp = None
        if valid is not None:
            vp = valid.copy()
            vp[live:] = 1
        for mp in (7, n):
            what = "n_dev %d, valid %s, max_picks %d" % (n_dev, valid is not None, mp)
            res = ops.nms_multi_debug(ctx, bp, sp, 0.5, mp, vp, n_dev)
            assert res["rc"] == 0 and res["picks"].shape == (Q + g, mp)
            assert (res["picks"][Q:] == R.I32_FILL).all() and (res["counts"][Q:] == R.I32_FILL).all(), what
            got = M.as_lists(res["picks"][:Q], res["counts"][:Q])                 # (checks the -1 padding)
            ref = M.nms_multi_ref(bp[:live], sp[:live], 0.5, mp, None if vp is None else vp[:live])
            diff = M.first_difference(got, ref)
            assert diff is None, "%s: %s" % (what, diff)
    # a null count is the whole list: dc_op_nms_multi's result
    res = ops.nms_multi_debug(ctx, b, s, 0.5, 7)
    p, c = ops.nms_multi(ctx, b, s, 0.5, 7)
    assert np.array_equal(res["picks"][:Q], p) and np.array_equal(res["counts"][:Q], c)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _untouched(res, keys):
    return all((res[k] == R.I32_FILL).all() for k in keys)


def test_refusals_launch_nothing(ctx):
    """each call breaks one rule only; the sentinel-filled outputs stay as they were and the ctx stays usable"""
    from densecap_amd import ops
    case = R.device_count_build(R.DEV_N, True, None)
    n = len(case.boxes5)
    keys = ("picks", "count", "order", "nvalid")
    broken = [("null boxes", dict(null=("boxes",))), ("null scores", dict(null=("scores",))), ("null picks", dict(null=("picks",))),
              ("null count", dict(null=("count",))), ("n = 0", dict(n=0)), ("n = -1", dict(n=-1)),
              ("ws_rows below n", dict(ws_rows=n - 1)), ("max_boxes = -2", dict(max_boxes=-2))]
    for what, kw in broken:
        args = dict(max_boxes=None, valid=case.valid, n_dev=n, ws_rows=n, raise_errors=False)
        args.update(kw)
        res = ops.nms_debug(ctx, case.boxes5, case.thresh, **args)
        assert res["rc"] == DC_E_INVALID, what
        assert "dc_debug_nms" in _last_error(ctx), what
        assert _untouched(res, keys), "%s: a refused call wrote to its outputs" % what
    _run(ctx, case, "after the refusals", n_dev=n)

    b = M.clustered_boxes(np.random.default_rng(3), 4097, 8)
    s = M.score_columns(np.random.default_rng(4), 4097, 2)
    broken = [("null boxes", dict(null=("boxes",)), DC_E_INVALID), ("null scores", dict(null=("scores",)), DC_E_INVALID),
              ("null picks", dict(null=("picks",)), DC_E_INVALID), ("null counts", dict(null=("counts",)), DC_E_INVALID),
              ("n = 0", dict(n=0), DC_E_INVALID), ("Q = 0", dict(Q=0), DC_E_INVALID), ("max_picks = 0", dict(max_picks=0), DC_E_INVALID),
              ("max_picks = 4097", dict(max_picks=4097), DC_E_INVALID), ("n = 4097", dict(n=4097), DC_E_UNSUPPORTED)]
    for what, kw, rc in broken:
        args = dict(max_picks=7, n=100, n_dev=100, raise_errors=False)
        args.update(kw)
        res = ops.nms_multi_debug(ctx, b, s, 0.5, **args)
        assert res["rc"] == rc, what
        assert "dc_debug_nms_multi" in _last_error(ctx), what
        assert _untouched(res, ("picks", "counts")), "%s: a refused call wrote to its outputs" % what
    res = ops.nms_multi_debug(ctx, b[:200], s[:200], 0.5, 7, n_dev=200)
    assert M.first_difference(M.as_lists(res["picks"][:2], res["counts"][:2]), M.nms_multi_ref(b[:200], s[:200], 0.5, 7)) is None
