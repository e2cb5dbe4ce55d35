"""CPU: the reference of the evaluation tests (tests/eval_rules.py) on hand-worked cases, its two forms against each other, and
the teeth of the comparison the GPU tests use."""
import copy

import numpy as np

from tests import eval_rules as R

F = np.float32


def test_threshold_count_is_100():
    t = R.recall_thresholds()
    assert len(t) == 100 and t[0] == 0.0 and 0.98 < t[-1] < 1.0
    acc = 0.0
    for _ in range(100):
        acc += 0.01
    assert acc > 1.0                                    # why the 101st iteration never runs


def test_merge_threshold_reads_the_float_as_the_decimal_it_was_written_as():
    assert R.merge_threshold(F(0.7)) == 0.7 and float(F(0.7)) != 0.7
    assert R.merge_threshold(0.5) == 0.5 and R.merge_threshold(1.0) == 1.0 and R.merge_threshold(F(0.3)) == 0.3
    x = np.nextafter(F(0.7), F(1))
    assert F(R.merge_threshold(x)) == x and R.merge_threshold(x) != 0.7


def test_exact_ious():
    big, strip, half = [0, 0, 9, 9], [0, 0, 9, 6], [0, 0, 9, 4]
    assert R.iou(big, strip) == 70 / 100 == 0.7         # 10x7 nested in 10x10
    assert R.iou(big, half) == 0.5
    assert R.iou(big, [10, 0, 19, 9]) == 0.0 and R.iou(big, [9, 9, 18, 18]) == 1 / 199
    c = R.corners(R.to_xcycwh([big, strip, half]))
    assert c.dtype == F and c.tolist() == [big, strip, half]
    # the 10x7 box merges with its 10x10 parent at 0.7 (>=), the 10x5 box does not
    assert R.merge_boxes(c[[0, 1]], 0.7) == [[0, 1]] and R.merge_boxes(c[[0, 2]], 0.7) == [[0], [1]]
    # all three: the 10x7 box overlaps both others (50/70 with the 10x5 box), its column counts 3 and takes everything
    assert R.merge_boxes(c, 0.7) == [[0, 1, 2]]
    r = R.match_image(R.to_xcycwh([half]), [0.5], R.to_xcycwh([big]))
    assert r["ov"].tolist() == [0.5] and r["ok"].tolist() == [1] and r["group"].tolist() == [0]
    ev = R.evaluate([0.5], r["ok"], r["ov"], 1)
    assert ev["det_breakdown"]["ov0.5"] == 1.0 and ev["det_breakdown"]["ov0.6"] == 0.0 and ev["det_breakdown"]["ov0.3"] == 1.0


def test_nan_follows_lua_max_min():
    nan = float("nan")
    assert R._max(nan, 1.0) != R._max(nan, 1.0) and R._max(1.0, nan) == 1.0
    a, b = [nan, 0, 9, 9], [0, 0, 9, 9]
    # a NaN in the second box is skipped by max (the intersection is then positive and the NaN comes back through the area);
    # in the first box it stays and fails `iw > 0`: the order of the two matters
    assert R.iou(a, b) == 0.0 and np.isnan(R.iou(b, a))
    assert R.iou_row(a, [b])[0] == 0.0 and np.isnan(R.iou_row(b, [a])[0])


def test_two_ground_truth_boxes_three_detections_by_hand():
    gt = R.to_xcycwh([[0, 0, 9, 9], [100, 100, 119, 119]])
    det = R.to_xcycwh([[0, 0, 9, 9], [500, 500, 520, 520], [100, 100, 119, 119]])
    sc = [0.9, 0.8, 0.7]
    th = R.recall_thresholds()
    low = sum(1 for t in th if t <= 0.5)
    assert low in (50, 51)

    def by_hand(p_low, p_high):
        ap = 0.0
        for t in th:
            ap += p_low if t <= 0.5 else p_high
        return ap / 100
    # without the used[-1] rule: tp, fp, tp -> rec .5 .5 1, prec 1 .5 2/3
    r = R.match_image(det, sc, gt, claim_last=False)
    assert (r["order"].tolist(), r["group"].tolist(), r["ok"].tolist(), r["ov"].tolist()) == ([0, 1, 2], [0, -1, 1], [1, 0, 1], [1.0, 0.0, 1.0])
    ev = R.evaluate(sc, r["ok"], r["ov"], r["n_groups"])
    assert ev["detmap"] == by_hand(1.0, 2 / 3) and ev["map"] is None and ev["ap_breakdown"] is None
    assert set(ev["det_breakdown"]) == {"ov0.3", "ov0.4", "ov0.5", "ov0.6", "ov0.7"}
    # the reference rule: the detection that overlaps nothing takes the last group, its true match comes too late
    r = R.match_image(det, sc, gt, claim_last=True)
    assert r["group"].tolist() == [0, -1, 1] and r["ok"].tolist() == [1, 1, 0]
    ev = R.evaluate(sc, r["ok"], r["ov"], r["n_groups"])
    assert ev["detmap"] == by_hand(1.0, 0.0)
    # with caption scores: the rows of ap_breakdown are keyed as the reference keys them
    ev = R.evaluate(sc, [1, 0, 1], [1.0, 0.0, 1.0], 2, caption_scores=[0.12, 0.5, 0.3])
    assert len(ev["ap_breakdown"]) == 30 and "ov0.3_score0.05" in ev["ap_breakdown"] and "ov0.7_score0" in ev["ap_breakdown"]
    assert ev["ap_breakdown"]["ov0.5_score0.1"] == by_hand(1.0, 2 / 3)          # both still score above 0.1
    assert ev["ap_breakdown"]["ov0.5_score0.15"] == by_hand(1 / 3, 0.0)   # only the third record is a tp: rec 0 0 .5, prec 0 0 1/3


def test_merge_takes_the_largest_count_first_not_connectivity():
    # a chain: A ~ B and B ~ C at >= 0.7, A and C below it.  B's column counts 3 and wins: one group of all three, although A and C
    # do not overlap enough themselves
    A, B, C = [0, 0, 99, 9], [15, 0, 114, 9], [30, 0, 129, 9]
    assert R.iou(A, B) >= 0.7 > R.iou(A, C)
    c = np.asarray([A, B, C], F)
    assert R.merge_boxes(c, 0.7) == [[0, 1, 2]]
    # a longer chain A ~ B ~ C ~ D: B (index 1) and C tie at 3, the lower index wins and D is left on its own
    Dd = [45, 0, 144, 9]
    assert R.merge_boxes(np.asarray([A, B, C, Dd], F), 0.7) == [[0, 1, 2], [3]]
    # ... in whatever order the boxes come: the winner is the lowest INDEX among the tied columns
    assert R.merge_boxes(np.asarray([Dd, C, B, A], F), 0.7) == [[0, 1, 2], [3]]
    assert R.merge_boxes(np.asarray([A, Dd, C, B], F), 0.7) == [[1, 2, 3], [0]]


def test_duplicates_merge_and_groups_are_numbered_by_creation():
    one, far = [10, 10, 40, 40], [300, 300, 350, 350]
    c = np.asarray([far, one, one, one, far], F)
    assert R.merge_boxes(c, 0.7) == [[1, 2, 3], [0, 4]]              # the larger group first
    r = R.match_image(np.zeros((0, 4), F), [], R.to_xcycwh(c))
    assert r["gt_group"].tolist() == [1, 0, 0, 0, 1] and r["n_groups"] == 2
    assert r["merged"].tolist() == [[10.0, 10.0, 40.0, 40.0], [300.0, 300.0, 350.0, 350.0]]


def test_merged_box_is_a_float32_mean():
    c = np.asarray([[0, 0, 10, 10], [1, 0, 10, 11], [1, 1, 11, 11]], F)
    m = R.merged_box(c, [0, 1, 2])
    assert m.dtype == np.float64 and m.tolist() == [float(F(2) / F(3)), float(F(1) / F(3)), float(F(31) / F(3)), float(F(32) / F(3))]
    assert m[0] != 2 / 3


def test_claim_modes_differ_only_where_a_detection_overlaps_nothing():
    rng = np.random.default_rng(3)
    gt = R.clustered_gt(rng, 40, 4)
    s = R.special_scores(rng, 120)
    d = R.detections_for(rng, gt, 120, far=0.0)
    a, b = (R.match_image(d, s, gt, claim_last=cl) for cl in (True, False))
    assert (a["group"] >= 0).all() and R.first_difference(a, b) is None
    d = R.detections_for(rng, gt, 120, far=0.5)
    a, b = (R.match_image(d, s, gt, claim_last=cl) for cl in (True, False))
    assert (a["group"] == -1).any() and np.array_equal(a["group"], b["group"]) and a["ov"].tobytes() == b["ov"].tobytes()
    assert not np.array_equal(a["ok"], b["ok"]) and not b["ok"][b["group"] == -1].any()
    # no ground truth: nothing to claim in either mode
    for cl in (True, False):
        r = R.match_image(d, s, np.zeros((0, 4), F), claim_last=cl)
        assert r["n_groups"] == 0 and not r["ok"].any() and (r["group"] == -1).all()


def test_fast_form_equals_the_literal_loops():
    rng = np.random.default_rng(4)
    for B, M, per in ((40, 20, 4), (30, 40, 40), (10, 0, 1), (0, 5, 1), (50, 30, 1), (70, 12, 2)):
        gt = R.clustered_gt(rng, M, per) if M else np.zeros((0, 4), F)
        d = R.detections_for(rng, gt, B); s = R.special_scores(rng, B)
        if B > 5:
            d[3, 1] = np.nan; d[4, 2] = np.inf; d[5, 2:] = 0
        if M > 5:
            gt[2, 0] = np.nan; gt[3, 3] = -np.inf; gt[4, 2:] = 0
        for cl in (True, False):
            assert R.first_difference(R.match_image(d, s, gt, 0.7, cl, fast=True), R.match_image(d, s, gt, 0.7, cl)) is None
    g = R.on_threshold_gt(20)
    assert [len(m) for m in R.merge_boxes(R.corners(g), 0.7, fast=True)] == [2] * 10


def test_score_order():
    nan, inf = float("nan"), float("inf")
    assert R.score_order([0.5, nan, 0.5, inf, -inf, 0.0, -0.0, 0.7, nan]) == [3, 7, 0, 2, 5, 6, 4, 1, 8]


# ---- teeth: the comparison goes red on each of these ------------------------------------------------------------------------------
def _case():
    rng = np.random.default_rng(6)
    gt = R.clustered_gt(rng, 30, 4)
    d = R.detections_for(rng, gt, 60, far=0.2)
    s = np.round(rng.uniform(0, 1, 60), 1).astype(F)             # many ties
    return d, s, gt, R.match_image(d, s, gt)


def test_teeth_swapped_tied_detections():
    d, s, gt, ref = _case()
    k = next(i for i in range(59) if s[ref["order"][i]] == s[ref["order"][i + 1]])
    bad = copy.deepcopy(ref)
    bad["order"][[k, k + 1]] = bad["order"][[k + 1, k]]
    assert R.first_difference(ref, copy.deepcopy(ref)) is None and "order" in R.first_difference(bad, ref)


def test_teeth_claim_given_to_the_second_detection():
    d, s, gt, ref = _case()
    g = next(int(g) for g in ref["group"] if g >= 0 and (ref["group"] == g).sum() >= 2 and ref["ok"][np.flatnonzero(ref["group"] == g)[0]])
    first, second = np.flatnonzero(ref["group"] == g)[:2]
    assert ref["ok"][first] == 1 and ref["ok"][second] == 0
    bad = copy.deepcopy(ref)
    bad["ok"][first], bad["ok"][second] = 0, 1
    assert "ok" in R.first_difference(bad, ref)


def test_teeth_group_numbered_out_of_creation_order():
    d, s, gt, ref = _case()
    assert ref["n_groups"] >= 2
    bad = copy.deepcopy(ref)
    swap = {0: 1, 1: 0}
    bad["gt_group"] = np.asarray([swap.get(int(g), int(g)) for g in ref["gt_group"]], np.int32)
    bad["group"] = np.asarray([swap.get(int(g), int(g)) for g in ref["group"]], np.int32)
    bad["merged"] = ref["merged"].copy(); bad["merged"][[0, 1]] = ref["merged"][[1, 0]]
    assert R.first_difference(bad, ref) is not None


def test_teeth_ov_one_ulp_off():
    d, s, gt, ref = _case()
    bad = copy.deepcopy(ref)
    k = int(np.flatnonzero(ref["ov"] > 0)[0])
    bad["ov"][k] = np.nextafter(bad["ov"][k], 2.0)
    assert "ov" in R.first_difference(bad, ref)


def test_teeth_101_point_ap():
    d, s, gt, ref = _case()
    a100 = R.evaluate(s[ref["order"]], ref["ok"], ref["ov"], ref["n_groups"])
    a101 = R.evaluate(s[ref["order"]], ref["ok"], ref["ov"], ref["n_groups"], thresholds=[k / 100 for k in range(101)])
    assert a100["detmap"] != a101["detmap"] and a100["det_breakdown"] != a101["det_breakdown"]
