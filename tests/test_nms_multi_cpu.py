"""CPU: the reference of the multi-order NMS tests (tests/nms_multi_rules.py) is the oracle's box_utils.nms where the two agree
by definition, its candidate rule is compaction, and the comparison the GPU tests make detects the mistakes a kernel could make."""
import numpy as np
import pytest

from oracle import densecap_oracle as O
from tests import nms_multi_rules as R


def _case(seed=0, n=300, Q=5, per=8):
    rng = np.random.default_rng(seed)
    return R.clustered_boxes(rng, n, per), R.score_columns(rng, n, Q)


@pytest.mark.parametrize("M", [1, 7, 300])
def test_reference_is_the_oracle_on_clean_columns(M):
    b, s = _case()
    ref = R.nms_multi_ref(b, s, 0.3, M)
    for q in range(s.shape[1]):
        assert ref[q] == O.nms(np.concatenate([b, s[:, q:q + 1]], 1), 0.3, M).tolist()
        assert ref[q] == O.nms_py(np.concatenate([b, s[:, q:q + 1]], 1), 0.3, M).tolist()
    assert ref[2] == ref[0]                                   # the copied column
    full = R.nms_multi_ref(b, s, 0.3, 300)
    assert full[4] == sorted(full[4])                         # the constant column: index order


def test_nan_and_valid_rule_is_compaction():
    b, s = _case(1)
    rng = np.random.default_rng(2)
    s[rng.choice(300, 40, replace=False), 1] = np.nan
    s[rng.choice(300, 5, replace=False), 3] = np.inf
    s[rng.choice(300, 5, replace=False), 3] = -np.inf
    s[:, 0] = np.nan                                          # a column without candidates
    valid = rng.uniform(0, 1, 300) < 0.6
    ref = R.nms_multi_ref(b, s, 0.4, 20, valid)
    assert ref[0] == []
    for q in range(1, 5):
        keep = np.flatnonzero(valid & ~np.isnan(s[:, q]))
        packed = O.nms(np.concatenate([b[keep], s[keep, q:q + 1]], 1), 0.4, 20)
        assert ref[q] == keep[packed].tolist()
        assert all(valid[i] and not np.isnan(s[i, q]) for i in ref[q])
    # a NaN row is not ranked first (the single-order NMS would pick it), and it does not suppress its neighbours either
    one = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [100, 100, 110, 110]], np.float32)
    sc = np.array([[np.nan], [0.5], [0.9]], np.float32)
    assert R.nms_multi_ref(one, sc, 0.3, 3) == [[2, 1]]
    assert O.nms(np.concatenate([one, sc], 1), 0.3, 3).tolist() == [0, 2]


def test_ties_zero_signs_and_infinities():
    b = R.disjoint_boxes(6)
    s = np.array([[0.5, 0.0, np.inf], [0.5, -0.0, 1.0], [0.7, 0.0, -np.inf], [0.5, -0.0, np.inf], [0.1, 1.0, 0.0], [0.7, -1.0, 2.0]],
                 np.float32)
    assert R.nms_multi_ref(b, s, 0.3, 6) == [[2, 5, 0, 1, 3, 4], [4, 0, 1, 2, 3, 5], [0, 3, 5, 1, 4, 2]]


def test_the_comparison_has_teeth():
    b, s = _case(3)
    s[::7, 1] = np.nan
    ref = R.nms_multi_ref(b, s, 0.3, 300)
    M = 300
    picks = np.full((5, M), -1, np.int32); counts = np.zeros((5,), np.int32)
    for q, p in enumerate(ref):
        picks[q, :len(p)] = p; counts[q] = len(p)
    assert R.first_difference(R.as_lists(picks, counts), ref) is None
    # two tied picks swapped (column 1 is rounded; on disjoint boxes every row is a pick, so tied neighbours exist)
    d = R.nms_multi_ref(R.disjoint_boxes(300), s, 0.3, 300)
    p1 = d[1]
    k = next(i for i in range(len(p1) - 1) if s[p1[i], 1] == s[p1[i + 1], 1])
    assert p1[k] < p1[k + 1]                                  # the lower index first
    swapped = [list(p) for p in d]
    swapped[1][k], swapped[1][k + 1] = swapped[1][k + 1], swapped[1][k]
    assert "query 1" in R.first_difference(swapped, d) and "pick %d" % k in R.first_difference(swapped, d)
    # a suppressed box's suppressor dropped: the best-scoring box that was not picked (something better suppressed it) takes
    # its suppressor's place
    p0 = ref[0]
    victim = int(next(j for j in np.argsort(-s[:, 0], kind="stable") if j not in set(p0)))
    k = max(i for i in range(len(p0)) if s[p0[i], 0] >= s[victim, 0])
    bad = picks.copy(); bad[0, k] = victim
    assert "query 0" in R.first_difference(R.as_lists(bad, counts), ref)
    # a NaN row picked
    bad = picks.copy(); bc = counts.copy()
    bad[1, bc[1]] = 0; bc[1] += 1                               # row 0 of column 1 is NaN
    assert np.isnan(s[0, 1]) and "query 1" in R.first_difference(R.as_lists(bad, bc), ref)
    # a count that hides picks, and padding that is not -1
    bc = counts.copy(); bc[2] -= 1
    with pytest.raises(AssertionError, match="must be -1"):
        R.as_lists(picks, bc)
