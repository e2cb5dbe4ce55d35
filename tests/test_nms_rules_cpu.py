"""tests/nms_rules.py on the CPU: every builder's closed form is the oracle's list (the C restatement, and nms_py where the list is
short enough for it), every case reaches the path it is named for -- asserted from the restated bucket and window arithmetic --
and the comparison the GPU tests use fails on six wrong variants of the rule."""
import numpy as np
import pytest

from oracle import densecap_oracle as O
from tests import nms_rules as R

PY_ROWS = 5000                # nms_py is one numpy pass per pick: lists up to this size are also held against it


def _holds(case, name):
    ref = R.reference(case.boxes5, case.thresh, case.max_boxes, case.valid)
    assert case.expected == ref, "%s: closed form differs from the oracle" % name
    if len(case.boxes5) <= PY_ROWS:
        assert case.expected == R.reference(case.boxes5, case.thresh, case.max_boxes, case.valid, nms=O.nms_py), name
    return ref


# ---- the restated arithmetic ------------------------------------------------------------------------------------------------------
def test_sort_key_orders_as_the_oracle_sorts():
    """ascending (key, index) is the oracle's order on every special value at once"""
    rng = np.random.default_rng(1)
    u = np.concatenate([rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32),
                        np.uint32([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff,
                                   0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001] * 3)])
    s = rng.permutation(u).view(np.float32)
    b5, order, _ = R.sort_case(s)
    assert order == O.nms(b5, 0.5).tolist() == O.nms_py(b5, 0.5).tolist()
    k = R.sort_key(s)
    assert (k[np.isnan(s)] == 0).all() and k[s == 0].tolist() == [0x7fffffff] * int((s == 0).sum())
    assert (R.sort_key(s, np.zeros(len(s), np.uint8)) == 0xffffffff).all()
    assert (R.bucket(k) == (k >> 16)).all() and R.bucket(np.uint32([0xffffffff]))[0] == 65535


def test_window_ladder():
    assert [R.win_start(k) for k in range(4)] == [0, 4096, 36864, 69632]
    assert [R.win_start(k, True) for k in range(4)] == [0, 4096, 12288, 45056]
    assert R.windows(4096) == [(0, 4096)] and R.windows(4097) == [(0, 4096), (4096, 4097)]
    assert R.windows(12289, 2000) == [(0, 4096), (4096, 12288), (12288, 12289)] and R.windows(12288, 2000) == [(0, 4096), (4096, 12288)]
    assert R.windows(12289, 1024) == R.windows(12289) == [(0, 4096), (4096, 12289)]
    assert R.windows(37000) == [(0, 4096), (4096, 36864), (36864, 37000)]
    assert [R.window_of(p, 37000) for p in (0, 4095, 4096, 36863, 36864)] == [0, 0, 1, 1, 2]
    assert R.live_rows(10, None) == 10 and [R.live_rows(10, c) for c in (-3, 0, 9, 10, 15)] == [0, 0, 9, 10, 10]


# ---- the sort cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.sort_names())
def test_sort_cases(name):
    c = R.sort_build(name)
    _holds(c, name)
    assert c.expected == R.sorted_order(c.boxes5[:, 4], c.valid)
    s, f = c.boxes5[:, 4], c.facts
    if name.startswith("equal_"):
        assert c.expected == list(range(len(s))) and len(f["buckets"]) == 1 and f["buckets"][0].cnt == len(s)
    if name == "one_bucket_distinct_keys":
        assert len(f["buckets"]) == 1 and len(set(R.sort_key(s).tolist())) == len(s) and c.expected != sorted(c.expected)
    if name == "negative_logits":
        assert (s < 0).all() and np.isfinite(s).all() and len(set(s.tolist())) < len(s)
    if name == "mixed_signs":
        assert (s < 0).sum() > 1000 and (s > 0).sum() > 1000
    if name == "signed_zeros":
        z = np.flatnonzero(s == 0)
        assert np.signbit(s[z]).any() and not np.signbit(s[z]).all()
        assert [i for i in c.expected if s[i] == 0] == z.tolist()        # the two zeros tie: index order
    if name == "denormals":
        a = np.abs(s)
        assert ((a > 0) & (a < np.float32(1.17549435e-38)) & (s > 0)).sum() >= 100 and ((a > 0) & (a < np.float32(1.17549435e-38)) & (s < 0)).sum() >= 100
    if name == "infinities":
        assert np.isposinf(s[c.expected[0]]) and np.isneginf(s[c.expected[-1]])
    if name == "nan_first":
        k = int(np.isnan(s).sum())
        assert k > 40 and np.isnan(s[c.expected[:k]]).all() and c.expected[:k] == sorted(c.expected[:k])
        assert (s.view(np.uint32)[np.isnan(s)] >> 31).any()
    if name.startswith("valid_"):
        assert f["nvalid"] == int(name.split("_")[1]) == int(c.valid.sum()) < len(s)
        assert f["buckets"][-1].bucket == 65535 and f["buckets"][-1].cnt == len(s) - f["nvalid"]     # the invalid rows' bucket


def test_alignment_table_reaches_every_loop_of_the_rank_kernel():
    """bucket starts with lo % 4 in {1, 2, 3}; counts that end inside the prologue, that reach the 4-wide loop, and that leave a
    remainder after it -- for an aligned start and for every misaligned one"""
    t = R.sort_build("alignment_table").facts["buckets"]
    assert [b.cnt for b in t] == list(R.ALIGN_COUNTS) and [b.lo for b in t] == np.concatenate([[0], np.cumsum(R.ALIGN_COUNTS)[:-1]]).tolist()
    for r in (1, 2, 3):
        mis = [b for b in t if b.lo % 4 == r]
        assert any(b.prologue == 4 - r and b.wide > 0 and b.rest > 0 for b in mis), r       # all three loops
        assert any(b.prologue == 4 - r and b.wide > 0 and b.rest == 0 for b in mis) or any(b.wide == 0 for b in mis), r
    assert any(b.lo % 4 and b.cnt < 4 - b.lo % 4 for b in t)                                # ends inside the prologue
    assert any(b.lo % 4 and b.cnt == b.prologue for b in t)
    al = [b for b in t if b.lo % 4 == 0]
    assert any(b.prologue == 0 and b.wide > 0 and b.rest > 0 for b in al) and any(b.wide == 0 and b.rest > 0 for b in al)
    assert all(b.prologue + 4 * b.wide + b.rest == b.cnt for b in t)
    s = R.alignment_scores()
    assert len(set(s.tolist())) < len(s)                                                     # equal keys: the index decides


# ---- the scan cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SCAN))
def test_scan_cases(name):
    c = R.scan_build(name)
    _holds(c, name)
    f = c.facts
    order = R.sorted_order(c.boxes5[:, 4])
    if name.startswith("staircase_"):
        assert c.expected == order[::2] and order != sorted(order)          # (permuted rows)
        assert f["chain"] == len(order) and f["picks_per_full_chunk"] == 32
    if name == "twins_rows_1_63_64":
        assert f["row_dist"] == [1, 63, 64] and f["chunk_dist"] == [0, 0, 1]
    if name == "twins_exactly_3_chunks":
        assert f["chunk_dist"] == [3, 3, 3] and min(f["row_dist"]) == 129 and max(f["row_dist"]) == 254
    if name == "twins_exactly_4_chunks":
        assert f["chunk_dist"] == [4, 4, 4] and min(f["row_dist"]) == 193 and max(f["row_dist"]) == 319
    if name == "twins_4_chunks_less_a_row":
        assert f["row_dist"] == [255, 255, 255] and f["chunk_dist"] == [4, 3, 4]
    if name == "twins_first_to_last_chunk":
        assert f["n"] == 4096 and f["chunk_dist"] == [63, 63, 63, 4] and f["windows"] == [(0, 0)] * 4
    if name == "far_twin_chunks_17_33_64":
        assert f["far_chunks"] == {0: 64, 1: 33, 2: 17}                      # every pick of the chunk has a twin >= 4 chunks on
        assert [f["chunk_picks"][k] for k in (0, 1, 2)] == [64, 33, 17]
        assert f["chunk_picks"][5] == 0 and all(f["chunk_picks"][k] > 0 for k in range(6, 12))
    if name == "nan_box_first":
        assert len(c.expected) == 1 and np.isnan(c.boxes5[c.expected[0], 0])
    if name == "nan_box_later":
        assert len(c.expected) == f["n"] - 1 and np.isnan(c.boxes5[order[300], 0]) and order[300] not in c.expected
    if name == "degenerate_boxes":
        assert f["zero_area"] > 20 and f["negative_area"] > 20 and 0 < len(c.expected) < f["n"]
    if name == "threshold_exact":
        assert c.thresh == np.float32(2.0 / 3.0) and c.expected == order
    if name == "threshold_one_ulp_below":
        assert c.thresh < np.float32(2.0 / 3.0) and np.nextafter(c.thresh, np.float32(1)) == np.float32(2.0 / 3.0)
        assert c.expected == order[::2]


def test_staircase_holds_at_the_sizes_the_windows_need():
    for n in (4097, 16386):
        b5, exp, _ = R.staircase(n, n)
        assert exp == O.nms(b5, 0.5).tolist() == R.sorted_order(b5[:, 4])[::2]


# ---- the window cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.WINDOWS))
def test_window_cases(name):
    c = R.window_build(name)
    _holds(c, name)
    f = c.facts
    n = f["n"]
    assert f["windows"] == R.windows(n, c.max_boxes)
    assert c.max_boxes is None or len(c.expected) < c.max_boxes           # the budget is not met: every window is walked
    nw = len(f["windows"])
    order = R.sorted_order(c.boxes5[:, 4])
    if name == "many_picks_before_the_border":
        assert nw == 3 and n > 4096 + 32768 and f["picks_before"][36864] > 4096
        assert f["cross_residues"][2] == list(range(16)) and f["cross_residues"][1] == list(range(16))
        return
    assert f["graded"] == (c.max_boxes == 2000 and n > 12288)
    assert nw == {4095: 1, 4096: 1, 4097: 2, 12288: 2}.get(n, 3 if f["graded"] else 2)
    for w in range(1, nw):
        r0, r1 = f["windows"][w]
        assert (0, w) in f["pair_windows"] or r1 - r0 < 8, "no pair from window 0 into window %d" % w
        # the staircase across the border: the window's first row is an odd member, suppressed by the last row before the border
        st, en = f["stairs_cross"][w - 1]
        assert st == r0 - 5 and r0 < en <= n and order[r0] not in c.expected and order[r0 - 1] in c.expected


# ---- the budget cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disjoint", "staircase"])
def test_budget_cases(kind):
    for mb in R.BUDGETS:
        c = R.budget_build(kind, mb)
        _holds(c, "%s %d" % (kind, mb))
        assert len(c.expected) == min(mb, c.facts["uncut"])
        order = R.sorted_order(c.boxes5[:, 4])
        assert c.expected == (order if kind == "disjoint" else order[::2])[:mb]
    assert R.budget_build(kind, 4096).facts["windows"] == [(0, 4096), (4096, 12288), (12288, 12400)]
    assert R.budget_build(kind, 64).facts["windows"] == [(0, 4096), (4096, 12400)]
    # a disjoint list's pick k is position k - 1: 64 / 4096 / 12288 are the last rows of a chunk / window 0 / the middle window
    assert {64, 4096, 12288} <= set(R.BUDGETS) and {63, 65, 4095, 4097} <= set(R.BUDGETS)


# ---- the device count -------------------------------------------------------------------------------------------------------------
def test_device_count_cases():
    for n_dev in R.DEV_COUNTS:
        for wv in (False, True):
            for mb in (None, 20):
                c = R.device_count_build(n_dev, wv, mb)
                live = c.facts["live"]
                assert live == max(0, min(n_dev, R.DEV_N))
                assert np.isnan(c.boxes5[live:, :4]).all() and np.isposinf(c.boxes5[live:, 4]).all()
                assert c.valid is None or (c.valid[live:] == 1).all()
                assert all(i < live for i in c.expected)
                # the same rows cut off for good give the same list: the tail is not there
                head = c.boxes5[:live]
                assert c.expected == R.reference(head, c.thresh, mb, None if c.valid is None else c.valid[:live])
                assert c.expected == R.nms_variant(c.boxes5, c.thresh, mb, c.valid, n_dev)[0]


# ---- the comparison catches wrong rules ---------------------------------------------------------------------------------------------
def _judge(case, variant, n_dev=None):
    n = len(case.boxes5)
    cap = n if case.max_boxes is None else min(n, case.max_boxes)
    picks, order = R.nms_variant(case.boxes5, case.thresh, case.max_boxes, case.valid, n_dev, variant)
    return R.first_difference(R.as_result(picks, order, n, cap), case.expected, R.sorted_order(case.boxes5[:, 4], case.valid, n_dev),
                              n, cap)


WRONG = {"higher_index_first": lambda: (R.sort_build("equal_65"), None),
         "lt_at_threshold": lambda: (R.scan_build("threshold_exact"), None),
         "nan_last": lambda: (R.sort_build("nan_first"), None),
         "neg_zero_below_zero": lambda: (R.sort_build("signed_zeros"), None),
         "rows_past_count": lambda: (R.device_count_build(R.DEV_N - 1, True, None), R.DEV_N - 1),
         "budget_off_by_one": lambda: (R.budget_build("disjoint", 64), None)}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_comparison_fails_on_a_wrong_rule(variant):
    case, n_dev = WRONG[variant]()
    assert _judge(case, None, n_dev) is None                                  # the rule itself passes
    msg = _judge(case, variant, n_dev)
    assert msg is not None, "the %s variant went unnoticed" % variant
    assert set(WRONG) == set(R.VARIANTS)


def test_the_comparison_sees_writes_past_the_count():
    c = R.budget_build("disjoint", 63)
    n = len(c.boxes5)
    order = R.sorted_order(c.boxes5[:, 4])
    good = R.as_result(c.expected, order, n, 63)
    assert R.first_difference(good, c.expected, order, n, 63) is None
    for key, at in (("picks", 63), ("picks", 64), ("count", 1), ("nvalid", 2), ("order", n)):
        bad = {k: np.array(v) for k, v in good.items()}
        bad[key][at] = 7
        assert R.first_difference(bad, c.expected, order, n, 63) is not None, (key, at)
    bad = dict(good, rc=-1)
    assert R.first_difference(bad, c.expected, order, n, 63) is not None


# ---- the hooks' header ------------------------------------------------------------------------------------------------------------
def test_hook_header_symbols_are_exported_and_off_the_boundary():
    import os
    import re
    from densecap_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))
    hooks = declared("densecap_debug_nms.h")
    assert hooks == sorted(_lib._NMS_HOOK_SIGS) == ["dc_debug_nms", "dc_debug_nms_multi"]
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    assert not [h for h in hooks if h in open(os.path.join(root, "lua", "densecap_hip.lua")).read()]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
    for other in sorted(os.listdir(os.path.join(root, "include"))):
        if other != "densecap_debug_nms.h":
            assert not set(hooks) & set(declared(other)), other
    # the argument counts of the prototypes and of the bindings agree
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "densecap_debug_nms.h")).read(), flags=re.S)
    for name in hooks:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._NMS_HOOK_SIGS[name][1]), name
