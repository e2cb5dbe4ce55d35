"""The evaluator's matching on the GPU (dc_op_eval_match): every comparison is exact equality -- integers as integers, float64
bit for bit -- with the reference of tests/eval_rules.py (its `fast` form, which tests/test_eval_rules_cpu.py ties to the
literal loops)."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_rules as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _check(ctx, dets, scores, gts, thr=0.7, what=""):
    """Both claim modes; returns the claim-last results."""
    from densecap_amd import ops
    out = None
    for claim_last in (True, False):
        got = ops.eval_match(ctx, dets, scores, gts, thr, claim_last)
        assert len(got) == len(dets)
        for i, g in enumerate(got):
            ref = R.match_image(dets[i], scores[i], gts[i], thr, claim_last, fast=True)
            diff = R.first_difference(g, ref)
            assert diff is None, "%s, image %d, claim_last=%s: %s" % (what, i, claim_last, diff)
            assert not g["merged_tail"].any(), "%s: merged rows past n_groups must be zero" % what
            assert sorted(g["order"].tolist()) == list(range(len(dets[i])))
        out = out or got
    return out


def _image(rng, B, M, per, far=0.2):
    gt = R.clustered_gt(rng, M, per) if M else np.zeros((0, 4), np.float32)
    return R.detections_for(rng, gt, B, far), R.special_scores(rng, B), gt


@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 130, 1000, 4096])
def test_detection_counts(ctx, B):
    rng = np.random.default_rng(B)
    for M, per in ((50, 4), (40, 40), (7, 1)):
        d, s, g = _image(rng, B, M, per)
        _check(ctx, [d], [s], [g], what="B=%d M=%d clusters of %d" % (B, M, per))


@pytest.mark.parametrize("M", [0, 1, 2, 63, 64, 65, 200, R.MAX_GT])
def test_ground_truth_counts(ctx, M):
    rng = np.random.default_rng(1000 + M)
    for per in (1, 4, 40):
        d, s, g = _image(rng, 130, M, per)
        got = _check(ctx, [d], [s], [g], what="M=%d clusters of %d" % (M, per))[0]
        assert got["n_groups"] <= M and (M == 0 or got["n_groups"] >= 1)
        if per == 40 and M >= 40:
            assert got["n_groups"] < M                                   # the clusters do merge


@pytest.mark.parametrize("n_images", [1, 3, 17])
def test_groups_of_images_and_independence(ctx, n_images):
    """Every image different, empty ones mixed in; an image's result is what it is alone, and in another company."""
    from densecap_amd import ops
    rng = np.random.default_rng(n_images)
    shapes = [(130, 50, 4), (0, 12, 4), (65, 0, 1), (300, 80, 40), (0, 0, 1), (64, 64, 1), (1, 1, 1)]
    imgs = [_image(rng, *shapes[i % len(shapes)]) for i in range(n_images)]
    d, s, g = ([im[k] for im in imgs] for k in range(3))
    got = _check(ctx, d, s, g, what="n_images=%d" % n_images)
    for i in range(0, n_images, 4):
        alone = ops.eval_match(ctx, [d[i]], [s[i]], [g[i]])[0]
        assert R.first_difference(alone, got[i]) is None, i
    if n_images > 1:
        perm = rng.permutation(n_images)
        other = ops.eval_match(ctx, [d[i] for i in perm], [s[i] for i in perm], [g[i] for i in perm])
        for k, i in enumerate(perm):
            assert R.first_difference(other[k], got[i]) is None, (k, i)


def test_ious_exactly_on_the_threshold(ctx):
    """10x10 boxes with the 10x7 box nested in them: IoU exactly 70/100, >= 0.7, every pair merges."""
    rng = np.random.default_rng(5)
    for M in (2, 64, 200):
        g = R.on_threshold_gt(M)
        d = R.detections_for(rng, g, 130)
        got = _check(ctx, [d], [R.special_scores(rng, 130)], [g], what="on threshold, M=%d" % M)[0]
        assert got["n_groups"] == M // 2
        assert got["gt_group"].tolist() == [j // 2 for j in range(M)]


def test_detections_that_overlap_nothing(ctx):
    """Two far-apart ground-truth boxes; the best detection overlaps nothing, the next matches the LAST group exactly: under the
    reference rule the first has taken that group (ok 1 at ov 0) and the true match is refused; without it the match stands."""
    from densecap_amd import ops
    gt = R.to_xcycwh([[0, 0, 9, 9], [100, 100, 119, 119]])
    det = R.to_xcycwh([[100, 100, 119, 119], [500, 500, 520, 520], [0, 0, 9, 9], [600, 600, 610, 610]])
    sc = np.asarray([0.5, 0.9, 0.4, 0.1], np.float32)
    last, none = (ops.eval_match(ctx, [det], [sc], [gt], 0.7, cl)[0] for cl in (True, False))
    assert last["order"].tolist() == none["order"].tolist() == [1, 0, 2, 3]
    assert last["group"].tolist() == none["group"].tolist() == [-1, 1, 0, -1]
    assert last["ov"].tolist() == none["ov"].tolist() == [0.0, 1.0, 1.0, 0.0]
    assert last["ok"].tolist() == [1, 0, 1, 0] and none["ok"].tolist() == [0, 1, 1, 0]
    _check(ctx, [det], [sc], [gt], what="overlaps nothing")
    # nothing to claim at all: M = 0
    for r in ops.eval_match(ctx, [det], [sc], [np.zeros((0, 4), np.float32)]):
        assert r["n_groups"] == 0 and not r["ok"].any() and (r["group"] == -1).all() and not r["ov"].any()
    rng = np.random.default_rng(9)
    d, s, g = _image(rng, 300, 60, 4, far=0.6)
    _check(ctx, [d], [s], [g], what="many far detections")


def test_special_scores(ctx):
    rng = np.random.default_rng(11)
    d, _, g = _image(rng, 200, 50, 4)
    s = np.zeros((200,), np.float32)
    s[::2] = -0.0                                                          # -0 == +0: index order
    got = _check(ctx, [d], [s], [g], what="signed zeros")[0]
    assert got["order"].tolist() == list(range(200))
    s = rng.uniform(0, 1, 200).astype(np.float32)
    s[[3, 50, 199]] = np.nan; s[[4, 60]] = np.inf; s[[5, 70]] = -np.inf
    got = _check(ctx, [d], [s], [g], what="nan / inf")[0]
    assert got["order"].tolist()[:2] == [4, 60] and got["order"].tolist()[-5:] == [5, 70, 3, 50, 199]
    _check(ctx, [d], [np.full((200,), np.nan, np.float32)], [g], what="all NaN")


def test_non_finite_and_zero_size_boxes(ctx):
    rng = np.random.default_rng(13)
    for per in (4, 40):
        d, s, g = _image(rng, 300, 120, per)
        d, g = d.copy(), g.copy()
        for k, row in enumerate(rng.choice(300, 12, replace=False)):
            d[row, k % 4] = (np.nan, np.inf, -np.inf)[k % 3]
        for k, row in enumerate(rng.choice(120, 9, replace=False)):
            g[row, k % 4] = (np.nan, np.inf, -np.inf)[k % 3]
        d[rng.choice(300, 10, replace=False), 2:] = 0.0                      # w = h = 0: corners cross, extent 0 after the +1
        g[rng.choice(120, 6, replace=False), 2:] = 0.0
        d[rng.choice(300, 5, replace=False), 2] = -30.0                      # negative width
        _check(ctx, [d], [s], [g], what="non-finite, clusters of %d" % per)


def test_other_thresholds(ctx):
    rng = np.random.default_rng(17)
    d, s, g = _image(rng, 130, 80, 40)
    for thr in (0.3, 0.5, 1.0, 1e-6):
        _check(ctx, [d], [s], [g], thr, what="thr=%g" % thr)


def test_refusals_enqueue_nothing_and_leave_the_ctx_usable(ctx):
    from densecap_amd import ops
    rng = np.random.default_rng(19)
    DC_E_INVALID, DC_E_UNSUPPORTED = -1, -5
    nb, ng = 4097, R.MAX_GT + 1
    db = ctx.to_device(np.zeros((nb, 4), np.float32)); ds = ctx.to_device(np.zeros((nb,), np.float32))
    gb = ctx.to_device(np.zeros((ng, 4), np.float32))
    sentinel = lambda shape, dt, v: ctx.to_device(np.full(shape, v, dt))
    outs = dict(order=sentinel((nb,), np.int32, -7), ov=sentinel((nb,), np.float64, -7.0), group=sentinel((nb,), np.int32, -7),
                ok=sentinel((nb,), np.uint8, 77), gt_group=sentinel((ng,), np.int32, -7), n_groups=sentinel((4,), np.int32, -7),
                merged=sentinel((ng, 4), np.float64, -7.0))
    before = {k: v.numpy() for k, v in outs.items()}

    def call(doff, goff, n=None, thr=0.7, flags=1, null=None):
        do = ctx.to_device(np.asarray(doff, np.int32)); go = ctx.to_device(np.asarray(goff, np.int32))
        p = dict(db=db.ptr, ds=ds.ptr, do=do.ptr, gb=gb.ptr, go=go.ptr, **{k: v.ptr for k, v in outs.items()})
        if null:
            p[null] = None
        return ctx.lib.dc_op_eval_match(ctx.h, p["db"], p["ds"], p["do"], p["gb"], p["go"], len(doff) - 1 if n is None else n,
                                        C.c_float(thr), flags, p["order"], p["ov"], p["group"], p["ok"], p["gt_group"],
                                        p["n_groups"], p["merged"])
    assert call([0, 4097], [0, 10]) == DC_E_UNSUPPORTED and b"4096" in ctx.lib.dc_last_error(ctx.h)
    assert call([0, 10], [0, ng]) == DC_E_UNSUPPORTED and str(R.MAX_GT).encode() in ctx.lib.dc_last_error(ctx.h)
    assert call([0, 5, 4102], [0, 1, 2]) == DC_E_UNSUPPORTED                 # a later image
    for thr in (float("nan"), 0.0, -0.5, 1.5, float("inf")):
        assert call([0, 10], [0, 10], thr=thr) == DC_E_INVALID, thr
    for flags in (2, 3, -1, 1 << 20):
        assert call([0, 10], [0, 10], flags=flags) == DC_E_INVALID, flags
    assert call([0, 10, 5], [0, 3, 6]) == DC_E_INVALID and call([0, 10, 20], [0, 6, 3]) == DC_E_INVALID
    assert call([-1, 10], [0, 3]) == DC_E_INVALID and call([0, 10], [-2, 3]) == DC_E_INVALID
    assert call([0, 10], [0, 3], n=0) == DC_E_INVALID and call([0, 10], [0, 3], n=-1) == DC_E_INVALID
    for null in ("db", "ds", "do", "gb", "go", "order", "ov", "group", "ok", "gt_group", "n_groups", "merged"):
        assert call([0, 10], [0, 3], null=null) == DC_E_INVALID, null
    for k, v in outs.items():                                                # nothing was launched: the outputs are untouched
        assert np.array_equal(v.numpy(), before[k]), k
    with pytest.raises(Exception, match="dc_op_eval_match"):
        ops.eval_match(ctx, [np.zeros((4097, 4), np.float32)], [np.zeros((4097,), np.float32)], [np.zeros((1, 4), np.float32)])
    assert call([0, 4096], [0, R.MAX_GT]) == 0                              # the largest call, on the buffers of the refused ones
    assert outs["n_groups"].numpy()[0] == R.MAX_GT                           # (w = h = 0: no box overlaps another)
    d, s, g = _image(rng, 130, 50, 4)
    _check(ctx, [d], [s], [g], what="after the refusals")
