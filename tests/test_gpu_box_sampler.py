"""nn.BoxSampler on the GPU (dc_op_box_sampler) against tests/loss_rules.py: every index list, count, flag, max_iou and arg is
compared for exact equality (integers as integers, float32 bit for bit)."""
import ctypes as C

import numpy as np
import pytest

from tests import loss_rules as R

pytestmark = pytest.mark.gpu
IMG = (600, 720)


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check(ctx, boxes, gt, img=IMG, what="", forced_pos=None, forced_neg=None, **opts):
    from densecap_amd import ops
    H, W = img
    o = dict(R.DEFAULTS, **opts)
    got = ops.box_sampler(ctx, boxes, gt, H, W, forced_pos=forced_pos, forced_neg=forced_neg, **opts)
    ref = R.box_sampler(boxes, gt, o["batch_size"], o["high_thresh"], o["low_thresh"], (1, 1, W, H) if o["remove_outbounds"] else None,
                        o["seed"], forced_pos, forced_neg)
    nan = np.isnan(ref["max_iou"])
    assert np.array_equal(np.isnan(got["max_iou"]), nan), what
    assert _same_bits(np.where(nan, 0, got["max_iou"]), np.where(nan, 0, ref["max_iou"])), what
    assert np.array_equal(got["arg"], ref["arg"]), what
    for k in ("num_pos", "num_neg", "total_pos", "total_neg", "flags"):
        assert got[k] == ref[k], "%s: %s %d != %d" % (what, k, got[k], ref[k])
    for k in ("pos_input_idx", "pos_target_idx", "neg_input_idx"):
        assert np.array_equal(got[k], ref[k]), "%s: %s" % (what, k)
    return got


@pytest.mark.parametrize("A", [1, 63, 64, 65, 255, 256, 257, 3360, 20520])
def test_input_counts(ctx, A):
    for G, batch in ((1, 2), (65, 256), (512, 1024)):
        boxes, gt = R.make_case(1000 + A + G, A, G, IMG)
        for rb in (1, 0):
            _check(ctx, boxes, gt, what="A=%d G=%d batch=%d bounds=%d" % (A, G, batch, rb), batch_size=batch, remove_outbounds=rb, seed=A)


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 512])
def test_ground_truth_counts(ctx, G):
    for A, batch, hits in ((257, 64, 0.5), (3360, 256, 0.05)):
        boxes, gt = R.make_case(2000 + G, A, G, IMG, hits=hits)
        _check(ctx, boxes, gt, what="G=%d A=%d" % (G, A), batch_size=batch, seed=G)


@pytest.mark.parametrize("batch", [2, 64, 256, 1024])
def test_batch_sizes_and_rank_order(ctx, batch):
    """A draw depends on the batch size through its rank in key order alone: a smaller batch's lists are prefixes."""
    boxes, gt = R.make_case(77, 3360, 64, IMG, hits=0.6)
    got = _check(ctx, boxes, gt, what="batch=%d" % batch, batch_size=batch, seed=5)
    big = _check(ctx, boxes, gt, what="batch=1024", batch_size=1024, seed=5)
    assert got["num_pos"] == batch // 2 and got["flags"] == 0
    assert np.array_equal(got["pos_input_idx"], big["pos_input_idx"][:batch // 2])
    assert np.array_equal(got["neg_input_idx"], big["neg_input_idx"][:got["num_neg"]])


def test_every_branch(ctx):
    for name, (boxes, gt, img, opts) in R.branch_cases().items():
        for rb in (1, 0):
            _check(ctx, boxes, gt, img, what=name, remove_outbounds=rb, **opts)


def test_nan_and_inf_rows(ctx):
    boxes, gt = R.make_case(9, 300, 6, IMG)
    boxes[3] = np.nan                                   # every IoU NaN: neither positive nor negative, nobody's best
    boxes[7] = [np.inf, 100, 50, 50]
    boxes[8] = [100, 100, np.inf, 50]
    boxes[9] = [-np.inf, -np.inf, 20, 20]
    got = _check(ctx, boxes, gt, what="nan/inf", batch_size=64)
    assert np.isnan(got["max_iou"][3]) and 3 not in got["pos_input_idx"] and 3 not in got["neg_input_idx"]
    allnan = np.full((5, 4), np.nan, np.float32)
    got = _check(ctx, allnan, gt, what="all NaN", batch_size=8)
    assert got["total_pos"] == 0 and got["num_pos"] == 0 and got["flags"] & R.FLAG_NO_NEGATIVES


def test_seeds(ctx):
    boxes, gt = R.make_case(11, 3360, 20, IMG, hits=0.5)
    a = _check(ctx, boxes, gt, what="seed 1", seed=1)
    b = _check(ctx, boxes, gt, what="seed 1 again", seed=1)
    c = _check(ctx, boxes, gt, what="seed 2^40+3", seed=(1 << 40) + 3)
    for k in ("pos_input_idx", "pos_target_idx", "neg_input_idx"):
        assert np.array_equal(a[k], b[k])
    assert not np.array_equal(a["pos_input_idx"], c["pos_input_idx"]) and not np.array_equal(a["neg_input_idx"], c["neg_input_idx"])


def test_forced_indices_pass_through(ctx):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    boxes, gt = R.make_case(12, 700, 9, IMG, hits=0.5)
    free = R.box_sampler(boxes, gt, 64, bounds=(1, 1, IMG[1], IMG[0]))
    fp = [free["total_pos"] - 1, 0, 3, 3]
    fn = [5, free["total_neg"] - 1, 0]
    got = _check(ctx, boxes, gt, what="forced", forced_pos=fp, forced_neg=fn, batch_size=64)
    assert got["num_pos"] == 4 and got["num_neg"] == 3
    _check(ctx, boxes, gt, what="forced positives only", forced_pos=fp, batch_size=64)
    _check(ctx, boxes, gt, what="forced, empty", forced_pos=[], forced_neg=[2], batch_size=64)
    with pytest.raises(DenseCapError, match="outside the candidate lists"):
        ops.box_sampler(ctx, boxes, gt, IMG[0], IMG[1], forced_pos=[free["total_pos"]], batch_size=64)
    with pytest.raises(DenseCapError, match="outside the candidate lists"):
        ops.box_sampler(ctx, boxes, gt, IMG[0], IMG[1], forced_neg=[-1], batch_size=64)


def test_philox_restatement_is_the_device_function(ctx):
    """The pure-Python Philox4x32-10 of tests/loss_rules.py against the library's ("sample_bits@seed": word v & 3 of the counter
    (v >> 2, t, r, s)); candidate i of class c is the coordinate (s, r, t, v) = (0, c, 0, 4 i)."""
    rng = np.random.default_rng(3)
    for seed in (0, 7, (0x299f31d0 << 32) | 0xa4093822, 2 ** 64 - 1):
        i = rng.integers(0, 1 << 28, 200)
        cls = rng.integers(0, 2, 200)
        co = np.stack([np.zeros(200), cls, np.zeros(200), 4 * i], 1).astype(np.int32)
        buf = co.copy()
        assert ctx.lib.dc_debug_fetch(ctx.h, b"sample_bits@%d" % seed, buf.ctypes.data, buf.nbytes) == 200
        got = buf.reshape(-1).view(np.uint32)[:200]
        want = [R.philox4x32_10(int(a), 0, int(c), 0, seed & 0xffffffff, seed >> 32)[0] for a, c in zip(i, cls)]
        assert np.array_equal(got, np.array(want, np.uint32))
        for c in (0, 1):
            assert np.array_equal(R.sample_key(i[cls == c], c, seed), got[cls == c])


def test_refusals_launch_nothing(ctx):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    boxes, gt = R.make_case(13, 100, 4, IMG)
    sentinel = np.full(64, -7, np.int32)
    bad = [dict(batch_size=0), dict(batch_size=3), dict(batch_size=1026), dict(high_thresh=float("nan")), dict(low_thresh=-0.1),
           dict(high_thresh=1.5), dict(low_thresh=0.8, high_thresh=0.7), dict(remove_outbounds=2)]
    for opts in bad:
        with pytest.raises(DenseCapError, match=r"\(-1\)"):
            ops.box_sampler(ctx, boxes, gt, IMG[0], IMG[1], **opts)
    # through the C ABI with sentinel-filled outputs: a refused call writes nothing
    bd, gd = ctx.to_device(boxes), ctx.to_device(gt)
    outs = [ctx.to_device(sentinel) for _ in range(4)]
    o = ops.loss_opts(batch_size=64)

    def call(A, G, opts=o):
        return ctx.lib.dc_op_box_sampler(ctx.h, bd.ptr, gd.ptr, A, G, IMG[0], IMG[1], C.byref(opts), None, outs[0].ptr, outs[1].ptr,
                                         outs[2].ptr, outs[3].ptr, None, None)
    assert call(100, 0) == -5 and call(100, 513) == -5 and call(0, 4) == -1
    assert call(100, 4, ops.loss_opts(batch_size=6, low_thresh=0.9)) == -1
    for a in outs:
        assert np.array_equal(a.numpy(), sentinel)
    assert call(100, 4) == 0
    assert not np.array_equal(outs[3].numpy()[:5], sentinel[:5])
