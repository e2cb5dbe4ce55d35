"""The five criteria on the GPU (loss_terms_kernel through dc_forward_losses): the `loss_*` intermediates of a call are fetched and
the terms recomputed from those float32 arrays in float64 by tests/loss_rules.py.

Bound: relative 1e-12 on each double.  Every term is a sum of at most 4096 non-negative summands (condition number 1): naive
summation's worst case n*u is 4.5e-13 for u = 1.1e-16, and the device's double log / exp are within an ulp or two of numpy's per
summand.  The rows' caption log-likelihoods, cast to float32, must equal the diagonal of dc_op_lm_score on the same codes and
captions bit for bit."""
import numpy as np
import pytest

from tests import loss_rules as R

pytestmark = pytest.mark.gpu
REL = 1e-12
V, T = 200, 15


@pytest.fixture(scope="module")
def small():
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=21, vocab_size=V, seq_length=T)
    m = DenseCapModel(W, device=0)
    yield m, W
    m.ctx.close()


def _labels(G, L, rng):
    """caption lengths 0, 1, L-1, L first, then random ones"""
    lab = np.zeros((G, L), np.int32)
    for j in range(G):
        n = [0, 1, L - 1, L][j] if j < 4 else int(rng.integers(0, L + 1))
        lab[j, :n] = rng.integers(1, V + 1, n)
    return lab


def _fetch(m, A, n, num_pos):
    f = lambda name, shape, dt=np.float32: m.debug_fetch(name, shape, dt)[0]
    return dict(boxes=f("loss_rpn_boxes", (A, 4)), anchors=f("loss_rpn_anchors", (A, 4)), trans=f("loss_rpn_trans", (A, 4)),
                scores=f("loss_rpn_scores", (A, 2)), obj=f("loss_obj", (n,)), final_trans=f("loss_final_trans", (n, 4)),
                roi_boxes=f("loss_roi_boxes", (n, 4)), codes=f("loss_codes", (n, m.fc_dim)),
                rowlik=f("loss_rowlik", (num_pos,), np.float64))


def _check(m, img, gt, lab, what, **kw):
    from densecap_amd import ops
    H, Wd = img.shape[1:]
    A = m.num_anchors * ((H + 15) // 16) * ((Wd + 15) // 16)
    r = m.forward_losses(img, gt, lab, dump=True, **kw)
    npos, nneg = r["num_pos"], r["num_neg"]
    d = _fetch(m, A, npos + nneg, npos)
    pi, pt, ni = r["pos_input_idx"], r["pos_target_idx"], r["neg_input_idx"]
    assert np.array_equal(d["roi_boxes"], d["boxes"][np.concatenate([pi, ni])]), what
    opts = {k: v for k, v in kw.items() if k in R.DEFAULTS}
    ref = R.losses(d["scores"][pi], d["scores"][ni], d["anchors"][pi], d["trans"][pi], gt[pt], d["obj"], d["boxes"][pi],
                   d["final_trans"][:npos], d["rowlik"], lab.shape[1], opts)
    for k in R.LOSS_KEYS:
        err = abs(r[k] - ref[k]) / max(abs(ref[k]), 1e-300)
        print("%s %s: device %.17g rules %.17g rel %.3g" % (what, k, r[k], ref[k], err))
        assert np.isfinite(r[k]) and r[k] >= 0
        assert err <= REL, (what, k, r[k], ref[k])
    assert (r["masked_mid"], r["masked_end"]) == (ref["masked_mid"], ref["masked_end"]), what
    if npos:
        ll = ops.lm_score(m.ctx, d["codes"][:npos], lab[pt])
        assert np.array_equal(d["rowlik"].astype(np.float32).view(np.uint32), np.diagonal(ll).copy().view(np.uint32)), what
    return r, d


def _gt_in_image(rng, G, H, Wd):
    return np.stack([rng.uniform(15, Wd - 15, G), rng.uniform(15, H - 15, G), rng.uniform(12, Wd / 2, G), rng.uniform(12, H / 2, G)], 1).astype(np.float32)


@pytest.mark.parametrize("size", [(64, 96), (224, 320)], ids=["96x64", "320x224"])
def test_terms_from_the_fetched_intermediates(small, size):
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    H, Wd = size
    img = make_synthetic_image(H, Wd, 3)
    rng = np.random.default_rng(H)
    gt, lab = _gt_in_image(rng, 6, H, Wd), _labels(6, T, rng)
    # default settings: a handful of positives (every ground-truth box's best input), num_pos < batch / 2
    r, d = _check(m, img, gt, lab, "default")
    assert 0 < r["num_pos"] < 128 and r["num_pos"] + r["num_neg"] == min(256, r["num_pos"] + 256 - r["num_pos"])
    # forced lists (ranks in the candidate lists of the rules on the fetched boxes), repeats included
    s = R.box_sampler(d["boxes"], gt, bounds=(1, 1, Wd, H))
    fp = [s["total_pos"] - 1, 0, 1, 1]
    fn = list(range(0, min(s["total_neg"], 40), 3)) + [s["total_neg"] - 1]
    r2, _ = _check(m, img, gt, lab, "forced", forced_pos=fp, forced_neg=fn, batch_size=64)
    want = R.box_sampler(d["boxes"], gt, 64, bounds=(1, 1, Wd, H), forced_pos=fp, forced_neg=fn)
    for k in ("pos_input_idx", "pos_target_idx", "neg_input_idx"):
        assert np.array_equal(r2[k], want[k]), k
    # other weights, a narrow label matrix (L = 4: every caption is cut by the caller), a small batch
    _check(m, img, gt, lab[:, :4], "weights", batch_size=32, mid_box_reg_weight=1.0, mid_objectness_weight=2.0, end_box_reg_weight=0.5,
           end_objectness_weight=3.0, captioning_weight=0.25, seed=9)


def test_masked_rows_stay_in_the_denominator(small):
    """A ground-truth box 1e5 times as wide as any anchor: every positive row matched to it has a width target above 10, is zeroed
    and still counted.  Thresholds 0 / 0 make every input that overlaps anything positive and leave no negatives."""
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    H, Wd = 224, 320
    img = make_synthetic_image(H, Wd, 4)
    rng = np.random.default_rng(5)
    gt = _gt_in_image(rng, 5, H, Wd)
    gt[4] = [Wd / 2, H / 2, 724e5, 60]
    lab = _labels(5, T, rng)
    r, d = _check(m, img, gt, lab, "masked", high_thresh=0.0, low_thresh=0.0, batch_size=64, seed=2)
    assert r["masked_mid"] >= 1 and r["masked_end"] >= 1 and r["flags"] & R.FLAG_NO_NEGATIVES
    assert r["num_pos"] == 32 and (r["pos_target_idx"] == 4).sum() == r["masked_mid"]
    # the rows count: without them in the denominator the term would be larger
    pi, pt = r["pos_input_idx"], r["pos_target_idx"]
    rows, mask = R.box_reg_rows(d["anchors"][pi], d["trans"][pi], gt[pt])
    if mask.sum() < len(mask):
        assert r["mid_box_reg_loss"] < np.float32(0.05) * rows.sum() / (4.0 * (len(mask) - mask.sum()))
