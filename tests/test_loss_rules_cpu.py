"""tests/loss_rules.py tied to the reference: the known answers of test/BoxSampler_test.lua and test/LanguageModel_test.lua
(tests/golden/loss_vectors.json, transcribed by hand), the InvertBoxTransform / ApplyBoxTransform round trip, the rules' teeth,
and the branch coverage of the fixtures the GPU tests run.

Which reference tests are STALE: simpleTest, anotherTest, boundsTest and noNegativesTest were written for nn.BoxIoU's original
converter (corners xc -/+ w/2, BoxIoU.lua:15-37, commented out there).  Their masks hold under convention="legacy_half_w" and no
longer under the live (w-1)/2 converter (simpleTest's positives are 0100001001 against the 0100001101 the
test expects).  Both are pinned here: the vectors under the legacy convention, the live code's masks under the module
convention.  negativeReplacementTest checks counts only and holds under either."""
import json
import os

import numpy as np

from tests import loss_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "loss_vectors.json")) as f:
    V = json.load(f)


def _run(case, convention, **kw):
    c = V[case]
    b = c.get("bounds")
    bounds = (b["x_min"], b["y_min"], b["x_max"], b["y_max"]) if b else None
    fp = [i - 1 for i in c["debug_pos_sample_idx"]] if "debug_pos_sample_idx" in c else None
    fn = [i - 1 for i in c["debug_neg_sample_idx"]] if "debug_neg_sample_idx" in c else None
    return R.box_sampler(c["input_boxes"], c["target_boxes"], c.get("batch_size", 256), c["high_thresh"], c["low_thresh"], bounds,
                         forced_pos=fp, forced_neg=fn, convention=convention, **kw)


def _masks(r):
    return r["pos_mask"].astype(int).tolist(), r["neg_mask"].astype(int).tolist()


def test_simple_test_vectors():
    c = V["simpleTest"]
    r = _run("simpleTest", "legacy_half_w")
    assert _masks(r) == (c["expected_pos_mask"], c["expected_neg_mask"])
    assert (r["pos_input_idx"] + 1).tolist() == c["expected_pos_input_idx"]
    assert (r["pos_target_idx"] + 1).tolist() == c["expected_pos_target_idx"]
    assert (r["neg_input_idx"] + 1).tolist() == c["expected_neg_input_idx"]
    live = _run("simpleTest", "boxiou_module")               # stale under the live converter
    assert _masks(live) == (c["live_pos_mask"], c["live_neg_mask"]) and c["live_pos_mask"] != c["expected_pos_mask"]


def test_another_test_vectors():
    c = V["anotherTest"]
    r = _run("anotherTest", "legacy_half_w")
    assert _masks(r) == (c["expected_pos_mask"], c["expected_neg_mask"])
    assert r["max_iou"][1] == np.float32(c["expected_iou_2_1"])
    assert (r["pos_input_idx"] + 1).tolist() == c["expected_pos_input_idx"] and (r["pos_target_idx"] + 1).tolist() == c["expected_pos_target_idx"]
    assert sorted((r["neg_input_idx"] + 1).tolist()) == c["expected_neg_input_idx_sorted"]        # all three, whatever the draw
    assert r["flags"] == 0 and r["num_pos"] + r["num_neg"] == c["batch_size"]
    # live converter: every IoU is zero, and the all-zero column forces input 1 positive (TH's strict > scan keeps the first)
    live = _run("anotherTest", "boxiou_module")
    assert not live["max_iou"].any() and _masks(live) == (c["live_pos_mask"], c["live_neg_mask"])


def test_bounds_test_vectors():
    c = V["boundsTest"]
    r = _run("boundsTest", "legacy_half_w")
    assert _masks(r) == (c["expected_pos_mask"], c["expected_neg_mask"])
    assert r["pos_mask"][1] and R.corners(np.asarray(c["input_boxes"], np.float32))[1, 0] < c["bounds"]["x_min"]    # out of bounds, still positive
    assert _masks(_run("boundsTest", "boxiou_module")) == (c["live_pos_mask"], c["live_neg_mask"])


def test_negative_replacement_test():
    c = V["negativeReplacementTest"]
    for seed in range(5):
        rng = np.random.default_rng(seed)
        b, g = rng.standard_normal((c["B1"], 4)), rng.standard_normal((c["B2"], 4))
        for conv in ("legacy_half_w", "boxiou_module"):
            r = R.box_sampler(b, g, c["batch_size"], c["high_thresh"], c["low_thresh"], seed=seed, convention=conv)
            assert len(r["pos_input_idx"]) == len(r["pos_target_idx"])
            assert len(r["pos_input_idx"]) + len(r["neg_input_idx"]) == c["batch_size"]
            assert r["flags"] & R.FLAG_NEG_REPLACEMENT and r["total_neg"] < r["num_neg"]
            assert set(r["neg_input_idx"].tolist()) <= set(np.nonzero(r["neg_mask"])[0].tolist())


def test_no_negatives_test_vectors():
    c = V["noNegativesTest"]
    r = _run("noNegativesTest", "legacy_half_w")
    assert _masks(r) == (c["expected_pos_mask"], c["expected_neg_mask"])
    assert bool(r["flags"] & R.FLAG_NO_NEGATIVES) == c["expected_no_negatives"]
    live = _run("noNegativesTest", "boxiou_module")
    assert _masks(live) == (c["live_pos_mask"], c["live_neg_mask"]) and bool(live["flags"] & R.FLAG_NO_NEGATIVES) == c["live_no_negatives"]


def test_invert_apply_round_trip():
    """InvertBoxTransform_test.lua:15-58: Apply(anchors, Invert(anchors, targets)) == targets."""
    rng = np.random.default_rng(0)
    a = np.stack([rng.uniform(-50, 700, 200), rng.uniform(-50, 700, 200), rng.uniform(1, 400, 200), rng.uniform(1, 400, 200)], 1).astype(np.float32)
    t = np.stack([rng.uniform(-50, 700, 200), rng.uniform(-50, 700, 200), rng.uniform(1, 400, 200), rng.uniform(1, 400, 200)], 1).astype(np.float32)
    back = R.apply_box_transform(a, R.invert_box_transform(a, t))
    assert np.abs(back - t).max() <= 1e-9 * 1000
    tr = rng.standard_normal((200, 4))
    again = R.invert_box_transform(a, R.apply_box_transform(a, tr).astype(np.float32))
    assert np.abs(again - tr).max() < 1e-4                                      # (the boxes went through float32)


def test_get_target():
    c = V["getTargetTest"]
    assert R.get_target(c["gt_sequence"], c["vocab_size"]).tolist() == c["expected_target"]


def test_philox_forms_agree_and_known_answer():
    # Random123's known-answer vectors for philox4x32_10
    assert R.philox4x32_10(0, 0, 0, 0, 0, 0) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert R.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    i = np.arange(0, 3000, 7)
    for seed in (0, 5, (1 << 40) + 3, 2 ** 64 - 1):
        for cls in (0, 1):
            want = [R.philox4x32_10(int(v), 0, cls, 0, seed & 0xffffffff, seed >> 32)[0] for v in i]
            assert R.sample_key(i, cls, seed).tolist() == want


def _teeth_case():
    return R.make_case(21, 400, 8, (600, 720), hits=0.4)


def test_the_rules_have_teeth():
    b, g = _teeth_case()
    bounds = (1, 1, 720, 600)
    base = R.box_sampler(b, g, 64, bounds=bounds)
    flipped = R.box_sampler(b, g, 64, bounds=bounds, tie="higher")                # duplicates and the zero column tie
    assert not np.array_equal(base["pos_mask"], flipped["pos_mask"]) or not np.array_equal(base["arg"], flipped["arg"])
    assert base["pos_mask"][0] and not flipped["pos_mask"][0]                     # the all-zero column forces input 0, or the last
    no_scatter = R.box_sampler(b, g, 64, bounds=bounds, scatter=False)
    assert not np.array_equal(base["pos_mask"], no_scatter["pos_mask"])
    no_bounds = R.box_sampler(b, g, 64, bounds=None)
    assert not np.array_equal(base["neg_mask"], no_bounds["neg_mask"])
    # the masked-row denominator: one target 1e5 times as wide as its anchor
    rng = np.random.default_rng(1)
    anchors = np.stack([rng.uniform(50, 600, 6), rng.uniform(50, 500, 6), rng.uniform(20, 200, 6), rng.uniform(20, 200, 6)], 1).astype(np.float32)
    targets = (anchors * (1 + 0.1 * rng.uniform(-1, 1, (6, 4)))).astype(np.float32)
    targets[2, 2] = anchors[2, 2] * 1e5
    pred = (0.1 * rng.standard_normal((6, 4))).astype(np.float32)
    args = (rng.standard_normal((6, 2)), rng.standard_normal((10, 2)), anchors, pred, targets, rng.standard_normal(16), anchors, pred,
            -rng.uniform(1, 20, 6), 15)
    full = R.losses(*args)
    assert full["masked_mid"] == 1 and full["masked_end"] == 1
    assert R.losses(*args, masked_in_denominator=False)["mid_box_reg_loss"] > full["mid_box_reg_loss"]
    assert R.losses(*args, mask_rows=False)["mid_box_reg_loss"] > 10 * full["mid_box_reg_loss"]
    assert abs(full["total_loss"] - sum(full[k] for k in R.LOSS_KEYS[:5])) < 1e-12


def test_gpu_fixtures_reach_every_branch():
    cases = R.branch_cases()
    seen = {}
    for name, (b, g, img, o) in cases.items():
        seen[name] = R.box_sampler(b, g, o.get("batch_size", 256), o.get("high_thresh", 0.7), o.get("low_thresh", 0.3), (1, 1, img[1], img[0]))
    bs = lambda n: cases[n][3]["batch_size"]
    assert seen["many_positives"]["total_pos"] > bs("many_positives") // 2 and seen["many_positives"]["flags"] == 0
    assert 0 < seen["few_positives"]["total_pos"] < bs("few_positives") // 2
    assert seen["neg_replacement"]["flags"] == R.FLAG_NEG_REPLACEMENT and seen["neg_replacement"]["total_neg"] < seen["neg_replacement"]["num_neg"]
    assert seen["no_negatives"]["flags"] & R.FLAG_NO_NEGATIVES and seen["no_negatives"]["total_neg"] > 0
    assert seen["single_input"]["total_neg"] == 0 and seen["single_input"]["num_neg"] == 0
    # make_case: an all-zero IoU column (it forces input 0), duplicate ground truth and duplicate inputs, boxes that leave the image
    b, g, img, _ = cases["many_positives"]
    from oracle import densecap_oracle as O
    iou = O.box_iou(b, g)
    assert not iou[:, -1].any() and seen["many_positives"]["target_idx"][-1] == 0 and seen["many_positives"]["pos_mask"][0]
    assert np.array_equal(g[0], g[1]) and np.array_equal(b[0], b[1])
    c = R.corners(b)
    assert ((c[:, 0] < 1) | (c[:, 1] < 1) | (c[:, 2] > img[1]) | (c[:, 3] > img[0])).any()
    # the shapes of tests/test_gpu_box_sampler.py: A = 1 and A < batch / 2 reach the small branches, the large ones both sides
    r = R.box_sampler(*R.make_case(1000 + 20520 + 512, 20520, 512), 1024, bounds=(1, 1, 720, 600))
    assert r["total_pos"] > 512 and r["total_neg"] > 512
