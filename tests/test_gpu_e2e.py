"""End-to-end and language-model parity of the HIP path against the CPU oracle on the
synthetic 720x600 / 1000-proposal configuration (BASELINE.json configs[1]) and a small one.

Greedy NMS and arg-max are discontinuous: an fp32 rounding difference upstream (device expf
vs glibc, MFMA summation order vs BLAS) can flip a near-tie.  The comparison (tests/parity.py) therefore has three
parts, none of them a percentage: continuous tensors within 1e-4 relative; integer stages bit-exact when the oracle is
fed the HIP path's own stage inputs; final outputs identical to the oracle's unless the oracle's own data prove a
near-tie (IoU-threshold / score / top-2 logit margin < 1e-4) at the point of departure."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    from densecap_amd.weights import make_synthetic_weights
    return make_synthetic_weights(seed=1234)


@pytest.fixture(scope="module")
def model(weights):
    from densecap_amd import DenseCapModel
    m = DenseCapModel(weights, device=0)
    yield m
    m.ctx.close()


def _check_against_oracle(model, weights, H, W, P, seed):
    """tests/parity.py::strict_check: continuous stages within 1e-4 relative, integer stages bit-exact under teacher
    forcing, final outputs identical to the oracle's or the departure proven an fp32 near-tie in the oracle."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    return parity.strict_check(model, weights, make_synthetic_image(H, W, seed), P)


def test_forward_small_image(model, weights):
    r = _check_against_oracle(model, weights, 224, 288, 100, seed=3)
    assert r["K"] > 0


@pytest.mark.parametrize("seed", [0, 1])
def test_forward_720x600_1000_proposals(model, weights, seed):
    """BASELINE.json configs[1]."""
    r = _check_against_oracle(model, weights, 600, 720, 1000, seed=seed)
    assert r["K"] > 0 and r["matched"] == r["K_oracle"]
    t = model.stage_times()
    assert set(t) >= {"vgg16_trunk", "rpn_nms", "bilinear_roi_pool", "lstm_decode"}
    assert all(v >= 0 for v in t.values())


def test_lm_sample_teacher_forced(model, weights):
    """LanguageModel:sample on the ORACLE's fc7 codes: tokens identical except where the oracle's
    own top-2 logit margin is within fp32 noise."""
    import ctypes as C
    import torch
    from densecap_amd._lib import check
    from oracle import densecap_oracle as O
    rng = np.random.default_rng(0)
    n = 300
    codes = np.maximum(rng.standard_normal((n, 4096)), 0).astype(np.float32)
    oseq, logits = O.lm_sample(torch.from_numpy(codes), weights, 15, return_logits=True)
    ctx = model.ctx
    cd = ctx.to_device(codes); td = ctx.empty((n, 15), np.int32)
    check(ctx.h, ctx.lib.dc_op_lm_sample(ctx.h, cd.ptr, n, td.ptr), "dc_op_lm_sample")
    seq = td.numpy()
    bad_rows = np.nonzero((seq != oseq).any(axis=1))[0]
    for r in bad_rows:
        t = int(np.nonzero(seq[r] != oseq[r])[0][0])   # first divergence must be a near-tie
        top2 = torch.topk(logits[t][r], 2).values
        margin = float(top2[0] - top2[1]) / max(1.0, float(top2[0].abs()))
        assert margin < 1e-4, "row %d step %d diverged with margin %g" % (r, t, margin)
    assert seq.min() >= 1 and seq.max() <= weights["vocab_size"] + 1


def test_forward_batch_equals_single(model, weights):
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
    imgs = np.stack([make_synthetic_image(224, 288, s) for s in range(5)])
    batch = model.forward_batch(imgs)
    for i in (0, 3, 4):
        b, s, t = model.forward_raw(imgs[i])
        np.testing.assert_array_equal(batch[i][0], b)
        np.testing.assert_array_equal(batch[i][1], s)
        np.testing.assert_array_equal(batch[i][2], t)


def test_extract_features(model, weights):
    """DenseCapModel:extractFeatures (DenseCapModel.lua:285-304): boxes AND fc7 codes against the oracle."""
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    from tests import parity
    parity.oracle_threads()
    for (H, W, P, seed) in [(224, 288, 100, 3), (600, 720, 1000, 0)]:
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
        img = make_synthetic_image(H, W, seed)
        b, s, _ = model.forward_raw(img)
        fb, ff = model.extractFeatures(img)
        np.testing.assert_array_equal(fb, b)
        st = {}
        ob, _, _ = O.forward_test(img, weights, 0.7, 0.3, P, 15, stages=st)
        ocodes = st["codes"][st["final_nms_idx"]]
        assert len(fb) == len(ob) and ff.shape == ocodes.shape
        assert parity.row_rel_err(fb, ob) <= parity.REL
        assert parity.rel_err(ff, ocodes) <= parity.REL, "fc7 codes of the surviving boxes"


def test_extract_features_always_runs_final_nms(model, weights):
    """DenseCapModel.lua:285-304 calls box_utils.nms unconditionally (no `final_nms_thresh > 0` guard as in
    forward_test): threshold 0 keeps only boxes that overlap no earlier pick."""
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    from tests import parity
    parity.oracle_threads()
    img = make_synthetic_image(224, 288, 3)
    try:
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.0, num_proposals=100)
        fb, ff = model.extractFeatures(img)
        st = {}
        O.forward_test(img, weights, 0.7, 0.0, 100, 15, stages=st)
        b5 = np.concatenate([O.xcycwh_to_x1y1x2y2(st["final_boxes_pre_nms"]), st["obj"][:, None]], 1)
        keep = O.nms(b5, 0.0, None)
        assert 0 < len(keep) < 100 and len(fb) == len(keep)
        assert parity.row_rel_err(fb, st["final_boxes_pre_nms"][keep]) <= parity.REL
        assert parity.rel_err(ff, st["codes"][keep]) <= parity.REL
    finally:
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)


def test_config4_shard_64_images_1000_proposals(model, weights):
    """BASELINE.json configs[3], one GPU's shard: 64 images x 1000 proposals through dc_forward_batch (the lane
    pipeline); every image's final (boxes, scores, tokens) against the oracle -- identical or proven near-tie."""
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    from tests import parity
    parity.oracle_threads()
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    imgs = np.stack([make_synthetic_image(600, 720, 100 + s) for s in range(64)])
    dev = model.ctx.to_device(imgs)
    batch = model.forward_batch_device(dev.ptr, 64, 600, 720)
    dev.free()
    proofs = []
    boxes_total = identical = 0
    for i in range(64):
        st = {}
        ora = O.forward_test(imgs[i], weights, 0.7, 0.3, 1000, 15, stages=st)
        # lists identical, or the departure is REPLAYED (tests/parity.py::hybrid_nms) through the single-image entry point
        # -- bit-identical to the batch result, asserted -- where the HIP path's own stage inputs exist
        rep = parity.final_or_replay(model, O, weights, imgs[i], batch[i], ora, st, 1000)
        why = rep.get("rpn_flips", []) + rep.get("final_list_flips", []) + rep.get("token_near_ties", [])
        if why:
            proofs.append(dict(image=100 + i, flipped_decisions=why, fc7_codes_rel_err=rep.get("fc7_codes_rel_err"),
                               final_boxes_pre_nms_rel_err=rep.get("final_boxes_pre_nms_rel_err")))
        identical += not why
        boxes_total += rep["matched"]
    assert boxes_total > 64 * 100
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    import json
    json.dump(dict(images=64, identical=identical, boxes_matched=boxes_total, replayed_departures=proofs),
              open(os.path.join(ROOT, "gpurun_out", "config4_shard_parity.json"), "w"), indent=1)


def test_errors_are_reported_not_thrown(model):
    from densecap_amd._lib import DenseCapError
    with pytest.raises(DenseCapError):
        model.setTestArgs(num_proposals=0)
    with pytest.raises(DenseCapError):
        model.setTestArgs(num_proposals=2000000)
    model.setTestArgs(num_proposals=100)
    with pytest.raises(AssertionError):
        model.forward_raw(np.zeros((1, 4, 64, 64), np.float32))


def test_config5_1080x720_2000_proposals(model, weights):
    """BASELINE.json configs[4]: 1080x720, 2000 proposals (NMS over 36,720 anchors + decode stress)."""
    r = _check_against_oracle(model, weights, 720, 1080, 2000, seed=5)
    assert r["K"] > 0


def test_config3_batch32_300_proposals(model, weights):
    """BASELINE.json configs[2]: batch of 32 720x600 images, 300 proposals each, through the lane pipeline.
    Size-independent properties: every image of the batch equals its single-image run; duplicate images
    give duplicate results; scores are sorted; token ids are in range."""
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    from tests import parity
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
    base = [make_synthetic_image(600, 720, s) for s in range(4)]
    imgs = np.stack([base[i % 4] for i in range(32)])
    batch = model.forward_batch(imgs)
    assert len(batch) == 32
    try:                                   # the same batch in groups of four images per lane (how bench.py runs this config)
        model.setGroup(4)
        grouped = model.forward_batch(imgs)
    finally:
        model.setGroup(0)
    for a, b in zip(batch, grouped):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    parity.oracle_threads()
    for i in range(4):
        # P=300 against the ORACLE (not against the HIP path itself): final lists identical or proven near-tie
        st = {}
        ora = O.forward_test(base[i], weights, 0.7, 0.3, 300, 15, stages=st)
        parity.final_or_replay(model, O, weights, base[i], batch[i], ora, st, 300)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
        b, s, t = model.forward_raw(base[i])
        for rep in range(i, 32, 4):
            np.testing.assert_array_equal(batch[rep][0], b)
            np.testing.assert_array_equal(batch[rep][1], s)
            np.testing.assert_array_equal(batch[rep][2], t)
        assert len(b) > 0 and (np.diff(s) <= 0).all()
        assert t.min() >= 1 and t.max() <= weights["vocab_size"] + 1


def _same(a, b, what=""):
    for x, y, n in zip(a, b, ("boxes", "scores", "tokens")):
        np.testing.assert_array_equal(x, y, err_msg="%s %s" % (what, n))


# the five BASELINE.json shapes: configs[0] size, configs[1], configs[2] (300 proposals), configs[4], and the webcam regime
CAPTION_ORDER_SHAPES = [(224, 288, 100, 3), (480, 720, 1000, 7), (600, 720, 1000, 0), (600, 720, 300, 2), (720, 1080, 2000, 5),
                        (320, 480, 50, 4)]


@pytest.mark.parametrize("shape", CAPTION_ORDER_SHAPES, ids=lambda s: "%dx%d_p%d" % (s[1], s[0], s[2]))
def test_caption_order_is_output_invariant(model, weights, shape):
    """dc_set_caption_order(1): final NMS first, ONE decode per group over the packed rows it kept -> the same outputs, and
    by construction: the language-model state of every kept row (image encoder output, final h and c) carries the bits the
    reference order gives that RoI -- the contraction routes are planned on one image's P rows in either order."""
    from densecap_amd.weights import make_synthetic_image
    H, W, P, seed = shape
    E, Hd = weights["lm_enc_w"].shape[0], weights["lstm_w"].shape[1] // 4
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    img = make_synthetic_image(H, W, seed)
    try:
        for lanes in (3, 1):                       # multi-lane planning and single-image mode (two-stream decode in the reference order)
            model.setLanes(lanes)
            model.setCaptionOrder(False)
            ref = model.forward_raw(img)
            K = len(ref[0])
            assert 0 < K < P
            idx = model.debug_fetch("final_nms_idx", (P,), np.int32)[0][:K]
            state0 = [model.debug_fetch(n, (P, d))[0][idx] for n, d in (("lm_enc", E), ("lm_h", Hd), ("lm_c", Hd))]
            model.setCaptionOrder(True)
            out = model.forward_raw(img)
            _same(ref, out, "lanes=%d" % lanes)
            assert int(model.debug_fetch("survivor_rows", (1,), np.int32)[0][0]) == K
            for n, d, want in zip(("lm_enc", "lm_h", "lm_c"), (E, Hd, Hd), state0):
                np.testing.assert_array_equal(model.debug_fetch(n, (P, d))[0][:K], want, err_msg="%s lanes=%d" % (n, lanes))
    finally:
        model.setCaptionOrder(False)
        model.setLanes(3)


@pytest.mark.parametrize("shape", [(224, 288, 100), (600, 720, 300), (600, 720, 1000)], ids=lambda s: "%dx%d_p%d" % (s[1], s[0], s[2]))
def test_caption_order_packs_the_survivors_of_a_group(model, weights, shape):
    """Captions after the final NMS in groups of 1..8 images (one packed decode per group, images with different survivor
    counts side by side, a ragged last group) == the reference order image by image."""
    from densecap_amd.weights import make_synthetic_image
    H, W, P = shape
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    imgs = np.stack([make_synthetic_image(H, W, 40 + s) for s in range(7)])
    try:
        model.setCaptionOrder(False); model.setGroup(1)
        ref = model.forward_batch(imgs)
        assert len({len(r[0]) for r in ref}) > 1, "the images should keep different numbers of boxes"
        model.setCaptionOrder(True)
        for g in (1, 2, 3, 4, 6, 8):
            model.setGroup(g)
            got = model.forward_batch(imgs)
            for i, (a, b) in enumerate(zip(ref, got)):
                _same(a, b, "group=%d image %d" % (g, i))
    finally:
        model.setCaptionOrder(False); model.setGroup(0)


def test_caption_order_edge_counts(model, weights):
    """Survivor counts at the edges: final NMS disabled (every RoI survives: the packed block is the whole group), a
    threshold that keeps a handful of rows, and fewer anchors than proposals."""
    from densecap_amd.weights import make_synthetic_image
    imgs = np.stack([make_synthetic_image(96, 128, 60 + s) for s in range(3)])
    try:
        for (P, fthr) in [(64, -1.0), (64, 0.0), (64, 1.0), (5000, 0.3), (1, 0.3)]:
            model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=fthr, num_proposals=P)
            model.setCaptionOrder(False); model.setGroup(1)
            ref = model.forward_batch(imgs)
            model.setCaptionOrder(True); model.setGroup(3)
            got = model.forward_batch(imgs)
            for i, (a, b) in enumerate(zip(ref, got)):
                _same(a, b, "P=%d final_thr=%g image %d" % (P, fthr, i))
    finally:
        model.setCaptionOrder(False); model.setGroup(0)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)


def test_run_model_cli_writes_results_json(tmp_path):
    """run_model.lua equivalent end to end (BASELINE configs[0] plumbing; synthetic weights: no .t7 offline):
    image file -> preprocess -> forward_test -> vis/data/results.json schema of run_model.lua:89-95,182-188."""
    import json
    from PIL import Image
    from densecap_amd import run_model as R
    rng = np.random.default_rng(4)
    img = rng.uniform(0, 255, (240, 360, 3)).astype(np.uint8)
    src = tmp_path / "elephant.png"
    Image.fromarray(img).save(src)
    out_dir = tmp_path / "vis"
    rc = R.main(["-input_image", str(src), "-synthetic_weights", "1", "-num_proposals", "50", "-image_size", "360",
                 "-output_vis_dir", str(out_dir), "-gpu", "0"])
    assert rc == 0
    d = json.load(open(out_dir / "results.json"))
    assert set(d) == {"results", "opt"} and len(d["results"]) == 1
    r = d["results"][0]
    assert r["img_name"] == "elephant.png" and set(r) == {"boxes", "scores", "captions", "img_name"}
    assert len(r["boxes"]) == len(r["scores"]) == len(r["captions"]) > 0 and len(r["boxes"][0]) == 4
    assert all(a >= b for a, b in zip(r["scores"], r["scores"][1:]))
    assert d["opt"]["num_proposals"] == 50 and (out_dir / "elephant.png").exists()


def test_extract_features_cli_writes_feats_and_boxes(tmp_path):
    """extract_features.lua equivalent: -input_txt list -> HDF5 /feats (N,M,4096), /boxes (N,M,4) xywh."""
    from PIL import Image
    from densecap_amd import extract_features as X
    rng = np.random.default_rng(6)
    lines = []
    for i in range(2):
        src = tmp_path / ("im%d.png" % i)
        Image.fromarray(rng.uniform(0, 255, (240, 360, 3)).astype(np.uint8)).save(src)
        lines.append(str(src))
    (tmp_path / "list.txt").write_text("\n".join(lines + ["/nonexistent/ignored_by_max_images.png"]) + "\n")
    out = tmp_path / "feats.h5"
    rc = X.main(["-input_txt", str(tmp_path / "list.txt"), "-output_h5", str(out), "-synthetic_weights", "1",
                 "-num_proposals", "60", "-boxes_per_image", "3", "-image_size", "360", "-max_images", "2",
                 "-final_nms_thresh", "0.4"])
    assert rc == 0
    from densecap_amd.hdf5_min import read_hdf5
    d = read_hdf5(str(out)); feats, boxes = d["feats"], d["boxes"]          # a real HDF5 file (tests/test_hdf5.py: libhdf5 reads it)
    assert feats.shape == (2, 3, 4096) and boxes.shape == (2, 3, 4)
    assert feats.dtype == np.float32 and (feats >= 0).all() and feats.max() > 0      # fc7 codes are post-ReLU
    assert (boxes[:, :, 2:] > 0).all()
    with pytest.raises(SystemExit):                                                 # fewer survivors than requested
        X.main(["-input_txt", str(tmp_path / "list.txt"), "-output_h5", str(out), "-synthetic_weights", "1",
                "-num_proposals", "5", "-boxes_per_image", "50", "-image_size", "360", "-max_images", "1"])


def test_edge_shapes_do_not_break(model, weights):
    """Tiny images (2x2 feature map), more proposals requested than anchors exist, non-multiple-of-16 sizes."""
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    b, s, t = model.forward_raw(make_synthetic_image(48, 64, 1))
    assert 0 < len(b) <= 50 and t.shape == (len(b), 15) and np.isfinite(b).all() and np.isfinite(s).all()
    model.setTestArgs(num_proposals=5000)                     # 96x128 -> 6x8 map -> 576 anchors < 5000
    b, s, t = model.forward_raw(make_synthetic_image(96, 128, 2))
    assert 0 < len(b) <= 576 and (np.diff(s) <= 0).all()
    model.setTestArgs(num_proposals=64)
    b, s, t = model.forward_raw(make_synthetic_image(203, 301, 3))   # odd sizes: ceil-mode pooling everywhere
    assert 0 < len(b) <= 64 and t.min() >= 1


def test_single_lane_mode_parity(model, weights):
    """dc_set_lanes(1) switches on the tail K-split of each conv layer's last partial round (other fp32
    summation order for those rows): same parity bar against the oracle, and still deterministic."""
    from densecap_amd.weights import make_synthetic_image
    model.setLanes(1)
    try:
        r = _check_against_oracle(model, weights, 600, 720, 1000, seed=0)
        assert r["K"] > 0
        img = make_synthetic_image(600, 720, 0)
        a = model.forward_raw(img)
        b = model.forward_batch(np.stack([img, img]))[1]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    finally:
        model.setLanes(3)


def test_uncapped_proposals_and_no_final_nms(model, weights):
    """num_proposals = -1 (LocalizationLayer.lua:322-324) and final_nms_thresh <= 0 (DenseCapModel.lua:261),
    against the oracle on a small image -- full strict check, in forward_raw, forward_batch and extractFeatures."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    img = make_synthetic_image(128, 160, 9)            # 8x10 map -> 960 anchors
    try:
        r = parity.strict_check(model, weights, img, -1)
        assert r["K"] > 0 and r["matched"] == r["K_oracle"]
        b, s, t = model.forward_raw(img)
        bb = model.forward_batch(np.stack([img, img]))          # -1 must work on every entry point
        for out in bb:
            np.testing.assert_array_equal(out[0], b); np.testing.assert_array_equal(out[2], t)
        fb, ff = model.extractFeatures(img)
        np.testing.assert_array_equal(fb, b)
        assert ff.shape == (len(b), 4096)
        r = parity.strict_check(model, weights, img, 40, final_thr=0.0)
        assert r["K"] == r["K_oracle"] == 40                   # RPN order, no sorting by objectness
    finally:
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)


def test_argmax_takes_first_index_on_exact_ties():
    """torch.max on ties (LanguageModel.lua:329): first maximum.  Every odd row of the vocabulary matrix duplicates
    the even row before it, so each step's maximum is an exact two-way tie inside one tile or across two tiles."""
    import ctypes as C
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import check
    from densecap_amd.weights import make_synthetic_weights
    for V, far in ((300, False), (2047, False), (2047, True)):
        w = make_synthetic_weights(seed=7, vocab_size=V, seq_length=6)
        ow, ob = w["lm_out_w"], w["lm_out_b"]
        n2 = (V + 1) // 2
        if far:                              # row j + n2 duplicates row j: the tie spans two column tiles
            ow[n2:2 * n2] = ow[:n2]
            ob[n2:2 * n2] = ob[:n2]
        else:                                # odd rows duplicate the even row before them: tie inside one tile
            ow[1:2 * n2:2] = ow[0:2 * n2:2]
            ob[1:2 * n2:2] = ob[0:2 * n2:2]
        m = DenseCapModel(w, device=0)
        try:
            ctx = m.ctx
            n = 333
            codes = np.maximum(np.random.default_rng(V).standard_normal((n, 4096)), 0).astype(np.float32)
            cd = ctx.to_device(codes); td = ctx.empty((n, 6), np.int32)
            check(ctx.h, ctx.lib.dc_op_lm_sample(ctx.h, cd.ptr, n, td.ptr), "dc_op_lm_sample")
            seq = td.numpy()
            assert seq.min() >= 1 and seq.max() <= V + 1
            if far:
                assert (seq <= n2).all()
            else:
                assert (seq % 2 == 1).all()  # 1-based ids of the even (first) rows are odd
            assert len(np.unique(seq)) > 10
        finally:
            m.ctx.close()


def test_randomised_shapes_and_thresholds_match_oracle():
    """tests/fuzz_e2e.py: random H, W, num_proposals (incl. -1, 1), thresholds (incl. 0, 1, disabled), lanes and
    caption order; every oracle box must be reproduced with identical tokens."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_e2e.py"), "10", "1"], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "FUZZ OK: 10/10" in p.stdout


def test_randomised_groups_and_lanes_are_pure_scheduling():
    """tests/fuzz_groups.py: random (lanes, group) settings -- including single-image mode with a group setting, which
    include/densecap.h documents as ignored there -- give every image of a batch the bits it gets alone."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_groups.py"), "12", "3"], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "GROUP FUZZ OK: 12/12" in p.stdout
    assert '"lanes": 1' in p.stdout                      # the seed draws single-image cases


def test_randomised_caption_order_is_invisible_in_the_outputs():
    """tests/fuzz_groups.py with FUZZ_CROSS_ORDER=1: batches decoded AFTER the final NMS (one packed decode per group, random
    lanes / groups / sizes / thresholds incl. a disabled final NMS) against the reference caption order image by image."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_groups.py"), "16", "11"], capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, FUZZ_CROSS_ORDER="1"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "GROUP FUZZ OK: 16/16" in p.stdout and '"cross_order": true' in p.stdout


def test_lane_count_is_a_pure_scheduling_knob(model, weights):
    """Any lanes >= 2 must give bit-identical results (bench.py picks the count by an untimed trial)."""
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=200)
    imgs = np.stack([make_synthetic_image(224, 288, 40 + s) for s in range(5)])
    dev = model.ctx.to_device(imgs)
    ref = None
    for lanes in (2, 3, 4):
        model.setLanes(lanes)
        out = model.forward_batch_device(dev.ptr, 5, 224, 288)
        if ref is None:
            ref = out
        else:
            for (b0, s0, t0), (b1, s1, t1) in zip(ref, out):
                np.testing.assert_array_equal(b0, b1); np.testing.assert_array_equal(s0, s1)
                np.testing.assert_array_equal(t0, t1)
    rates = model.autotuneLanes(dev.ptr, 5, 224, 288, reps=1)
    assert set(rates) == {2, 3, 4} and all(v > 0 for v in rates.values())
    model.setLanes(3)
    dev.free()


def _prefix(row, end):
    """tokens up to (excluding) END -- what decodeSequence keeps (LanguageModel.lua:86-103)."""
    row = list(int(v) for v in row)
    return row[:row.index(end)] if end in row else row


@pytest.mark.parametrize("beam", [1, 5, 20])
def test_beamsearch_teacher_forced(beam):
    """LM:beamsearch (LanguageModel.lua:170-290) through dc_op_lm_sample with dc_set_beam_size, on the ORACLE's codes:
    identical token rows (the whole row, including the deterministic filler after END), except rows where the oracle's
    own selection margin (gap at a top-k boundary or between neighbours in a merge) is below 1e-4.  (beam = 1 is not
    LM:sample in the reference: LanguageModel.lua:224 seeds the beams' hidden state with the cell state.)"""
    import torch
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import check
    from densecap_amd.weights import make_synthetic_weights
    from oracle import densecap_oracle as O
    W = make_synthetic_weights(seed=5, vocab_size=300, seq_length=7)
    m = DenseCapModel(W, device=0)
    try:
        ctx = m.ctx
        n = 70
        # all proposals advance together by default; a small cap on the logits buffer walks the chunk loop (64 + 6 rows)
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"beam_chunk_floats", 1), "dc_debug_set")
        codes = np.maximum(np.random.default_rng(beam).standard_normal((n, 4096)), 0).astype(np.float32)
        oseq, margins = O.lm_beamsearch(torch.from_numpy(codes), W, 7, beam, return_margins=True)
        m.setBeamSize(beam)
        cd = ctx.to_device(codes); td = ctx.empty((n, 7), np.int32)
        check(ctx.h, ctx.lib.dc_op_lm_sample(ctx.h, cd.ptr, n, td.ptr), "dc_op_lm_sample")
        seq = td.numpy()
        bad = np.nonzero((seq != oseq).any(axis=1))[0]
        for r in bad:
            assert margins[r] < 1e-4, "row %d differs (hip %s oracle %s) with oracle margin %g" % (r, seq[r], oseq[r], margins[r])
        assert seq.min() >= 1 and seq.max() <= 301
        with pytest.raises(Exception):
            m.setBeamSize(33)
    finally:
        m.ctx.close()


def test_forward_test_with_beam_search():
    """forward_test with language_model.beam_size set (LanguageModel.lua:129-131): boxes / scores as in the greedy run,
    captions = the oracle's beam-search captions for every final box."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    from oracle import densecap_oracle as O
    from tests import parity
    parity.oracle_threads()
    W = make_synthetic_weights(seed=1234, vocab_size=400, seq_length=8)
    img = make_synthetic_image(224, 288, 4)
    m = DenseCapModel(W, device=0)
    try:
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=120)
        g = m.forward_raw(img)
        for order in (False, True):
            m.setCaptionOrder(order)
            m.setBeamSize(4)
            b, s, t = m.forward_raw(img)
            m.setBeamSize(0)
            np.testing.assert_array_equal(b, g[0]); np.testing.assert_array_equal(s, g[1])
            st = {}
            ob, os_, oseq = O.forward_test(img, W, 0.7, 0.3, 120, 8, stages=st, beam_size=4)
            assert len(ob) == len(b) and parity.row_rel_err(b, ob) <= parity.REL
            end = 401
            for i in range(len(ob)):
                if _prefix(t[i], end) != _prefix(oseq[i], end):
                    mg = st["beam_margins"][st["final_nms_idx"][i]]
                    assert mg < 1e-4, "box %d caption differs with oracle margin %g" % (i, mg)
            caps = m.decodeSequence(t)
            assert len(caps) == len(b) and all(isinstance(c, str) for c in caps)
    finally:
        m.ctx.close()


def test_mixed_image_sizes_reuse_the_lane_workspace(model, weights):
    """run_model -input_dir over mixed aspect ratios: the lane arena grows to the largest size seen and is re-carved,
    not re-allocated, for every other size; results do not depend on what ran before."""
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
    sizes = [(240, 360), (360, 240), (270, 360), (240, 360), (360, 240), (200, 300)]
    first = {}
    model.forward_raw(make_synthetic_image(360, 360, 0))             # the largest footprint first
    a0, _ = model.debug_fetch("arena_allocs", (1,), np.int32)
    for i, (H, W) in enumerate(sizes):
        out = model.forward_raw(make_synthetic_image(H, W, 50 + (i % 3)))
        key = (H, W, i % 3)
        if key in first:
            for x, y in zip(out, first[key]):
                np.testing.assert_array_equal(x, y)
        first[key] = out
    a1, _ = model.debug_fetch("arena_allocs", (1,), np.int32)
    assert a1[0] == a0[0], "lane workspace was re-allocated %d times for smaller images" % (a1[0] - a0[0])


def test_graph_replay_is_bit_identical_and_follows_the_inputs(weights):
    """dc_set_graph_replay: the second forward of a (shape, settings) key is captured, later ones are one hipGraphLaunch.
    Replayed forwards must give exactly the eager bits for NEW image contents (the input copy stays outside the graph), a
    changed setting or shape must not reuse a stale graph, and every entry point (single image, batch over lanes, groups,
    caption order, extractFeatures) must survive replay."""
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import check
    from densecap_amd.weights import make_synthetic_image
    m = DenseCapModel(weights, device=0)
    try:
        def counters():
            return (int(m.debug_fetch("graph_captures", (1,), np.int32)[0][0]), int(m.debug_fetch("graph_launches", (1,), np.int32)[0][0]))
        H, W = 224, 288
        imgs = [make_synthetic_image(H, W, 300 + i) for i in range(6)]
        m.setLanes(1)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
        eager = [m.forward_raw(im) for im in imgs]
        m.setGraphReplay(True)
        c0, l0 = counters()
        replay = [m.forward_raw(im) for im in imgs]                  # eager, capture + launch, launch, launch ...
        c1, l1 = counters()
        assert c1 - c0 == 1 and l1 - l0 == len(imgs) - 1, (c0, l0, c1, l1)
        for a, b in zip(eager, replay):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        assert len(eager[0][0]) > 0 and not np.array_equal(eager[0][0], eager[1][0])
        # the NMS band switch (a debug knob, also the band-fault fallback) is part of the key too: eager once, captured again,
        # and the chunk scan's picks are the band scan's
        check(m.ctx.h, m.ctx.lib.dc_debug_set(m.ctx.h, b"nms_band", 0), "dc_debug_set")
        band_off = [m.forward_raw(imgs[0]) for _ in range(3)]
        check(m.ctx.h, m.ctx.lib.dc_debug_set(m.ctx.h, b"nms_band", 1), "dc_debug_set")
        cb, lb = counters()
        assert cb - c1 == 1 and lb - l1 == 2, (c1, l1, cb, lb)
        for r in band_off:
            for x, y in zip(r, eager[0]):
                np.testing.assert_array_equal(x, y)
        c1, l1 = cb, lb
        # a changed setting is a new key: eager once, captured again -- never the old graph
        m.setTestArgs(rpn_nms_thresh=0.5, final_nms_thresh=0.3, num_proposals=100)
        r2 = [m.forward_raw(imgs[0]) for _ in range(3)]
        c2, l2 = counters()
        assert c2 - c1 == 1 and l2 - l1 == 2
        m.setGraphReplay(False)
        ref2 = m.forward_raw(imgs[0])
        for r in r2:
            for x, y in zip(r, ref2):
                np.testing.assert_array_equal(x, y)
        assert not np.array_equal(ref2[0], eager[0][0]) or len(ref2[0]) != len(eager[0][0])
        # another shape in between re-carves the workspace: the old graph's pointers are stale and must not be replayed
        m.setGraphReplay(True)
        a = [m.forward_raw(imgs[1]) for _ in range(3)]
        other = m.forward_raw(make_synthetic_image(203, 301, 9))
        b = [m.forward_raw(imgs[1]) for _ in range(3)]
        m.setGraphReplay(False)
        ref = m.forward_raw(imgs[1]); ref_other = m.forward_raw(make_synthetic_image(203, 301, 9))
        for r in a + b:
            for x, y in zip(r, ref):
                np.testing.assert_array_equal(x, y)
        for x, y in zip(other, ref_other):
            np.testing.assert_array_equal(x, y)
        # single-image mode with >= 256 RoI rows: the decode forks onto two streams and the final NMS onto a third --
        # the capture has to follow the forks and the joins
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
        m.setGraphReplay(False)
        want300 = m.forward_raw(imgs[3])
        m.setGraphReplay(True)
        for _ in range(4):
            for x, y in zip(m.forward_raw(imgs[3]), want300):
                np.testing.assert_array_equal(x, y)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
        # batches over lanes and groups, both caption orders, and the feature path
        batch = np.stack(imgs)
        for lanes, group, order in ((2, 1, False), (2, 2, True), (3, 3, False), (1, 1, True)):
            m.setLanes(lanes); m.setGroup(group); m.setCaptionOrder(order)
            m.setGraphReplay(False)
            want = m.forward_batch(batch)
            m.setGraphReplay(True)
            for rep in range(3):
                got = m.forward_batch(batch)
                for i in range(len(imgs)):
                    for x, y in zip(got[i], want[i]):
                        np.testing.assert_array_equal(x, y, err_msg="lanes %d group %d order %s rep %d image %d" % (lanes, group, order, rep, i))
        m.setLanes(1); m.setGroup(0); m.setCaptionOrder(False)
        m.setGraphReplay(False)
        fb, ff = m.extractFeatures(imgs[2])
        m.setGraphReplay(True)
        for _ in range(3):
            gb, gf = m.extractFeatures(imgs[2])
            np.testing.assert_array_equal(gb, fb); np.testing.assert_array_equal(gf, ff)
        c3, l3 = counters()
        assert c3 > c2 and l3 > l2
    finally:
        m.ctx.close()


def test_webcam_daemon_with_the_hip_model(tmp_path):
    """webcam/daemon.lua:55-102 end to end with the real model (small vocabulary): a 640x480 frame dropped into the input
    directory is consumed, <id>.json carries boxes rescaled to the ORIGINAL frame, and the result equals what
    forward_test gives on the same preprocessed frame (webcam settings: 480 px, 50 proposals, single_machine_demo.lua:25-26)."""
    import json
    from PIL import Image
    from densecap_amd import DenseCapModel, daemon as D
    from densecap_amd.run_model import load_image_caffe, xcycwh_to_xywh
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=1234, vocab_size=300, seq_length=8)
    m = DenseCapModel(W, device=0)
    try:
        m.setLanes(1)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
        ind, outd = tmp_path / "in", tmp_path / "out"
        ind.mkdir()
        frame = np.random.default_rng(9).uniform(0, 255, (960, 1280, 3)).astype(np.uint8)
        Image.fromarray(frame).save(ind / "frame3.jpg", quality=95)
        x, _ = load_image_caffe(str(ind / "frame3.jpg"), 480)
        assert x.shape == (1, 3, 360, 480)
        eb, es, ecaps = m.forward_test(x)
        opt = D.build_parser().parse_args(["-input_dir", str(ind), "-output_dir", str(outd), "-max_polls", "1",
                                           "-max_image_size", "480", "-num_proposals", "50"])
        D.serve(m, opt)
        out = json.load(open(outd / "frame3.json"))
        assert not (ind / "frame3.jpg").exists()
        assert out["height"] == 960 and out["width"] == 1280 and out["captions"] == ecaps and len(ecaps) > 0
        np.testing.assert_allclose(out["boxes"], D.scale_boxes_xywh(xcycwh_to_xywh(eb), 960.0 / 360.0), rtol=1e-6)
        # (the daemon preprocessed the frame ON THE DEVICE -- dc_preprocess_u8 -- and `eb` came from the host restatement: the
        # equality above is end to end.)  The host route behind -host_preprocess 1 writes the same file:
        Image.fromarray(frame).save(ind / "frame3.jpg", quality=95)
        opt_h = D.build_parser().parse_args(["-input_dir", str(ind), "-output_dir", str(tmp_path / "out_host"), "-max_polls", "1",
                                             "-max_image_size", "480", "-num_proposals", "50", "-host_preprocess", "1"])
        D.serve(m, opt_h)
        assert json.load(open(tmp_path / "out_host" / "frame3.json")) == out
        # graph replay (the daemon's default): the second frame of a size is a hipGraph launch, same results
        m.setGraphReplay(True)
        for _ in range(2):
            Image.fromarray(frame).save(ind / "frame3.jpg", quality=95)
            D.serve(m, opt)
            assert json.load(open(outd / "frame3.json")) == out
        m.setGraphReplay(False)
    finally:
        m.ctx.close()


def test_image_groups_do_not_change_results(model, weights):
    """dc_set_group: 2, 3 or 4 images sharing the dense stages' launches (convolutions over all of them, fc6/fc7 and the
    decode over all their RoI rows) must give each image exactly the results it gets alone -- the kernel route and the
    split-K factor are planned per image.  Batch sizes that are no multiple of the group leave a smaller group at the end."""
    from densecap_amd.weights import make_synthetic_image
    try:
        for (H, W, P, n) in [(224, 288, 100, 7), (600, 720, 1000, 5), (203, 301, 64, 6), (600, 720, 300, 9)]:
            model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
            imgs = np.stack([make_synthetic_image(H, W, 70 + s) for s in range(n)])
            outs = {}
            for group in (1, 2, 3, 4, 6, 8, 0):
                model.setGroup(group)
                outs[group] = model.forward_batch(imgs)
            for i in range(n):
                single = model.forward_raw(imgs[i])
                for group in (1, 2, 3, 4, 6, 8, 0):
                    for x, y in zip(outs[group][i], single):
                        np.testing.assert_array_equal(x, y, err_msg="%dx%d P=%d group %d image %d" % (W, H, P, group, i))
                assert len(single[0]) > 0
        # random sizes / proposal counts / thresholds (odd sizes exercise the ceil-mode pool windows per image)
        rng = np.random.default_rng(11)
        for case in range(8):
            H = int(rng.integers(40, 330)); W = int(rng.integers(40, 400))
            P = int(rng.choice([1, 7, 50, 128, 300, -1]))
            model.setTestArgs(rpn_nms_thresh=float(rng.choice([0.3, 0.7])), final_nms_thresh=float(rng.choice([0.0, 0.3, 0.5])),
                              num_proposals=P)
            model.setCaptionOrder(bool(case % 2))
            G = 2 + case % 3
            imgs = np.stack([make_synthetic_image(H, W, 900 + 3 * case + s) for s in range(G + 1)])
            model.setGroup(G)
            grouped = model.forward_batch(imgs)
            model.setGroup(1)
            for i in range(G + 1):
                for x, y in zip(grouped[i], model.forward_raw(imgs[i])):
                    np.testing.assert_array_equal(x, y, err_msg="case %d (%dx%d, P=%d, group %d) image %d" % (case, W, H, P, G, i))
        with pytest.raises(Exception):
            model.setGroup(9)
    finally:
        model.setGroup(0)
        model.setCaptionOrder(False)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)


def test_abi_edge_cases_report_errors_and_truncate(model, weights):
    """C-ABI behaviour at the edges (include/densecap.h): a result capacity below K truncates to the best `capacity` rows,
    bad arguments come back as DC_E_* codes with a message, nothing aborts."""
    import ctypes as C
    from densecap_amd import _lib
    from densecap_amd._lib import DcResult, DenseCapError
    from densecap_amd.weights import make_synthetic_image
    lib, h = model.lib, model.ctx.h
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=100)
    img = make_synthetic_image(224, 288, 3)
    full = model.forward_raw(img)
    K = len(full[0])
    assert K > 5
    cap = 5
    b = np.zeros((cap, 4), np.float32); s_ = np.zeros(cap, np.float32); t = np.zeros((cap, 15), np.int32)
    r = DcResult(); r.capacity = cap
    r.boxes = b.ctypes.data_as(_lib.c_float_p); r.scores = s_.ctypes.data_as(_lib.c_float_p); r.tokens = t.ctypes.data_as(_lib.c_int32_p)
    assert lib.dc_forward_test(h, img.ctypes.data, 224, 288, 0, C.byref(r)) == 0
    assert r.K == cap and r.T == 15
    np.testing.assert_array_equal(b, full[0][:cap]); np.testing.assert_array_equal(t, full[2][:cap])
    # NULL output pointers are allowed (only K comes back)
    r2 = DcResult(); r2.capacity = 100
    assert lib.dc_forward_test(h, img.ctypes.data, 224, 288, 0, C.byref(r2)) == 0 and r2.K == K
    # bad arguments
    r3 = DcResult(); r3.capacity = 0
    assert lib.dc_forward_test(h, img.ctypes.data, 224, 288, 0, C.byref(r3)) == -1          # DC_E_INVALID
    assert b"capacity" in lib.dc_last_error(h)
    assert lib.dc_forward_test(h, img.ctypes.data, 16, 16, 0, C.byref(r2)) == -1             # below 32 px
    assert lib.dc_forward_test(h, None, 224, 288, 0, C.byref(r2)) == -1
    assert lib.dc_set_lanes(h, 0) == -1 and lib.dc_set_lanes(h, 5) == -1
    assert lib.dc_set_beam_size(h, -1) == -5 and lib.dc_set_group(h, 9) == -1                # DC_E_UNSUPPORTED / DC_E_INVALID
    assert lib.dc_debug_fetch(h, b"no_such_tensor", b.ctypes.data, b.nbytes) < 0
    # every dc_debug_set knob refuses values just outside what it accepts, with a message naming it; unknown names too
    refused = {"beam_chunk_floats": [0], "nms_band": [-1, 2], "v2_stages": [-1, 1, 4], "force_cfg": [-1, 7],
               "plan_mode": [-2, 2], "stagger": [-1, 4097], "epi_wide": [-1, 2], "walk": [-1, 2], "bf3_all": [-1, 2],
               "bf3_presplit": [-1, 2], "tail_mode": [-1, 3]}
    for name, values in refused.items():
        for v in values:
            assert lib.dc_debug_set(h, name.encode(), v) == -1, (name, v)
            assert name.encode() in lib.dc_last_error(h), (name, v)
    assert lib.dc_debug_set(h, b"no_such_knob", 0) == -1
    # an image whose conv1 activation would pass the kernels' 32-bit operand offsets (~16 Mpx) is refused up front
    assert lib.dc_forward_test(h, img.ctypes.data, 4200, 4200, 0, C.byref(r2)) == -5
    assert b"16 Mpx" in lib.dc_last_error(h)
    # and the context still works afterwards
    again = model.forward_raw(img)
    for x, y in zip(again, full):
        np.testing.assert_array_equal(x, y)


def test_forward_images_of_mixed_sizes_equals_one_by_one(model, weights, tmp_path):
    """dc_forward_images (run_model.lua -input_dir over photographs of different sizes): pipelined over the lanes, every
    image's result is bit for bit what dc_forward_test gives it; then the run_model CLI over such a directory."""
    import json
    from PIL import Image
    from densecap_amd import run_model as R
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=80)
    sizes = [(240, 360), (360, 240), (203, 301), (240, 360), (96, 128), (330, 330), (360, 240)]
    imgs = [make_synthetic_image(H, W, 300 + i) for i, (H, W) in enumerate(sizes)]
    outs = model.forward_images(imgs)
    assert len(outs) == len(imgs)
    for img, out in zip(imgs, outs):
        for x, y in zip(out, model.forward_raw(img)):
            np.testing.assert_array_equal(x, y)
    assert model.forward_images([]) == []
    # the same for extractFeatures (extract_features.lua's loop)
    feats = model.extractFeatures_images(imgs[:4])
    for img, (fb, ff) in zip(imgs[:4], feats):
        sb, sf = model.extractFeatures(img)
        np.testing.assert_array_equal(fb, sb); np.testing.assert_array_equal(ff, sf)
    rng = np.random.default_rng(8)
    d = tmp_path / "photos"
    d.mkdir()
    for i, (H, W) in enumerate([(240, 360), (360, 240), (300, 300)]):
        Image.fromarray(rng.uniform(0, 255, (H, W, 3)).astype(np.uint8)).save(d / ("p%d.png" % i))
    out_dir = tmp_path / "vis"
    rc = R.main(["-input_dir", str(d), "-synthetic_weights", "1", "-num_proposals", "40", "-image_size", "360",
                 "-output_vis_dir", str(out_dir), "-gpu", "0"])
    assert rc == 0
    res = json.load(open(out_dir / "results.json"))["results"]
    assert [r["img_name"] for r in res] == ["p0.png", "p1.png", "p2.png"]
    assert all(len(r["boxes"]) == len(r["captions"]) > 0 for r in res)


def test_large_image_beyond_65536_anchors(model, weights):
    """The reference puts no limit on the number of RPN boxes (box_utils.lua:154-256; `-image_size` above ~1184 px):
    1600x1200 -> 75x100 map x 12 = 90,000 anchors through the windowed NMS, final outputs against the oracle."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    r = parity.strict_check(model, weights, make_synthetic_image(1200, 1600, 21), 1000, stages=False)
    assert r["K"] > 0 and r["matched"] == r["K_oracle"]


def test_ring_depth_is_invisible_in_decode(model, weights):
    """dc_debug_set("v2_stages"): the 128x64-tile kernel with a two-stage LDS ring (three workgroups per CU; the default once
    a launch has >= 3 tiles per CU, i.e. the vocabulary projection at 1000 rows) and with three stages walks K in the same
    order: the sampled tokens must be identical whichever is forced, at row counts either side of the switch."""
    from densecap_amd._lib import check
    ctx = model.ctx
    rng = np.random.default_rng(12)
    try:
        for n in (130, 300, 1000):
            codes = np.maximum(rng.standard_normal((n, 4096)), 0).astype(np.float32)
            cd = ctx.to_device(codes); td = ctx.empty((n, 15), np.int32)
            outs = []
            for st in (0, 2, 3):
                check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"v2_stages", st), "dc_debug_set")
                check(ctx.h, ctx.lib.dc_op_lm_sample(ctx.h, cd.ptr, n, td.ptr), "dc_op_lm_sample")
                outs.append(td.numpy().copy())
            np.testing.assert_array_equal(outs[1], outs[0]); np.testing.assert_array_equal(outs[2], outs[0])
            assert outs[0].min() >= 1
            cd.free(); td.free()
    finally:
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"v2_stages", 0), "dc_debug_set")


def test_tile_walk_and_ring_depth_are_invisible_under_a_device_row_count(model, weights):
    """Round 6: with a device-side row count (captions after the final NMS) every contraction kernel rebuilds its tile map for the
    LIVE row tiles.  A launch the host made as a tile WALK (dc_debug_set "walk": fewer workgroups than tiles) must then walk the
    live tiles with the workgroups there are -- the first version mapped one tile per workgroup and left the tiles past the grid
    uncomputed: garbage tokens, then a fault in the xg row gather (found by tests/fuzz_e2e.py seed 61 case 95: 755x524, uncapped
    proposals, final threshold 1.0 = 5,977 kept rows of 19,008, single-image mode).  Same bits with the walk and the ring depths
    forced, in both caption orders, at that case's size and at 720x600 / 1000."""
    from densecap_amd._lib import check
    from densecap_amd.weights import make_synthetic_image
    ctx = model.ctx
    try:
        for (H, W, P, fthr, lanes) in ((755, 524, -1, 1.0, 1), (600, 720, 1000, 0.3, 1), (600, 720, 1000, 0.3, 2)):
            img = make_synthetic_image(H, W, 1095)
            model.setLanes(lanes)
            model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=fthr, num_proposals=P)
            base = None
            for order in (False, True):
                for walk, st in ((0, 0), (1, 3), (1, 2), (0, 2)):
                    model.setCaptionOrder(order)
                    check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"walk", walk), "dc_debug_set")
                    check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"v2_stages", st), "dc_debug_set")
                    out = model.forward_raw(img)
                    assert out[2].min() >= 1 and out[2].max() <= model.vocab_size + 1
                    if base is None:
                        base = out
                    for a, b in zip(out, base):
                        np.testing.assert_array_equal(a, b)
            assert len(base[0]) > (3000 if P < 0 else 100)
    finally:
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"walk", 0), "dc_debug_set")
        check(ctx.h, ctx.lib.dc_debug_set(ctx.h, b"v2_stages", 0), "dc_debug_set")
        model.setCaptionOrder(False)
        model.setLanes(3)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)


def test_webcam_regime_forward(model, weights):
    """forward_test at the webcam settings (480 px, 50 proposals, single_machine_demo.lua:25-26), single-image mode, against
    the oracle (every stage) -- also with captions after the final NMS (device-side row count) and for a pair of images in
    one group."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    img = make_synthetic_image(320, 480, 31)
    try:
        model.setLanes(1)
        r = parity.strict_check(model, weights, img, 50)
        assert r["K"] > 0 and r["matched"] == r["K_oracle"]
        outs = []
        for order in (False, True):
            model.setCaptionOrder(order)
            model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
            outs.append(model.forward_raw(img))
        for x, y in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(x, y)
        assert len(outs[0][0]) > 0
        model.setCaptionOrder(False)
        model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=30)
        imgs = np.stack([make_synthetic_image(320, 480, 40 + s) for s in range(2)])
        model.setLanes(3)                                   # (group invariance is a multi-lane property: single-image mode re-plans the last tile round)
        model.setGroup(2)
        pair = model.forward_batch(imgs)
        model.setGroup(0)
        for i in range(2):
            single = model.forward_raw(imgs[i])
            for x, y in zip(pair[i], single):
                np.testing.assert_array_equal(x, y)
    finally:
        model.setCaptionOrder(False); model.setGroup(0); model.setLanes(3)


def test_clip_boxes_false_matches_oracle(model, weights):
    """localization_layer.test_clip_boxes = false (LocalizationLayer.lua:235,272-300 skipped: no clipping, no valid mask),
    set through the layer's own setTestArgs as train.lua:139 does: every stage against the oracle run the same way; the
    model's setTestArgs then turns clipping back on (it passes no clip_boxes key, DenseCapModel.lua:185-191)."""
    from densecap_amd.weights import make_synthetic_image
    from tests import parity
    img = make_synthetic_image(224, 288, 5)
    r = parity.strict_check(model, weights, img, 100, clip_boxes=False)
    assert r["K"] > 0 and r["matched"] == r["K_oracle"]
    A = 12 * 14 * 18
    valid, _ = model.debug_fetch("rpn_valid", (A,), np.uint8)
    assert valid.all()
    rb, _ = model.debug_fetch("rpn_boxes", (A, 4))
    assert (rb[:, 0] - rb[:, 2] / 2 < 0).any() or (rb[:, 0] + rb[:, 2] / 2 > 288).any()   # boxes do leave the image
    unclipped = model.forward_raw(img)
    r2 = parity.strict_check(model, weights, img, 100)          # clipping is back on with the model's setTestArgs
    assert model.nets.localization_layer.test_clip_boxes is True
    valid, _ = model.debug_fetch("rpn_valid", (A,), np.uint8)
    assert r2["matched"] == r2["K_oracle"] and len(unclipped[0]) > 0


def test_overflowing_rpn_logits_end_to_end(model, weights):
    """a9 end to end: an RPN score head scaled until its logits reach +-60..+-120.  The device's p (inf/NaN/0 rows included)
    equals the oracle's decode of the device's own head tensor bit for bit, the RPN NMS -- NaN ranked first -- picks the
    same rows as the oracle on the same inputs, and the forward still returns boxes."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image
    from oracle import densecap_oracle as O
    H, Wd, P = 224, 288, 100
    fh, fw = (H + 15) // 16, (Wd + 15) // 16
    k = O.DEFAULT_ANCHORS.shape[1]
    A = k * fh * fw
    # how large the synthetic score logits are as they come: scale the head so that their upper third passes +-100
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    model.forward_raw(make_synthetic_image(H, Wd, 3))
    heads0, _ = model.debug_fetch("rpn_heads", (fh, fw, 6 * k))
    scale = float(100.0 / np.percentile(np.abs(heads0[..., 4 * k:]), 67))
    Wt = dict(weights)
    Wt["rpn_score_w"] = weights["rpn_score_w"] * scale
    Wt["rpn_score_b"] = weights["rpn_score_b"] * scale
    m = DenseCapModel(Wt, device=0)
    try:
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
        boxes, scores, tokens = m.forward_raw(make_synthetic_image(H, Wd, 3))
        heads, _ = m.debug_fetch("rpn_heads", (fh, fw, 6 * k))
        sc = heads[..., 4 * k:]
        assert np.abs(sc).max() > 100 and (np.abs(sc) > 89).mean() > 0.2, float(np.abs(sc).max())
        chw = heads.transpose(2, 0, 1)
        o = O.rpn_decode(np.ascontiguousarray(chw[:4 * k]), np.ascontiguousarray(chw[4 * k:]), H, Wd)
        p, _ = m.debug_fetch("rpn_p", (A,))
        valid, _ = m.debug_fetch("rpn_valid", (A,), np.uint8)
        xyxy, _ = m.debug_fetch("rpn_x1y1x2y2", (A, 4))
        np.testing.assert_array_equal(valid.astype(bool), o["valid"])
        rows = o["rows"]
        a, b = p[rows], o["p"]
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        assert same.mean() >= 1 - 1e-5 and np.isnan(a).sum() > 0, (float(same.mean()), int(np.isnan(a).sum()))
        idx, _ = m.debug_fetch("rpn_nms_idx", (P,), np.int32)
        cnt, _ = m.debug_fetch("rpn_nms_count", (1,), np.int32)
        B = int(cnt[0])
        tf = O.nms(np.concatenate([xyxy[rows], a[:, None]], 1), 0.7, P)
        np.testing.assert_array_equal(idx[:B], rows[tf])
        assert np.isnan(p[idx[0]]) and len(boxes) > 0 and np.isfinite(boxes).all()
    finally:
        m.ctx.close()


def test_beam_scratch_is_recarved_when_beam_or_chunk_grows():
    """Advisor finding (round 3): the beam scratch was reused whenever rows = chunk x beam did not grow, although bm_enc is
    sized by the chunk and bm_top_lp / bm_top_idx by rows x beam.  beam 2 x 1000 proposals then beam 20 x 100 (same 2000
    rows, 10x the top-k candidates); beam 5 x 300 then beam 1 x 1000 (fewer rows, 3.3x the encoder rows): the second call of
    each pair must give what a fresh context gives."""
    import torch
    from densecap_amd import DenseCapModel
    from densecap_amd._lib import check
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=5, vocab_size=300, seq_length=7)
    rng = np.random.default_rng(77)
    codes = np.maximum(rng.standard_normal((1000, 4096)), 0).astype(np.float32)

    def run(m, beam, n):
        m.setBeamSize(beam)
        cd = m.ctx.to_device(codes[:n]); td = m.ctx.empty((n, 7), np.int32)
        check(m.ctx.h, m.ctx.lib.dc_op_lm_sample(m.ctx.h, cd.ptr, n, td.ptr), "dc_op_lm_sample")
        out = td.numpy().copy()
        cd.free(); td.free()
        return out

    for (b1, n1), (b2, n2) in (((2, 1000), (20, 100)), ((5, 300), (1, 1000))):
        fresh = DenseCapModel(W, device=0)
        try:
            want = run(fresh, b2, n2)
        finally:
            fresh.ctx.close()
        m = DenseCapModel(W, device=0)
        try:
            run(m, b1, n1)
            got = run(m, b2, n2)
            again = run(m, b2, n2)
        finally:
            m.ctx.close()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(again, want)
        assert want.min() >= 1 and want.max() <= 301
