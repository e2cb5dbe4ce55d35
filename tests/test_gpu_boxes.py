"""Caller-supplied boxes on the GPU (dc_forward_boxes / dc_forward_boxes_images / dc_extract_features_boxes): the model after
the RPN on boxes the caller passes (docs/SEMANTICS.md "Caller-supplied boxes").

Everything that is derivable is asserted BITWISE: a forward on the boxes the RPN path itself pooled is that forward (same lane
capacity, same rows, same launches after the ingest), a list call is its images one by one, a feature row is the fc7 row of
its box.  Against the oracle the constants and procedures are those of tests/parity.py (REL, TOKEN_TOL, compare_final).
"""
import ctypes as C
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
VGG_MEAN_BGR = np.array([103.939, 116.779, 123.68], np.float32)


@pytest.fixture(scope="module")
def weights():
    from densecap_amd.weights import make_synthetic_weights
    return make_synthetic_weights(seed=1234)


@pytest.fixture(scope="module")
def shared_model(weights):
    from densecap_amd import DenseCapModel
    m = DenseCapModel(weights, device=0)
    yield m
    m.ctx.close()


@pytest.fixture
def model(shared_model):
    """The module's model with the scheduling knobs back at their defaults after every test."""
    yield shared_model
    m = shared_model
    m.setGraphReplay(False); m.setBeamSize(0); m.setCaptionOrder(False); m.setLanes(3); m.setGroup(0)
    m.setTestArgs()


def _image(H, W, seed):
    from densecap_amd.weights import make_synthetic_image
    return make_synthetic_image(H, W, seed)


def _random_boxes(rng, n, H, W):
    xc = rng.uniform(1, W, n); yc = rng.uniform(1, H, n); w = rng.uniform(8, 300, n); h = rng.uniform(8, 300, n)
    return np.stack([xc, yc, w, h], 1).astype(np.float32)


def _border_list(H, W):
    """Boxes inside, straddling each border, wholly outside on each side, a 1x1 and a sub-pixel box, the whole image."""
    return np.array([
        [W / 2, H / 2, 100, 80], [60.5, 70.25, 31, 17],                               # inside
        [5, H / 2, 40, 60], [W - 4, H / 2, 40, 60], [W / 2, 3, 60, 40], [W / 2, H - 2, 60, 40],   # straddling left, right, top, bottom
        [-200, H / 2, 50, 50], [W + 200, H / 2, 50, 50], [W / 2, -150, 50, 50], [W / 2, H + 150, 50, 50],   # outside
        [100, 100, 1, 1], [200.3, 150.6, 0.5, 0.25],                                  # 1x1, sub-pixel
        [(W + 1) / 2, (H + 1) / 2, W, H],                                             # the whole image
        [30, 40, 90, 120],
    ], np.float32)


def _fetch(model, name, shape, dtype=np.float32):
    return model.debug_fetch(name, shape, dtype)[0]


def _assert_same(a, b, what=""):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


# ---- 1. round trip ------------------------------------------------------------------------------------------------------
def _round_trip(model, H, W, P, order, lanes, beam=0):
    model.setLanes(lanes); model.setCaptionOrder(bool(order)); model.setBeamSize(beam); model.setGraphReplay(True)
    model.setTestArgs(num_proposals=P)
    img = _image(H, W, 5)
    ref = model.forward_raw(img)
    roi = _fetch(model, "roi_boxes", (P, 4))
    cnt = int(_fetch(model, "rpn_nms_count", (1,), np.int32)[0])
    K = len(ref[0])
    picks = _fetch(model, "final_nms_idx", (P,), np.int32)[:K]
    assert 1 <= cnt <= P and 1 <= K <= cnt
    launches = []
    for call in range(3):
        out = model.forward_boxes(img, roi[:cnt])
        _assert_same(out[:3], ref, "forward_boxes call %d on the RPN path's own RoIs (%dx%d P=%d order=%d lanes=%d beam=%d)"
                     % (call, W, H, P, order, lanes, beam))
        np.testing.assert_array_equal(out[3], picks)
        launches.append(int(_fetch(model, "graph_launches", (1,), np.int32)[0]))
    if beam == 0:                                            # (beam search stays eager)
        assert int(_fetch(model, "graph_replay_on", (1,), np.int32)[0]) == 1
        assert launches[2] > launches[1] > launches[0], "the third call must be a graph replay: %s" % launches
    np.testing.assert_array_equal(_fetch(model, "box_src", (P,), np.int32)[:cnt], np.arange(cnt))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("H,W,P", [(600, 720, 1000), (320, 480, 50)])
def test_round_trip_is_bitwise(model, H, W, P, order, lanes):
    _round_trip(model, H, W, P, order, lanes)


@pytest.mark.parametrize("order", [0, 1])
def test_round_trip_is_bitwise_with_beam_search(model, order):
    _round_trip(model, 320, 480, 50, order, 2, beam=2)


# ---- 2. groups and lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_list_call_equals_image_by_image(model, group):
    P = 50
    model.setLanes(2); model.setTestArgs(num_proposals=P)
    rng = np.random.default_rng(11)
    sizes = [(320, 480), (320, 480), (320, 480), (224, 288), (320, 480), (224, 288)]
    counts = [7, P, 1, 1, 23, P]
    imgs = [_image(h, w, 20 + i) for i, (h, w) in enumerate(sizes)]
    boxes = [_random_boxes(rng, n, h, w) for n, (h, w) in zip(counts, sizes)]
    model.setGroup(1)
    single = [model.forward_boxes(im, b) for im, b in zip(imgs, boxes)]
    model.setGroup(group)
    for i, (a, b) in enumerate(zip(model.forward_boxes_images(imgs, boxes), single)):
        _assert_same(a, b, "image %d of the list (group %d)" % (i, group))
        assert len(a[3]) == len(a[0]) and set(a[3]) <= set(range(counts[i]))
    assert any(len(s[0]) < n for s, n in zip(single, counts)) and all(len(s[0]) >= 1 for s in single)


# ---- 3. features ----------------------------------------------------------------------------------------------------------
def test_feature_rows_are_the_codes_of_their_boxes(model, weights):
    P, H, W = 100, 320, 480
    D = int(weights["fc7_w"].shape[0])
    img = _image(H, W, 31)
    boxes = _random_boxes(np.random.default_rng(3), 64, H, W)
    model.setTestArgs(final_nms_thresh=0.3, num_proposals=P)
    fb, fs, _, fsrc = model.forward_boxes(img, boxes)
    codes = _fetch(model, "codes", (P, D))
    (eb, ef, esrc), = model.extractFeatures_boxes([img], [boxes])
    assert 1 <= len(eb) < 64
    np.testing.assert_array_equal(esrc, fsrc)
    np.testing.assert_array_equal(eb, fb)
    np.testing.assert_array_equal(ef, codes[esrc])
    # no threshold: every box, in input order
    model.setTestArgs(final_nms_thresh=0, num_proposals=P)
    fb0 = model.forward_boxes(img, boxes)
    codes = _fetch(model, "codes", (P, D))
    (eb, ef, esrc), = model.extractFeatures_boxes([img], [boxes])
    np.testing.assert_array_equal(esrc, np.arange(64))
    np.testing.assert_array_equal(fb0[3], np.arange(64))
    np.testing.assert_array_equal(eb, fb0[0])
    np.testing.assert_array_equal(ef, codes[:64])


# ---- 4. no RPN work ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P", [(600, 720, 1000), (320, 480, 50)])
def test_no_rpn_contractions_and_no_rpn_time(model, weights, H, W, P):
    model.setTestArgs(num_proposals=P)
    img = _image(H, W, 5)
    model.forward_raw(img)
    roi = _fetch(model, "roi_boxes", (P, 4))
    cnt = int(_fetch(model, "rpn_nms_count", (1,), np.int32)[0])
    model.mfma_profile(reset=1)
    try:
        ref = model.forward_raw(img)
        a = model.mfma_profile(reset=1)
        t_ref = model.stage_times()
        out = model.forward_boxes(img, roi[:cnt])
        b = model.mfma_profile()
        t_box = model.stage_times()
    finally:
        model.mfma_profile(reset=-1)
    _assert_same(out[:3], ref)
    fh, fw = -(-H // 16), -(-W // 16)
    R = int(weights["rpn_conv_w"].shape[0]); k = int(np.asarray(weights["anchors"]).shape[1])
    rpn_flops = 2.0 * fh * fw * R * 9 * 512 + 2.0 * fh * fw * 6 * k * R
    assert a["launches"] - b["launches"] == 2, (a, b)
    assert a["flops"] - b["flops"] == rpn_flops, (a["flops"] - b["flops"], rpn_flops)
    assert t_ref["rpn_conv_heads_decode"] > 0 and t_ref["rpn_nms"] > 0
    # (these two zeros are ASSIGNED by the library for a forward on supplied boxes -- nothing runs between the stages' events --,
    # not measured: that no RPN work runs is what the launch and FLOP differences above show)
    assert t_box["rpn_conv_heads_decode"] == 0 and t_box["rpn_nms"] == 0
    assert t_box["vgg16_trunk"] > 0 and t_box["bilinear_roi_pool"] > 0


# ---- 5. clip flag -----------------------------------------------------------------------------------------------------------
def test_clip_flag_is_the_oracle_clip_and_compaction(model):
    """Bit for bit oracle.clip_boxes_xcycwh + compaction.  What that clip drops is NOT the boxes outside the image: the
    reference clamps x1 into [1, W-1] and x2 into [2, W] (box_utils.lua:505-508), so a box wholly outside comes out as a
    valid sliver one pixel wide at the border; invalid are the boxes that are no wider (or higher) than a pixel after the
    clamp -- the 1x1 and the sub-pixel box here.  The K = 0 case is therefore a list of such boxes, not an all-outside list
    (which keeps every box: asserted below)."""
    from oracle import densecap_oracle as O
    P, H, W = 50, 320, 480
    model.setTestArgs(final_nms_thresh=0, num_proposals=P)
    img = _image(H, W, 2)
    boxes = _border_list(H, W)
    clipped, valid = O.clip_boxes_xcycwh(boxes, 1, 1, W, H)
    keep = np.nonzero(valid)[0]
    assert valid[:10].all() and not valid[10:12].any() and valid[12:].all()
    out = model.forward_boxes(img, boxes, clip=True)
    cnt = int(_fetch(model, "rpn_nms_count", (1,), np.int32)[0])
    assert cnt == len(keep) == len(out[0])
    np.testing.assert_array_equal(_fetch(model, "roi_boxes", (P, 4))[:cnt], clipped[keep])
    src = _fetch(model, "box_src", (P,), np.int32)
    np.testing.assert_array_equal(src[:cnt], keep)
    assert (src[cnt:] == -1).all()
    np.testing.assert_array_equal(out[3], keep)
    # flag clear: as given
    out = model.forward_boxes(img, boxes)
    np.testing.assert_array_equal(_fetch(model, "roi_boxes", (P, 4))[:len(boxes)], boxes)
    np.testing.assert_array_equal(out[3], np.arange(len(boxes)))
    # everything outside: the reference's clip keeps them all, as slivers at the border
    out = model.forward_boxes(img, boxes[6:10], clip=True)
    np.testing.assert_array_equal(out[3], np.arange(4))
    np.testing.assert_array_equal(_fetch(model, "roi_boxes", (P, 4))[:4], clipped[6:10])
    assert (clipped[6:8, 2] == 1).all() and (clipped[8:10, 3] == 1).all()
    # every box dropped: K = 0, and the call succeeds
    out = model.forward_boxes(img, boxes[10:12], clip=True)
    assert [len(x) for x in out] == [0, 0, 0, 0]
    assert int(_fetch(model, "rpn_nms_count", (1,), np.int32)[0]) == 0
    assert (_fetch(model, "box_src", (P,), np.int32) == -1).all()
    (eb, ef, esrc), = model.extractFeatures_boxes([img], [boxes[10:12]], clip=True)
    assert len(eb) == len(ef) == len(esrc) == 0


# ---- 6. against the oracle -----------------------------------------------------------------------------------------------
_CASES = {}


def _oracle_case(weights, H, W):
    """The recipe: rng(7), the image first (uniform(0,255) minus the VGG mean), then 64 boxes; and the oracle's trunk on it."""
    import torch
    from oracle import densecap_oracle as O
    from tests import parity
    if (H, W) not in _CASES:
        rng = np.random.default_rng(7)
        img = (rng.uniform(0, 255, (3, H, W)).astype(np.float32) - VGG_MEAN_BGR[:, None, None]).astype(np.float32)
        boxes = _random_boxes(rng, 64, H, W)
        parity.oracle_threads()
        torch.set_grad_enabled(False)
        feat = O.vgg16_trunk(torch.from_numpy(img)[None], weights["conv_w"], weights["conv_b"])[0].numpy()
        _CASES[(H, W)] = (img, boxes, feat)
    return _CASES[(H, W)]


@pytest.mark.parametrize("H,W,which,clip,thr", [
    (320, 480, "random", False, 0.0), (320, 480, "random", False, 0.3),
    (600, 720, "random", False, 0.0), (600, 720, "random", False, 0.3),
    (320, 480, "borders", True, 0.0), (320, 480, "borders", True, 0.3), (320, 480, "borders", False, 0.0)])
def test_against_the_oracle(model, weights, H, W, which, clip, thr):
    import torch
    from oracle import densecap_oracle as O
    from tests import parity
    P, T, D = 100, int(weights["seq_length"]), int(weights["fc7_w"].shape[0])
    img, boxes, feat = _oracle_case(weights, H, W)
    if which == "borders":
        boxes = _border_list(H, W)
    model.setTestArgs(final_nms_thresh=thr, num_proposals=P)
    hip = model.forward_boxes(img, boxes, clip=clip)
    B = int(_fetch(model, "rpn_nms_count", (1,), np.int32)[0])
    roi = _fetch(model, "roi_boxes", (P, 4))[:B]
    # ---- the oracle on its own trunk features -----------------------------------------------------------------------
    rois, rows = boxes, np.arange(len(boxes))
    if clip:
        c, valid = O.clip_boxes_xcycwh(boxes, 1, 1, W, H)
        rois, rows = c[valid], np.nonzero(valid)[0]
    np.testing.assert_array_equal(roi, rois)
    oroi = O.bilinear_roi_pool(feat, rois, H, W)                                     # (B,512,7,7)
    x = torch.from_numpy(oroi.reshape(B, -1))
    x = torch.relu(x @ weights["fc6_w"].t() + weights["fc6_b"])
    ocodes = torch.relu(x @ weights["fc7_w"].t() + weights["fc7_b"])
    st = dict(feat=feat, codes=ocodes.numpy())
    fo, oo = parity.oracle_recog_from_rois(O, st, rois, weights, H, W)
    oseq = O.lm_sample(ocodes, weights, T)
    idx2 = O.nms(np.concatenate([O.xcycwh_to_x1y1x2y2(fo), oo[:, None]], 1), thr, None) if thr > 0 else np.arange(B)
    st.update(final_boxes_pre_nms=fo, obj=oo, final_nms_idx=idx2)
    ora = (fo[idx2], oo[idx2], oseq[idx2])
    # ---- continuous stages ------------------------------------------------------------------------------------------
    hroi = _fetch(model, "roi_feats", (P, 7, 7, 512))[:B].transpose(0, 3, 1, 2)
    codes = _fetch(model, "codes", (P, D))[:B]
    obj = _fetch(model, "obj", (P,))[:B]
    fb = _fetch(model, "final_boxes", (P, 4))[:B]
    errs = dict(roi_feats=parity.rel_err(hroi, oroi), codes=parity.rel_err(codes, st["codes"]),
                obj=parity.row_rel_err(obj, oo), final_boxes=parity.row_rel_err(fb, fo))
    print("oracle parity %dx%d %s clip=%d thr=%g: B=%d %s obj %.3f..%.3f" % (W, H, which, clip, thr, B, errs, oo.min(), oo.max()))
    for name, e in errs.items():
        assert e <= parity.REL, "%s: relative error %.3g" % (name, e)
    # ---- tokens, teacher-forced on the HIP codes ---------------------------------------------------------------------
    seq = _fetch(model, "seq", (P, T), np.int32)[:B]
    tf_seq = O.lm_sample(torch.from_numpy(np.ascontiguousarray(codes)), weights, T)
    excused = []
    for r in np.nonzero((seq != tf_seq).any(axis=1))[0]:
        ok, why = parity.token_divergence_proven(O, codes[r], weights, T, seq[r], tf_seq[r])
        assert ok, "decode row %d differs from the oracle on identical codes without a near-tie (%s)" % (r, why)
        excused.append(why)
    # ---- the final list ------------------------------------------------------------------------------------------------
    K = int(_fetch(model, "final_nms_count", (1,), np.int32)[0])
    picks = _fetch(model, "final_nms_idx", (P,), np.int32)[:K].astype(np.int64)
    np.testing.assert_array_equal(hip[3], rows[picks])
    report = {}
    hip_stage = dict(final_boxes=fb, obj=obj, picks=picks, roi_boxes=roi, same_rois=True, H=H, W=W)
    parity.compare_final(O, weights, hip[:3], ora, st, thr, T, report, hip_stage=hip_stage)
    print("   final: %s, teacher-forced near-ties %s" % (report, excused))
    assert len(excused) <= 1 and len(report.get("token_near_ties", [])) <= 1, "at most one row may be excused as a near-tie"
    if which == "random":
        assert np.isfinite(oo).all() and report["K_oracle"] >= 1
        assert report["K_oracle"] == B if thr == 0 else report["K_oracle"] < B      # both branches of the NMS are walked


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(model):
    from densecap_amd import _lib
    P, H, W = 50, 320, 480
    model.setTestArgs(num_proposals=P)
    img = _image(H, W, 9)
    before = model.forward_raw(img)
    good = _random_boxes(np.random.default_rng(1), 8, H, W)
    lib, h = model.lib, model.ctx.h

    def call(boxes, n=None, capacity=P, null_list=False, features=False):
        b = np.ascontiguousarray(boxes, np.float32)
        bl = (_lib.DcBoxList * 1)()
        bl[0].boxes = b.ctypes.data_as(_lib.c_float_p)
        bl[0].n = len(b) if n is None else n
        r = model._new_result(max(capacity, 1))
        r[0].capacity = capacity
        if features:
            ptrs, Hs, Ws = model._image_list([img])
            fb = np.zeros((max(capacity, 1), 4), np.float32); ff = np.zeros((max(capacity, 1), model.fc_dim), np.float32)
            K = np.zeros((1,), np.int32)
            rc = lib.dc_extract_features_boxes(h, ptrs, Hs, Ws, 1, 0, None if null_list else bl, 0, capacity, fb.ctypes.data,
                                               ff.ctypes.data, K.ctypes.data_as(_lib.c_int32_p))
        else:
            rc = lib.dc_forward_boxes(h, img.ctypes.data, H, W, 0, None if null_list else bl, 0, C.byref(r[0]))
        return rc, lib.dc_last_error(h).decode()

    def bad(i, col, v):
        b = good.copy(); b[i, col] = v
        return b

    many = _random_boxes(np.random.default_rng(2), P + 1, H, W)
    cases = [("NaN", dict(boxes=bad(3, 0, np.nan)), "box 3"), ("inf", dict(boxes=bad(5, 1, np.inf)), "box 5"),
             ("w = 0", dict(boxes=bad(2, 2, 0.0)), "box 2"), ("h < 0", dict(boxes=bad(7, 3, -4.0)), "box 7"),
             ("w = inf", dict(boxes=bad(0, 2, np.inf)), "box 0"),
             ("n = 0", dict(boxes=good, n=0), "n >= 1"), ("n = P + 1", dict(boxes=many), "dc_set_test_args"),
             ("NULL list", dict(boxes=good, null_list=True), "bad arguments"),
             ("capacity < n", dict(boxes=good, capacity=7), "capacity"),
             ("features: capacity < n", dict(boxes=good, capacity=7, features=True), "capacity"),
             ("features: NaN", dict(boxes=bad(4, 3, np.nan), features=True), "box 4")]
    for what, kw, needle in cases:
        rc, msg = call(**kw)
        assert rc == -1, "%s: rc %d (%s)" % (what, rc, msg)             # DC_E_INVALID
        assert needle in msg, "%s: %r lacks %r" % (what, msg, needle)
        _assert_same(model.forward_raw(img), before, "forward_test after the refusal of " + what)
    rc, msg = call(good)
    assert rc == 0, msg
    with pytest.raises(ValueError, match="box 3"):
        model.forward_boxes(img, bad(3, 0, np.nan))


# ---- 8. permutation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 1])
def test_a_box_gets_the_same_row_wherever_it_stands(model, weights, lanes):
    """Multi-lane planning: bitwise (a row's summation order does not depend on its tile).  Single-image planning shares a
    layer's partial last round along K, so the order may depend on the tile: parity.REL there (docs/SEMANTICS.md says which
    was observed)."""
    from tests import parity
    P, H, W = 100, 320, 480
    D = int(weights["fc7_w"].shape[0])
    model.setLanes(lanes); model.setTestArgs(final_nms_thresh=0, num_proposals=P)
    img = _image(H, W, 17)
    rng = np.random.default_rng(5)
    boxes = _random_boxes(rng, 64, H, W)
    perm = rng.permutation(64)
    a = model.forward_boxes(img, boxes)
    ca = _fetch(model, "codes", (P, D))[:64]
    b = model.forward_boxes(img, boxes[perm])
    cb = _fetch(model, "codes", (P, D))[:64]
    np.testing.assert_array_equal(a[3], np.arange(64)); np.testing.assert_array_equal(b[3], np.arange(64))
    bitwise = all((x[perm] == y).all() for x, y in zip(a[:3] + (ca,), b[:3] + (cb,)))
    print("permutation, lanes %d: %s" % (lanes, "bitwise" if bitwise else "not bitwise: boxes %.3g scores %.3g codes %.3g" % (
        parity.row_rel_err(b[0], a[0][perm]), parity.row_rel_err(b[1], a[1][perm]), parity.rel_err(cb, ca[perm]))))
    if lanes >= 2:
        assert bitwise
    else:
        assert parity.row_rel_err(b[0], a[0][perm]) <= parity.REL and parity.row_rel_err(b[1], a[1][perm]) <= parity.REL
        assert parity.rel_err(cb, ca[perm]) <= parity.REL


def test_a_context_that_only_sees_supplied_boxes_has_its_fault_word(weights):
    """The final NMS and the packed records report a hand-off that never arrived through the ctx's fault word; on the RPN
    path the first NMS used to be what made it.  A fresh context on two lanes (no stream-K, which would make it too) whose
    first and only forwards are on supplied boxes must have it, cleared."""
    from densecap_amd import DenseCapModel
    m = DenseCapModel(weights, device=0)
    try:
        m.setLanes(2); m.setTestArgs(num_proposals=50)
        img = _image(320, 480, 1)
        out = m.forward_boxes(img, _random_boxes(np.random.default_rng(0), 20, 320, 480))
        assert len(out[0]) >= 1
        assert int(_fetch(m, "fault_word", (1,), np.int32)[0]) == 0
        m.extractFeatures_boxes([img], [_random_boxes(np.random.default_rng(1), 5, 320, 480)])
        assert int(_fetch(m, "fault_word", (1,), np.int32)[0]) == 0
    finally:
        m.ctx.close()


# ---- 9. the command line ------------------------------------------------------------------------------------------------------
def test_run_model_input_boxes(tmp_path):
    from PIL import Image
    from densecap_amd import DenseCapModel, run_model
    from densecap_amd.weights import make_synthetic_weights
    rng = np.random.default_rng(4)
    indir = tmp_path / "in"; indir.mkdir()
    for i, (h, w) in enumerate([(200, 300), (200, 300), (260, 180)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(indir / ("im%d.png" % i))
    common = ["-synthetic_weights", "1", "-input_dir", str(indir), "-image_size", "320", "-num_proposals", "50", "-gpu", "0"]
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "a")]) == 0
    first = json.load(open(tmp_path / "a" / "results.json"))["results"]
    assert [r["img_name"] for r in first] == ["im0.png", "im1.png", "im2.png"] and all("src" not in r for r in first)
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "b"), "-input_boxes", str(tmp_path / "a" / "results.json"),
                                    "-final_nms_thresh", "0"]) == 0
    second = json.load(open(tmp_path / "b" / "results.json"))["results"]
    m = DenseCapModel(make_synthetic_weights(), device=0)
    try:
        m.setLanes(2)                                            # what run_model uses for several images
        m.setTestArgs(final_nms_thresh=0, num_proposals=50)
        for a, b in zip(first, second):
            n = len(a["boxes"])
            assert n >= 1 and len(b["boxes"]) == len(b["scores"]) == len(b["captions"]) == n
            assert b["src"] == list(range(n)) and b["img_name"] == a["img_name"]
            x, _ = run_model.load_image_caffe(str(indir / a["img_name"]), 320)
            boxes, scores, tokens, src = m.forward_boxes(x[0], run_model.xywh_to_xcycwh(a["boxes"]))
            np.testing.assert_array_equal(np.asarray(b["boxes"], np.float32), run_model.xcycwh_to_xywh(boxes))
            np.testing.assert_array_equal(np.asarray(b["scores"], np.float32), scores)
            assert b["captions"] == m.decodeSequence(tokens)
    finally:
        m.ctx.close()
    # extract_features with the same flag: the codes of those boxes, in their order, and /src
    from densecap_amd import extract_features
    from densecap_amd.hdf5_min import read_hdf5
    M = min(len(r["boxes"]) for r in first)
    (tmp_path / "paths.txt").write_text("".join("%s\n" % (indir / r["img_name"]) for r in first))
    assert extract_features.main(["-synthetic_weights", "1", "-input_txt", str(tmp_path / "paths.txt"), "-image_size", "320",
                                  "-num_proposals", "50", "-final_nms_thresh", "0", "-boxes_per_image", str(M), "-gpu", "0",
                                  "-input_boxes", str(tmp_path / "a" / "results.json"), "-output_h5", str(tmp_path / "f.h5")]) == 0
    h5 = read_hdf5(str(tmp_path / "f.h5"))
    assert h5["feats"].shape == (3, M, 4096) and h5["src"].dtype == np.int32
    for i, b in enumerate(second):
        np.testing.assert_array_equal(h5["src"][i], np.arange(M))
        np.testing.assert_array_equal(h5["boxes"][i], np.asarray(b["boxes"], np.float32)[:M])
    # an image without an entry is refused by name
    json.dump(dict(results=first[:2]), open(tmp_path / "short.json", "w"))
    with pytest.raises(SystemExit, match="im2.png"):
        run_model.main(common + ["-output_vis_dir", str(tmp_path / "c"), "-input_boxes", str(tmp_path / "short.json")])
