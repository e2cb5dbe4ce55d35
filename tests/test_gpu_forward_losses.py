"""dc_forward_losses end to end at 320x224, at the default dimensions and at one other point of tests/test_gpu_dims.py's family:
the sampler's lists against the rules on the fetched RPN boxes (exact), the six losses from pixels against the float64
restatement fed by the oracle's forward (the project's continuous-stage bar, 1e-4 relative, with an absolute floor of 1e-4 times
the term's weight), the invariances, and the evaluate_model command line."""
import json
import os

import numpy as np
import pytest

from tests import loss_rules as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, WD = 224, 320
REL = 1e-4
WEIGHT_OF = dict(mid_objectness_loss="mid_objectness_weight", mid_box_reg_loss="mid_box_reg_weight",
                 end_objectness_loss="end_objectness_weight", end_box_reg_loss="end_box_reg_weight", captioning_loss="captioning_weight")


def _weights(name):
    from densecap_amd.weights import make_synthetic_weights
    if name == "default":
        return make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    from tests.test_gpu_dims import set_weights
    return set_weights(name)


@pytest.fixture(scope="module", params=["default", "odd32"])
def model(request):
    from densecap_amd import DenseCapModel
    W = _weights(request.param)
    m = DenseCapModel(W, device=0)
    yield m, W, request.param
    m.ctx.close()


def _labels(G, L, V, rng):
    lab = np.zeros((G, L), np.int32)
    for j in range(G):
        n = int(rng.integers(0, L + 1))
        lab[j, :n] = rng.integers(1, V + 1, n)
    return lab


def _oracle_stages(img, W):
    """The oracle's training-form RPN: all rows, boxes not clipped, raw scores."""
    import torch
    from oracle import densecap_oracle as O
    torch.set_grad_enabled(False)
    feat = O.vgg16_trunk(torch.as_tensor(np.asarray(img, np.float32))[None], W["conv_w"], W["conv_b"])
    box_head, score_head = O.rpn_heads(feat, W)
    d = O.rpn_decode(box_head, score_head, img.shape[1], img.shape[2], anchors=np.asarray(W["anchors"], np.float32), clip_boxes=False)
    return feat[0].numpy(), d


def _oracle_losses(img, W, feat, d, gt, lab, pi, pt, ni, opts):
    import torch
    from oracle import densecap_oracle as O
    from tests import score_restatement
    sel = np.concatenate([pi, ni])
    roi = O.bilinear_roi_pool(feat, d["boxes"][sel], img.shape[1], img.shape[2])
    x = torch.from_numpy(roi.reshape(len(sel), -1))
    x = torch.relu(x @ W["fc6_w"].t() + W["fc6_b"])
    codes = torch.relu(x @ W["fc7_w"].t() + W["fc7_b"])
    obj = (codes @ W["obj_w"].t() + W["obj_b"])[:, 0].numpy()
    ft = (codes @ W["boxreg_w"].t() + W["boxreg_b"]).numpy()
    rowlik = np.array([score_restatement.lm_score(codes[r:r + 1].numpy(), W, lab[pt[r]][None])[0, 0] for r in range(len(pi))])
    return R.losses(d["scores2"][pi], d["scores2"][ni], d["anchors"][pi], d["trans"][pi], gt[pt], obj, d["boxes"][pi], ft[:len(pi)],
                    rowlik, lab.shape[1], opts)


def _ranks(mask, idx):
    """ranks of the inputs idx in the ascending list of a mask's members (all must be members)"""
    assert mask[idx].all(), "an input the oracle's rules sampled is no candidate on the device's boxes"
    return (np.cumsum(mask) - 1)[idx].tolist()


def test_three_passes(model):
    from densecap_amd.weights import make_synthetic_image
    m, W, name = model
    V, L = m.vocab_size, m.seq_length
    img = make_synthetic_image(H, WD, 6)
    A = m.num_anchors * 14 * 20
    rng = np.random.default_rng(7)
    bounds = (1, 1, WD, H)
    opts = dict(batch_size=64, seed=3)
    # ---- pass 1: arbitrary ground truth; fetch the RPN boxes ----
    gt0 = np.array([[100, 100, 60, 40], [200, 120, 80, 90]], np.float32)
    m.forward_losses(img, gt0, _labels(2, L, V, rng), **opts)
    boxes = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
    # ---- pass 2: ground truth = a few in-bounds RPN boxes shifted by a pixel or two: positives above the threshold exist ----
    c = R.corners(boxes)
    inb = np.nonzero((c[:, 0] >= 1) & (c[:, 1] >= 1) & (c[:, 2] <= WD) & (c[:, 3] <= H) & (boxes[:, 2] > 20) & (boxes[:, 3] > 20))[0]
    assert len(inb) >= 5
    pick = inb[np.linspace(0, len(inb) - 1, 5).astype(int)]
    gt = (boxes[pick] + np.array([[1, -1, 0, 0], [2, 1, 0, 0], [-1, 2, 0, 0], [0, 1, 1, 0], [1, 1, 0, -1]], np.float32)).astype(np.float32)
    lab = _labels(5, L, V, rng)
    r = m.forward_losses(img, gt, lab, dump=True, **opts)
    boxes2 = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
    assert np.array_equal(boxes, boxes2)
    dev = R.box_sampler(boxes, gt, 64, bounds=bounds, seed=3)
    assert (dev["max_iou"] > np.float32(0.7)).sum() >= 5
    for k in ("pos_input_idx", "pos_target_idx", "neg_input_idx"):
        assert np.array_equal(r[k], dev[k]), k
    for k in ("num_pos", "num_neg", "total_pos", "total_neg", "flags"):
        assert r[k] == dev[k], k
    # ---- pass 3: the lists of the rules on the ORACLE's boxes, forced; the losses from pixels ----
    feat, d = _oracle_stages(img, W)
    print("%s: max |device - oracle| over the RPN boxes: %.3g" % (name, np.abs(d["boxes"] - boxes).max()))
    orc = R.box_sampler(d["boxes"], gt, 64, bounds=bounds, seed=3)
    pi, pt, ni = orc["pos_input_idx"], orc["pos_target_idx"], orc["neg_input_idx"]
    got = m.forward_losses(img, gt, lab, dump=True, forced_pos=_ranks(dev["pos_mask"], pi), forced_neg=_ranks(dev["neg_mask"], ni), **opts)
    assert np.array_equal(got["pos_input_idx"], pi) and np.array_equal(got["neg_input_idx"], ni)
    assert np.array_equal(dev["arg"][pi], pt), "the arg-max ground-truth box of a sampled row differs between the device's boxes and the oracle's"
    ref = _oracle_losses(img, W, feat, d, gt, lab, pi, pt, ni, {})
    floor_total = 0.0
    for k in R.LOSS_KEYS:
        floor = REL * float(np.float32(R.DEFAULTS[WEIGHT_OF[k]])) if k in WEIGHT_OF else floor_total
        floor_total += floor if k in WEIGHT_OF else 0.0
        err = abs(got[k] - ref[k])
        print("%s %s: device %.9g oracle %.9g |diff| %.3g rel %.3g" % (name, k, got[k], ref[k], err, err / max(abs(ref[k]), 1e-300)))
        assert err <= REL * abs(ref[k]) + floor, (k, got[k], ref[k])
    assert (got["masked_mid"], got["masked_end"]) == (ref["masked_mid"], ref["masked_end"])


def test_invariances(model):
    """The same losses bit for bit under lanes 1 and 3, group 1 and 4, both caption orders, num_proposals 50 and 1000, beam size and
    math mode; dc_forward_test before and after a losses call returns identical bits."""
    from densecap_amd.weights import make_synthetic_image
    m, W, name = model
    img = make_synthetic_image(H, WD, 8)
    rng = np.random.default_rng(9)
    gt = np.array([[100, 100, 60, 40], [200, 120, 80, 90], [60, 150, 50, 70]], np.float32)
    lab = _labels(3, m.seq_length, m.vocab_size, rng)
    try:
        m.setTestArgs(num_proposals=50)
        before = m.forward_raw(img)
        base = m.forward_losses(img, gt, lab, dump=True, seed=4)
        after = m.forward_raw(img)
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        settings = [lambda: m.setLanes(1), lambda: m.setLanes(3), lambda: m.setGroup(4), lambda: m.setGroup(1),
                    lambda: m.setCaptionOrder(True), lambda: m.setCaptionOrder(False), lambda: m.setTestArgs(num_proposals=1000),
                    lambda: m.setBeamSize(2), lambda: m.setBeamSize(0), lambda: m.setMathMode(1), lambda: m.setMathMode(0)]
        for i, change in enumerate(settings):
            change()
            r = m.forward_losses(img, gt, lab, dump=True, seed=4)
            for k in R.LOSS_KEYS:
                assert r[k] == base[k], (i, k, r[k], base[k])
            for k in ("pos_input_idx", "pos_target_idx", "neg_input_idx"):
                assert np.array_equal(r[k], base[k]), (i, k)
        assert m.forward_losses(img, gt, lab, seed=5)["total_loss"] != base["total_loss"]          # another draw, another number
    finally:
        m.setGraphReplay(False); m.setBeamSize(0); m.setCaptionOrder(False); m.setLanes(3); m.setGroup(0); m.setMathMode(0)
        m.setTestArgs()


def test_refusals(model):
    from densecap_amd._lib import DenseCapError
    from densecap_amd.weights import make_synthetic_image
    m, W, name = model
    img = make_synthetic_image(64, 96, 1)
    gt = np.array([[40, 30, 20, 20]], np.float32)
    lab = np.zeros((1, 3), np.int32)
    assert m.forward_losses(img, gt, lab)["num_pos"] == 1
    bad = [(gt, np.full((1, 3), m.vocab_size + 1, np.int32), {}), (gt, np.full((1, 3), -1, np.int32), {}),
           (gt, np.array([[0, 1, 0]], np.int32), {}), (gt, np.zeros((1, 65), np.int32), {}),
           (np.array([[40, 30, 0, 20]], np.float32), lab, {}), (np.array([[40, np.nan, 20, 20]], np.float32), lab, {}),
           (np.array([[np.inf, 30, 20, 20]], np.float32), lab, {}), (gt, lab, dict(batch_size=5)), (gt, lab, dict(high_thresh=2.0)),
           (gt, lab, dict(forced_pos=[0] * 40, forced_neg=[0] * 40, batch_size=64))]
    for g, l, kw in bad:
        with pytest.raises(DenseCapError, match=r"\(-1\)"):
            m.forward_losses(img, g, l, **kw)
    with pytest.raises(DenseCapError, match=r"\(-5\)"):
        m.forward_losses(img, np.tile(gt, (513, 1)), np.zeros((513, 3), np.int32))
    assert m.forward_losses(img, gt, lab)["num_pos"] == 1          # the ctx works on


def test_evaluate_model_cli_reports_the_mean_of_the_per_image_calls(tmp_path, capsys):
    """Two synthetic images through `evaluate_model -losses 1`: loss_results is the mean of the per-image forward_losses calls,
    printed, in the result JSON and in eval_state.json; the second phase reports it again."""
    from PIL import Image
    from densecap_amd import DenseCapModel, evaluate_model, ops
    from densecap_amd.run_model import load_weights
    rng = np.random.default_rng(0)
    names = ["a.png", "b.png"]
    gtj = {}
    for i, n in enumerate(names):
        Image.fromarray(rng.integers(0, 255, (120 + 40 * i, 200, 3), dtype=np.uint8)).save(tmp_path / n)
        gtj[n] = dict(boxes=[[20, 30, 80, 60], [100, 40, 70, 50 + 10 * i]], captions=["w3 w7 w7", "w%d" % (5 + i)])
    json.dump(gtj, open(tmp_path / "gt.json", "w"))
    argv = ["-synthetic_weights", "1", "-gt_json", str(tmp_path / "gt.json"), "-image_dir", str(tmp_path), "-image_size", "160",
            "-num_proposals", "50", "-output_records", str(tmp_path / "rec"), "-losses", "1", "-sampler_batch_size", "64", "-loss_seed", "7"]
    assert evaluate_model.main(argv) == 0
    out = capsys.readouterr().out
    res = json.loads(out.strip().splitlines()[-1])
    assert "loss_results:" in out and set(res["loss_results"]) == set(R.LOSS_KEYS)
    assert json.load(open(tmp_path / "rec" / "eval_state.json"))["loss_results"] == res["loss_results"]
    # the per-image calls, on the pixels the command line's pipeline makes of the files
    opt = evaluate_model.build_parser().parse_args(argv)
    m = DenseCapModel(load_weights(opt), device=0)
    try:
        from densecap_amd.run_model import ImagePipeline
        sizes = {n: (120 + 40 * i, 200) for i, n in enumerate(names)}
        gt_boxes, gt_caps = evaluate_model.read_gt_json(str(tmp_path / "gt.json"), names, sizes, 160)
        pipe = ImagePipeline([str(tmp_path / n) for n in names], 160, 0, m.ctx, io_threads=1, chunk=2, want_rgb=False)
        per = []
        try:
            for chunk in pipe:
                for i, dev, _ in chunk:
                    lab = evaluate_model.encode_gt_captions(gt_caps[names[i]], m.idx_to_token, m.seq_length)
                    per.append(ops.forward_losses(m.ctx, dev, gt_boxes[names[i]], lab, on_device=True, batch_size=64, seed=7))
        finally:
            pipe.close()
    finally:
        m.ctx.close()
    assert len(per) == 2
    for k in R.LOSS_KEYS:
        assert res["loss_results"][k] == (per[0][k] + per[1][k]) / 2, k
    assert evaluate_model.main(["-records", str(tmp_path / "rec")]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["loss_results"] == res["loss_results"]
