"""The evaluator end to end on the GPU: the synthetic-weights model's own detections against ground truth made from them, records
per image and per group, detmap against the rules of tests/eval_rules.py, and the command line's two phases."""
import json

import numpy as np
import pytest

from tests import eval_rules as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_weights
    m = DenseCapModel(make_synthetic_weights(seed=1234, vocab_size=200, seq_length=8), device=0)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    yield m
    m.ctx.close()


@pytest.fixture(scope="module")
def images(model):
    """[(scores, boxes, captions, gt_boxes, gt_captions)] for two 160x224 images: ground truth = every third detection, a jittered
    copy of each of those (most merge with their original), and boxes far from everything."""
    from densecap_amd.weights import make_synthetic_image
    rng = np.random.default_rng(0)
    out = []
    for seed in (1, 2):
        boxes, scores, tokens = model.forward_raw(make_synthetic_image(160, 224, seed))
        assert len(boxes) >= 6
        own = boxes[::3]
        jit = own + rng.integers(-2, 3, own.shape).astype(np.float32)
        far = np.asarray([[900 + 60 * k, 900, 30, 30] for k in range(3)], np.float32)
        gt = np.concatenate([own, jit, far]).astype(np.float32)
        out.append((scores, boxes, model.decodeSequence(tokens), gt, ["gt %d %d" % (seed, j) for j in range(len(gt))]))
    return out


def test_records_per_image_and_per_group_and_detmap(model, images):
    from densecap_amd.evaluate import DenseCaptioningEvaluator
    one = DenseCaptioningEvaluator(model.ctx)
    for im in images:
        one.add_result(*im)
    grp = DenseCaptioningEvaluator(model.ctx)
    grp.add_result(*[[im[k] for im in images] for k in range(5)])
    assert one.records() == grp.records() and one.state() == grp.state() and one.num_added() == 2
    ref = [R.match_image(im[1], im[0], im[3], fast=True) for im in images]
    recs = one.records()
    k = 0
    for i, (im, r) in enumerate(zip(images, ref)):
        assert r["n_groups"] < len(im[3]) and (r["group"] >= 0).any()             # the copies merged, something matched
        for d in range(len(im[0])):
            g = int(r["group"][d])
            assert recs[k] == dict(ok=int(r["ok"][d]), ov=float(r["ov"][d]), candidate=im[2][int(r["order"][d])],
                                   references=[im[4][j] for j in r["groups"][g]] if g >= 0 else [], imgid=i + 1), (i, d)
            k += 1
    st = one.state()
    assert st["npos"] == sum(r["n_groups"] for r in ref)
    res = one.evaluate()
    want = R.evaluate(st["scores"], np.concatenate([r["ok"] for r in ref]), np.concatenate([r["ov"] for r in ref]), st["npos"])
    assert res == want and res["map"] is None and res["detmap"] > 0
    cs = [0.01 * (j % 30) for j in range(len(recs))]
    assert one.evaluate(cs) == R.evaluate(st["scores"], st["ok"], st["ov"], st["npos"], cs)
    # the other claim mode, through the same class
    other = DenseCaptioningEvaluator(model.ctx, claim_last=False)
    other.add_result(*[[im[k] for im in images] for k in range(5)])
    ref0 = [R.match_image(im[1], im[0], im[3], claim_last=False, fast=True) for im in images]
    assert other.state()["ok"] == [int(v) for r in ref0 for v in r["ok"]]


def test_command_line_round_trip(tmp_path, capsys):
    from PIL import Image
    from densecap_amd import evaluate as E, evaluate_model
    rng = np.random.default_rng(4)
    indir = tmp_path / "in"; indir.mkdir()
    sizes = {}
    gt = {}
    for i, (h, w) in enumerate([(200, 300), (200, 300), (260, 180)]):
        name = "im%d.png" % i
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(indir / name)
        sizes[name] = (h, w)
        big = [[1 + 10 * k, 1 + 8 * k, w // 2, h // 2] for k in range(4)]          # overlapping quarter-image boxes
        gt[name] = dict(boxes=big + [[w - 30, h - 30, 20, 20]], captions=["c%d" % k for k in range(5)])
    gt["im2.png"] = dict(boxes=[], captions=[])                                   # an image without ground truth
    json.dump(gt, open(tmp_path / "gt.json", "w"))
    rec = tmp_path / "rec"
    assert evaluate_model.main(["-synthetic_weights", "1", "-gt_json", str(tmp_path / "gt.json"), "-image_dir", str(indir),
                                "-image_size", "320", "-num_proposals", "50", "-gpu", "0", "-output_records", str(rec)]) == 0
    out = capsys.readouterr().out
    recs = json.load(open(rec / "input.json")); st = json.load(open(rec / "eval_state.json"))
    assert len(recs) == len(st["ok"]) == len(st["ov"]) == len(st["scores"]) > 0 and {r["imgid"] for r in recs} <= {1, 2, 3}
    assert [r["ok"] for r in recs] == st["ok"] and [r["ov"] for r in recs] == st["ov"]
    # the merge depends on the ground truth alone: npos is what the rules make of the scaled boxes
    boxes, _ = evaluate_model.read_gt_json(str(tmp_path / "gt.json"), sorted(gt), sizes, 320)
    assert st["npos"] == sum(len(R.merge_boxes(R.corners(boxes[n]), 0.7)) for n in sorted(gt))
    res = E.evaluate_from_files(str(rec))
    assert res == R.evaluate(st["scores"], st["ok"], st["ov"], st["npos"]) and json.loads(out.strip().splitlines()[-1]) == res
    assert "detmAP: " in out and "mAP: " not in out.replace("detmAP: ", "")
    json.dump(dict(scores=[0.02 * (j % 20) for j in range(len(recs))]), open(tmp_path / "output.json", "w"))
    assert evaluate_model.main(["-records", str(rec), "-caption_scores", str(tmp_path / "output.json")]) == 0
    full = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert full["det_breakdown"] == res["det_breakdown"] and len(full["ap_breakdown"]) == 30 and full["map"] is not None
