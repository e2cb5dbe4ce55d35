"""CPU: densecap_amd.evaluate's vectorised `evaluate_records` against the literal loops of tests/eval_rules.py, the records and
state files, the second (GPU-free) phase of the command line, flag parsing, and hdf5_min's seeking reader."""
import json

import numpy as np
import pytest

from tests import eval_rules as R


def _random_records(rng, n, npos, p_ok=0.6, ties=False):
    scores = np.round(rng.uniform(-3, 3, n), 1) if ties else rng.uniform(-3, 3, n)
    ok = (rng.uniform(0, 1, n) < p_ok).astype(np.uint8)
    ov = np.where(rng.uniform(0, 1, n) < 0.3, 0.0, rng.uniform(0, 1, n))
    ov[rng.uniform(0, 1, n) < 0.2] = 0.5                                      # exactly on a min_overlap
    cs = np.round(rng.uniform(0, 0.4, n), 2)                                   # some exactly on a min_score
    return scores, ok, ov, npos, cs


def _same(a, b):
    assert set(a) == set(b) == {"map", "ap_breakdown", "detmap", "det_breakdown"}
    assert a == b, (a, b)                                                      # exact: floats compare by value


def test_vectorised_evaluate_equals_the_literal_loops():
    from densecap_amd.evaluate import evaluate_records
    rng = np.random.default_rng(0)
    cases = [_random_records(rng, n, npos, ties=t) for n, npos, t in ((1, 1, False), (7, 3, False), (60, 25, True), (200, 90, False),
                                                                       (200, 400, True), (33, 1, True))]
    s, ok, ov, npos, cs = _random_records(rng, 50, 20)
    cases.append((s, np.zeros_like(ok), ov, npos, cs))                         # all fp
    cases.append((s, np.ones_like(ok), np.ones_like(ov), 50, np.ones_like(cs)))   # all tp
    cases.append((s, ok, ov, 0, cs))                                           # npos = 0
    cases.append((np.zeros_like(s), ok, ov, npos, cs))                         # every score tied
    sn = s.copy(); sn[[3, 9]] = np.nan; sn[[4]] = np.inf; sn[[5, 6]] = -np.inf
    cases.append((sn, ok, ov, npos, cs))
    cases.append((np.zeros((0,)), np.zeros((0,), np.uint8), np.zeros((0,)), 5, np.zeros((0,))))   # no records
    for s, ok, ov, npos, cs in cases:
        _same(evaluate_records(s, ok, ov, npos), R.evaluate(s, ok, ov, npos))
        _same(evaluate_records(s, ok, ov, npos, cs), R.evaluate(s, ok, ov, npos, cs))
    with pytest.raises(ValueError):
        evaluate_records([0.5, 0.4], [1, 1], [0.5, 0.5], 2, caption_scores=[0.1])
    # keys as the reference writes them
    r = evaluate_records(*cases[2])
    assert sorted(r["det_breakdown"]) == ["ov0.3", "ov0.4", "ov0.5", "ov0.6", "ov0.7"]
    assert len(r["ap_breakdown"]) == 30 and {"ov0.3_score0", "ov0.5_score0.05", "ov0.7_score0.25"} <= set(r["ap_breakdown"])
    assert r["map"] == sum(r["ap_breakdown"].values()) / 30 and r["detmap"] == sum(r["det_breakdown"].values()) / 5


def test_thresholds_are_the_accumulated_hundred():
    from densecap_amd.evaluate import recall_thresholds
    assert recall_thresholds().tolist() == R.recall_thresholds() and len(recall_thresholds()) == 100


def _evaluator_on_rules(monkeypatch, claim_last=True):
    """A DenseCaptioningEvaluator whose device call is replaced by the rules (no GPU here)."""
    from densecap_amd import evaluate as E, ops

    def fake(ctx, det_boxes, det_scores, gt_boxes, merge_thresh=0.7, claim_last=True):
        return [R.match_image(d, s, g, merge_thresh, claim_last) for d, s, g in zip(det_boxes, det_scores, gt_boxes)]
    monkeypatch.setattr(ops, "eval_match", fake)
    return E.DenseCaptioningEvaluator(None, claim_last=claim_last)


def _images(rng, n):
    out = []
    for i in range(n):
        gt = R.clustered_gt(rng, 6 + 3 * i, 3)
        B = 10 + 5 * i
        out.append((np.round(rng.uniform(0, 1, B), 1).astype(np.float32), R.detections_for(rng, gt, B), ["cap %d %d" % (i, k) for k in range(B)],
                    gt, ["ref %d %d" % (i, j) for j in range(len(gt))]))
    return out


def test_records_state_and_both_file_phases(monkeypatch, tmp_path):
    from densecap_amd import evaluate as E, evaluate_model
    rng = np.random.default_rng(1)
    imgs = _images(rng, 3) + [(np.zeros((0,), np.float32), np.zeros((0, 4), np.float32), [], np.zeros((0, 4), np.float32), [])]
    one = _evaluator_on_rules(monkeypatch)
    for im in imgs:
        one.add_result(*im)
    grp = _evaluator_on_rules(monkeypatch)
    grp.add_result(*[[im[k] for im in imgs[:2]] for k in range(5)])
    grp.add_result(*[[im[k] for im in imgs[2:]] for k in range(5)])
    assert one.records() == grp.records() and one.state() == grp.state() and one.num_added() == 4
    recs = one.records()
    assert len(recs) == sum(len(im[0]) for im in imgs)
    for r in recs:
        assert set(r) == {"ok", "ov", "candidate", "references", "imgid"}
        assert r["ok"] in (0, 1) and isinstance(r["ov"], float) and isinstance(r["references"], list)
        assert (r["references"] == []) == (r["ov"] == 0.0)
    # the references of a record are the captions of its group's members, ascending
    m = R.match_image(imgs[0][1], imgs[0][0], imgs[0][3])
    for d in range(len(imgs[0][0])):
        g = m["group"][d]
        assert recs[d]["candidate"] == imgs[0][2][m["order"][d]] and recs[d]["imgid"] == 1
        assert recs[d]["references"] == ([imgs[0][4][j] for j in m["groups"][g]] if g >= 0 else [])
    st = one.state()
    assert set(st) == {"scores", "ok", "ov", "npos"} and st["npos"] == sum(R.match_image(im[1], im[0], im[3])["n_groups"] for im in imgs)
    assert st["scores"][:len(imgs[0][0])] == sorted((float(v) for v in imgs[0][0]), reverse=True)
    res = one.evaluate()
    assert res == R.evaluate(st["scores"], st["ok"], st["ov"], st["npos"]) and res["map"] is None and res["detmap"] > 0
    # ---- files ----
    d = tmp_path / "rec"
    E.write_records(str(d), one)
    assert json.load(open(d / "input.json")) == recs and json.load(open(d / "eval_state.json")) == st
    assert E.evaluate_from_files(str(d)) == res
    cs = [round(float(v), 3) for v in rng.uniform(0, 0.4, len(recs))]
    json.dump(dict(scores=cs, average_score=0.1), open(tmp_path / "output.json", "w"))
    full = E.evaluate_from_files(str(d), str(tmp_path / "output.json"))
    assert full == R.evaluate(st["scores"], st["ok"], st["ov"], st["npos"], cs) and full["det_breakdown"] == res["det_breakdown"]
    # ---- the second phase of the command line: no GPU, no model ----
    assert evaluate_model.main(["-records", str(d), "-caption_scores", str(tmp_path / "output.json")]) == 0
    assert evaluate_model.main(["-records", str(d)]) == 0
    json.dump(dict(scores=cs[:-1]), open(tmp_path / "short.json", "w"))
    with pytest.raises(SystemExit) as e:
        evaluate_model.main(["-records", str(d), "-caption_scores", str(tmp_path / "short.json")])
    assert "scores" in str(e.value) and str(len(recs)) in str(e.value)


def test_cli_prints_the_result(monkeypatch, tmp_path, capsys):
    from densecap_amd import evaluate as E, evaluate_model
    ev = _evaluator_on_rules(monkeypatch)
    for im in _images(np.random.default_rng(2), 2):
        ev.add_result(*im)
    E.write_records(str(tmp_path), ev)
    json.dump(dict(scores=[0.3] * len(ev.records())), open(tmp_path / "output.json", "w"))
    assert evaluate_model.main(["-records", str(tmp_path), "-caption_scores", str(tmp_path / "output.json")]) == 0
    out = capsys.readouterr().out
    assert "mAP: " in out and "detmAP: " in out and "ov0.5_score0.05" in out
    assert json.loads(out.strip().splitlines()[-1]) == ev.evaluate([0.3] * len(ev.records()))


def test_flag_parsing_and_up_front_refusals(tmp_path):
    from densecap_amd import evaluate_model
    opt = evaluate_model.build_parser().parse_args([])
    assert (opt.split, opt.max_images, opt.rpn_nms_thresh, opt.final_nms_thresh, opt.num_proposals, opt.image_size, opt.claim_last) == (
        "val", -1, 0.7, 0.3, 1000, 720, 1)
    opt = evaluate_model.build_parser().parse_args(["-split", "test", "-max_images", "5", "-claim_last", "0", "-gt_json", "g.json"])
    assert (opt.split, opt.max_images, opt.claim_last, opt.gt_json) == ("test", 5, 0, "g.json")
    with pytest.raises(SystemExit):
        evaluate_model.build_parser().parse_args(["-split", "train"])
    for args, word in (([], "-gt_json"), (["-gt_json", "a", "-data_h5", "b", "-data_json", "c"], "-gt_json"),
                       (["-data_h5", "b", "-output_records", "o"], "-data_json"), (["-gt_json", "a"], "-output_records"),
                       (["-caption_scores", "x.json", "-gt_json", "a"], "-records"),
                       (["-records", "r", "-gt_json", "a"], "second phase")):
        with pytest.raises(SystemExit) as e:
            evaluate_model.main(args)
        assert word in str(e.value), (args, e.value)


def test_gt_json_is_scaled_like_the_image(tmp_path):
    from densecap_amd import evaluate_model
    from densecap_amd.run_model import xcycwh_to_xywh
    json.dump({"a.png": dict(boxes=[[10, 20, 100, 50], [1, 1, 400, 200]], captions=["x", "y"]), "b.png": dict(boxes=[], captions=[])},
              open(tmp_path / "gt.json", "w"))
    boxes, caps = evaluate_model.read_gt_json(str(tmp_path / "gt.json"), ["a.png", "b.png"], {"a.png": (200, 400), "b.png": (50, 50)}, 200)
    assert evaluate_model.scaled_size(200, 400, 200) == (100, 200)
    assert xcycwh_to_xywh(boxes["a.png"]).tolist() == [[5.0, 10.0, 50.0, 25.0], [0.5, 0.5, 200.0, 100.0]]
    assert boxes["b.png"].shape == (0, 4) and caps == {"a.png": ["x", "y"], "b.png": []}
    with pytest.raises(SystemExit):
        evaluate_model.read_gt_json(str(tmp_path / "gt.json"), ["c.png"], {"c.png": (1, 1)}, 200)


def test_read_hdf5_names_and_the_dataset_layout(tmp_path):
    from densecap_amd import evaluate_model, hdf5_min as H
    rng = np.random.default_rng(3)
    nimg, nbox = 6, 20
    first = np.asarray([1, 4, 8, 11, 15, 18], np.int32); last = np.asarray([3, 7, 10, 14, 17, 20], np.int32)
    ds = dict(boxes=rng.uniform(1, 700, (nbox, 4)).astype(np.float32), labels=rng.integers(0, 30, (nbox, 5)).astype(np.int32),
              img_to_first_box=first, img_to_last_box=last, split=np.asarray([0, 1, 2, 1, 0, 1], np.int32),
              images=rng.integers(0, 255, (nimg, 3, 8, 8)).astype(np.uint8), lengths=np.arange(nbox, dtype=np.int32),
              box_to_img=np.arange(nbox, dtype=np.int32), image_heights=np.full((nimg,), 8, np.int32),
              image_widths=np.full((nimg,), 8, np.int32), original_heights=np.full((nimg,), 80, np.int32))
    assert len(ds) > 8
    p = str(tmp_path / "vg.h5")
    H.write_hdf5(p, ds)
    full = H.read_hdf5(p)
    assert set(full) == set(ds) and all(np.array_equal(full[k], ds[k]) and full[k].dtype == ds[k].dtype for k in ds)
    some = H.read_hdf5(p, names=("split", "boxes"))
    assert set(some) == {"split", "boxes"} and np.array_equal(some["boxes"], ds["boxes"]) and np.array_equal(some["split"], ds["split"])
    with pytest.raises(KeyError):
        H.read_hdf5(p, names=("split", "nope"))
    # names= does not read what it was not asked for: cut the file inside the last dataset stored (`split`), the others still read
    raw = open(p, "rb").read()
    open(tmp_path / "cut.h5", "wb").write(raw[:-8])
    assert np.array_equal(H.read_hdf5(str(tmp_path / "cut.h5"), names=("boxes",))["boxes"], ds["boxes"])
    with pytest.raises(ValueError):
        H.read_hdf5(str(tmp_path / "cut.h5"), names=("split",))
    # libhdf5 reads the many-dataset file too, where the library exists
    from tests.test_hdf5 import _libhdf5, _read_with_libhdf5
    lib = _libhdf5()
    if lib is not None:
        assert np.array_equal(_read_with_libhdf5(lib, p, "boxes"), ds["boxes"])
        assert np.array_equal(_read_with_libhdf5(lib, p, "split"), ds["split"].astype(np.float32))
    json.dump(dict(idx_to_filename={str(i + 1): "%d.jpg" % (i + 1) for i in range(nimg)}), open(tmp_path / "vg.json", "w"))
    val = evaluate_model.read_dataset(p, str(tmp_path / "vg.json"), "val", -1)
    assert [v[0] for v in val] == ["2.jpg", "4.jpg", "6.jpg"]
    assert np.array_equal(val[0][1], ds["boxes"][3:7]) and np.array_equal(val[0][2], ds["labels"][3:7])
    assert np.array_equal(val[2][1], ds["boxes"][17:20])
    test = evaluate_model.read_dataset(p, str(tmp_path / "vg.json"), "test", -1)
    assert [v[0] for v in test] == ["3.jpg"] and np.array_equal(test[0][1], ds["boxes"][7:10])
    assert len(evaluate_model.read_dataset(p, str(tmp_path / "vg.json"), "val", 2)) == 2
