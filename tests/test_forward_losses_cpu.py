"""CPU: the host side of the validation losses -- the flags of the evaluate_model command line, `-losses 0` leaving the result as
it was, loss_results travelling through eval_state.json into the second phase, and the -gt_json tokenisation."""
import json

import numpy as np
import pytest

from tests import loss_rules as R
from tests.test_evaluate_cpu import _evaluator_on_rules, _images


def test_cli_accepts_the_loss_flags_with_the_reference_defaults():
    from densecap_amd import evaluate_model, ops
    opt = evaluate_model.build_parser().parse_args([])
    assert opt.losses == 0
    assert evaluate_model.loss_options(opt) == R.DEFAULTS == ops.LOSS_DEFAULTS
    argv = ["-losses", "1", "-sampler_batch_size", "64", "-sampler_high_thresh", "0.6", "-sampler_low_thresh", "0.2",
            "-train_remove_outbounds_boxes", "0", "-mid_box_reg_weight", "0.5", "-mid_objectness_weight", "0.25", "-end_box_reg_weight",
            "0.75", "-end_objectness_weight", "1.5", "-captioning_weight", "2", "-loss_seed", "12345678901"]
    opt = evaluate_model.build_parser().parse_args(argv)
    assert opt.losses == 1
    assert evaluate_model.loss_options(opt) == dict(batch_size=64, high_thresh=0.6, low_thresh=0.2, remove_outbounds=0,
                                                    mid_box_reg_weight=0.5, mid_objectness_weight=0.25, end_box_reg_weight=0.75,
                                                    end_objectness_weight=1.5, captioning_weight=2.0, seed=12345678901)
    o = ops.loss_opts(**evaluate_model.loss_options(opt))
    assert (o.batch_size, o.remove_outbounds, o.seed) == (64, 0, 12345678901) and o.captioning_weight == 2.0
    with pytest.raises(SystemExit):
        evaluate_model.build_parser().parse_args(["-losses", "2"])
    with pytest.raises(ValueError):
        ops.loss_opts(batchsize=3)


def test_losses_off_leaves_state_and_result_as_they_are(monkeypatch, tmp_path, capsys):
    from densecap_amd import evaluate as E, evaluate_model
    ev = _evaluator_on_rules(monkeypatch)
    for im in _images(np.random.default_rng(2), 2):
        ev.add_result(*im)
    E.write_records(str(tmp_path / "off"), ev)
    E.write_records(str(tmp_path / "none"), ev, None)
    off = open(tmp_path / "off" / "eval_state.json").read()
    assert off == open(tmp_path / "none" / "eval_state.json").read() == json.dumps(ev.state())
    assert set(json.loads(off)) == {"scores", "ok", "ov", "npos"}
    res = E.evaluate_from_files(str(tmp_path / "off"))
    assert set(res) == {"map", "ap_breakdown", "detmap", "det_breakdown"} and res == ev.evaluate()
    assert evaluate_model.main(["-records", str(tmp_path / "off")]) == 0
    assert "loss_results" not in capsys.readouterr().out


def test_loss_results_travel_through_the_state_file(monkeypatch, tmp_path, capsys):
    from densecap_amd import evaluate as E, evaluate_model
    ev = _evaluator_on_rules(monkeypatch)
    for im in _images(np.random.default_rng(3), 2):
        ev.add_result(*im)
    per_image = [dict(zip(R.LOSS_KEYS, (0.1, 0.2, 0.3, 0.4, 2.0, 3.0))), dict(zip(R.LOSS_KEYS, (0.3, 0.2, 0.1, 0.0, 4.0, 4.6)))]
    avg = E.dict_average(per_image)
    assert avg == {k: (per_image[0][k] + per_image[1][k]) / 2 for k in R.LOSS_KEYS} and E.dict_average([]) == {}
    E.write_records(str(tmp_path), ev, avg)
    st = json.load(open(tmp_path / "eval_state.json"))
    assert st["loss_results"] == avg and {k: st[k] for k in ("scores", "ok", "ov", "npos")} == ev.state()
    res = E.evaluate_from_files(str(tmp_path))
    assert res["loss_results"] == avg and {k: res[k] for k in ("map", "ap_breakdown", "detmap", "det_breakdown")} == ev.evaluate()
    assert evaluate_model.main(["-records", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert "loss_results:" in out and "captioning_loss: 3.000000" in out and "total_loss: 3.800000" in out
    assert json.loads(out.strip().splitlines()[-1])["loss_results"] == avg


def test_gt_json_captions_become_label_rows():
    from densecap_amd.evaluate_model import encode_gt_captions
    vocab = {1: "a", 2: "dog", 3: "<UNK>", 4: "red", 5: "on", 6: "grass"}
    rows = encode_gt_captions(["A red dog.", "a zebra on grass", "", "a a a a a a a a", "Dog, on; GRASS!"], vocab, 5)
    assert rows.dtype == np.int32 and rows.tolist() == [[1, 4, 2, 0, 0], [1, 3, 5, 6, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [2, 5, 6, 0, 0]]
    assert encode_gt_captions([], vocab, 5).shape == (0, 5)
    no_unk = {1: "a", 2: "dog"}
    assert encode_gt_captions(["a dog"], no_unk, 3).tolist() == [[1, 2, 0]]
    with pytest.raises(ValueError, match="zebra"):
        encode_gt_captions(["a zebra"], no_unk, 3)
    # the same tokenisation query_regions applies to its queries
    from densecap_amd.model import encode_captions
    assert np.array_equal(encode_gt_captions(["A red dog."], vocab, 5), encode_captions(["A red dog."], vocab, 5))
