"""python -m densecap_amd.train end to end on a three-image dataset fixture made on the spot (the project's HDF5 writer, PNG files):
20 iterations from a .t7, the `iter %d:` lines, the loss history, and a checkpoint that run_model's loader reads back into a
model whose weights are the trained ones."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_twenty_iterations_write_a_checkpoint_run_model_loads(tmp_path, capsys):
    from PIL import Image
    from densecap_amd import DenseCapModel, hdf5_min as H, run_model, t7, train
    from tests.test_gpu_dims import SETS, set_weights
    W = set_weights("e_lt_h")
    s = SETS["e_lt_h"]
    t7.save(str(tmp_path / "start.t7"), t7.checkpoint_from_weights(W))
    rng = np.random.default_rng(5)
    nimg, per = 4, 3
    for i in range(nimg):
        Image.fromarray(rng.integers(0, 255, (96, 128, 3)).astype(np.uint8)).save(tmp_path / ("%d.png" % i))
    boxes = np.stack([rng.uniform(30, 100, nimg * per), rng.uniform(25, 70, nimg * per), rng.uniform(20, 60, nimg * per),
                      rng.uniform(20, 50, nimg * per)], 1).astype(np.float32)
    labels = np.zeros((nimg * per, s["T"]), np.int32)
    for r in range(len(labels)):
        n = int(rng.integers(1, s["T"] + 1))
        labels[r, :n] = rng.integers(1, s["V"] + 1, n)
    first = np.arange(nimg, dtype=np.int32) * per + 1
    H.write_hdf5(str(tmp_path / "vg.h5"), dict(boxes=boxes, labels=labels, img_to_first_box=first, img_to_last_box=first + per - 1,
                                               split=np.asarray([0, 1, 0, 0], np.int32)))
    json.dump({"idx_to_filename": {str(i + 1): "%d.png" % i for i in range(nimg)}}, open(tmp_path / "vg.json", "w"))
    out = str(tmp_path / "out.t7")
    rc = train.main(["-checkpoint_start_from", str(tmp_path / "start.t7"), "-data_h5", str(tmp_path / "vg.h5"), "-data_json",
                     str(tmp_path / "vg.json"), "-image_dir", str(tmp_path), "-image_size", "128", "-max_iters", "20",
                     "-sampler_batch_size", "16", "-learning_rate", "1e-4", "-losses_log_every", "5", "-save_checkpoint_every", "10",
                     "-checkpoint_path", out])
    assert rc == 0
    text = capsys.readouterr().out
    assert [l.split(":")[0] for l in text.splitlines() if l.startswith("iter ")] == ["iter 5", "iter 10", "iter 15", "iter 20"]
    assert "total_loss:" in text and text.count("wrote %s" % out) == 2
    hist = json.load(open(os.path.splitext(out)[0] + ".json"))
    assert hist["iter"] == 20 and sorted(hist["loss_history"], key=int) == ["5", "10", "15", "20"]
    assert all(np.isfinite(v) for e in hist["loss_history"].values() for v in e.values())
    # run_model's own loader reads it; the model built from it holds the trained weights, and they moved
    opt = run_model.build_parser().parse_args(["-checkpoint", out])
    Wt = run_model.load_weights(opt)
    m = DenseCapModel(Wt, device=0)
    try:
        got = m.get_weights()
        boxes_out, scores, tokens = m.forward_raw(np.zeros((3, 96, 128), np.float32))
    finally:
        m.ctx.close()
    as_np = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
    for k in ("fc7_w", "lstm_w", "rpn_conv_w", "lm_out_b"):
        assert np.array_equal(got[k], as_np(Wt[k])) and not np.array_equal(got[k], as_np(W[k]).reshape(got[k].shape)), k
    assert np.array_equal(got["conv_w"][5], as_np(W["conv_w"][5]))
    assert np.isfinite(scores).all()
