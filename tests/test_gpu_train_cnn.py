"""dc_forward_backward_cnn (docs/SEMANTICS.md, "CNN gradients"): dc_forward_backward with conv_net2's activations kept by the
forward and the backward through conv5_3 .. conv3_1 behind it, on tests/test_gpu_train_step.py's weights and inputs.

The kept-activation forward runs conv3_1 .. conv5_3 through the unfused convolution and a pool launch where the test-time trunk
fuses the pool into the convolution's epilogue.  Its conv5_3 map must be the fused trunk's bit for bit, at an even-sized image
and at one whose conv3 and conv4 maps are odd in both directions (84 x 68: 21 x 17, then 11 x 9, then 6 x 5), where the two
forms plan their tiles on different row counts.  Then forward_backward(cnn=True) is forward_backward's dict bit for bit, and its
18 further tensors are ops.cnn_grad's on the kept pool2 map and the returned grad_cnn_features.

dc_train_set_cnn: mode 0 is today's step; mode 1 (decay and Adam on a zero gradient) and mode 2 (the full backward) give the
float32 restatement of tests/optim_rules.py on forward_backward(cnn=True)'s gradients, with the CNN's own t; the refresh, the
checkpoint, the call order and the tool's -finetune_cnn_after."""
import numpy as np
import pytest

from tests import optim_rules as R
from tests.test_gpu_train_step import (DECAY, FAST, FORCED, H, LOSS, WD, _assert_weights, _bits, _cfg_default, _cfg_graph,  # noqa: F401
                                       _cfg_math_after, _cfg_math_before, _model, _np, _rule_step, _same as _same_tree,
                                       _step, setup)          # (setup: a fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
ODD = (84, 68)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    if isinstance(a, float):
        return _bits(np.float64(a)) == _bits(np.float64(b))
    return a == b


@pytest.mark.parametrize("size", [(H, WD), ODD], ids=["96x128", "84x68"])
def test_kept_activation_forward_gives_the_fused_trunks_feat(setup, size):
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    W = setup[0]
    hh, ww = size
    img = make_synthetic_image(hh, ww, 6)
    gt, lab = np.array([[40, 36, 40, 30]], F32), np.ones((1, 1), np.int32)
    h4, w4 = ops.cnn_input_size(hh, ww)
    layers, (fh, fw) = ops.cnn_shapes(h4, w4)
    if size == ODD:
        assert [(h % 2, w % 2) for i, h, w, _, _ in layers if i in (4, 7)] == [(1, 1), (1, 1)]
    m = _model(W)
    try:
        m.forward_losses(img, gt, lab, **LOSS)
        fused = m.debug_fetch("loss_feat", (fh, fw, 512))[0].copy()
        res = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, cnn=True, **LOSS)
        x4, kept = ops.cnn_kept(m.ctx, hh, ww)
        again = m.debug_fetch("loss_feat", (fh, fw, 512))[0]       # (the record of the call names the map it ran on)
    finally:
        m.ctx.close()
    assert np.abs(fused).max() > 0 and x4.shape == (128, h4, w4)
    assert np.array_equal(_bits(kept), _bits(np.ascontiguousarray(fused.transpose(2, 0, 1))))
    assert np.array_equal(_bits(again), _bits(fused))
    assert all(np.isfinite(res["conv_w%d" % i]).all() for i in ops.CNN_GRAD_CONVS)


def test_forward_backward_cnn_is_forward_backward_plus_the_chain(setup):
    from densecap_amd import ops
    W, img, gt, lab, grads, _ = setup
    m = _model(W)
    try:
        res = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, cnn=True, **FORCED, **LOSS)
        x4, feat = ops.cnn_kept(m.ctx, H, WD)
        chain = ops.cnn_grad(m.ctx, x4, res["feat"], want_x=False)
        twice = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, cnn=True, **FORCED, **LOSS)
        plain = m.forward_backward(img, gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
    finally:
        m.ctx.close()
    assert sorted(set(res) - set(grads)) == sorted(ops.CNN_GRAD_KEYS) and not set(grads) - set(res)
    for k in grads:                                                      # (grads: dc_forward_backward on a context of its own)
        assert _same(grads[k], res[k]), k
        assert _same(grads[k], plain[k]), k
    for k in ops.CNN_GRAD_KEYS:
        assert np.array_equal(_bits(res[k]), _bits(chain[k])), k
        assert np.array_equal(_bits(res[k]), _bits(twice[k])), k
        assert np.abs(res[k]).max() > 0, k
    assert sorted(plain) == sorted(grads)


# ---- dc_train_set_cnn -----------------------------------------------------------------------------------------------------------
CNN = tuple(range(4, 13))
# steps large enough that a stale derived operand shows, small enough that three steps on the nine convolutions (Adam moves every
# weight by about the learning rate, against He-scaled weights of 0.02 .. 0.03) leave the forced sampler ranks inside the lists
STEP = dict(learning_rate=1e-4, weight_decay=1e-2)
OPTS = dict(R.DEFAULTS, **STEP)


def _grads_cnn(W, img, gt, lab):
    """dc_forward_backward_cnn's result on a context of its own loaded with W"""
    m = _model(W)
    try:
        return m.forward_backward(img, gt, lab, box_reg_decay=DECAY, cnn=True, **FORCED, **LOSS)
    finally:
        m.ctx.close()


def _cnn_rule_step(Wk, grads, mom, t, **opts):
    """the restatement on the 18 CNN tensors: {("w" | "b", i): new array}; grads None: the zero gradient of mode 1"""
    out = {}
    for i in CNN:
        for kind, key in (("w", "conv_w"), ("b", "conv_b")):
            p = _np(Wk[key][i])
            g = np.zeros(p.size, F32) if grads is None else _np(grads["%s%d" % (key, i)]).reshape(-1)
            m, v = mom.get((kind, i), (np.zeros(p.size, F32), np.zeros(p.size, F32)))
            pn, mn, vn = R.adam_step32(p.reshape(-1), g, m, v, t, **opts)
            out[(kind, i)] = pn.reshape(p.shape)
            mom[(kind, i)] = (mn, vn)
    return out


def _assert_cnn(got, want, W0, what):
    for (kind, i), a in want.items():
        b = got["conv_w" if kind == "w" else "conv_b"][i]
        bad = np.flatnonzero(_bits(_np(a).reshape(-1)) != _bits(_np(b).reshape(-1)))
        assert bad.size == 0, (what, kind, i, int(bad.size), int(bad[0]))
    for i in range(4):                                                    # conv1_1 .. conv2_2 are never trained
        assert np.array_equal(_bits(got["conv_w"][i]), _bits(_np(W0["conv_w"][i]))), (what, i)
        assert np.array_equal(_bits(got["conv_b"][i]), _bits(_np(W0["conv_b"][i]))), (what, i)


def _cnn_t(m):
    return int(m.debug_fetch("train_cnn_t", (1,), np.int32)[0][0])


def test_mode_0_is_the_step_of_a_context_that_never_heard_of_it(setup):
    W, img, gt, lab, _g, _w = setup
    got = []
    for tell in (False, True):
        m = _model(W)
        try:
            m.train_begin(**STEP)
            for _ in range(3):
                if tell:
                    m.train_set_cnn(0)
                _step(m, img, gt, lab)
            assert _cnn_t(m) == -1
            got.append(m.get_weights())
            m.train_end()
        finally:
            m.ctx.close()
    _assert_weights(got[1], got[0], "mode 0")
    for i in range(13):
        assert np.array_equal(_bits(got[1]["conv_w"][i]), _bits(_np(W["conv_w"][i]))), i
        assert np.array_equal(_bits(got[1]["conv_b"][i]), _bits(_np(W["conv_b"][i]))), i


def test_mode_1_then_mode_2_twice_is_the_rule_with_the_cnns_own_t(setup):
    """One step in mode 0 first, so that the 21 tensors' t (2, 3, 4) and the CNN's (1, 2, 3) differ.  Teacher-forced: every step's
    gradients come from a fresh context loaded with the weights the step before left."""
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    try:
        m.train_begin(**STEP)
        Wk, mom, cmom, ct = W, {}, {}, 0
        for t, mode in ((1, 0), (2, 1), (3, 2), (4, 2)):
            grads = _grads_cnn(Wk, img, gt, lab)
            want = _rule_step(Wk, grads, mom, t, **OPTS)
            if mode:
                ct += 1
                cwant = _cnn_rule_step(Wk, grads if mode == 2 else None, cmom, ct, **OPTS)
            else:
                cwant = {(kd, i): _np(Wk["conv_w" if kd == "w" else "conv_b"][i]) for i in CNN for kd in "wb"}
            m.train_set_cnn(mode)
            res = _step(m, img, gt, lab)
            assert _bits(np.float64(res["total_loss"])) == _bits(np.float64(grads["total_loss"])), t
            Wk = m.get_weights()
            _assert_weights(Wk, want, "step %d" % t)                      # the 21 others: the rule on the same gradients, as in mode 0
            _assert_cnn(Wk, cwant, W, "step %d, mode %d" % (t, mode))
            assert _cnn_t(m) == (ct if ct else -1) and int(m.debug_fetch("train_t", (1,), np.int32)[0][0]) == t
        assert not np.array_equal(_bits(Wk["conv_w"][4]), _bits(_np(W["conv_w"][4])))
        m.train_end()
        _assert_cnn(m.get_weights(), cwant, W, "after end")
    finally:
        m.ctx.close()


def test_mode_1_without_decay_moves_nothing_but_t(setup):
    W, img, gt, lab, _g, _w = setup
    opts = dict(OPTS, weight_decay=0.0)
    m = _model(W)
    try:
        m.train_begin(learning_rate=STEP["learning_rate"], weight_decay=0.0)
        m.train_set_cnn(1)
        _step(m, img, gt, lab)
        W1 = m.get_weights()
        for i in range(13):
            assert np.array_equal(_bits(W1["conv_w"][i]), _bits(_np(W["conv_w"][i]))), i
            assert np.array_equal(_bits(W1["conv_b"][i]), _bits(_np(W["conv_b"][i]))), i
        assert _cnn_t(m) == 1
        grads = _grads_cnn(W1, img, gt, lab)
        m.train_set_cnn(2)
        _step(m, img, gt, lab)
        W2 = m.get_weights()
    finally:
        m.ctx.close()
    _assert_cnn(W2, _cnn_rule_step(W1, grads, {}, 2, **opts), W, "t = 2 after the empty step")       # (its moments stayed zero)
    t1 = _cnn_rule_step(W1, grads, {}, 1, **opts)
    assert not np.array_equal(_bits(t1[("w", 12)]), _bits(W2["conv_w"][12]))                          # t = 1 would show


def test_call_order_and_a_refused_step(setup):
    from densecap_amd._lib import DenseCapError
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    try:
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_set_cnn(2)                                            # before begin
        m.train_begin(**STEP)
        for bad in (-1, 3):
            with pytest.raises(DenseCapError, match=r"\(-1\)"):
                m.train_set_cnn(bad)
        m.train_set_cnn(2)
        bad_gt = gt.copy(); bad_gt[1, 2] = 0.0
        with pytest.raises(DenseCapError):
            m.train_step(img, bad_gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
        assert _cnn_t(m) == 0 and int(m.debug_fetch("train_t", (1,), np.int32)[0][0]) == 0
        got = m.get_weights()
        _assert_weights(got, W, "after a refused step")
        for i in range(13):
            assert np.array_equal(_bits(got["conv_w"][i]), _bits(_np(W["conv_w"][i]))), i
        m.train_end()
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_set_cnn(0)                                            # after end
    finally:
        m.ctx.close()


def _observe(m, img, gt, lab):
    """tests/test_gpu_train_step.py's observation with the sampler drawing its own rows: once the convolutions have moved, the
    positive candidates are other boxes and ranks forced for the loaded weights need not exist"""
    q = np.ascontiguousarray(lab[:3], dtype=np.int32)
    return dict(forward_test=m.forward_raw(img), forward_losses=m.forward_losses(img, gt, lab, **LOSS),
                scoreCaptions=m.scoreCaptions(img, q), sampleCaptions=m.sampleCaptions(img, 2, temperature=0.9, seed=5))


@pytest.mark.parametrize("cfg", [_cfg_default, _cfg_math_before, _cfg_math_after, _cfg_graph],
                         ids=["default", "math_mode_before", "math_mode_after", "graph_replay"])
def test_trained_convolutions_are_refreshed(setup, cfg):
    """tests/test_gpu_train_step.py::test_derived_operands_are_refreshed with the CNN in the steps: the trained context computes
    what a fresh one loaded with its exported weights computes, in both math modes and through a graph captured before."""
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    try:
        m.setTestArgs(num_proposals=LOSS["batch_size"])
        cfg(m, "before")
        before = [m.forward_raw(img) for _ in range(3)]
        m.train_begin(**STEP)
        for mode in (1, 2, 2):
            m.train_set_cnn(mode)
            _step(m, img, gt, lab)
        m.train_end()
        cfg(m, "after")
        captures0 = int(m.debug_fetch("graph_captures", (1,), np.int32)[0][0])
        got = _observe(m, img, gt, lab)
        if cfg is _cfg_graph:
            assert int(m.debug_fetch("graph_captures", (1,), np.int32)[0][0]) == captures0
        Wt = m.get_weights()
    finally:
        m.ctx.close()
    assert not np.array_equal(_bits(Wt["conv_w"][6]), _bits(_np(W["conv_w"][6])))
    f = _model(Wt)
    try:
        f.setTestArgs(num_proposals=LOSS["batch_size"])
        cfg(f, "fresh")
        want = _observe(f, img, gt, lab)
    finally:
        f.ctx.close()
    _same_tree(got, want, cfg.__name__)
    assert not np.array_equal(got["forward_test"][1], before[0][1])


def test_save_checkpoint_round_trips_the_trained_convolutions(setup, tmp_path):
    from densecap_amd import t7
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    try:
        m.train_begin(**STEP)
        m.train_set_cnn(2)
        _step(m, img, gt, lab)
        path = str(tmp_path / "ckpt.t7")
        m.save_checkpoint(path)
        got = m.get_weights()
    finally:
        m.ctx.close()
    back = t7.weights_from_checkpoint(t7.load(path))
    _assert_weights(back, got, "t7 round trip")
    for i in range(13):
        assert np.array_equal(_bits(_np(back["conv_w"][i])), _bits(got["conv_w"][i])), i
        assert np.array_equal(_bits(_np(back["conv_b"][i])), _bits(got["conv_b"][i])), i
    assert not np.array_equal(_bits(got["conv_w"][9]), _bits(_np(W["conv_w"][9])))


def test_tool_finetunes_the_cnn_after_iteration_1(tmp_path, capsys):
    """-synthetic_weights 1 -finetune_cnn_after 1 -max_iters 3 on a two-image fixture: iteration 1 leaves the CNN alone, 2 is the
    decay-only step, 3 the full one; the checkpoint's conv3_1 has moved, its conv2_2 has not."""
    import json
    from PIL import Image
    from densecap_amd import hdf5_min as Hd, t7, train
    from densecap_amd.weights import make_synthetic_weights
    rng = np.random.default_rng(5)
    nimg, per, T = 2, 3, 15
    for i in range(nimg):
        Image.fromarray(rng.integers(0, 255, (96, 128, 3)).astype(np.uint8)).save(tmp_path / ("%d.png" % i))
    boxes = np.stack([rng.uniform(30, 100, nimg * per), rng.uniform(25, 70, nimg * per), rng.uniform(20, 60, nimg * per),
                      rng.uniform(20, 50, nimg * per)], 1).astype(F32)
    labels = np.zeros((nimg * per, T), np.int32)
    for r in range(len(labels)):
        n = int(rng.integers(1, T + 1))
        labels[r, :n] = rng.integers(1, 1000, n)
    first = np.arange(nimg, dtype=np.int32) * per + 1
    Hd.write_hdf5(str(tmp_path / "vg.h5"), dict(boxes=boxes, labels=labels, img_to_first_box=first, img_to_last_box=first + per - 1,
                                                split=np.zeros(nimg, np.int32)))
    json.dump({"idx_to_filename": {str(i + 1): "%d.png" % i for i in range(nimg)}}, open(tmp_path / "vg.json", "w"))
    out = str(tmp_path / "out.t7")
    rc = train.main(["-synthetic_weights", "1", "-finetune_cnn_after", "1", "-max_iters", "3", "-data_h5", str(tmp_path / "vg.h5"),
                     "-data_json", str(tmp_path / "vg.json"), "-image_dir", str(tmp_path), "-image_size", "128",
                     "-sampler_batch_size", "16", "-learning_rate", "1e-4", "-losses_log_every", "1", "-checkpoint_path", out])
    assert rc == 0
    assert "iter 3:" in capsys.readouterr().out
    back = t7.weights_from_checkpoint(t7.load(out))
    W = make_synthetic_weights()
    assert not np.array_equal(_bits(_np(back["conv_w"][4])), _bits(_np(W["conv_w"][4])))
    assert np.array_equal(_bits(_np(back["conv_w"][3])), _bits(_np(W["conv_w"][3])))
    assert not np.array_equal(_bits(_np(back["fc7_w"])), _bits(_np(W["fc7_w"])))
