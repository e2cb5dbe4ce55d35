"""Adam's state out and in (dc_train_get_state / dc_train_set_state; docs/SEMANTICS.md, "Training step") on
tests/test_gpu_train_step.py's tiny setup: the moments after one step from zero are the rule's on dc_forward_backward's gradients
in checkpoint layouts, bit for bit (which pins fc6's permutation, the split of the fused heads and the lm_out_w rows); a context
resumed from exported weights and state continues bit for bit, with the CNN's own step count and with clipping on; get -> set ->
get is the identity; the refusals, each with its code and without effect; the .npz file."""
import ctypes as C

import numpy as np
import pytest

from tests import optim_rules as R
from tests.test_gpu_train_step import DECAY, FORCED, LOSS, _assert_weights, _bits, _model, _np, setup  # noqa: F401 (setup: a fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32


def _step(m, img, gt, lab, seed):
    return m.train_step(img, gt, lab, box_reg_decay=DECAY, **FORCED, **dict(LOSS, seed=seed))


def _assert_state(got, want, what):
    assert got["t"] == want["t"] and got["cnn_t"] == want["cnn_t"], (what, got["t"], got["cnn_t"], want["t"], want["cnn_t"])
    for mom in ("m", "v"):
        assert sorted(got[mom]) == sorted(want[mom]), (what, mom)
        for k in want[mom]:
            a, b = _bits(_np(got[mom][k]).reshape(-1)), _bits(_np(want[mom][k]).reshape(-1))
            bad = np.flatnonzero(a != b)
            assert got[mom][k].shape == want[mom][k].shape and bad.size == 0, (what, mom, k, int(bad.size))


def test_moments_after_one_step_are_the_rule_in_checkpoint_layouts(setup):
    from densecap_amd.ops import WEIGHT_KEYS
    W, img, gt, lab, grads, _want = setup
    m = _model(W)
    try:
        m.train_begin(weight_decay=0.0)
        zero = m.train_state()
        m.train_step(img, gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
        st = m.train_state()
    finally:
        m.ctx.close()
    assert zero["t"] == 0 and zero["cnn_t"] == 0 and sorted(zero["m"]) == sorted(WEIGHT_KEYS)
    assert all(not a.any() for mom in "mv" for a in zero[mom].values())
    assert st["t"] == 1 and st["cnn_t"] == 0
    _b1, c1, _b2, c2, _eps, _wd, _ns = R.scalars32(1, **dict(R.DEFAULTS, weight_decay=0.0))
    assert c1 == F32(1.0 - 0.9)
    for k in WEIGHT_KEYS:
        g = _np(grads[k])
        z = np.zeros(g.size, F32)
        _p, wm, wv = R.adam_step32(z, g.reshape(-1), z, z, 1, **dict(R.DEFAULTS, weight_decay=0.0))
        assert st["m"][k].shape == g.shape and st["v"][k].shape == g.shape, k
        assert np.array_equal(_bits(st["m"][k].reshape(-1)), _bits(wm)), k
        assert np.array_equal(_bits(st["v"][k].reshape(-1)), _bits(wv)), k
        assert np.array_equal(st["m"][k], c1 * g) and np.array_equal(st["v"][k], (c2 * g) * g), k      # (the same but for a zero's sign)
        assert np.abs(st["m"][k]).max() > 0, k


@pytest.mark.parametrize("variant", ["plain", "cnn", "clip"])
def test_a_resumed_context_continues_bit_for_bit(setup, variant):
    """A: two steps, export, two more.  B: a fresh context loaded with A's exported weights and state, the same two more."""
    W, img, gt, lab, _g, _w = setup
    opts = dict(learning_rate=1e-4, weight_decay=1e-2)

    def configure(m, it):
        if variant == "cnn":
            m.train_set_cnn(0 if it == 1 else 2)                  # A's first step leaves the CNN alone: t and cnn_t differ
        if variant == "clip":
            m.train_set_grad_clip(0.05)

    a = _model(W)
    try:
        a.train_begin(**opts)
        for it in (1, 2):
            configure(a, it)
            _step(a, img, gt, lab, seed=it)
        Wk, state = a.get_weights(), a.train_state()
        assert state["t"] == 2 and state["cnn_t"] == (1 if variant == "cnn" else 0)
        assert ("conv_w4" in state["m"]) == (variant == "cnn")
        res_a = []
        for it in (3, 4):
            configure(a, it)
            res_a.append(_step(a, img, gt, lab, seed=it))
        Wa, sa = a.get_weights(), a.train_state()
    finally:
        a.ctx.close()
    b = _model(Wk)
    try:
        b.train_begin(**opts)
        b.train_load_state(state)
        _assert_state(b.train_state(), state, "straight after the load")
        res_b = []
        for it in (3, 4):
            configure(b, it)
            res_b.append(_step(b, img, gt, lab, seed=it))
        Wb, sb = b.get_weights(), b.train_state()
    finally:
        b.ctx.close()
    for ra, rb in zip(res_a, res_b):
        assert sorted(ra) == sorted(rb)
        for k in ("total_loss", "grad_norm", "grad_scale"):
            if k in ra:
                assert ra[k] == rb[k], k
    if variant == "clip":
        assert res_a[-1]["grad_scale"] < 1.0
    _assert_weights(Wb, Wa, variant)
    for i in range(13):
        assert np.array_equal(_bits(Wb["conv_w"][i]), _bits(Wa["conv_w"][i])) and np.array_equal(_bits(Wb["conv_b"][i]), _bits(Wa["conv_b"][i])), i
    _assert_state(sb, sa, variant)
    assert sa["t"] == 4 and sa["cnn_t"] == (3 if variant == "cnn" else 0)
    assert not np.array_equal(_bits(Wa["fc7_w"]), _bits(Wk["fc7_w"]))
    if variant == "cnn":
        assert not np.array_equal(_bits(Wa["conv_w"][8]), _bits(Wk["conv_w"][8]))
    # a context that restarts Adam from zero is a different run: what the state is for
    c = _model(Wk)
    try:
        c.train_begin(**opts)
        configure(c, 3)
        _step(c, img, gt, lab, seed=3)
        assert not np.array_equal(_bits(c.get_weights()["fc7_w"]), _bits(Wa["fc7_w"]))
    finally:
        c.ctx.close()


def test_get_set_get_is_the_identity_and_the_file_round_trips(setup, tmp_path):
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    try:
        m.train_begin()
        m.train_set_cnn(2)
        for it in (1, 2):
            _step(m, img, gt, lab, seed=it)
        first = m.train_state()
        m.train_load_state(first)
        _assert_state(m.train_state(), first, "get, set, get")
        path = str(tmp_path / "ckpt.optim.npz")
        m.save_train_state(path)
        m.train_end()
        m.train_begin()                                          # zero moments again
        assert m.load_train_state(path) == (2, 2)
        _assert_state(m.train_state(), first, "through the file")
        with np.load(path) as z:
            assert sorted(z.files) == sorted(["t", "cnn_t"] + ["%s/%s" % (mom, k) for mom in "mv" for k in first["m"]])
    finally:
        m.ctx.close()


def test_refusals_each_with_its_code_and_without_effect(setup):
    from densecap_amd import ops
    W, img, gt, lab, _g, _w = setup
    m = _model(W)
    h, lib = m.ctx.h, m.lib
    t, ct = C.c_int(-7), C.c_int(-7)

    def structs(state, cnn):
        keep = {mom: {k: np.ascontiguousarray(a, dtype=F32) for k, a in state[mom].items()} for mom in "mv"}
        return ops._state_struct(keep["m"], cnn), ops._state_struct(keep["v"], cnn), keep

    try:
        shapes = m._weight_shapes
        blank = {mom: {k: np.zeros(s, F32) for k, s in ops._state_shapes(shapes, True).items()} for mom in "mv"}
        wm, wv, _k0 = structs(blank, False)
        assert lib.dc_train_get_state(h, C.byref(wm), C.byref(wv), C.byref(t), C.byref(ct)) == -3        # before begin
        assert lib.dc_train_set_state(h, C.byref(wm), C.byref(wv), 0, 0) == -3
        m.train_begin(learning_rate=1e-4)
        _step(m, img, gt, lab, seed=1)
        good = m.train_state()
        # ---- get ----
        assert lib.dc_train_get_state(h, None, None, C.byref(t), C.byref(ct)) == 0 and (t.value, ct.value) == (1, 0)
        cm, cv, _k1 = structs(blank, True)
        assert lib.dc_train_get_state(h, C.byref(cm), C.byref(cv), None, None) == -3                      # the CNN has no state yet
        for field, i in (("conv_w", 0), ("conv_b", 3)):
            wm, wv, _k2 = structs(blank, False)
            getattr(wm, field)[i] = blank["m"]["fc7_b"].ctypes.data_as(ops._lib.c_float_p)
            assert lib.dc_train_get_state(h, C.byref(wm), C.byref(wv), None, None) == -1
        wm, wv, _k3 = structs(blank, False)
        wv.anchors = blank["v"]["fc7_b"].ctypes.data_as(ops._lib.c_float_p)
        assert lib.dc_train_get_state(h, C.byref(wm), C.byref(wv), None, None) == -1
        wm, wv, part = structs(blank, False)                                                               # a null pointer is skipped
        part["m"]["fc7_b"][:] = 9.0
        wm.fc7_b = None
        assert lib.dc_train_get_state(h, C.byref(wm), None, None, None) == 0
        assert (part["m"]["fc7_b"] == 9.0).all() and np.array_equal(_bits(part["m"]["fc6_b"]), _bits(good["m"]["fc6_b"]))
        # ---- set: every breach is -1 and changes nothing ----
        other = {mom: {k: a + F32(1.0) for k, a in good[mom].items()} for mom in "mv"}
        for breach in ("null_m", "null_v", "no_v", "t", "cnn_t_sign", "cnn_t_without_cnn", "cnn_partial", "cnn_one_side", "conv0", "anchors"):
            full = {mom: dict(blank[mom], **other[mom]) for mom in "mv"}
            cnn = breach in ("cnn_partial", "cnn_one_side")
            wm, wv, _k4 = structs(full, cnn)
            args = [C.byref(wm), C.byref(wv), 5, 0]
            if breach == "null_m":
                wm.lm_out_w = None
            elif breach == "null_v":
                wv.rpn_conv_b = None
            elif breach == "no_v":
                args[1] = None
            elif breach == "t":
                args[2] = -1
            elif breach == "cnn_t_sign":
                args[3] = -1
            elif breach == "cnn_t_without_cnn":
                args[3] = 2
            elif breach == "cnn_partial":
                wm.conv_b[7] = None; wv.conv_b[7] = None
            elif breach == "cnn_one_side":
                for i in range(4, 13):
                    wv.conv_w[i] = None; wv.conv_b[i] = None
            elif breach == "conv0":
                wm.conv_w[0] = full["m"]["fc7_b"].ctypes.data_as(ops._lib.c_float_p)
            elif breach == "anchors":
                wm.anchors = full["m"]["fc7_b"].ctypes.data_as(ops._lib.c_float_p)
            assert lib.dc_train_set_state(h, *args) == -1, breach
            now = m.train_state()
            assert "conv_w4" not in now["m"], breach                                                       # no CNN state was made
            assert now["t"] == 1 and now["cnn_t"] == 0, breach
            for mom in "mv":
                for k in good[mom]:
                    assert np.array_equal(_bits(now[mom][k]), _bits(good[mom][k])), (breach, mom, k)
        # ---- set with the CNN's 18: the state is made, the mode stays 0 ----
        full = {mom: dict(blank[mom], **other[mom]) for mom in "mv"}
        for mom in "mv":
            full[mom]["conv_b12"] = full[mom]["conv_b12"] + F32(0.5)
        wm, wv, _k5 = structs(full, True)
        assert lib.dc_train_set_state(h, C.byref(wm), C.byref(wv), 7, 3) == 0
        now = m.train_state()
        assert (now["t"], now["cnn_t"]) == (7, 3) and (now["m"]["conv_b12"] == 0.5).all() and not now["v"]["conv_w4"].any()
        assert np.array_equal(_bits(now["m"]["fc6_w"]), _bits(other["m"]["fc6_w"]))
        before = m.get_weights()
        _step(m, img, gt, lab, seed=2)                                                                     # mode 0: the CNN stays
        after = m.get_weights()
        assert all(np.array_equal(_bits(after["conv_w"][i]), _bits(before["conv_w"][i])) for i in range(13))
        assert m.train_state()["cnn_t"] == 3 and m.train_state()["t"] == 8
    finally:
        m.ctx.close()
