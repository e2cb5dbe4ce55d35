"""dc_train_step end to end (docs/SEMANTICS.md, "Training step") on a 96 x 128 image at the "minimal" dimensions of
tests/test_gpu_dims.py with forced sampler lists: the weights after a step are the float32 restatement of tests/optim_rules.py
applied to dc_forward_backward's gradients from a second context, bit for bit, for all 21 tensors; over three steps too, each
against a fresh context loaded with the step before's exported weights (a stale transposed or flipped copy in the backward would
show there); the same at the default dimensions; dc_get_weights gives back what was loaded; call order and refusals; every
operand the library derives from a weight is refreshed (a trained context computes what a fresh one loaded from its exported
weights computes, in four configurations); save_checkpoint round-trips."""
import numpy as np
import pytest

from tests import lm_grad_rules as G
from tests import optim_rules as R

pytestmark = pytest.mark.gpu

F32 = np.float32
H, WD, MAP = 96, 128, (6, 8)
LOSS = dict(batch_size=16, seed=3, remove_outbounds=0)
FORCED = dict(forced_pos=[1, 0], forced_neg=[2, 0, 2, 1])
DECAY = 5e-5
LOSS_KEYS = ("mid_objectness_loss", "mid_box_reg_loss", "end_objectness_loss", "end_box_reg_loss", "captioning_loss", "total_loss")
COUNTS = ("num_pos", "num_neg", "total_pos", "total_neg", "masked_mid", "masked_end", "flags")
FAST = dict(learning_rate=1e-3, weight_decay=1e-2)          # steps large enough that a stale derived operand changes results


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _np(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=F32)


def _model(W):
    from densecap_amd import DenseCapModel
    return DenseCapModel(W, device=0)


def _grads(W, img, gt, lab):
    """dc_forward_backward's result on a context of its own loaded with W"""
    m = _model(W)
    try:
        return m.forward_backward(img, gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
    finally:
        m.ctx.close()


def _rule_step(Wk, grads, mom, t, **opts):
    """the restatement on all 21 tensors: new {name: array in Wk's shape}; mom ({name: (m, v)}) is updated in place"""
    from densecap_amd.ops import WEIGHT_KEYS
    out = {}
    for k in WEIGHT_KEYS:
        p = _np(Wk[k])
        m, v = mom.get(k, (np.zeros(p.size, F32), np.zeros(p.size, F32)))
        pn, mn, vn = R.adam_step32(p.reshape(-1), _np(grads[k]).reshape(-1), m, v, t, **opts)
        out[k] = pn.reshape(p.shape)
        mom[k] = (mn, vn)
    return out


def _assert_weights(got, want, what):
    from densecap_amd.ops import WEIGHT_KEYS
    for k in WEIGHT_KEYS:
        a, b = _bits(_np(got[k]).reshape(-1)), _bits(_np(want[k]).reshape(-1))
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]))


def _assert_cnn_unchanged(got, W):
    for i in range(13):
        assert np.array_equal(_bits(got["conv_w"][i]), _bits(_np(W["conv_w"][i]))), i
        assert np.array_equal(_bits(got["conv_b"][i]), _bits(_np(W["conv_b"][i]))), i
    assert np.array_equal(_bits(got["anchors"]), _bits(_np(W["anchors"])))


def _make_inputs(W, img_seed=6, model=None):
    """image, ground truth made of RPN boxes (as tests/test_gpu_forward_backward.py makes its own) and labels; on `model`, or
    on a context of its own"""
    from densecap_amd.weights import make_synthetic_image
    m = model or _model(W)
    try:
        img = make_synthetic_image(H, WD, img_seed)
        A = m.num_anchors * MAP[0] * MAP[1]
        m.forward_losses(img, np.array([[60, 50, 60, 40]], F32), np.ones((1, 1), np.int32), **LOSS)
        boxes = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
        big = np.nonzero((boxes[:, 2] > 20) & (boxes[:, 3] > 20))[0]
        pick = big[np.linspace(0, len(big) - 1, 4).astype(int)]
        gt = (boxes[pick] + np.array([[1, -1, 0, 0], [2, 1, 0, 0], [-1, 2, 0, 0], [0, 1, 1, 0]], F32)).astype(F32)
        lab = G.draw_labels(4, m.seq_length, m.vocab_size, np.random.default_rng(11))
        return img, gt, lab
    finally:
        if model is None:
            m.ctx.close()


@pytest.fixture(scope="module")
def setup():
    """weights, inputs, and the reference of ONE step with train_opts.lua's defaults: dc_forward_backward's result on a second
    context and the restatement's weights (computed once, shared, never changed)"""
    from tests.test_gpu_dims import set_weights
    W = set_weights("minimal")
    img, gt, lab = _make_inputs(W)
    grads = _grads(W, img, gt, lab)
    want = _rule_step(W, grads, {}, 1, **R.DEFAULTS)
    return W, img, gt, lab, grads, want


def _step(m, img, gt, lab):
    return m.train_step(img, gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_one_step_is_the_rule_on_forward_backwards_gradients(setup):
    W, img, gt, lab, grads, want = setup
    m = _model(W)
    try:
        m.train_begin(weight_decay=1e-6)
        res = _step(m, img, gt, lab)
        got = m.get_weights()
        m.train_end()
    finally:
        m.ctx.close()
    assert res["num_pos"] == 2 and res["num_neg"] == 4
    for k in LOSS_KEYS:
        assert _bits(np.float64(res[k])) == _bits(np.float64(grads[k])), k
    for k in COUNTS:
        assert res[k] == grads[k], k
    _assert_weights(got, want, "one step")
    _assert_cnn_unchanged(got, W)
    moved = [k for k in want if not np.array_equal(_bits(_np(want[k])), _bits(_np(W[k])))]
    assert len(moved) == 21, sorted(set(want) - set(moved))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def test_three_steps_teacher_forced(setup):
    W, img, gt, lab, _grads0, _want = setup
    m = _model(W)
    try:
        m.train_begin(**FAST)
        Wk, mom = W, {}
        for t in (1, 2, 3):
            grads = _grads(Wk, img, gt, lab)                 # a fresh context loaded with step t-1's exported weights
            want = _rule_step(Wk, grads, mom, t, **dict(R.DEFAULTS, **FAST))
            res = _step(m, img, gt, lab)
            assert _bits(np.float64(res["total_loss"])) == _bits(np.float64(grads["total_loss"])), t
            Wk = m.get_weights()
            _assert_weights(Wk, want, "step %d" % t)
        m.train_end()
    finally:
        m.ctx.close()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_one_step_at_the_default_dimensions():
    """fc6 at 25088 x 4096, updated in the engine's input order; a small vocabulary, as tests/test_gpu_recog_grad.py chooses"""
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    m0 = _model(W)                                          # the second context: the inputs and dc_forward_backward's gradients
    try:
        img, gt, lab = _make_inputs(W, img_seed=4, model=m0)
        grads = m0.forward_backward(img, gt, lab, box_reg_decay=DECAY, **FORCED, **LOSS)
    finally:
        m0.ctx.close()
    m = _model(W)
    try:
        m.train_begin(weight_decay=1e-6)
        res = _step(m, img, gt, lab)
        got = m.get_weights(conv=False)
    finally:
        m.ctx.close()
    for k in LOSS_KEYS:
        assert _bits(np.float64(res[k])) == _bits(np.float64(grads[k])), k
    _assert_weights(got, _rule_step(W, grads, {}, 1, **R.DEFAULTS), "default dimensions")
    assert not np.array_equal(got["fc6_w"], _np(W["fc6_w"]))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_get_weights_returns_what_was_loaded(setup):
    W = setup[0]
    m = _model(W)
    try:
        got = m.get_weights()
        _assert_weights(got, W, "after load"); _assert_cnn_unchanged(got, W)
        for k in ("rpn_conv_w", "fc6_w", "lstm_w"):
            assert got[k].shape == tuple(_np(W[k]).shape)
        m.train_begin()
        got = m.get_weights()
        _assert_weights(got, W, "after begin"); _assert_cnn_unchanged(got, W)
    finally:
        m.ctx.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_call_order_and_a_refused_step_changes_nothing(setup):
    from densecap_amd._lib import DenseCapError
    W, img, gt, lab, _grads0, want = setup
    m = _model(W)
    try:
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            _step(m, img, gt, lab)                            # before begin
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_end()
        with pytest.raises(DenseCapError, match=r"\(-1\)"):
            m.train_begin(beta1=1.0)                          # refused: still not training
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            _step(m, img, gt, lab)
        m.train_begin(weight_decay=1e-6)
        with pytest.raises(DenseCapError, match=r"\(-3\)"):
            m.train_begin()                                   # twice
        bad_gt = gt.copy(); bad_gt[1, 2] = 0.0                # a box without width
        bad_lab = lab.copy(); bad_lab[0, 0] = m.vocab_size + 5
        for args, kw in (((img, bad_gt, lab), {}), ((img, gt, bad_lab), {}), ((img, gt, lab), dict(box_reg_decay=-1.0)),
                         ((img, gt, lab), dict(forced_pos=[10 ** 6]))):
            with pytest.raises(DenseCapError):
                m.train_step(*args, **dict(dict(box_reg_decay=DECAY, **FORCED, **LOSS), **kw))
            assert m.debug_fetch("train_t", (1,), np.int32)[0][0] == 0
        _assert_weights(m.get_weights(), W, "after refused steps")
        _step(m, img, gt, lab)                                # the good step of a context that never saw a bad call (setup's)
        assert m.debug_fetch("train_t", (1,), np.int32)[0][0] == 1
        _assert_weights(m.get_weights(), want, "good step after refused ones")
        m.train_end()
        _assert_weights(m.get_weights(), want, "after end: the weights stay as trained")
    finally:
        m.ctx.close()


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], "%s[%s]" % (what, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    elif isinstance(a, float):
        assert _bits(np.float64(a)) == _bits(np.float64(b)), what
    else:
        assert a == b, what


def _observe(m, img, gt, lab):
    q = np.ascontiguousarray(lab[:3], dtype=np.int32)
    return dict(forward_test=m.forward_raw(img), forward_losses=m.forward_losses(img, gt, lab, **FORCED, **LOSS),
                scoreCaptions=m.scoreCaptions(img, q), sampleCaptions=m.sampleCaptions(img, 2, temperature=0.9, seed=5))


def _debug_set(m, name, v):
    from densecap_amd._lib import check
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, name.encode(), int(v)), "dc_debug_set(%s)" % name)


def _cfg_default(m, when):
    pass


def _cfg_screen(m, when):
    if when != "after":
        _debug_set(m, "decode_screen", 1)


def _cfg_math_before(m, when):
    if when != "after":
        m.setMathMode(1); _debug_set(m, "bf3_all", 1)        # every contraction takes the split-bf16 planes at these sizes


def _cfg_math_after(m, when):
    if when != "before":
        m.setMathMode(1); _debug_set(m, "bf3_all", 1)


def _cfg_graph(m, when):
    if when != "after":
        m.setLanes(1); m.setGraphReplay(True)


@pytest.mark.parametrize("cfg", [_cfg_default, _cfg_screen, _cfg_math_before, _cfg_math_after, _cfg_graph],
                         ids=["default", "decode_screen", "math_mode_before", "math_mode_after", "graph_replay"])
def test_derived_operands_are_refreshed(setup, cfg):
    """`when`: "before" = on the trained context before its steps, "after" = on it after them, "fresh" = on the fresh context"""
    W, img, gt, lab, _grads0, _want = setup
    m = _model(W)
    try:
        m.setTestArgs(num_proposals=LOSS["batch_size"])      # the lane's workspace then serves the steps as it is: a captured forward stays valid
        cfg(m, "before")
        before = [m.forward_raw(img) for _ in range(3)]       # (graph replay: eager, capture, replay)
        if cfg is _cfg_graph:
            assert m.debug_fetch("graph_captures", (1,), np.int32)[0][0] >= 1
        m.train_begin(**FAST)
        for _ in range(3):
            _step(m, img, gt, lab)
        m.train_end()
        cfg(m, "after")
        launches0 = int(m.debug_fetch("graph_launches", (1,), np.int32)[0][0])
        captures0 = int(m.debug_fetch("graph_captures", (1,), np.int32)[0][0])
        got = _observe(m, img, gt, lab)
        if cfg is _cfg_graph:                                 # the forward captured before the steps was replayed, not re-captured
            assert int(m.debug_fetch("graph_launches", (1,), np.int32)[0][0]) > launches0
            assert int(m.debug_fetch("graph_captures", (1,), np.int32)[0][0]) == captures0
        Wt = m.get_weights()
    finally:
        m.ctx.close()
    f = _model(Wt)
    try:
        f.setTestArgs(num_proposals=LOSS["batch_size"])
        cfg(f, "fresh")
        want = _observe(f, img, gt, lab)
    finally:
        f.ctx.close()
    _same(got, want, cfg.__name__)
    assert not np.array_equal(got["forward_test"][1], before[0][1]), "three steps did not move the objectness scores"


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
def test_save_checkpoint_round_trips(setup, tmp_path):
    from densecap_amd import t7
    W, img, gt, lab, _grads0, _want = setup
    m = _model(W)
    try:
        m.train_begin(**FAST)
        _step(m, img, gt, lab)
        path = str(tmp_path / "ckpt.t7")
        m.save_checkpoint(path)
        got = m.get_weights()
    finally:
        m.ctx.close()
    back = t7.weights_from_checkpoint(t7.load(path))
    _assert_weights(back, got, "t7 round trip")
    _assert_cnn_unchanged(back, got)
    assert int(back["vocab_size"]) == int(W["vocab_size"]) and int(back["seq_length"]) == int(W["seq_length"])
