"""dc_op_rpn_grad (docs/SEMANTICS.md, "RPN gradients") and its kernels alone (the hooks of include/densecap_debug_rpn.h) against
the float64 restatement of tests/rpn_grad_rules.py.

Every tensor is held to max|dev - ref64| <= REL * max|ref64| and the 2-D ones, per row, to tests/grad_bars.py's bar (8x the worst
row of the float32 CPU evaluation of the same rules, computed here): rpn_conv_w per output channel, feat per pixel, rpn_box_w and
rpn_score_w per row.  Worst observed ratios (MI355X): DESIGN.md §18."""
import ctypes as C

import numpy as np
import pytest

from tests import grad_bars as GB
from tests import rpn_grad_rules as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = F32(-7.25)
MAPS = {(6, 8): (96, 128), (5, 7): (80, 112)}      # feature map (h, w) -> an image (H, W) that gives it
# case -> (weights, map, num_pos, num_neg, box_reg_decay, draw_rpn_case's keywords)
CASES = {
    "minimal_no_pos": ("minimal", (6, 8), 0, 6, 5e-5, {}),
    "minimal_no_neg": ("minimal", (6, 8), 5, 0, 5e-5, {}),
    "minimal_corners": ("minimal", (6, 8), 5, 5, 5e-5, dict(corners=True)),
    "minimal_masked": ("minimal", (6, 8), 6, 7, 5e-5, dict(masked_rows=(0, 3), far_rows=(1,))),
    "minimal_dup_neg": ("minimal", (6, 8), 5, 8, 5e-5, dict(dup_neg=3)),
    "minimal_neg_on_pos": ("minimal", (6, 8), 5, 7, 5e-5, dict(neg_on_pos=2, masked_rows=(4,))),
    "minimal_dup_pos": ("minimal", (6, 8), 7, 5, 5e-5, dict(dup_pos=2, far_rows=(0,))),
    "minimal_no_droi": ("minimal", (6, 8), 5, 6, 5e-5, dict(with_droi=False, neg_on_pos=1)),
    "minimal_decay_0": ("minimal", (6, 8), 5, 6, 0.0, dict(dup_neg=1)),
    "minimal_decay_half": ("minimal", (6, 8), 5, 6, 0.5, dict(dup_neg=1, masked_rows=(0,))),
    "odd32_corners": ("odd32", (6, 8), 6, 6, 5e-5, dict(corners=True, far_rows=(1,))),
    "odd32_5x7": ("odd32", (5, 7), 9, 11, 5e-5, dict(dup_neg=2, neg_on_pos=1, dup_pos=1, masked_rows=(2,))),
    "default_6x8": ("default", (6, 8), 20, 30, 5e-5, dict(dup_neg=2, masked_rows=(0,), far_rows=(1,))),
    "default_1024": ("default", (6, 8), 200, 824, 5e-5, dict(dup_neg=448, masked_rows=(0,), far_rows=(1,))),
}
SEEDS = {"default_6x8": 600, "default_1024": 600}                         # cases whose default seed (500 + rank of the name) needs a redraw: the seed that does not
_models, _draws, _runs = {}, {}, {}


def _weights(name):
    from densecap_amd.weights import make_synthetic_weights
    from tests.test_gpu_dims import set_weights
    return make_synthetic_weights(seed=21, vocab_size=200, seq_length=15) if name == "default" else set_weights(name)


_wcache = {}


def draw(case):
    """(W, feat, pos_idx, pos_tgt, neg_idx, gt, droi, redraws) of a case: no GPU needed (tests/test_rpn_grad_rules_cpu.py calls it)."""
    if case not in _draws:
        name, (h, w), np_, nn_, _decay, kw = CASES[case]
        if name not in _wcache:
            _wcache[name] = _weights(name)
        seed = SEEDS.get(case, 500 + sorted(CASES).index(case))
        _draws[case] = (_wcache[name],) + R.draw_rpn_case(_wcache[name], h, w, np_, nn_, seed, **kw)
    return _draws[case]


def _model(name):
    if name not in _models:
        from densecap_amd import DenseCapModel
        if name not in _wcache:
            _wcache[name] = _weights(name)
        _models[name] = DenseCapModel(_wcache[name], device=0)
    return _models[name]


def _run(case):
    """(model, device result, float64 reference, float32 reference) of a case, computed once."""
    if case not in _runs:
        from densecap_amd import ops
        name, hw, _np, _nn, decay, _kw = CASES[case]
        W, feat, pi, pt, ni, gt, droi, _ = draw(case)
        m = _model(name)
        H, Wd = MAPS[hw]
        dev = ops.rpn_grad(m.ctx, feat, pi, pt, ni, gt, H, Wd, droi_boxes=droi, box_reg_decay=decay)
        _runs[case] = (m, dev, R.rpn_grad(W, feat, pi, pt, ni, gt, droi, decay), R.rpn_grad(W, feat, pi, pt, ni, gt, droi, decay, dtype="float32"))
    return _runs[case]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.ctx.close()
    _models.clear(); _runs.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def check(what, dev, ref64, ref32):
    figs, bad = [], []
    for k in R.RPN_TENSORS:
        assert dev[k].shape == ref64[k].shape, (k, dev[k].shape, ref64[k].shape)
        scale = float(np.abs(ref64[k]).max())
        err = float(np.abs(dev[k].astype(np.float64) - ref64[k]).max())
        assert np.isfinite(dev[k]).all(), (what, k)
        figs.append("%s %.2e" % (k, err / scale if scale > 0 else err))
        if err > R.REL * scale:
            bad.append((k, "max-norm", err / max(scale, 1e-300)))
        if k in R.RPN_ROW_TENSORS:
            bar = GB.FACTOR * GB.worst(GB.row_ratios(R.rpn_rows(k, ref32[k]), R.rpn_rows(k, ref64[k])))
            worst, rows = GB.check_rows(k + "_rows", R.rpn_rows(k, dev[k]), R.rpn_rows(k, ref64[k]), bar)
            figs.append("rows %.2e (bar %.2e)" % (worst, bar))
            if rows:
                bad.append((k, "rows, bar %.3e" % bar, rows))
    print("rpn_grad %s: " % what + ", ".join(figs))
    assert not bad, (what, bad)


@pytest.mark.parametrize("case", list(CASES))
def test_rpn_grad_matches_the_rules(case):
    m, dev, ref64, ref32 = _run(case)
    check(case, dev, ref64, ref32)
    for k in ("mid_objectness_loss", "mid_box_reg_loss"):
        assert abs(dev[k] - ref64[k]) <= 1e-6 * abs(ref64[k]), (k, dev[k], ref64[k])
    assert dev["masked_mid"] == ref64["masked_mid"] == len(CASES[case][5].get("masked_rows", ()))


@pytest.mark.parametrize("case", ["minimal_neg_on_pos", "odd32_5x7", "default_1024"])
def test_two_calls_give_the_same_bits(case):
    from densecap_amd import ops
    m, dev, _r64, _r32 = _run(case)
    name, hw, _np, _nn, decay, _kw = CASES[case]
    W, feat, pi, pt, ni, gt, droi, _ = draw(case)
    again = ops.rpn_grad(m.ctx, feat, pi, pt, ni, gt, *MAPS[hw], droi_boxes=droi, box_reg_decay=decay)
    for k in R.RPN_TENSORS:
        assert np.array_equal(_bits(dev[k]), _bits(again[k])), k
    assert (again["mid_objectness_loss"], again["mid_box_reg_loss"]) == (dev["mid_objectness_loss"], dev["mid_box_reg_loss"])


def test_decay_term_alone_stands_above_the_bar():
    """At box_reg_decay = 0.5 the dense term is not lost beside the criteria: leaving it out moves a tensor by more than REL."""
    W, feat, pi, pt, ni, gt, droi, _ = draw("minimal_decay_half")
    _m, dev, ref64, _r32 = _run("minimal_decay_half")
    without = R.rpn_grad(W, feat, pi, pt, ni, gt, droi, 0.5, variant="no_decay")
    assert max(np.abs(without[k] - ref64[k]).max() / np.abs(ref64[k]).max() for k in R.RPN_TENSORS) > 100 * R.REL


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------
def _tables(W, ref, h, w):
    """The forward's rows as float32 tables from the rules' float64 forward: trans, scores, anchors, boxes."""
    from tests import loss_rules as LR
    anc = R.anchor_rows(W, h, w)
    trans, scores = ref["rows"]
    return trans.astype(F32), scores.astype(F32), anc, LR.apply_box_transform(anc, trans).astype(F32)


def _rows(W, feat):
    import torch
    with torch.no_grad():
        _pre, _hid, trans, scores = R._forward(W, feat, torch.float64)
    return trans.numpy(), scores.numpy()


def _dheads_layout(dtrans, dscores, h, w, k):
    hw = h * w
    out = np.zeros((hw, 6 * k))
    for a in range(k):
        out[:, a * 4:a * 4 + 4] = dtrans[a * hw:(a + 1) * hw]
        out[:, 4 * k + 2 * a:4 * k + 2 * a + 2] = dscores[a * hw:(a + 1) * hw]
    return out


@pytest.mark.parametrize("case", ["minimal_neg_on_pos", "minimal_dup_pos", "minimal_masked", "odd32_5x7", "default_1024", "minimal_no_droi"])
def test_rpn_dheads_alone(case):
    from densecap_amd import ops
    name, (h, w), _np, _nn, decay, _kw = CASES[case]
    W, feat, pi, pt, ni, gt, droi, _ = draw(case)
    m, _dev, ref64, _r32 = _run(case)
    k = np.asarray(W["anchors"]).shape[1]
    ref = dict(ref64, rows=_rows(W, feat))
    trans, scores, anc, boxes = _tables(W, ref, h, w)
    got = ops.rpn_dheads(m.ctx, trans, scores, anc, boxes, h, w, k, pi, pt, ni, gt, droi, decay=decay)
    want = _dheads_layout(ref64["dheads"][0], ref64["dheads"][1], h, w, k)
    box_cols = np.arange(6 * k) < 4 * k
    for what, cols in (("box", box_cols), ("score", ~box_cols)):
        scale = np.abs(want[:, cols]).max()
        err = np.abs(got[:, cols] - want[:, cols]).max()
        print("rpn_dheads %s %s: %.2e" % (case, what, err / scale if scale else err))
        assert err <= R.REL * scale, (what, err, scale)
    assert np.array_equal(_bits(got), _bits(ops.rpn_dheads(m.ctx, trans, scores, anc, boxes, h, w, k, pi, pt, ni, gt, droi, decay=decay)))


def test_rpn_dheads_untouched_elements_are_plus_zero():
    """decay = 0 and no droi: an element no sampled row reaches is +0.0 bits, and with no sampled row at all every element is."""
    from densecap_amd import ops
    case = "minimal_no_droi"
    _name, (h, w), _np, _nn, _decay, _kw = CASES[case]
    W, feat, pi, pt, ni, gt, _droi, _ = draw(case)
    m = _model("minimal")
    ref = dict(rows=_rows(W, feat))
    trans, scores, anc, boxes = _tables(W, ref, h, w)
    got = ops.rpn_dheads(m.ctx, trans, scores, anc, boxes, h, w, 1, pi, pt, ni, gt, None, decay=0.0)
    touched = np.zeros(h * w, bool)
    touched[np.concatenate([pi, ni])] = True
    assert not _bits(got[~touched]).any() and got[touched].any()
    neg_only = np.zeros(h * w, bool)
    neg_only[ni] = True
    neg_only[pi] = False
    assert not _bits(got[neg_only][:, :4]).any()                     # negatives carry no transform gradient
    none = np.zeros(0, np.int32)
    assert not _bits(ops.rpn_dheads(m.ctx, trans, scores, anc, boxes, h, w, 1, none, none, none, gt, None, decay=0.0)).any()


@pytest.mark.parametrize("P,K6,R_", [(1, 6, 32), (48, 6, 32), (35, 30, 96), (48, 72, 256), (7, 72, 300)])
def test_rpn_heads_bwd_alone(P, K6, R_):
    from densecap_amd import ops
    ctx = _model("minimal").ctx
    rng = np.random.default_rng(P + K6 + R_)
    d = rng.standard_normal((P, K6)).astype(F32)
    Wh = rng.standard_normal((K6, R_)).astype(F32)
    y = np.maximum(rng.standard_normal((P, R_)), 0).astype(F32)
    got = ops.rpn_heads_bwd(ctx, d, Wh, y)
    want = (d.astype(np.float64) @ Wh.astype(np.float64)) * (y > 0)
    assert np.abs(got - want).max() <= R.REL * np.abs(want).max()
    assert not _bits(got[y <= 0]).any()                              # a masked element is +0.0
    assert np.array_equal(_bits(got), _bits(ops.rpn_heads_bwd(ctx, d, Wh, y)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_the_outputs_alone():
    from densecap_amd import _lib
    m = _model("minimal")
    ctx = m.ctx
    W, feat, pi, pt, ni, gt, droi, _ = draw("minimal_masked")
    h, w = 6, 8
    k, Rh = 1, 32
    fd = ctx.to_device(np.ascontiguousarray(feat.transpose(1, 2, 0)))
    gd = ctx.to_device(gt)
    shapes = {"rpn_conv_w": (Rh, 512, 3, 3), "rpn_conv_b": (Rh,), "rpn_box_w": (4 * k, Rh), "rpn_box_b": (4 * k,),
              "rpn_score_w": (2 * k, Rh), "rpn_score_b": (2 * k,), "feat": (h, w, 512)}
    bufs = {n: ctx.to_device(np.full(s, SENTINEL, F32)) for n, s in shapes.items()}
    lo, lb, mm = C.c_double(-1.0), C.c_double(-1.0), C.c_int32(-1)

    def call(pi_=pi, pt_=pt, ni_=ni, decay=5e-5, hw=(h, w), drop=None, G=len(gt), img=(96, 128)):
        pg = _lib.DcRpnGrads(**{n: (None if n == drop else b.ptr) for n, b in bufs.items()})
        dev = [ctx.to_device(np.asarray(a, np.int32)) if len(a) else None for a in (pi_, pt_, ni_)]
        ptr = lambda d: None if d is None else d.ptr
        return ctx.lib.dc_op_rpn_grad(ctx.h, fd.ptr, hw[0], hw[1], ptr(dev[0]), ptr(dev[1]), len(pi_), ptr(dev[2]), len(ni_), gd.ptr, G,
                                      None, img[0], img[1], None, float(decay), C.byref(pg), C.byref(lo), C.byref(lb), C.byref(mm))
    A = k * h * w
    bad_pi, bad_pt, bad_ni = pi.copy(), pt.copy(), ni.copy()
    bad_pi[0], bad_pt[1], bad_ni[-1] = A, len(gt), -1
    assert call(pi_=bad_pi) == -1 and call(pt_=bad_pt) == -1 and call(ni_=bad_ni) == -1
    assert call(ni_=np.zeros(1025 - len(pi), np.int32)) == -1                       # n = 1025
    assert call(decay=-1e-3) == -1 and call(decay=float("nan")) == -1 and call(decay=float("inf")) == -1
    assert call(drop="rpn_score_b") == -1 and call(drop="feat") == -1
    assert call(hw=(257, 256)) == -5
    assert call(img=(16, 128)) == -1 and call(G=0) == -1
    for n, b in bufs.items():
        assert np.array_equal(_bits(b.numpy()), _bits(np.full(shapes[n], SENTINEL, F32))), n
    assert (lo.value, lb.value, mm.value) == (-1.0, -1.0, -1)
    assert call() == 0 and lo.value > 0 and np.isfinite(bufs["feat"].numpy()).all()   # and the context still works
