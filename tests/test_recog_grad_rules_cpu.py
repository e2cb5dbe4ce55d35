"""tests/recog_grad_rules.py tied down on the CPU: its forward is the oracle's RoI pooling and tests/loss_rules.py's two end
losses, its gradients are what central differences in float64 give, its generated cases keep their distance from the floors and
the SmoothL1 kink, and every wrong variant is caught by the bar the GPU tests use."""
import os
import re

import numpy as np
import pytest

from oracle import densecap_oracle as O
from tests import loss_rules as LR
from tests import recog_grad_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-4                     # tests/parity.py's continuous-stage bar, the one the GPU tests use
IMG, MAP = (96, 128), (6, 8)   # image (H, W) and feature map (h, w)


@pytest.fixture(scope="module")
def W():
    from densecap_amd.weights import make_synthetic_weights
    return make_synthetic_weights(seed=11, vocab_size=5, seq_length=1, rpn_hidden=32, enc_size=32, rnn_size=32, fc_dim=256,
                                  anchors=np.array([[96], [80]], np.float32))


@pytest.fixture(scope="module")
def case(W):
    """n = 6 rows, 3 positive: row 0 masked, row 1 on SmoothL1's linear branch, some boxes across the border."""
    rng = np.random.default_rng(5)
    feat, boxes, targets = R.draw_case(W, rng, 6, 3, IMG[0], IMG[1], MAP[0], MAP[1], masked_rows=(0,), far_rows=(1,), outside=0.4)
    g = (rng.standard_normal((3, 256)) * 1e-3).astype(np.float32)
    return feat, boxes, targets, g


def _ratio(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_forward_is_the_oracles_pooling_and_the_two_end_losses(W, case):
    import torch
    feat, boxes, targets, g = case
    P = R._torch_params(W, torch.float64, requires_grad=False)
    out = R.forward(P, torch.tensor(feat.astype(np.float64)), torch.tensor(boxes.astype(np.float64)), 3,
                    torch.tensor(targets.astype(np.float64)), None, IMG[0], IMG[1])
    ref = O.bilinear_roi_pool_np(feat, boxes, IMG[0], IMG[1])
    assert np.abs(out["pooled"].numpy() - ref).max() <= 2e-5 * np.abs(ref).max()
    obj = out["obj"].numpy().astype(np.float32)
    trans = (out["codes"][:3] @ P["boxreg_w"].T + P["boxreg_b"]).numpy().astype(np.float32)
    want_box = LR.box_reg_rows(boxes[:3], trans, targets)
    assert float(out["end_objectness_loss"]) == pytest.approx(float(np.float32(0.1)) * LR.logistic_rows(obj, 3).sum() / 6, rel=1e-6)
    assert float(out["end_box_reg_loss"]) == pytest.approx(float(np.float32(0.1)) * want_box[0].sum() / 12.0, rel=1e-6)
    assert out["masked_end"] == int(want_box[1].sum()) == 1
    res = out["residual"].numpy()
    assert (np.abs(res[1]) > 1).any() and (np.abs(res[2]) < 1).all()           # both SmoothL1 branches are in the case


def test_central_differences_agree_with_autograd(W, case):
    """Float64 coordinates throughout (coords="float64"), so that a perturbed box moves its sampling points."""
    import torch
    feat, boxes, targets, g = case
    ref = R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1], coords="float64")
    rng = np.random.default_rng(9)
    P = R._torch_params(W, torch.float64, requires_grad=False)
    base = dict(P, feat=torch.tensor(feat.astype(np.float64)), roi_boxes=torch.tensor(boxes.astype(np.float64)))
    t, gt = torch.tensor(targets.astype(np.float64)), torch.tensor(g.astype(np.float64))

    def total(v):
        with torch.no_grad():
            return float(R.forward({k: v[k] for k in R.PARAMS}, v["feat"], v["roi_boxes"], 3, t, gt, IMG[0], IMG[1], coords="float64")["total"])
    for k in R.TENSORS:
        d = torch.tensor(rng.standard_normal(tuple(base[k].shape)))
        d = d / d.norm()
        eps = 1e-6 * max(float(base[k].abs().max()), 1.0)
        num = (total(dict(base, **{k: base[k] + eps * d})) - total(dict(base, **{k: base[k] - eps * d}))) / (2 * eps)
        ana = float((torch.tensor(ref[k]) * d).sum())
        assert abs(num - ana) <= 1e-5 * max(abs(ana), float(np.abs(ref[k]).max()) * 1e-3), (k, num, ana)


def test_straight_through_coordinates_change_little(W, case):
    """float32 coordinates move a sampling point by at most an ulp of a coordinate below 2^7 px, 8e-6 px, so a blend weight by as
    much: the two forms of the restatement agree to 1e-3 of a tensor's largest entry, far inside which the device must land."""
    feat, boxes, targets, g = case
    a = R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1])
    b = R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1], coords="float64")
    for k in R.TENSORS:
        assert _ratio(a[k], b[k]) <= 1e-3, k


def test_generated_cases_keep_their_distance(W, case):
    import torch
    feat, boxes, targets, g = case
    assert (R.edge_distance(boxes, IMG[0], IMG[1], MAP[0], MAP[1], 7, 7) > R.EDGE).all()
    rng = np.random.default_rng(1)
    for (h, w), (HH, WW) in (((38, 45), (7, 7)), ((2, 2), (7, 7)), ((5, 4), (2, 3))):
        b = R.draw_boxes(rng, 40, 600, 720, h, w, HH, WW, outside=0.3)
        assert (R.edge_distance(b, 600, 720, h, w, HH, WW) > R.EDGE).all()
    P = R._torch_params(W, torch.float64, requires_grad=False)
    res = R.forward(P, torch.tensor(feat.astype(np.float64)), torch.tensor(boxes.astype(np.float64)), 3,
                    torch.tensor(targets.astype(np.float64)), None, IMG[0], IMG[1])["residual"].numpy()
    assert (np.abs(np.abs(res[1:]) - 1.0) > R.EDGE).all()


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_is_caught_by_the_bar(W, case, variant):
    feat, boxes, targets, g = case
    ref, bad = R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1]), R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1],
                                                                                          variant=variant)
    worst = max(_ratio(bad[k], ref[k]) for k in R.TENSORS)
    assert worst > 100 * REL, (variant, worst)


@pytest.mark.parametrize("variant", ("no_w_factor", "clamp_taps"))
def test_pooling_variants_are_caught_on_the_pooling_alone(case, variant):
    feat, boxes, targets, g = case
    dout = np.random.default_rng(2).standard_normal((6, 512, 7, 7)).astype(np.float32)
    ref, bad = R.roi_pool_grad(feat, boxes, IMG[0], IMG[1], dout), R.roi_pool_grad(feat, boxes, IMG[0], IMG[1], dout, variant=variant)
    assert max(_ratio(bad[0], ref[0]), _ratio(bad[1], ref[1])) > 100 * REL


def test_float32_autograd_is_inside_the_bar(W, case):
    """The error any fp32 implementation carries: float32 autograd against float64 autograd of the same restatement."""
    import torch
    feat, boxes, targets, g = case
    a, b = R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1]), R.recog_grad(W, feat, boxes, 3, targets, g, IMG[0], IMG[1],
                                                                                    dtype=torch.float32)
    for k in R.TENSORS:
        assert _ratio(b[k], a[k]) <= 0.1 * REL, (k, _ratio(b[k], a[k]))


def _declared_symbols(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"\bint\s+(dc_[a-z0-9_]+)\s*\([^;]*?\)\s*;", text)}


def test_prototypes_are_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name, nargs in (("dc_op_roi_pool_grad", 14), ("dc_op_recog_grad", 16), ("dc_loss_gradients", 15), ("dc_feature_size", 4)):
        assert name in hp and lp.get(name) == hp[name], name
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1 == nargs, name
    strip = lambda t: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    st = re.search(r"typedef struct dc_recog_grads \{(.*?)\} dc_recog_grads;", strip(hdr)).group(1)
    assert st == re.search(r"typedef struct dc_recog_grads \{(.*?)\} dc_recog_grads;", strip(cdef)).group(1)
    assert [f for f, _ in _lib.DcRecogGrads._fields_] == re.findall(r"float\* (\w+);", st) == list(R.TENSORS)
    assert "model:loss_gradients" in open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read().replace("Model:", "model:")


def test_hook_header_symbols_are_exported_and_not_bound_by_lua():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_recog.h")
    assert sorted(hooks) == sorted(_lib._RECOG_HOOK_SIGS) and len(hooks) == 5
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    assert not [h for h in hooks if h in lua]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
