"""tests/rpn_grad_rules.py checked on the CPU: the restated convolution and RPN gradients equal central differences of the
restated objectives (and, with an input row named twice, do NOT: the sampler's backward is a copy), every named wrong variant
leaves the bar, the float32 evaluation sits a decade inside it, the case generators need no redraw on the seeds the GPU tests
use, and the new prototypes and the hook header are where the binding, the Lua cdef and the other headers expect them."""
import os
import re

import numpy as np
import pytest

from tests import rpn_grad_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# maps on which every tap meets the border somewhere, and a rectangular one (so that a swap of (kh, kw) cannot hide)
CASES = [(3, 4, 32, 32, 1), (5, 2, 32, 64, 2), (4, 7, 64, 32, 3)]


def _ratio(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("case", CASES, ids=["%dx%d_%dto%d" % c[:4] for c in CASES])
def test_rules_equal_central_differences(case):
    """The objective is linear in each of w, b and x, so a central difference along a random direction is exact up to float64
    rounding: the directional derivative <grad, direction> must match it to 1e-9 relative."""
    h, w, Cin, Cout, seed = case
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed)
    g = R.conv3x3_grad(x, wt, dy)
    rng = np.random.default_rng(seed + 100)
    b0 = np.zeros(Cout)
    x64, w64 = x.astype(np.float64), wt.astype(np.float64)
    eps = 1e-3
    for name, base in (("dw", w64), ("db", b0), ("dx", x64)):
        d = rng.standard_normal(base.shape)
        args = lambda t: {"dw": (x64, t, b0, dy), "db": (x64, w64, t, dy), "dx": (t, w64, b0, dy)}[name]
        num = (R.objective(*args(base + eps * d)) - R.objective(*args(base - eps * d))) / (2 * eps)
        ana = float((g[name] * d).sum())
        assert abs(num - ana) <= 1e-9 * max(abs(ana), 1.0), (name, num, ana)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_leaves_the_bar(variant):
    h, w, Cin, Cout, seed = CASES[2]
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed)
    good, bad = R.conv3x3_grad(x, wt, dy), R.conv3x3_grad(x, wt, dy, variant=variant)
    worst = max(_ratio(bad[k], good[k]) for k in R.TENSORS)
    assert worst > 100 * R.REL, (variant, worst)


@pytest.mark.parametrize("case", CASES, ids=["%dx%d_%dto%d" % c[:4] for c in CASES])
def test_float32_evaluation_is_a_decade_inside_the_bar(case):
    h, w, Cin, Cout, seed = case
    x, wt, dy = R.make_case(h, w, Cin, Cout, seed)
    a, b = R.conv3x3_grad(x, wt, dy), R.conv3x3_grad(x, wt, dy, dtype="float32")
    for k in R.TENSORS:
        assert _ratio(b[k], a[k]) <= 0.1 * R.REL, (k, _ratio(b[k], a[k]))


def test_one_hot_gradient_picks_the_shifted_patch_and_the_weights():
    """dy one-hot at (o, y0, x0): dw[o, c, kh, kw] = x[c, y0 + kh - 1, x0 + kw - 1] (zero outside) and
    dx[c, y0 + kh - 1, x0 + kw - 1] = w[o, c, kh, kw] -- what the device test asks for bit for bit."""
    h, w, Cin, Cout = 4, 5, 32, 32
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, (Cin, h, w)).astype(F32)
    wt = rng.integers(-4, 5, (Cout, Cin, 3, 3)).astype(F32)
    for o, y0, x0 in ((3, 0, 0), (7, 2, 4), (31, 2, 2)):
        dy = np.zeros((Cout, h, w), F32)
        dy[o, y0, x0] = 1
        g = R.conv3x3_grad(x, wt, dy)
        dw, dx = R.one_hot_expected(x, wt, o, y0, x0)
        assert np.array_equal(g["dw"], dw) and np.array_equal(g["dx"], dx)


def _declared_symbols(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"\bint\s+(dc_[a-z0-9_]+)\s*\([^;]*?\)\s*;", text)}


def test_prototype_is_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name, nargs in (("dc_op_conv3x3_grad", 11), ("dc_op_rpn_grad", 20), ("dc_forward_backward", 17)):
        assert name in hp and lp.get(name) == hp[name], name
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1 == nargs, name
        assert name in _lib.EXPORTED_SYMBOLS
    strip = lambda t: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    st = re.search(r"typedef struct dc_rpn_grads \{(.*?)\} dc_rpn_grads;", strip(hdr)).group(1)
    assert st == re.search(r"typedef struct dc_rpn_grads \{(.*?)\} dc_rpn_grads;", strip(cdef)).group(1)
    assert [f for f, _ in _lib.DcRpnGrads._fields_] == re.findall(r"float\* (\w+);", st) == list(R.RPN_TENSORS)
    assert "model:forward_backward" in open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read().replace("Model:", "model:")


def test_hook_header_symbols_are_exported_and_not_bound_by_lua():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_rpn.h")
    assert sorted(hooks) == sorted(_lib._RPN_HOOK_SIGS) and len(hooks) == 4
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    assert not [h for h in hooks if h in lua]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
    for other in ("densecap_debug.h", "densecap_debug_grad.h", "densecap_debug_recog.h", "densecap_debug_bwd.h",
                  "densecap_debug_sample.h", "densecap_debug_beam.h"):
        assert not set(hooks) & set(_declared_symbols(other)), other


# ---- the RPN's backward --------------------------------------------------------------------------------------------------------------
MAP = (6, 8)


def _weights(name="minimal"):
    from tests.test_gpu_dims import set_weights
    return set_weights(name)


def _fd(W, feat, pi, pt, ni, gt, droi, decay, name, d, eps):
    """Central difference of the restated loss along direction d of tensor `name`."""
    import torch

    def at(sign):
        leaves = {n: torch.as_tensor(np.asarray(W[n], np.float64)) for n in R.RPN_PARAMS}
        leaves["feat"] = torch.as_tensor(np.asarray(feat, np.float64))
        leaves[name] = leaves[name] + sign * eps * torch.as_tensor(d.reshape(tuple(leaves[name].shape)))
        with torch.no_grad():
            return float(R.rpn_loss(W, feat, pi, pt, ni, gt, droi, decay, leaves=leaves)[0])
    return (at(1.0) - at(-1.0)) / (2 * eps)


def _directional(W, case, decay, seed):
    """Per tensor: (central difference, <gradient, direction>) along one random direction."""
    feat, pi, pt, ni, gt, droi, _ = case
    g = R.rpn_grad(W, feat, pi, pt, ni, gt, droi, decay)
    rng = np.random.default_rng(seed)
    out = {}
    for name in R.RPN_TENSORS:
        d = rng.standard_normal(g[name].shape)
        scale = float(np.abs(np.asarray(W[name] if name != "feat" else feat, np.float64)).max())
        out[name] = (_fd(W, feat, pi, pt, ni, gt, droi, decay, name, d, 1e-7 * scale), float((g[name] * d).sum()))
    return out


def test_rpn_rules_equal_central_differences_without_duplicates():
    """No input row is named twice: copy and sum coincide, and the seven tensors are the gradient of mid_objectness + mid_box_reg
    + 0.5 decay |trans|^2 + <droi, boxes>.  The kink, the mask and the ReLU are EDGE / HIDDEN_EDGE away, so a step of 1e-7 of the
    tensor's size crosses none of them (it moves a pre-activation by about 1e-7); float64 rounding leaves 1e-5 relative."""
    W = _weights()
    case = R.draw_rpn_case(W, MAP[0], MAP[1], 5, 6, seed=1, masked_rows=(0,), far_rows=(1,))
    assert case[6] == 0 and len(set(case[1].tolist()) | set(case[3].tolist())) == 11
    for name, (num, ana) in _directional(W, case, 0.5, 7).items():
        assert abs(num - ana) <= 1e-5 * max(abs(ana), 1e-6), (name, num, ana)


def test_rpn_rules_with_a_duplicate_are_not_a_gradient():
    """A negative that names a positive's input row overwrites the positive's score and box gradients: the seven tensors are no
    longer the gradient of the restated loss.  This records the quirk (BoxSamplerHelper.lua:166-177)."""
    W = _weights()
    case = R.draw_rpn_case(W, MAP[0], MAP[1], 5, 6, seed=2, neg_on_pos=2, dup_neg=1)
    assert case[6] == 0
    off = [abs(num - ana) / max(abs(ana), 1e-6) for num, ana in _directional(W, case, 0.0, 8).values()]
    assert max(off) > 1e-2, off


@pytest.mark.parametrize("variant", R.RPN_VARIANTS)
def test_every_wrong_rpn_variant_leaves_the_bar(variant):
    W = _weights()
    feat, pi, pt, ni, gt, droi, redraw = R.draw_rpn_case(W, MAP[0], MAP[1], 6, 7, seed=3, masked_rows=(0, 2), far_rows=(1,), dup_neg=1,
                                                         neg_on_pos=1, dup_pos=1)
    assert redraw == 0
    good, bad = R.rpn_grad(W, feat, pi, pt, ni, gt, droi, 0.5), R.rpn_grad(W, feat, pi, pt, ni, gt, droi, 0.5, variant=variant)
    worst = max(_ratio(bad[k], good[k]) for k in R.RPN_TENSORS)
    assert worst > R.REL, (variant, worst)


@pytest.mark.parametrize("name", ["minimal", "odd32"])
def test_float32_rpn_evaluation_is_a_decade_inside_the_bar(name):
    W = _weights(name)
    feat, pi, pt, ni, gt, droi, redraw = R.draw_rpn_case(W, MAP[0], MAP[1], 6, 7, seed=4, masked_rows=(0,), far_rows=(1,), dup_neg=1)
    assert redraw == 0
    a, b = R.rpn_grad(W, feat, pi, pt, ni, gt, droi, 5e-5), R.rpn_grad(W, feat, pi, pt, ni, gt, droi, 5e-5, dtype="float32")
    for k in R.RPN_TENSORS:
        assert _ratio(b[k], a[k]) <= 0.1 * R.REL, (k, _ratio(b[k], a[k]))


def test_gpu_cases_need_no_redraw():
    """The seeds tests/test_gpu_rpn_grad.py draws its cases on give a clean case at the first try."""
    from tests import test_gpu_rpn_grad as T
    for case in T.CASES:
        assert T.draw(case)[-1] == 0, case
