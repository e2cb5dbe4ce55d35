"""tests/cnn_grad_rules.py checked on the CPU: chain on torch's own float64 activations equals torch autograd through conv2d /
relu / max_pool2d(ceil_mode=True) of the nine layers, every named wrong variant fails on a constructed case, the input conditions
of the GPU chain test hold in float32 (He-scaled weights, no dead or saturated ReLU mask, no pixel of the input gradient that
float32 alone kills), and the new prototypes are where the binding and the Lua cdef expect them."""
import os
import re

import numpy as np
import pytest

from tests import cnn_grad_rules as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
REL = 1e-12


@pytest.fixture(scope="module")
def params():
    return CR.conv_params(CR.model_weights())


def _rel(a, b):
    s = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / s if s > 0 else float(np.abs(a).max())


@pytest.mark.parametrize("shape", CR.CHAIN_SHAPES, ids=["%dx%d" % s for s in CR.CHAIN_SHAPES])
def test_chain_equals_autograd_on_torchs_own_activations(params, shape):
    w, b = params
    x4, dfeat = CR.make_chain_case(*shape, seed=shape[0] * 10 + shape[1])
    want, acts, prepool = CR.autograd(x4, w, b, dfeat)
    got = CR.chain(acts, prepool, w, dfeat, "float64")
    figs = {k: _rel(got[k], want[k]) for k in want}
    print("chain vs autograd %dx%d: worst %.2e" % (shape + (max(figs.values()),)))
    assert all(v <= REL for v in figs.values()), {k: v for k, v in figs.items() if v > REL}
    assert np.abs(want["x"]).max() > 0 and all(np.abs(want["conv_w%d" % i]).max() > 0 for i in CR.CONVS)


def test_pool_rule_by_hand():
    """One channel, 3 x 3: four windows, three of them clipped.  The tie of window (0, 0) goes to its first place; the window of
    the single corner element is dead (zero); the right edge's window holds its maximum in its second row."""
    y = np.array([[[2, 2, 1], [2, 0, 3], [0, 5, 0]]], F32)
    g = np.array([[[10, 20], [30, 40]]], F32)
    want = np.array([[[10, 0, 0], [0, 0, 20], [0, 30, 0]]], F32)
    assert np.array_equal(CR.pool_relu_grad(y, g), want)
    assert np.array_equal(CR.relu_grad(np.array([1, 0, -0.0, -1, 1e-45], F32), np.arange(1, 6, dtype=F32)), np.array([1, 0, 0, 0, 5], F32))


def test_every_wrong_variant_fails_on_a_constructed_case():
    g = np.array([[[10, 20], [30, 40]]], F32)
    tie = np.array([[[2, 2, 1], [2, 0, 3], [0, 5, 0]]], F32)
    assert not np.array_equal(CR.pool_relu_grad(tie, g, "tie_last"), CR.pool_relu_grad(tie, g))
    zero = np.array([[[0, -1, 1], [-2, -3, 1], [1, 1, 0]]], F32)                      # window (0, 0): maximum 0, dead
    assert not np.array_equal(CR.pool_relu_grad(zero, g, "mask_ge"), CR.pool_relu_grad(zero, g))
    assert not np.array_equal(CR.relu_grad(zero, zero + 7, "mask_ge"), CR.relu_grad(zero, zero + 7))
    edge = np.array([[[1, 1, 1], [9, 1, 2], [1, 1, 1]]], F32)                         # the right edge's window must not see the 9
    assert not np.array_equal(CR.pool_relu_grad(edge, g, "edge_not_clipped"), CR.pool_relu_grad(edge, g))
    assert sorted(CR.VARIANTS) == ["edge_not_clipped", "mask_ge", "tie_last"]


def test_chain_variants_leave_the_reference(params):
    """On a full chain case with one tie and one exact zero planted in conv4_3's output, the wrong variants move the weight
    gradients by far more than the 1e-12 the right one keeps."""
    w, b = params
    x4, dfeat = CR.make_chain_case(5, 7, seed=57)
    acts, prepool = CR.forward(x4, w, b, "float64")
    p = prepool[9].copy()
    top = p[:, 0:2, 0:2].reshape(512, -1).max(1)
    p[:, 0, 0] = top; p[:, 1, 1] = top                                                # a tie in window (0, 0) of every channel
    prepool = {6: prepool[6], 9: p}
    ref = CR.chain(acts, prepool, w, dfeat)
    assert _rel(CR.chain(acts, prepool, w, dfeat, variant="tie_last")["conv_w9"], ref["conv_w9"]) > 1e-3
    acts0 = dict(acts)
    a = acts[12].copy(); a[a == 0] = -0.0; a[:, 0, 0] = 0                              # exact zeros in conv5_2's output
    acts0[12] = a
    ref0 = CR.chain(acts0, prepool, w, dfeat)
    assert _rel(CR.chain(acts0, prepool, w, dfeat, variant="mask_ge")["conv_w11"], ref0["conv_w11"]) > 1e-3


@pytest.mark.parametrize("shape", CR.CHAIN_SHAPES, ids=["%dx%d" % s for s in CR.CHAIN_SHAPES])
def test_input_conditions_of_the_gpu_chain_case(params, shape):
    """In float32 on the CPU: He-scaled weights, a live share of every ReLU mask in [0.2, 0.8], and no all-zero pixel of the
    gradient at conv3_1's input beyond those of the float64 reference on the same activations."""
    w, b = params
    for i in CR.CONVS:
        cin = CR.CHANNELS[i][0]
        assert w[i].shape == CR.CHANNELS[i][::-1] + (3, 3)
        assert abs(float(w[i].std()) / np.sqrt(2.0 / (9 * cin)) - 1) < 0.02, i
    x4, dfeat = CR.make_chain_case(*shape, seed=shape[0] * 10 + shape[1])
    acts, prepool = CR.forward(x4, w, b, "float32")
    for i in CR.CONVS:
        out = prepool[i] if i in CR.POOL_AFTER else acts[i + 1]
        live = float((out > 0).mean())
        print("conv %d live share %.3f" % (i, live))
        assert 0.2 <= live <= 0.8, (i, live)
    r64, r32 = CR.chain(acts, prepool, w, dfeat, "float64"), CR.chain(acts, prepool, w, dfeat, "float32")
    dead64 = ~np.abs(r64["x"]).reshape(128, -1).any(0)
    dead32 = ~np.abs(r32["x"]).reshape(128, -1).any(0)
    assert not (dead32 & ~dead64).any()
    assert np.isfinite(r32["x"]).all() and np.abs(r64["x"]).max() > 0


def test_pool_case_covers_what_it_says():
    """Positive ties at each of the four places of a window, all-zero windows, windows whose maximum is -0.0 and negative ones."""
    y, g = CR.make_pool_case(32, 5, 7, seed=3)
    first = set()
    zero = neg0 = neg = 0
    for c in range(32):
        for yo in range(2):
            for xo in range(3):                                                      # the full windows
                win = y[0, c, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].reshape(-1)
                m = win.max()
                if m > 0 and (win == m).sum() > 1:
                    first.add(int(np.argmax(win)))
                    first.update(int(p) + 10 for p in np.flatnonzero(win == m))
                zero += int(not win.view(np.uint32).any())
                neg0 += int(m == 0 and np.signbit(win).all())
                neg += int(m < 0)
    assert {10, 11, 12, 13} <= first and zero and neg0 and neg, (first, zero, neg0, neg)
    assert np.isnan(g).sum() == 1


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"\bint\s+(dc_[a-z0-9_]+)\s*\([^;]*?\)\s*;", text)}


def test_prototypes_are_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name, nargs in (("dc_op_maxpool2x2_grad", 8), ("dc_op_relu_grad", 4), ("dc_op_cnn_grad", 7), ("dc_forward_backward_cnn", 18), ("dc_train_set_cnn", 2)):
        assert name in hp and lp.get(name) == hp[name], name
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1 == nargs, name
        assert name in _lib.EXPORTED_SYMBOLS
    strip = lambda t: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    for st, cls in (("dc_cnn_grads", _lib.DcCnnGrads), ("dc_cnn_dump", _lib.DcCnnDump)):
        pat = r"typedef struct %s \{(.*?)\} %s;" % (st, st)
        body = re.search(pat, strip(hdr)).group(1)
        assert body == re.search(pat, strip(cdef)).group(1)
        fields = re.findall(r"float\* (\w+)(?:\[(\d+)\])?;", body)
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields]
        assert [C_sizeof(t) for _, t in cls._fields_] == [8 * int(n or 1) for _, n in fields]


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_finetune_cnn_after_maps_iterations_to_modes():
    """train.lua's iter is 0-based: k = it - 1 before the step; mode 0 below N, 1 at N (the decay-only step), 2 above."""
    from densecap_amd.ops import finetune_cnn_mode
    want = {-1: [0, 0, 0, 0, 0], 0: [1, 2, 2, 2, 2], 3: [0, 0, 0, 1, 2]}
    for N, modes in want.items():
        assert [finetune_cnn_mode(N, it) for it in range(1, 6)] == modes, N
    from densecap_amd import train
    assert train.build_parser().parse_args([]).finetune_cnn_after == -1
