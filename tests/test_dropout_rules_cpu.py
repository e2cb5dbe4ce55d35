"""tests/dropout_rules.py tied down on the CPU (docs/SEMANTICS.md, "Dropout"): the threshold at the ends of p's range, the mask as
a pure function of (seed, layer, row, col), the autograd restatement against central differences, the kept fraction of the
seeds the GPU tests use, and every wrong variant rejected by the comparators the GPU tests use -- bit equality for the masks and
the activations, tests/grad_bars.py's per-row rule at its own bar for the gradients."""
import os
import re

import numpy as np
import pytest

from tests import dropout_rules as DR
from tests import loss_rules as LR
from tests import recog_grad_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
IMG, MAP = (96, 128), (6, 8)
P, SEED = 0.5, 7
FRACTION_SEEDS = {0.1: 3, 0.5: 3, 0.9: 3}          # the kept-fraction check below passes for these; the GPU tests then compare bits


@pytest.fixture(scope="module")
def W():
    from densecap_amd.weights import make_synthetic_weights
    return make_synthetic_weights(seed=11, vocab_size=5, seq_length=1, rpn_hidden=32, enc_size=32, rnn_size=32, fc_dim=256,
                                  anchors=np.array([[96], [80]], np.float32))


@pytest.fixture(scope="module")
def case(W):
    """n = 3 rows, 2 positive, row 1 on SmoothL1's linear branch; a gradient g of the positive codes."""
    rng = np.random.default_rng(5)
    feat, boxes, targets = R.draw_case(W, rng, 3, 2, IMG[0], IMG[1], MAP[0], MAP[1], far_rows=(1,), outside=0.3)
    g = (rng.standard_normal((2, 256)) * 1e-3).astype(F32)
    return feat, boxes, targets, g


@pytest.fixture(scope="module")
def refs(W, case):
    """The restatement under the rule's masks in float64 and in float32: the reference and the evaluation the bar comes from."""
    import torch
    feat, boxes, targets, g = case
    m1, m2 = DR.masks_for(3, 256, P, SEED)
    args = (W, feat, boxes, 2, targets, g, IMG[0], IMG[1], m1, m2, P)
    return DR.recog_grad(*args), DR.recog_grad(*args, dtype=torch.float32)


def test_threshold_and_scale_at_the_ends_of_the_range():
    tiny, top = np.nextafter(F32(0), F32(1)), np.nextafter(F32(1), F32(0))
    assert DR.threshold(0.0) == 2 ** 32 and DR.threshold(0.5) == 2 ** 31
    assert DR.threshold(0.1) == (2 ** 27 - 13421773) * 32 == 3865470560      # 0.1f = 13421773 * 2^-27: the product is exact
    assert DR.threshold(top) == 256                      # 1 - p = 2^-24
    assert DR.threshold(tiny) == 2 ** 32                 # 1 - 2^-149 rounds to 1 in double: every element is kept
    assert DR.scale(0.5) == F32(2) and DR.scale(0.0) == F32(1) and DR.scale(tiny) == F32(1) and DR.scale(top) == F32(2 ** 24)
    assert DR.scale(0.1).dtype == F32 and DR.scale(0.1) == F32(1) / F32(0.9)                   # inexact: 1.1111112
    assert DR.mask(3, 5, 1, tiny, 9).all() and DR.mask(3, 5, 1, 0.0, 9).all()


def test_the_mask_of_a_matrix_is_the_mask_of_any_sub_block_of_a_larger_one():
    big = DR.mask(9, 23, 2, 0.3, 2 ** 40 + 5)
    for r0, c0, rows, cols in ((0, 0, 9, 23), (0, 0, 4, 7), (2, 3, 5, 6), (8, 22, 1, 1), (1, 4, 3, 8), (3, 17, 6, 5)):
        assert np.array_equal(DR.mask(rows, cols, 2, 0.3, 2 ** 40 + 5, row0=r0, col0=c0), big[r0:r0 + rows, c0:c0 + cols])
    assert np.array_equal(DR.mask(4, 7, 2, 0.3, 2 ** 40 + 5), big[:4, :7])       # no dependence on the row count or the width
    assert not np.array_equal(DR.mask(9, 23, 1, 0.3, 2 ** 40 + 5), big)            # the layer
    assert not np.array_equal(DR.mask(9, 23, 2, 0.3, 5), big)                      # the seed's high word alone
    assert np.array_equal(DR.words(2, 8, 1, 5)[1, 4:], np.array(LR.philox4x32_10(1, 1, 1, 1, 5, 0), np.uint32))


def test_forward_and_backward_of_one_layer():
    x = np.array([[1.5, -0.0, np.inf, np.nan, 1e-45, -2.0, 3.0]], F32)
    keep = DR.mask(1, 7, 1, 0.5, 4)
    y = DR.dropout_forward(x, 1, 0.5, 4)
    assert keep.any() and not keep.all()
    assert not y[~keep].view(np.uint32).any()                                      # +0.0 bits, whatever x was
    want = x * F32(2)
    assert np.array_equal(y[keep].view(np.uint32)[~np.isnan(want[keep])], want[keep].view(np.uint32)[~np.isnan(want[keep])])
    assert np.array_equal(DR.dropout_forward(x, 1, 0.0, 4).view(np.uint32), x.view(np.uint32))
    dy = np.arange(1, 8, dtype=F32).reshape(1, 7)
    d = DR.relu_dropout_grad(x, dy, 0.5)
    assert np.array_equal(d, np.array([[2, 0, 6, 0, 10, 0, 14]], F32)) and not d[0, [1, 3, 5]].view(np.uint32).any()
    assert np.array_equal(DR.relu_dropout_grad(x, dy, 0.0), np.array([[1, 0, 3, 0, 5, 0, 7]], F32))


def test_central_differences_agree_with_autograd(W, case):
    """Float64 coordinates throughout, as in the recognition rules' own test; the masks are held fixed."""
    import torch
    feat, boxes, targets, g = case
    m1, m2 = DR.masks_for(3, 256, P, SEED)
    ref = DR.recog_grad(W, feat, boxes, 2, targets, g, IMG[0], IMG[1], m1, m2, P, coords="float64")
    rng = np.random.default_rng(9)
    Pt = R._torch_params(W, torch.float64, requires_grad=False)
    base = dict(Pt, feat=torch.tensor(feat.astype(np.float64)), roi_boxes=torch.tensor(boxes.astype(np.float64)))
    t, gt = torch.tensor(targets.astype(np.float64)), torch.tensor(g.astype(np.float64))

    def total(v):
        with torch.no_grad():
            return float(DR.forward({k: v[k] for k in R.PARAMS}, v["feat"], v["roi_boxes"], 2, t, gt, IMG[0], IMG[1], m1, m2, P,
                                    coords="float64")["total"])
    for k in R.TENSORS:
        d = torch.tensor(rng.standard_normal(tuple(base[k].shape)))
        d = d / d.norm()
        eps = 1e-6 * max(float(base[k].abs().max()), 1.0)
        num = (total(dict(base, **{k: base[k] + eps * d})) - total(dict(base, **{k: base[k] - eps * d}))) / (2 * eps)
        ana = float((torch.tensor(ref[k]) * d).sum())
        assert abs(num - ana) <= 1e-5 * max(abs(ana), float(np.abs(ref[k]).max()) * 1e-3), (k, num, ana)


def test_the_restatement_drops_what_the_masks_drop_and_at_p_0_is_the_recognition_rules(W, case, refs):
    feat, boxes, targets, g = case
    m1, m2 = DR.masks_for(3, 256, P, SEED)
    ref = refs[0]
    assert not ref["fc6_out"][~m1].any() and not ref["codes_fwd"][~m2].any()
    assert (ref["fc6_out"][m1] > 0).any() and (ref["codes_fwd"][m2] > 0).any()
    dead7 = ~(ref["codes_fwd"] > 0).any(0)                                         # ReLU-dead or dropped in every row
    assert dead7.any() and not ref["fc7_w"][dead7].any()
    ones = np.ones((3, 256), bool)
    a, b = DR.recog_grad(W, feat, boxes, 2, targets, g, IMG[0], IMG[1], ones, ones, 0.0), R.recog_grad(W, feat, boxes, 2, targets, g, IMG[0], IMG[1])
    for k in R.TENSORS:
        assert np.array_equal(a[k], b[k]), k


def test_the_float32_evaluation_passes_its_own_comparator(refs):
    assert not DR.row_failures("float32 evaluation", refs[1], refs[0], refs[1])


@pytest.mark.parametrize("variant", DR.VARIANTS)
def test_every_wrong_variant_is_rejected_by_the_gpu_tests_comparators(W, case, refs, variant):
    """A float32 evaluation of the wrong form stands in for the device.  Mask variants: the masks differ (what the bit comparison
    of "loss_fc6_out" and of ops.dropout sees).  All five: the per-row rule at its own bar rejects the gradients."""
    import torch
    feat, boxes, targets, g = case
    m1, m2 = DR.masks_for(3, 256, P, SEED)
    w1, w2 = DR.masks_for(3, 256, P, SEED, variant=variant)
    if variant in DR.MASK_VARIANTS:
        assert not (np.array_equal(w1, m1) and np.array_equal(w2, m2))
        assert abs(w1.mean() - 0.5) < 0.1 and abs(w2.mean() - 0.5) < 0.1            # (a mask, only not the rule's)
    else:
        x = np.random.default_rng(1).standard_normal((3, 256)).astype(F32)
        good = DR.apply_mask(x, m1, P)
        assert not np.array_equal(np.where(m1, x, F32(0)).view(np.uint32), good.view(np.uint32))             # forward, bits
        assert not np.array_equal(DR.relu_dropout_grad(good, x, 0.0).view(np.uint32), DR.relu_dropout_grad(good, x, P).view(np.uint32))
    bad = DR.recog_grad(W, feat, boxes, 2, targets, g, IMG[0], IMG[1], w1, w2, P, variant=variant, dtype=torch.float32)
    fails = DR.row_failures(variant, bad, refs[0], refs[1])
    assert fails, variant
    if variant == "no_forward_scale":                                                # fc6's forward does not see it; its gradient does
        assert np.abs(bad["fc6_out"] - refs[0]["fc6_out"]).max() > 0.1 * np.abs(refs[0]["fc6_out"]).max()


def test_kept_fraction_over_2_to_the_20_elements():
    """|kept / N - (1 - p)| <= 5 sqrt(p (1 - p) / N), N = 2^20, for the seeds named above (one Philox draw serves all three p)."""
    N = 2 ** 20
    cache = {}
    for p, seed in FRACTION_SEEDS.items():
        if seed not in cache:
            cache[seed] = DR.words(256, 4096, 1, seed).astype(np.uint64)
        frac = float((cache[seed] < np.uint64(DR.threshold(p))).mean())
        print("kept fraction at p = %.1f, seed %d: %.6f" % (p, seed, frac))
        assert abs(frac - (1.0 - float(F32(p)))) <= 5.0 * np.sqrt(p * (1 - p) / N), (p, frac)


# ---- the three copies of the C ABI and the places that describe it -------------------------------------------------------------------
def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"\bint\s+(dc_[a-z0-9_]+)\s*\([^;]*?\)\s*;", text)}


def test_prototypes_are_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name, nargs in (("dc_set_dropout", 2), ("dc_get_dropout", 2), ("dc_op_dropout", 7), ("dc_op_relu_dropout_grad", 5)):
        assert name in hp and lp.get(name) == hp[name], name
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1 == nargs, name
    shim = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    assert "dc_set_dropout" in shim and "drop_prob" in shim


def test_the_command_line_flags_default_to_no_dropout():
    from densecap_amd import evaluate_model as E, train as T
    assert T.build_parser().parse_args([]).drop_prob == 0.0 and T.build_parser().parse_args(["-drop_prob", "0.5"]).drop_prob == 0.5
    assert E.build_parser().parse_args([]).drop_prob == 0.0 and E.build_parser().parse_args(["-losses", "1", "-drop_prob", "0.5"]).drop_prob == 0.5
    assert "drop_prob" not in T.loss_options(T.build_parser().parse_args(["-drop_prob", "0.5"]), 1)
    assert "-drop_prob 0.5" in T.__doc__ and "reference" in T.__doc__
    src = open(os.path.join(ROOT, "tools", "train_step_bench.py")).read()
    assert "--drop_prob" in src


def test_the_documents_describe_dropout():
    sem = open(os.path.join(ROOT, "docs", "SEMANTICS.md")).read()
    assert "\n## Dropout" in sem and "+0.0" in sem[sem.index("\n## Dropout"):]
    assert "Dropout" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for path in ("README.md", os.path.join("include", "densecap.h"), os.path.join("densecap_amd", "train.py")):
        assert "Dropout is the identity" not in open(os.path.join(ROOT, path)).read().replace("\n * ", " ").replace("\n", " "), path
