"""CPU checks of the language-model gradient restatement (tests/lm_grad_rules.py) and of the new prototype's three copies."""
import os
import re

import numpy as np
import pytest

from tests import lm_grad_rules as G
from tests.test_abi_and_host import _declared_symbols, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-4            # the continuous-stage bar the device is held to (tests/parity.py)


def _minimal():
    from tests.test_gpu_dims import SETS, set_weights
    return set_weights("minimal"), SETS["minimal"]


@pytest.fixture(scope="module")
def case():
    W, s = _minimal()
    rng = np.random.default_rng(5)
    n, L = 4, 3
    return W, s, G.draw_codes(n, s["D"], rng), G.draw_labels(n, L, s["V"], rng)


def test_rowlik_is_the_scoring_restatements_number(case):
    from tests import score_restatement
    W, s, codes, lab = case
    ref = G.lm_grad(W, codes, lab)
    want = np.diag(score_restatement.lm_score(codes, W, lab))          # float32 pieces, float64 sums
    assert np.abs(ref["rowlik"] - want).max() <= 1e-5 * np.abs(want).max()
    assert ref["loss"] == pytest.approx(-ref["rowlik"].sum() / (lab.shape[0] * (lab.shape[1] + 2)), rel=1e-14)


def test_gradients_agree_with_central_differences(case):
    import torch
    W, s, codes, lab = case
    ref = G.lm_grad(W, codes, lab, weight=0.7)
    rng = np.random.default_rng(9)
    eps = 1e-5
    for name in G.TENSORS:
        g = ref[name]
        base = codes.astype(np.float64) if name == "codes" else W[name].double().numpy()
        bar = 1e-6 * np.abs(g).max()
        flat = rng.choice(g.size, size=min(12, g.size), replace=False)
        if name == "lm_emb":                                                  # make sure fed rows are among the entries
            E = g.shape[1]
            rows = G.fed_rows(lab, s["V"])[:4]
            flat[:len(rows)] = [r * E + int(rng.integers(E)) for r in rows]
        for i in flat:
            vals = []
            for sgn in (+1, -1):
                p = base.copy().ravel()
                p[i] += sgn * eps
                Wp = dict(W)
                cp = codes
                if name == "codes":
                    cp = torch.from_numpy(p.reshape(base.shape))
                else:
                    Wp[name] = torch.from_numpy(p.reshape(base.shape))
                vals.append(G.loss_only(Wp, cp, lab, weight=0.7))
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - g.ravel()[i]) <= bar, (name, int(i), fd, g.ravel()[i])


def test_never_fed_embedding_rows_are_zero_in_the_restatement(case):
    W, s, codes, lab = case
    g = G.lm_grad(W, codes, lab)["lm_emb"]
    fed = G.fed_rows(lab, s["V"])
    rest = [r for r in range(g.shape[0]) if r not in fed]
    assert s["V"] + 1 in rest and not g[rest].any() and all(g[r].any() for r in fed)


@pytest.mark.parametrize("variant", ["swap_fo", "div_L1", "image_step"])
def test_wrong_restatements_miss_the_bar_by_a_wide_margin(case, variant):
    """Teeth: each of these mistakes moves some tensor (or the loss) by far more than the 1e-4 the device is held to."""
    W, s, codes, lab = case
    ref, bad = G.lm_grad(W, codes, lab), G.lm_grad(W, codes, lab, variant=variant)
    worst = max(np.abs(bad[k] - ref[k]).max() / np.abs(ref[k]).max() for k in G.TENSORS)
    worst = max(worst, abs(bad["loss"] - ref["loss"]) / abs(ref["loss"]))
    assert worst > 100 * REL, (variant, worst)


def test_float32_autograd_is_far_inside_the_bar(case):
    """The error any fp32 implementation carries: float32 autograd against float64 autograd of the same restatement."""
    import torch
    W, s, codes, lab = case
    a, b = G.lm_grad(W, codes, lab), G.lm_grad(W, codes, lab, dtype=torch.float32)
    for k in G.TENSORS:
        assert np.abs(a[k] - b[k]).max() <= 1e-2 * REL * np.abs(a[k]).max(), k
    assert abs(a["loss"] - b["loss"]) <= 1e-6 * abs(a["loss"])


def test_prototype_is_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    assert "dc_op_lm_grad" in hp and lp.get("dc_op_lm_grad") == hp["dc_op_lm_grad"]
    res, args = _lib._SIGS["dc_op_lm_grad"]
    assert len(args) == hp["dc_op_lm_grad"].count(",") + 1 == 9
    strip = lambda t: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    st = re.search(r"typedef struct dc_lm_grads \{(.*?)\} dc_lm_grads;", strip(hdr)).group(1)
    assert st == re.search(r"typedef struct dc_lm_grads \{(.*?)\} dc_lm_grads;", strip(cdef)).group(1)
    assert [f for f, _ in _lib.DcLmGrads._fields_] == re.findall(r"float\* (\w+);", st) == list(G.TENSORS)
    assert "model:lm_gradients" in open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read().replace("Model:", "model:")


def test_hook_header_symbols_are_exported_and_not_bound_by_lua():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_grad.h")
    assert sorted(hooks) == sorted(_lib._GRAD_HOOK_SIGS) and len(hooks) == 5
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    assert not [h for h in hooks if h in lua]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
