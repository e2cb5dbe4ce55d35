"""CPU checks of the per-row comparator (tests/grad_bars.py): it rejects what the max-norm bar lets through, the float32
evaluation of the rules stays inside its own bar on every case the GPU modules add (so the inputs are fair: no row of theirs
is a cancelled sum that float32 cannot follow), and the hooks of include/densecap_debug_bwd.h are bound and kept off the boundary."""
import os

import numpy as np
import pytest

from tests import grad_bars as GB
from tests import lm_grad_rules as G
from tests import recog_grad_rules as R
from tests.test_abi_and_host import _declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-4            # the max-norm bar of the gradient tests
F32 = np.float32


@pytest.fixture(scope="module")
def ckpt():
    """The checkpoint's vocabulary, n = 3, L = 2: (labels, V, float64 reference, float32 evaluation)."""
    import torch
    from tests.test_gpu_lm_grad import case_inputs
    W, codes, lab = case_inputs("ckpt_vocab_3x2")
    V = int(W["lm_out_w"].shape[0]) - 1
    assert V == 10497
    return lab, V, G.lm_grad(W, codes, lab), G.lm_grad(W, codes, lab, dtype=torch.float32)


def test_scaled_non_target_rows_pass_the_max_norm_and_fail_the_comparator(ckpt):
    """Teeth: every non-target row of the lm_out_w gradient times 1.05 -- a softmax that is 5 % off everywhere but at the
    targets.  max|dev - ref| <= 1e-4 max|ref| accepts it; the per-row bar rejects thousands of rows."""
    lab, V, ref, ref32 = ckpt
    g = ref["lm_out_w"]
    targets = sorted(set(int(w) - 1 for w in lab.ravel() if w != 0) | {V})                   # the words and END (row V)
    wrong = g.copy()
    rest = np.setdiff1d(np.arange(V + 1), targets)
    wrong[rest] *= 1.05
    small = np.abs(g).max(1) < 1e-3 * np.abs(g).max()
    assert small.sum() >= V - 10 and not small[targets].all()                                # almost every row is far below the maximum
    assert np.abs(wrong - g).max() <= REL * np.abs(g).max()                                  # the old bar lets it through
    bar = GB.bar_from_float32("lm_out_w", ref32["lm_out_w"], g)
    assert 0 < bar < REL
    w, bad = GB.check_rows("lm_out_w", wrong.astype(F32), g, bar)
    assert bad and w == pytest.approx(0.05, rel=1e-3)
    assert not GB.check_rows("lm_out_w", g.astype(F32), g, bar)[1]                           # the reference rounded to float32 passes
    # the comparator looks at every row: ONE wrong small row is enough
    one = g.copy()
    one[rest[len(rest) // 2]] *= 1.0001
    assert np.abs(one - g).max() <= 1e-3 * REL * np.abs(g).max()
    assert [r for r, _ in GB.check_rows("lm_out_w", one.astype(F32), g, bar)[1]] == [int(rest[len(rest) // 2])]


@pytest.mark.parametrize("junk", [-0.0, 1e-30])
def test_a_never_fed_row_must_be_plus_zero(ckpt, junk):
    lab, V, ref, ref32 = ckpt
    g = ref["lm_emb"]
    fed = G.fed_rows(lab, V)
    never = [r for r in (0, V // 2, V + 1) if r not in fed]
    assert V + 1 in never and not g[never].any()
    bar = GB.bar_from_float32("lm_emb", ref32["lm_emb"], g)
    dev = g.astype(F32)
    assert not GB.check_rows("lm_emb", dev, g, bar)[1]
    for r in never:
        bad = dev.copy()
        bad[r, 3] = junk
        assert GB.check_rows("lm_emb", bad, g, bar)[1] == [(r, "not +0.0")]
    nan = dev.copy()
    nan[fed[0], 0] = np.nan                                                                   # and a NaN in a live row is a miss
    assert GB.check_rows("lm_emb", nan, g, bar)[1]


def test_feat_rows_are_pixels():
    a = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    rows = GB.rows_of("feat", a)
    assert rows.shape == (12, 2) and np.array_equal(rows[5], a[:, 1, 1])
    with pytest.raises(ValueError):
        GB.rows_of("lstm_b", np.zeros(4))


def _float32_passes_its_own_bar(what, tensors, ref64, ref32):
    for k in tensors:
        bar = GB.bar_from_float32(k, ref32[k], ref64[k])
        w, bad = GB.check_rows(k, ref32[k].astype(F32), ref64[k], bar)
        print("float32 evaluation, %s %s: worst per-row ratio %.2e, bar %.2e" % (what, k, w, bar))
        assert not bad, (what, k, bad)
        # The row-sparse tensors the comparator is for stay below the max-norm bar they stand beside, on every row.  (lm_enc_w and
        # lstm_w rows are sums over n or P rows of d(pre-activation) values that are themselves cancelled sums of 4 Hd terms: with
        # a handful of rows the float32 evaluation's own worst row reaches 1e-4 there, and the bar follows it.)
        if k in ("lm_out_w", "lm_emb", "dfeat"):
            assert bar < REL, (what, k, bar)


def _lm_new_cases():
    from tests.test_gpu_lm_grad import NEW_CASES
    return list(NEW_CASES)


@pytest.mark.parametrize("case", _lm_new_cases())
def test_float32_evaluation_of_the_new_language_model_cases_passes_its_own_bar(case):
    import torch
    from tests.test_gpu_lm_grad import case_inputs
    W, codes, lab = case_inputs(case)
    _float32_passes_its_own_bar(case, GB.LM_ROW_TENSORS, G.lm_grad(W, codes, lab), G.lm_grad(W, codes, lab, dtype=torch.float32))


def _roi_new_cases():
    from tests.test_gpu_roi_pool_grad import LIMIT_MAPS, POOL_LIMIT
    return list(LIMIT_MAPS) + [POOL_LIMIT]


@pytest.mark.parametrize("name", _roi_new_cases())
def test_float32_evaluation_of_the_new_roi_cases_passes_its_own_bar(name):
    import torch
    from tests import test_gpu_roi_pool_grad as T
    img, (h, w), C, (HH, WW), boxes, _ = T._case(name)
    rng = np.random.default_rng(len(name) * 7 + C)
    feat = rng.standard_normal((C, h, w)).astype(F32)
    dout = rng.standard_normal((len(boxes), C, HH, WW)).astype(F32)
    assert (R.edge_distance(boxes, img[0], img[1], h, w, HH, WW) > R.EDGE).all()
    a = R.roi_pool_grad(feat, boxes, img[0], img[1], dout, HH, WW)
    b = R.roi_pool_grad(feat, boxes, img[0], img[1], dout, HH, WW, dtype=torch.float32)
    _float32_passes_its_own_bar(name, ("dfeat",), {"dfeat": a[0]}, {"dfeat": b[0]})


def test_bwd_hook_header_symbols_are_exported_and_not_bound_by_lua():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_bwd.h")
    assert sorted(hooks) == sorted(_lib._BWD_HOOK_SIGS) and len(hooks) == 3
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    assert not [h for h in hooks if h in lua]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
    for other in ("densecap_debug.h", "densecap_debug_grad.h", "densecap_debug_recog.h"):
        assert not set(hooks) & set(_declared_symbols(other)), other
