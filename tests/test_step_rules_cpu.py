"""tests/step_rules.py checked on the CPU: the rules agree with their plain definitions on random logits, and on the crafted operands
the device tests use they reject five wrong variants -- the last maximum in the place of the first, a `>=` merge, a padding column
in the sum, a sentinel read as column 0, noise drawn per column in the place of per 4-column run.  The padding variant is also
shown to pass the whole-model bar it used to hide behind (1e-4 relative on a caption's log-likelihood) and to miss the kernel
test's bound by a wide factor.  Last, the hook header is where the binding expects it and off the drop-in boundary."""
import os
import re

import numpy as np
import pytest

from tests import step_rules as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = np.array([[3, 0], [3, 1], [900, 7], [0, 255], [17, 17]], np.int32)


def _random_z(M, V1, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal((M, V1)) * scale).astype(np.float32)


# ---- the rules against their definitions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V1", [1, 31, 32, 33, 64, 65, 97, 201])
def test_partials_and_merge_are_the_row_argmax(V1):
    z = _random_z(5, V1, V1)
    z[1, V1 // 2] = z[1].max()                                 # a tie: the first one wins
    slots = S.slots_of(V1)
    val, col = S.argmax_partials(z, V1, slots)
    assert val.shape == (5, slots) and ((col == S.NO_COL) == (np.arange(slots)[None, :] * 32 >= V1)).all()
    tok, slot = S.row_merge(val, col)
    np.testing.assert_array_equal(tok, z.argmax(1) + 1)
    np.testing.assert_array_equal(val[np.arange(5), slot], z.max(1))
    for s in range(slots):
        if 32 * s < V1:
            np.testing.assert_array_equal(col[:, s], 32 * s + z[:, 32 * s:32 * s + 32].argmax(1))


@pytest.mark.parametrize("V1", [1, 33, 64, 97, 201])
def test_lse_partials_sum_to_the_row_logsumexp(V1):
    z = _random_z(5, V1, 100 + V1)
    slots = S.slots_of(V1)
    mx, s = S.lse_partials(z, V1, slots)
    z64 = z.astype(np.float64)
    ref = z64.max(1) + np.log(np.exp(z64 - z64.max(1, keepdims=True)).sum(1))
    np.testing.assert_allclose(S.lse_rows(mx, s), ref, rtol=1e-14)
    empty = np.arange(slots) * 32 >= V1
    assert (mx[:, empty] == -np.inf).all() and (s[:, empty] == 0).all()
    tgt = np.array([1, V1, min(5, V1), 1, V1], np.int32)
    np.testing.assert_array_equal(S.target_logit(z, tgt), z[np.arange(5), tgt - 1])


def test_sampling_partials_at_zero_temperature_are_the_other_two():
    z = _random_z(5, 97, 7)
    slots = S.slots_of(97)
    mx, s, score, col, v = S.sample_partials(z, 97, slots, KEYS, 1, 5, 0.0)
    lm, ls = S.lse_partials(z, 97, slots)
    av, ac = S.argmax_partials(z, 97, slots)
    for a, b in ((mx, lm), (s, ls), (score, av), (col, ac), (v, av)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("inv_temp", [1.0, 0.5, 100.0])
def test_sampling_partials_follow_the_restatement(inv_temp):
    """The best perturbed entry over the slots is the restatement's word: arg-max of fp32(fp32(v inv_temp) + g) over the real
    columns with the noise of (seed, s, r, t, column), first maximum."""
    from tests import sample_restatement as R
    V1, t, seed = 97, 3, (5 << 32) | 9
    z = _random_z(5, V1, 8)
    slots = S.slots_of(V1)
    _, _, score, col, v = S.sample_partials(z, V1, slots, KEYS, t, seed, inv_temp)
    tok, slot = S.row_merge(score, col)
    g = R.gumbel(R.noise_bits(seed, KEYS[:, 1:2], KEYS[:, 0:1], t, np.arange(V1)[None, :])).astype(np.float32)
    pert = (z * np.float32(inv_temp)).astype(np.float32) + g
    np.testing.assert_array_equal(tok, pert.argmax(1) + 1)
    np.testing.assert_array_equal(v[np.arange(5), slot], z[np.arange(5), tok - 1])


def test_specials_follow_the_entry_rule():
    """An entry needs v > -inf: a -inf slot is empty, a NaN never wins, an all-NaN row has no word."""
    z = _random_z(4, 97, 9)
    z[0, 32:64] = -np.inf
    z[1, 40] = np.nan
    z[2, :] = np.nan
    z[3, :] = -np.inf
    slots = S.slots_of(97)
    val, col = S.argmax_partials(z, 97, slots)
    assert col[0, 1] == S.NO_COL and val[0, 1] == -np.inf
    assert col[1, 1] != 40 and col[1, 1] == 32 + np.nanargmax(z[1, 32:64])
    assert (col[2:] == S.NO_COL).all()
    tok, _ = S.row_merge(val, col)
    assert tok[2] == 0 and tok[3] == 0 and tok[0] == np.nanargmax(z[0]) + 1 and tok[1] == np.nanargmax(z[1]) + 1
    mx, s = S.lse_partials(z, 97, slots)
    assert mx[0, 1] == -np.inf and s[0, 1] == 0 and (mx[3] == -np.inf).all() and (s[3] == 0).all()


def test_lstm_update_is_torchs_lstm_cell():
    """torch.nn.LSTMCell orders its gates i, f, g, o: with the rows of torch-rnn's i, f, o, g moved there, zero recurrent
    weights and an identity input map, it is the same cell."""
    import torch
    rng = np.random.default_rng(3)
    Hd = 8
    x, gp, c = rng.standard_normal((3, 4 * Hd)), rng.standard_normal((3, 4 * Hd)), rng.standard_normal((3, Hd))
    cell = torch.nn.LSTMCell(4 * Hd, Hd, bias=False).double()
    perm = np.concatenate([np.arange(0, 2 * Hd), np.arange(3 * Hd, 4 * Hd), np.arange(2 * Hd, 3 * Hd)])
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(4 * Hd, dtype=torch.float64)[perm])
        cell.weight_hh.zero_()
        h1, c1 = cell(torch.from_numpy(x + gp), (torch.zeros(3, Hd, dtype=torch.float64), torch.from_numpy(c)))
    rc, rh = S.lstm_update(x, gp, c)
    np.testing.assert_allclose(rc, c1.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(rh, h1.numpy(), rtol=1e-12, atol=1e-14)
    zc, _ = S.lstm_update(None, gp, c, zero_c=True)
    np.testing.assert_allclose(zc, S.lstm_update(None, gp, np.zeros_like(c))[0])
    np.testing.assert_array_equal(S.xg_rows_of(x, [0, 2, 3]), np.stack([np.zeros(4 * Hd), x[1], x[2]]))


# ---- wrong variants ----------------------------------------------------------------------------------------------------------------
def _last_max_partials(z, an, slots):
    p = S.slotted(z, an, slots)
    j = 31 - p[:, :, ::-1].argmax(2)
    has = (p > -np.inf).any(2)
    col = np.where(has, 32 * np.arange(slots)[None, :] + j, S.NO_COL).astype(np.int32)
    return p.max(2), col


def _ge_merge(val, col):
    """A merge that lets a later entry replace an equal one."""
    tok = np.zeros(len(val), np.int64)
    for m in range(len(val)):
        best, bi = -np.inf, S.NO_COL
        for s in range(val.shape[1]):
            if col[m, s] != S.NO_COL and (bi == S.NO_COL or val[m, s] >= best):
                best, bi = val[m, s], col[m, s]
        tok[m] = 0 if bi == S.NO_COL else bi + 1
    return tok


def _sentinel_is_a_column(val, col):
    """A merge that drops the sentinel test: a row of sentinels decodes to column 0x7fffffff & (slots - 1), an address."""
    col0 = np.where(col == S.NO_COL, 0, col)
    return np.where(np.isneginf(val).all(1), col0[:, 0] + 1, S.row_merge(val, col0)[0])


def _tie_case(name, K=32):
    cols = S.TIE_SETS[name]
    V1 = max(cols) + 40
    A, W, b = S.tie_operands(cols, 3, V1, K, seed=len(name) + V1)
    return cols, V1, S.host_logits(A, W, b)


@pytest.mark.parametrize("name", ["c0_1", "c3_4", "c7_8", "c3_4_64"])
def test_last_maximum_is_rejected_inside_a_slot(name):
    cols, V1, z = _tie_case(name)
    slots = S.slots_of(V1)
    val, col = S.argmax_partials(z, V1, slots)
    assert (col[:, 0] == cols[0]).all() and (S.row_merge(val, col)[0] == cols[0] + 1).all()
    wv, wc = _last_max_partials(z, V1, slots)
    np.testing.assert_array_equal(wv, val)                                   # the values cannot tell
    assert (wc[:, 0] != col[:, 0]).all()


@pytest.mark.parametrize("name", ["c31_32", "c63_64", "c0_2048", "c5_8197", "c3_4_64"])
def test_ge_merge_is_rejected_between_slots(name):
    cols, V1, z = _tie_case(name)
    val, col = S.argmax_partials(z, V1, S.slots_of(V1))
    tok, _ = S.row_merge(val, col)
    assert (tok == cols[0] + 1).all()
    assert (_ge_merge(val, col) == cols[-1] + 1).all()


def test_sentinel_read_as_column_zero_is_rejected():
    val = np.full((2, 4), -np.inf, np.float32)
    col = np.full((2, 4), S.NO_COL, np.int32)
    val[1, 2], col[1, 2] = 1.5, 70
    np.testing.assert_array_equal(S.row_merge(val, col)[0], [0, 71])
    assert _sentinel_is_a_column(val, col)[0] == 1                           # a word where the row has none


@pytest.mark.parametrize("V1", [1, 33, 97, 8257])
def test_padding_column_in_the_sum_is_rejected_by_the_bound_and_passed_by_the_model_bar(V1):
    """A mask off by one lets the first padding column (logit 0: zero weights, no bias) into its slot's sum.  On near-uniform
    logits that moves a step's lse by about 1 / (V1 + 1) -- at model vocabularies under the 1e-4 relative bar on a caption's
    log-likelihood of about ln(V1) per step -- while the slot's own sum leaves the kernel test's bound by orders of magnitude."""
    z = (np.random.default_rng(V1).standard_normal((4, V1)) * 0.05).astype(np.float32)      # what synthetic weights give
    cols = (V1 + 63) // 64 * 64
    assert cols > V1 and V1 % 32                                             # a padding column in a slot that has a real one
    slots = S.slots_of(cols)
    mx, s = S.lse_partials(z, V1, slots)
    zp = np.zeros((4, cols), np.float32)
    zp[:, :V1] = z
    wmx, ws = S.lse_partials(zp, V1 + 1, slots)
    hit = V1 // 32
    err = np.abs(ws - s)[:, hit]
    bound = S.lse_sum_bound(z, V1, slots, S.U_EXP)[:, hit]
    assert (err > 1000 * bound).all(), (err, bound)
    other = np.delete(np.arange(slots), hit)
    np.testing.assert_array_equal(ws[:, other], s[:, other])
    if V1 == 8257:
        lp = S.target_logit(z, np.ones(4, np.int32)) - S.lse_rows(mx, s)
        wlp = S.target_logit(z, np.ones(4, np.int32)) - S.lse_rows(wmx, ws)
        assert (wlp != lp).all() and (np.abs(wlp - lp) <= 1e-4 * np.abs(lp)).all()     # the whole-model bar does not see it


def test_noise_per_column_is_rejected():
    """One Philox call serves a run of four columns (word n & 3 of counter n >> 2).  A kernel that calls once per column
    (counter n, word 0) draws other noise for every column but 0."""
    from tests import sample_restatement as R
    V1, t, seed = 97, 2, 11
    z = np.zeros((5, V1), np.float32)                                        # flat logits: the noise alone decides
    slots = S.slots_of(V1)
    per_column = lambda seed, s, r, t, v: R.philox4x32_10(np.asarray(v, np.uint32), np.asarray(t, np.uint32),
                                                          np.asarray(r, np.uint32), np.asarray(s, np.uint32),
                                                          int(seed) & 0xffffffff, int(seed) >> 32)[0]
    good = S.sample_partials(z, V1, slots, KEYS, t, seed, 1.0)
    bad = S.sample_partials(z, V1, slots, KEYS, t, seed, 1.0, bits=per_column)
    assert (good[3] != bad[3]).mean() > 0.5
    assert (S.row_merge(good[2], good[3])[0] != S.row_merge(bad[2], bad[3])[0]).any()


def test_lse_bound_holds_a_float32_evaluation():
    """An fp32 evaluation in the kernel's order of operations (numpy's exp in the place of the hardware's) sits inside the bound at
    the u the device test uses: the bound is no tighter than fp32 arithmetic allows."""
    z = _random_z(64, 97, 12, scale=4.0)
    slots = S.slots_of(97)
    mx, s = S.lse_partials(z, 97, slots)
    p = S.slotted(z, 97, slots)
    with np.errstate(invalid="ignore"):
        d = (p - mx[..., None]).astype(np.float32)
        e = np.where(p > -np.inf, np.exp((d * np.float32(1.4426950408889634)).astype(np.float32).astype(np.float64) * np.log(2.0)), 0.0)
    acc = np.zeros(e.shape[:2], np.float32)
    for k in range(32):
        acc = (acc + e[..., k].astype(np.float32)).astype(np.float32)
    live = mx > -np.inf
    ratio = (np.abs(acc.astype(np.float64) - s)[live] / S.lse_sum_bound(z, 97, slots, S.U_EXP)[live]).max()
    assert ratio <= 1.0, ratio


# ---- the hooks' header ------------------------------------------------------------------------------------------------------------
def _declared_symbols(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def test_hook_header_symbols_are_exported_and_off_the_boundary():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_step.h")
    assert sorted(hooks) == sorted(_lib._STEP_HOOK_SIGS) and len(hooks) == 2
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    assert not [h for h in hooks if h in open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
    for other in ("densecap_debug.h", "densecap_debug_grad.h", "densecap_debug_recog.h", "densecap_debug_bwd.h",
                  "densecap_debug_sample.h", "densecap_debug_beam.h", "densecap_debug_rpn.h", "densecap_debug_optim.h"):
        assert not set(hooks) & set(_declared_symbols(other)), other


def test_struct_bindings_mirror_the_header():
    from densecap_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap_debug_step.h")).read(), flags=re.S)
    for name, cls in (("dc_step_gemm", _lib.DcStepGemm), ("dc_step_tail", _lib.DcStepTail)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f for f, _ in cls._fields_], name
