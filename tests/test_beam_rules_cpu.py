"""The reference and the rule of tests/test_gpu_beam.py, checked without a GPU (tests/beam_rules.py).

  * the step-wise restatements, chained from the oracle's start state, are oracle.lm_beamsearch token for token at beams 1, 5,
    20 and 32 -- so a device step checked against them is checked against the oracle;
  * the rank-wise rule accepts another arithmetic on the same inputs (every step recomputed in float64) at all four beams, with
    no row, step or rank left out, and rejects three seeded errors applied to that stand-in: a swapped pair with a gap of 1e-3,
    a parent off by one, an unmasked finished row;
  * the four hooks are exported and their header prototypes are the ctypes signatures of densecap_amd/_lib.py.

Measured with the float64 stand-in at beam 32 (7 steps, 70 proposals): 7547 live lists, worst value difference 1.9e-6, worst
rank slack 4.8e-7 against TOKEN_TOL = 2e-5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import beam_rules as R
from tests import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAMS = (1, 5, 20, 32)
N, T, V = 70, 7, 300


@pytest.fixture(scope="module")
def weights():
    from densecap_amd.weights import make_synthetic_weights
    parity.oracle_threads()
    return make_synthetic_weights(seed=5, vocab_size=V, seq_length=T)


_WALKS = {}


def _walk(weights, beam):
    """(codes, oracle_walk) of a beam, computed once and left unchanged."""
    if beam not in _WALKS:
        codes = np.maximum(np.random.default_rng(beam).standard_normal((N, 4096)), 0).astype(np.float32)
        _WALKS[beam] = (codes, R.oracle_walk(codes, weights, T, beam))
    return _WALKS[beam]


@pytest.mark.parametrize("beam", BEAMS)
def test_chained_restatements_are_the_oracle(weights, beam):
    import torch
    from oracle import densecap_oracle as O
    codes, walk = _walk(weights, beam)
    want = O.lm_beamsearch(torch.from_numpy(codes), weights, T, beam)
    np.testing.assert_array_equal(walk["seq"], want)
    assert sorted(walk["steps"]) == list(range(1, T))
    # the walk is a chain: what a step hands on is what the next one reads
    for t in range(1, T - 1):
        assert walk["steps"][t]["next"] is walk["steps"][t + 1]["state"]


def _stand_in_checked(weights, beam, mutate=None):
    """Every step of every proposal recomputed in float64 from the oracle's state and put through the rule, as the GPU test
    puts the device through it.  mutate(t, state, lists, merged, gathered) may damage the stand-in's outputs first."""
    _, walk = _walk(weights, beam)
    worst_val = worst_slack = 0.0
    lists = 0
    for t in range(1, T):
        st = walk["steps"][t]
        state = st["state"]
        top_lp, top_idx, h2, c2 = R.float64_step(state, weights, beam)
        merged = R.merge_ref(top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1)
        par = merged["parent"][:, :, None].astype(np.int64)
        gathered = dict(h=np.take_along_axis(h2, par, 1), c=np.take_along_axis(c2, par, 1))
        if mutate is not None:
            top_lp, top_idx = top_lp.copy(), top_idx.copy()
            mutate(t, state, top_lp, top_idx, merged, gathered)
        what = "beam %d step %d" % (beam, t)
        v, s, n = R.check_lists(top_lp.reshape(N * beam, beam), top_idx.reshape(N * beam, beam), st["lp"], state["fin"],
                                parity.TOKEN_TOL, what)
        R.check_merge(merged, top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1, what)
        R.check_gather(gathered["h"], gathered["c"], merged["parent"], st["h_post"], st["c_post"], parity.REL, what)
        worst_val, worst_slack, lists = max(worst_val, v), max(worst_slack, s), lists + n
    return worst_val, worst_slack, lists


@pytest.mark.parametrize("beam", BEAMS)
def test_rule_accepts_another_arithmetic(weights, beam):
    v, s, n = _stand_in_checked(weights, beam)
    print("beam %d: %d live lists, worst value difference %.3g, worst rank slack %.3g, excused 0" % (beam, n, v, s))
    assert n > 0 and v <= parity.TOKEN_TOL and s <= 2 * parity.TOKEN_TOL


def _live_row_with_gap(state, top_lp, gap):
    """(proposal, beam, rank q) of a live list whose entries q and q + 1 are at least `gap` apart."""
    d = top_lp[:, :, :-1].astype(np.float64) - top_lp[:, :, 1:]
    ok = (d >= gap) & (state["fin"] == 0)[:, :, None]
    assert ok.any()
    return tuple(np.argwhere(ok)[0])


@pytest.mark.parametrize("beam", (5, 32))
def test_rule_rejects_a_swapped_pair(weights, beam):
    """Two neighbours of a list 1e-3 apart change places: as whole entries (the order is wrong), as words only (the values no
    longer belong to the words), and a word replaced by one 1e-3 below the entry of its rank (values adjusted to match)."""
    def whole(t, state, top_lp, top_idx, merged, gathered):
        if t == 1:
            p, b, q = _live_row_with_gap(state, top_lp, 1e-3)
            top_lp[p, b, [q, q + 1]] = top_lp[p, b, [q + 1, q]]
            top_idx[p, b, [q, q + 1]] = top_idx[p, b, [q + 1, q]]
            merged.update(R.merge_ref(top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1))

    def words(t, state, top_lp, top_idx, merged, gathered):
        if t == 1:
            p, b, q = _live_row_with_gap(state, top_lp, 1e-3)
            top_idx[p, b, [q, q + 1]] = top_idx[p, b, [q + 1, q]]
            merged.update(R.merge_ref(top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1))

    def wrong_pick(t, state, top_lp, top_idx, merged, gathered):
        if t == 1:
            _, walk = _walk(weights, beam)
            lp = walk["steps"][1]["lp"]
            p, b = np.argwhere(state["fin"] == 0)[0]
            order = np.argsort(-lp[p, b].astype(np.float64), kind="stable")
            q = beam - 1
            j = next(int(i) for i in order[beam:] if lp[p, b, order[q]] - lp[p, b, i] >= 1e-3)
            top_idx[p, b, q] = j + 1
            top_lp[p, b, q] = lp[p, b, j]
            merged.update(R.merge_ref(top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1))

    for mutate, msg in ((whole, "values increase"), (words, "difference"), (wrong_pick, "the entry of that rank")):
        with pytest.raises(AssertionError, match=msg):
            _stand_in_checked(weights, beam, mutate)


@pytest.mark.parametrize("beam", (5, 32))
def test_rule_rejects_a_parent_off_by_one(weights, beam):
    """The merge reports the neighbour of the parent it took: in the merge outputs alone, and carried into the beams and the
    state consistently (the state then belongs to another beam)."""
    def parent_only(t, state, top_lp, top_idx, merged, gathered):
        if t == 2:
            merged["parent"] = (merged["parent"] + 1) % beam

    with pytest.raises(AssertionError, match="parent differs"):
        _stand_in_checked(weights, beam, parent_only)

    def state_only(t, state, top_lp, top_idx, merged, gathered):
        if t == 2:
            gathered["h"] = np.roll(gathered["h"], 1, axis=1); gathered["c"] = np.roll(gathered["c"], 1, axis=1)

    with pytest.raises(AssertionError, match="same parent differ|state after the step"):
        _stand_in_checked(weights, beam, state_only)


@pytest.mark.parametrize("beam", (5, 32))
def test_rule_rejects_an_unmasked_finished_row(weights, beam):
    """A finished row goes through the top-k as a live one."""
    seen = []

    def unmask(t, state, top_lp, top_idx, merged, gathered):
        f = np.argwhere(state["fin"] != 0)
        if len(f) and not seen:
            seen.append(t)
            p, b = f[0]
            live = dict(state, fin=np.zeros_like(state["fin"]))
            lp, ix, _, _ = R.float64_step(live, weights, beam)
            top_lp[p, b], top_idx[p, b] = lp[p, b], ix[p, b]
            merged.update(R.merge_ref(top_lp, top_idx, state["beam_lp"], state["beams"], t, V + 1))

    with pytest.raises(AssertionError, match="a finished row"):
        _stand_in_checked(weights, beam, unmask)
    assert seen, "no finished row on the trajectory: the case is not exercised"


def test_merge_ref_planted_cases():
    """merge_ref on a case small enough to do by hand: ties go to the lower flat index, a finished parent's candidates all tie at
    its own log-probability, END at column t and END already in the row both finish the beam."""
    END = 9
    top_lp = np.array([[[-1.0, -2.0], [0.0, 0.0]]], np.float32)               # beam 1 is finished: zeros, words 1, 2
    top_idx = np.array([[[4, END], [1, 2]]], np.int32)
    beam_lp = np.array([[-0.5, -1.5]], np.float32)
    beams = np.array([[[3, 1, 1], [END, 1, 1]]], np.int32)
    out = R.merge_ref(top_lp, top_idx, beam_lp, beams, 1, END)
    # candidates: -1.5 (b0, 4), -2.5 (b0, END), -1.5 (b1, 1), -1.5 (b1, 2): the tie at -1.5 goes to flat 0, then flat 2
    np.testing.assert_array_equal(out["beam_lp"], np.array([[-1.5, -1.5]], np.float32))
    np.testing.assert_array_equal(out["parent"], [[0, 1]])
    np.testing.assert_array_equal(out["beams"], [[[3, 4, 1], [END, 1, 1]]])
    np.testing.assert_array_equal(out["tok"], [[4, 1]])
    np.testing.assert_array_equal(out["fin"], [[0, 1]])


# ---- the hooks' declarations ---------------------------------------------------------------------------------------------------
HOOKS = ("dc_debug_beam_merge", "dc_debug_beam_start", "dc_debug_beam_step", "dc_debug_beam_topk")


def _ctype_of(decl):
    """The ctypes type _lib.py uses for a C parameter declaration of the debug header."""
    from densecap_amd import _lib
    t = re.sub(r"\b(const)\b", "", decl).strip()
    t = re.sub(r"\s*\*\s*", "* ", t)
    base = t.rsplit(" ", 1)[0].strip() if not t.endswith("*") else t       # drop the parameter name
    if base == "dc_beam_state*":
        return C.POINTER(_lib.DcBeamState)
    if base.endswith("*"):
        assert base[:-1].strip() in ("dc_ctx", "float", "int32_t", "uint8_t"), decl
        return C.c_void_p
    assert base == "int", decl
    return C.c_int


def test_hooks_are_exported_with_the_header_prototypes():
    from densecap_amd import _lib
    from tests.test_abi_and_host import DEBUG_SYMBOLS, _prototypes
    hdr = open(os.path.join(ROOT, "include", "densecap_debug.h")).read()
    protos = _prototypes(hdr)
    lib = _lib.lib()
    for name in HOOKS:
        assert name in DEBUG_SYMBOLS and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.fullmatch(r"int %s\((.*)\)" % name, protos[name])
        assert m, protos[name]
        want = [_ctype_of(a) for a in m.group(1).split(",")]
        res, args = _lib._SIGS[name]
        assert res is C.c_int and args == want, (name, args, want)
    assert DEBUG_SYMBOLS == sorted(DEBUG_SYMBOLS)
    # not part of the boundary: neither header nor the LuaJIT binding knows the hooks
    for f in ("include/densecap.h", "lua/densecap_hip.lua"):
        txt = open(os.path.join(ROOT, f)).read()
        assert "dc_debug_beam" not in txt and "dc_beam_state" not in txt, f
    # dc_beam_state: the fields of the header, in order, all device pointers
    body = re.search(r"typedef struct dc_beam_state \{(.*?)\} dc_beam_state;", hdr, flags=re.S).group(1)
    fields = [d.split("*")[-1].strip() for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _lib.DcBeamState._fields_] == list(__import__("densecap_amd.ops", fromlist=["x"]).BEAM_STATE_FIELDS)
    assert all(t is C.c_void_p for _, t in _lib.DcBeamState._fields_)
