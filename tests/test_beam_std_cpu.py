"""The reference and the rules of tests/test_gpu_beam_std.py, checked without a GPU (tests/beam_std_rules.py).

  * the fixture does what the GPU tests need of it: finished and live hypotheses side by side, hypotheses of every length, a
    length penalty that reorders -- asserted as conditions, so that the GPU tests cannot pass on a fixture where nothing finishes;
  * std_walk at B = 1, alpha 0 is oracle.lm_sample up to every row's first END; a finished hypothesis's lp is the teacher-forced
    score of its caption (tests/score_restatement.py) and its bits never change once it has finished;
  * the step rules accept another arithmetic on the same inputs (every step recomputed in float64) and reject three wrong
    searches: h seeded from c, a finished parent that contributes B candidates, columns without a word that are not 0;
  * check_beam_args accepts and refuses what the library does; header, cdef and ctypes agree on the new entry points.

Measured on the fixture in fp32 (24 proposals, T = 15): B = 4: 24 proposals mixed at some step, 77 hypotheses finished and 19 live
at the end, lengths 1..15, alpha 1 reorders 22 proposals; B = 8: 24 mixed, 153 finished."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import beam_rules as R
from tests import beam_std_rules as S
from tests import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 1e-4                     # the scorer's bound (docs/SEMANTICS.md, "Scoring captions")
V, T, N = S.FIX_V, S.FIX_T, S.FIX_N
END = V + 1


@pytest.fixture(scope="module")
def fix():
    parity.oracle_threads()
    return S.fixture()


def _mixed(walk):
    m = np.zeros(N, bool)
    for st in walk["steps"].values():
        f = st["state"]["fin"].astype(bool)
        m |= f.any(axis=1) & ~f.all(axis=1)
    return m


def test_fixture_exercises_the_new_rules(fix):
    w = S.fixture_walk(4)
    fin = w["final"]["fin"].astype(bool)
    c0, _ = S.std_search(w, 4, 0.0)
    c1, _ = S.std_search(w, 4, 1.0)
    reordered = sum(bool((c0[i] != c1[i]).any()) for i in range(N))
    ln = w["final"]["len"]
    print("B = 4: mixed %d, finished %d, live %d, lengths %d..%d, alpha 1 reorders %d" % (
        _mixed(w).sum(), fin.sum(), (~fin).sum(), ln.min(), ln.max(), reordered))
    assert _mixed(w).sum() >= 12
    assert fin.sum() >= 24 and (~fin).sum() >= 5
    assert reordered >= 12
    assert ln.min() == 1 and ln.max() == T
    w8 = S.fixture_walk(8)
    assert _mixed(w8).sum() >= 12 and w8["final"]["fin"].sum() >= 48
    # the edge of every selection is clear of the rank-wise tolerance: the smallest gap between the last candidate taken and the
    # first one left is well above 2 x TOKEN_TOL, so the device's trajectory is the reference's
    for beam, walk in ((4, w), (8, w8)):
        worst = np.inf
        for t, st in walk["steps"].items():
            f = st["state"]; pf = f["fin"].astype(bool)
            cand = np.where(pf[:, :, None], f["beam_lp"][:, :, None], st["top_lp"] + f["beam_lp"][:, :, None]).astype(np.float64)
            cand[np.broadcast_to(pf[:, :, None], cand.shape) & (np.arange(beam)[None, None, :] > 0)] = -np.inf
            srt = -np.sort(-cand.reshape(N, -1), axis=1)
            gap = srt[:, beam - 1] - srt[:, beam]
            worst = min(worst, gap[np.isfinite(gap)].min())
        print("B = %d: smallest gap at the edge of a selection %.3g" % (beam, worst))
        assert worst > 4 * parity.TOKEN_TOL


def test_width_one_is_the_greedy_caption(fix):
    import torch
    from oracle import densecap_oracle as O
    W, codes = fix
    seq = O.lm_sample(torch.from_numpy(codes), W, T)
    caps, lp = S.std_search(S.fixture_walk(1), 1, 0.0)
    ended = 0
    for i in range(N):
        e = np.nonzero(seq[i] == END)[0]
        n = e[0] + 1 if len(e) else T
        ended += bool(len(e))
        np.testing.assert_array_equal(caps[i, 0, :n], seq[i, :n])
        assert (caps[i, 0, n:] == 0).all()
    assert ended >= 12 and np.isfinite(lp).all()


def test_finished_logprob_is_the_teacher_forced_score(fix):
    from tests import score_restatement
    W, codes = fix
    w = S.fixture_walk(4)
    f = w["final"]
    checked = 0
    worst = 0.0
    for i in range(N):
        done = np.nonzero(f["fin"][i])[0]
        if len(done) == 0:
            continue
        rows = f["beams"][i, done]
        assert ((rows == END).sum(axis=1) == 1).all()
        q = np.where(rows == END, 0, rows)
        assert (np.cumsum(q == 0, axis=1)[q != 0] == 0).all(), "a word after END"
        want = score_restatement.lm_score(codes[i:i + 1], W, q)[0]
        d = np.abs(f["beam_lp"][i, done].astype(np.float64) - want)
        worst = max(worst, d.max())
        checked += len(done)
        assert (f["len"][i, done] == (rows != 0).sum(axis=1)).all()
    print("%d finished hypotheses, worst |lp - score| %.3g (bound %.3g)" % (checked, worst, STAGE))
    assert checked >= 24 and worst <= STAGE


@pytest.mark.parametrize("beam", [4, 8])
def test_a_finished_hypothesis_keeps_its_bits(fix, beam):
    w = S.fixture_walk(beam)
    kept = 0
    for t, st in w["steps"].items():
        fed, nxt = st["state"], st["next"]
        pf = np.take_along_axis(fed["fin"], nxt["parent"].astype(np.int64), 1).astype(bool)
        plp = np.take_along_axis(fed["beam_lp"], nxt["parent"].astype(np.int64), 1)
        prow = np.take_along_axis(fed["beams"], nxt["parent"][:, :, None].astype(np.int64), 1)
        plen = np.take_along_axis(fed["len"], nxt["parent"].astype(np.int64), 1)
        assert (nxt["beam_lp"].view(np.uint32)[pf] == plp.view(np.uint32)[pf]).all()
        assert (nxt["beams"][pf] == prow[pf]).all() and (nxt["beams"][pf][:, t] == 0).all()
        assert (nxt["len"][pf] == plen[pf]).all() and nxt["fin"][pf].all()
        # a finished parent is selected at most once
        for p in range(N):
            chosen = nxt["parent"][p][pf[p]]
            assert len(set(chosen.tolist())) == len(chosen)
        kept += int(pf.sum())
        # all finished: the proposal is unchanged
        allf = fed["fin"].all(axis=1)
        for k in ("beam_lp", "beams", "len", "fin"):
            assert (R._bits(nxt[k][allf]) == R._bits(fed[k][allf])).all(), k
    assert kept >= 100


def _run_rules(walk, stand_in, beam):
    """Every step of `stand_in` (a walk, or None = every step recomputed in float64 from the reference's state) against the
    reference walk's trajectory."""
    W, _ = S.fixture()
    worst_v = worst_s = 0.0
    lists = 0
    if stand_in is not None:
        from oracle import densecap_oracle as O
        tl, order = O._topk_sorted(stand_in["lp0"], beam)
        S.check_start(stand_in["first"], tl, (order + 1).astype(np.int32), walk, T, END, parity.TOKEN_TOL, parity.REL, "start")
    for t in range(1, T):
        st = walk["steps"][t]
        fed = st["state"]
        what = "beam %d step %d" % (beam, t)
        if stand_in is None:
            top_lp, top_idx, h2, c2 = R.float64_step(fed, W, beam)
            out = S.std_merge_ref(top_lp, top_idx, fed["beam_lp"], fed["beams"], fed["len"], fed["fin"], t, END)
            par = out["parent"][:, :, None].astype(np.int64)
            out["h"] = np.take_along_axis(h2, par, 1); out["c"] = np.take_along_axis(c2, par, 1)
        else:
            # the wrong search's own step on its own state: the merge rule is checked on the step's own inputs
            ws = stand_in["steps"][t]
            fed, out, top_lp, top_idx = ws["state"], ws["next"], ws["top_lp"], ws["top_idx"]
            st = ws
        v, s, n = S.check_step(out, top_lp, top_idx, fed, st, t, END, parity.TOKEN_TOL, parity.REL, what)
        worst_v, worst_s, lists = max(worst_v, v), max(worst_s, s), lists + n
    return worst_v, worst_s, lists


@pytest.mark.parametrize("beam", [1, 4, 8])
def test_rules_accept_another_arithmetic(fix, beam):
    v, s, n = _run_rules(S.fixture_walk(beam), None, beam)
    print("beam %d: %d live lists, worst value difference %.3g, worst rank slack %.3g, excused 0" % (beam, n, v, s))
    assert n > 0 and v <= parity.TOKEN_TOL and s <= 2 * parity.TOKEN_TOL


def test_rules_accept_the_reference_itself(fix):
    _run_rules(S.fixture_walk(4), S.fixture_walk(4), 4)


@pytest.mark.parametrize("variant,match", [("h_from_c", "state after the step"), ("flood", "differs"), ("ones", "beams differs")])
def test_rules_reject_a_wrong_search(fix, variant, match):
    W, codes = fix
    wrong = S.std_walk(codes, W, T, 4, variant=variant)
    with pytest.raises(AssertionError, match=match):
        _run_rules(S.fixture_walk(4), wrong, 4)


def test_merge_ref_on_hand_made_cases():
    """A finished parent whose lp ties a live candidate: the lower flat index first; every sum equal: flat order; sums all NaN:
    no word, NaN, finished, the rows kept."""
    B, Tt = 3, 5
    top_lp = np.full((1, B, B), -1.0, np.float32); top_idx = np.tile(np.arange(2, 2 + B, dtype=np.int32), (1, B, 1))
    beam_lp = np.array([[-1.0, -2.0, -2.0]], np.float32)
    beams = np.zeros((1, B, Tt), np.int32); beams[0, :, 0] = (7, 9, 8); beams[0, 1, 0] = 11
    length = np.ones((1, B), np.int32); fin = np.array([[0, 1, 0]], np.uint8)
    out = S.std_merge_ref(top_lp, top_idx, beam_lp, beams, length, fin, 1, 11)
    # candidates: (0, j) = -2 at flat 0..2, (1, 0) = -2 at flat 3 (finished), (2, j) = -3: picks flat 0, 1, 2
    assert out["parent"].tolist() == [[0, 0, 0]] and out["tok"].tolist() == [[2, 3, 4]]
    beam_lp = np.array([[-2.0, -1.0, -2.0]], np.float32)
    out = S.std_merge_ref(top_lp, top_idx, beam_lp, beams, length, fin, 1, 11)
    # the finished parent (-1) first, once; then flat 0, 1 (-3) before flat 6.. (-3)
    assert out["parent"].tolist() == [[1, 0, 0]] and out["beams"][0, 0].tolist() == [11, 0, 0, 0, 0]
    assert out["fin"].tolist() == [[1, 0, 0]] and out["len"].tolist() == [[1, 2, 2]] and out["tok"].tolist() == [[1, 2, 3]]
    assert out["beam_lp"].view(np.uint32)[0, 0] == beam_lp.view(np.uint32)[0, 1]
    out = S.std_merge_ref(top_lp * np.nan, top_idx, beam_lp * np.nan, beams, length, fin, 1, 11)
    assert np.isnan(out["beam_lp"]).all() and out["parent"].tolist() == [[0, 1, 2]] and out["fin"].all()
    assert (out["beams"][:, :, 1] == 0).all() and out["len"].tolist() == [[1, 1, 1]] and (out["tok"] == 1).all()


def test_finish_ref_and_its_rule():
    rng = np.random.default_rng(3)
    B, Tt = 5, 6
    lp = -np.sort(rng.random((4, B)).astype(np.float32) * 8, axis=1)
    length = rng.integers(1, Tt + 1, (4, B)).astype(np.int32)
    beams = np.zeros((4, B, Tt), np.int32)
    for p in range(4):
        for b in range(B):
            beams[p, b, :length[p, b]] = rng.integers(1, 9, length[p, b])
    lp[1, 2] = np.nan
    lp[2, 3] = lp[2, 1]; length[2, 3] = length[2, 1]                   # equal scores: hypothesis order
    caps, out = S.std_finish_ref(lp, beams, length, B, 0.0)
    assert (caps[0] == beams[0]).all() and (caps[1, 2] == 0).all() and np.isnan(out[1, 2])
    for a in (0.5, 1.0, 2.0):
        caps, out = S.std_finish_ref(lp, beams, length, B, a)
        assert np.isnan(out[1, -1]) and (caps[1, -1] == 0).all()
        sc = S.std_scores(out, (caps != 0).sum(axis=2), Tt, a)
        assert (np.diff(sc[0].astype(np.float64)) <= 0).all()
        S.check_finish(caps, out, lp, beams, length, B, a, "ref alpha %g" % a)
        i1 = [r for r in range(B) if (caps[2, r] == beams[2, 1]).all()][0]
        assert (caps[2, i1 + 1] == beams[2, 3]).all()
        # a wrong pick does not pass: the two ends of the ranking change places
        bad_c, bad_l = caps.copy(), out.copy()
        bad_c[0, [0, -1]] = caps[0, [-1, 0]]; bad_l[0, [0, -1]] = out[0, [-1, 0]]
        with pytest.raises(AssertionError):
            S.check_finish(bad_c, bad_l, lp, beams, length, B, a, "swapped")
    assert S.pen_table(15, 0.7)[15] == np.float32(15.0 ** float(np.float32(0.7)))


def test_check_beam_args():
    from densecap_amd import ops
    from densecap_amd.model import DenseCapModel

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was reached: %s" % name)

    o = ops.check_beam_args(5)
    assert (o.beam_size, o.n_best, o.length_alpha) == (5, 5, 0.0)
    o = ops.check_beam_args(32, 7, 2.0, vocab_size=200)
    assert (o.beam_size, o.n_best, o.length_alpha) == (32, 7, 2.0)
    assert ops.check_beam_args(1, 1, 0.7).length_alpha == np.float32(0.7)
    bad = [dict(beam_size=0), dict(beam_size=33), dict(beam_size=-1), dict(beam_size=2.5), dict(beam_size=None),
           dict(beam_size=4, n_best=0), dict(beam_size=4, n_best=5), dict(beam_size=4, n_best=1.5),
           dict(beam_size=4, length_alpha=-0.1), dict(beam_size=4, length_alpha=2.5), dict(beam_size=4, length_alpha=float("nan")),
           dict(beam_size=4, length_alpha=float("inf")), dict(beam_size=8, vocab_size=6)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.check_beam_args(**kw)
    ctx = NoLibrary()
    for kw in (dict(beam_size=0), dict(beam_size=4, n_best=5), dict(beam_size=4, length_alpha=3.0)):
        with pytest.raises(ValueError):
            ops.lm_beam_n(ctx, np.zeros((2, 8), np.float32), **kw)
        m = object.__new__(DenseCapModel)
        m.ctx = m.lib = ctx
        m.vocab_size = 200
        with pytest.raises(ValueError):
            m.beamCaptions(np.zeros((3, 8, 8), np.float32), **kw)


def test_header_cdef_and_ctypes_agree():
    from densecap_amd import _lib
    from tests.test_abi_and_host import _prototypes
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name in ("dc_beam_captions", "dc_op_lm_beam_n"):
        assert name in hp and name in _lib.EXPORTED_SYMBOLS and lp[name] == hp[name], name
    struct = r"typedef struct dc_beam_opts \{\s*int32_t beam_size; int32_t n_best; float length_alpha;\s*\} dc_beam_opts;"
    assert re.search(struct, hdr) and re.search(struct, cdef)
    assert C.sizeof(_lib.DcBeamOpts) == 12
    assert C.sizeof(_lib.DcBeamStdState) == C.sizeof(_lib.DcBeamState) + C.sizeof(C.c_void_p)
    dbg = open(os.path.join(ROOT, "include", "densecap_debug_beam.h")).read()
    dp = _prototypes(dbg)
    assert sorted(dp) == sorted(_lib._BEAM_STD_HOOK_SIGS)
    for name, (res, args) in _lib._BEAM_STD_HOOK_SIGS.items():
        assert name not in lua and name not in hdr
        assert len(args) == dp[name].count(",") + 1, name              # one ctypes argument per parameter of the prototype
    body = re.search(r"typedef struct dc_beam_std_state \{(.*?)\} dc_beam_std_state;", re.sub(r"/\*.*?\*/", "", dbg, flags=re.S),
                     flags=re.S).group(1)
    names = [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.DcBeamStdState._fields_]
    lm = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    assert "function Model:beamCaptions(input, beam_size, n_best, length_alpha)" in lm


def test_library_exports_the_entry_points():
    if not os.path.exists(os.path.join(ROOT, "densecap_amd", "lib", "libdensecap_hip.so")):
        import __graft_entry__ as g
        g.build()
    from densecap_amd import _lib
    lib = _lib.lib()
    for name in ("dc_beam_captions", "dc_op_lm_beam_n") + tuple(_lib._BEAM_STD_HOOK_SIGS):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None


def test_run_model_parser_and_up_front_checks():
    from densecap_amd import run_model
    opt = run_model.build_parser().parse_args([])
    assert (opt.num_beams, opt.n_best, opt.length_alpha) == (0, 0, 0.0)
    opt = run_model.build_parser().parse_args(["-num_beams", "3", "-n_best", "2", "-length_alpha", "0.7"])
    assert (opt.num_beams, opt.n_best, opt.length_alpha) == (3, 2, 0.7)
    assert set(run_model.BEAM_FLAGS) == {"num_beams", "n_best", "length_alpha"}
    assert not set(run_model.BEAM_FLAGS) & set(run_model.SAMPLING_FLAGS)
    base = ["-synthetic_weights", "1", "-input_dir", ROOT]
    for extra, word in ((["-num_beams", "40"], "beam_size"), (["-num_beams", "3", "-n_best", "4"], "n_best"),
                        (["-num_beams", "3", "-length_alpha", "2.5"], "length_alpha"),
                        (["-num_beams", "3", "-num_samples", "2"], "-num_samples"),
                        (["-num_beams", "3", "-input_boxes", "x.json"], "-input_boxes"), (["-n_best", "2"], "-num_beams")):
        with pytest.raises(SystemExit) as e:
            run_model.main(base + extra)
        assert word in str(e.value), (extra, e.value)
