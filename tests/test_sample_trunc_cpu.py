"""Truncated caption sampling, the parts that need no GPU: the float64 restatement (tests/sample_trunc_rules.py) and its
properties, the decision rule and its teeth -- five wrong samplers must each fail it on the restatement's own scores -- the
ABI surface, and the refusals of the Python / CLI surface."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    codes = (np.random.default_rng(1).standard_normal((12, W["fc7_w"].shape[0])) * 2).astype(np.float32)
    return W, codes


@pytest.fixture(scope="module")
def base(model):
    """One run of the restatement that several tests share: (40, 0.9) at temperature 1, 12 codes x 4 draws x 6 steps."""
    from tests import sample_trunc_rules as TR
    W, codes = model
    return TR.lm_sample_n_trunc(codes, W, 4, temperature=1.0, seed=7, top_k=40, top_p=0.9, steps=6)


# ---- the kept set -----------------------------------------------------------------------------------------------------------
def test_kept_set_is_a_minimal_prefix_of_the_rank_order():
    from tests import sample_trunc_rules as TR
    rng = np.random.default_rng(0)
    for V1, k, p, temp in ((33, 0, 0.9, 1.0), (201, 40, 0.5, 0.5), (201, 7, 1.0, 2.0), (500, 0, 0.95, 1.0), (64, 64, 0.3, 0.1)):
        for _ in range(20):
            x = (rng.standard_normal(V1) * 3).astype(np.float32)
            x[rng.integers(0, V1, 5)] = x[0]                      # some exact ties
            kept, order, C, Z, pp = TR.kept_set(x, temp, k, p, detail=True)
            np.testing.assert_array_equal(kept, order[:len(kept)])                 # a prefix of the rank order
            xs = x[order].astype(np.float64)
            assert (np.diff(xs) <= 0).all()
            same = np.nonzero(np.diff(xs) == 0)[0]
            assert (order[same] < order[same + 1]).all()                            # the lower column first among equals
            K = min(k, V1) if k else V1
            assert 1 <= len(kept) <= K
            if p < 1.0:
                m = len(kept)
                assert C[m - 1] >= pp * Z and (m == 1 or C[m - 2] < pp * Z)         # the smallest prefix that reaches p Z
            else:
                assert len(kept) == K


def test_kept_set_edges():
    from tests import sample_trunc_rules as TR
    x = np.array([0.5, np.nan, 2.0, -np.inf, 2.0, 1.0], np.float32)
    np.testing.assert_array_equal(TR.rank_order(x), [2, 4, 5, 0, 3])
    np.testing.assert_array_equal(TR.kept_set(x, 1.0, 3, 1.0), [2, 4, 5])
    np.testing.assert_array_equal(TR.kept_set(x, 1.0, 6, 1.0), [2, 4, 5, 0, 3])     # top_k beyond the candidates: all of them
    np.testing.assert_array_equal(TR.kept_set(x, 1.0, 1, 1.0), [2])
    np.testing.assert_array_equal(TR.kept_set(x, 1.0, 0, 1e-6), [2])                # top_p just above 0 keeps one word
    np.testing.assert_array_equal(TR.kept_set(x, 1.0, 0, np.float32(1) - np.float32(2.0 ** -24)), [2, 4, 5, 0])   # -Inf: zero mass
    assert TR.kept_set(np.full(5, np.nan, np.float32), 1.0, 2, 0.5) is None
    assert TR.kept_set(np.array([1.0, np.inf, 0.0], np.float32), 1.0, 2, 0.5) is None
    # top-k first, the nucleus on the renormalised survivors: two equal words hold 2/3 of the top three, 1/2 of them suffices
    y = np.array([np.log(4.0), np.log(4.0), np.log(4.0), np.log(100.0)], np.float32)
    np.testing.assert_array_equal(TR.kept_set(y, 1.0, 0, 0.85), [3])
    np.testing.assert_array_equal(TR.kept_set(-y, 1.0, 3, 0.5), [0, 1])
    # the rank does not depend on the temperature
    x = np.random.default_rng(1).standard_normal(50).astype(np.float32)
    np.testing.assert_array_equal(TR.kept_set(x, 0.1, 9, 1.0), TR.kept_set(x, 2.0, 9, 1.0))


def test_top_k_one_is_the_greedy_choice_for_every_seed(model):
    from tests import sample_restatement as R
    from tests import sample_trunc_rules as TR
    W, codes = model
    greedy = R.lm_sample_n(codes[:4], W, 1, temperature=0, steps=5)
    for seed in (0, 1, 99, 2 ** 64 - 1):
        for temp in (0.5, 2.0):
            r = TR.lm_sample_n_trunc(codes[:4], W, 2, temperature=temp, seed=seed, top_k=1, steps=5)
            for s in range(2):
                np.testing.assert_array_equal(r["choice"][:, s], greedy["choice"][:, 0])
            np.testing.assert_array_equal(r["sample_logprob"], np.zeros((4, 2)))    # one word kept: probability 1


def test_no_truncation_is_the_plain_restatement_word_for_word(model):
    from tests import sample_restatement as R
    from tests import sample_trunc_rules as TR
    W, codes = model
    for temp in (0.5, 1.0):
        a = R.lm_sample_n(codes[:6], W, 3, temperature=temp, seed=5, steps=6)
        b = TR.lm_sample_n_trunc(codes[:6], W, 3, temperature=temp, seed=5, top_k=201, top_p=1.0, steps=6)
        np.testing.assert_array_equal(b["choice"], a["choice"])
        np.testing.assert_array_equal(b["samples"], a["samples"])
        np.testing.assert_allclose(b["logprob"], a["logprob"], rtol=1e-6)            # THNN's float rows against float64
        if temp == 1.0:
            np.testing.assert_allclose(b["sample_logprob"], b["logprob"], rtol=1e-12, atol=1e-12)


def test_top_p_just_above_zero_keeps_one_word(model):
    from tests import sample_restatement as R
    from tests import sample_trunc_rules as TR
    W, codes = model
    greedy = R.lm_sample_n(codes[:4], W, 1, temperature=0, steps=5)
    r = TR.lm_sample_n_trunc(codes[:4], W, 2, temperature=1.0, seed=3, top_p=1e-6, steps=5)
    for s in range(2):
        np.testing.assert_array_equal(r["choice"][:, s], greedy["choice"][:, 0])


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_the_restatement_passes_its_own_rule(model, base):
    from tests import sample_trunc_rules as TR
    total, needed = TR.check_words(base["samples"], base, 1.0, 40, 0.9, 201)
    assert total > 200 and needed == 0
    # ... and every word, run through the rule explicitly, is accepted
    for i in range(3):
        for t in range(6):
            if base["samples"][i, 0, t]:
                ok, why = TR.decide(base["scores"][i, 0, t], base["pert"][i, 0, t], base["samples"][i, 0, t], 1.0, 40, 0.9)
                assert ok, why


def _failures(model, base, chooser=None, delta=None, **other):
    """Decisions of a wrong sampler, teacher-forced on the right one's words so that every decision is made on the
    restatement's own scores, that the rule of (40, 0.9) at temperature 1 rejects."""
    from tests import sample_trunc_rules as TR
    W, codes = model
    kw = dict(top_k=40, top_p=0.9)
    kw.update(other)
    wrong = TR.lm_sample_n_trunc(codes, W, 4, temperature=1.0, seed=7, steps=6, forced=base["samples"], chooser=chooser, **kw)
    bad = total = 0
    for i in range(len(codes)):
        for s in range(4):
            for t in range(6):
                if base["samples"][i, s, t] == 0:
                    break
                total += 1
                ok, _ = TR.decide(base["scores"][i, s, t], base["pert"][i, s, t], wrong["choice"][i, s, t], 1.0, 40, 0.9,
                                  **({} if delta is None else dict(delta=delta)))
                bad += not ok
    return bad, total


def test_rule_rejects_k_plus_one_and_k_minus_one(model):
    """With top_k alone (the nucleus off) the cut sits at rank k: a sampler on k + 1 words draws the extra one, a sampler on
    k - 1 misses the k-th when it wins."""
    from tests import sample_trunc_rules as TR
    W, codes = model
    right = TR.lm_sample_n_trunc(codes, W, 8, temperature=2.0, seed=11, top_k=3, steps=6)
    for k_wrong in (4, 2):
        wrong = TR.lm_sample_n_trunc(codes, W, 8, temperature=2.0, seed=11, top_k=k_wrong, steps=6, forced=right["samples"])
        bad = 0
        for i in range(len(codes)):
            for s in range(8):
                for t in range(6):
                    if right["samples"][i, s, t] == 0:
                        break
                    ok, _ = TR.decide(right["scores"][i, s, t], right["pert"][i, s, t], wrong["choice"][i, s, t], 2.0, 3, 1.0)
                    bad += not ok
        print("top_k %d in the place of 3: %d decisions rejected" % (k_wrong, bad))
        assert bad >= 1, k_wrong


def test_rule_rejects_a_nucleus_cut_at_p_plus_002(model, base):
    bad, total = _failures(model, base, top_p=0.92)
    print("top_p 0.92 in the place of 0.9: %d of %d decisions rejected" % (bad, total))
    assert bad >= 1


def test_rule_rejects_a_sampler_that_ignores_truncation(model, base):
    bad, total = _failures(model, base, top_k=0, top_p=1.0)
    print("no truncation in the place of (40, 0.9): %d of %d decisions rejected" % (bad, total))
    assert bad >= 1


def test_rule_rejects_ties_broken_by_the_higher_column():
    """A tie has no room under any delta > 0 -- a perturbation reorders it -- so the tie rule is held at delta = 0, on exact
    scores (the kernel test does the same: kept and theta are compared exactly on host-made rows).  Two-valued rows with the
    duplicate straddling rank k: the sampler that ranks the higher column first keeps the wrong twin."""
    from tests import sample_restatement as R
    from tests import sample_trunc_rules as TR
    rng = np.random.default_rng(5)
    bad = 0
    for trial in range(40):
        x = np.where(rng.random(33) < 0.2, 1.0, 0.0).astype(np.float32)
        n_hi = int((x == 1.0).sum())
        k = n_hi + 2                                         # the cut falls inside the run of zeros
        pert = TR.scaled(x, 1.0) + R.gumbel(R.noise_bits(3, 0, trial, 1, np.arange(33)))
        # the wrong sampler: ranks by x descending, the HIGHER column first among equals
        order = np.argsort(-x[::-1].astype(np.float64), kind="stable")
        kept_wrong = np.sort((32 - order)[:k])
        word = int(kept_wrong[np.argmax(pert[kept_wrong])]) + 1
        ok, _ = TR.decide(x, pert, word, 1.0, k, 1.0, delta=0.0)
        bad += not ok
        right = np.sort(TR.kept_set(x, 1.0, k, 1.0))
        ok, why = TR.decide(x, pert, int(right[np.argmax(pert[right])]) + 1, 1.0, k, 1.0, delta=0.0)
        assert ok, why
    print("ties by the higher column: %d of 40 decisions rejected" % bad)
    assert bad >= 1


def test_wide_contains_kept_contains_narrow():
    from tests import sample_trunc_rules as TR
    rng = np.random.default_rng(2)
    for k, p, temp in ((10, 1.0, 1.0), (0, 0.9, 0.5), (40, 0.5, 0.1), (1, 1.0, 1.0), (0, 1.0, 1.0)):
        for _ in range(10):
            x = (rng.standard_normal(201) * 2).astype(np.float32)
            x[5] = x[6]
            kept = np.zeros(201, bool); kept[TR.kept_set(x, temp, k, p)] = True
            wide, narrow = TR.wide_narrow(x, temp, k, p, 2e-4)
            assert (wide | ~kept).all() and (kept | ~narrow).all()
            w0, n0 = TR.wide_narrow(x, temp, k, p, 0.0)
            np.testing.assert_array_equal(w0, kept)
            np.testing.assert_array_equal(n0, kept)


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_header_cdef_and_ctypes_agree():
    from tests.test_abi_and_host import _prototypes
    import ctypes as C
    from densecap_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name in ("dc_sample_captions_trunc", "dc_op_lm_sample_n_trunc"):
        assert name in hp and name in _lib.EXPORTED_SYMBOLS and lp[name] == hp[name], name
    struct = r"typedef struct dc_sample_trunc \{\s*int32_t top_k; float top_p;\s*\} dc_sample_trunc;"
    assert re.search(struct, hdr) and re.search(struct, cdef)
    assert C.sizeof(_lib.DcSampleTrunc) == 8 and C.sizeof(_lib.DcSampleOpts) == 16             # dc_sample_opts stays as it is
    dbg = open(os.path.join(ROOT, "include", "densecap_debug_sample.h")).read()
    assert "dc_debug_sample_trunc_rows" in dbg and "dc_debug_sample_trunc_rows" not in lua and "dc_debug_sample_trunc_rows" not in hdr
    lm = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    assert "function Model:sampleCaptions(input, num_samples, temperature, seed, top_k, top_p)" in lm


def test_library_exports_the_truncation_entry_points():
    if not os.path.exists(os.path.join(ROOT, "densecap_amd", "lib", "libdensecap_hip.so")):
        import __graft_entry__ as g
        g.build()
    from densecap_amd import _lib
    lib = _lib.lib()
    for name in ("dc_sample_captions_trunc", "dc_op_lm_sample_n_trunc", "dc_debug_sample_trunc_rows"):
        assert hasattr(lib, name), name
    assert lib.dc_debug_sample_trunc_rows.argtypes is not None


def test_check_sample_args_refusals():
    from densecap_amd import ops
    from densecap_amd.model import DenseCapModel

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was reached: %s" % name)

    ctx = NoLibrary()
    codes = np.zeros((2, 8), np.float32)
    bad = [dict(top_k=-1), dict(top_k=1.5), dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5),
           dict(top_p=float("nan")), dict(temperature=0.0, top_k=5), dict(temperature=0.0, top_p=0.9),
           dict(temperature=0.0, want_sample_logprob=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.check_sample_args(1, kw.pop("temperature", 1.0), 0, **kw)
    for kw in [dict(top_k=-1), dict(top_p=0.0), dict(top_p=float("nan")), dict(temperature=0.0, top_k=5)]:
        with pytest.raises(ValueError):
            ops.lm_sample_n(ctx, codes, 1, **kw)
        m = object.__new__(DenseCapModel)
        m.ctx = m.lib = ctx
        with pytest.raises(ValueError):
            m.sampleCaptions(np.zeros((3, 8, 8), np.float32), 1, **kw)
    with pytest.raises(ValueError):
        ops.check_sample_args(1, 1.0, 0, top_k=202, vocab_size=200)
    o = ops.check_sample_args(2, 1.0, 0, top_k=201, top_p=0.5, vocab_size=200)
    assert (o.num_samples, o.temperature, o.seed) == (2, 1.0, 0)
    assert ops.sample_trunc_arg(1.0) is None and ops.sample_trunc_arg(0.0) is None
    t = ops.sample_trunc_arg(1.0, 0, 1.0, want_sample_logprob=True)
    assert (t.top_k, t.top_p) == (0, 1.0)
    t = ops.sample_trunc_arg(0.5, 40, 0.9)
    assert t.top_k == 40 and t.top_p == np.float32(0.9)


def test_run_model_parser_and_up_front_checks():
    from densecap_amd import run_model
    opt = run_model.build_parser().parse_args([])
    assert opt.top_k == 0 and opt.top_p == 1.0
    opt = run_model.build_parser().parse_args(["-num_samples", "2", "-top_k", "40", "-top_p", "0.9"])
    assert (opt.top_k, opt.top_p) == (40, 0.9)
    assert {"top_k", "top_p"} <= set(run_model.SAMPLING_FLAGS)
    for extra in (["-top_k", "-3"], ["-top_p", "0"], ["-top_p", "1.2"], ["-temperature", "0", "-num_samples", "1", "-top_k", "5"]):
        with pytest.raises(SystemExit) as e:
            run_model.main(["-synthetic_weights", "1", "-input_dir", ROOT, "-num_samples", "2"] + extra)
        assert "top_k" in str(e.value) or "top_p" in str(e.value), (extra, e.value)
