"""Sampling captions (dc_sample_captions / dc_op_lm_sample_n), the parts that need no GPU: the noise definition, the ABI
surface, the CPU restatement pinned against the oracle's greedy decode and the scoring restatement, the distribution of
its first words, and the argument checks of the Python / CLI surface."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    from tests.sample_restatement import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(*[np.uint32(c) for c in ctr], *key)
        assert tuple(int(g) for g in got) == want


def test_noise_bits_pick_the_word_of_the_column():
    from tests.sample_restatement import noise_bits, philox4x32_10
    a = noise_bits(5, 1, 2, 3, np.arange(8))
    b = philox4x32_10(np.uint32([0, 1]), np.uint32(3), np.uint32(2), np.uint32(1), 5, 0)
    np.testing.assert_array_equal(a, np.stack(b, 1).reshape(-1))


def test_uniform_is_strictly_inside_the_unit_interval_and_exact_in_fp32():
    from tests.sample_restatement import gumbel, uniform
    u = uniform(np.array([0, 0xffffffff, 0x1ff, 0x200], np.uint32))
    assert 0.0 < u[0] == 2.0 ** -24 and u[1] == 1.0 - 2.0 ** -24 < 1.0 and u[2] == u[0] and u[3] == 3 * 2.0 ** -24
    np.testing.assert_array_equal(u.astype(np.float32).astype(np.float64), u)
    np.testing.assert_array_equal((1.0 - u).astype(np.float32).astype(np.float64), 1.0 - u)
    g = gumbel(np.array([0, 0xffffffff], np.uint32))
    # u = 2^-24: g = -log(24 log 2) = -2.8115; u = 1 - 2^-24: g = 24 log 2 to first order = 16.6355
    assert abs(g[0] + np.log(24 * np.log(2))) < 1e-12 and abs(g[1] - 24 * np.log(2)) < 1e-6


def _header(name="densecap.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_in_header_exports_and_cdef():
    from tests.test_abi_and_host import _prototypes
    hdr = _header()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    from densecap_amd import _lib
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name in ("dc_sample_captions", "dc_op_lm_sample_n"):
        assert name in hp and name in _lib.EXPORTED_SYMBOLS, name
        assert lp[name] == hp[name]
    assert hp["dc_sample_captions"] == ("int dc_sample_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, "
                                        "const dc_sample_opts* opts, dc_result* out, int32_t* samples, float* logprob)")
    assert hp["dc_op_lm_sample_n"] == ("int dc_op_lm_sample_n(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, "
                                       "const dc_sample_opts* opts, int32_t* samples, float* logprob)")
    struct = r"typedef struct dc_sample_opts \{\s*int32_t num_samples; float temperature; uint64_t seed;\s*\} dc_sample_opts;"
    assert re.search(struct, hdr) and re.search(struct, cdef)
    assert [f[0] for f in _lib.DcSampleOpts._fields_] == ["num_samples", "temperature", "seed"]
    import ctypes as C
    assert C.sizeof(_lib.DcSampleOpts) == 16 and _lib.DcSampleOpts.seed.offset == 8
    assert "function Model:sampleCaptions" in open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    # the debug entries live in the debug header, not in the boundary header or the Lua cdef
    dbg = open(os.path.join(ROOT, "include", "densecap_debug.h")).read()
    assert "sample_rows_cap" in dbg and "sample_gumbel@" in dbg and "sample_bits@" in dbg
    assert "sample_rows_cap" not in lua and "sample_gumbel" not in lua


def test_library_exports_the_sampling_entry_points():
    if not os.path.exists(os.path.join(ROOT, "densecap_amd", "lib", "libdensecap_hip.so")):
        import __graft_entry__ as g
        g.build()
    from densecap_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "dc_sample_captions") and hasattr(lib, "dc_op_lm_sample_n")


def test_restatement_greedy_is_the_oracle_decode_and_its_logprob_the_score():
    """temperature 0: the restatement's words are the oracle's greedy decode (cut after the first END), and for the rows that
    contain END its log-probability is score_restatement.lm_score of that caption."""
    import torch
    from oracle import densecap_oracle as O
    from densecap_amd.weights import make_synthetic_weights
    from tests import sample_restatement, score_restatement
    W = make_synthetic_weights(seed=7, vocab_size=300, seq_length=8)
    T, V = 8, 300
    codes = torch.randn(24, W["fc7_w"].shape[0], generator=torch.Generator().manual_seed(3)) * 2
    seq = O.lm_sample(codes, W, T)
    r = sample_restatement.lm_sample_n(codes.numpy(), W, 1, temperature=0)
    np.testing.assert_array_equal(r["choice"][:, 0], seq)
    ended = 0
    for i in range(len(seq)):
        ends = np.nonzero(seq[i] == V + 1)[0]
        te = int(ends[0]) + 1 if len(ends) else T
        np.testing.assert_array_equal(r["samples"][i, 0, :te], seq[i, :te])
        assert (r["samples"][i, 0, te:] == 0).all()
        if len(ends):
            ended += 1
            q = np.zeros((1, T), np.int32)
            q[0, :te - 1] = seq[i, :te - 1]
            assert r["logprob"][i, 0] == score_restatement.lm_score(codes.numpy(), W, q)[i, 0]      # same rows, same products
    assert (r["gap"] >= 0).all()
    # (no greedy row of this model produces END within 8 words: the END rule is exercised on sampled rows, which do)
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    codes = (np.random.default_rng(4).standard_normal((6, W["fc7_w"].shape[0])) * 2).astype(np.float32)
    r = sample_restatement.lm_sample_n(codes, W, 8, temperature=1.0, seed=7)
    for i in range(6):
        for s in range(8):
            row = r["samples"][i, s]
            ends = np.nonzero(row == 201)[0]
            if len(ends):
                ended += 1
                assert (row[ends[0] + 1:] == 0).all() and (row[:ends[0]] > 0).all()
                q = np.zeros((1, 15), np.int32)
                q[0, :ends[0]] = row[:ends[0]]
                # the scoring restatement on the same 48 rows (row s * 6 + i): every matrix product has the same shape in both
                want = score_restatement.lm_score(np.tile(codes, (8, 1)), W, q)[s * 6 + i, 0]
                assert r["logprob"][i, s] == want, (i, s, r["logprob"][i, s], want)
            else:
                assert (row > 0).all()
    assert ended >= 1


def chi_square_of_first_words(first_words, scores, temperature):
    """Pearson chi-square of the first-word counts against SoftMax(scores / temperature): the words with expected count >= 5
    are cells of their own, the rest is pooled.  Returns (chi2, dof, limit = dof + 6 * sqrt(2 * dof))."""
    S = len(first_words)
    z = scores.astype(np.float64) * np.float64(np.float32(1.0) / np.float32(temperature))
    p = np.exp(z - z.max())
    p /= p.sum()
    exp = p * S
    big = exp >= 5
    counts = np.bincount(np.asarray(first_words) - 1, minlength=len(p)).astype(np.float64)
    o = list(counts[big]); e = list(exp[big])
    if (~big).any() and exp[~big].sum() > 0:
        o.append(counts[~big].sum()); e.append(exp[~big].sum())
    o, e = np.array(o), np.array(e)
    chi2 = float(((o - e) ** 2 / e).sum())
    dof = len(o) - 1
    return chi2, dof, dof + 6.0 * np.sqrt(2.0 * dof)


def first_step_scores(code, W):
    """scores_1 of one region (the START step's output), as the restatement computes them."""
    import torch
    from oracle import densecap_oracle as O
    Hd = W["lstm_w"].shape[1] // 4
    E = W["lstm_w"].shape[0] - Hd
    Wx, Wh = W["lstm_w"][:E], W["lstm_w"][E:]
    V1 = W["lm_out_w"].shape[0]
    x = torch.from_numpy(np.ascontiguousarray(code, np.float32))[None]
    enc = torch.relu(x @ W["lm_enc_w"].t() + W["lm_enc_b"])
    h, c = O.lstm_step(W["lstm_b"] + enc @ Wx, torch.zeros(1, Hd), torch.zeros(1, Hd), Wh)
    h, c = O.lstm_step(W["lstm_b"] + W["lm_emb"][V1 - 1][None] @ Wx, h, c, Wh)
    return (h @ W["lm_out_w"].t() + W["lm_out_b"]).numpy()[0]


@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_first_words_follow_the_softmax(temperature):
    from densecap_amd.weights import make_synthetic_weights
    from tests import sample_restatement
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    code = (np.random.default_rng(99).standard_normal((1, W["fc7_w"].shape[0])) * 2).astype(np.float32)
    r = sample_restatement.lm_sample_n(code, W, 8192, temperature=temperature, seed=99, steps=1)
    words = r["choice"][0, :, 0]
    assert words.min() >= 1 and words.max() <= 201
    chi2, dof, limit = chi_square_of_first_words(words, first_step_scores(code[0], W), temperature)
    print("temperature %g: chi-square %.1f at dof %d (limit %.1f)" % (temperature, chi2, dof, limit))
    assert dof >= 10 and chi2 <= limit, (chi2, dof, limit)


def test_run_model_parser_takes_the_sampling_flags():
    from densecap_amd.run_model import build_parser
    opt = build_parser().parse_args([])
    assert opt.num_samples == 0 and opt.temperature == 1.0 and opt.sample_seed == 0
    opt = build_parser().parse_args(["-num_samples", "4", "-temperature", "0.5", "-sample_seed", "7"])
    assert (opt.num_samples, opt.temperature, opt.sample_seed) == (4, 0.5, 7)


def test_python_argument_checks_raise_before_the_library_is_called():
    from densecap_amd import ops
    from densecap_amd.model import DenseCapModel

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was reached: %s" % name)

    ctx = NoLibrary()
    codes = np.zeros((2, 8), np.float32)
    bad = [dict(num_samples=0), dict(num_samples=257), dict(num_samples=2, temperature=0.005),
           dict(num_samples=2, temperature=float("nan")), dict(num_samples=2, temperature=0.0),
           dict(num_samples=2, temperature=100.5), dict(num_samples=1.5), dict(num_samples=1, seed=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.lm_sample_n(ctx, codes, **kw)
        m = object.__new__(DenseCapModel)          # no ctx, no library: the checks come first
        m.ctx = m.lib = ctx
        with pytest.raises(ValueError):
            m.sampleCaptions(np.zeros((3, 8, 8), np.float32), **kw)
    o = ops.check_sample_args(1, 0.0, 2 ** 64 - 1)
    assert (o.num_samples, o.temperature, o.seed) == (1, 0.0, 2 ** 64 - 1)
