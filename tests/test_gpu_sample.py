"""Sampling captions on the GPU (dc_sample_captions / dc_op_lm_sample_n; docs/SEMANTICS.md, "Sampling captions"): the device's
noise against its definition, the greedy rule against the greedy decode, words and log-probabilities against the CPU
restatement (teacher-forced on the device's own words), the equality with the scorer on rows that contain END, the
bit-identities (region subsets, S, chunking, region count, lanes, caption order), the distribution of the first words, and
the C / Python / CLI surface.

Not covered: K = 0 through dc_sample_captions -- the final NMS keeps its best box whenever the RPN proposes one, so no input
of this suite yields an image without regions; the entry point returns before the sampling then, as dc_score_captions does."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 1e-4          # the project's bound for a continuous stage against the oracle (tests/parity.py::strict_check)
NOISE = 1e-5          # the bound of the device's g against float64 (test_noise_function)


@pytest.fixture(scope="module")
def small():
    """vocab_size 200 as in test_gpu_score.py: V+1 = 201 columns padded to 256 -- the last 32-column slot is padding only,
    the one before it partly."""
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    m = DenseCapModel(W, device=0)
    yield m, W
    m.ctx.close()


@pytest.fixture(scope="module")
def full():
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    m = DenseCapModel(W, device=0)
    yield m, W
    m.ctx.close()


def _codes(n, D, seed):
    return (np.random.default_rng(seed).standard_normal((n, D)) * 2).astype(np.float32)


def _greedy(m, codes):
    """dc_op_lm_sample on the codes: (n, T) tokens."""
    from densecap_amd._lib import check
    cd = m.ctx.to_device(codes)
    td = m.ctx.empty((len(codes), m.seq_length), np.int32)
    check(m.ctx.h, m.lib.dc_op_lm_sample(m.ctx.h, cd.ptr, len(codes), td.ptr), "dc_op_lm_sample")
    return td.numpy()


def _cut(tokens, end):
    """rows as the sampler writes them: up to and including the first END, zeros after it."""
    out = np.array(tokens, np.int32)
    for row in out:
        e = np.nonzero(row == end)[0]
        if len(e):
            row[e[0] + 1:] = 0
    return out


def _t_end(row, end):
    e = np.nonzero(row == end)[0]
    return int(e[0]) + 1 if len(e) else len(row)


def _fetch(m, name, buf):
    n = m.lib.dc_debug_fetch(m.ctx.h, name.encode(), buf.ctypes.data, buf.nbytes)
    assert n >= 0, m.lib.dc_last_error(m.ctx.h)
    return n


def _decisions(dev, ref, margin, end):
    """The per-decision rule on rows dev (n, S, T) against a restatement fed dev: every word up to a row's end is the
    restatement's, or the restatement's best-to-second gap is at most `margin` and the device's word scores within `margin` of
    the best.  Returns (decisions, decisions that needed the margin); asserts the rule."""
    total = needed = 0
    n, S, T = dev.shape
    for i in range(n):
        for s in range(S):
            te = _t_end(dev[i, s], end)
            same = dev[i, s, :te] == ref["choice"][i, s, :te]
            total += te
            for t in np.nonzero(~same)[0]:
                needed += 1
                assert ref["gap"][i, s, t] <= margin, (i, s, t, ref["gap"][i, s, t], margin)
                assert ref["best"][i, s, t] - ref["fed_score"][i, s, t] <= margin, (i, s, t)
    return total, needed


# ---- 1. the noise function ------------------------------------------------------------------------------------------------
def test_noise_function(small):
    from tests import sample_restatement as R
    m, _ = small
    g = np.empty(1 << 23, np.float32)
    assert _fetch(m, "sample_gumbel@0", g) == 1 << 23
    want = R.gumbel(np.arange(1 << 23, dtype=np.uint32) << np.uint32(9))
    err = np.abs(g.astype(np.float64) - want)
    print("max |g_device - g_float64| over 2^23 values: %.3g (at index %d)" % (err.max(), int(err.argmax())))
    assert np.isfinite(g).all() and err.max() <= NOISE
    part = np.empty(5, np.float32)
    assert _fetch(m, "sample_gumbel@%d" % ((1 << 23) - 5), part) == 5
    np.testing.assert_array_equal(part, g[-5:])
    rng = np.random.default_rng(11)
    for seed in (0, 7, 0xffffffff, (0x299f31d0 << 32) | 0xa4093822, 2 ** 64 - 1):
        co = np.stack([rng.integers(0, 256, 300), rng.integers(0, 7000, 300), rng.integers(1, 65, 300),
                       rng.integers(0, 10498, 300)], 1).astype(np.int32)
        co[0] = [0, 0, 1, 0]
        co[1] = [255, 2 ** 31 - 1, 64, 10497]
        buf = co.copy()
        assert _fetch(m, "sample_bits@%d" % seed, buf) == 300
        got = buf.reshape(-1).view(np.uint32)[:300]
        np.testing.assert_array_equal(got, R.noise_bits(seed, co[:, 0], co[:, 1], co[:, 2], co[:, 3]))
    assert m.lib.dc_debug_fetch(m.ctx.h, b"sample_gumbel@8388607", g.ctypes.data, 8) < 0      # past 2^23
    for name in (b"sample_gumbel@", b"sample_gumbel@12x", b"sample_gumbel@8388608", b"sample_gumbel@-1", b"sample_bits@",
                 b"sample_bits@7 ", b"sample_bits@18446744073709551616"):
        assert m.lib.dc_debug_fetch(m.ctx.h, name, g.ctypes.data, 64) < 0, name
        assert "must follow the '@'" in m.lib.dc_last_error(m.ctx.h).decode()


# ---- 2. the greedy rule -----------------------------------------------------------------------------------------------------
def _check_greedy(m, W, codes, got, greedy):
    """got (n, T) = temperature-0 rows of the sampler on `codes`, greedy (n, T) = the greedy decode of the same regions."""
    from tests import sample_restatement as R
    end = m.vocab_size + 1
    want = _cut(greedy, end)
    diff = np.nonzero((got != want).any(axis=1))[0]
    print("greedy rule: %d of %d rows differ from the greedy decode" % (len(diff), len(got)))
    assert len(diff) <= 0.01 * len(got), len(diff)
    if len(diff) == 0:
        return
    margin = 2 * STAGE
    fed_greedy = R.lm_sample_n(codes[diff], W, 1, temperature=0, forced=greedy[diff][:, None, :])
    fed_own = R.lm_sample_n(codes[diff], W, 1, temperature=0, forced=np.where(got[diff] > 0, got[diff], 0)[:, None, :])
    for j, i in enumerate(diff):
        te = _t_end(want[i], end)
        assert fed_greedy["gap"][j, 0, :te].min() <= margin, (i, fed_greedy["gap"][j, 0, :te].min())
        first = int(np.nonzero(got[i] != want[i])[0][0])
        te2 = _t_end(got[i], end)
        for t in range(first, te2):
            if got[i, t] != fed_own["choice"][j, 0, t]:
                assert fed_own["gap"][j, 0, t] <= margin and fed_own["best"][j, 0, t] - fed_own["fed_score"][j, 0, t] <= margin


def test_greedy_rule_op(small, full):
    from densecap_amd import ops
    for (m, W), n in ((small, 300), (full, 1000)):
        codes = _codes(n, m.fc_dim, 12)
        got, lp = ops.lm_sample_n(m.ctx, codes, 1, temperature=0.0)
        assert got.shape == (n, 1, m.seq_length) and lp.shape == (n, 1) and np.isfinite(lp).all() and (lp <= 0).all()
        _check_greedy(m, W, codes, got[:, 0], _greedy(m, codes))


@pytest.mark.parametrize("which", ["small", "full"])
@pytest.mark.parametrize("order", [0, 1])
def test_greedy_rule_sample_captions(small, full, order, which):
    from densecap_amd.weights import make_synthetic_image
    m, W = small if which == "small" else full
    m.setCaptionOrder(bool(order))
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
    img = np.ascontiguousarray(make_synthetic_image(320, 480, 3), np.float32)
    b0, s0, t0 = m.forward_raw(img)
    boxes, scores, tokens, samples, lp = m.sampleCaptions(img, 1, temperature=0.0)
    np.testing.assert_array_equal(boxes, b0)
    np.testing.assert_array_equal(scores, s0)
    np.testing.assert_array_equal(tokens, t0)
    fb, feats = m.extractFeatures(img)
    np.testing.assert_array_equal(fb, b0)
    _check_greedy(m, W, feats, samples[:, 0], t0)
    m.setCaptionOrder(True)


# ---- 3., 4. words and log-probabilities against the restatement; equality with the scorer -----------------------------------
@pytest.mark.parametrize("temperature", [0.1, 0.5, 1.0, 2.0])
def test_words_and_logprob_match_restatement(small, temperature):
    from densecap_amd import ops
    from tests import sample_restatement as R
    m, W = small
    end = 201
    codes = _codes(300, m.fc_dim, 1)
    dev, lp = ops.lm_sample_n(m.ctx, codes, 8, temperature=temperature, seed=7)
    ref = R.lm_sample_n(codes, W, 8, temperature=temperature, seed=7, forced=dev)
    margin = 2 * (STAGE / temperature + NOISE)
    total, needed = _decisions(dev, ref, margin, end)
    print("temperature %g: %d of %d decisions needed the margin %.3g" % (temperature, needed, total, margin))
    assert needed <= 0.01 * total
    # the output rows are the restatement's rows of the words fed
    np.testing.assert_array_equal(ref["samples"], dev)
    rel = np.abs(lp - ref["logprob"]) / np.maximum(np.abs(ref["logprob"]), 1e-3)
    print("temperature %g: max relative error of logprob %.3g" % (temperature, rel.max()))
    assert rel.max() < 1e-4, rel.max()
    # every draw that contains END: logprob IS the scorer's number for that caption on that region
    rows = [(i, s) for i in range(300) for s in range(8) if (dev[i, s] == end).any()]
    print("temperature %g: %d of %d draws contain END" % (temperature, len(rows), 300 * 8))
    assert len(rows) >= 1
    q = np.zeros((len(rows), 15), np.int32)
    for k, (i, s) in enumerate(rows):
        q[k] = np.where(dev[i, s] == end, 0, dev[i, s])
    ll = ops.lm_score(m.ctx, codes, q)
    np.testing.assert_array_equal(lp[[i for i, _ in rows], [s for _, s in rows]], ll[[i for i, _ in rows], np.arange(len(rows))])


# ---- 5. bit-identities ------------------------------------------------------------------------------------------------------
def test_op_bit_identities(small):
    from densecap_amd import ops
    from densecap_amd._lib import check
    m, W = small
    codes = _codes(300, m.fc_dim, 2)
    base, blp = ops.lm_sample_n(m.ctx, codes, 8, temperature=1.0, seed=3)
    again, alp = ops.lm_sample_n(m.ctx, codes, 8, temperature=1.0, seed=3)
    np.testing.assert_array_equal(again, base)
    np.testing.assert_array_equal(alp, blp)
    other, _ = ops.lm_sample_n(m.ctx, codes, 8, temperature=1.0, seed=4)
    assert (other != base).any(axis=2).mean() > 0.9
    assert (base[:, 0] != base[:, 1]).any(axis=1).mean() > 0.9         # several different captions for one region
    sub = np.array([3, 17, 100, 101, 299])
    a, alp = ops.lm_sample_n(m.ctx, codes[sub], 8, temperature=1.0, seed=3, row_ids=sub)
    np.testing.assert_array_equal(a, base[sub])
    np.testing.assert_array_equal(alp, blp[sub])
    a, alp = ops.lm_sample_n(m.ctx, codes, 3, temperature=1.0, seed=3)
    np.testing.assert_array_equal(a, base[:, :3])
    np.testing.assert_array_equal(alp, blp[:, :3])
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"sample_rows_cap", 700), "dc_debug_set")     # chunks of two draws
    try:
        a, alp = ops.lm_sample_n(m.ctx, codes, 8, temperature=1.0, seed=3)
    finally:
        check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"sample_rows_cap", 0), "dc_debug_set")
    np.testing.assert_array_equal(a, base)
    np.testing.assert_array_equal(alp, blp)


def test_op_rows_do_not_depend_on_the_region_count(small):
    """6,500 regions (the kScorePlanRows rule, as test_gpu_score.py): the rows must be those of a small call."""
    from densecap_amd import ops
    m, W = small
    codes = _codes(6500, m.fc_dim, 8)
    big, blp = ops.lm_sample_n(m.ctx, codes, 2, temperature=1.0, seed=5)
    assert np.isfinite(blp).all()
    sub = np.array([0, 1, 2, 1000, 4095, 4096, 6499])
    a, alp = ops.lm_sample_n(m.ctx, codes[sub], 2, temperature=1.0, seed=5, row_ids=sub)
    np.testing.assert_array_equal(a, big[sub])
    np.testing.assert_array_equal(alp, blp[sub])


def test_sample_captions_bit_identities(full):
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, W = full
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
    img = np.ascontiguousarray(make_synthetic_image(320, 480, 3), np.float32)
    m.setLanes(1)
    m.setCaptionOrder(True)
    b0, s0, t0 = m.forward_raw(img)
    base = m.sampleCaptions(img, 4, temperature=1.0, seed=9)
    assert len(b0) > 0
    np.testing.assert_array_equal(base[0], b0)
    np.testing.assert_array_equal(base[2], t0)
    # the op on the codes dc_extract_features returns for the image
    fb, feats = m.extractFeatures(img)
    a, alp = ops.lm_sample_n(m.ctx, feats, 4, temperature=1.0, seed=9)
    np.testing.assert_array_equal(a, base[3])
    np.testing.assert_array_equal(alp, base[4])
    try:
        for lanes, order in ((3, 1), (3, 0), (1, 0)):
            m.setLanes(lanes)
            m.setCaptionOrder(bool(order))
            r = m.sampleCaptions(img, 4, temperature=1.0, seed=9)
            for x, y in zip(r, base):
                np.testing.assert_array_equal(x, y)
        m.setLanes(2)
        m.setGroup(2)
        m.setCaptionOrder(True)
        outs = m.forward_batch(np.stack([img, img]))
        np.testing.assert_array_equal(outs[0][0], b0)
        r = m.sampleCaptions(img, 4, temperature=1.0, seed=9)
        for x, y in zip(r, base):
            np.testing.assert_array_equal(x, y)
        r = m.sampleCaptions(img, 4, temperature=1.0, seed=9, want_tokens=False)
        assert r[2] is None
        for k in (0, 1, 3, 4):
            np.testing.assert_array_equal(r[k], base[k])
        other = m.sampleCaptions(img, 4, temperature=1.0, seed=10)
        assert (other[3] != base[3]).any()
        np.testing.assert_array_equal(other[0], b0)
    finally:
        m.setGroup(1)
        m.setLanes(2)
        m.setCaptionOrder(True)


# ---- 6. the distribution on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_first_words_follow_the_softmax_on_the_device(small, temperature):
    """8,192 draws of one region's first word: 32 region rows x 256 draws of the same code (a call holds at most 256 draws)."""
    from densecap_amd import ops
    from tests.test_sample_captions_cpu import chi_square_of_first_words, first_step_scores
    m, W = small
    code = (np.random.default_rng(99).standard_normal((1, m.fc_dim)) * 2).astype(np.float32)
    dev, _ = ops.lm_sample_n(m.ctx, np.repeat(code, 32, 0), 256, temperature=temperature, seed=99)
    words = dev[:, :, 0].reshape(-1)
    assert len(words) == 8192 and words.min() >= 1 and words.max() <= 201
    chi2, dof, limit = chi_square_of_first_words(words, first_step_scores(code[0], W), temperature)
    print("temperature %g: chi-square %.1f at dof %d (limit %.1f)" % (temperature, chi2, dof, limit))
    assert dof >= 10 and chi2 <= limit, (chi2, dof, limit)


# ---- 7. the surface ---------------------------------------------------------------------------------------------------------
def test_output_format_and_refusals(small):
    from densecap_amd import Context, _lib, ops
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    V1 = 201
    codes = _codes(64, m.fc_dim, 4)
    dev, lp = ops.lm_sample_n(m.ctx, codes, 16, temperature=1.5, seed=1)
    assert dev.dtype == np.int32 and lp.dtype == np.float32 and np.isfinite(lp).all() and (lp < 0).all()
    assert dev.min() >= 0 and dev.max() <= V1
    ended = 0
    for row in dev.reshape(-1, 15):
        e = np.nonzero(row == V1)[0]
        if len(e):
            ended += 1
            assert (row[:e[0]] > 0).all() and (row[e[0] + 1:] == 0).all()
        else:
            assert (row > 0).all()
    assert ended >= 1
    lib = m.lib
    cd = m.ctx.to_device(codes)
    tok = m.ctx.empty((64, 256, 15), np.int32); out = m.ctx.empty((64, 256), np.float32)
    O = _lib.DcSampleOpts
    bad = [(O(0, 1.0, 0), "num_samples must be in 1..256"), (O(257, 1.0, 0), "num_samples must be in 1..256"),
           (O(2, 0.005, 0), "temperature must be 0 or in"), (O(2, float("nan"), 0), "temperature must be 0 or in"),
           (O(2, 100.5, 0), "temperature must be 0 or in"), (O(2, -1.0, 0), "temperature must be 0 or in"),
           (O(2, 0.0, 0), "num_samples must be 1")]
    for o, msg in bad:
        assert lib.dc_op_lm_sample_n(m.ctx.h, cd.ptr, 64, None, C.byref(o), tok.ptr, out.ptr) == -1      # DC_E_INVALID
        assert msg in lib.dc_last_error(m.ctx.h).decode(), lib.dc_last_error(m.ctx.h)
    ok = O(1, 1.0, 0)
    assert lib.dc_op_lm_sample_n(m.ctx.h, cd.ptr, 64, None, None, tok.ptr, out.ptr) < 0
    assert "null options" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_op_lm_sample_n(m.ctx.h, None, 64, None, C.byref(ok), tok.ptr, out.ptr) < 0
    assert "null pointer" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_op_lm_sample_n(m.ctx.h, cd.ptr, 0, None, C.byref(ok), tok.ptr, out.ptr) < 0
    ids = m.ctx.to_device(np.full(64, -3, np.int32))
    assert lib.dc_op_lm_sample_n(m.ctx.h, cd.ptr, 64, ids.ptr, C.byref(ok), tok.ptr, out.ptr) < 0
    assert "negative" in lib.dc_last_error(m.ctx.h).decode()
    img = np.ascontiguousarray(make_synthetic_image(160, 224, 1), np.float32)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    r, *_ = m._new_result(1)
    sm = np.zeros((1, 1, 15), np.int32); sl = np.zeros((1, 1), np.float32)
    assert lib.dc_sample_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(ok), C.byref(r), sm.ctypes.data,
                                  sl.ctypes.data) < 0
    assert "out->capacity is 1" in lib.dc_last_error(m.ctx.h).decode()
    for o, msg in bad:
        assert lib.dc_sample_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(o), C.byref(r), sm.ctypes.data,
                                      sl.ctypes.data) == -1
        assert msg in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_sample_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(ok), C.byref(r), None, sl.ctypes.data) < 0
    assert "null pointer" in lib.dc_last_error(m.ctx.h).decode()
    ctx = Context(0)
    try:
        assert lib.dc_op_lm_sample_n(ctx.h, cd.ptr, 64, None, C.byref(ok), tok.ptr, out.ptr) < 0
        assert "weights not loaded" in lib.dc_last_error(ctx.h).decode()
    finally:
        ctx.close()
    # the ctx still works, and gives what it gave
    again, alp = ops.lm_sample_n(m.ctx, codes, 16, temperature=1.5, seed=1)
    np.testing.assert_array_equal(again, dev)
    np.testing.assert_array_equal(alp, lp)


def test_non_finite_codes_end_the_row_cleanly(small):
    """An Inf among a row's codes makes about half of its image-encoder outputs +Inf (the others are clamped by the ReLU), the
    gates Inf - Inf = NaN, and from there the state and every score NaN: no perturbed score compares greater than anything,
    so the step GEMM hands the row kernel no column at all.  The drawn token selects an embedding row by address, so it is
    checked before use: the row must then have no word (zeros, NaN log-probability), while the call succeeds, every other row
    is what it is without the bad rows, and the ctx keeps working.  (A NaN code does not get that far on this path -- the
    encoder's ReLU is `v > 0 ? v : 0` -- and neither does a row of Infs, whose encoder sums are Inf - Inf = NaN already: for
    those rows only the general properties are demanded.)"""
    from densecap_amd import ops
    m, W = small
    codes = _codes(40, m.fc_dim, 6)
    for temperature, S in ((1.0, 4), (0.0, 1)):
        base, blp = ops.lm_sample_n(m.ctx, codes, S, temperature=temperature, seed=2)
        bad = codes.copy()
        bad[3, :] = np.inf
        bad[29, 100] = np.inf
        bad[17, 5] = np.nan
        bad[18, :] = np.nan
        got, lp = ops.lm_sample_n(m.ctx, bad, S, temperature=temperature, seed=2)
        good = np.setdiff1d(np.arange(40), [3, 17, 18, 29])
        np.testing.assert_array_equal(got[good], base[good])
        np.testing.assert_array_equal(lp[good], blp[good])
        assert (got[29] == 0).all() and np.isnan(lp[29]).all(), (got[29], lp[29])
        assert got.min() >= 0 and got.max() <= 201            # every id written anywhere is a word, END or 0
        for r in (3, 17, 18):
            for s_ in range(S):
                assert np.isnan(lp[r, s_]) or (lp[r, s_] < 0 and got[r, s_, 0] > 0), (r, s_, lp[r, s_], got[r, s_])
        again, alp = ops.lm_sample_n(m.ctx, codes, S, temperature=temperature, seed=2)
        np.testing.assert_array_equal(again, base)
        np.testing.assert_array_equal(alp, blp)


def test_cli_makes_no_sampling_call_without_the_flag_and_seeds_image_by_image(tmp_path, monkeypatch):
    """run_model in this process with DenseCapModel.sampleCaptions watched: without -num_samples it is never called; with it,
    once per image, image i with seed s + i."""
    from PIL import Image
    from densecap_amd import DenseCapModel, run_model
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(120, 160), (140, 100), (120, 160)]):
        rgb = (np.random.default_rng(i).random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(d / ("im%d.png" % i)))
    calls = []
    real = DenseCapModel.sampleCaptions

    def watched(self, img, num_samples, temperature=1.0, seed=0, want_tokens=True):
        calls.append((num_samples, temperature, seed))
        return real(self, img, num_samples, temperature, seed, want_tokens)
    monkeypatch.setattr(DenseCapModel, "sampleCaptions", watched)
    common = ["-input_dir", str(d), "-synthetic_weights", "1", "-num_proposals", "50", "-image_size", "160"]
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "plain")]) == 0
    assert calls == []
    plain = json.load(open(tmp_path / "plain" / "results.json"))
    assert len(plain["results"]) == 3 and all(set(e) == {"boxes", "scores", "captions", "img_name"} for e in plain["results"])
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "sampled"), "-num_samples", "2", "-temperature", "0.5",
                                    "-sample_seed", "40"]) == 0
    assert sorted(calls) == [(2, 0.5, 40), (2, 0.5, 41), (2, 0.5, 42)]
    res = json.load(open(tmp_path / "sampled" / "results.json"))
    names = sorted(os.listdir(str(d)))
    assert [e["img_name"] for e in res["results"]] == names         # image i of the run = i-th file: seed 40 + i
    # the draws in the file are those of that seed: image 1 again, directly
    from densecap_amd.run_model import load_image_caffe
    from densecap_amd.weights import make_synthetic_weights
    monkeypatch.setattr(DenseCapModel, "sampleCaptions", real)
    m = DenseCapModel(make_synthetic_weights(), device=0)
    try:
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
        _, _, _, samples, lp = m.sampleCaptions(load_image_caffe(str(d / names[1]), 160)[0], 2, 0.5, 41)
        assert res["results"][1]["sampled_captions"] == [m.decodeSequence(samples[k]) for k in range(len(samples))]
        assert res["results"][1]["sampled_logprobs"] == [[float(v) for v in row] for row in lp]
    finally:
        m.ctx.close()
    with pytest.raises(SystemExit):
        run_model.main(common + ["-num_samples", "2", "-sample_seed", str(2 ** 64 - 2)])      # image 2 would need seed 2^64
    with pytest.raises(SystemExit):
        run_model.main(common + ["-num_samples", "2", "-temperature", "0"])


def test_python_against_the_c_call_and_cli(tmp_path):
    from densecap_amd import DenseCapModel, _lib
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    W = make_synthetic_weights(seed=1234, vocab_size=200, seq_length=8)
    m = DenseCapModel(W, device=0)
    try:
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
        img = np.ascontiguousarray(make_synthetic_image(160, 224, 1), np.float32)
        boxes, scores, tokens, samples, lp = m.sampleCaptions(img, 3, temperature=0.8, seed=5)
        b0, s0, t0 = m.forward_raw(img)
        K = len(b0)
        np.testing.assert_array_equal(boxes, b0)
        np.testing.assert_array_equal(tokens, t0)
        assert samples.shape == (K, 3, 8) and lp.shape == (K, 3)
        P = m._capacity(160, 224)
        r, rb, rs, rt = m._new_result(P)
        sm = np.zeros((P, 3, 8), np.int32); sl = np.zeros((P, 3), np.float32)
        o = _lib.DcSampleOpts(3, 0.8, 5)
        _lib.check(m.ctx.h, m.lib.dc_sample_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(o), C.byref(r),
                                                     sm.ctypes.data, sl.ctypes.data), "dc_sample_captions")
        assert r.K == K
        np.testing.assert_array_equal(sm[:K], samples)
        np.testing.assert_array_equal(sl[:K], lp)
        caps = m.decodeSequence(samples[:, 1])
        assert len(caps) == K and all(isinstance(c, str) for c in caps)
    finally:
        m.ctx.close()
    from PIL import Image
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(120, 160), (140, 100)]):
        rgb = (np.random.default_rng(i).random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(d / ("im%d.png" % i)))
    common = [sys.executable, "-m", "densecap_amd.run_model", "-input_dir", str(d), "-synthetic_weights", "1",
              "-num_proposals", "50", "-image_size", "160"]
    vis = tmp_path / "vis_plain"
    out = subprocess.run(common + ["-output_vis_dir", str(vis)], cwd=ROOT, check=True, capture_output=True, text=True)
    plain = json.load(open(vis / "results.json"))
    assert len(plain["results"]) == 2
    for e in plain["results"]:
        assert set(e) == {"boxes", "scores", "captions", "img_name"}
    assert not {"num_samples", "temperature", "sample_seed"} & set(plain["opt"])
    vis2 = tmp_path / "vis_sampled"
    subprocess.run(common + ["-output_vis_dir", str(vis2), "-num_samples", "3", "-temperature", "0.7", "-sample_seed", "11"],
                   cwd=ROOT, check=True, capture_output=True, text=True)
    res = json.load(open(vis2 / "results.json"))
    assert res["opt"]["num_samples"] == 3 and len(res["results"]) == 2
    for e, p in zip(res["results"], plain["results"]):
        assert set(e) == {"boxes", "scores", "captions", "img_name", "sampled_captions", "sampled_logprobs"}
        assert e["boxes"] == p["boxes"] and e["scores"] == p["scores"] and e["captions"] == p["captions"]
        K = len(e["boxes"])
        assert len(e["sampled_captions"]) == K and len(e["sampled_logprobs"]) == K
        for caps, lps in zip(e["sampled_captions"], e["sampled_logprobs"]):
            assert len(caps) == 3 and len(lps) == 3 and all(isinstance(c, str) for c in caps)
            assert all(np.isfinite(v) and v < 0 for v in lps)
