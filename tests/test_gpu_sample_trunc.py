"""Truncated caption sampling on the GPU through the calls (dc_sample_captions_trunc / dc_op_lm_sample_n_trunc;
docs/SEMANTICS.md, "Truncation: top-k and nucleus"): words and both log-probabilities against the float64 restatement under
the decision rule of tests/sample_trunc_rules.py, the greedy and the untruncated ends against the existing routes, the
bit-identity of the untruncated call with dc_op_lm_sample_n / dc_sample_captions, the bit-identities of the row route, the
distribution of the first words, rows without a word, the refusals, and the Python / CLI surface."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.test_gpu_sample import _check_greedy, _codes, _greedy, _t_end, full, small       # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
STAGE = 1e-4
END = 201


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-3)


# ---- words and log-probabilities against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("top_k,top_p", [(10, 1.0), (0, 0.9), (40, 0.5), (1, 1.0)])
def test_words_and_logprobs_match_restatement(small, top_k, top_p, temperature):
    from densecap_amd import ops
    from tests import sample_trunc_rules as TR
    m, W = small
    codes = _codes(300, m.fc_dim, 1)
    dev, lp, lq = ops.lm_sample_n(m.ctx, codes, 8, temperature=temperature, seed=7, top_k=top_k, top_p=top_p,
                                  want_sample_logprob=True)
    ref = TR.lm_sample_n_trunc(codes, W, 8, temperature=temperature, seed=7, top_k=top_k, top_p=top_p, forced=dev)
    total, needed = TR.check_words(dev, ref, temperature, top_k, top_p, END)       # asserts: no word outside the wide set
    print("(%d, %g) at temperature %g: %d of %d decisions needed the margin" % (top_k, top_p, temperature, needed, total))
    assert needed <= 0.01 * total
    np.testing.assert_array_equal(ref["samples"], dev)
    r1, r2 = _rel(lp, ref["logprob"]), _rel(lq, ref["sample_logprob"])
    print("  max relative error: logprob %.3g, sample_logprob %.3g" % (r1.max(), r2.max()))
    assert r1.max() < STAGE and r2.max() < STAGE
    assert (lq <= 0).all() and (lq >= lp - 1e-4 * np.abs(lp)).all() if temperature == 1.0 else (lq <= 0).all()
    rows = [(i, s) for i in range(300) for s in range(8) if (dev[i, s] == END).any()][:64]
    if top_k != 1:
        assert len(rows) >= 1
    if rows:
        q = np.zeros((len(rows), 15), np.int32)
        for k, (i, s) in enumerate(rows):
            q[k] = np.where(dev[i, s] == END, 0, dev[i, s])
        ll = ops.lm_score(m.ctx, codes, q)
        got = lp[[i for i, _ in rows], [s for _, s in rows]]
        want = ll[[i for i, _ in rows], np.arange(len(rows))]
        assert _rel(got, want).max() < STAGE, _rel(got, want).max()


def test_full_vocabulary(full):
    from densecap_amd import ops
    from tests import sample_trunc_rules as TR
    m, W = full
    V1 = m.vocab_size + 1
    codes = _codes(64, m.fc_dim, 3)
    dev, lp, lq = ops.lm_sample_n(m.ctx, codes, 2, temperature=1.0, seed=5, top_k=40, top_p=0.9, want_sample_logprob=True)
    ref = TR.lm_sample_n_trunc(codes, W, 2, temperature=1.0, seed=5, top_k=40, top_p=0.9, forced=dev)
    total, needed = TR.check_words(dev, ref, 1.0, 40, 0.9, V1)
    print("full vocabulary: %d of %d decisions needed the margin" % (needed, total))
    assert needed <= 0.01 * total
    np.testing.assert_array_equal(ref["samples"], dev)
    assert _rel(lp, ref["logprob"]).max() < STAGE and _rel(lq, ref["sample_logprob"]).max() < STAGE


# ---- the two ends ------------------------------------------------------------------------------------------------------------
def test_top_k_one_is_the_greedy_decode(small):
    from densecap_amd import ops
    m, W = small
    codes = _codes(300, m.fc_dim, 12)
    got, lp, lq = ops.lm_sample_n(m.ctx, codes, 2, temperature=0.7, seed=3, top_k=1, want_sample_logprob=True)
    np.testing.assert_array_equal(got[:, 0], got[:, 1])                    # one word kept: the draw does not matter
    np.testing.assert_array_equal(lq, np.zeros_like(lq))
    _check_greedy(m, W, codes, got[:, 0], _greedy(m, codes))


def test_top_k_all_against_the_fused_route(small):
    from densecap_amd import ops
    from tests import sample_trunc_rules as TR
    m, W = small
    codes = _codes(300, m.fc_dim, 1)
    for temperature in (0.5, 1.0):
        fused, flp = ops.lm_sample_n(m.ctx, codes, 8, temperature=temperature, seed=7)
        rows, rlp = ops.lm_sample_n(m.ctx, codes, 8, temperature=temperature, seed=7, top_k=END)
        diff = np.nonzero((fused != rows).any(axis=2).any(axis=1))[0]
        ndiff = int((fused != rows).any(axis=2).sum())
        print("top_k = V+1 against the fused route at temperature %g: %d of %d draws differ" % (temperature, ndiff, 300 * 8))
        assert ndiff <= 0.01 * 300 * 8
        same = (fused == rows).all(axis=2)
        assert _rel(rlp[same], flp[same]).max() < STAGE
        if len(diff):
            for words in (rows, fused):            # every differing decision is a near-tie on the scores of the words that were fed
                ref = TR.lm_sample_n_trunc(codes[diff], W, 8, temperature=temperature, seed=7, row_ids=diff, forced=words[diff])
                TR.check_words(words[diff], ref, temperature, 0, 1.0, END)


def test_the_untruncated_call_is_the_existing_call_bit_for_bit(small):
    from densecap_amd import _lib, ops
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    lib = m.lib
    codes = _codes(64, m.fc_dim, 4)
    base, blp = ops.lm_sample_n(m.ctx, codes, 4, temperature=0.8, seed=9)
    cd = m.ctx.to_device(codes)
    o = _lib.DcSampleOpts(4, 0.8, 9)
    for trunc in (None, _lib.DcSampleTrunc(0, 1.0)):
        tok = m.ctx.empty((64, 4, 15), np.int32); lp = m.ctx.empty((64, 4), np.float32)
        _lib.check(m.ctx.h, lib.dc_op_lm_sample_n_trunc(m.ctx.h, cd.ptr, 64, None, C.byref(o), C.byref(trunc) if trunc else None,
                                                        tok.ptr, lp.ptr, None), "dc_op_lm_sample_n_trunc")
        np.testing.assert_array_equal(tok.numpy(), base)
        np.testing.assert_array_equal(lp.numpy(), blp)
    o0 = _lib.DcSampleOpts(1, 0.0, 0)                                     # the greedy rule stays available through the new call
    g0, _ = ops.lm_sample_n(m.ctx, codes, 1, temperature=0.0)
    tok = m.ctx.empty((64, 1, 15), np.int32); lp = m.ctx.empty((64, 1), np.float32)
    _lib.check(m.ctx.h, lib.dc_op_lm_sample_n_trunc(m.ctx.h, cd.ptr, 64, None, C.byref(o0), None, tok.ptr, lp.ptr, None), "trunc")
    np.testing.assert_array_equal(tok.numpy(), g0)
    # dc_sample_captions_trunc with NULL, NULL against dc_sample_captions
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    img = np.ascontiguousarray(make_synthetic_image(160, 224, 1), np.float32)
    ref = m.sampleCaptions(img, 3, temperature=0.8, seed=5)
    P = m._capacity(160, 224)
    r, rb, rs, rt = m._new_result(P)
    sm = np.zeros((P, 3, 15), np.int32); sl = np.zeros((P, 3), np.float32)
    o = _lib.DcSampleOpts(3, 0.8, 5)
    _lib.check(m.ctx.h, lib.dc_sample_captions_trunc(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(o), None, C.byref(r),
                                                     sm.ctypes.data, sl.ctypes.data, None), "dc_sample_captions_trunc")
    assert r.K == len(ref[0])
    np.testing.assert_array_equal(sm[:r.K], ref[3])
    np.testing.assert_array_equal(sl[:r.K], ref[4])
    np.testing.assert_array_equal(rb[:r.K], ref[0])


# ---- the bit-identities of the row route ---------------------------------------------------------------------------------------
def test_op_bit_identities(small):
    from densecap_amd import ops
    from densecap_amd._lib import check
    m, W = small
    codes = _codes(300, m.fc_dim, 2)
    kw = dict(temperature=1.0, seed=3, top_k=40, top_p=0.9, want_sample_logprob=True)
    base = ops.lm_sample_n(m.ctx, codes, 8, **kw)
    again = ops.lm_sample_n(m.ctx, codes, 8, **kw)
    for x, y in zip(again, base):
        np.testing.assert_array_equal(x, y)
    other = ops.lm_sample_n(m.ctx, codes, 8, **dict(kw, seed=4))
    assert (other[0] != base[0]).any(axis=2).mean() > 0.5
    sub = np.array([3, 17, 100, 101, 299])
    a = ops.lm_sample_n(m.ctx, codes[sub], 8, row_ids=sub, **kw)
    for x, y in zip(a, base):
        np.testing.assert_array_equal(x, y[sub])
    a = ops.lm_sample_n(m.ctx, codes, 3, **kw)
    for x, y in zip(a, base):
        np.testing.assert_array_equal(x, y[:, :3])
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"sample_rows_cap", 700), "dc_debug_set")     # chunks of two draws
    try:
        a = ops.lm_sample_n(m.ctx, codes, 8, **kw)
    finally:
        check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"sample_rows_cap", 0), "dc_debug_set")
    for x, y in zip(a, base):
        np.testing.assert_array_equal(x, y)
    # a plain call that only asks for sample_logprob takes the row route too: at temperature 1 the two numbers are one
    tok, lp, lq = ops.lm_sample_n(m.ctx, codes[:32], 2, temperature=1.0, seed=3, want_sample_logprob=True)
    assert _rel(lq, lp).max() < 1e-6


def test_op_rows_do_not_depend_on_the_region_count(small):
    from densecap_amd import ops
    m, W = small
    codes = _codes(6500, m.fc_dim, 8)
    kw = dict(temperature=1.0, seed=5, top_k=40, top_p=0.9, want_sample_logprob=True)
    big = ops.lm_sample_n(m.ctx, codes, 2, **kw)
    assert np.isfinite(big[1]).all() and np.isfinite(big[2]).all()
    sub = np.array([0, 1, 2, 1000, 4095, 4096, 6499])
    a = ops.lm_sample_n(m.ctx, codes[sub], 2, row_ids=sub, **kw)
    for x, y in zip(a, big):
        np.testing.assert_array_equal(x, y[sub])


def test_sample_captions_bit_identities(full):
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, W = full
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=300)
    img = np.ascontiguousarray(make_synthetic_image(320, 480, 3), np.float32)
    m.setLanes(1)
    m.setCaptionOrder(True)
    kw = dict(temperature=1.0, seed=9, top_k=40, top_p=0.9, want_sample_logprob=True)
    b0, s0, t0 = m.forward_raw(img)
    base = m.sampleCaptions(img, 4, **kw)
    assert len(b0) > 0 and len(base) == 6
    np.testing.assert_array_equal(base[0], b0)
    np.testing.assert_array_equal(base[2], t0)
    fb, feats = m.extractFeatures(img)
    a = ops.lm_sample_n(m.ctx, feats, 4, **kw)
    for x, y in zip(a, base[3:]):
        np.testing.assert_array_equal(x, y)
    try:
        for lanes, order in ((3, 1), (3, 0), (1, 0)):
            m.setLanes(lanes)
            m.setCaptionOrder(bool(order))
            r = m.sampleCaptions(img, 4, **kw)
            for x, y in zip(r, base):
                np.testing.assert_array_equal(x, y)
    finally:
        m.setLanes(2)
        m.setCaptionOrder(True)


# ---- the distribution -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p,temperature", [(10, 1.0, 1.0), (0, 0.9, 1.0), (40, 0.5, 2.0)])
def test_first_words_follow_the_truncated_distribution(small, top_k, top_p, temperature):
    """8,192 draws of one region's first word (32 region rows x 256 draws of the same code) against the truncated, renormalised
    distribution: Pearson chi-square over the cells with expected count >= 5 (the rest pooled), and no draw outside the kept set."""
    from densecap_amd import ops
    from tests import sample_trunc_rules as TR
    from tests.test_sample_captions_cpu import first_step_scores
    m, W = small
    code = (np.random.default_rng(99).standard_normal((1, m.fc_dim)) * 2).astype(np.float32)
    dev, _ = ops.lm_sample_n(m.ctx, np.repeat(code, 32, 0), 256, temperature=temperature, seed=99, top_k=top_k, top_p=top_p)
    words = dev[:, :, 0].reshape(-1)
    x = first_step_scores(code[0], W)
    wide, _ = TR.wide_narrow(x, temperature, top_k, top_p, 2 * STAGE)
    kept = TR.kept_set(x, temperature, top_k, top_p)
    assert len(words) == 8192 and wide[words - 1].all(), np.unique(words[~wide[words - 1]])
    y = TR.scaled(x, temperature)[kept]
    p = np.exp(y - y.max()); p /= p.sum()
    exp = p * 8192
    counts = np.bincount(words - 1, minlength=len(x)).astype(np.float64)[kept]
    assert counts.sum() == 8192                          # zero draws outside the kept set
    big = exp >= 5
    o, e = list(counts[big]), list(exp[big])
    if (~big).any():
        o.append(counts[~big].sum()); e.append(exp[~big].sum())
    o, e = np.array(o), np.array(e)
    chi2, dof = float(((o - e) ** 2 / e).sum()), len(o) - 1
    limit = dof + 6.0 * np.sqrt(2.0 * dof)
    print("(%d, %g) at temperature %g: %d words kept, chi-square %.1f at dof %d (limit %.1f)" % (top_k, top_p, temperature, len(kept),
                                                                                              chi2, dof, limit))
    assert dof >= 3 and chi2 <= limit, (chi2, dof, limit)


# ---- rows without a word, refusals ---------------------------------------------------------------------------------------------
def test_non_finite_codes_end_the_row_cleanly(small):
    from densecap_amd import ops
    m, W = small
    codes = _codes(40, m.fc_dim, 6)
    kw = dict(temperature=1.0, seed=2, top_k=40, top_p=0.9, want_sample_logprob=True)
    base = ops.lm_sample_n(m.ctx, codes, 4, **kw)
    bad = codes.copy()
    bad[29, 100] = np.inf
    got = ops.lm_sample_n(m.ctx, bad, 4, **kw)
    good = np.setdiff1d(np.arange(40), [29])
    for x, y in zip(got, base):
        np.testing.assert_array_equal(x[good], y[good])
    assert (got[0][29] == 0).all() and np.isnan(got[1][29]).all() and np.isnan(got[2][29]).all(), (got[0][29], got[1][29])
    again = ops.lm_sample_n(m.ctx, codes, 4, **kw)
    for x, y in zip(again, base):
        np.testing.assert_array_equal(x, y)


def test_refusals_leave_the_ctx_working(small):
    from densecap_amd import _lib, ops
    m, W = small
    lib = m.lib
    codes = _codes(16, m.fc_dim, 4)
    base = ops.lm_sample_n(m.ctx, codes, 2, temperature=1.0, seed=1, top_k=5)
    cd = m.ctx.to_device(codes)
    tok = m.ctx.empty((16, 2, 15), np.int32); lp = m.ctx.empty((16, 2), np.float32); lq = m.ctx.empty((16, 2), np.float32)
    O, Tr = _lib.DcSampleOpts, _lib.DcSampleTrunc
    bad = [(O(2, 1.0, 0), Tr(-1, 1.0), "top_k must be"), (O(2, 1.0, 0), Tr(202, 1.0), "top_k must be"),
           (O(2, 1.0, 0), Tr(0, 0.0), "top_p must be"), (O(2, 1.0, 0), Tr(0, 1.5), "top_p must be"),
           (O(2, 1.0, 0), Tr(0, float("nan")), "top_p must be"), (O(1, 0.0, 0), Tr(5, 1.0), "greedy rule"),
           (O(1, 0.0, 0), Tr(0, 0.5), "greedy rule"), (O(0, 1.0, 0), Tr(5, 1.0), "num_samples must be")]
    for o, t, msg in bad:
        assert lib.dc_op_lm_sample_n_trunc(m.ctx.h, cd.ptr, 16, None, C.byref(o), C.byref(t), tok.ptr, lp.ptr, None) == -1
        assert msg in lib.dc_last_error(m.ctx.h).decode(), lib.dc_last_error(m.ctx.h)
    o = O(1, 0.0, 0)
    assert lib.dc_op_lm_sample_n_trunc(m.ctx.h, cd.ptr, 16, None, C.byref(o), None, tok.ptr, lp.ptr, lq.ptr) == -1     # sample_logprob at temperature 0
    assert "greedy rule" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_op_lm_sample_n_trunc(m.ctx.h, cd.ptr, 16, None, None, None, tok.ptr, lp.ptr, None) < 0
    assert "null options" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_op_lm_sample_n_trunc(m.ctx.h, None, 16, None, C.byref(O(2, 1.0, 0)), None, tok.ptr, lp.ptr, None) < 0
    assert "null pointer" in lib.dc_last_error(m.ctx.h).decode()
    again = ops.lm_sample_n(m.ctx, codes, 2, temperature=1.0, seed=1, top_k=5)
    for x, y in zip(again, base):
        np.testing.assert_array_equal(x, y)


# ---- Python against C, the CLI -------------------------------------------------------------------------------------------------
def test_python_against_the_c_call(small):
    from densecap_amd import _lib
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    img = np.ascontiguousarray(make_synthetic_image(160, 224, 1), np.float32)
    boxes, scores, tokens, samples, lp, lq = m.sampleCaptions(img, 3, temperature=0.8, seed=5, top_k=20, top_p=0.95,
                                                              want_sample_logprob=True)
    K = len(boxes)
    assert samples.shape == (K, 3, 15) and lp.shape == (K, 3) and lq.shape == (K, 3) and K > 0
    assert (lq <= 0).all() and np.isfinite(lq).all()
    five = m.sampleCaptions(img, 3, temperature=0.8, seed=5, top_k=20, top_p=0.95)
    assert len(five) == 5
    np.testing.assert_array_equal(five[3], samples)
    P = m._capacity(160, 224)
    r, rb, rs, rt = m._new_result(P)
    sm = np.zeros((P, 3, 15), np.int32); sl = np.zeros((P, 3), np.float32); sq = np.zeros((P, 3), np.float32)
    o, t = _lib.DcSampleOpts(3, 0.8, 5), _lib.DcSampleTrunc(20, 0.95)
    _lib.check(m.ctx.h, m.lib.dc_sample_captions_trunc(m.ctx.h, img.ctypes.data, 160, 224, 0, C.byref(o), C.byref(t), C.byref(r),
                                                       sm.ctypes.data, sl.ctypes.data, sq.ctypes.data), "dc_sample_captions_trunc")
    assert r.K == K
    np.testing.assert_array_equal(sm[:K], samples)
    np.testing.assert_array_equal(sl[:K], lp)
    np.testing.assert_array_equal(sq[:K], lq)


def test_cli(tmp_path, monkeypatch):
    from PIL import Image
    from densecap_amd import DenseCapModel, run_model
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(120, 160), (140, 100)]):
        rgb = (np.random.default_rng(i).random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(d / ("im%d.png" % i)))
    calls = []
    real = DenseCapModel.sampleCaptions

    def watched(self, img, *a, **kw):
        calls.append((a, kw))
        return real(self, img, *a, **kw)
    monkeypatch.setattr(DenseCapModel, "sampleCaptions", watched)
    common = ["-input_dir", str(d), "-synthetic_weights", "1", "-num_proposals", "50", "-image_size", "160"]
    # the truncation flags alone make no sampling call and leave no trace in `opt`
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "plain"), "-top_k", "5", "-top_p", "0.5"]) == 0
    assert calls == []
    plain = json.load(open(tmp_path / "plain" / "results.json"))
    assert not set(run_model.SAMPLING_FLAGS) & set(plain["opt"])
    assert all(set(e) == {"boxes", "scores", "captions", "img_name"} for e in plain["results"])
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "trunc"), "-num_samples", "2", "-temperature", "0.5",
                                    "-sample_seed", "40", "-top_k", "7"]) == 0
    assert len(calls) == 2 and all(kw == dict(top_k=7, top_p=1.0, want_sample_logprob=True) for _, kw in calls)
    res = json.load(open(tmp_path / "trunc" / "results.json"))
    assert res["opt"]["top_k"] == 7 and res["opt"]["top_p"] == 1.0 and res["opt"]["num_samples"] == 2
    for e, p in zip(res["results"], plain["results"]):
        assert set(e) == {"boxes", "scores", "captions", "img_name", "sampled_captions", "sampled_logprobs", "sampled_sample_logprobs"}
        assert e["boxes"] == p["boxes"] and e["captions"] == p["captions"]
        K = len(e["boxes"])
        assert len(e["sampled_sample_logprobs"]) == K and all(len(r) == 2 for r in e["sampled_sample_logprobs"])
        assert all(np.isfinite(v) and v <= 0 for r in e["sampled_sample_logprobs"] for v in r)
    # sampling without truncation: the file is the one of the existing flag
    calls.clear()
    assert run_model.main(common + ["-output_vis_dir", str(tmp_path / "sampled"), "-num_samples", "2"]) == 0
    assert len(calls) == 2 and all(kw == {} for _, kw in calls)
    res = json.load(open(tmp_path / "sampled" / "results.json"))
    assert all("sampled_sample_logprobs" not in e and "sampled_logprobs" in e for e in res["results"])
    with pytest.raises(SystemExit):
        run_model.main(common + ["-num_samples", "2", "-top_p", "0"])
