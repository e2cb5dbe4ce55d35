"""Scoring captions on the GPU: dc_op_lm_score against the CPU restatement, its bit-identities (query order, queries
alone, chunking, region subsets), dc_score_captions against dc_forward_test / dc_extract_features, the refusals, and the
Python / CLI surface."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    """A model with a 200-word vocabulary for the restatement checks: V+1 = 201 columns padded to 256, so the last 32-column
    slot of the log-sum-exp epilogue holds padding only and the one before it is partly padding."""
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


def _queries(V, T, rng, n=40):
    """lengths 0..T, the ids 1 and V, repeated words."""
    Tq = T
    q = np.zeros((n, Tq), np.int32)
    for i in range(n):
        L = i % (T + 1)
        q[i, :L] = rng.integers(1, V + 1, L)
    q[1, 0] = 1
    q[2, :2] = [V, V]
    q[3, :3] = [1, V, 1]
    q[4, :4] = [7, 7, 7, 7]
    return q


def _codes(n, D, seed):
    return (np.random.default_rng(seed).standard_normal((n, D)) * 2).astype(np.float32)


def test_op_matches_restatement(small):
    from densecap_amd import ops
    from tests import score_restatement
    m, W = small
    q = _queries(200, 15, np.random.default_rng(0))
    codes = _codes(300, m.fc_dim, 1)
    got = ops.lm_score(m.ctx, codes, q)
    ref = score_restatement.lm_score(codes, W, q)
    assert got.shape == (300, len(q)) and np.isfinite(got).all()
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
    assert rel.max() < 1e-4, rel.max()


def test_op_bit_identities(small):
    from densecap_amd import ops
    m, W = small
    rng = np.random.default_rng(5)
    q = _queries(200, 15, rng, n=24)
    codes = _codes(300, m.fc_dim, 2)
    base = ops.lm_score(m.ctx, codes, q)
    perm = rng.permutation(len(q))
    np.testing.assert_array_equal(ops.lm_score(m.ctx, codes, q[perm]), base[:, perm])
    for i in (0, 5, 15):
        np.testing.assert_array_equal(ops.lm_score(m.ctx, codes, q[i:i + 1])[:, 0], base[:, i])
    from densecap_amd._lib import check
    check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"score_rows_cap", 700), "dc_debug_set")   # chunks of two queries
    try:
        np.testing.assert_array_equal(ops.lm_score(m.ctx, codes, q), base)
    finally:
        check(m.ctx.h, m.lib.dc_debug_set(m.ctx.h, b"score_rows_cap", 0), "dc_debug_set")
    sub = np.array([3, 17, 100, 101, 299])
    np.testing.assert_array_equal(ops.lm_score(m.ctx, codes[sub], q), base[sub])
    np.testing.assert_array_equal(ops.lm_score(m.ctx, codes[:150], q), base[:150])


def test_op_rows_do_not_depend_on_the_region_count(small):
    """6,500 regions: planned on that many rows, the image encoder (K = 4096) would leave the sequential-K kernels for the
    K-split kernel and its other summation order; the rows must still be those of a small call."""
    from densecap_amd import ops
    m, W = small
    q = np.array([[3, 9, 0], [0, 0, 0]], np.int32)
    codes = _codes(6500, m.fc_dim, 8)
    big = ops.lm_score(m.ctx, codes, q)
    assert np.isfinite(big).all()
    sub = np.array([0, 1, 2, 1000, 4095, 4096, 6499])
    np.testing.assert_array_equal(ops.lm_score(m.ctx, codes[sub], q), big[sub])


def _score(m, img, q, want_tokens=True):
    from densecap_amd import _lib
    P = m._capacity(img.shape[1], img.shape[2])
    r, boxes, scores, tokens = m._new_result(P)
    if not want_tokens:
        r.tokens = None
    loglik = np.full((P, q.shape[0]), np.nan, np.float32)
    _lib.check(m.ctx.h, m.lib.dc_score_captions(m.ctx.h, img.ctypes.data, img.shape[1], img.shape[2], 0, q.ctypes.data,
                                                q.shape[0], q.shape[1], C.byref(r), loglik.ctypes.data), "dc_score_captions")
    K = r.K
    return boxes[:K], scores[:K], tokens[:K], loglik[:K]


@pytest.mark.parametrize("H,W,P", [(600, 720, 1000), (160, 224, 50)])
@pytest.mark.parametrize("order", [0, 1])
def test_score_captions_matches_forward_and_op(full, H, W, P, order):
    from densecap_amd import ops
    from densecap_amd.weights import make_synthetic_image
    m, Wt = full
    m.setCaptionOrder(bool(order))
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    img = np.ascontiguousarray(make_synthetic_image(H, W, 3), np.float32)
    q = _queries(10497, 15, np.random.default_rng(9), n=12)
    b0, s0, t0 = m.forward_raw(img)
    m.mfma_profile(1)                            # count the MFMA launches of each call from here on
    b1, s1, t1, ll = _score(m, img, q)
    with_tokens = m.mfma_profile(1)["launches"]
    assert len(b0) > 0 and np.isfinite(ll).all()
    np.testing.assert_array_equal(b1, b0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(t1, t0)
    # no tokens wanted: the forward runs without the language model (>= T fewer GEMM launches), same boxes, scores, loglik
    b2, s2, _, ll2 = _score(m, img, q, want_tokens=False)
    without_tokens = m.mfma_profile(-1)["launches"]
    assert without_tokens <= with_tokens - int(Wt["seq_length"]), (with_tokens, without_tokens)
    np.testing.assert_array_equal(b2, b0)
    np.testing.assert_array_equal(s2, s0)
    np.testing.assert_array_equal(ll2, ll)
    fb, feats = m.extractFeatures(img)
    np.testing.assert_array_equal(fb, b0)
    np.testing.assert_array_equal(ll, ops.lm_score(m.ctx, feats, q))
    b3, s3, t3 = m.forward_raw(img)
    np.testing.assert_array_equal(b3, b0)
    np.testing.assert_array_equal(s3, s0)
    np.testing.assert_array_equal(t3, t0)
    m.setCaptionOrder(True)


def test_refusals_leave_the_ctx_working(small):
    from densecap_amd import Context, ops
    from densecap_amd._lib import DenseCapError
    from densecap_amd.weights import make_synthetic_image
    m, W = small
    V = 200
    codes = _codes(8, m.fc_dim, 4)
    ok = np.array([[5, 6, 0]], np.int32)
    base = ops.lm_score(m.ctx, codes, ok)
    bad = [
        (np.zeros((0, 3), np.int32), "Q must be >= 1"),
        (np.zeros((1, 65), np.int32), "Tq must be in 1..64"),
        (np.array([[5, 0, 6]], np.int32), "query 0, column 2: a word after a zero"),
        (np.array([[0, 0], [V + 1, 0]], np.int32), "query 1, column 0: token 201 is outside 1..200"),
        (np.array([[V + 2]], np.int32), "token 202 is outside"),
        (np.array([[3, -4]], np.int32), "token -4 is outside"),
    ]
    for q, msg in bad:
        with pytest.raises(DenseCapError, match=msg):
            ops.lm_score(m.ctx, codes, q)
    lib = m.lib
    assert lib.dc_op_lm_score(m.ctx.h, None, 8, None, 1, 3, None) < 0
    assert "null pointer" in lib.dc_last_error(m.ctx.h).decode()
    img = np.ascontiguousarray(make_synthetic_image(160, 224, 1), np.float32)
    q = np.array([[5, 0]], np.int32)
    r, *_ = m._new_result(1)
    ll = np.zeros((1, 1), np.float32)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    assert lib.dc_score_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, q.ctypes.data, 1, 2, C.byref(r), ll.ctypes.data) < 0
    assert "out->capacity is 1" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_score_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, q.ctypes.data, 1, 0, C.byref(r), ll.ctypes.data) < 0
    assert "Tq must be" in lib.dc_last_error(m.ctx.h).decode()
    assert lib.dc_score_captions(m.ctx.h, img.ctypes.data, 160, 224, 0, None, 1, 2, C.byref(r), ll.ctypes.data) < 0
    assert "null pointer" in lib.dc_last_error(m.ctx.h).decode()
    ctx = Context(0)
    try:
        assert lib.dc_op_lm_score(ctx.h, None, 8, None, 1, 3, None) < 0
        assert "weights not loaded" in lib.dc_last_error(ctx.h).decode()
        assert lib.dc_score_captions(ctx.h, img.ctypes.data, 160, 224, 0, q.ctypes.data, 1, 2, C.byref(r), ll.ctypes.data) < 0
        assert "weights not loaded" in lib.dc_last_error(ctx.h).decode()
    finally:
        ctx.close()
    np.testing.assert_array_equal(ops.lm_score(m.ctx, codes, ok), base)
    b, s, L = m.scoreCaptions(img, q)
    assert L.shape == (len(b), 1) and np.isfinite(L).all()


def test_score_captions_python_and_cli(tmp_path, full):
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    W = make_synthetic_weights(seed=1234, vocab_size=200, seq_length=8)
    m = DenseCapModel(W, device=0)
    try:
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
        img = make_synthetic_image(160, 224, 1)
        boxes, scores, ll, caps = m.scoreCaptions(img, ["w12 w7", "w3"], return_captions=True)
        b0, s0, c0 = m.forward_test(img)
        np.testing.assert_array_equal(boxes, b0)
        assert caps == c0 and ll.shape == (len(boxes), 2)
        ll2 = m.scoreCaptions(img, np.array([[12, 7], [3, 0]], np.int32))[2]
        np.testing.assert_array_equal(ll, ll2)
    finally:
        m.ctx.close()
    from PIL import Image
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(120, 160), (140, 100)]):
        rgb = (np.random.default_rng(i).random((h, w, 3)) * 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(d / ("im%d.png" % i)))
    out = tmp_path / "q.json"
    subprocess.check_call([sys.executable, "-m", "densecap_amd.query_regions", "-input_dir", str(d), "-query", "w12 w7",
                           "-query", "w3", "-topk", "3", "-synthetic_weights", "1", "-num_proposals", "50",
                           "-image_size", "160", "-output_json", str(out)], cwd=ROOT)
    res = json.load(open(out))
    assert res["queries"] == ["w12 w7", "w3"] and len(res["images"]) == 2 and len(res["ranking"]) == 2
    for im in res["images"]:
        for qi, r in enumerate(im["results"]):
            assert r["query"] == res["queries"][qi] and r["words"] == (2 if qi == 0 else 1)
            regs = r["regions"]
            assert 1 <= len(regs) <= 3
            lls = [g["loglik"] for g in regs]
            assert lls == sorted(lls, reverse=True)
            for g in regs:
                assert set(g) == {"box", "score", "loglik", "loglik_per_word", "caption"} and len(g["box"]) == 4
                assert abs(g["loglik_per_word"] - g["loglik"] / (r["words"] + 1)) < 1e-6
    # the whole loglik columns of the same images and settings (the CLI's synthetic weights are `full`'s): the reported
    # regions are each column's top-k, the first one its arg-max
    from densecap_amd.run_model import load_image_caffe
    fm, _ = full
    fm.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=50)
    for im in res["images"]:
        _, _, cols = fm.scoreCaptions(load_image_caffe(im["image"], 160)[0], ["w12 w7", "w3"])
        assert np.isfinite(cols).all() and len(cols) >= 1
        for qi, r in enumerate(im["results"]):
            col = cols[:, qi]
            assert r["regions"][0]["loglik"] == float(col.max())
            best_k = [e for e in res["ranking"][qi]["images"] if e["image"] == im["image"]][0]["best_region"]
            assert best_k == int(np.argmax(col))
            np.testing.assert_array_equal([g["loglik"] for g in r["regions"]], np.sort(col)[::-1][:len(r["regions"])])
    for qi, rk in enumerate(res["ranking"]):
        best = [e["best_loglik"] for e in rk["images"]]
        assert best == sorted(best, reverse=True) and len(best) == 2
        for e in rk["images"]:
            im = [x for x in res["images"] if x["image"] == e["image"]][0]
            assert e["best_loglik"] == im["results"][qi]["regions"][0]["loglik"]
