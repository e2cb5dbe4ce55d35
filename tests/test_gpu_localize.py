"""Localising phrases on the GPU (dc_localize_captions): the reference is built from the device's own data -- the corners, the
objectness and, through scoreCaptions under final_nms_thresh = 0, the log-likelihoods of all proposals -- and the rules of
tests/nms_multi_rules.py; every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import nms_multi_rules as R

pytestmark = pytest.mark.gpu

P = 130                                                    # three mask words, the last one ragged
QUERIES = np.array([[0, 0, 0], [5, 0, 0], [9, 17, 3]], np.int32)     # 0, 1 and 3 words
# (image H, W, seed, rpn_nms_thresh): the second is small enough that the RPN NMS keeps fewer than P rows
IMAGES = {"full": (240, 320, 3, 0.7), "short": (96, 128, 4, 0.2)}


@pytest.fixture(scope="module")
def model():
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=21, vocab_size=200, seq_length=15)
    m = DenseCapModel(W, device=0)
    yield m
    m.ctx.close()


def _image(name):
    from densecap_amd.weights import make_synthetic_image
    H, W, seed, _ = IMAGES[name]
    return np.ascontiguousarray(make_synthetic_image(H, W, seed), np.float32)


def _args(m, name, final=0.3):
    m.setTestArgs(rpn_nms_thresh=IMAGES[name][3], final_nms_thresh=final, num_proposals=P)


def _localize(m, img, q, thresh=0.3, M=5, min_obj=None, want_tokens=True, rc_only=False, null=()):
    """The library call itself: (rc) or dict of the raw arrays (rows past count filled with a sentinel) plus `out`.
    null: names of the pointers to pass as NULL."""
    from densecap_amd import _lib
    m._push_test_args()
    r, boxes, scores, tokens = m._new_result(P)
    if not want_tokens:
        r.tokens = None
    Q = q.shape[0]
    o = _lib.DcLocalizeOpts(thresh, M, float("-inf") if min_obj is None else min_obj)
    Mb = max(1, min(M, 4096))
    cnt = np.full((Q,), -7, np.int32); lb = np.full((Q, Mb, 4), -7, np.float32); ll = np.full((Q, Mb), -7, np.float32)
    lo = np.full((Q, Mb), -7, np.float32); reg = np.full((Q, Mb), -7, np.int32)
    ptr = lambda a, k: None if k in null else a.ctypes.data
    rc = m.lib.dc_localize_captions(m.ctx.h, ptr(img, "img"), img.shape[1], img.shape[2], 0, ptr(q, "q"), Q, q.shape[1],
                                    None if "opts" in null else C.byref(o), None if "out" in null else C.byref(r),
                                    ptr(cnt, "count"), ptr(lb, "boxes"), ptr(ll, "loglik"), ptr(lo, "objectness"), ptr(reg, "region"))
    if rc_only:
        return rc
    _lib.check(m.ctx.h, rc, "dc_localize_captions")
    K = r.K
    final_idx = m.debug_fetch("final_nms_idx", (P,), np.int32)[0][:K].copy()      # the final picks of this call's forward
    return dict(count=cnt, boxes=lb, loglik=ll, objectness=lo, region=reg, out_boxes=boxes[:K].copy(), out_scores=scores[:K].copy(),
                out_tokens=tokens[:K].copy(), final_idx=final_idx)


_REF = {}


def _reference(m, name):
    """Computed once per image, from the device's own data: corners, final boxes and objectness of the n = count1 proposals, and
    the (n, Q) log-likelihoods of scoreCaptions under final_nms_thresh = 0 (its rows are the proposals in order)."""
    if name not in _REF:
        img = _image(name)
        _args(m, name, final=0.0)
        fb, fs, ll = m.scoreCaptions(img, QUERIES)
        n = int(m.debug_fetch("rpn_nms_count", (1,), np.int32)[0][0])
        assert len(fb) == n and ll.shape == (n, 3) and np.isfinite(ll).all()
        xyxy = m.debug_fetch("final_x1y1x2y2", (P, 4))[0][:n].copy()
        obj = m.debug_fetch("obj", (P,))[0][:n].copy()
        boxes = m.debug_fetch("final_boxes", (P, 4))[0][:n].copy()
        assert np.array_equal(boxes, fb) and np.array_equal(obj, fs)
        _REF[name] = dict(img=img, n=n, xyxy=xyxy, obj=obj, boxes=boxes, ll=ll)
    return _REF[name]


def _expect(ref, got, thresh, M, valid=None, cols=(0, 1, 2), what=""):
    """picks, boxes, loglik and objectness of `got` are those of the reference, bit for bit; rows past count are untouched;
    region is consistent with `out`: out row `region` is the same proposal with the same box and score, and region is -1 exactly
    for a proposal that is not among the final picks."""
    picks = R.nms_multi_ref(ref["xyxy"], ref["ll"][:, list(cols)], thresh, M, valid)
    kept = set(got["final_idx"].tolist())
    assert len(kept) == len(got["final_idx"]) == len(got["out_boxes"])
    for i, q in enumerate(cols):
        c = int(got["count"][i])
        assert c == len(picks[i]), "%s: query %d: %d picks, expected %d" % (what, q, c, len(picks[i]))
        rows = picks[i]
        assert np.array_equal(got["boxes"][i, :c], ref["boxes"][rows]), (what, q)
        assert np.array_equal(got["loglik"][i, :c], ref["ll"][rows, q]), (what, q)
        assert np.array_equal(got["objectness"][i, :c], ref["obj"][rows]), (what, q)
        for j, r in enumerate(rows):
            k = int(got["region"][i, j])
            if r in kept:
                assert 0 <= k < len(got["out_boxes"]) and got["final_idx"][k] == r, (what, q, j, k)
                assert np.array_equal(got["out_boxes"][k], got["boxes"][i, j]) and got["out_scores"][k] == got["objectness"][i, j]
            else:
                assert k == -1, (what, q, j, k)
        for a in ("boxes", "loglik", "objectness", "region"):
            assert (got[a][i, c:] == -7).all(), "%s: query %d: %s written past count" % (what, q, a)
    return picks


@pytest.mark.parametrize("name", ["full", "short"])
def test_localize_equals_the_reference(model, name):
    ref = _reference(model, name)
    if name == "full":
        assert ref["n"] == P
    else:
        assert 1 <= ref["n"] < P, "the small image must leave the RPN NMS with fewer than %d rows (got %d)" % (P, ref["n"])
    base = None
    for final in (0.3, 0.0):
        for order in (False, True):
            for want_tokens in (True, False):
                model.setCaptionOrder(order)
                _args(model, name, final)
                got = _localize(model, ref["img"], QUERIES, 0.3, 5, want_tokens=want_tokens)
                what = "%s final=%g order=%d tokens=%d" % (name, final, order, want_tokens)
                _expect(ref, got, 0.3, 5, what=what)
                mine = {k: got[k] for k in ("count", "boxes", "loglik", "objectness")}
                if base is None:
                    base = mine
                for k in mine:                                     # identical whatever the final NMS, the order, the decode
                    assert np.array_equal(mine[k], base[k]), (what, k)
                if final == 0.0:
                    assert (got["region"][got["region"] != -7] >= 0).all()
    model.setCaptionOrder(False)
    _args(model, name, 0.3)
    got = _localize(model, ref["img"], QUERIES, 0.3, 5)
    b0, s0, t0 = model.forward_raw(ref["img"])                     # `out` is what dc_forward_test returns
    assert np.array_equal(got["out_boxes"], b0) and np.array_equal(got["out_scores"], s0) and np.array_equal(got["out_tokens"], t0)
    if name == "full":
        assert len(b0) < ref["n"], "the final NMS drops nothing: region = -1 is not exercised"


@pytest.mark.parametrize("thresh,M", [(0.0, 130), (0.5, 1), (1.0, 64), (0.7, 4096)])
def test_thresholds_and_budgets(model, thresh, M):
    ref = _reference(model, "full")
    _args(model, "full", 0.3)
    got = _localize(model, ref["img"], QUERIES, thresh, M)
    picks = _expect(ref, got, thresh, M, what="thresh=%g M=%d" % (thresh, M))
    if thresh == 1.0:
        assert [len(p) for p in picks] == [64] * 3                 # nothing is suppressed: the budget ends the walk at a chunk's end


def test_a_query_alone_or_with_others(model):
    ref = _reference(model, "full")
    _args(model, "full", 0.3)
    both = _localize(model, ref["img"], QUERIES, 0.3, 7)
    for q in range(3):
        one = _localize(model, ref["img"], np.ascontiguousarray(QUERIES[q:q + 1]), 0.3, 7)
        _expect(ref, one, 0.3, 7, cols=(q,), what="query %d alone" % q)
        for k in ("count", "boxes", "loglik", "objectness", "region"):
            assert np.array_equal(one[k][0], both[k][q]), (q, k)
    rev = _localize(model, ref["img"], np.ascontiguousarray(QUERIES[::-1]), 0.3, 7)
    for k in ("count", "boxes", "loglik", "objectness", "region"):
        assert np.array_equal(rev[k][::-1], both[k]), k


@pytest.mark.parametrize("name", ["full", "short"])
def test_min_objectness(model, name):
    ref = _reference(model, name)
    _args(model, name, 0.3)
    med = float(np.float32(np.median(ref["obj"])))
    got = _localize(model, ref["img"], QUERIES, 0.3, 9, min_obj=med)
    valid = ref["obj"] >= np.float32(med)
    assert 0 < valid.sum() < ref["n"]
    _expect(ref, got, 0.3, 9, valid, what="min_objectness = median")
    assert (got["objectness"][got["objectness"] != -7] >= np.float32(med)).all()
    none = _localize(model, ref["img"], QUERIES, 0.3, 9, min_obj=float("inf"))
    assert none["count"].tolist() == [0, 0, 0]
    _expect(ref, _localize(model, ref["img"], QUERIES, 0.3, 9, min_obj=-1e30), 0.3, 9, what="min_objectness below every score")


def test_refusals(model):
    from densecap_amd._lib import DenseCapError
    ref = _reference(model, "full")
    _args(model, "full", 0.3)
    img = ref["img"]
    INVALID, UNSUPPORTED = -1, -5
    nan = float("nan")
    for kw in (dict(thresh=-0.01), dict(thresh=1.01), dict(thresh=nan), dict(M=0), dict(M=-1), dict(M=4097), dict(min_obj=nan)):
        assert _localize(model, img, QUERIES, rc_only=True, **kw) == INVALID, kw
    for k in ("img", "q", "opts", "out", "count", "boxes", "loglik", "objectness", "region"):
        assert _localize(model, img, QUERIES, rc_only=True, null=(k,)) == INVALID, k
    bad = QUERIES.copy(); bad[1, 0] = 201                            # outside 1..V
    assert _localize(model, img, bad, rc_only=True) == INVALID
    bad = QUERIES.copy(); bad[1] = [0, 5, 0]                         # a word after a zero
    assert _localize(model, img, bad, rc_only=True) == INVALID
    # the Python method refuses the same ranges before the library is called
    for kw in (dict(nms_thresh=-0.1), dict(nms_thresh=1.5), dict(nms_thresh=nan), dict(max_regions=0), dict(max_regions=4097),
               dict(max_regions=2.5), dict(min_objectness=nan)):
        with pytest.raises(ValueError):
            model.localizeCaptions(img, QUERIES, **kw)
    # uncapped proposals on this image: 15 x 20 x 12 = 3600 rows fit, a 320 x 480 image (20 x 30 x 12 = 7200) does not
    from densecap_amd.weights import make_synthetic_image
    model.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=-1)
    big = np.ascontiguousarray(make_synthetic_image(320, 480, 5), np.float32)
    with pytest.raises(DenseCapError, match=r"\(-5\)"):
        model.localizeCaptions(big, QUERIES)
    assert UNSUPPORTED == -5
    _args(model, "full", 0.3)
    _expect(ref, _localize(model, img, QUERIES, 0.3, 5), 0.3, 5, what="after the refusals")


def test_python_and_query_regions_surface(model):
    from densecap_amd import query_regions
    from densecap_amd.run_model import xcycwh_to_xywh
    ref = _reference(model, "full")
    _args(model, "full", 0.3)
    raw = _localize(model, ref["img"], QUERIES, 0.3, 4)
    boxes, scores, captions, found = model.localizeCaptions(ref["img"], QUERIES, 0.3, 4, return_captions=True)
    assert np.array_equal(boxes, raw["out_boxes"]) and len(captions) == len(boxes) and len(found) == 3
    for q, f in enumerate(found):
        c = int(raw["count"][q])
        assert c >= 1 and np.array_equal(f["boxes"], raw["boxes"][q, :c]) and np.array_equal(f["loglik"], raw["loglik"][q, :c])
        assert np.array_equal(f["objectness"], raw["objectness"][q, :c]) and np.array_equal(f["region"], raw["region"][q, :c])
    words = ["", "w5", "w9 w17 w3"]                                   # QUERIES as strings
    res = query_regions.query_images(model, [("a", ref["img"][None])], words, 4,
                                     localize={"nms_thresh": 0.3, "max_regions": 4, "min_objectness": None})
    assert res["queries"] == words and len(res["images"]) == 1 and len(res["ranking"]) == 3
    for q, r in enumerate(res["images"][0]["results"]):
        c = int(raw["count"][q])
        assert r["words"] == (0, 1, 3)[q] and len(r["regions"]) == c
        xywh = xcycwh_to_xywh(raw["boxes"][q, :c])
        for j, g in enumerate(r["regions"]):
            k = int(raw["region"][q, j])
            assert set(g) == {"box", "score", "loglik", "loglik_per_word", "region"} | ({"caption"} if k >= 0 else set())
            assert g["box"] == [float(v) for v in xywh[j]] and g["loglik"] == float(raw["loglik"][q, j])
            assert g["score"] == float(raw["objectness"][q, j]) and g["region"] == k
            if k >= 0:
                assert g["caption"] == captions[k]
        top = res["ranking"][q]["images"][0]
        assert top["best_loglik"] == r["regions"][0]["loglik"] and top["best_box"] == r["regions"][0]["box"]
        assert top["best_region"] == r["regions"][0]["region"]
