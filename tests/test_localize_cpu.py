"""CPU: the host side of localising phrases -- argument rules of DenseCapModel.localizeCaptions and of the query_regions flags
(checked before any library call), the JSON shape with -localize 1, the unchanged output without it, and header = exports = cdef
for the new entry points."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_localize_args_are_checked_before_the_library():
    from densecap_amd import _lib
    from densecap_amd.model import DenseCapModel
    from densecap_amd.ops import check_localize_args
    o = check_localize_args(0.3, 5, None)
    assert isinstance(o, _lib.DcLocalizeOpts) and o.max_regions == 5 and o.min_objectness == float("-inf")
    assert abs(o.nms_thresh - 0.3) < 1e-7
    assert check_localize_args(0, 1, -2.5).min_objectness == -2.5 and check_localize_args(1, 4096, float("inf")).max_regions == 4096
    bad = [dict(nms_thresh=-1e-3), dict(nms_thresh=1.001), dict(nms_thresh=NAN), dict(max_regions=0), dict(max_regions=-3),
           dict(max_regions=4097), dict(max_regions=1.5), dict(min_objectness=NAN)]
    m = DenseCapModel.__new__(DenseCapModel)              # no ctx, no library: the checks must come first
    for kw in bad:
        args = dict(dict(nms_thresh=0.3, max_regions=5, min_objectness=None), **kw)
        with pytest.raises(ValueError):
            check_localize_args(**args)
        with pytest.raises(ValueError):
            m.localizeCaptions(np.zeros((1, 3, 64, 64), np.float32), ["w1"], **kw)


def test_query_regions_flags():
    from densecap_amd import query_regions as qr
    parse = lambda *a: qr.build_parser().parse_args(["-query", "w1"] + list(a))
    assert qr.localize_options(parse()) is None and qr.localize_options(parse("-localize", "0")) is None
    assert qr.localize_options(parse("-localize", "1")) == {"nms_thresh": 0.3, "max_regions": 5, "min_objectness": None}
    assert qr.localize_options(parse("-localize", "1", "-localize_nms_thresh", "0.5", "-min_objectness", "-1.5", "-topk", "9")) == {
        "nms_thresh": 0.5, "max_regions": 9, "min_objectness": -1.5}
    for bad in (("-localize", "2"), ("-localize", "1", "-localize_nms_thresh", "1.5"), ("-localize", "1", "-localize_nms_thresh", "nan"),
                ("-localize", "1", "-min_objectness", "nan"), ("-localize", "1", "-topk", "5000"), ("-min_objectness", "0.5"),
                ("-localize_nms_thresh", "0.5"), ("-localize_nms_thresh", "0.3")):
        with pytest.raises(SystemExit):
            qr.localize_options(parse(*bad))


class _FakeModel:
    """What query_images reads of a model, with canned numbers (no library)."""
    idx_to_token = {i: "w" + str(i) for i in range(1, 21)}
    boxes = np.array([[10, 20, 8, 6], [30, 40, 10, 10], [50, 60, 4, 2]], np.float32)
    scores = np.array([0.5, 0.25, -1.5], np.float32)
    captions = ["w1 w2", "w3", ""]

    def scoreCaptions(self, img, ids, return_captions=False):
        ll = np.array([[-3.5, -1.25], [-2.0, -1.25], [-7.0, -0.5]], np.float32)
        return self.boxes, self.scores, ll, self.captions

    def localizeCaptions(self, img, ids, nms_thresh=0.3, max_regions=5, min_objectness=None, return_captions=False):
        self.seen = (np.asarray(ids).tolist(), nms_thresh, max_regions, min_objectness, return_captions)
        found = [{"boxes": np.array([[70, 80, 2, 2], [30, 40, 10, 10]], np.float32), "loglik": np.array([-1.0, -2.0], np.float32),
                  "objectness": np.array([-3.0, 0.25], np.float32), "region": np.array([-1, 1], np.int32)},
                 {"boxes": np.zeros((0, 4), np.float32), "loglik": np.zeros((0,), np.float32),
                  "objectness": np.zeros((0,), np.float32), "region": np.zeros((0,), np.int32)}]
        return self.boxes, self.scores, self.captions, found


# json.dumps of query_images(_FakeModel(), [("a.jpg", None)], ["w4 w5", "w6"], 2) as the commit before -localize produced it
WITHOUT_LOCALIZE = (
    '{"queries": ["w4 w5", "w6"], "images": [{"image": "a.jpg", "results": [{"query": "w4 w5", "words": 2, '
    '"regions": [{"box": [25.5, 35.5, 10.0, 10.0], "score": 0.25, "loglik": -2.0, "loglik_per_word": '
    '-0.6666666666666666, "caption": "w3"}, {"box": [6.5, 17.5, 8.0, 6.0], "score": 0.5, "loglik": -3.5, '
    '"loglik_per_word": -1.1666666666666667, "caption": "w1 w2"}]}, {"query": "w6", "words": 1, "regions": [{"box":'
    ' [48.5, 59.5, 4.0, 2.0], "score": -1.5, "loglik": -0.5, "loglik_per_word": -0.25, "caption": ""}, {"box": '
    '[6.5, 17.5, 8.0, 6.0], "score": 0.5, "loglik": -1.25, "loglik_per_word": -0.625, "caption": "w1 w2"}]}]}], '
    '"ranking": [{"query": "w4 w5", "images": [{"image": "a.jpg", "best_loglik": -2.0, "best_region": 1}]}, '
    '{"query": "w6", "images": [{"image": "a.jpg", "best_loglik": -0.5, "best_region": 2}]}]}')


def test_output_without_localize_is_unchanged():
    from densecap_amd import query_regions as qr
    res = qr.query_images(_FakeModel(), [("a.jpg", None)], ["w4 w5", "w6"], 2)
    assert json.dumps(res) == WITHOUT_LOCALIZE
    assert json.dumps(qr.query_images(_FakeModel(), [("a.jpg", None)], ["w4 w5", "w6"], 2, None)) == WITHOUT_LOCALIZE


def test_json_shape_with_localize():
    from densecap_amd import query_regions as qr
    m = _FakeModel()
    loc = {"nms_thresh": 0.4, "max_regions": 2, "min_objectness": -1.0}
    res = qr.query_images(m, [("a.jpg", None), ("b.jpg", None)], ["w4 w5", "w6"], 2, loc)
    assert m.seen == ([[4, 5], [6, 0]], 0.4, 2, -1.0, True)
    json.loads(json.dumps(res))
    assert set(res) == {"queries", "images", "ranking"} and res["queries"] == ["w4 w5", "w6"]
    assert [im["image"] for im in res["images"]] == ["a.jpg", "b.jpg"]
    r0, r1 = res["images"][0]["results"]
    assert (r0["query"], r0["words"], r1["query"], r1["words"]) == ("w4 w5", 2, "w6", 1) and r1["regions"] == []
    a, b = r0["regions"]
    assert a == {"box": [69.5, 79.5, 2.0, 2.0], "score": -3.0, "loglik": -1.0, "loglik_per_word": -1.0 / 3, "region": -1}
    assert b == {"box": [25.5, 35.5, 10.0, 10.0], "score": 0.25, "loglik": -2.0, "loglik_per_word": -2.0 / 3, "region": 1,
                 "caption": "w3"}
    # the image ranking goes by the best localised box; an image without a pick for a query is not ranked for it
    assert res["ranking"][0] == {"query": "w4 w5", "images": [
        {"image": n, "best_loglik": -1.0, "best_region": -1, "best_box": [69.5, 79.5, 2.0, 2.0]} for n in ("a.jpg", "b.jpg")]}
    assert res["ranking"][1] == {"query": "w6", "images": []}


def test_header_exports_and_cdef_agree():
    from densecap_amd import _lib
    from tests.test_abi_and_host import _prototypes
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name in ("dc_op_nms_multi", "dc_localize_captions"):
        assert name in hp and name in _lib.EXPORTED_SYMBOLS and lp[name] == hp[name], name
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1, name
    struct = r"typedef struct dc_localize_opts \{ float nms_thresh; int32_t max_regions; float min_objectness; \} dc_localize_opts;"
    assert re.search(struct, hdr) and re.search(struct, cdef)
    assert [f[0] for f in _lib.DcLocalizeOpts._fields_] == ["nms_thresh", "max_regions", "min_objectness"]
    assert "final_x1y1x2y2" in open(os.path.join(ROOT, "include", "densecap_debug.h")).read()
    model_lua = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    assert "function Model:localizeCaptions" in model_lua and "C.dc_localize_captions(" in model_lua
