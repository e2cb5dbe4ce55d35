"""Caller-supplied boxes, host side (CPU only): what the new model.py methods hand to dc_forward_boxes /
dc_forward_boxes_images / dc_extract_features_boxes and what they return, against a recording stand-in for the library (as
tests/test_boundary_semantics.py does for the other forward methods); the box checks made before the library is called; and
the -input_boxes reader of run_model / extract_features."""
import ctypes as C
import json

import numpy as np
import pytest

from tests.test_boundary_semantics import _ForwardRecordingLib, _model

# entry point -> position among the arguments (the context is 0) of n (None: one image), of the box lists and of the flags
_ENTRIES = {"dc_forward_boxes": (None, 5, 6), "dc_forward_boxes_images": (4, 6, 7), "dc_extract_features_boxes": (4, 6, 7)}


class _BoxesRecordingLib(_ForwardRecordingLib):
    """Records the box lists of every call on caller-supplied boxes (contents copied while the call is in progress) and, like
    the library, returns K = n rows per image with src = n-1 .. 0."""

    def __init__(self):
        super().__init__()
        self.lists = []

    def __getattr__(self, name):
        fn = _ForwardRecordingLib.__getattr__(self, name)
        if name not in _ENTRIES:
            return fn

        def rec(*args):
            n_at, bl_at, _ = _ENTRIES[name]
            n = 1 if n_at is None else args[n_at]
            bl = args[bl_at]
            seen = []
            for i in range(n):
                k = bl[i].n
                seen.append(np.ctypeslib.as_array(bl[i].boxes, shape=(k, 4)).copy())
                for r in range(k):
                    bl[i].src[r] = k - 1 - r
                if name == "dc_extract_features_boxes":
                    args[-1][i] = k
                else:
                    args[-1][i].K = k
            self.lists.append(seen)
            return fn(*args)
        return rec


def _boxes(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(1, 90, n), rng.uniform(1, 60, n), rng.uniform(2, 40, n), rng.uniform(2, 40, n)], 1).astype(np.float32)


def test_every_boxes_method_passes_sizes_lists_and_capacities():
    from densecap_amd.ops import DeviceArray
    m, _ = _model()
    m.setTestArgs(num_proposals=40)
    lib = m.lib = m.ctx.lib = _BoxesRecordingLib()
    T, D, P = m.seq_length, m.fc_dim, 40
    sizes = [(64, 96), (80, 48)]
    counts = [5, 3]
    lists = [_boxes(n, i) for i, n in enumerate(counts)]

    def host(hw):
        return np.zeros((3,) + hw, np.float32)

    def dev(i, hw):
        a = DeviceArray(m.ctx, (3,) + hw, np.float32)
        a.ptr = C.c_void_p(0x10000 * (i + 1))
        return a

    det = [((4,), np.float32), ((), np.float32), ((T,), np.int32), ((), np.int32)]
    feat = [((4,), np.float32), ((D,), np.float32), ((), np.int32)]
    cases = [
        ("forward_boxes", lambda clip: [m.forward_boxes(host(sizes[0]), lists[0], clip=clip)], "dc_forward_boxes", 1, 0, det),
        ("forward_boxes_device", lambda clip: [m.forward_boxes_device(dev(0, sizes[0]), lists[0], clip=clip)],
         "dc_forward_boxes", 1, 1, det),
        ("forward_boxes_images", lambda clip: m.forward_boxes_images([host(hw) for hw in sizes], lists, clip=clip),
         "dc_forward_boxes_images", 2, 0, det),
        ("forward_boxes_images_device",
         lambda clip: m.forward_boxes_images_device([dev(i, hw) for i, hw in enumerate(sizes)], lists, clip=clip),
         "dc_forward_boxes_images", 2, 1, det),
        ("extractFeatures_boxes", lambda clip: m.extractFeatures_boxes([host(hw) for hw in sizes], lists, clip=clip),
         "dc_extract_features_boxes", 2, 0, feat),
        ("extractFeatures_boxes_device",
         lambda clip: m.extractFeatures_boxes_device([dev(i, hw) for i, hw in enumerate(sizes)], lists, clip=clip),
         "dc_extract_features_boxes", 2, 1, feat),
    ]
    for what, call, entry, n, on_dev, widths in cases:
        for clip in (False, True):
            lib.raw.clear(); lib.lists.clear()
            out = call(clip)
            hits = [c for c in lib.raw if c[0] in _ENTRIES]
            assert [c[0] for c in hits] == [entry], what
            names = [c[0] for c in lib.raw]
            assert names.index("dc_set_test_args") < names.index(entry), what
            args = hits[0][1:]
            n_at, bl_at, flags_at = _ENTRIES[entry]
            assert args[flags_at] == (1 if clip else 0), what                  # DC_BOXES_CLIP
            if n_at is None:
                assert tuple(args[2:5]) == sizes[0] + (on_dev,), what
                assert [r.capacity for r in [args[-1][0]]] == [P], what
            else:
                assert [list(args[2])[:n], list(args[3])[:n]] == [[hw[0] for hw in sizes], [hw[1] for hw in sizes]], what
                assert (args[4], args[5]) == (n, on_dev), what
                if entry == "dc_extract_features_boxes":
                    assert args[8] == max(counts), what                          # capacity: the longest list
                else:
                    assert [args[-1][i].capacity for i in range(n)] == [P] * n, what
            # the box lists: contents, counts, a src buffer each
            assert len(lib.lists) == 1 and len(lib.lists[0]) == n, what
            for got, want in zip(lib.lists[0], lists):
                np.testing.assert_array_equal(got, want)
            # what comes back: K = n rows per image and the src the library wrote
            assert len(out) == n
            for i, parts in enumerate(out):
                assert len(parts) == len(widths), what
                for a, (w, dt) in zip(parts, widths):
                    assert a.dtype == dt and a.shape == (counts[i],) + w and a.flags.owndata, what
                np.testing.assert_array_equal(parts[-1], np.arange(counts[i])[::-1])
    # empty lists: the test args still travel, no entry point is called; a length mismatch is refused
    for method in (m.forward_boxes_images, m.forward_boxes_images_device, m.extractFeatures_boxes, m.extractFeatures_boxes_device):
        lib.raw.clear()
        assert method([], []) == []
        assert [c[0] for c in lib.raw] == ["dc_set_test_args"]
        with pytest.raises(ValueError, match="1 images but 2 box lists"):
            method([host(sizes[0])], lists)


def test_boxes_are_checked_before_the_library_is_called():
    m, _ = _model()
    m.setTestArgs(num_proposals=8)
    lib = m.lib = m.ctx.lib = _BoxesRecordingLib()
    img = np.zeros((3, 64, 96), np.float32)
    good = _boxes(6)

    def bad(i, col, v):
        b = good.copy(); b[i, col] = v
        return b

    cases = [(bad(3, 0, np.nan), "image 0: box 3 "), (bad(5, 1, np.inf), "image 0: box 5 "), (bad(2, 2, 0.0), "image 0: box 2 "),
             (bad(4, 3, -1.0), "image 0: box 4 "), (bad(1, 2, np.inf), "image 0: box 1 "),
             (good[:0], r"n >= 1"), (np.zeros((3, 5), np.float32), r"\(n,4\)"), (good[0], r"\(n,4\)"),
             (_boxes(9), "9 boxes exceed the row capacity 8 of a forward; raise num_proposals")]
    for boxes, msg in cases:
        for call in (lambda b: m.forward_boxes(img, b), lambda b: m.forward_boxes_images([img], [b]),
                     lambda b: m.extractFeatures_boxes([img], [b])):
            lib.raw.clear()
            with pytest.raises(ValueError, match=msg):
                call(boxes)
            assert not [c for c in lib.raw if c[0] in _ENTRIES]
    with pytest.raises(ValueError, match="image 1: box 0 "):
        m.forward_boxes_images([img, img], [good, bad(0, 2, -3.0)])
    assert len(m.forward_boxes(img, _boxes(8))[0]) == 8              # n = P is accepted


def _results_json(path, names, rng):
    res = []
    for name in names:
        n = int(rng.integers(1, 9))
        xywh = np.stack([rng.uniform(-50, 700, n), rng.uniform(-50, 500, n), rng.uniform(0.5, 400, n), rng.uniform(0.5, 400, n)], 1)
        xywh = xywh.astype(np.float32)
        res.append(dict(img_name=name, boxes=[[float(v) for v in r] for r in xywh], scores=[0.0] * n, captions=[""] * n))
    with open(path, "w") as f:
        json.dump(dict(results=res, opt={}), f)
    return res


def test_input_boxes_reader_round_trip(tmp_path):
    from densecap_amd import run_model
    rng = np.random.default_rng(0)
    names = ["a.jpg", "b.png", "c.jpg"]
    res = _results_json(tmp_path / "results.json", names, rng)
    got = run_model.read_input_boxes(str(tmp_path / "results.json"), names[::-1])
    assert list(got) == names[::-1]
    for r in res:
        want = np.asarray(r["boxes"], np.float32)
        b = got[r["img_name"]]
        assert b.dtype == np.float32 and b.shape == want.shape
        # xywh -> xcycwh -> xywh: a handful of rounded fp32 adds each way (6e-8 each), far inside 1e-5 of max(1, |coordinate|)
        back = run_model.xcycwh_to_xywh(b)
        assert (np.abs(back.astype(np.float64) - want) <= 1e-5 * np.maximum(1.0, np.abs(want))).all()
        np.testing.assert_array_equal(b[:, 2:], want[:, 2:])                       # w and h travel unchanged
    # xcycwh -> xywh -> xcycwh as well (the direction a results.json is made in)
    xc = np.stack([rng.uniform(1, 720, 200), rng.uniform(1, 600, 200), rng.uniform(0.5, 500, 200), rng.uniform(0.5, 500, 200)], 1)
    xc = xc.astype(np.float32)
    again = run_model.xywh_to_xcycwh(run_model.xcycwh_to_xywh(xc))
    assert (np.abs(again.astype(np.float64) - xc) <= 1e-5 * np.maximum(1.0, np.abs(xc))).all()


def test_input_boxes_reader_refuses_a_missing_image_by_name(tmp_path):
    from densecap_amd import extract_features, run_model
    rng = np.random.default_rng(1)
    res = _results_json(tmp_path / "results.json", ["a.jpg", "b.jpg"], rng)
    with pytest.raises(SystemExit, match="no entry for image c.jpg"):
        run_model.read_input_boxes(str(tmp_path / "results.json"), ["a.jpg", "c.jpg", "b.jpg"])
    res[1]["boxes"] = []
    json.dump(dict(results=res), open(tmp_path / "empty.json", "w"))
    with pytest.raises(SystemExit, match="lists no boxes for image b.jpg"):
        run_model.read_input_boxes(str(tmp_path / "empty.json"), ["b.jpg"])
    # a name listed twice in the file, or shared by two inputs, is refused (lists are looked up by file name)
    json.dump(dict(results=[res[0], res[0]]), open(tmp_path / "twice.json", "w"))
    with pytest.raises(SystemExit, match="lists image a.jpg more than once"):
        run_model.read_input_boxes(str(tmp_path / "twice.json"), ["a.jpg"])
    with pytest.raises(SystemExit, match="two input images are called a.jpg"):
        run_model.read_input_boxes(str(tmp_path / "results.json"), ["a.jpg", "a.jpg"])
    # both command lines know the flags, off by default
    for mod in (run_model, extract_features):
        opt = mod.build_parser().parse_args([])
        assert opt.input_boxes == "" and opt.clip_input_boxes == 0
        opt = mod.build_parser().parse_args(["-input_boxes", "x.json", "-clip_input_boxes", "1"])
        assert opt.input_boxes == "x.json" and opt.clip_input_boxes == 1


def test_header_cdef_and_binding_agree_on_the_box_list():
    """The struct is new: tests/test_abi_and_host.py compares the prototypes; the fields are compared here."""
    import os
    import re
    from densecap_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "densecap.h")).read(), flags=re.S)
    lua = open(os.path.join(root, "lua", "densecap_hip.lua")).read()

    def fields(text):
        body = re.search(r"typedef struct dc_box_list \{(.*?)\} dc_box_list;", text, flags=re.S).group(1)
        return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert fields(hdr) == fields(lua) == ["const float* boxes", "int32_t n", "int32_t* src"]
    assert [f[0] for f in _lib.DcBoxList._fields_] == ["boxes", "n", "src"]
    assert re.search(r"#define DC_BOXES_CLIP 1\b", hdr) and _lib.DC_BOXES_CLIP == 1
    assert "function Model:forward_boxes(input, boxes" in open(os.path.join(root, "lua", "DenseCapModelHIP.lua")).read()
