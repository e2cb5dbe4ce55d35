"""dc_op_roi_pool_grad and the tap index behind it (densecap_amd/csrc/recog_grad.hip) against the float64 autograd restatement
of tests/recog_grad_rules.py and the oracle's sampling positions (docs/SEMANTICS.md, "Recognition-net gradients").

Largest observed max|dev - ref64| / max|ref64| per case (MI355X; the bar is 1e-4), and the worst per-pixel ratio beside the bar it
was held to (tests/grad_bars.py): see DESIGN.md §17."""
import numpy as np
import pytest

from tests import grad_bars as GB
from tests import recog_grad_rules as R

pytestmark = pytest.mark.gpu

REL = 1e-4                     # tests/parity.py's continuous-stage bar
F32 = np.float32
FAR = np.array([[-3000.0, -2000.0, 50.0, 40.0]], F32)      # a box wholly outside the map


def _boxes(seed, B, img, hw, pool=(7, 7), **kw):
    return R.draw_boxes(np.random.default_rng(seed), B, img[0], img[1], hw[0], hw[1], pool[0], pool[1], **kw)


# name -> (image (H, W), map (h, w), C, (HH, WW), boxes, compare dboxes)
def _cases():
    c = {}
    img = (96, 128)
    c["one_box"] = (img, (6, 8), 4, (7, 7), _boxes(1, 1, img, (6, 8)), True)
    c["three_identical"] = (img, (6, 8), 8, (7, 7), np.repeat(_boxes(2, 1, img, (6, 8)), 3, 0), True)
    c["outside"] = (img, (6, 8), 4, (7, 7), FAR, True)
    c["half_outside"] = (img, (6, 8), 4, (7, 7), _boxes(3, 5, img, (6, 8), outside=1.0), True)
    # sampling coordinates that are exact integers: image and map 5 x 9, box (5, 3, 4.5, 2.5), 3 x 3 points -> x in {2, 4, 6}, y in {1, 2, 3}
    c["integer_coords"] = ((5, 9), (5, 9), 4, (3, 3), np.array([[5.0, 3.0, 4.5, 2.5]], F32), False)
    c["tiny_map_64_rows"] = (img, (2, 2), 4, (7, 7), _boxes(4, 64, img, (2, 2), lo=0.3, hi=0.9), True)       # lists of many chunks
    # 136 scattered rows, 120 copies of one box (many rows over one pixel, the normal case for positives around one ground-truth
    # box) and the far box
    big = _boxes(5, 137, (600, 720), (38, 45), outside=0.1)
    c["map_38x45_257_rows"] = ((600, 720), (38, 45), 512, (7, 7), np.concatenate([big[:136], np.repeat(big[136:], 120, 0), FAR]), True)
    c["pool_2x3"] = (img, (6, 8), 8, (2, 3), _boxes(6, 9, img, (6, 8), (2, 3), outside=0.3), True)
    c["rows_1024"] = (img, (3, 3), 4, (7, 7), _boxes(7, 1024, img, (3, 3), lo=0.3, hi=0.9), True)            # lists past the LDS sort
    return c


CASES = _cases()
# The index at its limits.  roi_index_scan_kernel is ONE workgroup of 1024 threads, each owning ceil(npix / 1024) pixels:
# 1,023 px leaves a thread idle, 1,024 fills them, 1,025 and 2,049 are the first sizes with 2 and 3 pixels per thread, 65,536 the
# documented limit (64 per thread).  roi_sort_lists_kernel runs on min(npix, 65535) workgroups in a grid-stride loop: only the
# 65,536-pixel map gives it a second trip, for pixel 65,535.  C = 4, 7 x 7 points, six boxes (a share across the border), the image
# 16 times the map; the two largest maps also get one small box inside the bottom-right pixel quad and one inside the top-left, so
# that pixel h * w - 1 (the second trip) and pixel 0 have lists to sort.  Built on first use: drawing boxes away from integer
# coordinates takes seconds on the three-row maps.
LIMIT_MAPS = {"map_3x341": (3, 341), "map_32x32": (32, 32), "map_25x41": (25, 41), "map_3x683": (3, 683), "map_255x257": (255, 257),
              "map_256x256": (256, 256)}
CORNERED = ("map_255x257", "map_256x256")
POOL_LIMIT = "pool_16x16"          # HH * WW = 256 points: every thread of roi_taps_kernel has one
ALL = list(CASES) + list(LIMIT_MAPS) + [POOL_LIMIT]
_limit, _runs = {}, {}


def _corner_box(rng, img, hw, mx, my):
    """A box 6 image px (3/8 of a map px) wide whose 49 points all lie around map position (mx, my), strictly between two pixel
    columns and two pixel rows; redrawn until no sampling coordinate is within R.EDGE of an integer."""
    (H, Wd), (h, w) = img, hw
    while True:
        cx, cy = mx + rng.uniform(-0.05, 0.05), my + rng.uniform(-0.05, 0.05)
        xc = ((2 * cx / (w - 1) - 1) * (Wd - 1) + 1 + Wd) / 2                  # the centre's map coordinate is (th + 1) (w - 1) / 2
        yc = ((2 * cy / (h - 1) - 1) * (H - 1) + 1 + H) / 2
        b = np.array([[xc, yc, 6.0, 6.0]], F32)
        if R.edge_distance(b, H, Wd, h, w, 7, 7)[0] > R.EDGE:
            return b


def _case(name):
    if name in CASES:
        return CASES[name]
    if name not in _limit:
        if name == POOL_LIMIT:
            _limit[name] = ((96, 128), (6, 8), 4, (16, 16), _boxes(8, 3, (96, 128), (6, 8), (16, 16), outside=0.3), True)
        else:
            h, w = LIMIT_MAPS[name]
            img = (16 * h, 16 * w)
            boxes = _boxes(20 + list(LIMIT_MAPS).index(name), 6, img, (h, w), outside=0.3)
            if name in CORNERED:
                rng = np.random.default_rng(h)
                boxes = np.concatenate([boxes, _corner_box(rng, img, (h, w), w - 1.5, h - 1.5), _corner_box(rng, img, (h, w), 0.5, 0.5)])
            _limit[name] = (img, (h, w), 4, (7, 7), boxes, True)
    return _limit[name]


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd.ops import Context
    c = Context(0)
    yield c
    _runs.clear(); _limit.clear()
    c.close()


def _run(ctx, name):
    """(feat, dout, device (dfeat, dboxes), reference (dfeat, dboxes)) of a case, computed once."""
    if name not in _runs:
        from densecap_amd import ops
        img, (h, w), C, (HH, WW), boxes, _ = _case(name)
        rng = np.random.default_rng(len(name) * 7 + C)
        feat = rng.standard_normal((C, h, w)).astype(F32)
        dout = rng.standard_normal((len(boxes), C, HH, WW)).astype(F32)
        dev = ops.roi_pool_grad(ctx, feat, boxes, img[0], img[1], dout, HH, WW)
        _runs[name] = (feat, dout, dev, R.roi_pool_grad(feat, boxes, img[0], img[1], dout, HH, WW))
    return _runs[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _expected_index(name):
    """(tap_pix, tap_w, start, list) from the oracle's positions: float32 numpy, operation for operation."""
    img, (h, w), C, (HH, WW), boxes, _ = _case(name)
    yc, xc = R.coords32(boxes, img[0], img[1], h, w, HH, WW)
    x0, y0 = np.floor(xc), np.floor(yc)
    wx, wy = F32(1) - (xc - x0), F32(1) - (yc - y0)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    wts = np.stack([wx * wy, (F32(1) - wx) * wy, wx * (F32(1) - wy), (F32(1) - wx) * (F32(1) - wy)], -1).astype(F32)
    pix = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + dy, x0 + dx
        ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
        pix.append(np.where(ok, yy * w + xx, -1))
    pix = np.stack(pix, -1).reshape(-1)
    valid = np.flatnonzero(pix >= 0)
    lst = valid[np.argsort(pix[valid], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(pix[valid], minlength=h * w))])
    return pix.astype(np.int32), wts.reshape(-1), start.astype(np.int32), lst.astype(np.int32)


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_the_float64_restatement(ctx, name):
    feat, dout, (dfeat, dboxes), (rfeat, rboxes) = _run(ctx, name)
    pairs = [("dfeat", dfeat, rfeat)] + ([("dboxes", dboxes, rboxes)] if _case(name)[5] else [])
    for what, dev, ref in pairs:
        scale = np.abs(ref).max()
        err = np.abs(dev - ref).max()
        print("roi_pool_grad %s %s: max|ref| %.3e ratio %.2e" % (name, what, scale, err / scale if scale else 0.0))
        assert dev.shape == ref.shape and dev.dtype == F32
        assert err <= REL * scale, (name, what, err, scale)


@pytest.mark.parametrize("name", ALL)
def test_every_pixel_matches_the_float64_restatement_at_the_float32_evaluations_bar(ctx, name):
    """dfeat pixel by pixel over its channels (tests/grad_bars.py): within 8 x the float32 evaluation's worst per-pixel ratio of
    the pixel's OWN largest entry -- a border pixel with one tap is not measured against a pixel under 120 boxes -- and untouched
    pixels all +0.0 bits."""
    import torch
    img, (h, w), C, (HH, WW), boxes, _ = _case(name)
    feat, dout, (dfeat, dboxes), (rfeat, rboxes) = _run(ctx, name)
    f32 = R.roi_pool_grad(feat, boxes, img[0], img[1], dout, HH, WW, dtype=torch.float32)[0]
    GB.assert_rows("roi_pool_grad " + name, ("dfeat",), {"dfeat": dfeat}, {"dfeat": rfeat}, {"dfeat": f32})


@pytest.mark.parametrize("name", ALL)
def test_tap_list_and_pixel_lists_are_the_oracles_positions_bit_for_bit(ctx, name):
    from densecap_amd import ops
    img, (h, w), C, (HH, WW), boxes, _ = _case(name)
    pix, wts, start, lst = ops.roi_tap_index(ctx, boxes, h, w, img[0], img[1], HH, WW)
    epix, ewts, estart, elst = _expected_index(name)
    assert np.array_equal(pix, epix)
    assert np.array_equal(_bits(wts), _bits(ewts))
    assert np.array_equal(start, estart)
    assert np.array_equal(lst, elst)


@pytest.mark.parametrize("name", ALL)
def test_two_calls_give_identical_bits_and_untouched_pixels_are_plus_zero(ctx, name):
    from densecap_amd import ops
    img, (h, w), C, (HH, WW), boxes, _ = _case(name)
    feat, dout, (dfeat, dboxes), _ = _run(ctx, name)
    again = ops.roi_pool_grad(ctx, feat, boxes, img[0], img[1], dout, HH, WW)
    assert np.array_equal(_bits(again[0]), _bits(dfeat)) and np.array_equal(_bits(again[1]), _bits(dboxes))
    only_feat = ops.roi_pool_grad(ctx, feat, boxes, img[0], img[1], dout, HH, WW, want_boxes=False)
    assert only_feat[1] is None and np.array_equal(_bits(only_feat[0]), _bits(dfeat))
    pix = _expected_index(name)[0]
    untouched = np.bincount(pix[pix >= 0], minlength=h * w).reshape(h, w) == 0
    assert not _bits(dfeat[:, untouched]).any()


def test_a_box_outside_the_map_gives_nothing(ctx):
    feat, dout, (dfeat, dboxes), _ = _run(ctx, "outside")
    assert not _bits(dfeat).any() and not dboxes.any()
    assert not _run(ctx, "map_38x45_257_rows")[2][1][-1].any()                     # the far row of the large case


def test_long_lists_take_the_chunked_and_the_in_place_paths(ctx):
    """The cases meant to reach them do: lists above one chunk of 128 entries, and above the 4096 entries sorted in LDS."""
    assert np.diff(_expected_index("tiny_map_64_rows")[2]).max() > 128
    assert np.diff(_expected_index("rows_1024")[2]).max() > 4096
    assert np.diff(_expected_index("map_38x45_257_rows")[2]).max() > 128


def test_the_limit_cases_reach_what_they_are_meant_to():
    """Pixel h * w - 1 and pixel 0 of the two largest maps have lists of at least two taps (on 256 x 256 the former is the one
    pixel of the sort's second grid-stride trip); the pool-limit case has exactly 256 points."""
    for name in CORNERED:
        h, w = LIMIT_MAPS[name]
        start = _expected_index(name)[2]
        assert start[h * w] - start[h * w - 1] >= 2 and start[1] - start[0] >= 2, name
    assert LIMIT_MAPS["map_256x256"][0] * LIMIT_MAPS["map_256x256"][1] == 65536 > 65535
    assert _case(POOL_LIMIT)[3][0] * _case(POOL_LIMIT)[3][1] == 256
    for name in list(LIMIT_MAPS) + [POOL_LIMIT]:
        img, (h, w), C, (HH, WW), boxes, _ = _case(name)
        assert (R.edge_distance(boxes, img[0], img[1], h, w, HH, WW) > R.EDGE).all(), name


def test_a_map_past_65536_pixels_is_refused_and_nothing_is_written(ctx):
    """1 x 65,537: DC_E_UNSUPPORTED with a message naming 65536, and the output buffers keep their sentinel.  (The index's other
    limit, B * HH * WW * 4 <= 2^30 taps, needs a million rows of inputs and is left out.)"""
    h, w, C = 1, 65537, 4
    fd, bd = ctx.to_device(np.zeros((h, w, C), F32)), ctx.to_device(np.array([[500.0, 8.0, 300.0, 6.0]], F32))
    dd = ctx.to_device(np.zeros((1, 7, 7, C), F32))
    sent, sentb = np.full((h, w, C), -7.25, F32), np.full((1, 4), -7.25, F32)
    od, ob = ctx.to_device(sent), ctx.to_device(sentb)
    rc = ctx.lib.dc_op_roi_pool_grad(ctx.h, fd.ptr, h, w, C, bd.ptr, 1, 16, 16 * w, 7, 7, dd.ptr, od.ptr, ob.ptr)
    assert rc == -5                                                               # DC_E_UNSUPPORTED
    assert "65536" in ctx.lib.dc_last_error(ctx.h).decode()
    assert np.array_equal(_bits(od.numpy()), _bits(sent)) and np.array_equal(_bits(ob.numpy()), _bits(sentb))


def test_refusals(ctx):
    from densecap_amd import ops
    from densecap_amd._lib import DenseCapError
    feat, box = np.zeros((4, 6, 8), F32), np.array([[60.0, 40.0, 50.0, 30.0]], F32)
    with pytest.raises(DenseCapError, match="-1|bad shape"):
        ops.roi_pool_grad(ctx, np.zeros((3, 6, 8), F32), box, 96, 128, np.zeros((1, 3, 7, 7), F32))       # C % 4
    with pytest.raises(DenseCapError, match="256"):
        ops.roi_pool_grad(ctx, feat, box, 96, 128, np.zeros((1, 4, 17, 16), F32), 17, 16)                 # 272 points
    with pytest.raises(DenseCapError):
        ops.roi_pool_grad(ctx, feat, box, 96, 128, np.zeros((1, 4, 1, 7), F32), 1, 7)                     # HH < 2
