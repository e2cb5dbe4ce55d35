"""The kernels between the trunk and the language model in enqueue_forward, one launch each on crafted operands through the hooks
of include/densecap_debug_glue.h: boxes_ingest_kernel, bilinear_roi_pool_kernel in its group form, recog_heads_kernel,
iota_count_kernel, gather_rows_kernel / gather_rows_i32_kernel, survivor_compact_kernel, final_pack_kernel<false> / <true>.

Whole forwards reach them only with inputs that cannot tell right from wrong (every clip test is one compaction step of one wave,
every larger list keeps every row; RoI pooling alone runs as one image below the workgroup cap).  Here every output buffer holds a
sentinel before the launch and carries guard rows; the tests hold the values written bit for bit to tests/glue_rules.py and
everything a kernel must not write to the sentinel.  Only the heads' dot products have a tolerance: the bar of their summation order
(glue_rules.heads).  No model and no weights."""
import numpy as np
import pytest

from tests import glue_rules as G

pytestmark = pytest.mark.gpu

F32 = np.float32
DC_E_INVALID, DC_E_HIP = -1, -2


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


def _last_error(ctx):
    msg = ctx.lib.dc_last_error(ctx.h)
    return msg.decode() if msg else ""


def _count_patterns(nimg, P, seed):
    """Per-image counts: a mix, 0 in a middle image, every count P, counts above P (the first image's, so that every later
    offset depends on the clamp, and the last)."""
    rng = np.random.default_rng(seed)
    mix = rng.integers(0, P + 1, nimg)
    zero_mid = rng.integers(1, P + 1, nimg); zero_mid[nimg // 2] = 0
    above = rng.integers(0, P + 1, nimg); above[0] = P + 7; above[-1] = P + 1
    return {"mix": mix.tolist(), "zero_in_the_middle": zero_mid.tolist(), "all_P": [P] * nimg, "above_P": above.tolist()}


def _perms(nimg, P, rng):
    return np.concatenate([rng.permutation(P) for _ in range(nimg)]).astype(np.int32)


# ---- boxes_ingest_kernel ----------------------------------------------------------------------------------------------------------------
ING_P, ING_H, ING_W = 700, 320, 480
# every in_n of {0, 1, 63, 64, 65, 255, 256, 257, 600, 700, 900 (> P), -3} over calls of three images
ING_LISTS = [(600, 0, 257), (1, 63, 64), (65, 255, 256), (700, 900, -3)]
ING_LANE63_WAVE3_STEP1 = 256 + 3 * 64 + 63


def _ingest_invalid(pattern, P):
    """Which rows of a list the clip must drop."""
    i = np.arange(P)
    return {"none_invalid": i < 0,
            "all_invalid_count_0": i >= 0,
            "every_other_row": i % 2 == 1,
            "waves_0_and_2_of_step_0": (i < 64) | ((i >= 128) & (i < 192)),
            "all_but_lane_63_of_wave_3_of_step_1": i != ING_LANE63_WAVE3_STEP1,
            "step_0_invalid_step_1_valid": i < 256,
            "random_third": np.random.default_rng(33).uniform(size=P) < 1.0 / 3}[pattern]


def _ingest_boxes(invalid, seed):
    """(3 * P, 4): valid boxes inside, straddling and wholly outside the image (the reference's clip keeps those as slivers at the
    border); the rows of `invalid` are what it drops: 1 x 1 boxes and boxes half a pixel wide or high."""
    rng = np.random.default_rng(seed)
    n = 3 * ING_P
    b = np.stack([rng.uniform(-40, ING_W + 40, n), rng.uniform(-40, ING_H + 40, n), rng.uniform(3, 90, n), rng.uniform(3, 90, n)], 1)
    b[::17, 0] = ING_W + 300                                        # wholly outside
    bad = np.stack([rng.uniform(20, ING_W - 20, n), rng.uniform(20, ING_H - 20, n), np.ones(n), np.ones(n)], 1)
    bad[1::3, 2] = 0.5
    bad[2::3, 3] = 0.5
    inv = np.tile(invalid, 3)
    b[inv] = bad[inv]
    return b.astype(F32)


def _check_ingest(ctx, boxes, in_n, clip, stride, what):
    from densecap_amd import ops
    want = G.ingest(boxes, in_n, ING_P, clip, ING_H, ING_W)
    got = ops.glue_boxes_ingest(ctx, boxes, in_n, ING_P, clip, ING_H, ING_W, count_stride=stride)
    G.assert_counts(got["count"], [c for _, _, c in want], stride, what + " count")
    G.assert_rows(got["roi_boxes"], np.concatenate([r for r, _, _ in want]), what + " roi_boxes")
    G.assert_rows(got["box_src"], np.concatenate([s for _, s, _ in want]), what + " box_src")
    return [c for _, _, c in want]


@pytest.mark.parametrize("stride", [1, 64], ids=["count_stride_1", "count_stride_64"])
def test_ingest_without_the_clip(ctx, stride):
    """Clip off: rows [0, n) as given, n = max(0, min(in_n, P)) for in_n from 0 over the 64 and 256 seams to above P and below 0;
    zeros and -1 from n on; each image's block holds only its own rows."""
    boxes = _ingest_boxes(np.zeros(ING_P, bool), 1)
    for in_n in ING_LISTS:
        counts = _check_ingest(ctx, boxes, in_n, False, stride, "in_n %s" % (in_n,))
        assert counts == [max(0, min(n, ING_P)) for n in in_n]


@pytest.mark.parametrize("pattern", ["none_invalid", "all_invalid_count_0", "every_other_row", "waves_0_and_2_of_step_0",
                                     "all_but_lane_63_of_wave_3_of_step_1", "step_0_invalid_step_1_valid", "random_third"])
def test_ingest_clip_compaction_across_waves_and_steps_with_rows_dropped(ctx, pattern):
    """Clip on, with rows actually dropped: the cross-wave prefix (whole waves invalid), the cross-step carry of `kept` (a whole
    256-row step invalid, a single survivor in the last lane of the second step), in_n above P and below 0.  The invalid rows are
    invalid by the reference's own rule; bit for bit oracle clip + stable compaction."""
    from oracle import densecap_oracle as O
    invalid = _ingest_invalid(pattern, ING_P)
    boxes = _ingest_boxes(invalid, 2)
    _, valid = O.clip_boxes_xcycwh(boxes, 1, 1, ING_W, ING_H)
    np.testing.assert_array_equal(valid, ~np.tile(invalid, 3))         # the crafted rows, and only they, are what the reference drops
    for k, in_n in enumerate(ING_LISTS):
        counts = _check_ingest(ctx, boxes, in_n, True, (1, 64)[k % 2], "%s in_n %s" % (pattern, in_n))
        assert counts == [int((~invalid[:max(0, min(n, ING_P))]).sum()) for n in in_n]
    if pattern == "all_but_lane_63_of_wave_3_of_step_1":
        assert _check_ingest(ctx, boxes, (511, 512, 513), True, 64, pattern) == [0, 1, 1]


# ---- bilinear_roi_pool_kernel, group form -----------------------------------------------------------------------------------------------
ROI_H, ROI_W = 96, 128
#             C    h  w  HH  WW layout bdev_stride pick
ROI_VARIANTS = [(4, 3, 4, 2, 2, 0, None, False),
                (8, 5, 6, 7, 7, 1, 1, True),
                (512, 3, 4, 7, 7, 1, 64, False),
                (8, 5, 6, 16, 16, 0, 64, True),          # 16 x 16 = 256 points: exactly ROI_MAX_PTS
                (4, 5, 6, 16, 16, 1, None, True)]
#           nimg  B   path
ROI_GROUPS = [(1, 5, "single_image"), (3, 7, "interleaved_order"), (2, 40, "xcd_order"), (4, 9, "xcd_order"), (8, 3, "xcd_order"),
              (5, 11, "interleaved_order")]
ROI_CASES = [g + v for g in ROI_GROUPS for v in ROI_VARIANTS]
# 4800 and 4500 boxes at split = 1 are more than the 4096-workgroup cap: the grid-stride loop under either order
ROI_CASES += [(8, 600, "xcd_order_grid_stride", 4, 5, 6, 2, 2, 1, 64, True), (8, 600, "xcd_order_grid_stride", 4, 3, 4, 7, 7, 0, None, False),
              (3, 1500, "interleaved_order_grid_stride", 4, 5, 6, 2, 2, 1, 64, True),
              (3, 1500, "interleaved_order_grid_stride", 4, 3, 4, 7, 7, 0, 1, False)]


def _roi_id(c):
    nimg, B, path, C, h, w, HH, WW, layout, bs, pick = c
    return "%s-nimg%d-B%d-C%d-map%dx%d-grid%dx%d-layout%d-%s-%s" % (path, nimg, B, C, h, w, HH, WW, layout,
                                                                    "no_B_dev" if bs is None else "B_dev_stride_%d" % bs,
                                                                    "pick" if pick else "boxes")


def _roi_boxes(rng, n):
    """Boxes inside, straddling and wholly outside the map, so that the -1 taps occur."""
    b = np.stack([rng.uniform(-20, ROI_W + 20, n), rng.uniform(-20, ROI_H + 20, n), rng.uniform(4, 90, n), rng.uniform(4, 90, n)], 1)
    b[3::7] = [ROI_W + 400, -300, 10, 10]
    return b.astype(F32)


@pytest.mark.parametrize("case", ROI_CASES, ids=[_roi_id(c) for c in ROI_CASES])
def test_roi_pool_group(ctx, case):
    """Every image's block bit for bit what the single-image op gives on that image's map and live boxes (one thread computes an
    element in a fixed order: grouping, split and block order change no bit); the whole output against the oracle; dead rows zero;
    with a pick list -- repeats, unsorted, a source stride above the rows used -- the gathered boxes are written back, zeros past
    the count, without one `boxes` is left alone.  Per-image device counts 0, 1, B // 2, B, B + 5 at stride 1 or 64."""
    from densecap_amd import ops
    nimg, B, _, C, h, w, HH, WW, layout, bs, pick = case
    rng = np.random.default_rng(nimg * 1000 + B + C + HH)
    feats = rng.standard_normal((nimg, C, h, w)).astype(F32)
    opts = [0, 1, B // 2, B, B + 5]
    live = [opts[(i + C + HH) % 5] for i in range(nimg)] if bs is not None else None
    kw = dict(B_dev=live, bdev_stride=bs or 1)
    if pick:
        S = 13
        src = _roi_boxes(rng, nimg * S).reshape(nimg, S, 4)
        pk = rng.integers(0, S, nimg * B).astype(np.int32)
        got = ops.glue_roi_pool_group(ctx, feats, B, ROI_H, ROI_W, HH, WW, layout, pick=pk, src_boxes=src, **kw)
        want, wboxes = G.roi_pool_group(feats, B, ROI_H, ROI_W, HH, WW, layout, pick=pk, src_boxes=src, live=live)
        G.assert_rows(got["boxes"], wboxes, "boxes")
        boxes = wboxes
    else:
        boxes = _roi_boxes(rng, nimg * B)
        got = ops.glue_roi_pool_group(ctx, feats, B, ROI_H, ROI_W, HH, WW, layout, boxes=boxes, **kw)
        want, _ = G.roi_pool_group(feats, B, ROI_H, ROI_W, HH, WW, layout, boxes=boxes, live=live)
        G.assert_rows(got["boxes"], boxes, "boxes")                          # unmodified
    out = got["out"]
    G.assert_untouched(out[nimg * B:], "out's guard rows")
    out = out[:nimg * B]
    for i in range(nimg):
        n = G.live_count(live[i], B) if live is not None else B
        blk = out[i * B:(i + 1) * B]
        if n:
            one = ops.bilinear_roi_pool(ctx, feats[i], boxes[i * B:i * B + n], ROI_H, ROI_W, HH, WW, out_layout=layout)
            G.assert_bits_equal(blk[:n], one, "image %d against the single-image op" % i)
        G.assert_bits_equal(blk[n:], np.zeros_like(blk[n:]), "image %d dead rows" % i)
    np.testing.assert_allclose(out, want, atol=1e-6, rtol=0)
    if live is None or max(live) > 0:
        assert np.abs(want).sum() > 0
    if not pick and B >= 4:
        assert (np.abs(want).reshape(nimg * B, -1).sum(1) == 0).any()         # a box wholly outside the map: every tap is -1


# ---- recog_heads_kernel ---------------------------------------------------------------------------------------------------------------
def _heads_operands(n, D, seed):
    """Post-ReLU-like codes with many exact zeros, random-signed weights; crafted rows: the last row's fifth pre-activation is 95
    (exp overflows float32), with n >= 3 row 0's is -100 and row 1 holds one NaN code."""
    rng = np.random.default_rng(seed)
    codes = np.maximum(rng.standard_normal((n, D)) - 0.5, 0).astype(F32)
    w5 = (rng.standard_normal((5, D)) * 0.05).astype(F32)
    b5 = (rng.standard_normal(5) * 0.1).astype(F32)
    roi = np.stack([rng.uniform(0, 700, n), rng.uniform(0, 500, n), rng.uniform(5, 300, n), rng.uniform(5, 300, n)], 1).astype(F32)
    up, down = np.maximum(w5[4], 0).astype(np.float64), np.maximum(-w5[4], 0).astype(np.float64)
    codes[n - 1] = (up * (95.0 - b5[4]) / (up * up).sum()).astype(F32)
    if n >= 3:
        codes[0] = (down * (100.0 + b5[4]) / (down * down).sum()).astype(F32)
        codes[1, D // 3] = np.nan
    return codes, w5, b5, roi


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("D", [256, 512, 4096])
def test_recog_heads(ctx, D, n):
    """Five dot products a row against float64 within the bar of the kernel's summation order, D = 256 (one trip of the k loop)
    to 4096, n % 4 != 0 included; an overflowing exp, a pre-activation of -100 and a NaN code stay in their rows; fin and fin_xyxy
    bit for bit the device's own ApplyBoxTransform and corner conversion of the stored values; fin_xyxy present and null."""
    from densecap_amd import ops
    codes, w5, b5, roi = _heads_operands(n, D, 7 * D + n)
    ref = G.heads(codes, w5, b5, roi)
    assert 94.9 < ref["trans"][n - 1, 3] < 95.1
    if n >= 3:
        assert -100.1 < ref["trans"][0, 3] < -99.9 and np.isnan(ref["trans"][1]).all() and np.isnan(ref["obj"][1])
        assert np.isfinite(ref["trans"][[0] + list(range(2, n))]).all()
    for with_xyxy in (True, False):
        got = ops.glue_recog_heads(ctx, codes, w5, b5, roi, with_xyxy=with_xyxy)
        for k in ("obj", "trans", "fin") + (("fin_xyxy",) if with_xyxy else ()):
            G.assert_untouched(got[k][n:], k + "'s guard rows")
        worst = max(G.assert_within_bar(got["obj"][:n], ref["obj"], ref["bar_obj"], "obj"),
                    G.assert_within_bar(got["trans"][:n], ref["trans"], ref["bar_trans"], "trans"))
        print("HEADS_STAT D=%d n=%d: worst err / bar %.3f" % (D, n, worst))
        fin = got["fin"][:n]
        assert np.isinf(fin[n - 1, 3]) and fin[n - 1, 3] > 0 and np.isfinite(fin[n - 1, :3]).all()
        if n >= 3:
            assert np.isnan(fin[1]).all() and np.isfinite(fin[[0] + list(range(2, n - 1))]).all()
            assert 0 <= fin[0, 3] < 1e-38
        G.assert_bits_equal(fin, ops.apply_box_transform(ctx, roi, got["trans"][:n]), "fin")
        if with_xyxy:
            G.assert_bits_equal(got["fin_xyxy"][:n], ops.xcycwh_to_x1y1x2y2(ctx, fin), "fin_xyxy")
        else:
            assert "fin_xyxy" not in got


# ---- iota_count_kernel, gather_rows_kernel, gather_rows_i32_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 255, 256, 257, 1000])
def test_iota_count_and_gather_rows(ctx, cap):
    """idx = 0 .. cap - 1 and the count copied; float and int32 rows gathered by an unsorted index with repeats, width 1, 3, 4, 512,
    count 0, 1, cap: rows from the count on are zero, nothing past cap is written."""
    from densecap_amd import ops
    rng = np.random.default_rng(cap)
    for count in (0, 1, cap):
        got = ops.glue_iota_count(ctx, cap, count)
        idx, cnt = G.iota_count(cap, count)
        G.assert_rows(got["idx"], idx, "idx")
        G.assert_rows(got["count_out"], np.array([cnt], np.int32), "count_out")
    src_rows = 37
    idx = rng.integers(0, src_rows, cap).astype(np.int32)
    for width in (1, 3, 4, 512):
        srcs = (rng.standard_normal((src_rows, width)).astype(F32), rng.integers(-2 ** 31, 2 ** 31 - 1, (src_rows, width)).astype(np.int32))
        for src in srcs:
            for count in (0, 1, cap):
                got = ops.glue_gather_rows(ctx, src, idx, count, cap)
                G.assert_rows(got["out"], G.gather_rows(src, idx, count, cap), "%s width %d count %d" % (src.dtype, width, count))


# ---- survivor_compact_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nimg,P,D", [(1, 1, 4), (3, 50, 64), (5, 64, 256), (4, 300, 512)])
def test_survivor_compact(ctx, nimg, P, D):
    """The packed row block in pick order at offsets of min(count, P) over the earlier images, *total, and rows [total, nimg * P)
    left alone; counts of 0 in a middle image, P and above P; (4, 300, 512) with every count P is 38400 items on 19200
    threads: the grid-stride loop."""
    from densecap_amd import ops
    rng = np.random.default_rng(P + D)
    codes = rng.standard_normal((nimg * P, D)).astype(F32)
    picks = _perms(nimg, P, rng)
    for k, (name, count) in enumerate(_count_patterns(nimg, P, P).items()):
        for stride in (1, 64):
            rows, total = G.survivor_compact(codes, picks, count, P)
            got = ops.glue_survivor_compact(ctx, codes, picks, count, P, count_stride=stride)
            G.assert_rows(got["total"], np.array([total], np.int32), "%s total" % name)
            G.assert_packed(got["out"], rows, total, got["total"][0], "%s stride %d" % (name, stride))


# ---- final_pack_kernel ------------------------------------------------------------------------------------------------------------------
def _pack_operands(nimg, P, rng):
    fb = rng.standard_normal((nimg * P, 4)).astype(F32)
    obj = rng.standard_normal(nimg * P).astype(F32)
    box_src = rng.integers(0, 5000, nimg * P).astype(np.int32)
    return fb, obj, _perms(nimg, P, rng), box_src


def _check_pack(ctx, fb, obj, picks, count, P, words, what, **kw):
    from densecap_amd import ops
    with_src = kw.get("box_src") is not None
    recs = G.final_pack(fb, obj, picks, count, P, fault=kw.get("fault") or 0, **{k: v for k, v in kw.items() if k not in ("fault", "count_stride")})
    got = ops.glue_final_pack(ctx, fb, obj, picks, count, P, **kw)
    nimg = len(count)
    stride = (len(got["pack"]) - 256) // nimg
    assert stride >= G.record_bytes(P, words, with_src) + 256
    for i, rec in enumerate(recs):
        G.assert_record(got["pack"][i * stride:(i + 1) * stride], rec, P, words, with_src, "%s image %d" % (what, i))
    G.assert_untouched(got["pack"][nimg * stride:], what + " after the last record")
    return recs


@pytest.mark.parametrize("tok_gather", [0, 1, 2], ids=["tok_gather_0_final_order", "tok_gather_1_by_pick", "tok_gather_2_packed_over_the_group"])
@pytest.mark.parametrize("nimg", [1, 3, 5])
def test_final_pack_tokens(ctx, nimg, tok_gather):
    """Token records, the three token orders, with and without box_src (final_pack_kernel<true> / <false>) and the fault word; the
    raw bytes: K, the fault word, every row below K of every section, and every other byte of the stride still the sentinel.  For
    tok_gather 2 the token block is packed with survivor_compact's offsets: a wrong offset for a later image reads another image's
    rows.  Counts 0 in a middle image, P, above P."""
    P, T = 40, 15
    rng = np.random.default_rng(10 * nimg + tok_gather)
    fb, obj, picks, box_src = _pack_operands(nimg, P, rng)
    rows = (np.arange(nimg * P * T, dtype=np.int32) + 1).reshape(nimg * P, T)         # every row of the block is another row
    for k, (name, count) in enumerate(_count_patterns(nimg, P, nimg).items()):
        tokens = rows
        if tok_gather == 2:
            K, off, total = G.group_offsets(count, P)
            tokens = -rows                                                        # what lies past the packed rows is never read
            for i in range(nimg):
                tokens[off[i]:off[i] + K[i]] = rows[i * P:i * P + K[i]] + 1000000
        _check_pack(ctx, fb, obj, picks, count, P, T, "%s" % name, tokens=tokens, tok_gather=tok_gather,
                    box_src=box_src if k % 2 == 0 else None, fault=0xdeadbeef if k % 2 == 0 else None, count_stride=(1, 64)[k % 2])
        _check_pack(ctx, fb, obj, picks, count, P, T, "%s" % name, tokens=tokens, tok_gather=tok_gather,
                    box_src=box_src if k % 2 == 1 else None, fault=0xdeadbeef if k % 2 == 1 else None, count_stride=(64, 1)[k % 2])


@pytest.mark.parametrize("nimg,P,D", [(1, 40, 8), (3, 40, 8), (5, 40, 8), (3, 600, 1024)],
                         ids=["nimg1-D8", "nimg3-D8", "nimg5-D8", "nimg3-P600-D1024-grid_stride"])
def test_final_pack_codes(ctx, nimg, P, D):
    """fc7 codes in the place of tokens (features-only forwards), with box_src (kSrc, the osrc loop on real picks with K = P) and
    without.  P = 600, D = 1024 is 2412 blocks of items against the cap of 2048: the grid-stride loop."""
    rng = np.random.default_rng(P + D + nimg)
    fb, obj, picks, box_src = _pack_operands(nimg, P, rng)
    codes = rng.standard_normal((nimg * P, D)).astype(F32)
    pats = _count_patterns(nimg, P, D)
    if P == 600:
        pats = {"all_P": pats["all_P"], "above_P": pats["above_P"]}
    for k, (name, count) in enumerate(pats.items()):
        with_src = (k % 2 == 0) or name == "all_P"
        recs = _check_pack(ctx, fb, obj, picks, count, P, D, "%s" % name, codes=codes, box_src=box_src if with_src else None,
                           fault=None if k % 2 == 0 else 0xdeadbeef, count_stride=(64, 1)[k % 2])
        if name == "all_P":
            assert all(r["K"] == P for r in recs)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_would_leave_the_buffers(ctx):
    """Out-of-range picks and indices, bad shapes and a short stride: the error code and a message that names the hook, every
    output still the sentinel, nothing launched; what the launchers themselves refuse (C % 4, 272 points, a pick list without
    source boxes, D = 260, D % 4) comes back as an error too.  The context is usable afterwards."""
    from densecap_amd import ops
    rng = np.random.default_rng(0)

    def refused(res, hook, code=DC_E_INVALID):
        assert res.pop("rc") == code, (hook, _last_error(ctx))
        assert hook in _last_error(ctx) or code == DC_E_HIP, _last_error(ctx)
        for k, v in res.items():
            if k != "boxes":
                G.assert_untouched(v, "%s %s" % (hook, k))
        return res

    boxes = _roi_boxes(rng, 12)
    # ingest
    refused(ops.glue_boxes_ingest(ctx, boxes, [3, 3], 0, 0, 20, 30, raise_errors=False), "dc_debug_boxes_ingest")
    refused(ops.glue_boxes_ingest(ctx, boxes, [3, 3], 6, 0, 20, 30, count_stride=0, raise_errors=False), "dc_debug_boxes_ingest")
    # RoI pooling: the launcher's refusals, then the hook's
    feats = rng.standard_normal((2, 8, 3, 4)).astype(F32)
    src = boxes.reshape(2, 6, 4)
    pk = np.array([0, 5, 1, 1, 2, 4], np.int32)
    roi = lambda f=feats, HH=7, WW=7, **kw: ops.glue_roi_pool_group(ctx, f, 3, ROI_H, ROI_W, HH, WW, 1, raise_errors=False, **kw)
    refused(roi(f=rng.standard_normal((2, 6, 3, 4)).astype(F32), boxes=boxes[:6]), "dc_debug_roi_pool_group", DC_E_HIP)     # C % 4
    refused(roi(HH=16, WW=17, boxes=boxes[:6]), "dc_debug_roi_pool_group", DC_E_HIP)                                     # 272 points
    res = refused(roi(pick=pk), "dc_debug_roi_pool_group", DC_E_HIP)                                                     # no src_boxes
    G.assert_untouched(res["boxes"], "boxes")
    for bad in (6, -1):
        p = pk.copy(); p[4] = bad
        res = refused(roi(pick=p, src_boxes=src), "dc_debug_roi_pool_group")
        G.assert_untouched(res["boxes"], "boxes")
        assert "pick[1][1] = %d" % bad in _last_error(ctx)
        p = pk.copy(); p[5] = bad                                             # the same pick in a dead row is never read
        ok = roi(pick=p, src_boxes=src, B_dev=[3, 2])
        assert ok["rc"] == 0 and not ok["boxes"][5].any()
    refused(roi(HH=1, boxes=boxes[:6]), "dc_debug_roi_pool_group")
    refused(roi(boxes=boxes[:6], B_dev=[1, 1], bdev_stride=0), "dc_debug_roi_pool_group")
    # heads
    codes, w5, b5, rb = _heads_operands(3, 260, 1)
    refused(ops.glue_recog_heads(ctx, codes, w5, b5, rb, raise_errors=False), "dc_debug_recog_heads", DC_E_HIP)
    # iota, gathers
    refused(ops.glue_iota_count(ctx, 0, 0, raise_errors=False), "dc_debug_iota_count")
    for src_rows in (rng.standard_normal((5, 3)).astype(F32), rng.integers(0, 9, (5, 3)).astype(np.int32)):
        for bad in (5, -1):
            refused(ops.glue_gather_rows(ctx, src_rows, [0, 4, bad, 1], 3, 4, raise_errors=False), "dc_debug_gather_rows")
            assert ops.glue_gather_rows(ctx, src_rows, [0, 4, bad, 1], 2, 4)["rc"] == 0          # past the count: never read
    # compaction
    P = 6
    codes = rng.standard_normal((3 * P, 8)).astype(F32)
    picks = _perms(3, P, rng)
    for bad in (P, -1):
        p = picks.copy(); p[2 * P + 1] = bad
        refused(ops.glue_survivor_compact(ctx, codes, p, [P, 0, 2], P, raise_errors=False), "dc_debug_survivor_compact")
        assert "picks[2][1] = %d" % bad in _last_error(ctx)
        assert ops.glue_survivor_compact(ctx, codes, p, [P, 0, 1], P)["rc"] == 0
    # min(count, P) goes into the later images' offsets unclamped from below: a negative count would move them before the block
    refused(ops.glue_survivor_compact(ctx, codes, picks, [-3, P, 2], P, raise_errors=False), "dc_debug_survivor_compact")
    assert "count[0] = -3" in _last_error(ctx)
    refused(ops.glue_survivor_compact(ctx, codes[:, :6], picks, [P, 0, 2], P, raise_errors=False), "dc_debug_survivor_compact", DC_E_HIP)
    refused(ops.glue_survivor_compact(ctx, codes, picks, [P, 0, 2], P, count_stride=0, raise_errors=False), "dc_debug_survivor_compact")
    # records
    fb, obj, picks, box_src = _pack_operands(3, P, rng)
    tokens = rng.integers(1, 99, (3 * P, 4)).astype(np.int32)
    pack = lambda **kw: ops.glue_final_pack(ctx, fb, obj, kw.pop("picks", picks), kw.pop("count", [P, 0, 2]), P, raise_errors=False, **kw)
    refused(pack(tokens=tokens, tok_gather=2, count=[P, -1, 2]), "dc_debug_final_pack")
    for bad in (P, -1):
        p = picks.copy(); p[2 * P + 1] = bad
        refused(pack(picks=p, tokens=tokens), "dc_debug_final_pack")
    need = G.record_bytes(P, 4, True)
    refused(pack(tokens=tokens, box_src=box_src, stride=need - 4), "dc_debug_final_pack")                 # short by the last src word
    refused(pack(tokens=tokens, stride=G.record_bytes(P, 4, False) + 2), "dc_debug_final_pack")           # no multiple of 4
    refused(pack(tokens=tokens, tok_gather=3), "dc_debug_final_pack")
    refused(pack(), "dc_debug_final_pack")                                                                  # neither tokens nor codes
    refused(pack(tokens=tokens, codes=codes[:, :4]), "dc_debug_final_pack")                               # both
    assert pack(tokens=tokens, box_src=box_src, stride=need)["rc"] == 0                                   # the record exactly
    # the context after all that: one valid call of each family's neighbour
    got = ops.glue_iota_count(ctx, 300, 17)
    G.assert_rows(got["idx"], np.arange(300, dtype=np.int32), "idx")
    assert got["count_out"][0] == 17
