"""tests/glue_rules.py checked on the CPU: every rule on a hand-written case with the expected values typed in, then negative
controls for every comparison helper tests/test_gpu_glue_kernels.py uses -- one perturbation of a correct output at a time (two
rows swapped, a count off by one, a guard word changed, a row of image 2 at image 1's offset, one element off by two units in the
last place), and the helper must raise.  Last, the hook header is where the binding expects it and off the drop-in boundary."""
import os
import re

import numpy as np
import pytest

from tests import glue_rules as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the rules on hand-written cases -------------------------------------------------------------------------------------------------
BOXES = np.array([[10, 10, 5, 5], [10, 10, 1, 1], [100, 10, 5, 5], [15, 5, 0.5, 3],       # image 0
                  [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16],          # image 1
                  [2, 2, 2, 2], [3, 3, 3, 3], [4, 4, 4, 4], [5, 5, 5, 5]], F32)           # image 2


def test_ingest_without_the_clip_keeps_the_first_n_rows():
    (r0, s0, c0), (r1, s1, c1), (r2, s2, c2) = G.ingest(BOXES, [3, 9, -2], 4, False, 20, 30)
    assert (c0, c1, c2) == (3, 4, 0)                                  # n, n above P, n below 0
    np.testing.assert_array_equal(r0, [[10, 10, 5, 5], [10, 10, 1, 1], [100, 10, 5, 5], [0, 0, 0, 0]])
    np.testing.assert_array_equal(s0, [0, 1, 2, -1])
    np.testing.assert_array_equal(r1, BOXES[4:8])
    np.testing.assert_array_equal(s1, [0, 1, 2, 3])
    assert not r2.any() and (s2 == -1).all()
    assert r0.dtype == F32 and s0.dtype == np.int32


def test_ingest_with_the_clip_drops_what_the_reference_drops():
    """On a 30 x 20 image: a box inside loses a pixel of width and height (the two conversions are not inverses), the 1 x 1 box and
    the half-pixel-wide box are invalid, the box wholly to the right stays as a sliver one pixel wide at the border."""
    (r0, s0, c0), = G.ingest(BOXES[:4], [4], 4, True, 20, 30)
    assert c0 == 2
    np.testing.assert_array_equal(r0, [[10, 10, 4, 4], [29.5, 10, 1, 4], [0, 0, 0, 0], [0, 0, 0, 0]])
    np.testing.assert_array_equal(s0, [0, 2, -1, -1])


def _ramp_maps(nimg):
    """(nimg, 4, 2, 2): channel c of image i is (c + 1) * [[1, 2], [3, 4]] + 100 i."""
    base = np.array([[1, 2], [3, 4]], F32)
    return np.stack([np.stack([(c + 1) * base + 100 * i for c in range(4)]) for i in range(nimg)])


def test_roi_pool_group_samples_each_image_on_its_own_map():
    """A box that is the whole image puts the 2 x 2 grid on the four corners of a 2 x 2 map: the output is the map."""
    H, W = 9, 11
    whole = [(W + 1) / 2, (H + 1) / 2, W, H]
    feats = _ramp_maps(2)
    boxes = np.array([whole, whole, whole, whole], F32)
    out, bx = G.roi_pool_group(feats, 2, H, W, 2, 2, 0, boxes=boxes, live=[2, 1])
    assert bx is None and out.shape == (4, 4, 2, 2)
    np.testing.assert_allclose(out[0], feats[0], atol=1e-5)
    np.testing.assert_allclose(out[1], feats[0], atol=1e-5)
    np.testing.assert_allclose(out[2], feats[1], atol=1e-5)              # image 1 reads image 1's map
    assert not out[3].any()                                                # its second row is dead
    # a pick list gathers the boxes, repeats allowed, and hands them back; layout 1 is channels last
    src = np.array([[[0, 0, 1, 1], whole, [1, 1, 1, 1]], [whole, [2, 2, 2, 2], [3, 3, 3, 3]]], F32)
    out1, bx = G.roi_pool_group(feats, 2, H, W, 2, 2, 1, pick=[1, 1, 0, 2], src_boxes=src, live=[5, 1])
    np.testing.assert_array_equal(bx, [whole, whole, whole, [0, 0, 0, 0]])
    assert out1.shape == (4, 2, 2, 4)
    np.testing.assert_array_equal(out1, out.transpose(0, 2, 3, 1))


def test_roi_pool_group_outside_taps_read_zero():
    H, W = 9, 11
    far = np.array([[500, 500, 4, 4]], F32)
    out, _ = G.roi_pool_group(_ramp_maps(1), 1, H, W, 2, 2, 0, boxes=far)
    assert not out.any()


def test_heads_values_and_bar():
    codes = np.array([[1, 2, 0, 0], [0, 0, 0, 3]], F32)
    w5 = np.array([[1, 1, 1, 1], [0.5, -0.5, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [-1, 0, 0, 2]], F32)
    b5 = np.array([0.25, 0, -1, 0, 0.5], F32)
    roi = np.array([[10, 20, 4, 8], [1, 2, 3, 4]], F32)
    r = G.heads(codes, w5, b5, roi)
    np.testing.assert_array_equal(r["obj"], [3.25, 3.25])
    np.testing.assert_array_equal(r["trans"], [[-0.5, -1, 0, -0.5], [0, 2, 0, 6.5]])
    assert G.heads_terms(4) == 12 and G.heads_terms(256) == 12 and G.heads_terms(512) == 16 and G.heads_terms(4096) == 72
    np.testing.assert_allclose(r["bar_obj"], np.array([3.25, 3.25]) * 12 * 2.0 ** -24, rtol=1e-15)
    np.testing.assert_allclose(r["bar_trans"], np.array([[1.5, 1, 0, 1.5], [0, 4, 0, 6.5]]) * 12 * 2.0 ** -24, rtol=1e-15)
    np.testing.assert_allclose(r["fin"], [[8, 12, 4, 8 * np.exp(-0.5)], [1, 10, 3, 4 * np.exp(6.5)]], rtol=1e-15)


def test_iota_gather_and_compact():
    idx, cnt = G.iota_count(5, 3)
    np.testing.assert_array_equal(idx, [0, 1, 2, 3, 4])
    assert cnt == 3 and idx.dtype == np.int32
    src = np.array([[1, 2], [3, 4], [5, 6]], np.int32)
    np.testing.assert_array_equal(G.gather_rows(src, [2, 0, 2, 1], 3, 4), [[5, 6], [1, 2], [5, 6], [0, 0]])
    np.testing.assert_array_equal(G.gather_rows(src, [2, 0, 2, 1], 9, 4), [[5, 6], [1, 2], [5, 6], [3, 4]])
    assert not G.gather_rows(src.astype(F32), [2, 0, 2, 1], 0, 4).any()
    # three images of P = 3 rows: counts 2, 0 (a middle image without survivors) and 7 (above P)
    codes = np.arange(9, dtype=F32)[:, None] * np.ones((1, 4), F32)
    picks = np.array([2, 0, 1, 1, 1, 1, 1, 2, 0], np.int32)
    K, off, total = G.group_offsets([2, 0, 7], 3)
    assert K.tolist() == [2, 0, 3] and off.tolist() == [0, 2, 2] and total == 5
    rows, total = G.survivor_compact(codes, picks, [2, 0, 7], 3)
    assert total == 5
    np.testing.assert_array_equal(rows[:, 0], [2, 0, 4 + 3, 5 + 3, 3 + 3])
    with pytest.raises(AssertionError):
        G.group_offsets([-4, 1], 3)                                   # an NMS count is never below 0


def _pack_case(tok_gather=0, with_src=False, codes=False):
    """Three images of P = 3: counts 2, 0, 7."""
    P, T = 3, 2
    fb = np.arange(36, dtype=F32).reshape(9, 4)
    obj = np.arange(9, dtype=F32) / 8
    picks = np.array([2, 0, 1, 1, 1, 1, 1, 2, 0], np.int32)
    tokens = np.arange(100, 118, dtype=np.int32).reshape(9, T)
    cds = (np.arange(18, dtype=F32).reshape(9, 2) + 0.5) if codes else None
    src = np.arange(50, 59, dtype=np.int32) if with_src else None
    recs = G.final_pack(fb, obj, picks, [2, 0, 7], P, tokens=None if codes else tokens, tok_gather=tok_gather, codes=cds,
                        fault=0xdeadbeef, box_src=src)
    return recs, P, T


def test_final_pack_rows_and_the_three_token_orders():
    recs, P, T = _pack_case(0, with_src=True)
    assert [r["K"] for r in recs] == [2, 0, 3] and all(r["fault"] == 0xdeadbeef for r in recs)
    np.testing.assert_array_equal(recs[0]["boxes"], [[8, 9, 10, 11], [0, 1, 2, 3]])
    np.testing.assert_array_equal(recs[0]["scores"], [0.25, 0])
    np.testing.assert_array_equal(recs[2]["boxes"][:, 0], [28, 32, 24])
    np.testing.assert_array_equal(recs[2]["src"], [57, 58, 56])
    assert recs[1]["boxes"].shape == (0, 4) and recs[1]["tokens"].shape == (0, T)
    np.testing.assert_array_equal(recs[2]["tokens"], [[112, 113], [114, 115], [116, 117]])     # 0: rows 6, 7, 8 as they stand
    np.testing.assert_array_equal(_pack_case(1)[0][2]["tokens"], [[114, 115], [116, 117], [112, 113]])   # 1: rows of the picks
    np.testing.assert_array_equal(_pack_case(2)[0][2]["tokens"], [[104, 105], [106, 107], [108, 109]])   # 2: packed, from row 2
    np.testing.assert_array_equal(_pack_case(2)[0][0]["tokens"], [[100, 101], [102, 103]])
    np.testing.assert_array_equal(_pack_case(codes=True)[0][0]["codes"], [[4.5, 5.5], [0.5, 1.5]])


def test_record_layout_is_the_documented_one():
    """K at byte 0, the fault word at byte 68, the payload at byte 256: boxes (P, 4), scores (P), P rows of values, P int32 of src
    (densecap_amd/csrc/common.h)."""
    hdr = open(os.path.join(ROOT, "densecap_amd", "csrc", "common.h")).read()
    assert re.search(r"kRecK = 0, kRecFault = 68, kRecPayload = 256;", hdr)
    assert (G.REC_K, G.REC_FAULT, G.REC_PAYLOAD) == (0, 68, 256)
    recs, P, T = _pack_case(0, with_src=True)
    assert G.record_bytes(P, T, True) == 256 + 4 * 3 * 8
    raw = G.pack_record(recs[2], P, T, True, 512)
    assert raw[0:4].view(np.int32)[0] == 3 and raw[68:72].view(np.uint32)[0] == 0xdeadbeef
    np.testing.assert_array_equal(raw[256:256 + 48].view(F32).reshape(3, 4)[:, 0], [28, 32, 24])
    np.testing.assert_array_equal(raw[256 + 48:256 + 60].view(F32), [7 / 8, 1, 6 / 8])
    np.testing.assert_array_equal(raw[256 + 60:256 + 84].view(np.int32), [112, 113, 114, 115, 116, 117])
    np.testing.assert_array_equal(raw[256 + 84:256 + 96].view(np.int32), [57, 58, 56])
    assert (raw[4:68] == G.BYTE_FILL).all() and (raw[72:256] == G.BYTE_FILL).all() and (raw[256 + 96:] == G.BYTE_FILL).all()
    u = G.unpack_record(raw, P, T, True)
    assert u["K"] == 3 and u["fault"] == 0xdeadbeef and u["values"].shape == (3, 2) and u["src"].tolist() == [57, 58, 56]
    # a record of two rows leaves the third row of every section at the sentinel
    raw0 = G.pack_record(recs[0], P, T, True, 512)
    u0 = G.unpack_record(raw0, P, T, True)
    assert u0["K"] == 2 and (u0["values"][2] == 0x5a5a5a5a).all() and u0["src"][2] == 0x5a5a5a5a
    G.assert_record(raw0, recs[0], P, T, True)
    G.assert_record(raw, recs[2], P, T, True)


# ---- negative controls: one perturbation, the helper must raise ---------------------------------------------------------------------
def _ulp2(x):
    """x moved by two units in the last place."""
    return (np.array([x], F32).view(np.uint32) + 2).view(F32)[0]


def _filled(shape, dtype):
    return np.full(shape, G.fill_of(dtype), {4: np.uint32, 1: np.uint8}[np.dtype(dtype).itemsize]).view(dtype)


def _raises(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def _compact_case():
    """Three images of P = 4, D = 4, counts 3, 2, 4, as a device buffer of nimg * P + 2 rows: (buffer, rows, total, codes, picks)."""
    rng = np.random.default_rng(3)
    codes = rng.standard_normal((12, 4)).astype(F32)
    picks = np.concatenate([rng.permutation(4) for _ in range(3)]).astype(np.int32)
    rows, total = G.survivor_compact(codes, picks, [3, 2, 4], 4)
    buf = _filled((14, 4), F32)
    buf[:total] = rows
    return buf, rows, total, codes, picks


def test_sentinels_are_what_the_wrappers_fill_with():
    from densecap_amd import ops
    assert (G.F32_FILL, G.I32_FILL, G.BYTE_FILL) == (ops.GLUE_F32_FILL, ops.GLUE_I32_FILL, ops.GLUE_BYTE_FILL)
    assert np.isnan(_filled((1,), F32)[0]) and _filled((1,), np.int32)[0] == 0x5a5a5a5a
    assert G.record_bytes(7, 15, True) == ops.glue_record_bytes(7, 15, True)


def test_negative_controls_bits_rows_and_untouched():
    buf, rows, total, _, _ = _compact_case()
    G.assert_bits_equal(buf[:total], rows)
    G.assert_rows(buf, rows)
    G.assert_untouched(buf[total:])
    swapped = buf.copy(); swapped[[1, 2]] = swapped[[2, 1]]
    _raises(G.assert_bits_equal, swapped[:total], rows)
    _raises(G.assert_rows, swapped, rows)
    ulp = buf.copy(); ulp[4, 1] = _ulp2(ulp[4, 1])
    _raises(G.assert_bits_equal, ulp[:total], rows)
    _raises(G.assert_rows, ulp, rows)
    guard = buf.copy(); guard[13, 3] = 0.0
    _raises(G.assert_rows, guard, rows)
    _raises(G.assert_untouched, guard[total:])
    _raises(G.assert_rows, buf, rows[:-1])                                  # a count off by one: a row too many was written
    _raises(G.assert_rows, buf, np.concatenate([rows, rows[:1]]))          # ... a row too few
    _raises(G.assert_bits_equal, np.zeros(3, F32), -np.zeros(3, F32))      # -0 is not +0
    ints = _filled((6,), np.int32)
    G.assert_untouched(ints)
    ints[5] = 0x5a5a5a5b
    _raises(G.assert_untouched, ints)
    _raises(G.assert_untouched, np.array([np.nan], F32))                    # another NaN is not the sentinel


def test_negative_controls_counts():
    buf = _filled((3 * 64 + 2,), np.int32)
    buf[::64][:3] = [5, 0, 9]
    G.assert_counts(buf, [5, 0, 9], 64)
    _raises(G.assert_counts, buf, [5, 1, 9], 64)                            # a count off by one
    _raises(G.assert_counts, buf, [5, 9, 0], 64)                            # two swapped
    moved = buf.copy(); moved[65] = 0
    _raises(G.assert_counts, moved, [5, 0, 9], 64)                          # a word between the slots
    tail = buf.copy(); tail[193] = 0
    _raises(G.assert_counts, tail, [5, 0, 9], 64)                           # the guard after the last slot
    one = _filled((5,), np.int32); one[:3] = [5, 0, 9]
    G.assert_counts(one, [5, 0, 9], 1)
    _raises(G.assert_counts, one, [5, 0, 8], 1)


def test_negative_controls_packed_block():
    buf, rows, total, codes, picks = _compact_case()
    G.assert_packed(buf, rows, total, total)
    _raises(G.assert_packed, buf, rows, total, total + 1)                  # *total off by one
    _raises(G.assert_packed, buf, rows, total, total - 1)
    swapped = buf.copy(); swapped[[3, 4]] = swapped[[4, 3]]
    _raises(G.assert_packed, swapped, rows, total, total)
    # a row of image 2 at image 1's offset: image 2's rows start where image 1's do (offset 3 in the place of 5)
    wrong = buf.copy(); wrong[3] = rows[5]
    _raises(G.assert_packed, wrong, rows, total, total)
    # offsets from the raw counts in the place of min(count, P): count 9 for image 0 moves every later image
    shifted = _filled((14, 4), F32); shifted[:3] = rows[:3]; shifted[4:4 + total - 3] = rows[3:]
    _raises(G.assert_packed, shifted, rows, total, total)
    ulp = buf.copy(); ulp[8, 0] = _ulp2(ulp[8, 0])
    _raises(G.assert_packed, ulp, rows, total, total)
    guard = buf.copy(); guard[total, 0] = 1.0
    _raises(G.assert_packed, guard, rows, total, total)


@pytest.mark.parametrize("tok_gather,with_src,codes", [(0, True, False), (2, False, False), (1, True, False), (0, True, True)])
def test_negative_controls_record(tok_gather, with_src, codes):
    recs, P, T = _pack_case(tok_gather, with_src, codes)
    stride = 512
    raws = [G.pack_record(r, P, T, with_src, stride) for r in recs]
    for raw, r in zip(raws, recs):
        G.assert_record(raw, r, P, T, with_src)
    raw, rec = raws[2], recs[2]
    def broken(at, value, dtype):
        b = raw.copy()
        b[at:at + np.dtype(dtype).itemsize] = np.array([value], dtype).view(np.uint8)
        return b
    vals = 256 + 20 * P
    _raises(G.assert_record, broken(0, 2, np.int32), rec, P, T, with_src)                    # K off by one
    _raises(G.assert_record, broken(0, 4, np.int32), rec, P, T, with_src)
    _raises(G.assert_record, broken(68, 0xdeadbeee, np.uint32), rec, P, T, with_src)        # the fault word
    _raises(G.assert_record, broken(64, 0, np.int32), rec, P, T, with_src)                   # padding between the header fields
    _raises(G.assert_record, broken(72, 0, np.int32), rec, P, T, with_src)
    _raises(G.assert_record, broken(G.record_bytes(P, T, with_src), 0, np.uint8), rec, P, T, with_src)   # after the record
    _raises(G.assert_record, broken(stride - 1, 0, np.uint8), rec, P, T, with_src)
    _raises(G.assert_record, broken(256 + 16 * P + 4, _ulp2(rec["scores"][1]), F32), rec, P, T, with_src)     # two ulp on a score
    sw = raw.copy()                                                                           # two value rows swapped
    sw[vals:vals + 8], sw[vals + 8:vals + 16] = raw[vals + 8:vals + 16], raw[vals:vals + 8]
    _raises(G.assert_record, sw, rec, P, T, with_src)
    # a row from K on written: image 0 keeps 2 of 3 rows
    r0 = raws[0].copy(); r0[256 + 32:256 + 36] = 0
    _raises(G.assert_record, r0, recs[0], P, T, with_src)
    r0 = raws[0].copy(); r0[vals + 16] = 0
    _raises(G.assert_record, r0, recs[0], P, T, with_src)
    if with_src:
        _raises(G.assert_record, broken(vals + 8 * P, int(rec["src"][0]) + 1, np.int32), rec, P, T, with_src)
        r0 = raws[0].copy(); r0[vals + 8 * P + 8] = 0
        _raises(G.assert_record, r0, recs[0], P, T, with_src)
    if tok_gather == 2:
        # image 2's token rows read at image 1's offset -- the same here, since image 1 is empty -- are right; read at
        # image 2's own block offset (6, the unpacked order) they are not: a wrong tok0 shows
        other = _pack_case(0, with_src, codes)[0][2]
        assert not np.array_equal(other["tokens"], rec["tokens"])
        _raises(G.assert_record, G.pack_record(other, P, T, with_src, stride), rec, P, T, with_src)


def test_negative_controls_bar():
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((6, 4))
    bar = np.full((6, 4), 1e-6)
    ref[2, 1] = np.nan
    got = ref + 0.9e-6 * rng.choice([-1.0, 1.0], ref.shape)
    assert 0.89 < G.assert_within_bar(got, ref, bar) < 0.91
    off = got.copy(); off[4, 0] = ref[4, 0] + 2e-6
    _raises(G.assert_within_bar, off, ref, bar)                             # one element past its bar
    sw = got.copy(); sw[[0, 1]] = sw[[1, 0]]
    _raises(G.assert_within_bar, sw, ref, bar)                              # two rows swapped
    sw = got.copy(); sw[[2, 3]] = sw[[3, 2]]
    _raises(G.assert_within_bar, sw, ref, bar)                              # the NaN in another row
    spread = got.copy(); spread[5, 3] = np.nan
    _raises(G.assert_within_bar, spread, ref, bar)                          # a NaN that left its row
    # two units in the last place are inside a bar of 12 .. 72 of them by design; a whole bar beyond is not
    tight = ref.astype(F32)
    fbar = np.abs(tight.astype(np.float64)) * 12 * 2.0 ** -24 + 1e-30
    moved = tight.copy(); moved[0, 0] = _ulp2(moved[0, 0])
    G.assert_within_bar(moved, tight.astype(np.float64), fbar)
    moved[0, 0] = F32(tight[0, 0] * (1 + 26 * 2.0 ** -24))
    _raises(G.assert_within_bar, moved, tight.astype(np.float64), fbar)


# ---- the hooks' header ------------------------------------------------------------------------------------------------------------
def _declared_symbols(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def test_hook_header_symbols_are_exported_and_off_the_boundary():
    from densecap_amd import _lib
    hooks = _declared_symbols("densecap_debug_glue.h")
    assert sorted(hooks) == sorted(_lib._GLUE_HOOK_SIGS) and len(hooks) == 7
    lib = _lib.lib()
    for name in hooks:
        assert hasattr(lib, name), name
    assert not [h for h in hooks if h in open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()]
    assert not set(hooks) & set(_lib.EXPORTED_SYMBOLS)
    for other in ("densecap.h", "densecap_debug.h", "densecap_debug_grad.h", "densecap_debug_recog.h", "densecap_debug_bwd.h",
                  "densecap_debug_sample.h", "densecap_debug_beam.h", "densecap_debug_rpn.h", "densecap_debug_optim.h",
                  "densecap_debug_step.h"):
        assert not set(hooks) & set(_declared_symbols(other)), other


def test_struct_bindings_mirror_the_header():
    from densecap_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap_debug_glue.h")).read(), flags=re.S)
    for name, cls in (("dc_glue_roi_pool", _lib.DcGlueRoiPool), ("dc_glue_final_pack", _lib.DcGlueFinalPack)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f for f, _ in cls._fields_], name
