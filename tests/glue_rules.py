"""Plain numpy restatements of the forward path's glue kernels -- boxes_ingest_kernel, bilinear_roi_pool_kernel in its group form,
recog_heads_kernel, iota_count_kernel, gather_rows_kernel, survivor_compact_kernel, final_pack_kernel -- and the comparison helpers
tests/test_gpu_glue_kernels.py rests on.  Integer logic is exact; floating point is float64 where it matters (the heads' dot
products, with the error bar of their summation order).  tests/test_glue_rules_cpu.py checks the rules on hand-written cases and
shows that every helper fails for the errors these kernels would make: rows swapped, a count off by one, a guard word changed, a
row of one image at another image's offset, an element off by two units in the last place.

Sentinels: every output buffer of a device test holds F32_FILL (a NaN pattern) in float32 buffers, I32_FILL in int32 buffers and
BYTE_FILL in the byte records before the launch."""
import numpy as np

from oracle import densecap_oracle as O

F32 = np.float32
F32_FILL = 0x7fc5a5a5
I32_FILL = 0x5a5a5a5a
BYTE_FILL = 0x5a
# one image's packed result record (densecap_amd/csrc/common.h: kRecK, kRecFault, kRecPayload)
REC_K, REC_FAULT, REC_PAYLOAD = 0, 68, 256


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def ingest(in_boxes, in_n, P, clip, H, W):
    """in_boxes (nimg * P, 4), in_n (nimg,) -> per image (roi_boxes (P, 4), box_src (P,), count): the first n = max(0, min(in_n, P))
    rows, clipped to the image and without the rows the clip makes invalid when `clip`, in order; zeros and -1 from count on."""
    b = np.asarray(in_boxes, F32).reshape(-1, P, 4)
    res = []
    for i, n_in in enumerate(in_n):
        n = max(0, min(int(n_in), P))
        rows = b[i, :n]
        valid = np.ones((n,), bool)
        if clip and n:
            rows, valid = O.clip_boxes_xcycwh(rows, 1, 1, W, H)
        keep = np.nonzero(valid)[0]
        roi, src = np.zeros((P, 4), F32), np.full((P,), -1, np.int32)
        roi[:len(keep)] = rows[keep]
        src[:len(keep)] = keep
        res.append((roi, src, len(keep)))
    return res


def live_count(count, cap):
    return max(0, min(int(count), int(cap)))


def roi_pool_group(feats, B, H, W, HH, WW, out_layout, boxes=None, live=None, pick=None, src_boxes=None):
    """feats (nimg, C, h, w); boxes (nimg * B, 4), or pick (nimg * B,) into src_boxes (nimg, S, 4); live (nimg,) device-side
    counts or None.  -> (out (nimg * B, C, HH, WW) or (nimg * B, HH, WW, C), boxes (nimg * B, 4) as the kernel leaves them with a
    pick list, else None): every image by the oracle on its own map and live boxes, dead rows zero."""
    f = np.asarray(feats, F32)
    nimg, C = f.shape[:2]
    out = np.zeros((nimg, B, C, HH, WW), F32)
    bout = np.zeros((nimg, B, 4), F32) if pick is not None else None
    for i in range(nimg):
        n = live_count(live[i], B) if live is not None else B
        if pick is not None:
            bx = np.asarray(src_boxes, F32)[i][np.asarray(pick).reshape(nimg, B)[i, :n]]
            bout[i, :n] = bx
        else:
            bx = np.asarray(boxes, F32).reshape(nimg, B, 4)[i, :n]
        if n:
            out[i, :n] = O.bilinear_roi_pool(f[i], bx, H, W, HH, WW)
    out = out.reshape(nimg * B, C, HH, WW)
    if out_layout == 1:
        out = np.ascontiguousarray(out.transpose(0, 2, 3, 1))
    return out, (bout.reshape(nimg * B, 4) if bout is not None else None)


def heads_terms(D):
    """Rounded additions behind one output of recog_heads_kernel: a lane adds 4 products per trip of its k loop, ceil(D / 256)
    trips, then six wave-reduction steps and the bias; one more for the products' own rounding."""
    return 4 * ((int(D) + 255) // 256) + 8


def heads(codes, w5, b5, roi):
    """codes (n, D), w5 (5, D) rows objectness then the four box-regression rows, b5 (5,), roi (n, 4) -> dict in float64: obj (n,),
    trans (n, 4), their error bars bar_obj, bar_trans -- |device - value| <= heads_terms(D) 2^-24 (sum_k |x_k w_k| + |b|) -- and
    fin (n, 4) = ApplyBoxTransform(roi, trans) (the device's fin is held bit for bit to the device's own transform op instead)."""
    x, w, b = np.asarray(codes, np.float64), np.asarray(w5, np.float64), np.asarray(b5, np.float64)
    r = np.asarray(roi, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x @ w.T + b
        bar = heads_terms(x.shape[1]) * 2.0 ** -24 * (np.abs(x) @ np.abs(w).T + np.abs(b))
        t = s[:, 1:]
        fin = np.stack([t[:, 0] * r[:, 2] + r[:, 0], t[:, 1] * r[:, 3] + r[:, 1], np.exp(t[:, 2]) * r[:, 2], np.exp(t[:, 3]) * r[:, 3]], 1)
    return dict(obj=s[:, 0], trans=t, bar_obj=bar[:, 0], bar_trans=bar[:, 1:], fin=fin)


def iota_count(cap, count_in):
    return np.arange(cap, dtype=np.int32), np.int32(count_in)


def gather_rows(src, idx, count, cap):
    """out (cap, width): row i = src[idx[i]] for i < count, zeros from there on."""
    src = np.asarray(src)
    out = np.zeros((cap, src.shape[1]), src.dtype)
    n = live_count(count, cap)
    out[:n] = src[np.asarray(idx)[:n]]
    return out


def group_offsets(count, P):
    """(K (nimg,), off (nimg,), total): K_i = min(count_i, P), off_i = the sum of the earlier K.  The counts are an NMS's: never
    below 0 (the kernels do not clamp from below, and the hooks refuse a negative count)."""
    assert min(int(c) for c in count) >= 0, "a count below 0"
    K = np.array([min(int(c), int(P)) for c in count], np.int64)
    off = np.concatenate([[0], np.cumsum(K)[:-1]]).astype(np.int64)
    return K, off, int(K.sum())


def survivor_compact(codes, picks, count, P):
    """codes (nimg * P, D), picks (nimg * P,) -> (packed rows (total, D), total): image by image, in pick order."""
    x, pk = np.asarray(codes), np.asarray(picks)
    K, _, total = group_offsets(count, P)
    rows = [x[i * P + pk[i * P:i * P + K[i]]] for i in range(len(K))]
    return np.concatenate(rows, 0).reshape(total, x.shape[1]), total


def final_pack(final_boxes, obj, picks, count, P, tokens=None, tok_gather=0, codes=None, fault=0, box_src=None):
    """What each image's record holds: dict(K, fault, boxes (K, 4), scores (K,), tokens (K, T) int32 | codes (K, D), src (K,) with
    box_src).  tok_gather 0: the token rows stand in final order at [i * P, i * P + K); 1: the token row of the pick; 2: final
    order, packed over the group at group_offsets."""
    fb, ob, pk = np.asarray(final_boxes, F32).reshape(-1, 4), np.asarray(obj, F32).reshape(-1), np.asarray(picks)
    K, off, _ = group_offsets(count, P)
    recs = []
    for i in range(len(K)):
        k = int(K[i])
        src = i * P + pk[i * P:i * P + k]
        r = dict(K=k, fault=int(fault), boxes=fb[src], scores=ob[src])
        if codes is not None:
            r["codes"] = np.asarray(codes, F32)[src]
        else:
            t = np.asarray(tokens, np.int32)
            rows = src if tok_gather == 1 else (off[i] if tok_gather == 2 else i * P) + np.arange(k)
            r["tokens"] = t[rows]
        if box_src is not None:
            r["src"] = np.asarray(box_src, np.int32)[src]
        recs.append(r)
    return recs


def record_bytes(P, words, with_src):
    return REC_PAYLOAD + 4 * P * (5 + words + (1 if with_src else 0))


def unpack_record(raw, P, words, with_src):
    """A raw record (uint8, at least record_bytes long) -> dict(K, fault, boxes (P, 4) float32, scores (P,) float32, values
    (P, words) uint32, src (P,) int32 with_src): ALL P rows of every section, written or not."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    word = lambda at, dt: raw[at:at + 4].view(dt)[0]
    o = REC_PAYLOAD
    sect = lambda n, dt, shape: raw[o:o + 4 * n].view(dt).reshape(shape)
    r = dict(K=int(word(REC_K, np.int32)), fault=int(word(REC_FAULT, np.uint32)))
    r["boxes"] = sect(4 * P, F32, (P, 4)); o += 16 * P
    r["scores"] = sect(P, F32, (P,)); o += 4 * P
    r["values"] = sect(P * words, np.uint32, (P, words)); o += 4 * P * words
    if with_src:
        r["src"] = sect(P, np.int32, (P,))
    return r


def pack_record(rec, P, words, with_src, stride):
    """The inverse: `stride` bytes holding BYTE_FILL and what final_pack_kernel writes of `rec` (a dict of final_pack)."""
    raw = np.full((stride,), BYTE_FILL, np.uint8)
    raw[REC_K:REC_K + 4] = np.array([rec["K"]], np.int32).view(np.uint8)
    raw[REC_FAULT:REC_FAULT + 4] = np.array([rec["fault"]], np.uint32).view(np.uint8)
    k, o = rec["K"], REC_PAYLOAD
    def put(at, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        raw[at:at + b.size] = b
    put(o, rec["boxes"].astype(F32)); o += 16 * P
    put(o, rec["scores"].astype(F32)); o += 4 * P
    put(o, rec["codes"].astype(F32) if "codes" in rec else rec["tokens"].astype(np.int32)); o += 4 * P * words
    if with_src:
        put(o, rec["src"].astype(np.int32))
    assert k <= P
    return raw


# ---- comparison helpers of the device tests --------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits_equal(got, want, what=""):
    """Same shape, same dtype size, same bits (a NaN equals only the same NaN; -0 is not +0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, wanted %s" % (what, got.shape, want.shape)
    assert got.dtype.itemsize == want.dtype.itemsize, what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, "%s: %d of %d elements differ, first at %s: %r, wanted %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def fill_of(dtype):
    dtype = np.dtype(dtype)
    return F32_FILL if dtype == np.float32 else I32_FILL if dtype.itemsize == 4 else BYTE_FILL


def assert_untouched(a, what=""):
    """Every element still holds the sentinel of its type."""
    a = np.ascontiguousarray(a)
    bad = np.argwhere(_bits(a) != fill_of(a.dtype))
    assert len(bad) == 0, "%s: %d elements were written, first at %s" % (what, len(bad), tuple(bad[0]))


def assert_rows(buf, want, what=""):
    """buf's first len(want) rows are `want` bit for bit, every later row (the rows a kernel must leave alone, guards included)
    still holds the sentinel."""
    buf, want = np.asarray(buf), np.asarray(want)
    assert len(buf) >= len(want), what
    assert_bits_equal(buf[:len(want)], want.reshape((len(want),) + buf.shape[1:]), what)
    assert_untouched(buf[len(want):], what + " past row %d" % len(want))


def assert_counts(buf, want, stride, what=""):
    """buf[i * stride] = want[i]; every other slot, the guards after the last image included, holds the sentinel."""
    buf, want = np.asarray(buf), np.asarray(want, np.int32).reshape(-1)
    slots = np.arange(len(want)) * stride
    assert_bits_equal(buf[slots], want, what)
    rest = np.ones(len(buf), bool)
    rest[slots] = False
    assert_untouched(buf[rest], what + " between the slots")


def assert_packed(buf, rows, total, got_total, what=""):
    """survivor_compact's block: *total, the packed rows at [0, total), sentinels from there on."""
    assert int(got_total) == int(total) == len(rows), "%s: total %d, wanted %d" % (what, int(got_total), int(total))
    assert_rows(buf, rows, what)


def assert_record(raw, rec, P, words, with_src, what=""):
    """One record's bytes (the whole stride) against a dict of final_pack: K, the fault word, every row below K of every section;
    every other byte -- the header's padding, the rows from K on, the bytes after the record up to the stride -- is BYTE_FILL."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    u = unpack_record(raw, P, words, with_src)
    assert u["K"] == rec["K"], "%s: K = %d, wanted %d" % (what, u["K"], rec["K"])
    assert u["fault"] == rec["fault"], "%s: fault word 0x%x, wanted 0x%x" % (what, u["fault"], rec["fault"])
    k = rec["K"]
    assert_bits_equal(u["boxes"][:k], rec["boxes"], what + " boxes")
    assert_bits_equal(u["scores"][:k], rec["scores"], what + " scores")
    assert_bits_equal(u["values"][:k], rec["codes"] if "codes" in rec else rec["tokens"], what + " values")
    if with_src:
        assert_bits_equal(u["src"][:k], rec["src"], what + " src")
    written = np.zeros(len(raw), bool)
    written[REC_K:REC_K + 4] = written[REC_FAULT:REC_FAULT + 4] = True
    o = REC_PAYLOAD
    for row_bytes in [16, 4, 4 * words] + ([4] if with_src else []):
        written[o:o + k * row_bytes] = True
        o += P * row_bytes
    bad = np.nonzero((raw != BYTE_FILL) & ~written)[0]
    assert len(bad) == 0, "%s: %d bytes outside the record's rows were written, first at byte %d" % (what, len(bad), bad[0])


def assert_within_bar(got, ref, bar, what=""):
    """|got - ref| <= bar element by element; where ref is not finite (a NaN or an overflow crafted into one row) got must be the
    same kind of value in the same place, and nowhere else."""
    got, ref, bar = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bar, np.float64)
    assert got.shape == ref.shape == bar.shape, what
    assert (np.isnan(got) == np.isnan(ref)).all(), "%s: NaNs at %s, wanted at %s" % (what, np.argwhere(np.isnan(got)).tolist(),
                                                                                     np.argwhere(np.isnan(ref)).tolist())
    fin = np.isfinite(ref)
    assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all(), what
    err = np.abs(got[fin] - ref[fin])
    worst = (err / np.maximum(bar[fin], 1e-300)).max(initial=0.0)
    assert (err <= bar[fin]).all(), "%s: worst err / bar = %.3f" % (what, worst)
    return worst
