"""Per-op host wrappers over the C ABI (numpy in / numpy out, device buffers via dc_malloc).

Names follow the reference's modules (densecap/modules/*.lua, densecap/box_utils.lua) so the
parity tests read like the reference's own tests.  Every function runs the HIP kernel; there is
no CPU path here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


class Context:
    """Owns a dc_ctx (utils.setup_gpus equivalent, densecap/utils.lua:22-36)."""

    def __init__(self, device=0):
        self.lib = _lib.lib()
        h = C.c_void_p()
        rc = self.lib.dc_create(C.byref(h), int(device))
        if rc < 0:
            msg = self.lib.dc_last_error(None)
            raise _lib.DenseCapError("dc_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.h = h
        self.device = device

    def set_math_mode(self, mode):
        """dc_set_math_mode (include/densecap.h): 0 = fp32 MFMA, 1 = split-bf16 -- applies to every contraction of this ctx."""
        check(self.h, self.lib.dc_set_math_mode(self.h, int(mode)), "dc_set_math_mode")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device buffers ----
    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceArray(self, arr.shape, arr.dtype)
        check(self.h, self.lib.dc_memcpy_h2d(self.h, buf.ptr, arr.ctypes.data, arr.nbytes), "dc_memcpy_h2d")
        return buf

    def empty(self, shape, dtype=np.float32):
        return DeviceArray(self, shape, dtype)


class DeviceArray:
    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(ctx.h, ctx.lib.dc_malloc(ctx.h, C.byref(p), max(self.nbytes, 16)), "dc_malloc")
        self.ptr = p

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            check(self.ctx.h, self.ctx.lib.dc_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes),
                  "dc_memcpy_d2h")
        return out

    def free(self):
        if self.ptr is not None and self.ctx.h:
            self.ctx.lib.dc_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- preprocessing (run_model.lua:67-74 on the device) ----------------------------------------
def preprocess_size(lib, H0, W0, image_size):
    H, W = C.c_int(0), C.c_int(0)
    rc = lib.dc_preprocess_size(int(H0), int(W0), int(image_size), C.byref(H), C.byref(W))
    if rc < 0:
        raise ValueError("image.scale: %dx%d -> size %d leaves no pixels" % (W0, H0, image_size))
    return H.value, W.value


def preprocess_u8(ctx, rgb_hwc_u8, image_size, want_rgb=True, out=None, rgb=None):
    """image.load's float conversion + image.scale(img, image_size) + BGR, x255, minus the VGG mean, on the device
    (dc_preprocess_u8).  rgb_hwc_u8: (H0,W0,3) uint8 as a JPEG decoder delivers it.  Returns (DeviceArray (3,H,W) float32 --
    what forward_images_device takes --, DeviceArray (H,W,3) uint8 of the scaled image for the visualiser or None).
    out / rgb: buffers of exactly those shapes to fill instead of new ones."""
    a = np.ascontiguousarray(rgb_hwc_u8, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("preprocess_u8 wants an (H,W,3) uint8 image")
    H0, W0 = a.shape[:2]
    H, W = preprocess_size(ctx.lib, H0, W0, image_size)
    if out is None:
        out = ctx.empty((3, H, W), np.float32)
    if rgb is None and want_rgb:
        rgb = ctx.empty((H, W, 3), np.uint8)
    if out.shape != (3, H, W) or (rgb is not None and rgb.shape != (H, W, 3)):
        raise ValueError("preprocess_u8: output buffers do not have the scaled image's shape")
    check(ctx.h, ctx.lib.dc_preprocess_u8(ctx.h, a.ctypes.data, H0, W0, 0, int(image_size), out.ptr, rgb.ptr if rgb else None),
          "dc_preprocess_u8")
    return out, rgb


# ---- layout ----------------------------------------------------------------------------------
def chw_to_hwc(ctx, x):
    C_, H, W = x.shape
    a = ctx.to_device(_f32(x)); o = ctx.empty((H, W, C_))
    check(ctx.h, ctx.lib.dc_op_chw_to_hwc(ctx.h, a.ptr, o.ptr, C_, H, W), "dc_op_chw_to_hwc")
    return o.numpy()


def hwc_to_chw(ctx, x):
    H, W, C_ = x.shape
    a = ctx.to_device(_f32(x)); o = ctx.empty((C_, H, W))
    check(ctx.h, ctx.lib.dc_op_hwc_to_chw(ctx.h, a.ptr, o.ptr, C_, H, W), "dc_op_hwc_to_chw")
    return o.numpy()


# ---- dense ops ---------------------------------------------------------------------------------
def conv3x3(ctx, x_nchw, w_oihw, bias, relu=True):
    """nn.SpatialConvolution(Cin,Cout,3,3,1,1,1,1)[+ReLU] on (N,Cin,H,W) -> (N,Cout,H,W)."""
    x = _f32(x_nchw); w = _f32(w_oihw)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if Cin == 3:
        assert N == 1
        xi = ctx.to_device(x[0]); wd = ctx.to_device(w); bd = ctx.to_device(_f32(bias))
        o = ctx.empty((H, W, Cout))
        check(ctx.h, ctx.lib.dc_op_conv3x3_c3(ctx.h, xi.ptr, wd.ptr, bd.ptr, o.ptr, H, W, Cout, int(relu)),
              "dc_op_conv3x3_c3")
        return np.ascontiguousarray(o.numpy().transpose(2, 0, 1))[None]
    xh = ctx.to_device(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    wd = ctx.to_device(w); wp = ctx.empty((Cout, 9 * Cin)); bd = ctx.to_device(_f32(bias))
    check(ctx.h, ctx.lib.dc_op_pack_conv3x3_weights(ctx.h, wd.ptr, wp.ptr, Cout, Cin), "pack")
    o = ctx.empty((N, H, W, Cout))
    check(ctx.h, ctx.lib.dc_op_conv3x3(ctx.h, xh.ptr, wp.ptr, bd.ptr, o.ptr, N, H, W, Cin, Cout, int(relu)),
          "dc_op_conv3x3")
    return np.ascontiguousarray(o.numpy().transpose(0, 3, 1, 2))


def conv3x3_relu_pool(ctx, x_chw, w_oihw, bias):
    """conv3x3 + ReLU + ceil-mode 2x2 max-pool in one launch: (Cin,H,W) -> (Cout, ceil(H/2), ceil(W/2))."""
    x = _f32(x_chw); w = _f32(w_oihw)
    Cin, H, W = x.shape
    Cout = w.shape[0]
    xh = ctx.to_device(np.ascontiguousarray(x.transpose(1, 2, 0)))
    wd = ctx.to_device(w); wp = ctx.empty((Cout, 9 * Cin)); bd = ctx.to_device(_f32(bias))
    check(ctx.h, ctx.lib.dc_op_pack_conv3x3_weights(ctx.h, wd.ptr, wp.ptr, Cout, Cin), "pack")
    o = ctx.empty(((H + 1) // 2, (W + 1) // 2, Cout))
    check(ctx.h, ctx.lib.dc_op_conv3x3_relu_pool(ctx.h, xh.ptr, wp.ptr, bd.ptr, o.ptr, H, W, Cin, Cout),
          "dc_op_conv3x3_relu_pool")
    return np.ascontiguousarray(o.numpy().transpose(2, 0, 1))


def maxpool2x2_ceil(ctx, x_nchw):
    x = _f32(x_nchw)
    N, C_, H, W = x.shape
    xh = ctx.to_device(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    o = ctx.empty((N, (H + 1) // 2, (W + 1) // 2, C_))
    check(ctx.h, ctx.lib.dc_op_maxpool2x2_ceil(ctx.h, xh.ptr, o.ptr, N, H, W, C_), "dc_op_maxpool2x2_ceil")
    return np.ascontiguousarray(o.numpy().transpose(0, 3, 1, 2))


def linear(ctx, x, w, bias=None, relu=False):
    """nn.Linear: x (M,K) . w (N,K)^T + bias."""
    x = _f32(x); w = _f32(w)
    M, K = x.shape
    N = w.shape[0]
    xd = ctx.to_device(x); wd = ctx.to_device(w)
    bd = ctx.to_device(_f32(bias)) if bias is not None else None
    o = ctx.empty((M, N))
    check(ctx.h, ctx.lib.dc_op_linear(ctx.h, xd.ptr, wd.ptr, bd.ptr if bd else None, o.ptr, M, N, K, int(relu)),
          "dc_op_linear")
    return o.numpy()


# ---- box ops ------------------------------------------------------------------------------------
def make_anchors(ctx, h, w, x0, y0, sx, sy, anchors):
    anchors = _f32(anchors)
    k = anchors.shape[1]
    ad = ctx.to_device(anchors); o = ctx.empty((k * h * w, 4))
    check(ctx.h, ctx.lib.dc_op_make_anchors(ctx.h, o.ptr, h, w, x0, y0, sx, sy, ad.ptr, k), "dc_op_make_anchors")
    return o.numpy()


def apply_box_transform(ctx, boxes, trans):
    b = _f32(boxes).reshape(-1, 4); t = _f32(trans).reshape(-1, 4)
    bd = ctx.to_device(b); td = ctx.to_device(t); o = ctx.empty(b.shape)
    check(ctx.h, ctx.lib.dc_op_apply_box_transform(ctx.h, bd.ptr, td.ptr, o.ptr, b.shape[0]), "apply_box_transform")
    return o.numpy().reshape(np.shape(boxes))


def clip_boxes(ctx, boxes, bounds):
    """box_utils.clip_boxes(boxes, bounds, 'xcycwh') -> (clipped, valid)."""
    b = _f32(boxes).reshape(-1, 4)
    bd = ctx.to_device(b); o = ctx.empty(b.shape); v = ctx.empty((b.shape[0],), np.uint8)
    check(ctx.h, ctx.lib.dc_op_clip_boxes(ctx.h, bd.ptr, o.ptr, v.ptr, b.shape[0], bounds["x_min"], bounds["y_min"],
                                          bounds["x_max"], bounds["y_max"]), "dc_op_clip_boxes")
    return o.numpy().reshape(np.shape(boxes)), v.numpy().astype(bool)


def xcycwh_to_x1y1x2y2(ctx, boxes):
    b = _f32(boxes).reshape(-1, 4)
    bd = ctx.to_device(b); o = ctx.empty(b.shape)
    check(ctx.h, ctx.lib.dc_op_xcycwh_to_x1y1x2y2(ctx.h, bd.ptr, o.ptr, b.shape[0]), "xcycwh_to_x1y1x2y2")
    return o.numpy().reshape(np.shape(boxes))


def box_iou(ctx, b1, b2, convention=0):
    b1 = _f32(b1); b2 = _f32(b2)
    d1 = ctx.to_device(b1); d2 = ctx.to_device(b2); o = ctx.empty((b1.shape[0], b2.shape[0]))
    check(ctx.h, ctx.lib.dc_op_box_iou(ctx.h, d1.ptr, d2.ptr, o.ptr, b1.shape[0], b2.shape[0], convention), "box_iou")
    return o.numpy()


def rpn_decode(ctx, box_head, score_head, img_h, img_w, anchors, field_centers):
    """box_head (4k,h,w), score_head (2k,h,w) as the reference's RPN convs emit them."""
    k = anchors.shape[1]
    h, w = box_head.shape[1:]
    heads = np.concatenate([_f32(box_head), _f32(score_head)], 0).transpose(1, 2, 0)  # (h,w,6k)
    hd = ctx.to_device(np.ascontiguousarray(heads)); ad = ctx.to_device(_f32(anchors))
    A = k * h * w
    boxes = ctx.empty((A, 4)); anc = ctx.empty((A, 4)); trans = ctx.empty((A, 4)); xyxy = ctx.empty((A, 4))
    p = ctx.empty((A,)); valid = ctx.empty((A,), np.uint8)
    x0, y0, sx, sy = field_centers
    check(ctx.h, ctx.lib.dc_op_rpn_decode(ctx.h, hd.ptr, h, w, k, ad.ptr, x0, y0, sx, sy, img_h, img_w, boxes.ptr,
                                          anc.ptr, trans.ptr, xyxy.ptr, p.ptr, valid.ptr), "dc_op_rpn_decode")
    return dict(boxes=boxes.numpy(), anchors=anc.numpy(), trans=trans.numpy(), x1y1x2y2=xyxy.numpy(),
                p=p.numpy(), valid=valid.numpy().astype(bool))


def nms(ctx, boxes5, overlap, max_boxes=None, valid=None):
    """box_utils.nms(boxes(N,5), overlap, max_boxes) -> 0-based picks (decreasing score)."""
    b = _f32(boxes5)
    n = b.shape[0]
    if n == 0:
        return np.zeros((0,), np.int64)
    bd = ctx.to_device(np.ascontiguousarray(b[:, :4])); sd = ctx.to_device(np.ascontiguousarray(b[:, 4]))
    vd = ctx.to_device(np.ascontiguousarray(valid, dtype=np.uint8)) if valid is not None else None
    cap = n if max_boxes is None else min(n, int(max_boxes))
    picks = ctx.empty((max(cap, 1),), np.int32); cnt = ctx.empty((1,), np.int32)
    check(ctx.h, ctx.lib.dc_op_nms(ctx.h, bd.ptr, sd.ptr, vd.ptr if vd else None, n, C.c_float(float(np.float32(overlap))),
                                   -1 if max_boxes is None else int(max_boxes), picks.ptr, cnt.ptr), "dc_op_nms")
    kk = int(cnt.numpy()[0])
    return picks.numpy()[:kk].astype(np.int64)


def nms_multi(ctx, boxes, scores, thresh, max_picks, valid=None):
    """The NMS of `nms` on one box list under Q score columns at once (dc_op_nms_multi): boxes (n,4) x1y1x2y2, scores (n,Q),
    valid (n) or None.  Column q's candidates are the valid rows whose score in q is not NaN; a row that is no candidate is never
    picked and never suppresses.  Returns (picks (Q, max_picks) int32 0-based, -1 past the count, counts (Q) int32)."""
    b = _f32(boxes).reshape(-1, 4)
    s = _f32(scores)
    if s.ndim == 1:
        s = s[:, None]
    n, Q = s.shape
    if b.shape[0] != n:
        raise ValueError("nms_multi: %d boxes but %d score rows" % (b.shape[0], n))
    M = int(max_picks)
    bd = ctx.to_device(b); sd = ctx.to_device(s)
    vd = ctx.to_device(np.ascontiguousarray(valid, dtype=np.uint8)) if valid is not None else None
    if vd is not None and vd.shape != (n,):
        raise ValueError("nms_multi: valid must have one entry per box")
    picks = ctx.empty((max(Q, 1), min(max(M, 1), 4096)), np.int32); cnt = ctx.empty((max(Q, 1),), np.int32)
    check(ctx.h, ctx.lib.dc_op_nms_multi(ctx.h, bd.ptr, sd.ptr, vd.ptr if vd else None, n, Q, C.c_float(float(np.float32(thresh))),
                                         M, picks.ptr, cnt.ptr), "dc_op_nms_multi")
    return picks.numpy(), cnt.numpy()


DC_EVAL_CLAIM_LAST = 1


def eval_match(ctx, det_boxes, det_scores, gt_boxes, merge_thresh=0.7, claim_last=True):
    """DenseCaptioningEvaluator:addResult's matching for a list of images in one launch (dc_op_eval_match; docs/SEMANTICS.md,
    "Evaluation").  det_boxes[i] (B_i,4) xcycwh, det_scores[i] (B_i), gt_boxes[i] (M_i,4) xcycwh, one entry per image.  Returns
    one dict per image: order (B) int32 -- the detection at every rank of the score order --, ov (B) float64, group (B) int32
    (-1 = overlaps nothing), ok (B) uint8, all by rank; gt_group (M) int32, n_groups, merged (n_groups,4) float64 x1y1x2y2."""
    n = len(det_boxes)
    if len(det_scores) != n or len(gt_boxes) != n:
        raise ValueError("eval_match: one box list, score list and ground-truth list per image")
    db = [_f32(b).reshape(-1, 4) for b in det_boxes]
    ds = [_f32(s).reshape(-1) for s in det_scores]
    gb = [_f32(b).reshape(-1, 4) for b in gt_boxes]
    for i in range(n):
        if len(db[i]) != len(ds[i]):
            raise ValueError("eval_match: image %d has %d boxes but %d scores" % (i, len(db[i]), len(ds[i])))
    doff = np.concatenate([[0], np.cumsum([len(b) for b in db])]).astype(np.int32)
    goff = np.concatenate([[0], np.cumsum([len(b) for b in gb])]).astype(np.int32)
    BT, MT = int(doff[-1]), int(goff[-1])
    cat = lambda lst, shape: np.concatenate(lst, 0) if lst else np.zeros(shape, np.float32)
    dbd = ctx.to_device(cat(db, (0, 4))); dsd = ctx.to_device(cat(ds, (0,))); gbd = ctx.to_device(cat(gb, (0, 4)))
    doffd = ctx.to_device(doff); goffd = ctx.to_device(goff)
    order = ctx.empty((BT,), np.int32); ov = ctx.empty((BT,), np.float64); group = ctx.empty((BT,), np.int32)
    ok = ctx.empty((BT,), np.uint8); gt_group = ctx.empty((MT,), np.int32); ng = ctx.empty((max(n, 1),), np.int32)
    merged = ctx.empty((MT, 4), np.float64)
    flags = DC_EVAL_CLAIM_LAST if claim_last else 0
    check(ctx.h, ctx.lib.dc_op_eval_match(ctx.h, dbd.ptr, dsd.ptr, doffd.ptr, gbd.ptr, goffd.ptr, n,
                                          C.c_float(float(np.float32(merge_thresh))), flags, order.ptr, ov.ptr, group.ptr, ok.ptr,
                                          gt_group.ptr, ng.ptr, merged.ptr), "dc_op_eval_match")
    order, ov, group, ok, gt_group, ng, merged = (a.numpy() for a in (order, ov, group, ok, gt_group, ng, merged))
    out = []
    for i in range(n):
        d0, d1, g0, g1 = int(doff[i]), int(doff[i + 1]), int(goff[i]), int(goff[i + 1])
        G = int(ng[i])
        out.append(dict(order=order[d0:d1], ov=ov[d0:d1], group=group[d0:d1], ok=ok[d0:d1], gt_group=gt_group[g0:g1], n_groups=G,
                        merged=merged[g0:g0 + G], merged_tail=merged[g0 + G:g1]))
    return out


LOSS_DEFAULTS = dict(batch_size=256, high_thresh=0.7, low_thresh=0.3, remove_outbounds=1, mid_box_reg_weight=0.05,
                     mid_objectness_weight=0.1, end_box_reg_weight=0.1, end_objectness_weight=0.1, captioning_weight=1.0, seed=0)
LOSS_KEYS = ("mid_objectness_loss", "mid_box_reg_loss", "end_objectness_loss", "end_box_reg_loss", "captioning_loss", "total_loss")


def loss_opts(**kw):
    """A filled DcLossOpts (train_opts.lua:18-40 defaults; docs/SEMANTICS.md, "Validation losses").  Unknown keys raise; the
    library checks the values."""
    unknown = set(kw) - set(LOSS_DEFAULTS)
    if unknown:
        raise ValueError("unknown loss option(s): %s" % ", ".join(sorted(unknown)))
    o = dict(LOSS_DEFAULTS, **kw)
    return _lib.DcLossOpts(int(o["batch_size"]), float(o["high_thresh"]), float(o["low_thresh"]), int(o["remove_outbounds"]),
                           float(o["mid_box_reg_weight"]), float(o["mid_objectness_weight"]), float(o["end_box_reg_weight"]),
                           float(o["end_objectness_weight"]), float(o["captioning_weight"]), int(o["seed"]) & (2 ** 64 - 1))


def _forced_lists(forced_pos, forced_neg):
    """(DcSamplerForced or None, the arrays it points into)"""
    if forced_pos is None and forced_neg is None:
        return None, ()
    f = _lib.DcSamplerForced()
    keep = []
    for name, lst in (("pos", forced_pos), ("neg", forced_neg)):
        if lst is None:
            continue
        a = np.ascontiguousarray(np.asarray(lst, dtype=np.int64).reshape(-1), dtype=np.int32)
        a = a if a.size else np.zeros(1, np.int32)          # a valid pointer for an empty list
        keep.append(a)
        setattr(f, name + "_sample_idx", a.ctypes.data_as(_lib.c_int32_p))
        setattr(f, "num_" + name, int(np.asarray(lst).size))
    return f, keep


def box_sampler(ctx, boxes, gt, img_h, img_w, forced_pos=None, forced_neg=None, want_iou=True, **opts):
    """nn.BoxSampler (dc_op_box_sampler; docs/SEMANTICS.md, "Validation losses"): boxes (A,4), gt (G,4) xcycwh.  Returns a dict:
    pos_input_idx, pos_target_idx (num_pos), neg_input_idx (num_neg) int32 0-based; num_pos, num_neg, total_pos, total_neg,
    flags; with want_iou max_iou (A) float32 and arg (A) int32.  forced_pos / forced_neg: ranks in the class's ascending candidate
    list that take the place of the draws.  opts: the keys of LOSS_DEFAULTS."""
    b = _f32(boxes).reshape(-1, 4); g = _f32(gt).reshape(-1, 4)
    A, G = len(b), len(g)
    o = loss_opts(**opts)
    f, keep = _forced_lists(forced_pos, forced_neg)
    cap = max(int(o.batch_size), 1)
    bd = ctx.to_device(b); gd = ctx.to_device(g)
    pi = ctx.empty((cap,), np.int32); pt = ctx.empty((cap,), np.int32); ni = ctx.empty((cap,), np.int32)
    counts = ctx.empty((8,), np.int32)
    mi = ctx.empty((max(A, 1),), np.float32) if want_iou else None
    ar = ctx.empty((max(A, 1),), np.int32) if want_iou else None
    check(ctx.h, ctx.lib.dc_op_box_sampler(ctx.h, bd.ptr, gd.ptr, A, G, int(img_h), int(img_w), C.byref(o),
                                           C.byref(f) if f is not None else None, pi.ptr, pt.ptr, ni.ptr, counts.ptr,
                                           mi.ptr if want_iou else None, ar.ptr if want_iou else None), "dc_op_box_sampler")
    c = counts.numpy()
    out = dict(pos_input_idx=pi.numpy()[:c[0]], pos_target_idx=pt.numpy()[:c[0]], neg_input_idx=ni.numpy()[:c[1]],
               num_pos=int(c[0]), num_neg=int(c[1]), total_pos=int(c[2]), total_neg=int(c[3]), flags=int(c[4]))
    if want_iou:
        out.update(max_iou=mi.numpy()[:A], arg=ar.numpy()[:A])
    return out


def _train_args(who, ctx, img, gt_boxes, gt_labels, forced_pos, forced_neg, dump, on_device, opts):
    """What forward_losses, loss_gradients and forward_backward hand to the library alike: (their C arguments up to the dump,
    the DcLosses the call fills, the dump's three lists or None, (H, W), batch_size, the objects the pointers point into)."""
    g = _f32(gt_boxes).reshape(-1, 4)
    lab = np.ascontiguousarray(gt_labels, dtype=np.int32)
    if lab.ndim != 2 or len(lab) != len(g):
        raise ValueError("%s: gt_labels must be (G, L) with one row per ground-truth box" % who)
    o = loss_opts(**opts)
    f, keep = _forced_lists(forced_pos, forced_neg)
    out = _lib.DcLosses()
    cap = max(int(o.batch_size), 1)
    lists = [np.zeros(cap, np.int32) for _ in range(3)] if dump else None
    d = _lib.DcLossDump(*[a.ctypes.data_as(_lib.c_int32_p) for a in lists]) if dump else None
    if not on_device:
        img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = int(img.shape[1]), int(img.shape[2])
    args = (ctx.h, img.ptr if on_device else img.ctypes.data, H, W, 1 if on_device else 0, g.ctypes.data, lab.ctypes.data, len(g),
            lab.shape[1], C.byref(o), C.byref(f) if f is not None else None, C.byref(out), C.byref(d) if d is not None else None)
    return args, out, lists, (H, W), cap, (img, g, lab, o, f, keep, d)


def _train_result(out, lists):
    """The losses, the counts and (with a dump) the three lists of a training call's result."""
    res = {k: float(getattr(out, k)) for k in LOSS_KEYS}
    res.update({k: int(getattr(out, k)) for k in ("num_pos", "num_neg", "total_pos", "total_neg", "masked_mid", "masked_end", "flags")})
    if lists is not None:
        res.update(pos_input_idx=lists[0][:out.num_pos].copy(), pos_target_idx=lists[1][:out.num_pos].copy(),
                   neg_input_idx=lists[2][:out.num_neg].copy())
    return res



def forward_losses(ctx, img, gt_boxes, gt_labels, forced_pos=None, forced_neg=None, dump=False, on_device=False, **opts):
    """The validation losses of one image (dc_forward_losses; docs/SEMANTICS.md, "Validation losses") on a ctx with weights
    loaded.  img: (3,H,W) float32 host array, or with on_device an ops.DeviceArray; gt_boxes (G,4) xcycwh in the resized frame;
    gt_labels (G,L) int32, words then zeros.  Returns a dict with the reference's six keys (float), the sampler's counts
    (num_pos, num_neg, total_pos, total_neg, masked_mid, masked_end, flags) and, with dump, its three index lists."""
    args, out, lists, _hw, _cap, _keep = _train_args("forward_losses", ctx, img, gt_boxes, gt_labels, forced_pos, forced_neg, dump,
                                                    on_device, opts)
    check(ctx.h, ctx.lib.dc_forward_losses(*args), "dc_forward_losses")
    return _train_result(out, lists)



def check_localize_args(nms_thresh, max_regions, min_objectness):
    """The rules of dc_localize_opts (docs/SEMANTICS.md, "Localising phrases"), checked before the library is called: nms_thresh
    in [0, 1], max_regions an integer in 1..4096, min_objectness None (= every proposal) or a number that is not NaN.  Returns
    the filled DcLocalizeOpts."""
    t = float(np.float32(nms_thresh))
    if not 0.0 <= t <= 1.0:                                   # NaN fails
        raise ValueError("nms_thresh must be in [0, 1] (got %r)" % (nms_thresh,))
    M = int(max_regions)
    if M != max_regions or not 1 <= M <= 4096:
        raise ValueError("max_regions must be an integer in 1..4096 (got %r)" % (max_regions,))
    lo = float("-inf") if min_objectness is None else float(np.float32(min_objectness))
    if lo != lo:
        raise ValueError("min_objectness must not be NaN")
    return _lib.DcLocalizeOpts(t, M, lo)


def bilinear_roi_pool(ctx, feat_chw, boxes, img_h, img_w, HH=7, WW=7, out_layout=0):
    """nn.BilinearRoiPooling forward: (C,h,w)+(B,4) -> (B,C,HH,WW) [layout 0] or (B,HH,WW,C) [1]."""
    f = _f32(feat_chw); b = _f32(boxes)
    C_, h, w = f.shape
    fd = ctx.to_device(np.ascontiguousarray(f.transpose(1, 2, 0))); bd = ctx.to_device(b)
    B = b.shape[0]
    o = ctx.empty((B, C_, HH, WW) if out_layout == 0 else (B, HH, WW, C_))
    check(ctx.h, ctx.lib.dc_op_bilinear_roi_pool(ctx.h, fd.ptr, h, w, C_, bd.ptr, B, img_h, img_w, HH, WW, o.ptr,
                                                 out_layout), "dc_op_bilinear_roi_pool")
    return o.numpy()


# ---- language model -------------------------------------------------------------------------------
def lm_score(ctx, codes, queries):
    """Teacher-forced log p(query | code) with the ctx's loaded language model (dc_op_lm_score): codes (n, fc_dim),
    queries (Q, Tq) int 1-based word ids, zero-padded -> loglik (n, Q) float32."""
    x = _f32(codes)
    q = np.ascontiguousarray(queries, dtype=np.int32)
    if q.ndim != 2:
        raise ValueError("queries must be (Q, Tq)")
    n = x.shape[0]
    Q, Tq = q.shape
    xd = ctx.to_device(x); qd = ctx.to_device(q)
    o = ctx.empty((n, max(Q, 1)))
    check(ctx.h, ctx.lib.dc_op_lm_score(ctx.h, xd.ptr, n, qd.ptr, Q, Tq, o.ptr), "dc_op_lm_score")
    return o.numpy()


LM_GRAD_KEYS = ("lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b", "codes")


def lm_grad(ctx, codes, labels, weight=1.0, want_codes=True):
    """The captioning loss of n (code, caption) pairs and its gradients (dc_op_lm_grad; docs/SEMANTICS.md, "Language-model
    gradients") with the ctx's loaded language model.  codes (n, fc_dim); labels (n, L) int, words in [1, V] then zeros.
    Returns a dict: the seven language-model tensors' gradients in checkpoint layouts and `codes` (n, fc_dim) as numpy arrays,
    `loss` (float) and `rowlik` (n,) float64, every row's caption log-likelihood."""
    dims = getattr(ctx, "lm_dims", None)
    if dims is None:
        raise _lib.DenseCapError("ops.lm_grad: the ctx carries no model dimensions (build a DenseCapModel on it first)")
    E, Hd, D, V = dims["E"], dims["Hd"], dims["D"], dims["V"]
    x = _f32(codes)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if x.ndim != 2 or x.shape[1] != D:
        raise ValueError("codes must be (n, %d), got %r" % (D, x.shape))
    if lab.ndim != 2 or lab.shape[0] != x.shape[0]:
        raise ValueError("labels must be (n, L) with one row per code, got %r for %d codes" % (lab.shape, x.shape[0]))
    n, L = lab.shape
    shapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
              "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (n, D)}
    xd = ctx.to_device(x)
    bufs = {k: ctx.empty(shapes[k]) for k in LM_GRAD_KEYS if want_codes or k != "codes"}
    g = _lib.DcLmGrads(**{k: b.ptr for k, b in bufs.items()})
    loss = C.c_double(0.0)
    rowlik = np.zeros((max(n, 1),), np.float64)
    check(ctx.h, ctx.lib.dc_op_lm_grad(ctx.h, xd.ptr, n, lab.ctypes.data, L, float(weight), C.byref(g), C.byref(loss),
                                       rowlik.ctypes.data), "dc_op_lm_grad")
    out = {k: b.numpy() for k, b in bufs.items()}
    out["loss"] = float(loss.value)
    out["rowlik"] = rowlik[:n]
    return out


def lm_grad_stage_ms(ctx):
    """The library's own event split of the last lm_grad call, in ms: forward, loop back through the steps, stacked
    gradients, embedding and codes rows."""
    ms = np.zeros(4, np.float32)
    check(ctx.h, ctx.lib.dc_debug_lm_grad_stage_ms(ctx.h, ms.ctypes.data_as(_lib.c_float_p)), "dc_debug_lm_grad_stage_ms")
    return dict(zip(("forward", "bptt", "stacked", "rows"), (float(v) for v in ms)))


# ---- recognition-net gradients (docs/SEMANTICS.md, "Recognition-net gradients") ---------------------------------------------------
RECOG_GRAD_KEYS = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b", "feat", "roi_boxes")


def feature_size(ctx, H, W):
    """(h, w) of the trunk's output map for an H x W image (dc_feature_size)."""
    h, w = C.c_int(0), C.c_int(0)
    check(ctx.h, ctx.lib.dc_feature_size(int(H), int(W), C.byref(h), C.byref(w)), "dc_feature_size")
    return h.value, w.value


def roi_pool_grad(ctx, feat_chw, boxes, img_h, img_w, dout, HH=7, WW=7, want_boxes=True):
    """nn.BilinearRoiPooling backward (dc_op_roi_pool_grad): feat (C,h,w), boxes (B,4) xcycwh, dout (B,C,HH,WW) in the reference's
    layout -> (dfeat (C,h,w), dboxes (B,4) or None)."""
    f = _f32(feat_chw); b = _f32(boxes).reshape(-1, 4); d = _f32(dout)
    C_, h, w = f.shape
    B = b.shape[0]
    if d.shape != (B, C_, HH, WW):
        raise ValueError("dout must be (B, C, HH, WW) = %r, got %r" % ((B, C_, HH, WW), d.shape))
    fd = ctx.to_device(np.ascontiguousarray(f.transpose(1, 2, 0))); bd = ctx.to_device(b)
    dd = ctx.to_device(np.ascontiguousarray(d.transpose(0, 2, 3, 1)))
    df = ctx.empty((h, w, C_)); db = ctx.empty((B, 4)) if want_boxes else None
    check(ctx.h, ctx.lib.dc_op_roi_pool_grad(ctx.h, fd.ptr, h, w, C_, bd.ptr, B, int(img_h), int(img_w), HH, WW, dd.ptr, df.ptr,
                                             db.ptr if want_boxes else None), "dc_op_roi_pool_grad")
    return np.ascontiguousarray(df.numpy().transpose(2, 0, 1)), (db.numpy() if want_boxes else None)


def roi_tap_index(ctx, boxes, h, w, img_h, img_w, HH=7, WW=7):
    """The tap list and the inverted index alone (dc_debug_roi_tap_index): (tap_pix (T,), tap_w (T,), start (h*w+1,), list
    (start[-1],)) for T = B*HH*WW*4 taps, tap id = (row*HH*WW + point)*4 + k."""
    b = _f32(boxes).reshape(-1, 4)
    B = b.shape[0]
    T = B * HH * WW * 4
    bd = ctx.to_device(b)
    tp = ctx.empty((T,), np.int32); tw = ctx.empty((T,)); st = ctx.empty((h * w + 1,), np.int32); li = ctx.empty((T,), np.int32)
    check(ctx.h, ctx.lib.dc_debug_roi_tap_index(ctx.h, bd.ptr, B, int(h), int(w), int(img_h), int(img_w), HH, WW, tp.ptr, tw.ptr,
                                                st.ptr, li.ptr), "dc_debug_roi_tap_index")
    start = st.numpy()
    return tp.numpy(), tw.numpy(), start, li.numpy()[:start[-1]]


def end_crit_grad(ctx, obj, trans, anchors, target, num_pos, w_obj=0.1, w_box=0.1):
    """The two end criteria's gradients alone (dc_debug_end_crit_grad): obj (n,), trans (n,4), anchors (n,4), target (num_pos,4)
    -> (dobj (n,), dtrans (num_pos,4), danchor (num_pos,4), masked)."""
    obj = _f32(obj).reshape(-1)
    n, np_ = len(obj), int(num_pos)
    d = [ctx.to_device(_f32(a)) for a in (obj, np.reshape(trans, (n, 4)), np.reshape(anchors, (n, 4)))]
    td = ctx.to_device(_f32(target).reshape(-1, 4)) if np_ > 0 else None
    do = ctx.empty((n,)); dt = ctx.empty((max(np_, 1), 4)); da = ctx.empty((max(np_, 1), 4)); m = ctx.empty((1,), np.int32)
    check(ctx.h, ctx.lib.dc_debug_end_crit_grad(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, td.ptr if td is not None else None, n, np_,
                                                float(w_obj), float(w_box), do.ptr, dt.ptr, da.ptr, m.ptr), "dc_debug_end_crit_grad")
    return do.numpy(), dt.numpy()[:np_], da.numpy()[:np_], int(m.numpy()[0])


def heads_bwd(ctx, codes, w5, dobj, dtrans, g=None):
    """The recognition heads' backward alone (dc_debug_heads_bwd): codes (n,D), w5 (5,D), dobj (n,), dtrans (num_pos,4), g
    (num_pos,D) or None -> (dcodes (n,D), dw5 (5,D), db5 (5,))."""
    x = _f32(codes)
    n, D = x.shape
    dt = _f32(dtrans).reshape(-1, 4)
    np_ = len(dt)
    xd = ctx.to_device(x); wd = ctx.to_device(_f32(w5).reshape(5, D)); od = ctx.to_device(_f32(dobj).reshape(n))
    td = ctx.to_device(dt if np_ else np.zeros((1, 4), np.float32))
    gd = ctx.to_device(_f32(g).reshape(np_, D)) if g is not None and np_ else None
    dc = ctx.empty((n, D)); dw = ctx.empty((5, D)); db = ctx.empty((5,))
    check(ctx.h, ctx.lib.dc_debug_heads_bwd(ctx.h, xd.ptr, wd.ptr, od.ptr, td.ptr, gd.ptr if gd is not None else None, n, np_, D,
                                            dc.ptr, dw.ptr, db.ptr), "dc_debug_heads_bwd")
    return dc.numpy(), dw.numpy(), db.numpy()


def permute_fc6_back(ctx, x, C_, HW):
    """(N, HW*C) with k' = p*C + c -> (N, C*HW) with k = c*HW + p (dc_debug_permute_fc6_back)."""
    x = _f32(x)
    N = x.shape[0]
    xd = ctx.to_device(x); o = ctx.empty((N, C_ * HW))
    check(ctx.h, ctx.lib.dc_debug_permute_fc6_back(ctx.h, xd.ptr, o.ptr, N, int(C_), int(HW)), "dc_debug_permute_fc6_back")
    return o.numpy()


def recog_grad_stage_ms(ctx):
    """The library's own event split of the last recognition backward, in ms."""
    ms = np.zeros(4, np.float32)
    check(ctx.h, ctx.lib.dc_debug_recog_grad_stage_ms(ctx.h, ms.ctypes.data_as(_lib.c_float_p)), "dc_debug_recog_grad_stage_ms")
    return dict(zip(("heads_fc", "dpool", "roi_scatter", "roi_boxes"), (float(v) for v in ms)))


def _recog_bufs(ctx, D, h, w, rows):
    shapes = {"fc6_w": (D, 512 * 49), "fc6_b": (D,), "fc7_w": (D, D), "fc7_b": (D,), "obj_w": (1, D), "obj_b": (1,),
              "boxreg_w": (4, D), "boxreg_b": (4,), "feat": (h, w, 512), "roi_boxes": (max(rows, 1), 4)}
    return {k: ctx.empty(shapes[k]) for k in RECOG_GRAD_KEYS}


def _recog_out(bufs, n):
    out = {k: b.numpy() for k, b in bufs.items()}
    out["feat"] = np.ascontiguousarray(out["feat"].transpose(2, 0, 1))           # (512, h, w), the reference's layout
    out["roi_boxes"] = out["roi_boxes"][:n]
    return out


def recog_grad(ctx, feat_chw, roi_boxes, num_pos, target_boxes, img_h, img_w, dcodes=None, **opts):
    """The recognition net's gradients on given rows (dc_op_recog_grad; docs/SEMANTICS.md, "Recognition-net gradients") with the
    ctx's loaded weights.  feat (512,h,w); roi_boxes (n,4), positives first; target_boxes (num_pos,4); dcodes (num_pos,fc_dim) or
    None.  Returns a dict: the eight parameter gradients in checkpoint layouts, feat (512,h,w), roi_boxes (n,4),
    end_objectness_loss, end_box_reg_loss (float) and masked_end."""
    dims = getattr(ctx, "lm_dims", None)
    if dims is None:
        raise _lib.DenseCapError("ops.recog_grad: the ctx carries no model dimensions (build a DenseCapModel on it first)")
    D = dims["D"]
    f = _f32(feat_chw); b = _f32(roi_boxes).reshape(-1, 4)
    n, np_ = len(b), int(num_pos)
    if f.ndim != 3 or f.shape[0] != 512:
        raise ValueError("feat must be (512, h, w), got %r" % (f.shape,))
    h, w = f.shape[1:]
    o = loss_opts(**opts)
    fd = ctx.to_device(np.ascontiguousarray(f.transpose(1, 2, 0))); bd = ctx.to_device(b)
    td = ctx.to_device(_f32(target_boxes).reshape(np_, 4)) if np_ > 0 else None
    gd = ctx.to_device(_f32(dcodes).reshape(np_, D)) if dcodes is not None and np_ > 0 else None
    bufs = _recog_bufs(ctx, D, h, w, n)
    g = _lib.DcRecogGrads(**{k: v.ptr for k, v in bufs.items()})
    lo, lb, m = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    check(ctx.h, ctx.lib.dc_op_recog_grad(ctx.h, fd.ptr, h, w, bd.ptr, n, np_, td.ptr if td is not None else None,
                                          gd.ptr if gd is not None else None, int(img_h), int(img_w), C.byref(o), C.byref(g),
                                          C.byref(lo), C.byref(lb), C.byref(m)), "dc_op_recog_grad")
    out = _recog_out(bufs, n)
    out.update(end_objectness_loss=float(lo.value), end_box_reg_loss=float(lb.value), masked_end=int(m.value))
    return out


def _grad_bufs(ctx, dims, h, w, cap):
    """Device buffers of the recognition and language-model gradients for up to cap rows, and the two structs over them."""
    E, Hd, D, V = dims["E"], dims["Hd"], dims["D"], dims["V"]
    rbufs = _recog_bufs(ctx, D, h, w, cap)
    lshapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
               "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (cap, D)}
    lbufs = {k: ctx.empty(lshapes[k]) for k in LM_GRAD_KEYS}
    rg = _lib.DcRecogGrads(**{k: v.ptr for k, v in rbufs.items()})
    return rbufs, lbufs, rg, _lib.DcLmGrads(**{k: v.ptr for k, v in lbufs.items()})


def _grad_out(ctx, out, rbufs, lbufs, D):
    """The host arrays of _grad_bufs after a call that sampled out.num_pos + out.num_neg rows."""
    n = out.num_pos + out.num_neg
    if n == 0:
        rbufs["roi_boxes"] = ctx.to_device(np.zeros((1, 4), np.float32))
    res = _recog_out(rbufs, n)
    res.update({k: b.numpy() for k, b in lbufs.items()})
    res["codes"] = res["codes"][:out.num_pos] if out.num_pos > 0 else np.zeros((0, D), np.float32)
    return res



def loss_gradients(ctx, img, gt_boxes, gt_labels, forced_pos=None, forced_neg=None, dump=False, on_device=False, **opts):
    """dc_loss_gradients: the losses of forward_losses (same arguments, same numbers) and the gradient of end_objectness +
    end_box_reg + captioning with respect to every parameter downstream of the RPN.  Returns forward_losses' dict plus the eight
    recognition and seven language-model parameter gradients in checkpoint layouts, `codes` (num_pos, fc_dim) -- the language
    model's gradient of the positive codes --, `feat` (512,h,w) -- RoI pooling's share of the feature map's gradient -- and
    `roi_boxes` (num_pos + num_neg, 4)."""
    dims = getattr(ctx, "lm_dims", None)
    if dims is None:
        raise _lib.DenseCapError("ops.loss_gradients: the ctx carries no model dimensions (build a DenseCapModel on it first)")
    args, out, lists, (H, W), cap, _keep = _train_args("loss_gradients", ctx, img, gt_boxes, gt_labels, forced_pos, forced_neg, dump,
                                                      on_device, opts)
    h, w = feature_size(ctx, H, W)
    rbufs, lbufs, rg, lg = _grad_bufs(ctx, dims, h, w, cap)
    check(ctx.h, ctx.lib.dc_loss_gradients(*args, C.byref(rg), C.byref(lg)), "dc_loss_gradients")
    res = _train_result(out, lists)
    res.update(_grad_out(ctx, out, rbufs, lbufs, dims["D"]))
    return res



def wgrad(ctx, A, B):
    """The weight-gradient kernel alone (dc_debug_wgrad): A (M, N), B (M, K) -> A^T B (N, K)."""
    A = _f32(A); B = _f32(B)
    (M, N), K = A.shape, B.shape[1]
    ad = ctx.to_device(A); bd = ctx.to_device(B)
    o = ctx.empty((N, K))
    check(ctx.h, ctx.lib.dc_debug_wgrad(ctx.h, ad.ptr, bd.ptr, M, N, K, o.ptr), "dc_debug_wgrad")
    return o.numpy()


def embed_segsum(ctx, dx, tok, rows_out):
    """The embedding segment sum alone (dc_debug_embed_segsum): dx (count, E), tok (count,) 1-based -> (rows_out, E)."""
    dx = _f32(dx)
    tok = np.ascontiguousarray(tok, dtype=np.int32)
    d = ctx.to_device(dx)
    o = ctx.empty((rows_out, dx.shape[1]))
    check(ctx.h, ctx.lib.dc_debug_embed_segsum(ctx.h, d.ptr, tok.ctypes.data, len(tok), dx.shape[1], int(rows_out), o.ptr),
          "dc_debug_embed_segsum")
    return o.numpy()


def softmax_grad(ctx, logits, tgt, scale, V1=None):
    """The softmax cross-entropy gradient rows alone (dc_debug_softmax_grad): logits (rows, ld) with V1 <= ld real columns, tgt
    (rows,) 1-based -> ((rows, ld) gradient rows, (rows,) float64 log-sum-exp)."""
    x = _f32(logits)
    rows, ld = x.shape
    V1 = ld if V1 is None else int(V1)
    xd = ctx.to_device(x); td = ctx.to_device(np.ascontiguousarray(tgt, dtype=np.int32))
    lse = ctx.empty((rows,), np.float64)
    check(ctx.h, ctx.lib.dc_debug_softmax_grad(ctx.h, xd.ptr, rows, V1, ld, td.ptr, float(scale), lse.ptr), "dc_debug_softmax_grad")
    return xd.numpy(), lse.numpy()


def lstm_cell_bwd(ctx, gates_pre, c_prev, c, dh, dc):
    """The LSTM cell backward alone (dc_debug_lstm_cell_bwd): gates_pre (rows, 4Hd) in gate order i,f,o,g; the rest (rows, Hd)
    -> (dgates (rows, 4Hd), dc_prev (rows, Hd))."""
    g = _f32(gates_pre)
    rows, Hd = g.shape[0], g.shape[1] // 4
    d = [ctx.to_device(_f32(a)) for a in (g, c_prev, c, dh, dc)]
    dg = ctx.empty((rows, 4 * Hd)); dcp = ctx.empty((rows, Hd))
    check(ctx.h, ctx.lib.dc_debug_lstm_cell_bwd(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, rows, Hd, dg.ptr, dcp.ptr),
          "dc_debug_lstm_cell_bwd")
    return dg.numpy(), dcp.numpy()


def wgrad_ld(ctx, A, B, N, K, C0):
    """The weight-gradient kernel with leading dimensions (dc_debug_wgrad_ld): A (M, lda) and B (M, ldb) of which the first N and
    K columns count, C0 (N, ldc) the output buffer's contents before the call -> the buffer after it (columns [K, ldc) untouched)."""
    A = _f32(A); B = _f32(B); C0 = _f32(C0)
    M = A.shape[0]
    if B.shape[0] != M or C0.shape[0] != N or A.shape[1] < N or B.shape[1] < K or C0.shape[1] < K:
        raise ValueError("wgrad_ld: shapes %r, %r, %r do not hold N = %d, K = %d" % (A.shape, B.shape, C0.shape, N, K))
    ad = ctx.to_device(A); bd = ctx.to_device(B); cd = ctx.to_device(C0)
    check(ctx.h, ctx.lib.dc_debug_wgrad_ld(ctx.h, ad.ptr, A.shape[1], bd.ptr, B.shape[1], M, int(N), int(K), cd.ptr, C0.shape[1]),
          "dc_debug_wgrad_ld")
    return cd.numpy()


def colsum(ctx, X, N):
    """The bias gradients' column sums alone (dc_debug_colsum): X (M, ldx) of which the first N columns count -> (N,)."""
    X = _f32(X)
    M, ldx = X.shape
    if ldx < N:
        raise ValueError("colsum: X has %d columns, N = %d" % (ldx, N))
    xd = ctx.to_device(X)
    o = ctx.empty((int(N),))
    check(ctx.h, ctx.lib.dc_debug_colsum(ctx.h, xd.ptr, ldx, M, int(N), o.ptr), "dc_debug_colsum")
    return o.numpy()


# ---- convolution gradients (docs/SEMANTICS.md, "Convolution gradients") ------------------------------------------------------------
def conv3x3_grad(ctx, x_chw, w_oihw, dy_chw, want=("dw", "db", "dx")):
    """The backward of nn.SpatialConvolution(Cin,Cout,3,3,1,1,1,1) on one map (dc_op_conv3x3_grad): x (Cin,h,w) the layer's input,
    w (Cout,Cin,3,3), dy (Cout,h,w) the gradient at its output -> a dict of the outputs named in `want`: dw (Cout,Cin,3,3), db
    (Cout,), dx (Cin,h,w).  x may be None when dw is not wanted, w when dx is not."""
    dy = _f32(dy_chw)
    Cout, h, w = dy.shape
    Cin = _f32(x_chw).shape[0] if x_chw is not None else _f32(w_oihw).shape[1]
    xd = ctx.to_device(np.ascontiguousarray(_f32(x_chw).transpose(1, 2, 0))) if x_chw is not None else None
    wd = ctx.to_device(_f32(w_oihw)) if w_oihw is not None else None
    dd = ctx.to_device(np.ascontiguousarray(dy.transpose(1, 2, 0)))
    shapes = {"dw": (Cout, Cin, 3, 3), "db": (Cout,), "dx": (h, w, Cin)}
    bufs = {k: ctx.empty(shapes[k]) for k in ("dw", "db", "dx") if k in want}
    ptr = lambda d: None if d is None else d.ptr
    check(ctx.h, ctx.lib.dc_op_conv3x3_grad(ctx.h, ptr(xd), ptr(wd), dd.ptr, h, w, Cin, Cout, ptr(bufs.get("dw")), ptr(bufs.get("db")),
                                            ptr(bufs.get("dx"))), "dc_op_conv3x3_grad")
    out = {k: b.numpy() for k, b in bufs.items()}
    if "dx" in out:
        out["dx"] = np.ascontiguousarray(out["dx"].transpose(2, 0, 1))
    return out


def conv3x3_wgrad(ctx, x_chw, dy_chw, slices=0):
    """The convolution's weight-gradient kernel alone (dc_debug_conv3x3_wgrad): x (Cin,h,w), dy (Cout,h,w) -> dw (Cout,Cin,3,3)
    with the pixels shared by `slices` slices per tile (0: the production choice)."""
    x = _f32(x_chw); dy = _f32(dy_chw)
    (Cin, h, w), Cout = x.shape, dy.shape[0]
    xd = ctx.to_device(np.ascontiguousarray(x.transpose(1, 2, 0))); dd = ctx.to_device(np.ascontiguousarray(dy.transpose(1, 2, 0)))
    o = ctx.empty((Cout, Cin, 3, 3))
    check(ctx.h, ctx.lib.dc_debug_conv3x3_wgrad(ctx.h, xd.ptr, dd.ptr, h, w, Cin, Cout, int(slices), o.ptr), "dc_debug_conv3x3_wgrad")
    return o.numpy()


# ---- CNN gradients (docs/SEMANTICS.md, "CNN gradients") -----------------------------------------------------------------------------
CNN_GRAD_CONVS = tuple(range(4, 13))          # conv3_1 .. conv5_3 as indices of the thirteen convolutions (weights.VGG16_CONVS)
CNN_GRAD_KEYS = tuple("conv_w%d" % i for i in CNN_GRAD_CONVS) + tuple("conv_b%d" % i for i in CNN_GRAD_CONVS)


def maxpool2x2_grad(ctx, y_nchw, dpool_nchw):
    """The backward of the ceil-mode 2x2/2 max pool fused with the mask of the ReLU in front of it (dc_op_maxpool2x2_grad):
    y (N,C,H,W) the map the pool read, dpool (N,C,ceil(H/2),ceil(W/2)) -> dy (N,C,H,W)."""
    y = _f32(y_nchw); g = _f32(dpool_nchw)
    N, C_, H, W = y.shape
    if g.shape != (N, C_, (H + 1) // 2, (W + 1) // 2):
        raise ValueError("maxpool2x2_grad: dpool has shape %s" % (g.shape,))
    yd = ctx.to_device(np.ascontiguousarray(y.transpose(0, 2, 3, 1))); gd = ctx.to_device(np.ascontiguousarray(g.transpose(0, 2, 3, 1)))
    o = ctx.empty((N, H, W, C_))
    check(ctx.h, ctx.lib.dc_op_maxpool2x2_grad(ctx.h, yd.ptr, gd.ptr, N, H, W, C_, o.ptr), "dc_op_maxpool2x2_grad")
    return np.ascontiguousarray(o.numpy().transpose(0, 3, 1, 2))


def relu_grad(ctx, y, dy):
    """dy where y > 0, +0.0 elsewhere (dc_op_relu_grad; the library works in place on its copy of dy): arrays of one shape."""
    y = _f32(y); dy = _f32(dy)
    if y.shape != dy.shape:
        raise ValueError("relu_grad: shapes %s and %s" % (y.shape, dy.shape))
    yd = ctx.to_device(y); dd = ctx.to_device(dy)
    check(ctx.h, ctx.lib.dc_op_relu_grad(ctx.h, yd.ptr, dd.ptr, int(y.size)), "dc_op_relu_grad")
    return dd.numpy()


# ---- Dropout (docs/SEMANTICS.md, "Dropout") ------------------------------------------------------------------------------------------
def dropout(ctx, x, layer, p, seed):
    """nn.Dropout's forward on a (rows, cols) matrix (dc_op_dropout; the library works in place on its copy of x): element
    (row, col) is kept, as x * (1 / (1 - p)), iff its Philox word of (seed, layer, row, col) is below floor((1 - p) 2^32), and
    is +0.0 otherwise."""
    x = _f32(x)
    if x.ndim != 2:
        raise ValueError("dropout: x has shape %s, a (rows, cols) matrix is needed" % (x.shape,))
    xd = ctx.to_device(x)
    check(ctx.h, ctx.lib.dc_op_dropout(ctx.h, xd.ptr, x.shape[0], x.shape[1], int(layer), float(p), int(seed) & (2 ** 64 - 1)),
          "dc_op_dropout")
    return xd.numpy()


def relu_dropout_grad(ctx, y, dy, p):
    """The backward of ReLU followed by an in-place Dropout, from the dropped activation y: dy * (1 / (1 - p)) where y > 0, +0.0
    elsewhere (dc_op_relu_dropout_grad; the library works in place on its copy of dy): arrays of one shape."""
    y = _f32(y); dy = _f32(dy)
    if y.shape != dy.shape:
        raise ValueError("relu_dropout_grad: shapes %s and %s" % (y.shape, dy.shape))
    yd = ctx.to_device(y); dd = ctx.to_device(dy)
    check(ctx.h, ctx.lib.dc_op_relu_dropout_grad(ctx.h, yd.ptr, dd.ptr, int(y.size), float(p)), "dc_op_relu_dropout_grad")
    return dd.numpy()


def cnn_shapes(h4, w4):
    """[(index of the convolution, h, w, Cin, Cout)] of conv3_1 .. conv5_3 on an (h4, w4) pool2 map, and conv5_3's map size."""
    from .weights import VGG16_CONVS
    out, h, w = [], int(h4), int(w4)
    for i in CNN_GRAD_CONVS:
        out.append((i, h, w) + tuple(VGG16_CONVS[i]))
        if i in (6, 9):                       # pool3 behind conv3_3, pool4 behind conv4_3
            h, w = (h + 1) // 2, (w + 1) // 2
    return out, (h, w)


def cnn_grad(ctx, x4_chw, dfeat_chw, want_x=True, dump=False):
    """The backward through conv3_1 .. conv5_3 with the ctx's loaded weights (dc_op_cnn_grad): x4 (128,h4,w4) the pool2 map,
    dfeat (512,h6,w6) the gradient at conv5_3's output -> {"conv_w4" .. "conv_w12" (Cout,Cin,3,3), "conv_b4" .. "conv_b12", "x"
    (128,h4,w4) if want_x}.  dump: also "act4" .. "act12" (the layers' inputs), "prepool6", "prepool9", "feat" and "dy4" .. "dy12"
    (the gradients at the convolutions' outputs after the mask), all CHW."""
    x = _f32(x4_chw); g = _f32(dfeat_chw)
    _, h4, w4 = x.shape
    layers, (fh, fw) = cnn_shapes(h4, w4)
    if x.shape[0] != 128 or g.shape != (512, fh, fw):
        raise ValueError("cnn_grad: x4 %s, dfeat %s (want (128, h4, w4) and (512, %d, %d))" % (x.shape, g.shape, fh, fw))
    xd = ctx.to_device(np.ascontiguousarray(x.transpose(1, 2, 0))); gd = ctx.to_device(np.ascontiguousarray(g.transpose(1, 2, 0)))
    bufs, cg, cd = {}, _lib.DcCnnGrads(), _lib.DcCnnDump()
    for j, (i, h, w, cin, cout) in enumerate(layers):
        bufs["conv_w%d" % i] = ctx.empty((cout, cin, 3, 3)); bufs["conv_b%d" % i] = ctx.empty((cout,))
        cg.conv_w[j] = bufs["conv_w%d" % i].ptr.value; cg.conv_b[j] = bufs["conv_b%d" % i].ptr.value
        if dump:
            bufs["act%d" % i] = ctx.empty((h, w, cin)); bufs["dy%d" % i] = ctx.empty((h, w, cout))
            cd.act[j] = bufs["act%d" % i].ptr.value; cd.dy[j] = bufs["dy%d" % i].ptr.value
            if i in (6, 9):
                bufs["prepool%d" % i] = ctx.empty((h, w, cout))
                cd.prepool[0 if i == 6 else 1] = bufs["prepool%d" % i].ptr.value
    if dump:
        bufs["feat"] = ctx.empty((fh, fw, 512)); cd.feat = bufs["feat"].ptr.value
    if want_x:
        bufs["x"] = ctx.empty((h4, w4, 128)); cg.x = bufs["x"].ptr.value
    check(ctx.h, ctx.lib.dc_op_cnn_grad(ctx.h, xd.ptr, h4, w4, gd.ptr, C.byref(cg), C.byref(cd) if dump else None), "dc_op_cnn_grad")
    out = {k: b.numpy() for k, b in bufs.items()}
    return {k: (np.ascontiguousarray(a.transpose(2, 0, 1)) if a.ndim == 3 else a) for k, a in out.items()}


def cnn_grad_ms(ctx):
    """(kept-activation forward, backward) in ms of the last dc_op_cnn_grad, from the library's own events."""
    ms = np.zeros(2, np.float32)
    n = ctx.lib.dc_debug_fetch(ctx.h, b"cnn_grad_ms", ms.ctypes.data, ms.nbytes)
    check(ctx.h, int(n), "dc_debug_fetch cnn_grad_ms")
    return float(ms[0]), float(ms[1])


# ---- RPN gradients (docs/SEMANTICS.md, "RPN gradients") -----------------------------------------------------------------------------
RPN_GRAD_KEYS = ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b", "feat")
BOX_REG_DECAY = 5e-5               # train_opts.lua:42


def _rpn_bufs(ctx, k, R, h, w):
    shapes = {"rpn_conv_w": (R, 512, 3, 3), "rpn_conv_b": (R,), "rpn_box_w": (4 * k, R, 1, 1), "rpn_box_b": (4 * k,),
              "rpn_score_w": (2 * k, R, 1, 1), "rpn_score_b": (2 * k,), "feat": (h, w, 512)}
    return {n: ctx.empty(shapes[n]) for n in RPN_GRAD_KEYS}


def _rpn_dims(ctx, who):
    dims = getattr(ctx, "lm_dims", None)
    if dims is None or "k" not in dims:
        raise _lib.DenseCapError("ops.%s: the ctx carries no model dimensions (build a DenseCapModel on it first)" % who)
    return dims["k"], dims["R"]


def rpn_grad_kept(ctx, pixels=None):
    """What the last RPN backward left (dc_debug_rpn_grad_kept): (feat_rpn (512, h*w) or None, the library's event split in ms)."""
    ms = np.zeros(4, np.float32)
    f = ctx.empty((pixels, 512)) if pixels else None
    check(ctx.h, ctx.lib.dc_debug_rpn_grad_kept(ctx.h, f.ptr if f is not None else None, int(pixels or 0),
                                                ms.ctypes.data_as(_lib.c_float_p)), "dc_debug_rpn_grad_kept")
    return (f.numpy() if f is not None else None), dict(zip(("dheads", "heads", "conv_wgrad", "conv_dgrad"), (float(v) for v in ms)))


def rpn_grad(ctx, feat_chw, pos_input_idx, pos_target_idx, neg_input_idx, gt_boxes, img_h, img_w, droi_boxes=None,
             box_reg_decay=BOX_REG_DECAY, **opts):
    """The RPN's gradients on given lists (dc_op_rpn_grad; docs/SEMANTICS.md, "RPN gradients") with the ctx's loaded weights.
    feat (512,h,w); the three lists as forward_losses dumps them; gt_boxes (G,4); droi_boxes (num_pos + num_neg, 4) or None.
    Returns a dict: the six RPN tensors' gradients in checkpoint layouts, feat (512,h,w) -- the RPN's share --,
    mid_objectness_loss, mid_box_reg_loss (float) and masked_mid."""
    k, R = _rpn_dims(ctx, "rpn_grad")
    f = _f32(feat_chw)
    if f.ndim != 3 or f.shape[0] != 512:
        raise ValueError("feat must be (512, h, w), got %r" % (f.shape,))
    h, w = f.shape[1:]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    pi, pt, ni = i32(pos_input_idx), i32(pos_target_idx), i32(neg_input_idx)
    if len(pi) != len(pt):
        raise ValueError("rpn_grad: pos_input_idx and pos_target_idx differ in length")
    g = _f32(gt_boxes).reshape(-1, 4)
    n = len(pi) + len(ni)
    o = loss_opts(**opts)
    fd = ctx.to_device(np.ascontiguousarray(f.transpose(1, 2, 0))); gd = ctx.to_device(g)
    dev = lambda a: ctx.to_device(a) if len(a) else None
    pid, ptd, nid = dev(pi), dev(pt), dev(ni)
    dd = ctx.to_device(_f32(droi_boxes).reshape(n, 4)) if droi_boxes is not None and n > 0 else None
    ptr = lambda d: None if d is None else d.ptr
    bufs = _rpn_bufs(ctx, k, R, h, w)
    pg = _lib.DcRpnGrads(**{name: b.ptr for name, b in bufs.items()})
    lo, lb, m = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    check(ctx.h, ctx.lib.dc_op_rpn_grad(ctx.h, fd.ptr, h, w, ptr(pid), ptr(ptd), len(pi), ptr(nid), len(ni), gd.ptr, len(g), ptr(dd),
                                        int(img_h), int(img_w), C.byref(o), float(box_reg_decay), C.byref(pg), C.byref(lo),
                                        C.byref(lb), C.byref(m)), "dc_op_rpn_grad")
    out = {name: b.numpy() for name, b in bufs.items()}
    out["feat"] = np.ascontiguousarray(out["feat"].transpose(2, 0, 1))
    out.update(mid_objectness_loss=float(lo.value), mid_box_reg_loss=float(lb.value), masked_mid=int(m.value))
    return out


def forward_backward(ctx, img, gt_boxes, gt_labels, box_reg_decay=BOX_REG_DECAY, forced_pos=None, forced_neg=None, dump=False,
                     on_device=False, cnn=False, **opts):
    """dc_forward_backward: loss_gradients (same arguments, the same numbers) and the RPN's gradients.  Returns loss_gradients'
    dict plus the six RPN tensors, `feat_rpn` and `feat_roi` (512,h,w) -- the RPN's and RoI pooling's shares of the feature map's
    gradient -- with `feat` now their sum, the complete grad_cnn_features.  cnn=True (dc_forward_backward_cnn): the same dict bit
    for bit, plus CNN_GRAD_KEYS, the backward of `feat` through conv5_3 .. conv3_1 on activations the forward kept."""
    dims = getattr(ctx, "lm_dims", None)
    k, R = _rpn_dims(ctx, "forward_backward")
    args, out, lists, (H, W), cap, _keep = _train_args("forward_backward", ctx, img, gt_boxes, gt_labels, forced_pos, forced_neg, dump,
                                                      on_device, opts)
    h, w = feature_size(ctx, H, W)
    rbufs, lbufs, rg, lg = _grad_bufs(ctx, dims, h, w, cap)
    pbufs = _rpn_bufs(ctx, k, R, h, w)
    pg = _lib.DcRpnGrads(**{n: v.ptr for n, v in pbufs.items()})
    cbufs = {}
    if cnn:
        layers, _ = cnn_shapes(*cnn_input_size(H, W))
        cg = _lib.DcCnnGrads()
        for j, (i, _h, _w, cin, cout) in enumerate(layers):
            cbufs["conv_w%d" % i] = ctx.empty((cout, cin, 3, 3)); cbufs["conv_b%d" % i] = ctx.empty((cout,))
            cg.conv_w[j] = cbufs["conv_w%d" % i].ptr.value; cg.conv_b[j] = cbufs["conv_b%d" % i].ptr.value
        check(ctx.h, ctx.lib.dc_forward_backward_cnn(*args, C.byref(rg), C.byref(lg), float(box_reg_decay), C.byref(pg), C.byref(cg)),
              "dc_forward_backward_cnn")
    else:
        check(ctx.h, ctx.lib.dc_forward_backward(*args, C.byref(rg), C.byref(lg), float(box_reg_decay), C.byref(pg)),
              "dc_forward_backward")
    res = _train_result(out, lists)
    res.update(_grad_out(ctx, out, rbufs, lbufs, dims["D"]))
    res["feat_roi"] = res["feat"]
    res.update({n: b.numpy() for n, b in pbufs.items() if n != "feat"})
    res["feat"] = np.ascontiguousarray(pbufs["feat"].numpy().transpose(2, 0, 1))
    share, _ms = rpn_grad_kept(ctx, h * w)
    res["feat_rpn"] = np.ascontiguousarray(share.reshape(h, w, 512).transpose(2, 0, 1))
    res.update({n: b.numpy() for n, b in cbufs.items()})
    return res


def cnn_input_size(H, W):
    """(h4, w4) of the pool2 map of an H x W image (two ceil-mode 2x2 pools)."""
    return ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2


def cnn_kept(ctx, H, W):
    """What the last forward_backward(cnn=True) of an H x W image kept (dc_debug_fetch "cnn_x4" / "cnn_feat"): the pool2 map
    (128, h4, w4) and conv5_3's map (512, h, w)."""
    h4, w4 = cnn_input_size(H, W)
    _, (fh, fw) = cnn_shapes(h4, w4)
    out = []
    for key, shape in ((b"cnn_x4", (h4, w4, 128)), (b"cnn_feat", (fh, fw, 512))):
        a = np.zeros(shape, np.float32)
        check(ctx.h, int(ctx.lib.dc_debug_fetch(ctx.h, key, a.ctypes.data, a.nbytes)), "dc_debug_fetch %s" % key.decode())
        out.append(np.ascontiguousarray(a.transpose(2, 0, 1)))
    return tuple(out)

# ---- the training step (docs/SEMANTICS.md, "Training step") -----------------------------------------------------------------------
TRAIN_DEFAULTS = dict(learning_rate=1e-5, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=1e-6)      # train_opts.lua


def train_opts(**kw):
    """A filled DcTrainOpts (train_opts.lua's defaults).  Unknown keys raise; the library checks the values."""
    unknown = set(kw) - set(TRAIN_DEFAULTS)
    if unknown:
        raise ValueError("unknown training option(s): %s" % ", ".join(sorted(unknown)))
    o = dict(TRAIN_DEFAULTS, **kw)
    return _lib.DcTrainOpts(*[float(o[k]) for k in ("learning_rate", "beta1", "beta2", "epsilon", "weight_decay")])


def adam(ctx, p, g, m, v, t, offset=0, guard=8, **opts):
    """The Adam kernel alone (dc_op_adam) on copies of the float32 vectors p, g, m, v: step t >= 1.  offset: floats by which
    every buffer is shifted off its 16-byte aligned allocation; guard: floats of a known pattern kept on both sides of every
    buffer.  Returns (p, m, v, g_after, guards_intact)."""
    arrs = [_f32(a).reshape(-1) for a in (p, g, m, v)]
    n = len(arrs[0])
    if any(len(a) != n for a in arrs):
        raise ValueError("adam: p, g, m, v differ in length")
    o = train_opts(**opts)
    pad = np.float32(-7.25)
    bufs = []
    for a in arrs:
        host = np.full(offset + guard + n + guard, pad, np.float32)
        host[offset + guard:offset + guard + n] = a
        bufs.append(ctx.to_device(host))
    at = lambda b: C.c_void_p(b.ptr.value + 4 * (offset + guard))
    check(ctx.h, ctx.lib.dc_op_adam(ctx.h, at(bufs[0]), at(bufs[1]), at(bufs[2]), at(bufs[3]), n, int(t), C.byref(o)), "dc_op_adam")
    outs = [b.numpy() for b in bufs]
    body = lambda h: h[offset + guard:offset + guard + n].copy()
    intact = all((h[:offset + guard] == pad).all() and (h[offset + guard + n:] == pad).all() for h in outs)
    return body(outs[0]), body(outs[2]), body(outs[3]), body(outs[1]), intact


def adam_multi(ctx, segments, t, grid=0, **opts):
    """dc_debug_adam_multi: `segments` is a list of (p, g, m, v) float32 vectors, updated in ONE launch as dc_train_step issues
    it.  Returns the list of (p, m, v) after the step."""
    o = train_opts(**opts)
    dev = [[ctx.to_device(_f32(a).reshape(-1)) for a in seg] for seg in segments]
    ns = len(dev)
    cols = [(C.c_void_p * ns)(*[d[j].ptr for d in dev]) for j in range(4)]
    sizes = (C.c_size_t * ns)(*[d[0].shape[0] for d in dev])
    check(ctx.h, ctx.lib.dc_debug_adam_multi(ctx.h, cols[0], cols[1], cols[2], cols[3], sizes, ns, int(t), C.byref(o), int(grid)),
          "dc_debug_adam_multi")
    return [(d[0].numpy(), d[2].numpy(), d[3].numpy()) for d in dev]


def screen_operands(ctx, W):
    """dc_debug_screen_operands on W (V1, Hd) float32: (wb (V1pad, Kp) uint16 bf16 bits, wn (V1pad) uint16 fp16 bits) with the
    padding the library uses (screen_pads)."""
    W = _f32(W)
    V1, Hd = W.shape
    V1pad, Kp = (V1 + 63) // 64 * 64, (Hd + 63) // 64 * 64
    wd = ctx.to_device(W)
    wb = ctx.to_device(np.full((V1pad, Kp), 0xAAAA, np.uint16)); wn = ctx.to_device(np.full((V1pad,), 0xAAAA, np.uint16))
    check(ctx.h, ctx.lib.dc_debug_screen_operands(ctx.h, wd.ptr, V1, Hd, V1pad, Kp, wb.ptr, wn.ptr), "dc_debug_screen_operands")
    return wb.numpy(), wn.numpy()


def unpack_conv3x3(ctx, w_packed, Cout, Cin):
    """dc_debug_unpack_conv3x3: (Cout, 9 Cin) packed -> (Cout, Cin, 3, 3)."""
    wd = ctx.to_device(_f32(w_packed).reshape(Cout, 9 * Cin))
    out = ctx.empty((Cout, Cin, 3, 3))
    check(ctx.h, ctx.lib.dc_debug_unpack_conv3x3(ctx.h, wd.ptr, out.ptr, int(Cout), int(Cin)), "dc_debug_unpack_conv3x3")
    return out.numpy()


def train_begin(ctx, **opts):
    """dc_train_begin: allocate the moments and the gradient arena, t = 0.  opts: the keys of TRAIN_DEFAULTS."""
    o = train_opts(**opts)
    check(ctx.h, ctx.lib.dc_train_begin(ctx.h, C.byref(o)), "dc_train_begin")
    ctx.grad_clip = 0.0


def train_set_cnn(ctx, mode):
    """dc_train_set_cnn: 0 = the CNN is left alone (the default), 1 = weight decay and Adam on conv3_1 .. conv5_3 with a zero
    gradient (train.lua's step at iter == finetune_cnn_after), 2 = the full backward, decay and Adam."""
    check(ctx.h, ctx.lib.dc_train_set_cnn(ctx.h, int(mode)), "dc_train_set_cnn")


def finetune_cnn_mode(finetune_cnn_after, it):
    """The CNN mode of 1-based iteration `it` under train.lua's -finetune_cnn_after N (its iter is 0-based: k = it - 1 before the
    step): 0 if N < 0 or k < N, 1 if k == N, 2 if k > N."""
    N, k = int(finetune_cnn_after), int(it) - 1
    if N < 0 or k < N:
        return 0
    return 1 if k == N else 2


def train_step(ctx, img, gt_boxes, gt_labels, box_reg_decay=BOX_REG_DECAY, forced_pos=None, forced_neg=None, dump=False,
               on_device=False, **opts):
    """dc_train_step: forward_backward's losses for the weights as they were (same arguments, the same numbers; no gradient
    leaves the device), then the Adam update of the 21 tensors outside the CNN and the refresh of what is derived from them.
    While train_set_grad_clip is on, the dict also holds `grad_norm` and `grad_scale` of this step."""
    args, out, lists, _hw, _cap, _keep = _train_args("train_step", ctx, img, gt_boxes, gt_labels, forced_pos, forced_neg, dump,
                                                    on_device, opts)
    check(ctx.h, ctx.lib.dc_train_step(*args, float(box_reg_decay)), "dc_train_step")
    res = _train_result(out, lists)
    if getattr(ctx, "grad_clip", 0.0) > 0:                   # (train_set_grad_clip's; the dict is the unclipped one otherwise)
        res["grad_norm"], res["grad_scale"] = train_grad_norm(ctx)
    return res


def train_set_grad_clip(ctx, max_norm):
    """dc_train_set_grad_clip: clip the step's gradient by its global L2 norm (docs/SEMANTICS.md, "Gradient clipping").  0: off
    (the default after train_begin); inf: the norm is computed and reported, nothing is scaled."""
    check(ctx.h, ctx.lib.dc_train_set_grad_clip(ctx.h, float(max_norm)), "dc_train_set_grad_clip")
    ctx.grad_clip = float(max_norm)


def train_grad_norm(ctx):
    """dc_train_grad_norm: (norm, scale) of the last completed clipped step."""
    norm, scale = C.c_double(0.0), C.c_float(0.0)
    check(ctx.h, ctx.lib.dc_train_grad_norm(ctx.h, C.byref(norm), C.byref(scale)), "dc_train_grad_norm")
    return float(norm.value), float(np.float32(scale.value))


def grad_norm(ctx, g, max_norm, offset=0, guard=8):
    """The two norm kernels alone (dc_op_grad_norm) on a copy of the float32 vector g.  offset: floats by which the buffer is
    shifted off its 16-byte aligned allocation; guard: floats on both sides of it, filled with NaN (a read outside g turns the
    sum into NaN).  Returns (sumsq, norm, scale): two floats and an np.float32."""
    a = _f32(g).reshape(-1)
    n = len(a)
    host = np.full(offset + guard + n + guard, np.nan, np.float32)
    host[offset + guard:offset + guard + n] = a
    buf = ctx.to_device(host)
    sumsq, norm, scale = C.c_double(0.0), C.c_double(0.0), C.c_float(0.0)
    check(ctx.h, ctx.lib.dc_op_grad_norm(ctx.h, C.c_void_p(buf.ptr.value + 4 * (offset + guard)), n, float(max_norm), C.byref(sumsq),
                                         C.byref(norm), C.byref(scale)), "dc_op_grad_norm")
    return float(sumsq.value), float(norm.value), np.float32(scale.value)


def adam_multi_clip(ctx, segments, t, max_norm, grid=0, **opts):
    """dc_debug_adam_multi_clip: adam_multi's segments through the sequence a clipped train_step issues (the norm over all the
    g, then the scaled Adam launch).  Returns (list of (p, m, v), sumsq, scale)."""
    o = train_opts(**opts)
    dev = [[ctx.to_device(_f32(a).reshape(-1)) for a in seg] for seg in segments]
    ns = len(dev)
    cols = [(C.c_void_p * ns)(*[d[j].ptr for d in dev]) for j in range(4)]
    sizes = (C.c_size_t * ns)(*[d[0].shape[0] for d in dev])
    sumsq, scale = C.c_double(0.0), C.c_float(0.0)
    check(ctx.h, ctx.lib.dc_debug_adam_multi_clip(ctx.h, cols[0], cols[1], cols[2], cols[3], sizes, ns, int(t), C.byref(o), int(grid),
                                                  float(max_norm), C.byref(sumsq), C.byref(scale)), "dc_debug_adam_multi_clip")
    return [(d[0].numpy(), d[2].numpy(), d[3].numpy()) for d in dev], float(sumsq.value), np.float32(scale.value)


def train_end(ctx):
    check(ctx.h, ctx.lib.dc_train_end(ctx.h), "dc_train_end")
    ctx.grad_clip = 0.0


def train_step_ms(ctx):
    """The library's event split of the last train_step in ms: backward (the three stages), the Adam launch, the refresh."""
    ms = np.zeros(3, np.float32)
    check(ctx.h, ctx.lib.dc_debug_fetch(ctx.h, b"train_step_ms", ms.ctypes.data, ms.nbytes), "dc_debug_fetch")
    return dict(zip(("backward", "adam", "refresh"), (float(x) for x in ms)))


WEIGHT_KEYS = ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b",
               "obj_w", "obj_b", "boxreg_w", "boxreg_b", "lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b")


def get_weights(ctx, shapes, conv=True):
    """dc_get_weights: the ctx's current weights in checkpoint layouts.  shapes: {name: shape} for WEIGHT_KEYS and "anchors",
    "conv_w" / "conv_b" lists of 13 shapes (read only with conv).  Returns a dict of float32 arrays (conv_w / conv_b: lists)."""
    w = _lib.DcWeights()
    out = {}
    for name in WEIGHT_KEYS + ("anchors",):
        out[name] = np.empty(tuple(shapes[name]), np.float32)
        setattr(w, name, out[name].ctypes.data_as(_lib.c_float_p))
    if conv:
        out["conv_w"] = [np.empty(tuple(sh), np.float32) for sh in shapes["conv_w"]]
        out["conv_b"] = [np.empty(tuple(sh), np.float32) for sh in shapes["conv_b"]]
        for i in range(_lib.DC_NUM_VGG_CONVS):
            w.conv_w[i] = out["conv_w"][i].ctypes.data_as(_lib.c_float_p)
            w.conv_b[i] = out["conv_b"][i].ctypes.data_as(_lib.c_float_p)
    check(ctx.h, ctx.lib.dc_get_weights(ctx.h, C.byref(w)), "dc_get_weights")
    return out


CNN_STATE_CONVS = tuple(range(4, 13))                       # conv3_1 .. conv5_3: the convolutions dc_train_set_cnn trains


def cnn_state_keys():
    """The names of the CNN's 18 trained tensors in a training state: conv_w4, conv_b4, .., conv_w12, conv_b12."""
    return tuple("conv_%s%d" % (wb, i) for i in CNN_STATE_CONVS for wb in "wb")


def _state_struct(arrs, cnn):
    w = _lib.DcWeights()
    for name in WEIGHT_KEYS:
        setattr(w, name, arrs[name].ctypes.data_as(_lib.c_float_p))
    if cnn:
        for i in CNN_STATE_CONVS:
            w.conv_w[i] = arrs["conv_w%d" % i].ctypes.data_as(_lib.c_float_p)
            w.conv_b[i] = arrs["conv_b%d" % i].ctypes.data_as(_lib.c_float_p)
    return w


def _state_shapes(shapes, cnn):
    out = {name: tuple(shapes[name]) for name in WEIGHT_KEYS}
    if cnn:
        for i in CNN_STATE_CONVS:
            out["conv_w%d" % i] = tuple(shapes["conv_w"][i])
            out["conv_b%d" % i] = tuple(shapes["conv_b"][i])
    return out


def train_get_state(ctx, shapes):
    """dc_train_get_state: {"m": {name: array}, "v": {...}, "t": int, "cnn_t": int} in checkpoint layouts; shapes as get_weights
    takes them.  The CNN's 18 moments (cnn_state_keys) are there once a non-zero train_set_cnn has made them."""
    t7 = np.zeros(1, np.int32)
    check(ctx.h, int(ctx.lib.dc_debug_fetch(ctx.h, b"train_cnn_t", t7.ctypes.data, t7.nbytes)), "dc_debug_fetch train_cnn_t")
    cnn = int(t7[0]) >= 0
    sh = _state_shapes(shapes, cnn)
    m = {k: np.empty(s, np.float32) for k, s in sh.items()}
    v = {k: np.empty(s, np.float32) for k, s in sh.items()}
    wm, wv = _state_struct(m, cnn), _state_struct(v, cnn)
    t, ct = C.c_int(0), C.c_int(0)
    check(ctx.h, ctx.lib.dc_train_get_state(ctx.h, C.byref(wm), C.byref(wv), C.byref(t), C.byref(ct)), "dc_train_get_state")
    return {"m": m, "v": v, "t": int(t.value), "cnn_t": int(ct.value)}


def train_set_state(ctx, state, shapes):
    """dc_train_set_state: load what train_get_state returned (the CNN's moments if the state holds them)."""
    cnn = "conv_w4" in state["m"]
    sh = _state_shapes(shapes, cnn)
    keep = []
    for mom in ("m", "v"):
        arrs = {}
        for k, s in sh.items():
            if k not in state[mom]:
                raise ValueError("training state: %s/%s is missing" % (mom, k))
            a = _f32(state[mom][k])
            if a.size != int(np.prod(s)):
                raise ValueError("training state: %s/%s has %d elements, the model %d" % (mom, k, a.size, int(np.prod(s))))
            arrs[k] = a
        keep.append(arrs)
    wm, wv = _state_struct(keep[0], cnn), _state_struct(keep[1], cnn)
    check(ctx.h, ctx.lib.dc_train_set_state(ctx.h, C.byref(wm), C.byref(wv), int(state["t"]), int(state["cnn_t"])), "dc_train_set_state")


def rpn_dheads(ctx, trans, scores, anchors, boxes, h, w, k, pos_input_idx, pos_target_idx, neg_input_idx, gt, droi=None,
               w_mid_obj=0.1, w_mid_box=0.05, decay=0.0):
    """The gradient at the RPN's head outputs alone (dc_debug_rpn_dheads): the forward's rows (A,4) / (A,2), the lists, gt (G,4),
    droi (n,4) or None -> dheads (h*w, 6k)."""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    pi, pt, ni = i32(pos_input_idx), i32(pos_target_idx), i32(neg_input_idx)
    A = k * h * w
    td, sd, ad, bd = (ctx.to_device(_f32(a).reshape(A, c)) for a, c in ((trans, 4), (scores, 2), (anchors, 4), (boxes, 4)))
    gd = ctx.to_device(_f32(gt).reshape(-1, 4))
    dev = lambda a: ctx.to_device(a) if len(a) else None
    pid, ptd, nid = dev(pi), dev(pt), dev(ni)
    n = len(pi) + len(ni)
    dd = ctx.to_device(_f32(droi).reshape(n, 4)) if droi is not None and n > 0 else None
    ptr = lambda d: None if d is None else d.ptr
    o = ctx.empty((h * w, 6 * k))
    check(ctx.h, ctx.lib.dc_debug_rpn_dheads(ctx.h, td.ptr, sd.ptr, ad.ptr, bd.ptr, int(h), int(w), int(k), ptr(pid), ptr(ptd), len(pi),
                                             ptr(nid), len(ni), gd.ptr, len(_f32(gt).reshape(-1, 4)), ptr(dd), float(w_mid_obj),
                                             float(w_mid_box), float(decay), o.ptr), "dc_debug_rpn_dheads")
    return o.numpy()


def rpn_heads_bwd(ctx, dheads, heads_w, hidden):
    """The heads' data gradient with the ReLU mask alone (dc_debug_rpn_heads_bwd): dheads (P,K6), heads_w (K6,R), hidden (P,R)
    -> dhidden (P,R)."""
    d = _f32(dheads); W = _f32(heads_w); y = _f32(hidden)
    (P, K6), R = d.shape, W.shape[1]
    dd, wd, yd = ctx.to_device(d), ctx.to_device(W), ctx.to_device(y)
    o = ctx.empty((P, R))
    check(ctx.h, ctx.lib.dc_debug_rpn_heads_bwd(ctx.h, dd.ptr, wd.ptr, yd.ptr, P, K6, R, o.ptr), "dc_debug_rpn_heads_bwd")
    return o.numpy()


def lstm_cell_bwd_ex(ctx, gates_pre, c, tok=None, xg=None, c_prev=None, dh_a=None, dh_b=None, dc_in=None, alias=False):
    """The LSTM cell backward with every operand of its launcher (dc_debug_lstm_cell_bwd_ex): gates_pre (rows, 4Hd); c (rows, Hd);
    tok (rows,) with xg (xg_rows, 4Hd), c_prev, dh_a, dh_b, dc_in (rows, Hd) or None.  alias=True writes dc_prev into dc_in's own
    buffer.  -> (dgates (rows, 4Hd), dc_prev (rows, Hd))."""
    g = _f32(gates_pre)
    rows, Hd = g.shape[0], g.shape[1] // 4
    dev = lambda a: None if a is None else ctx.to_device(_f32(a))
    ptr = lambda d: None if d is None else d.ptr
    gd, cd, xgd, cpd, had, hbd, dcd = (dev(a) for a in (g, c, xg, c_prev, dh_a, dh_b, dc_in))
    td = None if tok is None else ctx.to_device(np.ascontiguousarray(tok, dtype=np.int32))
    if alias and dcd is None:
        raise ValueError("lstm_cell_bwd_ex: alias=True needs dc_in")
    dg = ctx.empty((rows, 4 * Hd))
    dcp = dcd if alias else ctx.empty((rows, Hd))
    check(ctx.h, ctx.lib.dc_debug_lstm_cell_bwd_ex(ctx.h, gd.ptr, ptr(td), ptr(xgd), 0 if xg is None else len(xg), ptr(cpd), cd.ptr,
                                                   ptr(had), ptr(hbd), ptr(dcd), rows, Hd, dg.ptr, dcp.ptr),
          "dc_debug_lstm_cell_bwd_ex")
    return dg.numpy(), dcp.numpy()


def check_sample_args(num_samples, temperature, seed, top_k=0, top_p=1.0, want_sample_logprob=False, vocab_size=None):
    """The rules of dc_sample_opts and dc_sample_trunc (docs/SEMANTICS.md, "Sampling captions"), checked before the library is
    called.  Returns the filled DcSampleOpts (the DcSampleTrunc beside it: sample_trunc_arg).  vocab_size (V): top_k's upper
    end V + 1 is checked here when given, by the library otherwise."""
    S = int(num_samples)
    if S != num_samples or not 1 <= S <= 256:
        raise ValueError("num_samples must be an integer in 1..256 (got %r)" % (num_samples,))
    t = float(np.float32(temperature))
    if not (t == 0.0 or 0.01 <= t <= 100.0):         # NaN fails both
        raise ValueError("temperature must be 0 or in [0.01, 100] (got %r)" % (temperature,))
    if t == 0.0 and S != 1:
        raise ValueError("temperature 0 is the greedy rule: num_samples must be 1 (got %d)" % S)
    sd = int(seed)
    if sd != seed or not 0 <= sd < 1 << 64:
        raise ValueError("seed must be an integer in 0..2^64-1 (got %r)" % (seed,))
    sample_trunc_arg(t, top_k, top_p, want_sample_logprob, vocab_size)
    return _lib.DcSampleOpts(S, t, sd)


def sample_trunc_arg(temperature, top_k=0, top_p=1.0, want_sample_logprob=False, vocab_size=None):
    """The DcSampleTrunc of a call, or None when the call is the untruncated one (top_k 0, top_p 1.0, no sample_logprob wanted);
    ValueError where dc_sample_trunc's rules do not hold."""
    try:
        k = int(top_k)
    except (TypeError, ValueError, OverflowError):
        k = -1
    if k != top_k or k < 0 or k >= 1 << 31 or (vocab_size is not None and k > vocab_size + 1):
        raise ValueError("top_k must be 0 (off) or an integer in 1..V+1 (got %r)" % (top_k,))
    p = float(np.float32(top_p))
    if not 0.0 < p <= 1.0:                           # NaN fails
        raise ValueError("top_p must be in (0, 1] (got %r)" % (top_p,))
    on = k != 0 or p != 1.0
    if (on or want_sample_logprob) and float(np.float32(temperature)) == 0.0:
        raise ValueError("temperature 0 is the greedy rule: no top_k / top_p / sample_logprob with it")
    return _lib.DcSampleTrunc(k, p) if on or want_sample_logprob else None


def lm_sample_n(ctx, codes, num_samples, temperature=1.0, seed=0, row_ids=None, seq_length=None, top_k=0, top_p=1.0,
                want_sample_logprob=False):
    """num_samples draws per code row from the ctx's loaded language model (dc_op_lm_sample_n): every word drawn from
    SoftMax(scores / temperature) (temperature 0, num_samples 1: the greedy rule), noise a function of (seed, draw, row id,
    step, word) alone.  codes (n, fc_dim); row_ids (n) ints >= 0 or None (= 0..n-1).  Returns (samples (n, S, T) int32 --
    word ids up to and including the first END, zeros after it --, logprob (n, S) float32: the model's log-probability of
    the words written; NaN, with an all-zero row from that step on, for a row whose scores became NaN -- non-finite codes).
    seq_length: the loaded model's T; needed only when the weights were not loaded through DenseCapModel.
    top_k (0 = off) / top_p (1.0 = off) truncate the distribution of every step (dc_op_lm_sample_n_trunc; docs/SEMANTICS.md,
    "Truncation: top-k and nucleus"); want_sample_logprob appends sample_logprob (n, S) float32 -- the log-probability of
    every draw under the distribution it was drawn from -- to the result.  With neither, the call is the untruncated one."""
    opts = check_sample_args(num_samples, temperature, seed, top_k, top_p, want_sample_logprob)
    trunc = sample_trunc_arg(temperature, top_k, top_p, want_sample_logprob)
    x = _f32(codes)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("codes must be (n, fc_dim) with n >= 1")
    n, S = x.shape[0], opts.num_samples
    ids = None
    if row_ids is not None:
        ids = np.ascontiguousarray(row_ids, dtype=np.int32)
        if ids.shape != (n,) or (ids < 0).any():
            raise ValueError("row_ids must be (n,) ints >= 0")
    # T of the loaded model sizes the outputs: the caller's seq_length, or what DenseCapModel noted on the ctx it loaded
    T = int(seq_length or getattr(ctx, "seq_length", 0) or 0)
    if T < 1:
        raise ValueError("lm_sample_n: pass seq_length= (the loaded model's T) for a ctx that DenseCapModel did not load")
    xd = ctx.to_device(x)
    idd = ctx.to_device(ids) if ids is not None else None
    tok = ctx.empty((n, S, T), np.int32); lp = ctx.empty((n, S), np.float32)
    if trunc is None:
        check(ctx.h, ctx.lib.dc_op_lm_sample_n(ctx.h, xd.ptr, n, idd.ptr if idd is not None else None, C.byref(opts), tok.ptr,
                                               lp.ptr), "dc_op_lm_sample_n")
        return tok.numpy(), lp.numpy()
    lq = ctx.empty((n, S), np.float32) if want_sample_logprob else None
    check(ctx.h, ctx.lib.dc_op_lm_sample_n_trunc(ctx.h, xd.ptr, n, idd.ptr if idd is not None else None, C.byref(opts),
                                                 C.byref(trunc), tok.ptr, lp.ptr, lq.ptr if lq is not None else None),
          "dc_op_lm_sample_n_trunc")
    return (tok.numpy(), lp.numpy(), lq.numpy()) if want_sample_logprob else (tok.numpy(), lp.numpy())


def sample_trunc_rows(ctx, logits, keys, t, seed, temperature, top_k=0, top_p=1.0):
    """The selection of the truncated sampler alone (dc_debug_sample_trunc_rows): logits (rows, V1) float32, keys (rows, 2)
    int32 (r, s).  Returns dict(tok, kept, theta, lp, lq) of per-row arrays."""
    x = _f32(logits)
    k = np.ascontiguousarray(keys, dtype=np.int32)
    rows, V1 = x.shape
    if k.shape != (rows, 2):
        raise ValueError("keys must be (rows, 2)")
    xd = ctx.to_device(x); kd = ctx.to_device(k)
    tok = ctx.empty((rows,), np.int32); kept = ctx.empty((rows,), np.int32); theta = ctx.empty((rows,), np.float32)
    lp = ctx.empty((rows,), np.float64); lq = ctx.empty((rows,), np.float64)
    check(ctx.h, ctx.lib.dc_debug_sample_trunc_rows(ctx.h, xd.ptr, rows, V1, V1, kd.ptr, int(t), int(seed), float(temperature),
                                                    int(top_k), float(top_p), tok.ptr, kept.ptr, theta.ptr, lp.ptr, lq.ptr),
          "dc_debug_sample_trunc_rows")
    return dict(tok=tok.numpy(), kept=kept.numpy(), theta=theta.numpy(), lp=lp.numpy(), lq=lq.numpy())


# ---- beam search test hooks (include/densecap_debug.h) ----------------------------------------------------------------------
BEAM_STATE_FIELDS = ("h", "c", "beam_lp", "beams", "tok", "parent", "fin")


def beam_topk(ctx, logits, k, finished=None, ld=None):
    """dc_debug_beam_topk: LogSoftMax + top-k of every row of logits (rows, V1) -> (top_lp (rows, k) float32, top_idx (rows, k)
    int32, 1-based).  finished: (rows,) flags or None; ld: row stride in floats the logits are laid out with (>= V1)."""
    x = _f32(logits)
    rows, V1 = x.shape
    ld = V1 if ld is None else int(ld)
    if ld > V1:
        x = np.concatenate([x, np.full((rows, ld - V1), np.float32(7e37))], 1)      # never read: a huge value would show
    xd = ctx.to_device(x)
    fd = ctx.to_device(np.ascontiguousarray(finished, dtype=np.uint8)) if finished is not None else None
    lp = ctx.empty((rows, k), np.float32); idx = ctx.empty((rows, k), np.int32)
    check(ctx.h, ctx.lib.dc_debug_beam_topk(ctx.h, xd.ptr, rows, V1, ld, fd.ptr if fd is not None else None, int(k), lp.ptr,
                                            idx.ptr), "dc_debug_beam_topk")
    return lp.numpy(), idx.numpy()


def beam_merge(ctx, top_lp, top_idx, beam_lp, beams, t, END):
    """dc_debug_beam_merge: top_lp / top_idx (nprop, beam, beam), beam_lp (nprop, beam), beams (nprop, beam, T), 0-based column
    t -> dict(beam_lp, beams, parent, tok, fin)."""
    tl = _f32(top_lp); ti = np.ascontiguousarray(top_idx, dtype=np.int32)
    bl = _f32(beam_lp); bm = np.ascontiguousarray(beams, dtype=np.int32)
    nprop, beam, T = bm.shape
    assert tl.shape == ti.shape == (nprop, beam, beam) and bl.shape == (nprop, beam)
    d = [ctx.to_device(a) for a in (tl, ti, bl, bm)]
    o = dict(beam_lp=ctx.empty((nprop, beam), np.float32), beams=ctx.empty((nprop, beam, T), np.int32),
             parent=ctx.empty((nprop, beam), np.int32), tok=ctx.empty((nprop, beam), np.int32),
             fin=ctx.empty((nprop, beam), np.uint8))
    check(ctx.h, ctx.lib.dc_debug_beam_merge(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, nprop, beam, T, int(t), int(END),
                                             o["beam_lp"].ptr, o["beams"].ptr, o["parent"].ptr, o["tok"].ptr, o["fin"].ptr),
          "dc_debug_beam_merge")
    return {k: v.numpy() for k, v in o.items()}


def _beam_state_buffers(ctx, nprop, beam, Hd, T):
    shapes = dict(h=((nprop, beam, Hd), np.float32), c=((nprop, beam, Hd), np.float32), beam_lp=((nprop, beam), np.float32),
                  beams=((nprop, beam, T), np.int32), tok=((nprop, beam), np.int32), parent=((nprop, beam), np.int32),
                  fin=((nprop, beam), np.uint8))
    bufs = {k: ctx.empty(*v) for k, v in shapes.items()}
    return bufs, _lib.DcBeamState(*[bufs[k].ptr for k in BEAM_STATE_FIELDS]), shapes


def beam_start(ctx, codes, beam, rnn_size, seq_length):
    """dc_debug_beam_start at the ctx's beam size `beam` (dc_set_beam_size): codes (nprop, fc_dim) -> (state dict of
    BEAM_STATE_FIELDS, nprop x beam rows; top_lp, top_idx (nprop, beam) of the first step)."""
    x = _f32(codes)
    nprop = x.shape[0]
    xd = ctx.to_device(x)
    bufs, st, _ = _beam_state_buffers(ctx, nprop, beam, rnn_size, seq_length)
    lp = ctx.empty((nprop, beam), np.float32); idx = ctx.empty((nprop, beam), np.int32)
    check(ctx.h, ctx.lib.dc_debug_beam_start(ctx.h, xd.ptr, nprop, C.byref(st), lp.ptr, idx.ptr), "dc_debug_beam_start")
    return {k: v.numpy() for k, v in bufs.items()}, lp.numpy(), idx.numpy()


def beam_step(ctx, state, t):
    """dc_debug_beam_step: iteration t (1 <= t < T) of the search from `state` (a dict as beam_start returns it; `parent` may
    be missing) -> (new state, top_lp, top_idx (nprop, beam, beam): the lists the merge consumed)."""
    nprop, beam, Hd = np.shape(state["h"])
    T = np.shape(state["beams"])[2]
    bufs_in, st_in, shapes = _beam_state_buffers(ctx, nprop, beam, Hd, T)
    for k in BEAM_STATE_FIELDS:
        if k in state:
            a = np.ascontiguousarray(state[k], dtype=shapes[k][1])
            assert a.shape == shapes[k][0], (k, a.shape)
            check(ctx.h, ctx.lib.dc_memcpy_h2d(ctx.h, bufs_in[k].ptr, a.ctypes.data, a.nbytes), "dc_memcpy_h2d")
    bufs, st, _ = _beam_state_buffers(ctx, nprop, beam, Hd, T)
    lp = ctx.empty((nprop, beam, beam), np.float32); idx = ctx.empty((nprop, beam, beam), np.int32)
    check(ctx.h, ctx.lib.dc_debug_beam_step(ctx.h, nprop, int(t), C.byref(st_in), C.byref(st), lp.ptr, idx.ptr),
          "dc_debug_beam_step")
    return {k: v.numpy() for k, v in bufs.items()}, lp.numpy(), idx.numpy()


# ---- standard beam search (dc_op_lm_beam_n; docs/SEMANTICS.md, "Standard beam search") ---------------------------------------
def check_beam_args(beam_size, n_best=None, length_alpha=0.0, vocab_size=None):
    """The DcBeamOpts of a call; ValueError where dc_beam_opts' rules do not hold (what the library answers with DC_E_INVALID):
    beam_size an integer in 1..32 (and <= V+1 when vocab_size is given), n_best None (= beam_size) or an integer in
    1..beam_size, length_alpha in [0, 2]."""
    def as_int(v):
        try:
            i = int(v)
        except (TypeError, ValueError, OverflowError):
            return None
        return i if i == v else None
    B = as_int(beam_size)
    if B is None or not 1 <= B <= 32 or (vocab_size is not None and B > vocab_size + 1):
        raise ValueError("beam_size must be an integer in 1..32, at most V+1 (got %r)" % (beam_size,))
    N = B if n_best is None else as_int(n_best)
    if N is None or not 1 <= N <= B:
        raise ValueError("n_best must be an integer in 1..beam_size = %d (got %r)" % (B, n_best))
    try:
        a = float(np.float32(length_alpha))
    except (TypeError, ValueError):
        a = float("nan")
    if not 0.0 <= a <= 2.0:                          # NaN fails
        raise ValueError("length_alpha must be in [0, 2] (got %r)" % (length_alpha,))
    return _lib.DcBeamOpts(B, N, a)


def lm_beam_n(ctx, codes, beam_size, n_best=None, length_alpha=0.0, seq_length=None):
    """The n_best best captions of every code row by the standard beam search of width beam_size (dc_op_lm_beam_n): finished
    hypotheses are set aside, ranking by logprob / len^length_alpha.  codes (n, fc_dim).  Returns (captions (n, N, T) int32 --
    word ids up to and including END, zeros after it, best first --, logprob (n, N) float32: the model's unnormalised
    log-probability of the words written; NaN, with all-zero rows, for a row whose scores are NaN).  n_best None = beam_size.
    seq_length: the loaded model's T; needed only when the weights were not loaded through DenseCapModel."""
    opts = check_beam_args(beam_size, n_best, length_alpha)
    x = _f32(codes)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("codes must be (n, fc_dim) with n >= 1")
    T = int(seq_length or getattr(ctx, "seq_length", 0) or 0)
    if T < 1:
        raise ValueError("lm_beam_n: pass seq_length= (the loaded model's T) for a ctx that DenseCapModel did not load")
    n, N = x.shape[0], opts.n_best
    xd = ctx.to_device(x)
    cap = ctx.empty((n, N, T), np.int32); lp = ctx.empty((n, N), np.float32)
    check(ctx.h, ctx.lib.dc_op_lm_beam_n(ctx.h, xd.ptr, n, C.byref(opts), cap.ptr, lp.ptr), "dc_op_lm_beam_n")
    return cap.numpy(), lp.numpy()


# ---- standard beam search test hooks (include/densecap_debug_beam.h) ----------------------------------------------------------
BEAM_STD_STATE_FIELDS = BEAM_STATE_FIELDS + ("len",)
BEAM_STD_MERGE_OUT = ("beam_lp", "beams", "len", "parent", "tok", "fin")


def beam_std_merge(ctx, top_lp, top_idx, beam_lp, beams, length, fin, t, END):
    """dc_debug_beam_std_merge: top_lp / top_idx (nprop, beam, beam), beam_lp, length, fin (nprop, beam), beams (nprop, beam, T),
    0-based column t -> dict(beam_lp, beams, len, parent, tok, fin)."""
    tl = _f32(top_lp); ti = np.ascontiguousarray(top_idx, dtype=np.int32)
    bl = _f32(beam_lp); bm = np.ascontiguousarray(beams, dtype=np.int32)
    ln = np.ascontiguousarray(length, dtype=np.int32); fn = np.ascontiguousarray(fin, dtype=np.uint8)
    nprop, beam, T = bm.shape
    assert tl.shape == ti.shape == (nprop, beam, beam) and bl.shape == ln.shape == fn.shape == (nprop, beam)
    d = [ctx.to_device(a) for a in (tl, ti, bl, bm, ln, fn)]
    o = dict(beam_lp=ctx.empty((nprop, beam), np.float32), beams=ctx.empty((nprop, beam, T), np.int32),
             len=ctx.empty((nprop, beam), np.int32), parent=ctx.empty((nprop, beam), np.int32),
             tok=ctx.empty((nprop, beam), np.int32), fin=ctx.empty((nprop, beam), np.uint8))
    check(ctx.h, ctx.lib.dc_debug_beam_std_merge(ctx.h, *[a.ptr for a in d], nprop, beam, T, int(t), int(END),
                                                 *[o[k].ptr for k in BEAM_STD_MERGE_OUT]), "dc_debug_beam_std_merge")
    return {k: v.numpy() for k, v in o.items()}


def beam_std_finish(ctx, beam_lp, beams, length, n_best, length_alpha):
    """dc_debug_beam_std_finish: beam_lp, length (nprop, beam), beams (nprop, beam, T) -> (captions (nprop, n_best, T) int32,
    logprob (nprop, n_best) float32)."""
    bl = _f32(beam_lp); bm = np.ascontiguousarray(beams, dtype=np.int32); ln = np.ascontiguousarray(length, dtype=np.int32)
    nprop, beam, T = bm.shape
    assert bl.shape == ln.shape == (nprop, beam)
    d = [ctx.to_device(a) for a in (bl, bm, ln)]
    cap = ctx.to_device(np.full((nprop, n_best, T), -7, np.int32)); lp = ctx.to_device(np.full((nprop, n_best), 7.0, np.float32))
    check(ctx.h, ctx.lib.dc_debug_beam_std_finish(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, nprop, beam, T, int(n_best),
                                                  float(length_alpha), cap.ptr, lp.ptr), "dc_debug_beam_std_finish")
    return cap.numpy(), lp.numpy()


def _beam_std_state_buffers(ctx, nprop, beam, Hd, T):
    bufs, _, shapes = _beam_state_buffers(ctx, nprop, beam, Hd, T)
    shapes["len"] = ((nprop, beam), np.int32)
    bufs["len"] = ctx.empty(*shapes["len"])
    return bufs, _lib.DcBeamStdState(*[bufs[k].ptr for k in BEAM_STD_STATE_FIELDS]), shapes


def beam_std_start(ctx, codes, beam, rnn_size, seq_length):
    """dc_debug_beam_std_start at width `beam`: codes (nprop, fc_dim) -> (state dict of BEAM_STD_STATE_FIELDS, nprop x beam
    rows; top_lp, top_idx (nprop, beam) of the first step)."""
    x = _f32(codes)
    nprop = x.shape[0]
    xd = ctx.to_device(x)
    bufs, st, _ = _beam_std_state_buffers(ctx, nprop, beam, rnn_size, seq_length)
    lp = ctx.empty((nprop, beam), np.float32); idx = ctx.empty((nprop, beam), np.int32)
    check(ctx.h, ctx.lib.dc_debug_beam_std_start(ctx.h, xd.ptr, nprop, int(beam), C.byref(st), lp.ptr, idx.ptr),
          "dc_debug_beam_std_start")
    return {k: v.numpy() for k, v in bufs.items()}, lp.numpy(), idx.numpy()


def beam_std_step(ctx, state, t):
    """dc_debug_beam_std_step: iteration t (1 <= t < T) from `state` (a dict as beam_std_start returns it; `parent` may be
    missing) -> (new state, top_lp, top_idx (nprop, beam, beam): the lists of the step)."""
    nprop, beam, Hd = np.shape(state["h"])
    T = np.shape(state["beams"])[2]
    bufs_in, st_in, shapes = _beam_std_state_buffers(ctx, nprop, beam, Hd, T)
    for k in BEAM_STD_STATE_FIELDS:
        if k in state:
            a = np.ascontiguousarray(state[k], dtype=shapes[k][1])
            assert a.shape == shapes[k][0], (k, a.shape)
            check(ctx.h, ctx.lib.dc_memcpy_h2d(ctx.h, bufs_in[k].ptr, a.ctypes.data, a.nbytes), "dc_memcpy_h2d")
    bufs, st, _ = _beam_std_state_buffers(ctx, nprop, beam, Hd, T)
    lp = ctx.empty((nprop, beam, beam), np.float32); idx = ctx.empty((nprop, beam, beam), np.int32)
    check(ctx.h, ctx.lib.dc_debug_beam_std_step(ctx.h, nprop, beam, int(t), C.byref(st_in), C.byref(st), lp.ptr, idx.ptr),
          "dc_debug_beam_std_step")
    return {k: v.numpy() for k, v in bufs.items()}, lp.numpy(), idx.numpy()


# ---- screened greedy decode test hooks (include/densecap_debug.h) ------------------------------------------------------------
DEBUG_FILL = 0xA5            # the byte every output buffer of the two hooks below holds before the call


def screen_pads(rnn_size, vocab_size):
    """(Kp, V1pad) of a loaded model: the bf16 row length and the score row length of the screened route."""
    return (int(rnn_size) + 63) // 64 * 64, (int(vocab_size) + 1 + 63) // 64 * 64


def _filled(ctx, shape, dtype):
    return ctx.to_device(np.full(shape, DEBUG_FILL, np.uint8).view(dtype))


def _count(ctx, n_dev):
    return ctx.to_device(np.array([n_dev], np.int32)) if n_dev is not None else None


def screen_scores(ctx, h, vocab_size, n_dev=None, guard_rows=2):
    """dc_debug_screen_scores on the ctx's loaded model: h (n, rnn_size) -> (hb (n + g, Kp) uint16 bf16 patterns, hnorm (n + g,)
    float32, scores (n + g, V1pad) float16) with g = guard_rows rows the call must not touch after the n it may.  Every byte of
    the outputs is DEBUG_FILL before the call; n_dev: a device-side row count."""
    x = _f32(h)
    n, Hd = x.shape
    Kp, V1pad = screen_pads(Hd, vocab_size)
    g = int(guard_rows)
    xd = ctx.to_device(x); nd = _count(ctx, n_dev)
    hb = _filled(ctx, (n + g, 2 * Kp), np.uint16); hn = _filled(ctx, ((n + g) * 4,), np.float32)
    sc = _filled(ctx, (n + g, 2 * V1pad), np.float16)
    check(ctx.h, ctx.lib.dc_debug_screen_scores(ctx.h, xd.ptr, n, nd.ptr if nd is not None else None, hb.ptr, hn.ptr, sc.ptr),
          "dc_debug_screen_scores")
    return hb.numpy(), hn.numpy(), sc.numpy()


def rescore_tail(ctx, scores, h, hnorm, c=None, gates_pre=None, n_dev=None, guard_rows=2):
    """dc_debug_rescore_tail: scores (n, V1pad) float16, h (n, rnn_size), hnorm (n,) -> dict(tok, cand (int32), best (float32)),
    n + guard_rows rows each; with gates_pre (n, 4 rnn_size) and c (n, rnn_size) also h, c, hb (uint16 bf16 patterns), hnorm of
    the LSTM update.  Every byte of the outputs is DEBUG_FILL before the call; n_dev: a device-side row count."""
    s = np.ascontiguousarray(scores, dtype=np.float16)
    x = _f32(h); hn = _f32(hnorm)
    n, Hd = x.shape
    Kp = screen_pads(Hd, 0)[0]
    assert s.shape[0] == n and s.shape[1] % 64 == 0 and hn.shape == (n,)
    g = int(guard_rows)
    sd = ctx.to_device(s); xd = ctx.to_device(x); hd = ctx.to_device(hn); nd = _count(ctx, n_dev)
    o = dict(tok=_filled(ctx, ((n + g) * 4,), np.int32), cand=_filled(ctx, ((n + g) * 4,), np.int32),
             best=_filled(ctx, ((n + g) * 4,), np.float32))
    cd = gd = None
    if gates_pre is not None:
        cc = _f32(c); gp = _f32(gates_pre)
        assert cc.shape == (n, Hd) and gp.shape == (n, 4 * Hd)
        cd = ctx.to_device(cc); gd = ctx.to_device(gp)
        o.update(h=_filled(ctx, (n + g, 4 * Hd), np.float32), c=_filled(ctx, (n + g, 4 * Hd), np.float32),
                 hb=_filled(ctx, (n + g, 2 * Kp), np.uint16), hnorm=_filled(ctx, ((n + g) * 4,), np.float32))
    ptr = lambda k: o[k].ptr if k in o else None
    check(ctx.h, ctx.lib.dc_debug_rescore_tail(ctx.h, sd.ptr, xd.ptr, cd.ptr if cd is not None else None, hd.ptr,
                                               gd.ptr if gd is not None else None, n, nd.ptr if nd is not None else None,
                                               o["tok"].ptr, o["cand"].ptr, o["best"].ptr, ptr("h"), ptr("c"), ptr("hb"),
                                               ptr("hnorm")), "dc_debug_rescore_tail")
    return {k: v.numpy() for k, v in o.items()}


# ---- the classic decode step's test hooks (include/densecap_debug_step.h) -----------------------------------------------------
STEP_STORE, STEP_ARGMAX, STEP_LSE, STEP_SAMPLE = 0, 1, 2, 3
STEP_TAIL_GREEDY, STEP_TAIL_SCORE, STEP_TAIL_SAMPLE = 0, 1, 2
STEP_NO_COLUMN = 0x7fffffff      # the column of a partial without an entry
STEP_FLOATS_PER_SLOT = {STEP_ARGMAX: 1, STEP_LSE: 2, STEP_SAMPLE: 5}


def step_slots(columns):
    """32-column slots of an epilogue over `columns` columns (amax_cols with a prefix, N without): two per 64-column tile."""
    return 2 * ((int(columns) + 63) // 64)


def step_part_ld(epilogue, columns):
    """The least row length of an epilogue's partials, as include/densecap_debug_step.h documents it."""
    return STEP_FLOATS_PER_SLOT[epilogue] * step_slots(columns) + (1 if epilogue == STEP_LSE else 0)


def _on_device(ctx, a, dtype):
    """a as a DeviceArray: kept if it is one (operands a test uploads once), uploaded otherwise; None stays None."""
    if a is None or isinstance(a, DeviceArray):
        return a
    return ctx.to_device(np.ascontiguousarray(a, dtype=dtype))


def _ptr(buf):
    return buf.ptr if buf is not None else None


def step_gemm(ctx, A, W, bias, epilogue, M, N, K, plan_M=0, relu=False, amax_cols=0, amax_n=0, part_ld=None, ldc=None,
              rowidx=None, t=0, seed=0, inv_temp=0.0, m_dev=None, guard_rows=2, want_C=True, raise_errors=True):
    """dc_debug_step_gemm.  A (M, K), W (N, K), bias (N) or None: numpy arrays or DeviceArrays.  Returns a dict of the outputs the
    epilogue has, each with guard_rows rows after the M the call may write and every byte DEBUG_FILL before the call:
    C (M + g, ldc) float32 (a store, or the raw half of a prefix; want_C=False passes null), part (M + g, part_ld) float32,
    idx (M + g, part_ld) int32 (arg-max).  rc = the call's return code; raise_errors=False returns it with the (untouched)
    buffers instead of raising.  m_dev: a device-side row count."""
    g = int(guard_rows)
    Ad, Wd, bd = _on_device(ctx, A, np.float32), _on_device(ctx, W, np.float32), _on_device(ctx, bias, np.float32)
    rd = _on_device(ctx, rowidx, np.int32)
    nd = _count(ctx, m_dev)
    out = {}
    stored = N if epilogue == STEP_STORE else max(N - amax_cols, 0) if amax_cols > 0 else 0
    if ldc is None:
        ldc = stored
    if want_C and (epilogue == STEP_STORE or amax_cols > 0):
        out["C"] = _filled(ctx, (M + g, 4 * max(ldc, 1)), np.float32)
    if epilogue != STEP_STORE:
        if part_ld is None:
            part_ld = step_part_ld(epilogue, amax_cols if amax_cols > 0 else N)
        out["part"] = _filled(ctx, (M + g, 4 * max(part_ld, 1)), np.float32)
        if epilogue == STEP_ARGMAX:
            out["idx"] = _filled(ctx, (M + g, 4 * max(part_ld, 1)), np.int32)
    a = _lib.DcStepGemm(A=Ad.ptr, W=Wd.ptr, bias=_ptr(bd), M=M, N=N, K=K, plan_M=plan_M, epilogue=epilogue, relu=int(relu),
                        C=_ptr(out.get("C")), ldc=ldc, part_ld=part_ld or 0, part=_ptr(out.get("part")), part_idx=_ptr(out.get("idx")),
                        rowidx=_ptr(rd), t=int(t), inv_temp=float(inv_temp), seed=int(seed), amax_cols=amax_cols, amax_n=amax_n,
                        m_dev_or_null=_ptr(nd))
    rc = ctx.lib.dc_debug_step_gemm(ctx.h, C.byref(a))
    if raise_errors:
        check(ctx.h, rc, "dc_debug_step_gemm")
    res = {k: v.numpy() for k, v in out.items()}
    res["rc"] = rc
    return res


def step_tail(ctx, kind, n, Hd, part=None, idx=None, nslots=0, ld=0, xg=None, gates_pre=None, c=None, h=None, n_dev=None,
              zero_c=False, fixed_tok=0, tgt=None, end_tok=0, acc=None, fin=None, T=1, t=0, raise_errors=True):
    """dc_debug_step_tail: one launch of the greedy / scoring / sampling row tail on n rows.  part (n, ld) float32 (the sampling
    partials' column travels as a float's bits), idx (n, ld) int32 (greedy), xg (xg_rows, 4 Hd), gates_pre (n, 4 Hd) or None,
    c, h (n, Hd), tgt (n,) int32, acc (n,) float64 and fin (n,) uint8 as they stand before the launch.  Returns dict(rc, c, h,
    acc, fin, seq) of what the kind has, after the launch; seq (n, T) int32 with every byte DEBUG_FILL before it."""
    f = lambda a_: _on_device(ctx, a_, np.float32)
    pd, xd, gd, cd, hd = f(part), f(xg), f(gates_pre), f(c), f(h)
    idd, td = _on_device(ctx, idx, np.int32), _on_device(ctx, tgt, np.int32)
    ad, fd = _on_device(ctx, acc, np.float64), _on_device(ctx, fin, np.uint8)
    nd = _count(ctx, n_dev)
    seq = _filled(ctx, (n, 4 * T), np.int32) if kind != STEP_TAIL_SCORE else None
    a = _lib.DcStepTail(kind=kind, nslots=nslots, ld=ld, xg_rows=xd.shape[0] if xd is not None else 0, part=_ptr(pd),
                        part_idx=_ptr(idd), xg=_ptr(xd), gates_pre=_ptr(gd), c=_ptr(cd), h=_ptr(hd), n=n, Hd=Hd,
                        n_dev_or_null=_ptr(nd), zero_c=int(zero_c), fixed_tok=int(fixed_tok), tgt=_ptr(td), end_tok=int(end_tok),
                        T=T, t=t, acc=_ptr(ad), fin=_ptr(fd), seq=_ptr(seq))
    rc = ctx.lib.dc_debug_step_tail(ctx.h, C.byref(a))
    if raise_errors:
        check(ctx.h, rc, "dc_debug_step_tail")
    res = {k: v.numpy() for k, v in (("c", cd), ("h", hd), ("acc", ad), ("fin", fd), ("seq", seq)) if v is not None}
    res["rc"] = rc
    return res


# ---- the forward path's glue kernels, one launch each (include/densecap_debug_glue.h) -------------------------------------------
# Every output buffer holds a sentinel before the call -- a fixed NaN pattern in float32 buffers, 0x5a5a5a5a in int32 buffers, 0x5a
# in the byte records -- and carries guard rows after its end; the wrappers return the whole buffers, guards included, with
# rc = the call's return code (raise_errors=False: returned with the untouched buffers instead of raising).
GLUE_F32_FILL = 0x7fc5a5a5
GLUE_I32_FILL = 0x5a5a5a5a
GLUE_BYTE_FILL = 0x5a


def _glue_filled(ctx, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return ctx.to_device(np.full(shape, GLUE_F32_FILL, np.uint32).view(np.float32))
    return ctx.to_device(np.full(shape, GLUE_I32_FILL if dtype == np.int32 else GLUE_BYTE_FILL, dtype))


def _glue_guarded(ctx, a, dtype, guard_rows):
    """a on the device with guard_rows sentinel rows after it (a buffer a kernel reads AND writes)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    buf = _glue_filled(ctx, (a.shape[0] + guard_rows,) + a.shape[1:], dtype).numpy()
    buf[:a.shape[0]] = a
    return ctx.to_device(buf)


def _glue_counts(ctx, count, stride):
    """Per-image counts `stride` int32 apart; the slots between them hold the int32 sentinel (a large count)."""
    count = np.asarray(count, np.int32).reshape(-1)
    step = max(int(stride), 1)                       # (a stride below 1 is for the hook to refuse)
    a = np.full((len(count) * step,), GLUE_I32_FILL, np.int32)
    a[::step] = count
    return ctx.to_device(a)


def _glue_result(ctx, rc, who, out, raise_errors):
    if raise_errors:
        check(ctx.h, rc, who)
    res = {k: v.numpy() for k, v in out.items() if v is not None}
    res["rc"] = rc
    return res


def glue_boxes_ingest(ctx, in_boxes, in_n, P, clip, img_h, img_w, count_stride=1, guard_rows=2, raise_errors=True):
    """dc_debug_boxes_ingest: in_boxes (nimg * P, 4), in_n (nimg,) -> roi_boxes (nimg * P + g, 4), box_src (nimg * P + g,),
    count (nimg * count_stride + g,)."""
    nimg = len(in_n)
    g = int(guard_rows)
    bd, nd = ctx.to_device(_f32(in_boxes)), ctx.to_device(np.asarray(in_n, np.int32))
    out = dict(roi_boxes=_glue_filled(ctx, (nimg * P + g, 4), np.float32), box_src=_glue_filled(ctx, (nimg * P + g,), np.int32),
               count=_glue_filled(ctx, (nimg * count_stride + g,), np.int32))
    rc = ctx.lib.dc_debug_boxes_ingest(ctx.h, bd.ptr, nd.ptr, nimg, int(P), int(clip), int(img_h), int(img_w), out["roi_boxes"].ptr,
                                       out["box_src"].ptr, out["count"].ptr, int(count_stride))
    return _glue_result(ctx, rc, "dc_debug_boxes_ingest", out, raise_errors)


def glue_roi_pool_group(ctx, feats, B, img_h, img_w, HH, WW, out_layout, boxes=None, B_dev=None, bdev_stride=1, pick=None,
                        src_boxes=None, src_pad_rows=3, feat_pad=8, guard_rows=2, raise_errors=True):
    """dc_debug_roi_pool_group.  feats (nimg, C, h, w), uploaded channels last with feat_pad floats between two maps; boxes
    (nimg * B, 4) (without pick); B_dev (nimg,) or None; pick (nimg * B,) into src_boxes (nimg, S, 4), uploaded with
    src_pad_rows rows between two images' lists.  Returns out (nimg * B + g, ...) in the layout asked for and boxes
    (nimg * B + g, 4) as they stand after the call."""
    f = _f32(feats)
    nimg, C_, h, w = f.shape
    g = int(guard_rows)
    fs = h * w * C_ + int(feat_pad)
    fh = np.zeros((nimg, fs), np.float32)
    fh[:, :h * w * C_] = f.transpose(0, 2, 3, 1).reshape(nimg, -1)
    fd = ctx.to_device(fh)
    bd = _glue_guarded(ctx, _f32(boxes).reshape(nimg * B, 4), np.float32, g) if boxes is not None else _glue_filled(ctx, (nimg * B + g, 4), np.float32)
    cd = _glue_counts(ctx, B_dev, bdev_stride) if B_dev is not None else None
    pd = ctx.to_device(np.asarray(pick, np.int32).reshape(-1)) if pick is not None else None
    sd, S, ss = None, 0, 0
    if src_boxes is not None:
        sb = _f32(src_boxes)
        S = sb.shape[1]
        ss = (S + int(src_pad_rows)) * 4
        sh = np.full((nimg, ss), 1e30, np.float32)
        sh[:, :S * 4] = sb.reshape(nimg, -1)
        sd = ctx.to_device(sh)
    out = dict(out=_glue_filled(ctx, (nimg * B + g, C_, HH, WW) if out_layout == 0 else (nimg * B + g, HH, WW, C_), np.float32), boxes=bd)
    a = _lib.DcGlueRoiPool(feat_hwc=fd.ptr, feat_stride=fs, nimg=nimg, h=h, w=w, C=C_, boxes=bd.ptr, B=int(B), B_dev=_ptr(cd),
                           bdev_stride=int(bdev_stride), pick=_ptr(pd), src_boxes=_ptr(sd), src_stride=ss, src_rows=S,
                           img_h=int(img_h), img_w=int(img_w), HH=int(HH), WW=int(WW), out=out["out"].ptr, out_layout=int(out_layout))
    rc = ctx.lib.dc_debug_roi_pool_group(ctx.h, C.byref(a))
    return _glue_result(ctx, rc, "dc_debug_roi_pool_group", out, raise_errors)


def glue_recog_heads(ctx, codes, w5, b5, roi, with_xyxy=True, guard_rows=2, raise_errors=True):
    """dc_debug_recog_heads: codes (n, D), w5 (5, D), b5 (5,), roi (n, 4) -> obj (n + g,), trans, fin, fin_xyxy (n + g, 4)."""
    x = _f32(codes)
    n, D = x.shape
    g = int(guard_rows)
    xd, wd, bd, rd = ctx.to_device(x), ctx.to_device(_f32(w5)), ctx.to_device(_f32(b5)), ctx.to_device(_f32(roi))
    out = dict(obj=_glue_filled(ctx, (n + g,), np.float32), trans=_glue_filled(ctx, (n + g, 4), np.float32),
               fin=_glue_filled(ctx, (n + g, 4), np.float32), fin_xyxy=_glue_filled(ctx, (n + g, 4), np.float32) if with_xyxy else None)
    rc = ctx.lib.dc_debug_recog_heads(ctx.h, xd.ptr, wd.ptr, bd.ptr, rd.ptr, out["obj"].ptr, out["trans"].ptr, out["fin"].ptr,
                                      _ptr(out["fin_xyxy"]), n, D)
    return _glue_result(ctx, rc, "dc_debug_recog_heads", out, raise_errors)


def glue_iota_count(ctx, cap, count_in, guard_rows=2, raise_errors=True):
    """dc_debug_iota_count -> idx (cap + g,), count_out (1 + g,)."""
    g = int(guard_rows)
    cd = _count(ctx, int(count_in))
    out = dict(idx=_glue_filled(ctx, (max(cap, 0) + g,), np.int32), count_out=_glue_filled(ctx, (1 + g,), np.int32))
    rc = ctx.lib.dc_debug_iota_count(ctx.h, out["idx"].ptr, out["count_out"].ptr, cd.ptr, int(cap))
    return _glue_result(ctx, rc, "dc_debug_iota_count", out, raise_errors)


def glue_gather_rows(ctx, src, idx, count, cap, guard_rows=2, raise_errors=True):
    """dc_debug_gather_rows: src (src_rows, width) float32 or int32 (the dtype selects the kernel), idx (cap,) -> out (cap + g, width)."""
    src = np.ascontiguousarray(src)
    is_i32 = src.dtype == np.int32
    if not is_i32:
        src = _f32(src)
    g = int(guard_rows)
    sd, idd, cd = ctx.to_device(src), ctx.to_device(np.asarray(idx, np.int32)), _count(ctx, int(count))
    out = dict(out=_glue_filled(ctx, (max(cap, 0) + g, src.shape[1]), src.dtype))
    rc = ctx.lib.dc_debug_gather_rows(ctx.h, sd.ptr, src.shape[0], idd.ptr, cd.ptr, int(cap), src.shape[1], out["out"].ptr, int(is_i32))
    return _glue_result(ctx, rc, "dc_debug_gather_rows", out, raise_errors)


def glue_survivor_compact(ctx, codes, picks, count, P, count_stride=1, guard_rows=2, raise_errors=True):
    """dc_debug_survivor_compact: codes (nimg * P, D), picks (nimg * P,), count (nimg,) -> out (nimg * P + g, D), total (1 + g,)."""
    x = _f32(codes)
    nimg = len(count)
    g = int(guard_rows)
    xd, pd, cd = ctx.to_device(x), ctx.to_device(np.asarray(picks, np.int32)), _glue_counts(ctx, count, count_stride)
    out = dict(out=_glue_filled(ctx, (nimg * P + g, x.shape[1]), np.float32), total=_glue_filled(ctx, (1 + g,), np.int32))
    rc = ctx.lib.dc_debug_survivor_compact(ctx.h, xd.ptr, pd.ptr, cd.ptr, int(count_stride), nimg, int(P), x.shape[1], out["out"].ptr,
                                           out["total"].ptr)
    return _glue_result(ctx, rc, "dc_debug_survivor_compact", out, raise_errors)


def glue_record_bytes(P, words, with_src):
    """Bytes of one image's record: the header's 256, boxes, scores, `words` values a row and, with_src, one int32 a row."""
    return 256 + 4 * int(P) * (5 + int(words) + (1 if with_src else 0))


def glue_final_pack(ctx, final_boxes, obj, picks, count, P, tokens=None, tok_gather=0, codes=None, fault=None, box_src=None,
                    count_stride=1, stride=None, guard_bytes=256, raise_errors=True):
    """dc_debug_final_pack: final_boxes (nimg * P, 4), obj (nimg * P,), picks (nimg * P,), count (nimg,), tokens (nimg * P, T)
    int32 or codes (nimg * P, D), fault: the word the fault pointer points at (None: a null pointer), box_src (nimg * P,) or
    None.  stride: bytes between two records (default: the record, rounded up to 256, plus 256).  Returns pack (nimg * stride +
    guard_bytes,) uint8."""
    nimg = len(count)
    td = ctx.to_device(np.ascontiguousarray(tokens, dtype=np.int32)) if tokens is not None else None
    xd = ctx.to_device(_f32(codes)) if codes is not None else None
    T = td.shape[1] if td is not None else 0
    D = xd.shape[1] if xd is not None else 0
    if stride is None:
        stride = (glue_record_bytes(P, D if xd is not None else T, box_src is not None) + 255) // 256 * 256 + 256
    bd, od = ctx.to_device(_f32(final_boxes)), ctx.to_device(_f32(obj))
    pd, cd = ctx.to_device(np.asarray(picks, np.int32)), _glue_counts(ctx, count, count_stride)
    fd = ctx.to_device(np.array([fault], np.uint32)) if fault is not None else None
    sd = ctx.to_device(np.asarray(box_src, np.int32)) if box_src is not None else None
    out = dict(pack=_glue_filled(ctx, (nimg * int(stride) + int(guard_bytes),), np.uint8))
    a = _lib.DcGlueFinalPack(final_boxes=bd.ptr, obj=od.ptr, tokens=_ptr(td), tok_gather=int(tok_gather), codes=_ptr(xd), picks=pd.ptr,
                             count=cd.ptr, count_stride=int(count_stride), fault=_ptr(fd), nimg=nimg, P=int(P), T=T, D=D,
                             pack=out["pack"].ptr, stride=int(stride), box_src=_ptr(sd))
    rc = ctx.lib.dc_debug_final_pack(ctx.h, C.byref(a))
    return _glue_result(ctx, rc, "dc_debug_final_pack", out, raise_errors)


# ---- the two NMS launchers with a device-side row count (include/densecap_debug_nms.h) -------------------------------------------
# Output buffers are sentinel-filled and guarded as the glue wrappers' are; `null` names arguments to pass as null pointers.
def nms_debug(ctx, boxes5, thresh, max_boxes=None, valid=None, n_dev=None, ws_rows=None, n=None, guard_rows=2, null=(),
              raise_errors=True):
    """dc_debug_nms: launch_nms on boxes5 (N, 5) x1 y1 x2 y2 score.  max_boxes None: -1; valid (N,) bytes or None; n_dev: the
    value of the device-side row count or None (a null pointer); ws_rows: rows the workspace is bound for (default n); n: the
    row count passed (default N).  Returns dict(rc, picks (cap + g,), count (1 + g,), order (N + g,), nvalid (1 + g,)), all
    int32, cap = N or min(N, max_boxes)."""
    b = _f32(boxes5)
    N = b.shape[0]
    n = N if n is None else int(n)
    g = int(guard_rows)
    bd = ctx.to_device(np.ascontiguousarray(b[:, :4])) if "boxes" not in null else None
    sd = ctx.to_device(np.ascontiguousarray(b[:, 4])) if "scores" not in null else None
    vd = ctx.to_device(np.ascontiguousarray(valid, dtype=np.uint8)) if valid is not None else None
    nd = ctx.to_device(np.array([n_dev], np.int32)) if n_dev is not None else None
    mb = -1 if max_boxes is None else int(max_boxes)
    cap = N if mb < 0 else min(N, mb)
    out = dict(picks=_glue_filled(ctx, (cap + g,), np.int32), count=_glue_filled(ctx, (1 + g,), np.int32),
               order=_glue_filled(ctx, (N + g,), np.int32), nvalid=_glue_filled(ctx, (1 + g,), np.int32))
    rc = ctx.lib.dc_debug_nms(ctx.h, _ptr(bd), _ptr(sd), _ptr(vd), n, _ptr(nd), n if ws_rows is None else int(ws_rows),
                              C.c_float(float(np.float32(thresh))), mb, None if "picks" in null else out["picks"].ptr,
                              None if "count" in null else out["count"].ptr, out["order"].ptr, out["nvalid"].ptr)
    return _glue_result(ctx, rc, "dc_debug_nms", out, raise_errors)


def nms_multi_debug(ctx, boxes, scores, thresh, max_picks, valid=None, n_dev=None, n=None, Q=None, guard_rows=2, null=(),
                    raise_errors=True):
    """dc_debug_nms_multi: launch_nms_multi on boxes (N, 4), scores (N, Q) with the device-side row count n_dev (None: a null
    pointer).  Returns dict(rc, picks (Q + g, M) int32, counts (Q + g,) int32), M = max_picks clamped to 1..4096."""
    b = _f32(boxes).reshape(-1, 4)
    s = _f32(scores)
    if s.ndim == 1:
        s = s[:, None]
    N, Qs = s.shape
    n = N if n is None else int(n)
    Q = Qs if Q is None else int(Q)
    g = int(guard_rows)
    bd = ctx.to_device(b) if "boxes" not in null else None
    sd = ctx.to_device(s) if "scores" not in null else None
    vd = ctx.to_device(np.ascontiguousarray(valid, dtype=np.uint8)) if valid is not None else None
    nd = ctx.to_device(np.array([n_dev], np.int32)) if n_dev is not None else None
    M = min(max(int(max_picks), 1), 4096)
    out = dict(picks=_glue_filled(ctx, (Qs + g, M), np.int32), counts=_glue_filled(ctx, (Qs + g,), np.int32))
    rc = ctx.lib.dc_debug_nms_multi(ctx.h, _ptr(bd), _ptr(sd), _ptr(vd), n, _ptr(nd), Q, C.c_float(float(np.float32(thresh))),
                                    int(max_picks), None if "picks" in null else out["picks"].ptr,
                                    None if "counts" in null else out["counts"].ptr)
    return _glue_result(ctx, rc, "dc_debug_nms_multi", out, raise_errors)
