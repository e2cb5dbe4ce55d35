"""run_model.lua on the MI355X path.

Same flags, preprocessing and result JSON as the reference's `run_model.lua` (flags :26-61,
`run_image` :64-87, `result_to_json` :89-95, main loop :145-188); only the model object differs.

    python -m densecap_amd.run_model -input_image imgs/elephant.jpg -checkpoint model.t7
    python -m densecap_amd.run_model -input_dir imgs -synthetic_weights 1      # no checkpoint offline

File decode is third-party in the reference too (torch/image over libjpeg); PIL does it here.  `image.scale` is
restated from torch/image's C source (`image_scale` below: separable, interpolating when enlarging, area-averaging when
shrinking -- not PIL's resize) and checked against hand-computed values and the oracle's scalar restatement; no Torch7
binary exists here to pin it further.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys

import numpy as np

VGG_MEAN_BGR = np.array([103.939, 116.779, 123.68], np.float32)   # run_model.lua:73


def build_parser():
    """The reference's flags (run_model.lua:26-61), every one of them, plus the scheduling knobs of this path."""
    p = argparse.ArgumentParser(prefix_chars="-", description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    # Model options
    a("-checkpoint", default="data/models/densecap/densecap-pretrained-vgg16.t7")
    a("-image_size", type=int, default=720)
    a("-rpn_nms_thresh", type=float, default=0.7)
    a("-final_nms_thresh", type=float, default=0.3)
    a("-num_proposals", type=int, default=1000)
    # Input settings
    a("-input_image", default="", help="A path to a single specific image to caption")
    a("-input_dir", default="", help="A path to a directory with images to caption")
    a("-input_split", default="", help="A VisualGenome split identifier to process (train|val|test)")
    a("-splits_json", default="info/densecap_splits.json")             # only used when input_split is given
    a("-vg_img_root_dir", default="", help="root directory for vg images")
    # Output settings
    a("-max_images", type=int, default=100, help="max number of images to process")
    a("-output_dir", default="", help="if given: every image with its first num_to_draw boxes and captions drawn on it")
    a("-num_to_draw", type=int, default=10, help="max number of predictions per image")
    a("-text_size", type=int, default=2)
    a("-box_width", type=int, default=2, help="width of rendered box")
    a("-output_vis", type=int, default=1, help="if 1 then writes files needed for pretty vis into vis/")
    a("-output_vis_dir", default="vis/data")
    # Misc
    a("-gpu", type=int, default=0)
    a("-use_cudnn", type=int, default=1, help="accepted for compatibility; this path has no cuDNN / MIOpen to switch")
    # ---- not reference flags ----
    a("-lanes", type=int, default=2, help="images in flight when several images are processed")
    a("-group", type=int, default=4, help="equal-sized images that share the dense launches (dc_set_group)")
    a("-io_threads", type=int, default=8, help="threads that decode the input files / write the output images")
    a("-host_preprocess", type=int, default=0,
      help="1: image.scale on the host (the NumPy restatement) instead of dc_preprocess_u8; same bits, ~100x slower")
    a("-input_boxes", default="",
      help="a results.json as this tool writes it: every image is described on ITS boxes there (results[i].img_name, "
           "results[i].boxes as x,y,w,h in the resized frame) instead of the RPN's; the output gains `src` per image")
    a("-clip_input_boxes", type=int, default=0, help="1: clip the -input_boxes to the image first and drop the invalid ones")
    a("-timing", type=int, default=0, help="1: print the images/s of the image loop (files in -> results out) at the end")
    a("-math_mode", type=int, default=0, choices=[0, 1],
      help="dc_set_math_mode: 0 = fp32 MFMA (default; the reference's arithmetic), 1 = split-bf16 (opt-in: six bf16 partial products per fp32 multiply-add on the bf16 matrix cores, fp32-class accuracy, ~1.2-1.3x images/s)")
    a("-synthetic_weights", type=int, default=0,
      help="1: random weights in checkpoint shapes (no pretrained .t7 is available offline)")
    a("-caption_order", type=int, default=1, choices=[0, 1],
      help="dc_set_caption_order: 1 (default) = final NMS first, captions only for the boxes it keeps -- one packed decode per group "
           "of images; the outputs are the reference's bit for bit (LSTM rows are independent), ~1.3x images/s at 1000 proposals; "
           "0 = the reference's order (DenseCapModel.lua:127-162: all proposals are captioned, then the final NMS picks)")
    a("-num_samples", type=int, default=0,
      help="N > 0: every image also gets N sampled captions per region (dc_sample_captions; words drawn from "
           "SoftMax(scores / temperature)) and their log-probabilities: `sampled_captions` / `sampled_logprobs` in results.json; "
           "0 (default): output as without the flag")
    a("-temperature", type=float, default=1.0, help="temperature of -num_samples: 0.01..100, or 0 with -num_samples 1 (the greedy rule)")
    a("-sample_seed", type=int, default=0, help="seed of -num_samples: image i of the run uses seed + i")
    a("-top_k", type=int, default=0, help="with -num_samples: draw every word from the top_k best-scoring words only (0 = off)")
    a("-top_p", type=float, default=1.0,
      help="with -num_samples: nucleus truncation -- the smallest set of best-scoring words (among the top_k) whose probability "
           "reaches top_p (1 = off).  With either, results.json also carries `sampled_sample_logprobs`: every draw's "
           "log-probability under the truncated distribution it was drawn from")
    a("-num_beams", type=int, default=0,
      help="B > 0: every image also gets the -n_best best captions per region of a standard beam search of width B "
           "(dc_beam_captions; finished hypotheses set aside) and their log-probabilities: `beam_captions` / `beam_logprobs` in "
           "results.json; 0 (default): output as without the flag.  Not together with -num_samples or -input_boxes")
    a("-n_best", type=int, default=0, help="with -num_beams: hypotheses kept per region, 1..B (0 = B)")
    a("-length_alpha", type=float, default=0.0,
      help="with -num_beams: rank the hypotheses by logprob / len^alpha, alpha in [0, 2] (0 = by log-probability)")
    return p


SAMPLING_FLAGS = ("num_samples", "temperature", "sample_seed", "top_k", "top_p")
BEAM_FLAGS = ("num_beams", "n_best", "length_alpha")


def _scale_linear_axis(src, dst_len, axis):
    """torch/image generic/image.c `scaleLinear_rowcol` along one axis of the DoubleTensor image.load returns
    (run_model.lua never sets the default tensor type), with the library's `float` locals:
    longer output  -> linear interpolation at di*(src_len-1)/(dst_len-1) (float weights, double samples and sum), last
                      sample copied;
    shorter output -> area average: output di integrates the source over [di*s, (di+1)*s), s = src_len/dst_len, with
                      fractional end weights in a FLOAT accumulator (every update rounds the double expression to float),
                      divided by the accumulated float weight;
    equal          -> copy.  Vectorised over the other axes; the order of the operations along the axis is the library's."""
    src = np.moveaxis(np.asarray(src, np.float64), axis, 0)
    src_len = src.shape[0]
    F, D = np.float32, np.float64
    if dst_len == src_len:
        out = src.copy()
    elif dst_len > src_len:
        out = np.empty((dst_len,) + src.shape[1:], np.float64)
        if src_len == 1:
            out[:] = src[0]
        else:
            scale = F(src_len - 1) / F(dst_len - 1)
            for di in range(dst_len - 1):
                si_f = F(di) * scale
                si_i = int(si_f)
                si_f = F(si_f - F(si_i))
                out[di] = D(F(1) - si_f) * src[si_i] + D(si_f) * src[si_i + 1]
            out[dst_len - 1] = src[src_len - 1]
    else:
        out = np.empty((dst_len,) + src.shape[1:], np.float64)
        scale = F(src_len) / F(dst_len)
        si0_i, si0_f = 0, F(0)
        for di in range(dst_len):
            si1_f = F(di + 1) * scale
            si1_i = int(si1_f)
            si1_f = F(si1_f - F(si1_i))
            acc = (D(F(1) - si0_f) * src[si0_i]).astype(F)
            n = F(1) - si0_f
            for si in range(si0_i + 1, si1_i):
                acc = (acc.astype(D) + src[si]).astype(F)
                n = F(n + F(1))
            if si1_i < src_len:
                acc = (acc.astype(D) + D(si1_f) * src[si1_i]).astype(F)
                n = F(n + si1_f)
            out[di] = (acc / n).astype(D)
            si0_i, si0_f = si1_i, si1_f
    return np.moveaxis(out, 0, axis)


def image_scale(img_chw, size):
    """torch/image `image.scale(src, size)` with a number (run_model.lua:68): the LONGER side becomes `size`, the
    other keeps the aspect ratio (height = iheight*size/imax, truncated like a Lua number handed to Tensor:resize);
    mode 'bilinear' = `scaleBilinear`: rows first (width), then columns (height), each with `scaleLinear_rowcol`.
    img_chw: (C,H,W) as image.load returns it (a DoubleTensor); returns float64 (`:float()` is the caller's).
    torch/image is not vendored in the reference: restated from its published C source."""
    img = np.asarray(img_chw, np.float64)
    _, ih, iw = img.shape
    imax = max(ih, iw)
    oh, ow = int(ih * size / imax), int(iw * size / imax)
    if oh < 1 or ow < 1:
        raise ValueError("image.scale: %dx%d -> %dx%d" % (iw, ih, ow, oh))
    tmp = _scale_linear_axis(img, ow, 2)          # compress/expand rows first
    return _scale_linear_axis(tmp, oh, 1)         # then columns


def image_load_u8(rgb_u8_hwc):
    """image.load(path, 3) after the file decode: (H,W,3) bytes -> the DoubleTensor (3,H,W) of byte / 255."""
    return np.asarray(rgb_u8_hwc, dtype=np.uint8).astype(np.float64).transpose(2, 0, 1) / np.float64(255.0)


def preprocess_rgb01(img_rgb_chw, image_size):
    """run_model.lua:68-74 after image.load: scale (double), :float(), RGB->BGR, x255, minus the VGG mean.
    (3,H,W) in [0,1] -> ((1,3,H',W') float32, the scaled float32 RGB image)."""
    img = image_scale(img_rgb_chw, image_size).astype(np.float32)
    bgr = img[::-1] * np.float32(255.0) - VGG_MEAN_BGR[:, None, None]
    return np.ascontiguousarray(bgr[None], dtype=np.float32), img


def load_image_caffe(path, image_size):
    """run_model.lua:67-74: image.load(path, 3) (double RGB in [0,1] = byte/255), image.scale (max side = image_size),
    :float(), BGR, x255, minus VGG mean.  Returns (img_caffe (1,3,H,W) float32, scaled RGB uint8 (H,W,3) for the visualiser).
    Only the file DECODE is third-party here (PIL); the resize is image_scale above, not PIL's."""
    from PIL import Image
    im = Image.open(path).convert("RGB")
    img_caffe, scaled = preprocess_rgb01(image_load_u8(np.asarray(im, dtype=np.uint8)), image_size)
    # image.save clamps to [0,1] and writes bytes (x255, truncated)
    rgb = (np.clip(scaled, 0, 1) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0)
    return img_caffe, np.ascontiguousarray(rgb)


def xcycwh_to_xywh(boxes):
    """box_utils.xcycwh_to_xywh (box_utils.lua:441-445), host side like run_model.lua:78."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    hw = (b[:, 2] - np.float32(1)) / np.float32(2)
    hh = (b[:, 3] - np.float32(1)) / np.float32(2)
    x1 = -hw + b[:, 0]; y1 = -hh + b[:, 1]; x2 = hw + b[:, 0]; y2 = hh + b[:, 1]
    return np.stack([x1, y1, x2 - x1 + np.float32(1), y2 - y1 + np.float32(1)], 1)


def xywh_to_xcycwh(boxes):
    """The algebraic inverse of xcycwh_to_xywh above, in fp32: w and h are kept, xc = x + (w - 1) / 2, yc = y + (h - 1) / 2."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    hw = (b[:, 2] - np.float32(1)) / np.float32(2)
    hh = (b[:, 3] - np.float32(1)) / np.float32(2)
    return np.stack([b[:, 0] + hw, b[:, 1] + hh, b[:, 2], b[:, 3]], 1)


def read_input_boxes(path, names):
    """-input_boxes: {img_name: (n,4) fp32 xc,yc,w,h} from a file shaped like the results.json this tool writes.  Every image
    of `names` needs an entry with at least one box; the first that has none is refused by name.  Lists are keyed by file
    name, as results.json is: a name that the file lists twice, or that two input paths share, is refused too."""
    with open(path) as f:
        listed = {}
        for r in json.load(f)["results"]:
            if r["img_name"] in listed:
                raise SystemExit("-input_boxes %s lists image %s more than once" % (path, r["img_name"]))
            listed[r["img_name"]] = r["boxes"]
    out = {}
    for name in names:
        if name in out:
            raise SystemExit("-input_boxes: two input images are called %s; box lists are looked up by file name" % name)
        if name not in listed:
            raise SystemExit("-input_boxes %s has no entry for image %s" % (path, name))
        if len(listed[name]) == 0:
            raise SystemExit("-input_boxes %s lists no boxes for image %s" % (path, name))
        out[name] = xywh_to_xcycwh(listed[name])
    return out


def get_input_images(opt):
    """run_model.lua:115-143."""
    if opt.input_image:
        return [opt.input_image]
    if opt.input_dir:
        return [os.path.join(opt.input_dir, fn) for fn in sorted(os.listdir(opt.input_dir))
                if not fn.startswith(".")]
    if opt.input_split:
        with open(opt.splits_json) as f:
            info = json.load(f)
        return [os.path.join(opt.vg_img_root_dir, "%s.jpg" % i) for i in info[opt.input_split]]
    raise SystemExit("one of input_image, input_dir, or input_split must be provided.")


def result_to_json(boxes_xywh, scores, captions):
    return dict(boxes=[[float(v) for v in r] for r in boxes_xywh],
                scores=[float(s) for s in np.asarray(scores).reshape(-1)], captions=list(captions))


# vis_utils.WAD_COLORS (densecap/vis_utils.lua:5-27 defines the palette; any palette serves the purpose)
_COLORS = [(173, 35, 35), (42, 75, 215), (29, 105, 20), (129, 74, 25), (129, 38, 192), (160, 160, 160), (129, 197, 122),
           (157, 175, 255), (41, 208, 208), (255, 146, 51), (255, 238, 51), (233, 222, 187), (255, 205, 243)]


def render_result(rgb_hwc, boxes_xywh, captions, opt):
    """lua_render_result (run_model.lua:96-113) / vis_utils.densecap_draw (vis_utils.lua:44-79): the first num_to_draw boxes
    as rectangles of box_width pixels with their captions.  The font is PIL's (torch/image's bitmap font is not
    available): same layout, not the same pixels."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(rgb_hwc).copy()
    dr = ImageDraw.Draw(im)
    n = min(opt.num_to_draw, len(boxes_xywh))
    for i in range(n):
        x, y, w, h = (float(v) for v in boxes_xywh[i])
        col = _COLORS[(i + 1) % len(_COLORS)]
        dr.rectangle([x - opt.box_width, y - opt.box_width, x + w + opt.box_width, y + h + opt.box_width], outline=col,
                     width=max(1, int(opt.box_width)))
        try:
            from PIL import ImageFont
            font = ImageFont.load_default(size=6 * max(1, int(opt.text_size)) + 4)
        except Exception:
            font = None
        dr.text((x + opt.box_width + 1, y + opt.box_width + 1), captions[i], fill=col, font=font)
    return im


def _decode_file(path):
    """image.load(path, 3)'s decode (run_model.lua:67): RGB bytes.  PIL here, libjpeg through torch/image there."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class ImagePipeline:
    """The image loop of run_model.lua:160-180 / extract_features.lua:79-91 as a pipeline in front of the device:

        io threads : decode the next files (PIL releases the interpreter lock)            \\  all of it overlaps with the
        prep thread: dc_preprocess_u8 on a context of its own (upload + two launches)      >  device, which is busy with the
        (caller)   : writes results / images of finished chunks on the same io threads    /   previous chunk

    Iterating yields chunks [(index, device image (3,H,W) float32, scaled RGB bytes (H,W,3) or None), ...] in file order;
    give every device image back with recycle().  Round-4 verdict: done serially with a Python resize, the loop ran at
    5-10 images/s in front of a 180 images/s device."""

    def __init__(self, paths, image_size, gpu, model_ctx, io_threads=8, chunk=16, host_preprocess=False, want_rgb=True):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        from . import ops
        from ._lib import check
        self.paths, self.num, self.chunk = list(paths), len(paths), max(1, int(chunk))
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(io_threads)))
        self._decoded = [None] * self.num
        self._ahead = 3 * self.chunk
        self._ready = queue.Queue(maxsize=2 * self.chunk)      # bounds the device memory in flight
        # device buffers are recycled by shape: hipMalloc / hipFree synchronise the device.  A directory is mostly one or two
        # sizes, a Visual Genome split (-input_split) is hundreds of aspect ratios: the pool keeps the MAX_SHAPES most recently
        # used shapes and frees the rest (round-5 advisor finding: it only ever grew)
        import collections
        self._spare, self._lock = collections.OrderedDict(), threading.Lock()
        self._host = bool(host_preprocess)
        self._stop, self._pctx = False, None
        for i in range(min(self._ahead, self.num)):
            self._submit(i)

        def worker():
            try:
                pctx = self._pctx = ops.Context(gpu)     # a dc_ctx is not thread-safe: this thread never touches the model's
                for i in range(self.num):
                    if self._stop:                       # close() before the last image (the consumer raised)
                        break
                    rgb0 = self._decoded[i].result()
                    self._decoded[i] = True
                    self._submit(i + self._ahead)
                    if self._host:
                        img_caffe, sc = preprocess_rgb01(image_load_u8(rgb0), image_size)
                        rgb = np.ascontiguousarray((np.clip(sc, 0, 1) * 255.0).astype(np.uint8).transpose(1, 2, 0)) if want_rgb else None
                        x = np.ascontiguousarray(img_caffe[0], dtype=np.float32)
                        dev = self._take(pctx, x.shape, np.float32)
                        check(pctx.h, pctx.lib.dc_memcpy_h2d(pctx.h, dev.ptr, x.ctypes.data, x.nbytes), "dc_memcpy_h2d")
                        self._ready.put((i, dev, rgb))
                    else:
                        H, W = ops.preprocess_size(pctx.lib, rgb0.shape[0], rgb0.shape[1], image_size)
                        dev = self._take(pctx, (3, H, W), np.float32)
                        rgb_dev = self._take(pctx, (H, W, 3), np.uint8) if want_rgb else None
                        ops.preprocess_u8(pctx, rgb0, image_size, want_rgb=want_rgb, out=dev, rgb=rgb_dev)
                        self._ready.put((i, dev, rgb_dev.numpy() if want_rgb else None))
                        if rgb_dev is not None:
                            self.recycle(rgb_dev)
            except BaseException as e:                   # noqa: BLE001 -- handed to the consuming thread
                self._ready.put(e)
            finally:
                self._ready.put(None)
        self._thread = threading.Thread(target=worker, daemon=True)
        self._thread.start()

    def _submit(self, i):
        if i < self.num and self._decoded[i] is None:
            self._decoded[i] = self.pool.submit(_decode_file, self.paths[i])

    MAX_SHAPES = 8          # distinct (shape, dtype) keys whose spare buffers are kept

    def _take(self, ctx, shape, dtype):
        key, buf, evicted = (tuple(shape), np.dtype(dtype).str), None, []
        with self._lock:
            lst = self._spare.get(key)
            if lst is not None:
                self._spare.move_to_end(key)
                if lst:
                    buf = lst.pop()
            while len(self._spare) > self.MAX_SHAPES:
                evicted += self._spare.popitem(last=False)[1]
        for b in evicted:       # on the preparation thread: the buffers belong to its context
            b.free()
        return buf if buf is not None else ctx.empty(shape, dtype)

    def recycle(self, buf):
        # (never freed from the consuming thread while the preparation thread runs: the buffer belongs to that thread's context)
        with self._lock:
            self._spare.setdefault((buf.shape, buf.dtype.str), []).append(buf)
            self._spare.move_to_end((buf.shape, buf.dtype.str))

    def __iter__(self):
        done, chunk = False, []
        while not done:
            item = self._ready.get()
            if isinstance(item, BaseException):
                raise item
            if item is None:
                done = True
            else:
                chunk.append(item)
            if chunk and (done or len(chunk) >= self.chunk):
                yield chunk
                chunk = []

    def close(self):
        """Stops the preparation thread (also when the consumer gives up early: the thread may be blocked on a full queue),
        frees the spare device buffers and closes the thread's context.  Idempotent."""
        import queue
        self._stop = True
        while True:
            try:
                item = self._ready.get(timeout=0.05) if self._thread.is_alive() else self._ready.get_nowait()
            except queue.Empty:
                if not self._thread.is_alive():
                    break
                continue
            if isinstance(item, tuple):
                self.recycle(item[1])
        self._thread.join()
        self.pool.shutdown(wait=True, cancel_futures=True)
        with self._lock:
            bufs = [b for lst in self._spare.values() for b in lst]
            self._spare.clear()
        for b in bufs:          # the preparation thread has exited: its context is ours now
            b.free()
        if self._pctx is not None:
            self._pctx.close()
            self._pctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def load_weights(opt):
    """-synthetic_weights / -checkpoint -> the weights dict DenseCapModel takes (shared with evaluate_model)."""
    if opt.synthetic_weights:
        from .weights import make_synthetic_weights
        return make_synthetic_weights()
    from . import t7
    if not os.path.exists(opt.checkpoint):
        raise SystemExit("checkpoint %s not found (use -synthetic_weights 1 for random weights)" % opt.checkpoint)
    try:
        ck = t7.load(opt.checkpoint)
    except t7.T7FormatError as e:
        # the two checks that rest on torch.save's habits (object numbering, nothing after the object) must not lock a
        # user out of an unusual but well-formed file: say so and read it again with only the bounds checks on
        print("warning: %s -- reading %s again without the writer-habit checks" % (e, opt.checkpoint), file=sys.stderr)
        ck = t7.load(opt.checkpoint, strict=False)
    return t7.weights_from_checkpoint(ck)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    from . import DenseCapModel, ops
    if opt.num_beams:                      # before the weights are read: a refusal costs nothing
        try:
            ops.check_beam_args(opt.num_beams, opt.n_best or None, opt.length_alpha)
        except ValueError as e:
            raise SystemExit("-num_beams / -n_best / -length_alpha: %s" % e)
        if opt.num_samples:
            raise SystemExit("-num_beams with -num_samples: one run writes either the beam search's captions or the sampler's")
        if opt.input_boxes:
            raise SystemExit("-num_beams with -input_boxes: search on the boxes' codes instead (extract_features_boxes, then "
                             "ops.lm_beam_n)")
    elif opt.n_best or opt.length_alpha:
        raise SystemExit("-n_best / -length_alpha belong to -num_beams")
    weights = load_weights(opt)
    if opt.num_samples:
        try:                               # at start-up, not at the image whose seed would leave the range
            ops.check_sample_args(opt.num_samples, opt.temperature, opt.sample_seed, opt.top_k, opt.top_p)
        except ValueError as e:
            raise SystemExit("-num_samples / -temperature / -sample_seed / -top_k / -top_p: %s" % e)
        if opt.input_boxes:
            raise SystemExit("-num_samples with -input_boxes: sample on the boxes' codes instead (extract_features_boxes, then "
                             "ops.lm_sample_n)")
    truncated = bool(opt.num_samples) and (opt.top_k != 0 or opt.top_p != 1.0)
    paths = get_input_images(opt)
    num = min(len(paths), opt.max_images)
    if opt.num_samples and opt.sample_seed + max(num, 1) - 1 >= 1 << 64:
        raise SystemExit("-sample_seed %d: image i uses seed + i, which leaves 0..2^64-1 within these %d images" % (opt.sample_seed, num))
    in_boxes = read_input_boxes(opt.input_boxes, [os.path.basename(p) for p in paths[:num]]) if opt.input_boxes else None
    model = DenseCapModel(weights, device=opt.gpu)                      # utils.setup_gpus + model:convert
    # one image: single-image mode (lowest latency, like the reference); several: pipelined over the lanes, runs of
    # equal-sized images sharing their dense launches -- results identical to one-by-one processing
    model.setLanes(1 if num == 1 else opt.lanes)
    model.setMathMode(opt.math_mode)
    model.setGroup(1 if num == 1 else opt.group)
    model.setCaptionOrder(bool(opt.caption_order))
    model.setTestArgs(rpn_nms_thresh=opt.rpn_nms_thresh, final_nms_thresh=opt.final_nms_thresh,
                      num_proposals=opt.num_proposals)
    model.evaluate()
    if opt.output_vis == 1:
        os.makedirs(opt.output_vis_dir, exist_ok=True)
    if opt.output_dir:
        os.makedirs(opt.output_dir, exist_ok=True)

    # ---- the loop of run_model.lua:160-180 as a pipeline (ImagePipeline below) ------------------------------------------
    import time
    t_loop = time.perf_counter()
    CHUNK = max(1, opt.lanes) * max(1, opt.group) * 2
    pipe = ImagePipeline(paths[:num], opt.image_size, opt.gpu, model.ctx, io_threads=opt.io_threads, chunk=CHUNK,
                         host_preprocess=bool(opt.host_preprocess), want_rgb=True)
    pool = pipe.pool
    results = [None] * num
    writes = []

    def finish(i, rgb, out):
        """run_model.lua:78-95,170-180 for one image (runs on an io thread while the device works on the next chunk)"""
        boxes, scores, tokens = out[:3]
        xywh = xcycwh_to_xywh(boxes)
        captions = model.decodeSequence(tokens)
        name = os.path.basename(paths[i])
        if opt.output_dir:
            render_result(rgb, xywh, captions, opt).save(os.path.join(opt.output_dir, name))
        if opt.output_vis == 1:
            from PIL import Image
            Image.fromarray(rgb).save(os.path.join(opt.output_vis_dir, name))
            rj = result_to_json(xywh, scores, captions)
            rj["img_name"] = name
            if in_boxes is not None:
                rj["src"] = [int(v) for v in out[3]]         # the row of the image's -input_boxes behind every result row
            if opt.num_samples:
                samples, logprob = out[3], out[4]
                rj["sampled_captions"] = [model.decodeSequence(samples[k]) for k in range(len(samples))]
                rj["sampled_logprobs"] = [[float(v) for v in row] for row in logprob]
                if truncated:
                    rj["sampled_sample_logprobs"] = [[float(v) for v in row] for row in out[5]]
            if opt.num_beams:
                beams, logprob = out[3], out[4]
                rj["beam_captions"] = [model.decodeSequence(beams[k]) for k in range(len(beams))]
                rj["beam_logprobs"] = [[float(v) for v in row] for row in logprob]
            results[i] = rj

    try:
        for chunk in pipe:
            for i, _, _ in chunk:
                print("%d/%d processing image %s" % (i + 1, num, paths[i]))
            if opt.num_samples:
                # image by image: dc_sample_captions runs the forward itself (lane 0), then the draws -- same boxes, scores, captions
                if truncated:
                    outs = [model.sampleCaptions(d, opt.num_samples, opt.temperature, opt.sample_seed + i, top_k=opt.top_k,
                                                 top_p=opt.top_p, want_sample_logprob=True) for i, d, _ in chunk]
                else:
                    outs = [model.sampleCaptions(d, opt.num_samples, opt.temperature, opt.sample_seed + i) for i, d, _ in chunk]
            elif opt.num_beams:
                # image by image, as the sampler: dc_beam_captions runs the forward itself (lane 0), then the search
                outs = [model.beamCaptions(d, opt.num_beams, opt.n_best or None, opt.length_alpha) for _, d, _ in chunk]
            elif in_boxes is None:
                outs = model.forward_images_device([d for _, d, _ in chunk])
            else:
                outs = model.forward_boxes_images_device([d for _, d, _ in chunk],
                                                         [in_boxes[os.path.basename(paths[i])] for i, _, _ in chunk],
                                                         clip=bool(opt.clip_input_boxes))
            for (i, dev, rgb), out in zip(chunk, outs):
                pipe.recycle(dev)
                writes.append(pool.submit(finish, i, rgb, out))
        for w in writes:
            w.result()
    finally:
        pipe.close()
    if opt.timing:
        dt = time.perf_counter() - t_loop
        print("TIMING %d images in %.3f s = %.1f images/s (decode + preprocess + forward + captions + image files; "
              "lanes %d, group %d, %d io threads, %s preprocessing)" % (num, dt, num / dt, opt.lanes, opt.group, opt.io_threads,
                                                                      "host" if opt.host_preprocess else "device"))
    results = [r for r in results if r is not None]
    if results:
        # (without -num_samples the file is what it was before the flag existed: the sampling flags are left out of `opt`)
        # (and without -num_beams, what it was before that flag existed)
        out = dict(results=results, opt={k: v for k, v in vars(opt).items() if (opt.num_samples or k not in SAMPLING_FLAGS)
                                         and (opt.num_beams or k not in BEAM_FLAGS)})
        with open(os.path.join(opt.output_vis_dir, "results.json"), "w") as f:
            json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
