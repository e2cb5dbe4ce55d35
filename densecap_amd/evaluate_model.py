"""evaluate_model.lua on the MI355X path: detection mAP on the device, caption mAP through the reference's own file protocol.

Two phases, no subprocess and no Java (METEOR is the reference's eval/meteor_bridge.py plus a jar this tree does not hold):

    # 1. forward + matching on the GPU; writes DIR/input.json (what meteor_bridge.py reads) and DIR/eval_state.json; prints detmap
    python -m densecap_amd.evaluate_model -checkpoint model.t7 -gt_json gt.json -image_dir imgs -output_records DIR
    python -m densecap_amd.evaluate_model -checkpoint model.t7 -data_h5 VG.h5 -data_json VG.json -image_dir imgs -split val \\
        -max_images 100 -output_records DIR
    # 2. (after meteor_bridge.py turned DIR/input.json into output.json) no GPU: prints the full result, like eval_split's ap_results
    python -m densecap_amd.evaluate_model -records DIR -caption_scores output.json

Ground truth: -gt_json {img_name: {"boxes": [[x,y,w,h],..], "captions": [..]}} in ORIGINAL pixels (scaled to the resized frame the
way the image itself is scaled, then read like run_model's -input_boxes), or the reference's dataset pair -data_h5 / -data_json
(`boxes` xcycwh already in the -image_size frame, `labels`, `img_to_first_box`, `img_to_last_box`, `split`; `/images` is never
read: the pixels come from -image_dir through idx_to_filename).  The HDF5 reader is the project's minimal one: it reads files of
hdf5_min.write_hdf5's layout (classic superblock, contiguous datasets); files written by h5py itself have not been read with it.

-losses 1 adds eval_split's validation losses (eval/eval_utils.lua:54-59,78-81): every image also runs the training forward
(DenseCapModel.forward_losses; docs/SEMANTICS.md, "Validation losses") against its ground truth -- the dataset's label rows as
they are with -data_h5, the -gt_json captions tokenised like query_regions' queries (unknown words become <UNK>), cut to the
model's seq_length and zero-padded -- and the six losses, averaged over the images, are printed as `loss_results`, added to the
result under that key and kept in eval_state.json, so that the second phase reports them again.  The sampler's settings and the
five weights are train_opts.lua's, with its defaults; -loss_seed selects the sampler's draws.  -drop_prob P runs that forward
under Dropout (docs/SEMANTICS.md, "Dropout"; default 0, none; the reference's eval_split measures under 0.5); the detections
never drop.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prefix_chars="-", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    # evaluate_model.lua:15-26
    a("-checkpoint", default="data/models/densecap/densecap-pretrained-vgg16.t7")
    a("-data_h5", default="", help="the dataset's HDF5 file (boxes, labels, img_to_first_box, img_to_last_box, split)")
    a("-data_json", default="", help="the dataset's JSON file (idx_to_filename)")
    a("-gpu", type=int, default=0)
    a("-use_cudnn", type=int, default=1, help="accepted for compatibility")
    a("-split", default="val", choices=["val", "test"])
    a("-max_images", type=int, default=-1, help="how many images to evaluate; -1 for the whole split / file")
    a("-rpn_nms_thresh", type=float, default=0.7)
    a("-final_nms_thresh", type=float, default=0.3)
    a("-num_proposals", type=int, default=1000)
    # ---- not reference flags ----
    a("-image_size", type=int, default=720)
    a("-image_dir", default="", help="where the image files are")
    a("-gt_json", default="", help="ground truth per image name, boxes x,y,w,h in original pixels")
    a("-output_records", default="", help="phase 1: directory for input.json and eval_state.json")
    a("-records", default="", help="phase 2: the directory phase 1 wrote")
    a("-caption_scores", default="", help="phase 2: meteor_bridge.py's output.json (key `scores`, one per record)")
    a("-claim_last", type=int, default=1, choices=[0, 1],
      help="1 (default): the reference's used[-1] rule -- a detection that overlaps nothing claims the last merged box; 0: it claims nothing")
    a("-lanes", type=int, default=2)
    a("-group", type=int, default=4)
    a("-io_threads", type=int, default=8)
    a("-math_mode", type=int, default=0, choices=[0, 1])
    a("-caption_order", type=int, default=1, choices=[0, 1])
    a("-synthetic_weights", type=int, default=0, help="1: random weights in checkpoint shapes")
    # ---- validation losses: train_opts.lua:18-40, with its defaults ----
    a("-losses", type=int, default=0, choices=[0, 1], help="1: also compute eval_split's validation losses (a second forward per image)")
    a("-sampler_batch_size", type=int, default=256)
    a("-sampler_high_thresh", type=float, default=0.7)
    a("-sampler_low_thresh", type=float, default=0.3)
    a("-train_remove_outbounds_boxes", type=int, default=1, choices=[0, 1])
    a("-mid_box_reg_weight", type=float, default=0.05)
    a("-mid_objectness_weight", type=float, default=0.1)
    a("-end_box_reg_weight", type=float, default=0.1)
    a("-end_objectness_weight", type=float, default=0.1)
    a("-captioning_weight", type=float, default=1.0)
    a("-loss_seed", type=int, default=0, help="seed of the box sampler's draws (and of the Dropout masks)")
    a("-drop_prob", type=float, default=0.0,
      help="with -losses 1: Dropout after fc6 and fc7 in the training forward, a number in [0, 1); 0 (default) = none, 0.5 = what "
           "the reference's eval_split measures its losses under")
    return p


def loss_options(opt):
    """The flags above as the keyword arguments of DenseCapModel.forward_losses."""
    return dict(batch_size=opt.sampler_batch_size, high_thresh=opt.sampler_high_thresh, low_thresh=opt.sampler_low_thresh,
                remove_outbounds=opt.train_remove_outbounds_boxes, mid_box_reg_weight=opt.mid_box_reg_weight,
                mid_objectness_weight=opt.mid_objectness_weight, end_box_reg_weight=opt.end_box_reg_weight,
                end_objectness_weight=opt.end_objectness_weight, captioning_weight=opt.captioning_weight, seed=opt.loss_seed)


def encode_gt_captions(captions, idx_to_token, seq_length):
    """-gt_json captions -> (M, seq_length) int32 label rows: tokenised the way query_regions tokenises queries (words_preprocess;
    a word the vocabulary lacks becomes <UNK>), cut to seq_length words, zero-padded."""
    from .model import encode_captions, words_preprocess
    token_to_idx = {str(v): int(k) for k, v in (idx_to_token or {}).items()}
    rows = []
    for c in captions:
        words = words_preprocess(c)[:seq_length]
        unknown = [w for w in words if w not in token_to_idx]
        if unknown and "<UNK>" not in token_to_idx:
            raise ValueError("caption %r: word %r is not in the vocabulary (and it has no <UNK>)" % (c, unknown[0]))
        rows.append([token_to_idx.get(w, token_to_idx.get("<UNK>")) for w in words])
    return encode_captions(rows, idx_to_token, seq_length) if rows else np.zeros((0, seq_length), np.int32)


def scaled_size(h0, w0, image_size):
    """image.scale(img, size): the longer side becomes `size` (run_model.image_scale)."""
    imax = max(h0, w0)
    return int(h0 * image_size / imax), int(w0 * image_size / imax)


def read_gt_json(path, names, sizes, image_size):
    """-gt_json -> ({name: (M,4) float32 xcycwh in the resized frame}, {name: captions}).  sizes: {name: (H0, W0)}."""
    from .run_model import xywh_to_xcycwh
    with open(path) as f:
        listed = json.load(f)
    boxes, caps = {}, {}
    for name in names:
        if name not in listed:
            raise SystemExit("-gt_json %s has no entry for image %s" % (path, name))
        e = listed[name]
        b = np.asarray(e["boxes"], np.float64).reshape(-1, 4)
        if len(b) != len(e["captions"]):
            raise SystemExit("-gt_json %s: image %s has %d boxes but %d captions" % (path, name, len(b), len(e["captions"])))
        h0, w0 = sizes[name]
        h, w = scaled_size(h0, w0, image_size)
        b = b * np.asarray([w / w0, h / h0, w / w0, h / h0], np.float64)
        boxes[name] = xywh_to_xcycwh(b.astype(np.float32)) if len(b) else np.zeros((0, 4), np.float32)
        caps[name] = [str(c) for c in e["captions"]]
    return boxes, caps


def read_dataset(data_h5, data_json, split, max_images):
    """The reference's dataset layout (DataLoader.lua:28-76,168-194) -> [(filename, boxes (M,4) xcycwh, labels (M,L))] of the
    split, in index order."""
    from .hdf5_min import read_hdf5
    d = read_hdf5(data_h5, names=("boxes", "labels", "img_to_first_box", "img_to_last_box", "split"))
    with open(data_json) as f:
        info = json.load(f)
    want = {"train": 0, "val": 1, "test": 2}[split]
    out = []
    for ix in np.flatnonzero(np.asarray(d["split"]).reshape(-1) == want):
        r0, r1 = int(d["img_to_first_box"][ix]), int(d["img_to_last_box"][ix])          # 1-based, inclusive
        out.append((info["idx_to_filename"][str(int(ix) + 1)], np.asarray(d["boxes"][r0 - 1:r1], np.float32).reshape(-1, 4),
                    np.asarray(d["labels"][r0 - 1:r1])))
        if 0 < max_images <= len(out):
            break
    return out


def print_results(res):
    if res.get("loss_results"):
        print("loss_results:")
        for k in sorted(res["loss_results"]):
            print("%s: %f" % (k, res["loss_results"][k]))
    if res["map"] is not None:
        for k in sorted(res["ap_breakdown"]):
            print("%s: %f" % (k, res["ap_breakdown"][k]))
        print("mAP: %f" % (100 * res["map"]))
    for k in sorted(res["det_breakdown"]):
        print("%s: %f" % (k, res["det_breakdown"][k]))
    print("detmAP: %f" % (100 * res["detmap"]))


def main(argv=None):
    opt = build_parser().parse_args(argv)
    from . import evaluate as E
    if opt.records:                                   # ---- phase 2: no GPU ----
        if opt.output_records or opt.gt_json or opt.data_h5:
            raise SystemExit("-records is the second phase: it takes -caption_scores only")
        try:
            res = E.evaluate_from_files(opt.records, opt.caption_scores or None)
        except ValueError as e:
            raise SystemExit(str(e))
        print_results(res)
        print(json.dumps(res))
        return 0
    if opt.caption_scores:
        raise SystemExit("-caption_scores belongs to -records")
    if bool(opt.gt_json) == bool(opt.data_h5):
        raise SystemExit("one of -gt_json and -data_h5 (with -data_json) must be given")
    if opt.data_h5 and not opt.data_json:
        raise SystemExit("-data_h5 needs -data_json")
    if not opt.output_records:
        raise SystemExit("-output_records DIR must be given (the records and the state of the first phase)")
    from . import DenseCapModel
    from .run_model import ImagePipeline, load_weights
    weights = load_weights(opt)
    if opt.gt_json:
        from PIL import Image
        with open(opt.gt_json) as f:
            names = sorted(json.load(f))
        if opt.max_images > 0:
            names = names[:opt.max_images]
        sizes = {}
        for n in names:
            with Image.open(os.path.join(opt.image_dir, n)) as im:
                sizes[n] = (im.height, im.width)
        gt_boxes, gt_caps = read_gt_json(opt.gt_json, names, sizes, opt.image_size)
        labels = None
    else:
        ds = read_dataset(opt.data_h5, opt.data_json, opt.split, opt.max_images)
        names = [d[0] for d in ds]
        gt_boxes = {d[0]: d[1] for d in ds}
        labels = {d[0]: d[2] for d in ds}
    paths = [os.path.join(opt.image_dir, n) for n in names]
    num = len(paths)
    model = DenseCapModel(weights, device=opt.gpu)
    model.setLanes(1 if num == 1 else opt.lanes)
    model.setMathMode(opt.math_mode)
    model.setGroup(1 if num == 1 else opt.group)
    model.setCaptionOrder(bool(opt.caption_order))
    # (evaluate_model.lua:39-43 passes max_proposals=, which setTestArgs never reads: the reference runs with the default 1000;
    # here -num_proposals is honoured)
    model.setTestArgs(rpn_nms_thresh=opt.rpn_nms_thresh, final_nms_thresh=opt.final_nms_thresh, num_proposals=opt.num_proposals)
    model.evaluate()
    if labels is not None:
        gt_caps = {n: model.decodeSequence(labels[n]) for n in names}
    all_losses = []
    if opt.losses:
        from . import ops
        from .evaluate import dict_average
        model.set_dropout(opt.drop_prob)
        try:
            gt_labels = labels if labels is not None else {n: encode_gt_captions(gt_caps[n], model.idx_to_token, model.seq_length) for n in names}
        except ValueError as e:
            raise SystemExit(str(e))
    ev = E.DenseCaptioningEvaluator(model.ctx, claim_last=bool(opt.claim_last))
    pipe = ImagePipeline(paths, opt.image_size, opt.gpu, model.ctx, io_threads=opt.io_threads,
                         chunk=max(1, opt.lanes) * max(1, opt.group) * 2, want_rgb=False)
    try:
        for chunk in pipe:
            outs = model.forward_images_device([d for _, d, _ in chunk])
            ns = [names[i] for i, _, _ in chunk]
            if opt.losses:
                # eval_split calls forward_backward on every image (eval/eval_utils.lua:54-59): the training forward, one image a call
                for (_, dev, _), n in zip(chunk, ns):
                    if len(gt_boxes[n]) == 0:
                        print("Image %s has no ground truth: no losses" % n)
                        continue
                    lo = ops.forward_losses(model.ctx, dev, gt_boxes[n], gt_labels[n], on_device=True, **loss_options(opt))
                    all_losses.append({k: lo[k] for k in ops.LOSS_KEYS})
            for _, dev, _ in chunk:
                pipe.recycle(dev)
            # one dc_op_eval_match call for the chunk
            ev.add_result([o[1] for o in outs], [o[0] for o in outs], [model.decodeSequence(o[2]) for o in outs],
                          [gt_boxes[n] for n in ns], [gt_caps[n] for n in ns])
            for (i, _, _), o in zip(chunk, outs):
                print("Processed image %s (%d / %d), detected %d regions" % (names[i], i + 1, num, len(o[0])))
    finally:
        pipe.close()
    loss_results = dict_average(all_losses) if opt.losses else None
    E.write_records(opt.output_records, ev, loss_results)
    res = ev.evaluate()
    if opt.losses:
        res["loss_results"] = loss_results
    print_results(res)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
