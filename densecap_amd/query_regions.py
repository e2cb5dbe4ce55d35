"""Where in these photos is *a red car*?  Ranks an image's regions by log p(query | region) under the language model
(dc_score_captions: LanguageModel:updateOutput teacher-forced with the query, LanguageModel.lua:106-127, targets of
getTarget :148-167), and the images by their best region.

    python -m densecap_amd.query_regions -input_image photo.jpg -query "a red car" -query "white clouds"
    python -m densecap_amd.query_regions -input_dir imgs -query "w12 w7" -synthetic_weights 1 -output_json out.json

The regions are those run_model reports for the same image and flags.  Output JSON:
    {"queries": [...], "images": [{"image": path, "results": [{"query": q, "words": L, "regions": [top-k of
     {"box": xywh, "score": objectness, "loglik": ..., "loglik_per_word": loglik / (L+1), "caption": the region's own}]}]}],
     "ranking": [{"query": q, "images": [{"image": path, "best_loglik": ..., "best_region": k}, ...best first]}]}
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .run_model import get_input_images, load_image_caffe, xcycwh_to_xywh


def build_parser():
    p = argparse.ArgumentParser(prefix_chars="-", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    a("-input_image", default="", help="a path to a single image")
    a("-input_dir", default="", help="a path to a directory of images")
    a("-query", action="append", default=[], help="a query phrase (repeat the flag for several)")
    a("-topk", type=int, default=5, help="regions reported per image and query")
    a("-output_json", default="", help="write the result here (default: stdout)")
    # run_model's model and test-argument flags
    a("-checkpoint", default="data/models/densecap/densecap-pretrained-vgg16.t7")
    a("-synthetic_weights", type=int, default=0, help="1: random weights in checkpoint shapes")
    a("-image_size", type=int, default=720)
    a("-rpn_nms_thresh", type=float, default=0.7)
    a("-final_nms_thresh", type=float, default=0.3)
    a("-num_proposals", type=int, default=1000)
    a("-gpu", type=int, default=0)
    return p


def _load_weights(opt):
    if opt.synthetic_weights:
        from .weights import make_synthetic_weights
        return make_synthetic_weights()
    import os
    from . import t7
    if not os.path.exists(opt.checkpoint):
        raise SystemExit("checkpoint %s not found (use -synthetic_weights 1 for random weights)" % opt.checkpoint)
    try:
        ck = t7.load(opt.checkpoint)
    except t7.T7FormatError as e:
        # as run_model: the checks that rest on torch.save's habits must not lock a user out of a well-formed file
        print("warning: %s -- reading %s again without the writer-habit checks" % (e, opt.checkpoint), file=sys.stderr)
        ck = t7.load(opt.checkpoint, strict=False)
    return t7.weights_from_checkpoint(ck)


def query_images(model, images, queries, topk):
    """images: list of (name, (1,3,H,W) float32 preprocessed image).  Returns the result dict (module docstring)."""
    from .model import encode_captions, words_preprocess
    width = max(1, max(len(words_preprocess(q)) for q in queries))
    ids = encode_captions(queries, model.idx_to_token, width)
    lengths = [int(np.count_nonzero(r)) for r in ids]
    out = {"queries": list(queries), "images": [], "ranking": []}
    best = [[] for _ in queries]
    for name, img in images:
        boxes, scores, loglik, captions = model.scoreCaptions(img, ids, return_captions=True)
        xywh = xcycwh_to_xywh(boxes)
        per = []
        for qi, q in enumerate(queries):
            col = loglik[:, qi] if len(boxes) else np.zeros((0,), np.float32)
            order = np.argsort(-col.astype(np.float64), kind="stable")[:topk]
            regions = [{"box": [float(v) for v in xywh[k]], "score": float(scores[k]), "loglik": float(col[k]),
                        "loglik_per_word": float(col[k]) / (lengths[qi] + 1), "caption": captions[k]} for k in order]
            per.append({"query": q, "words": lengths[qi], "regions": regions})
            if len(order):
                best[qi].append({"image": name, "best_loglik": float(col[order[0]]), "best_region": int(order[0])})
        out["images"].append({"image": name, "results": per})
    for qi, q in enumerate(queries):
        out["ranking"].append({"query": q, "images": sorted(best[qi], key=lambda e: -e["best_loglik"])})
    return out


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not opt.query:
        raise SystemExit("give at least one -query")
    if opt.topk < 1:
        raise SystemExit("-topk must be >= 1")
    from . import DenseCapModel
    model = DenseCapModel(_load_weights(opt), device=opt.gpu)
    model.setTestArgs(rpn_nms_thresh=opt.rpn_nms_thresh, final_nms_thresh=opt.final_nms_thresh,
                      num_proposals=opt.num_proposals)
    paths = get_input_images(opt)
    images = ((p, load_image_caffe(p, opt.image_size)[0]) for p in paths)
    res = query_images(model, images, opt.query, opt.topk)
    txt = json.dumps(res, indent=1)
    if opt.output_json:
        with open(opt.output_json, "w") as f:
            f.write(txt)
    else:
        sys.stdout.write(txt + "\n")
    model.ctx.close()


if __name__ == "__main__":
    main()
