"""Where in these photos is *a red car*?  Ranks an image's regions by log p(query | region) under the language model
(dc_score_captions: LanguageModel:updateOutput teacher-forced with the query, LanguageModel.lua:106-127, targets of
getTarget :148-167), and the images by their best region.

    python -m densecap_amd.query_regions -input_image photo.jpg -query "a red car" -query "white clouds"
    python -m densecap_amd.query_regions -input_dir imgs -query "w12 w7" -synthetic_weights 1 -output_json out.json

The regions are those run_model reports for the same image and flags.  Output JSON:
    {"queries": [...], "images": [{"image": path, "results": [{"query": q, "words": L, "regions": [top-k of
     {"box": xywh, "score": objectness, "loglik": ..., "loglik_per_word": loglik / (L+1), "caption": the region's own}]}]}],
     "ranking": [{"query": q, "images": [{"image": path, "best_loglik": ..., "best_region": k}, ...best first]}]}

With -localize 1 the per-query regions come from dc_localize_captions instead (docs/SEMANTICS.md, "Localising phrases"): for
every query an NMS ordered by the query's own log-likelihood over ALL proposals, so that the best box for a phrase is not lost
to a neighbour with a higher objectness.

    python -m densecap_amd.query_regions -input_image photo.jpg -query "a red car" -localize 1 -localize_nms_thresh 0.3

Every region then carries "region": its row among the regions run_model reports, or -1 if the final NMS dropped it ("caption"
appears only where region >= 0), and the image ranking goes by the best localised box ("best_box" beside "best_region").
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
    a("-localize", type=int, default=0, help="1: per-query NMS over all proposals (at most -topk boxes per query)")
    a("-localize_nms_thresh", type=float, default=None, help="IoU threshold of the per-query NMS, in [0, 1] (default 0.3)")
    a("-min_objectness", type=float, default=None, help="with -localize: proposals with a lower raw objectness are no candidates")
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


def localize_options(opt):
    """The localisation flags of a parsed command line, checked before any model exists: None without -localize, else the
    keyword arguments of DenseCapModel.localizeCaptions."""
    from .ops import check_localize_args
    if opt.localize not in (0, 1):
        raise SystemExit("-localize must be 0 or 1")
    if not opt.localize:
        if opt.min_objectness is not None or opt.localize_nms_thresh is not None:
            raise SystemExit("-localize_nms_thresh / -min_objectness need -localize 1")
        return None
    thresh = 0.3 if opt.localize_nms_thresh is None else opt.localize_nms_thresh
    try:
        check_localize_args(thresh, opt.topk, opt.min_objectness)
    except ValueError as e:
        raise SystemExit("-localize: %s (max_regions is -topk)" % e)
    return {"nms_thresh": thresh, "max_regions": opt.topk, "min_objectness": opt.min_objectness}


def _localized_images(model, images, queries, ids, lengths, loc):
    out = {"queries": list(queries), "images": [], "ranking": []}
    best = [[] for _ in queries]
    for name, img in images:
        boxes, scores, captions, found = model.localizeCaptions(img, ids, return_captions=True, **loc)
        per = []
        for qi, q in enumerate(queries):
            f = found[qi]
            xywh = xcycwh_to_xywh(f["boxes"]) if len(f["boxes"]) else np.zeros((0, 4), np.float32)
            regions = []
            for j in range(len(xywh)):
                k = int(f["region"][j])
                reg = {"box": [float(v) for v in xywh[j]], "score": float(f["objectness"][j]), "loglik": float(f["loglik"][j]),
                       "loglik_per_word": float(f["loglik"][j]) / (lengths[qi] + 1), "region": k}
                if k >= 0:
                    reg["caption"] = captions[k]
                regions.append(reg)
            per.append({"query": q, "words": lengths[qi], "regions": regions})
            if regions:
                best[qi].append({"image": name, "best_loglik": regions[0]["loglik"], "best_region": regions[0]["region"],
                                 "best_box": regions[0]["box"]})
        out["images"].append({"image": name, "results": per})
    for qi, q in enumerate(queries):
        out["ranking"].append({"query": q, "images": sorted(best[qi], key=lambda e: -e["best_loglik"])})
    return out


def query_images(model, images, queries, topk, localize=None):
    """images: list of (name, (1,3,H,W) float32 preprocessed image).  Returns the result dict (module docstring).
    localize: None, or localize_options' keyword arguments (the regions then come from localizeCaptions)."""
    from .model import encode_captions, words_preprocess
    width = max(1, max(len(words_preprocess(q)) for q in queries))
    ids = encode_captions(queries, model.idx_to_token, width)
    lengths = [int(np.count_nonzero(r)) for r in ids]
    if localize is not None:
        return _localized_images(model, images, queries, ids, lengths, localize)
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
    loc = localize_options(opt)
    from . import DenseCapModel
    model = DenseCapModel(_load_weights(opt), device=opt.gpu)
    model.setTestArgs(rpn_nms_thresh=opt.rpn_nms_thresh, final_nms_thresh=opt.final_nms_thresh,
                      num_proposals=opt.num_proposals)
    paths = get_input_images(opt)
    images = ((p, load_image_caffe(p, opt.image_size)[0]) for p in paths)
    res = query_images(model, images, opt.query, opt.topk, loc)
    txt = json.dumps(res, indent=1)
    if opt.output_json:
        with open(opt.output_json, "w") as f:
            f.write(txt)
    else:
        sys.stdout.write(txt + "\n")
    model.ctx.close()


if __name__ == "__main__":
    main()
