"""Cost of the evaluation's matching (dc_op_eval_match) next to the forward it follows, synthetic data and weights.

For a group of 8 images: dc_op_eval_match at (B, M) = (300, 50), (1000, 50), (1000, 300) detections / ground-truth boxes per image
(ground truth in clusters of 4, detections jittered copies and far boxes: tests/eval_rules.py), inputs on the device before the
clock starts, the call synchronous; and, in the same process, the unchanged dc_forward_images of 8 images of 600x720 at 1000
proposals (lanes 2, group 4: run_model's defaults).  The two are timed alternately; times are the median of --reps runs, host
clock, milliseconds.  Writes one JSON document: the rows and the ratio eval_match / forward.
usage: python tools/eval_match_bench.py [--reps 7] [--out profiles/eval_match_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    from tests import eval_rules as R
    n = a.images
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    m.setLanes(2); m.setGroup(4)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    ctx, lib, h = m.ctx, m.lib, m.ctx.h
    dev_imgs = [ctx.to_device(np.ascontiguousarray(make_synthetic_image(600, 720, i), np.float32)) for i in range(n)]
    kept = []

    def forward():
        kept[:] = [len(o[0]) for o in m.forward_images_device(dev_imgs)]
    rng = np.random.default_rng(0)
    rows = []
    for B, M in ((300, 50), (1000, 50), (1000, 300)):
        gts = [R.clustered_gt(rng, M, 4) for _ in range(n)]
        dets = [R.detections_for(rng, g, B) for g in gts]
        scs = [rng.uniform(0, 1, B).astype(np.float32) for _ in range(n)]
        off = lambda k: np.arange(n + 1, dtype=np.int32) * k
        dbd, dsd, gbd = ctx.to_device(np.concatenate(dets)), ctx.to_device(np.concatenate(scs)), ctx.to_device(np.concatenate(gts))
        dod, god = ctx.to_device(off(B)), ctx.to_device(off(M))
        order, ov, grp = ctx.empty((n * B,), np.int32), ctx.empty((n * B,), np.float64), ctx.empty((n * B,), np.int32)
        ok, gg, ng, mb = ctx.empty((n * B,), np.uint8), ctx.empty((n * M,), np.int32), ctx.empty((n,), np.int32), ctx.empty((n * M, 4), np.float64)

        def match():
            _lib.check(h, lib.dc_op_eval_match(h, dbd.ptr, dsd.ptr, dod.ptr, gbd.ptr, god.ptr, n, C.c_float(0.7), 1, order.ptr, ov.ptr,
                                               grp.ptr, ok.ptr, gg.ptr, ng.ptr, mb.ptr), "dc_op_eval_match")
        match(); forward()
        tm, tf = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); match(); tm.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); forward(); tf.append(time.perf_counter() - t0)
        em, fm = float(np.median(tm)) * 1e3, float(np.median(tf)) * 1e3
        rows.append(dict(images=n, B=B, M=M, mean_groups=float(ng.numpy().mean()), ok_share=float(ok.numpy().mean()),
                         eval_match_ms=em, eval_match_ms_all=[t * 1e3 for t in tm], forward_images_ms=fm,
                         forward_kept_per_image=float(np.mean(kept)), eval_over_forward=em / fm))
        print(json.dumps(rows[-1]), flush=True)
    m.ctx.close()
    doc = dict(what="dc_op_eval_match against dc_forward_images, %d images of 600x720, 1000 proposals, lanes 2, group 4" % n,
               reps=a.reps, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
