"""Cost of the validation losses (dc_forward_losses) next to the test-time forward, synthetic data and weights.

One 600x720 image on the device, 50 ground-truth boxes (half of them jittered copies of RPN boxes, so that positives above the
threshold exist), labels of random length; dc_forward_losses with the reference's defaults and, in the same process, the
unchanged dc_forward_test of the same image at 1000 proposals in single-image mode (lanes 1).  --warmup calls of each, then
--reps timed calls alternating; host clock around the synchronous calls, milliseconds, median.  The split of a losses call is the
library's own HIP events ("loss_stage_ms": trunk + RPN, match + assign + draw, RoI pool + fc, paired scoring, loss terms), the
median over the same calls; dc_stage_times gives the forward's two NMS chains.  Writes one JSON document.
usage: python tools/forward_losses_bench.py [--reps 50] [--warmup 10] [--out profiles/forward_losses_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("trunk_rpn", "match_assign_draw", "roipool_fc", "paired_scoring", "loss_terms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gt", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, ops
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    H, W = 600, 720
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    m.setLanes(1)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    dev = m.ctx.to_device(np.ascontiguousarray(make_synthetic_image(H, W, 0), np.float32))
    rng = np.random.default_rng(0)
    G, L = a.gt, m.seq_length
    gt = np.stack([rng.uniform(40, W - 40, G), rng.uniform(40, H - 40, G), rng.uniform(20, 300, G), rng.uniform(20, 300, G)], 1).astype(np.float32)
    lab = np.zeros((G, L), np.int32)
    for j in range(G):
        n = int(rng.integers(1, L + 1))
        lab[j, :n] = rng.integers(1, m.vocab_size + 1, n)
    ops.forward_losses(m.ctx, dev, gt, lab, on_device=True)
    A = m.num_anchors * 38 * 45
    boxes = m.debug_fetch("loss_rpn_boxes", (A, 4))[0]
    inside = np.nonzero((boxes[:, 0] > 100) & (boxes[:, 0] < W - 100) & (boxes[:, 1] > 100) & (boxes[:, 1] < H - 100) & (boxes[:, 2] < 180) &
                        (boxes[:, 3] < 180) & (boxes[:, 2] > 20) & (boxes[:, 3] > 20))[0]
    pick = inside[np.linspace(0, len(inside) - 1, G // 2).astype(int)]
    gt[:len(pick)] = boxes[pick] + np.float32(1)

    def losses():
        return ops.forward_losses(m.ctx, dev, gt, lab, on_device=True)

    def forward():
        return m.forward_images_device([dev])
    for _ in range(a.warmup):
        r = losses(); forward()
    tl, tf, split, nms = [], [], [], []
    st = np.zeros(5, np.float32)
    for _ in range(a.reps):
        t0 = time.perf_counter(); r = losses(); tl.append(time.perf_counter() - t0)
        assert m.lib.dc_debug_fetch(m.ctx.h, b"loss_stage_ms", st.ctypes.data, 20) == 5
        split.append(st.copy())
        t0 = time.perf_counter(); forward(); tf.append(time.perf_counter() - t0)
        t = dict(m.stage_times())
        nms.append(t.get("rpn_nms", 0.0) + t.get("final_nms_gather", 0.0))
    med = lambda v: float(np.median(np.asarray(v, np.float64), axis=0)) if np.ndim(v) == 1 else np.median(np.asarray(v, np.float64), axis=0)
    sp = med(split)
    doc = dict(image="%dx%d" % (W, H), gt_boxes=G, reps=a.reps, warmup=a.warmup,
               forward_losses_ms=1e3 * med(tl), forward_test_ms=1e3 * med(tf), forward_test_nms_chains_ms=med(nms),
               split_ms={k: float(v) for k, v in zip(STAGES, sp)},
               sampler=dict(num_pos=r["num_pos"], num_neg=r["num_neg"], total_pos=r["total_pos"], total_neg=r["total_neg"], flags=r["flags"]),
               losses={k: r[k] for k in ops.LOSS_KEYS})
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
