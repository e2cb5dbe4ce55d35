"""What caller-supplied boxes cost and save (dc_forward_boxes against dc_forward_test), synthetic weights, one MI355X.

Both paths run in this process on the same image; forward_boxes gets the RoIs forward_test itself pooled ("roi_boxes"), so the
two do the same work after the RPN and return the same bits (asserted).  The difference is the RPN convolution, its heads,
the anchor decode and the RPN NMS against one ingest launch.  Calls alternate (test, boxes, test, boxes ...) after a warm-up
of both; medians over --reps pairs (100: 0.2 .. 0.6 s per path and leg) of host clocks around synchronous calls.
Shapes: 720x600 / 1000 proposals and 480x320 / 50; schedules:
one lane (single image, the latency regime) and two lanes x groups of four over a list of 8 images (ms per image).
Then ms per image for 16 / 64 / 256 / 1000 supplied boxes at 720x600 with final_nms_thresh = 0 ("describe these boxes").
Prints one JSON line per measurement.
usage: python tools/boxes_bench.py [--reps 100] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/boxes_bench.py --profile-calls 20"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clocks():
    """The device's current clocks as rocm-smi prints them (read only), or why they could not be read."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k}
    except Exception as e:                                    # noqa: BLE001 -- a note in the output, not a failure
        return "not read (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--profile-calls", type=int, default=0,
                    help="instead of timing: this many forward_boxes calls at 720x600 / 1000 boxes on one lane, half of them with "
                         "DC_BOXES_CLIP -- the program of a `rocprofv3 --kernel-trace --stats` run (profiles/boxes_kernel_stats.csv)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def alternate(f_test, f_boxes):
        for _ in range(3):
            f_test(); f_boxes()
        t, b = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); f_test(); t1 = time.perf_counter(); f_boxes(); t2 = time.perf_counter()
            t.append(t1 - t0); b.append(t2 - t1)
        q = lambda v, p: float(np.percentile(v, p)) * 1e3     # noqa: E731
        return dict(test_ms=q(t, 50), boxes_ms=q(b, 50), test_p10_p90=[q(t, 10), q(t, 90)], boxes_p10_p90=[q(b, 10), q(b, 90)])

    def rois_of(img, P):
        ref = m.forward_raw(img)
        roi, _ = m.debug_fetch("roi_boxes", (P, 4))
        cnt, _ = m.debug_fetch("rpn_nms_count", (1,), np.int32)
        return ref, roi[:int(cnt[0])].copy()

    if a.profile_calls:
        m.setLanes(1)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
        img = np.ascontiguousarray(make_synthetic_image(600, 720, 0), np.float32)
        _, roi = rois_of(img, 1000)
        for i in range(a.profile_calls):
            m.forward_boxes(img, roi, clip=i >= a.profile_calls // 2)
        m.ctx.close()
        return
    emit(dict(what="clocks", before=clocks()))
    for H, W, P in ((600, 720, 1000), (320, 480, 50)):
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
        imgs = [np.ascontiguousarray(make_synthetic_image(H, W, s), np.float32) for s in range(8)]
        # ---- one lane, one image per call -----------------------------------------------------------------------
        m.setLanes(1); m.setGroup(1)
        ref, roi = rois_of(imgs[0], P)
        out = m.forward_boxes(imgs[0], roi)
        assert all((x == y).all() for x, y in zip(out[:3], ref)), "forward_boxes on forward_test's RoIs must return its bits"
        r = alternate(lambda: m.forward_raw(imgs[0]), lambda: m.forward_boxes(imgs[0], roi))
        st_test = (m.forward_raw(imgs[0]), m.stage_times())[1]
        st_box = (m.forward_boxes(imgs[0], roi), m.stage_times())[1]
        emit(dict(what="forward_boxes_vs_forward_test", H=H, W=W, proposals=P, lanes=1, group=1, images=1, rois=len(roi), K=len(ref[0]),
                  saved_ms=r["test_ms"] - r["boxes_ms"], saved_fraction=1 - r["boxes_ms"] / r["test_ms"],
                  stage_ms_test={k: round(v, 4) for k, v in st_test.items()},
                  stage_ms_boxes={k: round(v, 4) for k, v in st_box.items()}, **r))
        # ---- two lanes x groups of four, a list of 8 images -----------------------------------------------------
        m.setLanes(2); m.setGroup(1)
        both = [rois_of(im, P) for im in imgs]                 # (multi-lane planning: its own RoIs)
        rois = [b[1] for b in both]
        m.setGroup(4)
        outs = m.forward_boxes_images(imgs, rois)
        assert all((x == y).all() for o, (rf, _) in zip(outs, both) for x, y in zip(o[:3], rf))
        r = alternate(lambda: m.forward_images(imgs), lambda: m.forward_boxes_images(imgs, rois))
        per = {k: (v / len(imgs) if not isinstance(v, list) else [x / len(imgs) for x in v]) for k, v in r.items()}
        emit(dict(what="forward_boxes_vs_forward_test", H=H, W=W, proposals=P, lanes=2, group=4, images=len(imgs),
                  per_image=True, saved_ms=per["test_ms"] - per["boxes_ms"], saved_fraction=1 - per["boxes_ms"] / per["test_ms"], **per))
    # ---- "describe these boxes": ms per image as a function of n -------------------------------------------------------
    H, W, P = 600, 720, 1000
    m.setLanes(1); m.setGroup(1)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=P)
    img = np.ascontiguousarray(make_synthetic_image(H, W, 0), np.float32)
    _, roi = rois_of(img, P)
    rng = np.random.default_rng(0)
    while len(roi) < P:                                        # (the RPN NMS may keep fewer than P: fill up with random boxes)
        roi = np.concatenate([roi, np.stack([rng.uniform(1, W, 8), rng.uniform(1, H, 8), rng.uniform(8, 300, 8),
                                             rng.uniform(8, 300, 8)], 1).astype(np.float32)])[:P]
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0, num_proposals=P)
    for n in (16, 64, 256, 1000):
        for cap in sorted({P, max(n, 16)}, reverse=True):      # at the capacity of a 1000-proposal context, and at num_proposals = n
            m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0, num_proposals=cap)
            f = lambda: m.forward_boxes(img, roi[:n])          # noqa: E731
            for _ in range(3):
                f()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); out = f(); ts.append(time.perf_counter() - t0)
            assert len(out[0]) == n
            emit(dict(what="describe_n_boxes", H=H, W=W, n=n, num_proposals=cap, lanes=1, final_nms_thresh=0,
                      ms=float(np.median(ts)) * 1e3, p10_p90=[float(np.percentile(ts, 10)) * 1e3, float(np.percentile(ts, 90)) * 1e3]))
    emit(dict(what="clocks", after=clocks()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    m.ctx.close()


if __name__ == "__main__":
    main()
