"""Cost of dc_loss_gradients next to dc_forward_losses of the same image, synthetic data and weights.

The real model (D = 4096, V = 10,497, L = 15) on a 720 x 600 image with 50 ground-truth boxes and batch_size 256 -- the shape
behind DESIGN.md §15's forward time.  Both calls go straight through the ABI; the gradient buffers are device buffers allocated
once (no gradient leaves the device inside the timed region).  --warmup calls, then --reps timed calls; host clock around the
synchronous call, milliseconds, median.  The yardstick is dc_forward_losses on the same build, timed in the same loop.  The split
of the backward is the library's own HIP events (dc_debug_lm_grad_stage_ms and dc_debug_recog_grad_stage_ms), the median over the
same calls.  dc_op_roi_pool_grad alone is timed at --roi-rows rows on a 38 x 45 x 512 map (boxes scattered over the image, a
third of them jittered copies of four boxes, as positives gather around ground-truth boxes).  Writes one JSON document.
usage: python tools/recog_grad_bench.py [--reps 50] [--warmup 10] [--roi-rows 256 1024] [--out profiles/recog_grad_bench.json]"""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--roi-rows", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib, ops
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    ctx, lib = m.ctx, m.lib
    d = ctx.lm_dims
    E, Hd, D, V, L = d["E"], d["Hd"], d["D"], d["V"], m.seq_length
    H, W, G, batch = 600, 720, 50, 256
    med = lambda v: float(np.median(np.asarray(v, np.float64)))
    rng = np.random.default_rng(0)
    img = np.ascontiguousarray(make_synthetic_image(H, W, 5), dtype=np.float32)
    # ground truth = jittered RPN boxes of the image itself, so that the sampler finds positives (a first pass fetches the boxes)
    o = ops.loss_opts(batch_size=batch)
    gt0 = np.stack([rng.uniform(80, W - 80, G), rng.uniform(80, H - 80, G), rng.uniform(40, 200, G), rng.uniform(40, 200, G)], 1).astype(np.float32)
    lab = np.zeros((G, L), np.int32)
    for r in range(G):
        k = int(rng.integers(1, L + 1))
        lab[r, :k] = rng.integers(1, V + 1, k)
    m.forward_losses(img, gt0, lab, batch_size=batch)
    h, w = ops.feature_size(ctx, H, W)
    boxes = m.debug_fetch("loss_rpn_boxes", (m.num_anchors * h * w, 4))[0]
    ok = np.nonzero((boxes[:, 2] > 30) & (boxes[:, 3] > 30) & (boxes[:, 0] > 60) & (boxes[:, 0] < W - 60) & (boxes[:, 1] > 60) & (boxes[:, 1] < H - 60))[0]
    gt = (boxes[ok[np.linspace(0, len(ok) - 1, G).astype(int)]] * (1 + 0.02 * rng.uniform(-1, 1, (G, 4)))).astype(np.float32)
    idev = ctx.to_device(img)
    rb = ops._recog_bufs(ctx, D, h, w, batch)
    lshapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
               "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (batch, D)}
    lb = {k: ctx.empty(s) for k, s in lshapes.items()}
    rg = _lib.DcRecogGrads(**{k: v.ptr for k, v in rb.items()})
    lg = _lib.DcLmGrads(**{k: v.ptr for k, v in lb.items()})
    out_g, out_f = _lib.DcLosses(), _lib.DcLosses()

    def grad():
        _lib.check(ctx.h, lib.dc_loss_gradients(ctx.h, idev.ptr, H, W, 1, gt.ctypes.data, lab.ctypes.data, G, L, C.byref(o), None,
                                                C.byref(out_g), None, C.byref(rg), C.byref(lg)), "dc_loss_gradients")

    def fwd():
        _lib.check(ctx.h, lib.dc_forward_losses(ctx.h, idev.ptr, H, W, 1, gt.ctypes.data, lab.ctypes.data, G, L, C.byref(o), None,
                                                C.byref(out_f), None), "dc_forward_losses")

    for _ in range(a.warmup):
        grad(); fwd()
    tg, tf, s_lm, s_rg = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); grad(); tg.append(time.perf_counter() - t0)
        s_lm.append(list(ops.lm_grad_stage_ms(ctx).values())); s_rg.append(list(ops.recog_grad_stage_ms(ctx).values()))
        t0 = time.perf_counter(); fwd(); tf.append(time.perf_counter() - t0)
    sl, sr = np.median(np.asarray(s_lm, np.float64), axis=0), np.median(np.asarray(s_rg, np.float64), axis=0)
    doc = dict(image=[H, W], gt_boxes=G, batch_size=batch, dims=dict(E=E, Hd=Hd, D=D, V=V, L=L), reps=a.reps, warmup=a.warmup,
               num_pos=int(out_g.num_pos), num_neg=int(out_g.num_neg), total_loss=out_g.total_loss,
               same_losses_as_forward=bool(out_g.total_loss == out_f.total_loss),
               loss_gradients_ms=1e3 * med(tg), forward_losses_ms=1e3 * med(tf), ratio=med(tg) / med(tf),
               lm_grad_split_ms=dict(zip(("forward", "bptt", "stacked", "rows"), (float(v) for v in sl))),
               recog_grad_split_ms=dict(zip(("heads_fc", "dpool", "roi_scatter", "roi_boxes"), (float(v) for v in sr))),
               roi_pool_grad={})
    # ---- dc_op_roi_pool_grad alone ----
    feat = ctx.to_device(rng.standard_normal((h, w, 512)).astype(np.float32))
    for B in a.roi_rows:
        bx = np.stack([rng.uniform(60, W - 60, B), rng.uniform(60, H - 60, B), rng.uniform(40, 400, B), rng.uniform(40, 400, B)], 1)
        third = B // 3
        bx[:third] = bx[B - 4 + rng.integers(0, 4, third)] * (1 + 0.05 * rng.uniform(-1, 1, (third, 4)))
        bd = ctx.to_device(bx.astype(np.float32))
        dd = ctx.to_device(rng.standard_normal((B, 7, 7, 512)).astype(np.float32))
        df, db = ctx.empty((h, w, 512)), ctx.empty((B, 4))
        res = {}
        for name, dbp in (("feat_and_boxes", db.ptr), ("feat_only", None)):
            ts = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                _lib.check(ctx.h, lib.dc_op_roi_pool_grad(ctx.h, feat.ptr, h, w, 512, bd.ptr, B, H, W, 7, 7, dd.ptr, df.ptr, dbp), "dc_op_roi_pool_grad")
                if i >= a.warmup:
                    ts.append(time.perf_counter() - t0)
            res[name + "_ms"] = 1e3 * med(ts)
        pix, _, start, _ = ops.roi_tap_index(ctx, bx.astype(np.float32), h, w, H, W)
        lens = np.diff(start)
        res.update(list_median=float(np.median(lens)), list_max=int(lens.max()), taps_in_map=int(start[-1]),
                   dout_bytes=B * 49 * 512 * 4, GBps_over_dout_read_4x=4.0 * B * 49 * 512 * 4 / (res["feat_only_ms"] * 1e-3) / 1e9)
        doc["roi_pool_grad"][str(B)] = res
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
