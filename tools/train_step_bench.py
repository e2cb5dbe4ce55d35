"""Cost of dc_train_step next to dc_forward_backward of the same image, and the Adam kernel against a device copy.

The real model (rpn_hidden = 256, k = 12, D = 4096, V = 10,497, L = 15) on a 720 x 600 image with 50 ground-truth boxes and
batch_size 256, set up as tools/rpn_grad_bench.py sets it up.  Calls go straight through the ABI on a device-resident image;
--warmup calls, then --reps timed calls; host clock around the synchronous call, milliseconds; median, 10th / 90th percentile,
minimum.

  forward_backward   before dc_train_begin (a context that never trains), gradients into caller buffers, checkpoint layouts
  train_step         the step; its split is the library's own HIP events (dc_debug_fetch "train_step_ms"): the three stages of the
                     backward (with their host synchronisations), the one Adam launch, the refresh of the derived operands
  adam               dc_op_adam on ONE segment of as many elements as the step updates (28 bytes an element: p, m, v read and
                     written, g read), and hipMemcpy device to device of the same byte count split as a copy moves it (half read,
                     half written), both timed by the host around a synchronous call in the same loop

--tree DIR: time forward_backward and train_step with the package of another checkout (the parent commit's, built), for the A/B
of "must not slow": run it alternating with this tree's in one job.  --cnn_mode M: dc_train_set_cnn(M) before the timed steps
(2: the step with the CNN's backward, decay and Adam; its backward stage from dc_debug_fetch "cnn_grad_ms").  --drop_prob P:
dc_set_dropout(P) before the timed calls (docs/SEMANTICS.md, "Dropout").  --grad_clip X: dc_train_set_grad_clip(X) before the
timed steps (docs/SEMANTICS.md, "Gradient clipping"; the norm pass counts in the "adam" stage of the split).
usage: python tools/train_step_bench.py [--reps 30] [--warmup 5] [--tree DIR] [--drop_prob P] [--grad_clip X]
                                        [--out profiles/train_step_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    a = 1e3 * np.asarray(v, np.float64)
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)),
                min_ms=float(a.min()), n=int(a.size))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", default="")
    ap.add_argument("--cnn_mode", type=int, default=0, help="dc_train_set_cnn before the timed steps (0: the CNN is left alone)")
    ap.add_argument("--drop_prob", type=float, default=0.0,
                    help="dc_set_dropout before the timed calls (0: never called, so that --tree may name a library without it)")
    ap.add_argument("--grad_clip", type=float, default=0.0,
                    help="dc_train_set_grad_clip before the timed steps (0: never called, so that --tree may name a library without it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    from densecap_amd import DenseCapModel, _lib, ops
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    ctx, lib = m.ctx, m.lib
    d = ctx.lm_dims
    E, Hd, D, V, L, k, R = d["E"], d["Hd"], d["D"], d["V"], m.seq_length, d["k"], d["R"]
    H, W, G, batch = 600, 720, 50, 256
    rng = np.random.default_rng(0)
    img = np.ascontiguousarray(make_synthetic_image(H, W, 5), dtype=np.float32)
    # ground truth = jittered RPN boxes of the image itself, so that the sampler finds positives (a first pass fetches the boxes)
    o = ops.loss_opts(batch_size=batch)
    gt0 = np.stack([rng.uniform(80, W - 80, G), rng.uniform(80, H - 80, G), rng.uniform(40, 200, G), rng.uniform(40, 200, G)], 1).astype(np.float32)
    lab = np.zeros((G, L), np.int32)
    for r in range(G):
        n = int(rng.integers(1, L + 1))
        lab[r, :n] = rng.integers(1, V + 1, n)
    m.forward_losses(img, gt0, lab, batch_size=batch)
    h, w = ops.feature_size(ctx, H, W)
    boxes = m.debug_fetch("loss_rpn_boxes", (m.num_anchors * h * w, 4))[0]
    ok = np.nonzero((boxes[:, 2] > 30) & (boxes[:, 3] > 30) & (boxes[:, 0] > 60) & (boxes[:, 0] < W - 60) & (boxes[:, 1] > 60) & (boxes[:, 1] < H - 60))[0]
    gt = (boxes[ok[np.linspace(0, len(ok) - 1, G).astype(int)]] * (1 + 0.02 * rng.uniform(-1, 1, (G, 4)))).astype(np.float32)
    idev = ctx.to_device(img)
    if a.drop_prob:
        m.set_dropout(a.drop_prob)
    rb = ops._recog_bufs(ctx, D, h, w, batch)
    lshapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
               "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (batch, D)}
    lb = {n: ctx.empty(s) for n, s in lshapes.items()}
    pb = ops._rpn_bufs(ctx, k, R, h, w)
    rg = _lib.DcRecogGrads(**{n: v.ptr for n, v in rb.items()})
    lg = _lib.DcLmGrads(**{n: v.ptr for n, v in lb.items()})
    pg = _lib.DcRpnGrads(**{n: v.ptr for n, v in pb.items()})
    out_b, out_t = _lib.DcLosses(), _lib.DcLosses()
    args = (idev.ptr, H, W, 1, gt.ctypes.data, lab.ctypes.data, G, L, C.byref(o), None)

    def fb():
        _lib.check(ctx.h, lib.dc_forward_backward(ctx.h, *args, C.byref(out_b), None, C.byref(rg), C.byref(lg), ops.BOX_REG_DECAY,
                                                  C.byref(pg)), "dc_forward_backward")

    doc = dict(image=[H, W], gt_boxes=G, batch_size=batch, dims=dict(E=E, Hd=Hd, D=D, V=V, L=L, k=k, R=R), reps=a.reps, warmup=a.warmup,
               tree=os.path.abspath(a.tree) if a.tree else "this tree", drop_prob=a.drop_prob)
    doc["forward_backward"] = stats(timed(fb, a.warmup, a.reps))
    doc["num_pos"], doc["num_neg"] = int(out_b.num_pos), int(out_b.num_neg)
    for b in list(rb.values()) + list(lb.values()) + list(pb.values()):      # the step keeps its gradients in an arena of its own
        b.free()
    ops.train_begin(ctx)
    if a.cnn_mode:
        ops.train_set_cnn(ctx, a.cnn_mode)
    if a.grad_clip:
        ops.train_set_grad_clip(ctx, a.grad_clip)
    doc["cnn_mode"], doc["grad_clip"] = a.cnn_mode, a.grad_clip
    split, cnn_ms = [], []

    def ts():
        _lib.check(ctx.h, lib.dc_train_step(ctx.h, *args, C.byref(out_t), None, ops.BOX_REG_DECAY), "dc_train_step")
        split.append(list(ops.train_step_ms(ctx).values()))
        if a.cnn_mode == 2:
            cnn_ms.append(ops.cnn_grad_ms(ctx)[1])

    doc["train_step"] = stats(timed(ts, a.warmup, a.reps))
    sp = np.asarray(split[a.warmup:], np.float64)
    doc["train_step_split_ms"] = {n: dict(median=float(np.median(sp[:, i])), p10=float(np.percentile(sp[:, i], 10)),
                                          p90=float(np.percentile(sp[:, i], 90))) for i, n in enumerate(("backward", "adam", "refresh"))}
    doc["loss_before_the_first_step"], doc["loss_before_the_last_step"] = float(out_b.total_loss), float(out_t.total_loss)
    if cnn_ms:
        doc["cnn_backward_ms"] = float(np.median(cnn_ms[a.warmup:]))
    if a.grad_clip:
        doc["grad_norm"], doc["grad_scale"] = ops.train_grad_norm(ctx)
    ops.train_end(ctx)
    if a.tree or a.cnn_mode or a.drop_prob or a.grad_clip:
        print(json.dumps(doc))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
        return
    # ---- the Adam kernel against a device-to-device copy of the same bytes ----
    n = int(sum(int(np.prod(s)) for name, s in list(lshapes.items()) if name != "codes") + D * 49 * 512 + D + D * D + D + 5 * D + 5 +
            R * 512 * 9 + R + 6 * k * R + 6 * k)
    bytes_adam = 28 * n
    bufs = [ctx.empty((n,)) for _ in range(4)]
    hip = C.CDLL("libamdhip64.so")                                         # (the runtime the library itself is linked against)
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    for b in bufs:
        assert hip.hipMemset(b.ptr, 0, 4 * n) == 0
    src = ctx.empty((bytes_adam // 8,)); dst = ctx.empty((bytes_adam // 8,))
    assert hip.hipMemset(src.ptr, 0, src.nbytes) == 0 and hip.hipDeviceSynchronize() == 0
    to = ops.train_opts()
    ta, tc, step = [], [], [0]

    def adam():
        step[0] += 1
        _lib.check(ctx.h, lib.dc_op_adam(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, step[0], C.byref(to)), "dc_op_adam")

    def copy():
        assert hip.hipMemcpy(dst.ptr, src.ptr, src.nbytes, 3) == 0 and hip.hipDeviceSynchronize() == 0

    for i in range(a.warmup + a.reps):
        for fn, acc in ((adam, ta), (copy, tc)):
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            if i >= a.warmup:
                acc.append(dt)
    sa, sc = stats(ta), stats(tc)
    doc["adam"] = dict(elements=n, bytes=bytes_adam, call=sa, copy_of_the_same_bytes=sc,
                       adam_TBps_host_clock=bytes_adam / (sa["median_ms"] * 1e-3) / 1e12,
                       copy_TBps_host_clock=2 * src.nbytes / (sc["median_ms"] * 1e-3) / 1e12,
                       adam_TBps_in_the_step=bytes_adam / (doc["train_step_split_ms"]["adam"]["median"] * 1e-3) / 1e12)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
