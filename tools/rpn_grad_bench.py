"""Cost of dc_forward_backward next to dc_loss_gradients and dc_forward_losses of the same image, synthetic data and weights.

The real model (rpn_hidden = 256, k = 12, D = 4096, V = 10,497, L = 15) on a 720 x 600 image with 50 ground-truth boxes and
batch_size 256, as tools/recog_grad_bench.py sets it up.  All three calls go straight through the ABI on device buffers allocated
once; --warmup calls, then --reps timed calls of each in the same loop; host clock around the synchronous call, milliseconds,
median.  The split of the RPN backward is the library's own HIP events (dc_debug_rpn_grad_kept), the median over the same calls;
for the convolution's weight and data gradient the algorithmic FLOPs over that time are given as a fraction of the 157.3 TF fp32
matrix peak.

--compare: the weight gradient of the RPN's convolution (38 x 45, 512 -> 256) two ways, for the design choice of DESIGN.md §18:
the conv3x3_wgrad kernel (dc_debug_conv3x3_wgrad, slices = 0), and the composition the library could already do without it --
nine calls of the weight-gradient hook with leading dimensions (dc_debug_wgrad_ld), one per tap, on a zero-ringed copy of the map
((h + 2) x (w + 2) pixels) and a zero-ringed copy of the gradient, the tap's shift being a row offset into the ringed map, plus
the two padding copies.  The two results are compared first.  The copies are not launched: they are counted at the bytes they
move (each map read and written once) over 4 TB/s, which flatters the composition.  Every hook call is synchronous and
allocates its own partial-tile scratch, so the host clock carries a fixed cost per call: the tool reports the raw medians and
the medians net of an empty hook call (dc_debug_colsum on one element).  The kernels' own times come from running
`--compare-only` under a kernel trace: conv3x3_wgrad_kernel + conv3x3_wgrad_finish_kernel against 9 x (wgrad_kernel +
wgrad_reduce_kernel).
usage: python tools/rpn_grad_bench.py [--reps 50] [--warmup 10] [--compare | --compare-only] [--out profiles/rpn_grad_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def compare(ctx, lib, _lib, ops, reps, warmup):
    h, w, Cin, Cout = 38, 45, 512, 256
    rng = np.random.default_rng(1)
    x = np.abs(rng.standard_normal((h, w, Cin))).astype(np.float32)
    dy = rng.standard_normal((h, w, Cout)).astype(np.float32)
    xd, dd = ctx.to_device(x), ctx.to_device(dy)
    dw = ctx.empty((Cout, Cin, 3, 3))
    # the composition's operands: both maps inside a ring of zero pixels, so that a tap's shift is a row offset and a row that
    # leaves the map reads zeros (from the ring of x) or is multiplied by zeros (the ring of dy)
    hp, wp = h + 2, w + 2
    xp = np.zeros((hp, wp, Cin), np.float32); xp[1:-1, 1:-1] = x
    dp = np.zeros((hp, wp, Cout), np.float32); dp[1:-1, 1:-1] = dy
    lead = wp + 1                                              # rows in front, so that the offset (kh - 1) * wp + (kw - 1) is never negative
    xpf = np.concatenate([np.zeros((lead, Cin), np.float32), xp.reshape(-1, Cin), np.zeros((lead, Cin), np.float32)])
    xpd, dpd = ctx.to_device(xpf), ctx.to_device(dp.reshape(-1, Cout))
    parts = [ctx.empty((Cout, Cin)) for _ in range(9)]
    M = hp * wp

    def new():
        _lib.check(ctx.h, lib.dc_debug_conv3x3_wgrad(ctx.h, xd.ptr, dd.ptr, h, w, Cin, Cout, 0, dw.ptr), "dc_debug_conv3x3_wgrad")

    def old():
        for tap in range(9):
            off = lead + (tap // 3 - 1) * wp + (tap % 3 - 1)
            _lib.check(ctx.h, lib.dc_debug_wgrad_ld(ctx.h, dpd.ptr, Cout, C.c_void_p(xpd.ptr.value + 4 * off * Cin), Cin, M, Cout, Cin,
                                                    parts[tap].ptr, Cin), "dc_debug_wgrad_ld")

    one = ctx.to_device(np.ones((1, 1), np.float32)); o1 = ctx.empty((1,))

    def empty():
        _lib.check(ctx.h, lib.dc_debug_colsum(ctx.h, one.ptr, 1, 1, 1, o1.ptr), "dc_debug_colsum")

    new(); old()
    a = dw.numpy()
    b = np.stack([p.numpy() for p in parts], 2).reshape(Cout, Cin, 3, 3)
    agree = float(np.abs(a - b).max() / np.abs(a).max())
    t = {"new": [], "old": [], "empty": []}
    for i in range(warmup + reps):
        for name, fn in (("new", new), ("old", old), ("empty", empty)):
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            if i >= warmup:
                t[name].append(dt)
    pad_bytes = 2 * (x.nbytes + dy.nbytes)                     # each padding copy reads and writes its map once
    flops = 2.0 * h * w * Cout * 9 * Cin
    return dict(shape=[h, w, Cin, Cout], max_rel_difference=agree, flops=flops,
                conv3x3_wgrad_call_ms=1e3 * med(t["new"]), nine_wgrad_calls_ms=1e3 * med(t["old"]), empty_call_ms=1e3 * med(t["empty"]),
                conv3x3_wgrad_net_ms=1e3 * (med(t["new"]) - med(t["empty"])),
                nine_wgrad_net_ms=1e3 * (med(t["old"]) - 9 * med(t["empty"])),
                padding_copies_ms_at_4TBps=1e3 * pad_bytes / 4e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--compare-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib, ops
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    if a.compare_only:
        ctx = ops.Context(0)
        doc = dict(wgrad_comparison=compare(ctx, ctx.lib, _lib, ops, a.reps, a.warmup))
        print(json.dumps(doc, indent=1))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
        return
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
    rb = ops._recog_bufs(ctx, D, h, w, batch)
    lshapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
               "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (batch, D)}
    lb = {n: ctx.empty(s) for n, s in lshapes.items()}
    pb = ops._rpn_bufs(ctx, k, R, h, w)
    rg = _lib.DcRecogGrads(**{n: v.ptr for n, v in rb.items()})
    lg = _lib.DcLmGrads(**{n: v.ptr for n, v in lb.items()})
    pg = _lib.DcRpnGrads(**{n: v.ptr for n, v in pb.items()})
    out_b, out_g, out_f = _lib.DcLosses(), _lib.DcLosses(), _lib.DcLosses()
    args = (idev.ptr, H, W, 1, gt.ctypes.data, lab.ctypes.data, G, L, C.byref(o), None)

    def fb():
        _lib.check(ctx.h, lib.dc_forward_backward(ctx.h, *args, C.byref(out_b), None, C.byref(rg), C.byref(lg), ops.BOX_REG_DECAY,
                                                  C.byref(pg)), "dc_forward_backward")

    def grad():
        _lib.check(ctx.h, lib.dc_loss_gradients(ctx.h, *args, C.byref(out_g), None, C.byref(rg), C.byref(lg)), "dc_loss_gradients")

    def fwd():
        _lib.check(ctx.h, lib.dc_forward_losses(ctx.h, *args, C.byref(out_f), None), "dc_forward_losses")

    for _ in range(a.warmup):
        fb(); grad(); fwd()
    tb, tg, tf, split = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); fb(); tb.append(time.perf_counter() - t0)
        split.append(list(ops.rpn_grad_kept(ctx)[1].values()))
        t0 = time.perf_counter(); grad(); tg.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); fwd(); tf.append(time.perf_counter() - t0)
    sp = np.median(np.asarray(split, np.float64), axis=0)
    names = ("dheads", "heads", "conv_wgrad", "conv_dgrad")
    flops = 2.0 * h * w * R * 9 * 512
    doc = dict(image=[H, W], gt_boxes=G, batch_size=batch, dims=dict(E=E, Hd=Hd, D=D, V=V, L=L, k=k, R=R), reps=a.reps, warmup=a.warmup,
               num_pos=int(out_b.num_pos), num_neg=int(out_b.num_neg), total_loss=out_b.total_loss,
               same_losses_as_forward=bool(out_b.total_loss == out_f.total_loss == out_g.total_loss),
               forward_backward_ms=1e3 * med(tb), loss_gradients_ms=1e3 * med(tg), forward_losses_ms=1e3 * med(tf),
               rpn_backward_ms=1e3 * (med(tb) - med(tg)),
               rpn_grad_split_ms=dict(zip(names, (float(v) for v in sp))),
               conv_flops=flops,
               conv_wgrad_fraction_of_fp32_matrix_peak=flops / (sp[2] * 1e-3) / (PEAK_TF * 1e12),
               conv_dgrad_fraction_of_fp32_matrix_peak=flops / (sp[3] * 1e-3) / (PEAK_TF * 1e12))
    if a.compare:
        doc["wgrad_comparison"] = compare(ctx, lib, _lib, ops, a.reps, a.warmup)
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
