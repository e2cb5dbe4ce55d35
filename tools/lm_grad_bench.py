"""Cost of the language-model gradients (dc_op_lm_grad) next to the scoring forward of the same rows, synthetic data and weights.

The real language model (E = Hd = 512, D = 4096, V = 10,497, L = 15), n in --rows fc7 codes with captions of random length.
dc_op_lm_grad is called straight through the ABI on device buffers allocated once (no gradient leaves the device inside the
timed region).  --warmup calls, then --reps timed calls; host clock around the synchronous call, milliseconds, median.  The split
is the library's own HIP events (dc_debug_lm_grad_stage_ms: forward, loop back through the steps, stacked gradients, embedding
and codes rows), the median over the same calls.  The yardstick is the scoring forward, not the code under test: `forward` of the
split IS the schedule of the paired scorer (plus one copy of c per step), and dc_op_lm_score of the same codes against ONE
full-length caption is timed beside it (every row alive at every step: an upper bound of the paired forward's work).  The
weight-gradient kernel alone is timed through its hook at the shape of dWout (the hook allocates and frees its scratch inside
the timed call, so the rate is a lower bound).  Writes one JSON document.
usage: python tools/lm_grad_bench.py [--rows 98 256] [--reps 50] [--warmup 10] [--out profiles/lm_grad_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MATRIX_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[98, 256])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib, ops
    from densecap_amd.weights import make_synthetic_weights
    m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
    ctx, lib = m.ctx, m.lib
    d = ctx.lm_dims
    E, Hd, D, V, L = d["E"], d["Hd"], d["D"], d["V"], m.seq_length
    med = lambda v: float(np.median(np.asarray(v, np.float64)))
    doc = dict(dims=dict(E=E, Hd=Hd, D=D, V=V, L=L), reps=a.reps, warmup=a.warmup, peak_fp32_matrix_tf=PEAK_FP32_MATRIX_TF, rows={})
    for n in a.rows:
        rng = np.random.default_rng(n)
        codes = np.maximum(rng.standard_normal((n, D)), 0).astype(np.float32)
        lab = np.zeros((n, L), np.int32)
        for r in range(n):
            k = int(rng.integers(1, L + 1))
            lab[r, :k] = rng.integers(1, V + 1, k)
        shapes = {"lm_enc_w": (E, D), "lm_enc_b": (E,), "lm_emb": (V + 2, E), "lstm_w": (E + Hd, 4 * Hd), "lstm_b": (4 * Hd,),
                  "lm_out_w": (V + 1, Hd), "lm_out_b": (V + 1,), "codes": (n, D)}
        xd = ctx.to_device(codes)
        bufs = {k: ctx.empty(s) for k, s in shapes.items()}
        g = _lib.DcLmGrads(**{k: b.ptr for k, b in bufs.items()})
        loss = C.c_double()

        def grad():
            _lib.check(ctx.h, lib.dc_op_lm_grad(ctx.h, xd.ptr, n, lab.ctypes.data, L, 1.0, C.byref(g), C.byref(loss), None), "dc_op_lm_grad")

        full = ctx.to_device(rng.integers(1, V + 1, (1, L)).astype(np.int32))
        sc = ctx.empty((n, 1))

        def score():
            _lib.check(ctx.h, lib.dc_op_lm_score(ctx.h, xd.ptr, n, full.ptr, 1, L, sc.ptr), "dc_op_lm_score")

        for _ in range(a.warmup):
            grad(); score()
        tg, ts, split = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); grad(); tg.append(time.perf_counter() - t0)
            split.append(list(ops.lm_grad_stage_ms(ctx).values()))
            t0 = time.perf_counter(); score(); ts.append(time.perf_counter() - t0)
        sp = np.median(np.asarray(split, np.float64), axis=0)
        # the weight-gradient kernel alone at the shape of dWout: M = all projection rows, N = V + 1, K = Hd
        Mp = int(((lab != 0).sum(1) + 1).sum())
        A = rng.standard_normal((Mp, V + 1)).astype(np.float32); B = rng.standard_normal((Mp, Hd)).astype(np.float32)
        ad, bd, od = ctx.to_device(A), ctx.to_device(B), ctx.empty((V + 1, Hd))
        tw = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            _lib.check(ctx.h, lib.dc_debug_wgrad(ctx.h, ad.ptr, bd.ptr, Mp, V + 1, Hd, od.ptr), "dc_debug_wgrad")
            if i >= a.warmup:
                tw.append(time.perf_counter() - t0)
        wg_ms = 1e3 * med(tw)
        wg_tf = 2.0 * Mp * (V + 1) * Hd / (wg_ms * 1e-3) / 1e12
        fwd = float(sp[0])
        doc["rows"][str(n)] = dict(
            projection_rows=Mp, lm_grad_ms=1e3 * med(tg), loss=loss.value,
            split_ms=dict(zip(("forward", "bptt", "stacked", "rows"), (float(v) for v in sp))),
            lm_score_one_full_caption_ms=1e3 * med(ts), ratio_call_to_own_forward=1e3 * med(tg) / fwd,
            ratio_call_to_lm_score=med(tg) / med(ts),
            wgrad_dWout=dict(M=Mp, N=V + 1, K=Hd, ms=wg_ms, tflops=wg_tf, of_peak=wg_tf / PEAK_FP32_MATRIX_TF))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
