"""Cost of sampling captions (dc_sample_captions / dc_op_lm_sample_n) at 720x600 / 1000 proposals, synthetic weights.

For S in {1, 8, 32, 128} draws per region at temperature 1: the extra time of dc_sample_captions over dc_forward_test, the
time of dc_op_lm_sample_n alone on the K region codes, and -- the same rows through the same schedule with the other
epilogue -- dc_op_lm_score with Q = S queries of T-1 words (K x S rows, T step GEMMs with the log-sum-exp epilogue) in the
same run: their ratio is what the noise generation costs a step.  Also temperature 0 / S = 1 against the greedy decode
(dc_op_lm_sample) on the same K rows: the price of carrying the log-probability.  Prints one JSON line per measurement.
--only S: just that draw count, a few repetitions of the two ops (for a kernel trace).
--top_k K --top_p P (several pairs: --top_k 40,0 --top_p 1,0.9; K = -1 stands for V + 1): the truncated sampler instead --
for every S, dc_op_lm_sample_n_trunc at each pair beside the fused dc_op_lm_sample_n on the same rows in the same run, and
their ratio (the row route writes the logits and runs two more launches per step).  With --only: a few repetitions of
the first pair and of the fused op.
usage: python tools/sample_bench.py [--reps 5] [--samples 1,8,32,128] [--only S] [--top_k K,.. --top_p P,..] [--out FILE]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", default="1,8,32,128")
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--top_k", default="")
    ap.add_argument("--top_p", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    m = DenseCapModel(W, device=0)
    m.setLanes(1)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    img = np.ascontiguousarray(make_synthetic_image(600, 720, 0), np.float32)
    V, T = m.vocab_size, m.seq_length
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def timed(fn, reps=None):
        fn()
        ts = []
        for _ in range(reps or a.reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    _, feats = m.extractFeatures(img)
    K = len(feats)
    codes_d = m.ctx.to_device(feats)
    rng = np.random.default_rng(0)

    def ops_for(S, temperature=1.0):
        opts = _lib.DcSampleOpts(S, temperature, 1)
        tok = m.ctx.empty((K, S, T), np.int32); lp = m.ctx.empty((K, S))
        q = rng.integers(1, V + 1, (S, T)).astype(np.int32)
        q[:, T - 1] = 0                                  # T-1 words: T projections, T-1 LSTM steps, as a draw
        qd = m.ctx.to_device(q); out = m.ctx.empty((K, S))

        def sample():
            _lib.check(m.ctx.h, m.lib.dc_op_lm_sample_n(m.ctx.h, codes_d.ptr, K, None, C.byref(opts), tok.ptr, lp.ptr),
                       "dc_op_lm_sample_n")

        def score():
            _lib.check(m.ctx.h, m.lib.dc_op_lm_score(m.ctx.h, codes_d.ptr, K, qd.ptr, S, T, out.ptr), "dc_op_lm_score")
        return sample, score, opts

    def trunc_op(S, top_k, top_p):
        opts = _lib.DcSampleOpts(S, 1.0, 1)
        tr = _lib.DcSampleTrunc(top_k, top_p)
        tok = m.ctx.empty((K, S, T), np.int32); lp = m.ctx.empty((K, S)); lq = m.ctx.empty((K, S))

        def sample():
            _lib.check(m.ctx.h, m.lib.dc_op_lm_sample_n_trunc(m.ctx.h, codes_d.ptr, K, None, C.byref(opts), C.byref(tr), tok.ptr,
                                                              lp.ptr, lq.ptr), "dc_op_lm_sample_n_trunc")
        return sample

    if a.top_k or a.top_p:
        ks = [V + 1 if int(x) < 0 else int(x) for x in (a.top_k or "0").split(",")]
        ps = [float(x) for x in (a.top_p or "1").split(",")]
        if len(ks) != len(ps):
            raise SystemExit("--top_k and --top_p take the same number of values")
        if a.only:
            fused, _, _ = ops_for(a.only)
            emit(dict(what="trunc_trace", S=a.only, K=K, rows=K * a.only, top_k=ks[0], top_p=ps[0],
                      op_lm_sample_n_trunc_ms=timed(trunc_op(a.only, ks[0], ps[0]), 3), op_lm_sample_n_ms=timed(fused, 3)))
        else:
            for S in [int(x) for x in a.samples.split(",")]:
                fused, _, _ = ops_for(S)
                f_ms = timed(fused)
                for k, p in zip(ks, ps):
                    t_ms = timed(trunc_op(S, k, p))
                    emit(dict(what="sample_trunc", S=S, K=K, rows=K * S, V1=V + 1, temperature=1.0, top_k=k, top_p=p,
                              op_lm_sample_n_trunc_ms=t_ms, op_lm_sample_n_ms=f_ms, trunc_over_fused=t_ms / f_ms))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(json.dumps(x) for x in lines) + "\n")
        m.ctx.close()
        return
    if a.only:
        sample, score, _ = ops_for(a.only)
        emit(dict(what="trace", S=a.only, K=K, rows=K * a.only, op_lm_sample_n_ms=timed(sample, 3), op_lm_score_ms=timed(score, 3)))
        m.ctx.close()
        return
    fwd_ms = timed(lambda: m.forward_raw(img))
    emit(dict(what="forward_test", H=600, W=720, proposals=1000, K=K, ms=fwd_ms))
    P = m._capacity(600, 720)
    for S in [int(x) for x in a.samples.split(",")]:
        sample, score, opts = ops_for(S)
        r, *_ = m._new_result(P)
        sm = np.zeros((P, S, T), np.int32); sl = np.zeros((P, S), np.float32)

        def full():
            _lib.check(m.ctx.h, m.lib.dc_sample_captions(m.ctx.h, img.ctypes.data, 600, 720, 0, C.byref(opts), C.byref(r),
                                                         sm.ctypes.data, sl.ctypes.data), "dc_sample_captions")
        sc_ms, op_ms, lse_ms = timed(full), timed(sample), timed(score)
        emit(dict(what="sample", S=S, K=K, rows=K * S, temperature=1.0, sample_captions_ms=sc_ms,
                  extra_over_forward_ms=sc_ms - fwd_ms, op_lm_sample_n_ms=op_ms, op_lm_score_same_rows_ms=lse_ms,
                  sample_over_score=op_ms / lse_ms))
    greedy_n, _, _ = ops_for(1, 0.0)
    toks = m.ctx.empty((K, T), np.int32)
    g_ms = timed(greedy_n)
    d_ms = timed(lambda: _lib.check(m.ctx.h, m.lib.dc_op_lm_sample(m.ctx.h, codes_d.ptr, K, toks.ptr), "dc_op_lm_sample"))
    emit(dict(what="greedy", K=K, op_lm_sample_n_t0_ms=g_ms, op_lm_sample_ms=d_ms, ratio=g_ms / d_ms))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    m.ctx.close()


if __name__ == "__main__":
    main()
