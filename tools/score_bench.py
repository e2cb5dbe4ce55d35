"""Cost of scoring query phrases (dc_score_captions / dc_op_lm_score) at 720x600 / 1000 proposals, synthetic weights.

For Q in {1, 16, 64, 256} queries of 1..8 words: the extra time of dc_score_captions over dc_forward_test, the time of
dc_op_lm_score alone on the K region codes, and the FLOPs it executes over that time against the fp32 MFMA peak (157.3 TF).
FLOPs per region: the image and START steps (2*D*E + 2*E*4Hd + 2*Hd*4Hd) plus sum_q (L_q+1) * 2*Hd*(V+1) + sum_q L_q * 2*Hd*4Hd.
Also the greedy decode of 1000 rows (dc_op_lm_sample) for comparison.  Prints one JSON line per measurement.
usage: python tools/score_bench.py [--reps 5] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", default="1,16,64,256")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    m = DenseCapModel(W, device=0)
    m.setLanes(1)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    img = np.ascontiguousarray(make_synthetic_image(600, 720, 0), np.float32)
    V, Hd, E = m.vocab_size, W["lstm_w"].shape[1] // 4, W["lm_enc_w"].shape[0]
    D = m.fc_dim
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    fwd_ms = timed(lambda: m.forward_raw(img))
    _, feats = m.extractFeatures(img)
    K = len(feats)
    emit(dict(what="forward_test", H=600, W=720, proposals=1000, K=K, ms=fwd_ms))
    codes_d = m.ctx.to_device(feats)
    rng = np.random.default_rng(0)
    for Q in [int(x) for x in a.queries.split(",")]:
        lens = rng.integers(1, 9, Q)
        q = np.zeros((Q, 8), np.int32)
        for i, L in enumerate(lens):
            q[i, :L] = rng.integers(1, V + 1, L)
        P = m._capacity(600, 720)
        r, *_ = m._new_result(P)
        ll = np.zeros((P, Q), np.float32)

        def score():
            _lib.check(m.ctx.h, m.lib.dc_score_captions(m.ctx.h, img.ctypes.data, 600, 720, 0, q.ctypes.data, Q, 8,
                                                        C.byref(r), ll.ctypes.data), "dc_score_captions")
        sc_ms = timed(score)
        qd = m.ctx.to_device(q)
        out = m.ctx.empty((K, Q))

        def op():
            _lib.check(m.ctx.h, m.lib.dc_op_lm_score(m.ctx.h, codes_d.ptr, K, qd.ptr, Q, 8, out.ptr), "dc_op_lm_score")
        op_ms = timed(op)
        flops = K * (2.0 * D * E + 2.0 * E * 4 * Hd + 2.0 * Hd * 4 * Hd)
        flops += K * (float(np.sum(lens + 1)) * 2 * Hd * (V + 1) + float(np.sum(lens)) * 2 * Hd * 4 * Hd)
        tf = flops / (op_ms * 1e-3) / 1e12
        emit(dict(what="score", Q=Q, K=K, rows=K * Q, mean_words=float(lens.mean()), score_captions_ms=sc_ms,
                  extra_over_forward_ms=sc_ms - fwd_ms, op_lm_score_ms=op_ms, gflop=flops / 1e9, tflops=tf,
                  fraction_of_peak=tf / PEAK_TF))
    codes1000 = m.ctx.to_device(np.random.default_rng(1).standard_normal((1000, D)).astype(np.float32))
    toks = m.ctx.empty((1000, m.seq_length), np.int32)
    dec_ms = timed(lambda: _lib.check(m.ctx.h, m.lib.dc_op_lm_sample(m.ctx.h, codes1000.ptr, 1000, toks.ptr), "lm_sample"))
    emit(dict(what="greedy_decode_op", rows=1000, ms=dec_ms))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    m.ctx.close()


if __name__ == "__main__":
    main()
