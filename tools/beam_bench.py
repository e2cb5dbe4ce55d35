"""Cost of the standard beam search (dc_beam_captions / dc_op_lm_beam_n) at 720x600 / 1000 proposals, synthetic weights.

For every beam width B (default 5 and 20): the time dc_beam_captions adds to dc_forward_test (n_best = B, length_alpha 0.7),
the time of dc_op_lm_beam_n alone on the K region codes, and -- for comparison -- the reference-rule search on the same codes:
dc_op_lm_sample under dc_set_beam_size(B).  The two searches alternate inside one timed loop, so that whatever else the host is
doing falls on both; every figure is a median with the smallest and largest repetition beside it (the run-to-run spread).
Prints one JSON line per measurement; --out FILE keeps them.
usage: python tools/beam_bench.py [--reps 7] [--beams 5,20] [--out FILE]"""
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
    ap.add_argument("--beams", default="5,20")
    ap.add_argument("--alpha", type=float, default=0.7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import DenseCapModel, _lib
    from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    m = DenseCapModel(W, device=0)
    m.setLanes(1)
    m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.3, num_proposals=1000)
    img = np.ascontiguousarray(make_synthetic_image(600, 720, 0), np.float32)
    T = m.seq_length
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def stats(ts):
        ts = np.asarray(ts) * 1e3
        return dict(ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()))

    def timed(fns):
        """Every function once unmeasured, then `reps` rounds in which they alternate: {name: stats}."""
        for fn in fns.values():
            fn()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter(); fn(); ts[k].append(time.perf_counter() - t0)      # every call ends in a synchronise
        return {k: stats(v) for k, v in ts.items()}

    _, feats = m.extractFeatures(img)
    K = len(feats)
    codes_d = m.ctx.to_device(feats)
    P = m._capacity(600, 720)
    for B in [int(x) for x in a.beams.split(",")]:
        opts = _lib.DcBeamOpts(B, B, a.alpha)
        cap = m.ctx.empty((K, B, T), np.int32); lp = m.ctx.empty((K, B))
        toks = m.ctx.empty((K, T), np.int32)
        r, *keep = m._new_result(P)
        hc = np.zeros((P, B, T), np.int32); hl = np.zeros((P, B), np.float32)

        def std_op():
            _lib.check(m.ctx.h, m.lib.dc_op_lm_beam_n(m.ctx.h, codes_d.ptr, K, C.byref(opts), cap.ptr, lp.ptr), "dc_op_lm_beam_n")

        def ref_op():
            m.setBeamSize(B)
            _lib.check(m.ctx.h, m.lib.dc_op_lm_sample(m.ctx.h, codes_d.ptr, K, toks.ptr), "dc_op_lm_sample")
            m.setBeamSize(0)

        def full():
            _lib.check(m.ctx.h, m.lib.dc_beam_captions(m.ctx.h, img.ctypes.data, 600, 720, 0, C.byref(opts), C.byref(r),
                                                       hc.ctypes.data, hl.ctypes.data), "dc_beam_captions")

        t = timed(dict(forward=lambda: m.forward_raw(img), beam_captions=full, std=std_op, ref=ref_op))
        finished = float((cap.numpy() == m.vocab_size + 1).any(axis=2).mean())
        emit(dict(what="beam_std", B=B, n_best=B, length_alpha=a.alpha, H=600, W=720, proposals=1000, K=K, rows=K * B, reps=a.reps,
                  forward_test=t["forward"], beam_captions=t["beam_captions"],
                  extra_over_forward_ms=t["beam_captions"]["ms"] - t["forward"]["ms"],
                  op_lm_beam_n=t["std"], op_lm_sample_reference_rule=t["ref"],
                  std_over_reference_rule=t["std"]["ms"] / t["ref"]["ms"], hypotheses_finished=finished))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    m.ctx.close()


if __name__ == "__main__":
    main()
