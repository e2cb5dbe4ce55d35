"""Cost of localising phrases (dc_op_nms_multi / dc_localize_captions), synthetic data and weights.

Op level: dc_op_nms_multi (one mask launch + one scan launch, a workgroup per query) against Q successive dc_op_nms calls on the
same boxes and score columns -- what a caller had before -- for n in {300, 1000, 2000} clustered boxes, Q in {1, 16, 64, 256},
max_picks in {5, n}.  All inputs are on the device before the clock starts; both sides synchronise before they return; the two
are timed alternately and their picks compared.
End to end: dc_localize_captions against dc_score_captions under final_nms_thresh = 0 (the same forward and the same n x Q
scoring; the difference is the per-query NMS and the result gather) at 720x600 / 1000 proposals.
Prints one JSON line per measurement (times: median of --reps, host clock around synchronous calls, milliseconds).
usage: python tools/localize_bench.py [--reps 7] [--out FILE] [--skip_e2e]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(fa, fb, reps):
    """median milliseconds of fa and fb, one warm-up each, then timed in turn"""
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); fb(); tb.append(time.perf_counter() - t0)
    return float(np.median(ta)) * 1e3, float(np.median(tb)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="300,1000,2000")
    ap.add_argument("--queries", default="1,16,64,256")
    ap.add_argument("--e2e_queries", default="1,16,64")
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from densecap_amd import _lib
    from densecap_amd.ops import Context
    from tests.nms_multi_rules import clustered_boxes
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    ctx = Context(0)
    lib, h = ctx.lib, ctx.h
    rng = np.random.default_rng(0)
    thr = C.c_float(0.3)
    for n in [int(x) for x in a.sizes.split(",")]:
        boxes = clustered_boxes(rng, n, 8)
        bd = ctx.to_device(boxes)
        for Q in [int(x) for x in a.queries.split(",")]:
            s = rng.uniform(0, 1, (n, Q)).astype(np.float32)
            sd = ctx.to_device(s)
            cols = [ctx.to_device(np.ascontiguousarray(s[:, q])) for q in range(Q)]
            for M in (5, n):
                picks = ctx.empty((Q, M), np.int32); cnt = ctx.empty((Q,), np.int32)
                lp = [ctx.empty((M,), np.int32) for _ in range(Q)]; lc = [ctx.empty((1,), np.int32) for _ in range(Q)]

                def multi():
                    _lib.check(h, lib.dc_op_nms_multi(h, bd.ptr, sd.ptr, None, n, Q, thr, M, picks.ptr, cnt.ptr), "dc_op_nms_multi")

                def loop():
                    for q in range(Q):
                        _lib.check(h, lib.dc_op_nms(h, bd.ptr, cols[q].ptr, None, n, thr, M, lp[q].ptr, lc[q].ptr), "dc_op_nms")
                multi_ms, loop_ms = alternate(multi, loop, a.reps)
                pm, cm = picks.numpy(), cnt.numpy()
                same = all(int(lc[q].numpy()[0]) == int(cm[q]) and np.array_equal(lp[q].numpy()[:cm[q]], pm[q, :cm[q]])
                           for q in range(Q))
                emit(dict(what="op", n=n, Q=Q, max_picks=M, mean_picks=float(cm.mean()), nms_multi_ms=multi_ms, nms_loop_ms=loop_ms,
                          loop_over_multi=loop_ms / multi_ms, same_picks=bool(same)))
    ctx.close()
    if not a.skip_e2e:
        from densecap_amd import DenseCapModel
        from densecap_amd.weights import make_synthetic_image, make_synthetic_weights
        m = DenseCapModel(make_synthetic_weights(seed=1234), device=0)
        m.setLanes(1)
        m.setTestArgs(rpn_nms_thresh=0.7, final_nms_thresh=0.0, num_proposals=1000)
        m._push_test_args()
        img = np.ascontiguousarray(make_synthetic_image(600, 720, 0), np.float32)
        P = 1000
        for Q in [int(x) for x in a.e2e_queries.split(",")]:
            lens = rng.integers(1, 9, Q)
            q = np.zeros((Q, 8), np.int32)
            for i, L in enumerate(lens):
                q[i, :L] = rng.integers(1, m.vocab_size + 1, L)
            r, *_keep = m._new_result(P)
            r.tokens = None
            ll = np.zeros((P, Q), np.float32)
            Mx = 5
            o = _lib.DcLocalizeOpts(0.3, Mx, float("-inf"))
            cnt = np.zeros((Q,), np.int32); lb = np.zeros((Q, Mx, 4), np.float32); lq = np.zeros((Q, Mx), np.float32)
            lo = np.zeros((Q, Mx), np.float32); reg = np.zeros((Q, Mx), np.int32)

            def score():
                _lib.check(m.ctx.h, m.lib.dc_score_captions(m.ctx.h, img.ctypes.data, 600, 720, 0, q.ctypes.data, Q, 8, C.byref(r),
                                                            ll.ctypes.data), "dc_score_captions")

            def localize():
                _lib.check(m.ctx.h, m.lib.dc_localize_captions(m.ctx.h, img.ctypes.data, 600, 720, 0, q.ctypes.data, Q, 8, C.byref(o),
                                                               C.byref(r), cnt.ctypes.data, lb.ctypes.data, lq.ctypes.data,
                                                               lo.ctypes.data, reg.ctypes.data), "dc_localize_captions")
            loc_ms, sc_ms = alternate(localize, score, max(3, a.reps // 2))
            emit(dict(what="e2e", H=600, W=720, proposals=int(r.K), Q=Q, max_regions=Mx, localize_captions_ms=loc_ms,
                      score_captions_all_proposals_ms=sc_ms, extra_ms=loc_ms - sc_ms, mean_picks=float(cnt.mean())))
        m.ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
