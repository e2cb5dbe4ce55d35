"""Cost of dc_op_cnn_grad at 720 x 600: the kept-activation forward of conv3_1 .. conv5_3 and the backward through them.

A 150 x 180 pool2 map and the gradient of conv5_3's output, random, on tests/cnn_grad_rules.py's small model (only the nine
He-scaled convolutions matter).  One warm-up call, then five timed calls, without and with the gradient at conv3_1's input; the
times are the library's own HIP events (dc_debug_fetch "cnn_grad_ms"), milliseconds.  For the per-kernel table of DESIGN.md
section 20 run it under `rocprofv3 --kernel-trace --stats -- python tools/cnn_grad_bench.py`.
usage: python tools/cnn_grad_bench.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from densecap_amd import DenseCapModel, _lib, ops  # noqa: E402
from tests import cnn_grad_rules as CR  # noqa: E402


def main():
    m = DenseCapModel(CR.model_weights(), device=0)
    x4, dfeat = CR.make_chain_case(150, 180, seed=1)
    layers, _ = ops.cnn_shapes(150, 180)
    xd = m.ctx.to_device(np.ascontiguousarray(x4.transpose(1, 2, 0))); gd = m.ctx.to_device(np.ascontiguousarray(dfeat.transpose(1, 2, 0)))
    cg = _lib.DcCnnGrads(); keep = []
    for j, (i, h, w, cin, cout) in enumerate(layers):
        a, b = m.ctx.empty((cout, cin, 3, 3)), m.ctx.empty((cout,)); keep += [a, b]
        cg.conv_w[j] = a.ptr.value; cg.conv_b[j] = b.ptr.value
    for want_x in (False, True):
        xb = m.ctx.empty((150, 180, 128)); cg.x = xb.ptr.value if want_x else None
        rows = []
        for it in range(6):
            rc = m.ctx.lib.dc_op_cnn_grad(m.ctx.h, xd.ptr, 150, 180, gd.ptr, C.byref(cg), None)
            assert rc == 0, m.ctx.lib.dc_last_error(m.ctx.h)
            rows.append(ops.cnn_grad_ms(m.ctx))
        r = np.array(rows[1:])
        print("cnn_grad 150x180 want_x=%d: forward ms %s median %.3f; backward ms %s median %.3f; ratio %.2f" % (
            want_x, np.round(r[:, 0], 3).tolist(), np.median(r[:, 0]), np.round(r[:, 1], 3).tolist(), np.median(r[:, 1]),
            np.median(r[:, 1]) / np.median(r[:, 0])))
    m.ctx.close()


if __name__ == "__main__":
    main()
