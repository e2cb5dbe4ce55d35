"""A per-row bar for the 2-D gradient tensors, beside the max-norm bars of the gradient tests.

A max-norm over a whole tensor checks the few largest rows only: the `lm_out_w` gradient's non-target rows carry p * h with p
about 1 / V and sit three to four orders of magnitude below the target rows, rarely fed embedding rows sit beside START, border
pixels of `feat` beside pixels under a hundred stacked boxes.  Here every row r is held to

    max_k |dev[r, k] - ref64[r, k]| <= bar * max_k |ref64[r, k]|

and a row whose float64 reference is exactly zero (a never-fed embedding row, a ReLU-dead row, an untouched pixel) must be all
+0.0 bits on the device.  The bar is not a constant: it is FACTOR times the worst per-row ratio of the SAME rules evaluated in
float32 on the CPU against float64 (`bar_from_float32`), per tensor and case, so it comes from the reference alone.  FACTOR = 8
covers the difference in summation order between a blocked MFMA fmaf chain and torch's CPU sums.

Rows: the tensor's rows for the 2-D tensors; `feat` (C, h, w) has one row per pixel over its channels.  Bias vectors are not
compared here: their entries are column sums that cancel (the float32 evaluation itself reaches 7.6e-4 per element on `lstm_b`);
they stay on the max-norm and the column-sum kernel has its own test (tests/test_gpu_bwd_kernels.py)."""
import numpy as np

FACTOR = 8.0
LM_ROW_TENSORS = ("lm_out_w", "lm_emb", "lstm_w", "lm_enc_w", "codes")
RECOG_ROW_TENSORS = ("fc6_w", "fc7_w", "boxreg_w", "feat", "roi_boxes")


def rows_of(name, a):
    """The 2-D view whose rows are compared: `feat` (C, h, w) -> (h * w, C); everything else as it is."""
    a = np.asarray(a)
    if name in ("feat", "dfeat"):
        return np.ascontiguousarray(a.reshape(a.shape[0], -1).T)
    if a.ndim != 2:
        raise ValueError("%s: a per-row comparison needs a 2-D tensor, got %r" % (name, a.shape))
    return a


def row_ratios(x, ref64):
    """Per row max|x - ref64| / max|ref64|, NaN where the reference row is exactly zero; x and ref64 2-D."""
    scale = np.abs(ref64).max(1) if ref64.size else np.zeros(len(ref64))
    err = np.abs(np.asarray(x, np.float64) - ref64).max(1) if ref64.size else np.zeros(len(ref64))
    out = np.full(len(ref64), np.nan)
    live = scale > 0
    out[live] = err[live] / scale[live]
    out[live & ~np.isfinite(err)] = np.inf                      # a NaN or an infinity on the device is a miss, not a skip
    return out


def worst(ratios):
    return float(np.nanmax(ratios)) if (~np.isnan(ratios)).any() else 0.0


def bar_from_float32(name, ref32, ref64):
    """FACTOR times the float32 evaluation's worst per-row ratio against float64 (0.0 for a tensor without a non-zero row)."""
    return FACTOR * worst(row_ratios(rows_of(name, ref32), rows_of(name, ref64)))


def zero_rows_are_plus_zero(x, ref64):
    """The rows of x (float32, 2-D) whose reference row is exactly zero hold +0.0 bits only: the list of offending rows."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    dead = np.flatnonzero(~np.abs(ref64).astype(bool).any(1)) if ref64.size else np.zeros(0, np.int64)
    return [int(r) for r in dead if x[r].view(np.uint32).any()]


def check_rows(name, dev, ref64, bar):
    """(worst per-row ratio, failures) of a device tensor: failures lists (row, ratio) above the bar and (row, "not +0.0") for a
    zero reference row that is not all +0.0 bits.  An empty list passes."""
    d, r = rows_of(name, dev), rows_of(name, ref64)
    if d.shape != r.shape:
        raise ValueError("%s: shapes %r and %r" % (name, d.shape, r.shape))
    ratios = row_ratios(d, r)
    with np.errstate(invalid="ignore"):
        over = np.flatnonzero(ratios > bar)                     # (NaN compares false: the zero rows are the next check's)
    bad = [(int(i), float(ratios[i])) for i in over[:8]]
    bad += [(i, "not +0.0") for i in zero_rows_are_plus_zero(d, r)[:8]]
    return worst(ratios), bad


def assert_rows(what, tensors, dev, ref64, ref32):
    """Every tensor of `tensors` through check_rows at its own bar; prints worst ratio and bar per tensor; returns them."""
    out, bad = {}, {}
    for k in tensors:
        bar = bar_from_float32(k, ref32[k], ref64[k])
        w, bad[k] = check_rows(k, dev[k], ref64[k], bar)
        out[k] = (w, bar)
    print("per-row %s: " % what + ", ".join("%s %.2e (bar %.2e)" % (k, w, b) for k, (w, b) in out.items()))
    for k in tensors:
        assert not bad[k], (what, k, "bar %.3e" % out[k][1], bad[k])
    return out
