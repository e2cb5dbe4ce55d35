"""Dropout restated (docs/SEMANTICS.md, "Dropout"): the counter-based mask on tests/loss_rules.py's Philox, the forward and the
backward of one layer in numpy float32, and the recognition net's training forward with its two Dropout layers in float64 torch
autograd -- tests/recog_grad_rules.py's pooling and criteria around fc6, ReLU, mask, fc7, ReLU, mask and the heads.  The autograd
form takes the masks as inputs, so a test can hand it the rule's masks or wrong ones.

Element (row, col) of layer l is kept iff word col & 3 of philox4x32_10(col >> 2, row, l, 1, seed_lo, seed_hi) is below
T = floor((1 - p) * 2^32), 1 - p in double from the float32 p.  A kept element is x * s with s = 1.0f / (1.0f - p) in float32, a
dropped one +0.0.  The backward reads the dropped activation: dy * s where y > 0, +0.0 elsewhere.

variant= gives WRONG forms for the teeth tests: "no_forward_scale" (kept elements are x, the backward still scales),
"no_backward_scale" (the forward scales, the backward passes dy), and for the masks "shared_mask" (layer 2 drawn as layer 1),
"flat_index" (the counter taken from the flat element index row * cols + col) and "c3_zero" (the sampler's counter space)."""
import math

import numpy as np

from tests import loss_rules as LR
from tests import recog_grad_rules as R

F32 = np.float32
SCALE_VARIANTS = ("no_forward_scale", "no_backward_scale")
MASK_VARIANTS = ("shared_mask", "flat_index", "c3_zero")
VARIANTS = SCALE_VARIANTS + MASK_VARIANTS


def threshold(p):
    """T: an element is kept iff its 32-bit word, as a 64-bit integer, is below it (2^32 where 1 - p rounds to 1 in double)."""
    return int(math.floor((1.0 - float(F32(p))) * 4294967296.0))


def scale(p):
    """s = 1.0f / (1.0f - p), both operations in float32."""
    return F32(1.0) / (F32(1.0) - F32(p))


def words(rows, cols, layer, seed, row0=0, col0=0, c3=1):
    """The 32-bit word of every element of rows [row0, row0 + rows) x columns [col0, col0 + cols): uint32 (rows, cols)."""
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    g0, g1 = col0 >> 2, (col0 + cols + 3) >> 2
    out = np.zeros((rows, (g1 - g0) * 4), np.uint32)
    for r in range(rows):
        for g in range(g0, g1):
            out[r, (g - g0) * 4:(g - g0) * 4 + 4] = LR.philox4x32_10(g, row0 + r, layer, c3, k0, k1)
    return np.ascontiguousarray(out[:, col0 - g0 * 4:col0 - g0 * 4 + cols])


def mask(rows, cols, layer, p, seed, row0=0, col0=0, variant=None):
    """bool (rows, cols): True where the element is kept."""
    T = threshold(p)
    if variant == "flat_index":
        if row0 or col0:
            raise ValueError("flat_index: whole matrices only")
        w = words(1, rows * cols, layer, seed).reshape(rows, cols)
    else:
        w = words(rows, cols, 1 if variant == "shared_mask" else layer, seed, row0, col0, c3=0 if variant == "c3_zero" else 1)
    return w.astype(np.uint64) < np.uint64(T) if T < 2 ** 32 else np.ones((rows, cols), bool)


def apply_mask(x, keep, p):
    """x (float32) through a given mask: x * s where kept, +0.0 elsewhere (a select: a dropped inf or NaN becomes +0.0)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(keep, x * scale(p), F32(0.0)).astype(F32)


def dropout_forward(x, layer, p, seed):
    """nn.Dropout's forward on a (rows, cols) float32 matrix; p = 0 is the identity, bit for bit."""
    x = np.asarray(x, F32)
    if F32(p) == 0:
        return x.copy()
    return apply_mask(x, mask(x.shape[0], x.shape[1], layer, p, seed), p)


def relu_dropout_grad(y, dy, p):
    """The backward of ReLU followed by an in-place Dropout, from the dropped activation y: dy * s where y > 0 (NaN: not), +0.0
    elsewhere; p = 0 is the ReLU's mask alone."""
    y, dy = np.asarray(y, F32), np.asarray(dy, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(y > 0, dy if F32(p) == 0 else dy * scale(p), F32(0.0)).astype(F32)


# ---- the recognition net with its two Dropout layers, torch autograd -------------------------------------------------------------------
def _drop(x, keep, p, variant):
    """x * keep * s; the scale variants take the scale out of the value or out of the gradient alone."""
    import torch
    s = float(scale(p))
    m = torch.as_tensor(np.asarray(keep, np.float64), dtype=x.dtype)
    y = x * m
    if variant == "no_forward_scale":                      # value x * m, gradient m * s
        return y * s - (y * (s - 1.0)).detach()
    if variant == "no_backward_scale":                     # value x * m * s, gradient m
        return y + (y * (s - 1.0)).detach()
    return y * s


def forward(P, feat, boxes, num_pos, targets, g, img_h, img_w, mask1, mask2, p, opts=None, variant=None, coords="float32"):
    """recog_grad_rules.forward with Dropout layer 1 on fc6's ReLU output and layer 2 on fc7's: mask1, mask2 bool (n, fc_dim).
    The heads and <codes_pos, g> read the dropped codes.  Also returns `fc6_out`, the dropped fc6 activation."""
    import torch
    o = dict(LR.DEFAULTS, **(opts or {}))
    w_obj, w_box = float(F32(o["end_objectness_weight"])), float(F32(o["end_box_reg_weight"]))
    n, np_ = boxes.shape[0], int(num_pos)
    pooled = R.roi_pool(feat, boxes, img_h, img_w, 7, 7, None, coords)
    x = pooled.reshape(n, -1)
    y6 = _drop(torch.relu(x @ P["fc6_w"].T + P["fc6_b"]), mask1, p, variant)
    codes = _drop(torch.relu(y6 @ P["fc7_w"].T + P["fc7_b"]), mask2, p, variant)
    obj = (codes @ P["obj_w"].T + P["obj_b"]).reshape(n)
    trans = codes[:np_] @ P["boxreg_w"].T + P["boxreg_b"]
    out = dict(pooled=pooled, fc6_out=y6, codes=codes, obj=obj, trans=trans)
    out.update(R.criteria(obj, trans, boxes[:np_], targets, w_obj, w_box))
    total = out["end_objectness_loss"] + out["end_box_reg_loss"]
    if np_ > 0 and g is not None:
        total = total + (codes[:np_] * g).sum()
    out["total"] = total
    return out


def recog_grad(W, feat, boxes, num_pos, targets, g, img_h, img_w, mask1, mask2, p, opts=None, variant=None, coords="float32",
               dtype=None):
    """numpy in, numpy out, as recog_grad_rules.recog_grad: the ten gradients of R.TENSORS (float64), the two losses, masked_end,
    and the dropped activations `fc6_out` and `codes_fwd` (n, fc_dim) float64."""
    import torch
    dtype = dtype or torch.float64
    with torch.enable_grad():
        P = R._torch_params(W, dtype)
        f = torch.tensor(np.asarray(feat, F32).astype(np.float64), dtype=dtype, requires_grad=True)
        b = torch.tensor(np.asarray(boxes, F32).reshape(-1, 4).astype(np.float64), dtype=dtype, requires_grad=True)
        t = torch.tensor(np.asarray(targets, F32).reshape(-1, 4).astype(np.float64), dtype=dtype)
        gt = None if g is None else torch.tensor(np.asarray(g, F32).astype(np.float64), dtype=dtype)
        out = forward(P, f, b, num_pos, t, gt, img_h, img_w, mask1, mask2, p, opts, variant, coords)
        leaves = [P[k] for k in R.PARAMS] + [f, b]
        grads = torch.autograd.grad(out["total"], leaves, allow_unused=True)
    res = {k: (np.zeros(tuple(v.shape)) if gr is None else gr.double().numpy()) for k, gr, v in zip(R.TENSORS, grads, leaves)}
    res.update(end_objectness_loss=float(out["end_objectness_loss"].detach()), end_box_reg_loss=float(out["end_box_reg_loss"].detach()),
               masked_end=out["masked_end"], total=float(out["total"].detach()), fc6_out=out["fc6_out"].detach().double().numpy(),
               codes_fwd=out["codes"].detach().double().numpy())
    return res


def row_failures(what, dev, ref64, ref32, tensors=None):
    """tests/grad_bars.py's per-row rule at its own bar (8 x the float32 evaluation's worst row), tensor by tensor: {tensor:
    failures} of the tensors that miss it.  The GPU tests assert that it is empty; the teeth tests that it is not."""
    from tests import grad_bars as GB
    bad, line = {}, []
    for k in tensors or GB.RECOG_ROW_TENSORS:
        bar = GB.bar_from_float32(k, ref32[k], ref64[k])
        worst, fails = GB.check_rows(k, dev[k], ref64[k], bar)
        line.append("%s %.2e (bar %.2e)" % (k, worst, bar))
        if fails:
            bad[k] = fails
    print("per-row %s: %s" % (what, ", ".join(line)))
    return bad


def masks_for(n, D, p, seed, variant=None):
    """(mask1, mask2) of an n-row call, by the rule or by a wrong mask variant."""
    v = variant if variant in MASK_VARIANTS else None
    return mask(n, D, 1, p, seed, variant=v), mask(n, D, 2, p, seed, variant=v)
