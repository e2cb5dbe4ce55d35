"""The backward of a 3x3 / stride 1 / pad 1 convolution restated with float64 torch autograd (docs/SEMANTICS.md, "Convolution
gradients"): y = conv2d(x, w, padding=1) as nn.SpatialConvolution(Cin, Cout, 3, 3, 1, 1, 1, 1) computes it, and the gradients of
<dy, y> with respect to w, the bias and x.  Everything runs under torch.enable_grad(): the oracle turns autograd off when it is
imported.

variant= gives WRONG restatements for the teeth tests: "dx_taps_not_flipped" (dx as the convolution of dy with the transposed
but unflipped weights) and "dw_taps_transposed" (dw with its (kh, kw) axes swapped)."""
import numpy as np

F32 = np.float32
TENSORS = ("dw", "db", "dx")
VARIANTS = ("dx_taps_not_flipped", "dw_taps_transposed")
REL = 1e-4                     # max-norm bar of a device tensor against float64, as the other gradient tests hold


def conv3x3_grad(x, w, dy, dtype="float64", variant=None):
    """x (Cin, h, w), w (Cout, Cin, 3, 3), dy (Cout, h, w) numpy -> {"dw", "db", "dx"} numpy float64, evaluated in `dtype`."""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.enable_grad():
        xt = torch.tensor(np.asarray(x), dtype=dt).requires_grad_(True)
        wt = torch.tensor(np.asarray(w), dtype=dt).requires_grad_(True)
        bt = torch.zeros(wt.shape[0], dtype=dt).requires_grad_(True)
        g = torch.tensor(np.asarray(dy), dtype=dt)
        y = Fn.conv2d(xt[None], wt, bt, padding=1)[0]
        (y * g).sum().backward()
        dx = xt.grad
        if variant == "dx_taps_not_flipped":
            dx = Fn.conv2d(g[None], wt.detach().transpose(0, 1).contiguous(), None, padding=1)[0]
        dw = wt.grad.transpose(2, 3) if variant == "dw_taps_transposed" else wt.grad
    return {"dw": dw.double().numpy().copy(), "db": bt.grad.double().numpy().copy(), "dx": dx.detach().double().numpy().copy()}


def objective(x, w, b, dy):
    """<dy, conv2d(x, w, b)> in float64: what the three gradients are the derivatives of."""
    import torch
    import torch.nn.functional as Fn
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return float((Fn.conv2d(t(x)[None], t(w), t(b), padding=1)[0] * t(dy)).sum())


def rows(name, a):
    """The 2-D view whose rows the per-row bars hold: dw per output channel, dx (Cin, h, w) per pixel."""
    a = np.asarray(a)
    if name == "dw":
        return a.reshape(a.shape[0], -1)
    if name == "dx":
        return np.ascontiguousarray(a.reshape(a.shape[0], -1).T)
    raise ValueError(name)


def one_hot_expected(x, wt, o, y0, x0):
    """(dw, dx) float64 for a dy that is 1 at (o, y0, x0) and 0 elsewhere: the shifted patch of x in row o, the weights of o around
    the pixel."""
    Cin, h, w = x.shape
    dw = np.zeros(wt.shape, np.float64)
    dx = np.zeros(x.shape, np.float64)
    for kh in range(3):
        for kw in range(3):
            yy, xx = y0 + kh - 1, x0 + kw - 1
            if 0 <= yy < h and 0 <= xx < w:
                dw[o, :, kh, kw] = x[:, yy, xx]
                dx[:, yy, xx] = wt[o, :, kh, kw]
    return dw, dx


def make_case(h, w, Cin, Cout, seed):
    """x, w, dy float32 with per-channel scales spread over a decade, so that rows of very different size sit side by side."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((Cin, h, w)) * rng.uniform(0.3, 3.0, (Cin, 1, 1))).astype(F32)
    wt = (rng.standard_normal((Cout, Cin, 3, 3)) * 0.05).astype(F32)
    dy = (rng.standard_normal((Cout, h, w)) * rng.uniform(0.3, 3.0, (Cout, 1, 1))).astype(F32)
    return x, wt, dy


# ---- the RPN's backward (docs/SEMANTICS.md, "RPN gradients") ------------------------------------------------------------------------
# Module by module as the reference composes them: the criteria on the sampled rows (tests/loss_rules.py's formulas), the
# sampler's backward written out as the COPY it is (BoxSamplerHelper.lua:166-177), ApplyBoxTransform:backward
# (ApplyBoxTransform.lua:115-118), the ConcatTable's sum, RegularizeLayer (RegularizeLayer.lua:18-22), and the two 1x1 heads, the
# in-place ReLU and the 3x3 convolution by torch autograd.
RPN_PARAMS = ("rpn_conv_w", "rpn_conv_b", "rpn_box_w", "rpn_box_b", "rpn_score_w", "rpn_score_b")
RPN_TENSORS = RPN_PARAMS + ("feat",)
RPN_ROW_TENSORS = ("rpn_conv_w", "rpn_box_w", "rpn_score_w", "feat")
RPN_VARIANTS = ("dx_taps_not_flipped", "dw_taps_transposed", "sum_not_last", "pos_after_neg", "no_decay", "no_box_w",
                "classes_swapped", "mask_not_zeroed", "mask_out_of_divisor", "relu_mask_from_input")
EDGE = 1e-3                    # distance a generated case keeps from the SmoothL1 kink and from the |target| = 10 mask
HIDDEN_EDGE = 1e-5             # ... and, relative to max|hidden|, of every pre-activation from zero
MID_DEFAULTS = dict(mid_objectness_weight=0.1, mid_box_reg_weight=0.05)


def anchor_rows(W, h, w):
    """(A, 4) float32 (xa, ya, wa, ha), row b = a * h * w + y * w + x, in rpn_decode_kernel's arithmetic."""
    x0, y0, sx, sy = (F32(v) for v in W["field_centers"])
    anc = np.asarray(W["anchors"], F32)
    k = anc.shape[1]
    ys, xs = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    xa, ya = (xs * sx + x0).astype(F32).reshape(-1), (ys * sy + y0).astype(F32).reshape(-1)
    return np.concatenate([np.stack([xa, ya, np.full(h * w, anc[0, a], F32), np.full(h * w, anc[1, a], F32)], 1) for a in range(k)]).astype(F32)


def _forward(W, feat, dt, leaves=None):
    """(hidden_pre, hidden, trans (A,4), scores (A,2)) torch tensors of the RPN's training forward on feat (512,h,w)."""
    import torch
    import torch.nn.functional as Fn
    t = leaves or {n: torch.as_tensor(np.asarray(W[n], np.float64)).to(dt) for n in RPN_PARAMS}
    x = leaves["feat"] if leaves else torch.as_tensor(np.asarray(feat, np.float64)).to(dt)
    k = t["rpn_box_w"].shape[0] // 4
    h, w = x.shape[1:]
    pre = Fn.conv2d(x[None], t["rpn_conv_w"], t["rpn_conv_b"], padding=1)
    hid = torch.relu(pre)
    box = Fn.conv2d(hid, t["rpn_box_w"].reshape(4 * k, -1, 1, 1), t["rpn_box_b"])[0]
    sc = Fn.conv2d(hid, t["rpn_score_w"].reshape(2 * k, -1, 1, 1), t["rpn_score_b"])[0]
    trans = box.reshape(k, 4, h, w).permute(0, 2, 3, 1).reshape(-1, 4)
    scores = sc.reshape(k, 2, h, w).permute(0, 2, 3, 1).reshape(-1, 2)
    return pre[0], hid[0], trans, scores


def _targets(anchors, gt, pos_tgt):
    import torch
    a = torch.as_tensor(anchors.astype(np.float64)); g = torch.as_tensor(np.asarray(gt, F32).astype(np.float64))[pos_tgt]
    return torch.stack([(g[:, 0] - a[:, 0]) / a[:, 2], (g[:, 1] - a[:, 1]) / a[:, 3], torch.log(g[:, 2] / a[:, 2]), torch.log(g[:, 3] / a[:, 3])], 1)


def rpn_loss(W, feat, pos_idx, pos_tgt, neg_idx, gt, droi=None, decay=0.0, opts=None, leaves=None):
    """mid_objectness + mid_box_reg + 0.5 * decay * |trans|^2 + <droi, boxes of the sampled rows> in float64 (a torch scalar), and
    (mid_objectness, mid_box_reg, masked_mid): what the gradients are the derivatives of where no input row is named twice."""
    import torch
    o = dict(MID_DEFAULTS, **(opts or {}))
    wo, wb = float(F32(o["mid_objectness_weight"])), float(F32(o["mid_box_reg_weight"]))
    pi, pt, ni = (torch.as_tensor(np.asarray(a, np.int64)) for a in (pos_idx, pos_tgt, neg_idx))
    x = leaves["feat"] if leaves else feat
    h, w = x.shape[1:]
    _pre, _hid, trans, scores = _forward(W, feat, torch.float64, leaves)
    anc = anchor_rows(W, h, w)
    A = torch.as_tensor(anc.astype(np.float64))
    np_, nn_ = len(pi), len(ni)
    ls = torch.log_softmax(scores, 1)
    mo = wo * ((-ls[pi, 0].sum() / np_ if np_ else 0.0) + (-ls[ni, 1].sum() / nn_ if nn_ else 0.0))
    mb, masked = torch.zeros((), dtype=torch.float64), 0
    if np_:
        tg = _targets(anc[np.asarray(pos_idx, np.int64)], gt, pt)
        keep = ~(tg.abs().max(1).values > 10.0)
        masked = int((~keep).sum())
        z = (trans[pi] - tg).abs()
        rows = torch.where(z < 1.0, 0.5 * z * z, z - 0.5).sum(1)
        mb = wb * (rows * keep).sum() / (4.0 * np_)
    total = mo + mb + 0.5 * float(F32(decay)) * (trans * trans).sum()
    if droi is not None and np_ + nn_:
        sel = torch.cat([pi, ni])
        t, a = trans[sel], A[sel]
        boxes = torch.stack([t[:, 0] * a[:, 2] + a[:, 0], t[:, 1] * a[:, 3] + a[:, 1], torch.exp(t[:, 2]) * a[:, 2], torch.exp(t[:, 3]) * a[:, 3]], 1)
        total = total + (boxes * torch.as_tensor(np.asarray(droi, F32).astype(np.float64))).sum()
    return total, (float(mo), float(mb), masked)


def rpn_grad(W, feat, pos_idx, pos_tgt, neg_idx, gt, droi=None, decay=0.0, opts=None, dtype="float64", variant=None):
    """The seven tensors of dc_op_rpn_grad as numpy float64 (evaluated in `dtype`), plus mid_objectness_loss, mid_box_reg_loss,
    masked_mid, and what the case generators check: `hidden_pre`, `residual` (num_pos, 4) and `target` (num_pos, 4)."""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    o = dict(MID_DEFAULTS, **(opts or {}))
    wo, wb, dec = float(F32(o["mid_objectness_weight"])), float(F32(o["mid_box_reg_weight"])), float(F32(decay))
    pi, pt, ni = (np.asarray(a, np.int64).reshape(-1) for a in (pos_idx, pos_tgt, neg_idx))
    np_, nn_ = len(pi), len(ni)
    feat = np.asarray(feat, F32)
    h, w = feat.shape[1:]
    with torch.enable_grad():
        leaves = {n: torch.as_tensor(np.asarray(W[n], np.float64)).to(dt).requires_grad_(True) for n in RPN_PARAMS}
        leaves["feat"] = torch.as_tensor(feat.astype(np.float64)).to(dt).requires_grad_(True)
        pre, hid, trans, scores = _forward(W, feat, dt, leaves)
        if variant == "relu_mask_from_input":                     # the mask read from the layer's input map, not its output
            R = pre.shape[0]
            hid2 = pre * (leaves["feat"][:R] > 0).to(dt).detach()
            k = leaves["rpn_box_w"].shape[0] // 4
            box = Fn.conv2d(hid[None].detach() + (hid2 - hid2.detach())[None], leaves["rpn_box_w"].reshape(4 * k, -1, 1, 1), leaves["rpn_box_b"])[0]
            sc = Fn.conv2d(hid[None].detach() + (hid2 - hid2.detach())[None], leaves["rpn_score_w"].reshape(2 * k, -1, 1, 1), leaves["rpn_score_b"])[0]
            trans = box.reshape(k, 4, h, w).permute(0, 2, 3, 1).reshape(-1, 4)
            scores = sc.reshape(k, 2, h, w).permute(0, 2, 3, 1).reshape(-1, 2)
        anc = anchor_rows(W, h, w)
        A = torch.as_tensor(anc.astype(np.float64)).to(dt)
        T, S = trans.detach(), scores.detach()
        n_rows = T.shape[0]
        # ---- the criteria's gradients on the sampled rows ----
        sm = torch.softmax(S, 1)
        c_pos, c_neg = (1, 0) if variant == "classes_swapped" else (0, 1)
        ds_pos = sm[pi].clone(); ds_neg = sm[ni].clone()
        if np_:
            ds_pos[:, c_pos] -= 1.0
            ds_pos = wo * ds_pos / np_
        if nn_:
            ds_neg[:, c_neg] -= 1.0
            ds_neg = wo * ds_neg / nn_
        ls = torch.log_softmax(S, 1)
        mo = wo * ((-ls[pi, 0].sum() / np_ if np_ else 0.0) + (-ls[ni, 1].sum() / nn_ if nn_ else 0.0))
        dt_pos = torch.zeros((np_, 4), dtype=dt)
        resid = torch.zeros((np_, 4), dtype=dt); tg = torch.zeros((np_, 4), dtype=dt)
        mb, masked = 0.0, 0
        if np_:
            tg = _targets(anc[pi], gt, torch.as_tensor(pt)).to(dt)
            m = tg.abs().max(1).values > 10.0
            masked = int(m.sum())
            resid = T[pi] - tg
            div = 4.0 * ((np_ - masked) if variant == "mask_out_of_divisor" else np_)
            dt_pos = wb * resid.clamp(-1.0, 1.0) / max(div, 1.0)
            z = resid.abs()
            rows = torch.where(z < 1.0, 0.5 * z * z, z - 0.5).sum(1)
            if variant != "mask_not_zeroed":
                dt_pos = dt_pos * (~m)[:, None]
            mb = wb * float((rows * (~m)).sum()) / (4.0 * np_)
        g = torch.as_tensor(np.asarray(droi, F32).astype(np.float64)).to(dt).reshape(-1, 4) if droi is not None and np_ + nn_ else None
        # ---- the sampler's backward: a copy, positives first, then negatives; the last write wins ----
        gb, gt_, gs = torch.zeros((n_rows, 4), dtype=dt), torch.zeros((n_rows, 4), dtype=dt), torch.zeros((n_rows, 2), dtype=dt)
        writes = [("pos", r) for r in range(np_)] + [("neg", r) for r in range(nn_)]
        if variant == "pos_after_neg":
            writes = writes[np_:] + writes[:np_]
        if variant == "sum_not_last":
            for cls, r in writes:
                i = pi[r] if cls == "pos" else ni[r]
                if g is not None: gb[i] += g[r if cls == "pos" else np_ + r]
                gs[i] += ds_pos[r] if cls == "pos" else ds_neg[r]
                if cls == "pos": gt_[i] += dt_pos[r]
        else:
            for cls, r in writes:
                i = pi[r] if cls == "pos" else ni[r]
                if g is not None: gb[i] = g[r if cls == "pos" else np_ + r]
                gs[i] = ds_pos[r] if cls == "pos" else ds_neg[r]
                if cls == "pos": gt_[i] = dt_pos[r]
        # ---- ApplyBoxTransform:backward, the ConcatTable's sum, RegularizeLayer ----
        bw, bh = torch.exp(T[:, 2]) * A[:, 2], torch.exp(T[:, 3]) * A[:, 3]
        if variant == "no_box_w":
            bw, bh = torch.ones_like(bw), torch.ones_like(bh)
        abt = torch.stack([gb[:, 0] * A[:, 2], gb[:, 1] * A[:, 3], gb[:, 2] * bw, gb[:, 3] * bh], 1)
        dtrans = (0.0 if variant == "no_decay" else dec) * T + (abt + gt_)
        names = list(RPN_PARAMS) + ["feat"]
        grads = torch.autograd.grad([trans, scores], [leaves[n] for n in names] + [pre], [dtrans, gs], allow_unused=True)
        out = {n: (gr if gr is not None else torch.zeros_like(leaves[n])).double().numpy().copy() for n, gr in zip(names, grads[:-1])}
        dpre = grads[-1] if grads[-1] is not None else torch.zeros_like(pre)
        if variant == "dx_taps_not_flipped":
            out["feat"] = Fn.conv2d(dpre[None], leaves["rpn_conv_w"].detach().transpose(0, 1).contiguous(), None, padding=1)[0].double().numpy().copy()
        if variant == "dw_taps_transposed":
            out["rpn_conv_w"] = np.ascontiguousarray(out["rpn_conv_w"].transpose(0, 1, 3, 2))
    out["rpn_box_w"] = out["rpn_box_w"].reshape(np.asarray(W["rpn_box_w"]).shape)
    out["rpn_score_w"] = out["rpn_score_w"].reshape(np.asarray(W["rpn_score_w"]).shape)
    out.update(mid_objectness_loss=float(mo), mid_box_reg_loss=float(mb), masked_mid=masked,
               hidden_pre=pre.detach().double().numpy(), residual=resid.double().numpy(), target=tg.double().numpy(),
               dheads=(dtrans.double().numpy(), gs.double().numpy()))
    return out


def rpn_rows(name, a):
    """The 2-D view whose rows the per-row bars hold: rpn_conv_w per output channel, feat (512, h, w) per pixel, the head weights
    per row."""
    a = np.asarray(a)
    if name == "feat":
        return np.ascontiguousarray(a.reshape(a.shape[0], -1).T)
    return a.reshape(a.shape[0], -1)


def case_defects(ref):
    """What a generated case must not have (the list is empty for a good one): a mid-box residual within EDGE of the SmoothL1 kink, a
    |target| within EDGE of 10, a hidden pre-activation within HIDDEN_EDGE * max|hidden| of zero (its ReLU mask could differ
    between fp32 and float64: a case defect, not a kernel error)."""
    bad = []
    keep = ~(np.abs(ref["target"]).max(1) > 10.0) if len(ref["target"]) else np.zeros(0, bool)
    if len(ref["residual"]) and (np.abs(np.abs(ref["residual"][keep]) - 1.0) < EDGE).any():
        bad.append("kink")
    if len(ref["target"]) and (np.abs(np.abs(ref["target"]) - 10.0) < EDGE).any():
        bad.append("mask")
    hp = ref["hidden_pre"]
    if (np.abs(hp) < HIDDEN_EDGE * np.abs(hp).max()).any():
        bad.append("relu")
    return bad


def draw_rpn_case(W, h, w, num_pos, num_neg, seed, masked_rows=(), far_rows=(), dup_neg=0, neg_on_pos=0, dup_pos=0, corners=False,
                  with_droi=True):
    """feat (512,h,w), the three lists, gt (G,4), droi (n,4) or None, drawn on the seed sequence seed, seed + 1000, .. until
    case_defects is empty; returns them and the number of redraws.  The positives' ground-truth boxes are jittered copies of
    their anchors (targets of a few tenths); masked_rows get a target 11 anchor heights away, far_rows one three anchor widths
    away (SmoothL1's linear branch).  dup_neg / dup_pos: that many extra rows repeating an earlier row of their class;
    neg_on_pos: that many negatives naming a positive's input row.  corners: the first rows sit on the map's four corner pixels
    for anchors 0 and k - 1."""
    anc = anchor_rows(W, h, w)
    A, k = len(anc), np.asarray(W["anchors"]).shape[1]
    for redraw in range(20):
        rng = np.random.default_rng(seed + 1000 * redraw)
        feat = np.abs(rng.standard_normal((512, h, w))).astype(F32)
        base_p, base_n = num_pos - dup_pos, num_neg - dup_neg - neg_on_pos
        rows = rng.permutation(A)[:base_p + base_n]
        if corners:
            cells = [0, w - 1, (h - 1) * w, h * w - 1]
            forced = [a * h * w + c for a in sorted({0, k - 1}) for c in cells]
            rest = [r for r in rows.tolist() if r not in forced]
            rows = np.asarray((forced + rest)[:base_p + base_n], np.int64)
            rows = rows[np.argsort(np.arange(len(rows)) % 2, kind="stable")]       # corners go to both classes
        pi, ni = rows[:base_p].tolist(), rows[base_p:].tolist()
        pi += [pi[int(rng.integers(0, max(base_p, 1)))] for _ in range(dup_pos)] if base_p else []
        ni += [ni[int(rng.integers(0, max(base_n, 1)))] for _ in range(dup_neg)] if base_n else []
        ni += [pi[int(rng.integers(0, len(pi)))] for _ in range(neg_on_pos)] if pi else []
        pi, ni = np.asarray(pi, np.int32), np.asarray(ni, np.int32)
        G = max(len(pi), 1)
        pt = rng.permutation(G)[:len(pi)].astype(np.int32)
        gt = np.tile(np.asarray([[50, 40, 30, 20]], F32), (G, 1))
        for r in range(len(pi)):
            a = anc[pi[r]].astype(np.float64)
            b = a * (1.0 + 0.3 * rng.uniform(-1, 1, 4))
            if r in masked_rows:
                b[1] = a[1] - 11.0 * a[3]
            if r in far_rows:
                b[0] = a[0] + 3.0 * a[2]
            gt[pt[r]] = b
        n = len(pi) + len(ni)
        droi = (rng.standard_normal((n, 4)) * np.asarray([1e-3, 1e-3, 1e-4, 1e-4])).astype(F32) if with_droi and n else None
        ref = rpn_grad(W, feat, pi, pt, ni, gt, droi, 0.0)
        if not case_defects(ref):
            return feat, pi, pt, ni, gt, droi, redraw
    raise AssertionError("no clean draw in 20 tries")
