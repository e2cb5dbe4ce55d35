"""The recognition net's backward restated with float64 torch autograd (docs/SEMANTICS.md, "Recognition-net gradients"):
bilinear RoI pooling with zero-padded taps, fc6 in the checkpoint's (c, i, j) flattening, the two ReLUs, the two heads, the two
end criteria as tests/loss_rules.py defines them (the mask included) and a <codes_pos, g> term for the language model's gradient.

Sampling coordinates are taken in float32 exactly as oracle.bilinear_sample_hwc forms them, so floors and weights are the
device's; they are made differentiable straight-through: c32 + (c64(box) - c64(box).detach()).  coords="float64" forms them in
float64 throughout instead (what central differences can follow).  Everything runs under torch.enable_grad(): the oracle turns
autograd off when it is imported.

variant= gives WRONG restatements for the teeth tests: "no_w_factor" (the (W-1)/2 factor dropped from d xcoord / d grid),
"clamp_taps" (out-of-map taps clamped to the edge instead of zeroed), "anchor_sign" (the anchor gradient of the box criterion
with its sign unflipped), "no_mask" (the > 10 mask ignored), "fc6_ijc" (fc6 fed in (i, j, c) order)."""
import numpy as np

from oracle import densecap_oracle as O
from tests import loss_rules as LR

F32 = np.float32
PARAMS = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "obj_w", "obj_b", "boxreg_w", "boxreg_b")
TENSORS = PARAMS + ("feat", "roi_boxes")
VARIANTS = ("no_w_factor", "clamp_taps", "anchor_sign", "no_mask", "fc6_ijc")
EDGE = 1e-3                    # px from an integer coordinate / from the SmoothL1 kink that a generated case keeps


def coords32(boxes, img_h, img_w, h, w, HH, WW):
    """(ycoord, xcoord), each (B, HH, WW) float32: the pixel coordinates oracle.bilinear_sample_hwc floors."""
    g = O.affine_grid(O.box_to_affine(np.asarray(boxes, F32).reshape(-1, 4), img_h, img_w), HH, WW)
    return (g[..., 0] + F32(1)) * F32(h - 1) / F32(2), (g[..., 1] + F32(1)) * F32(w - 1) / F32(2)


def edge_distance(boxes, img_h, img_w, h, w, HH, WW):
    """Per box, the smallest distance of a sampling coordinate from an integer."""
    yc, xc = coords32(boxes, img_h, img_w, h, w, HH, WW)
    d = np.minimum(np.abs(yc - np.round(yc)), np.abs(xc - np.round(xc)))
    return d.reshape(len(d), -1).min(1)


def _coords64(boxes, img_h, img_w, h, w, HH, WW, variant):
    import torch
    ys = torch.tensor([float(F32(-1.0 + (i / (HH - 1)) * 2)) for i in range(HH)], dtype=boxes.dtype)
    xs = torch.tensor([float(F32(-1.0 + (j / (WW - 1)) * 2)) for j in range(WW)], dtype=boxes.dtype)
    th23 = (boxes[:, 0] * 2 + (-1 - img_w)) / (img_w - 1)
    th13 = (boxes[:, 1] * 2 + (-1 - img_h)) / (img_h - 1)
    th22, th11 = boxes[:, 2] / img_w, boxes[:, 3] / img_h
    gy = (ys[None, :, None] * th11[:, None, None] + th13[:, None, None]).expand(-1, HH, WW)
    gx = (xs[None, None, :] * th22[:, None, None] + th23[:, None, None]).expand(-1, HH, WW)
    fx = 1.0 if variant == "no_w_factor" else (w - 1) / 2.0
    return (gy + 1) * ((h - 1) / 2.0), (gx + 1) * fx


def roi_pool(feat, boxes, img_h, img_w, HH=7, WW=7, variant=None, coords="float32"):
    """feat (C, h, w) and boxes (B, 4) torch tensors -> (B, C, HH, WW), differentiable in both."""
    import torch
    C, h, w = feat.shape
    Y, X = _coords64(boxes, img_h, img_w, h, w, HH, WW, variant)
    if coords == "float32":
        yc, xc = coords32(boxes.detach().numpy(), img_h, img_w, h, w, HH, WW)
        Y = torch.from_numpy(yc.astype(np.float64)).to(boxes.dtype) + (Y - Y.detach())
        X = torch.from_numpy(xc.astype(np.float64)).to(boxes.dtype) + (X - X.detach())
    y0, x0 = torch.floor(Y.detach()), torch.floor(X.detach())
    wy, wx = 1 - (Y - y0), 1 - (X - x0)
    y0, x0 = y0.long(), x0.long()

    def tap(yy, xx):
        ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
        v = feat[:, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]                  # (C, B, HH, WW)
        return v if variant == "clamp_taps" else v * ok.to(feat.dtype)
    out = (wx * wy * tap(y0, x0) + (1 - wx) * wy * tap(y0, x0 + 1) + wx * (1 - wy) * tap(y0 + 1, x0)
           + (1 - wx) * (1 - wy) * tap(y0 + 1, x0 + 1))
    return out.permute(1, 0, 2, 3)


def roi_pool_grad(feat, boxes, img_h, img_w, dout, HH=7, WW=7, variant=None, coords="float32", dtype=None):
    """(dfeat (C, h, w), dboxes (B, 4)) float64 of sum(dout * pooled) for numpy inputs; dout (B, C, HH, WW).  dtype: the type the
    rules are evaluated in (float64; torch.float32 gives the error any fp32 evaluation carries)."""
    import torch
    dtype = dtype or torch.float64
    with torch.enable_grad():
        f = torch.tensor(np.asarray(feat, F32).astype(np.float64), dtype=dtype, requires_grad=True)
        b = torch.tensor(np.asarray(boxes, F32).reshape(-1, 4).astype(np.float64), dtype=dtype, requires_grad=True)
        d = torch.tensor(np.asarray(dout, F32).astype(np.float64), dtype=dtype)
        s = (roi_pool(f, b, img_h, img_w, HH, WW, variant, coords) * d).sum()
        df, db = torch.autograd.grad(s, [f, b])
    return df.double().numpy(), db.double().numpy()


def _torch_params(W, dtype, requires_grad=True):
    import torch
    return {k: torch.tensor(np.asarray(W[k], F32).astype(np.float64), dtype=dtype, requires_grad=requires_grad) for k in PARAMS}


def forward(P, feat, boxes, num_pos, targets, g, img_h, img_w, opts=None, variant=None, coords="float32"):
    """The differentiable total end_objectness + end_box_reg + <codes_pos, g> and what it is made of: a dict of torch values.
    P: the eight parameters; feat (512, h, w), boxes (n, 4), targets (num_pos, 4), g (num_pos, D) or None: torch tensors."""
    import torch
    o = dict(LR.DEFAULTS, **(opts or {}))
    w_obj, w_box = float(F32(o["end_objectness_weight"])), float(F32(o["end_box_reg_weight"]))
    n, np_ = boxes.shape[0], int(num_pos)
    pooled = roi_pool(feat, boxes, img_h, img_w, 7, 7, variant, coords)                      # (n, 512, 7, 7)
    x = (pooled.permute(0, 2, 3, 1) if variant == "fc6_ijc" else pooled).reshape(n, -1)
    y6 = torch.relu(x @ P["fc6_w"].T + P["fc6_b"])
    codes = torch.relu(y6 @ P["fc7_w"].T + P["fc7_b"])
    obj = (codes @ P["obj_w"].T + P["obj_b"]).reshape(n)
    trans = codes[:np_] @ P["boxreg_w"].T + P["boxreg_b"]
    out = dict(pooled=pooled, codes=codes, obj=obj, trans=trans)
    out.update(criteria(obj, trans, boxes[:np_], targets, w_obj, w_box, variant))
    total = out["end_objectness_loss"] + out["end_box_reg_loss"]
    if np_ > 0 and g is not None:
        total = total + (codes[:np_] * g).sum()
    out["total"] = total
    return out


def criteria(obj, trans, anchors, targets, w_obj, w_box, variant=None):
    """The two end criteria on torch values: obj (n) logits, the first len(trans) rows labelled 1; trans, anchors, targets
    (num_pos, 4).  LogisticCriterion.lua:85-92 per row, SmoothL1 against InvertBoxTransform(anchors, targets) with the > 10 mask."""
    import torch
    n, np_ = obj.shape[0], trans.shape[0]
    a = torch.where(obj < 0, obj, torch.zeros_like(obj))
    rows = torch.log(torch.exp(a) + torch.exp(a - obj)) - a
    rows = rows + torch.cat([torch.zeros(np_, dtype=obj.dtype), obj[np_:]])
    out = dict(end_objectness_loss=w_obj * (rows.sum() / n), end_box_reg_loss=torch.zeros((), dtype=obj.dtype), masked_end=0)
    if np_ > 0:
        A = anchors
        t = torch.stack([(targets[:, 0] - A[:, 0]) / A[:, 2], (targets[:, 1] - A[:, 1]) / A[:, 3], torch.log(targets[:, 2] / A[:, 2]),
                         torch.log(targets[:, 3] / A[:, 3])], 1)
        if variant == "anchor_sign":
            t = t.detach() - (t - t.detach())
        masked = (t.detach().abs().max(1).values > 10.0) if variant != "no_mask" else torch.zeros(np_, dtype=torch.bool)
        z = torch.where(masked[:, None], torch.zeros_like(t), trans - t)
        az = z.abs()
        out["end_box_reg_loss"] = w_box * (torch.where(az < 1.0, 0.5 * z * z, az - 0.5).sum() / (4.0 * np_))
        out["masked_end"] = int(masked.sum())
        out["residual"] = (trans - t).detach()
    return out


def end_crit_grad(obj, trans, anchors, targets, num_pos, w_obj=0.1, w_box=0.1):
    """(dobj (n), dtrans (num_pos, 4), danchor (num_pos, 4), masked) float64 of the two end criteria for numpy inputs; trans and
    anchors hold n rows, of which the first num_pos count."""
    import torch
    with torch.enable_grad():
        x = torch.tensor(np.asarray(obj, F32).astype(np.float64).reshape(-1), requires_grad=True)
        tr = torch.tensor(np.asarray(trans, F32).astype(np.float64).reshape(-1, 4)[:num_pos], requires_grad=True)
        an = torch.tensor(np.asarray(anchors, F32).astype(np.float64).reshape(-1, 4)[:num_pos], requires_grad=True)
        tg = torch.tensor(np.asarray(targets, F32).astype(np.float64).reshape(-1, 4))
        c = criteria(x, tr, an, tg, float(F32(w_obj)), float(F32(w_box)))
        gs = torch.autograd.grad(c["end_objectness_loss"] + c["end_box_reg_loss"], [x, tr, an], allow_unused=True)
    return tuple(np.zeros(tuple(v.shape)) if gr is None else gr.numpy() for gr, v in zip(gs, (x, tr, an))) + (c["masked_end"],)


def recog_grad(W, feat, boxes, num_pos, targets, g, img_h, img_w, opts=None, variant=None, coords="float32", dtype=None):
    """numpy in, numpy out: the ten gradients of TENSORS (float64; feat (512, h, w), roi_boxes (n, 4)), the two losses, masked_end."""
    import torch
    dtype = dtype or torch.float64
    with torch.enable_grad():
        P = _torch_params(W, dtype)
        f = torch.tensor(np.asarray(feat, F32).astype(np.float64), dtype=dtype, requires_grad=True)
        b = torch.tensor(np.asarray(boxes, F32).reshape(-1, 4).astype(np.float64), dtype=dtype, requires_grad=True)
        t = torch.tensor(np.asarray(targets, F32).reshape(-1, 4).astype(np.float64), dtype=dtype)
        gt = None if g is None else torch.tensor(np.asarray(g, F32).astype(np.float64), dtype=dtype)
        out = forward(P, f, b, num_pos, t, gt, img_h, img_w, opts, variant, coords)
        grads = torch.autograd.grad(out["total"], [P[k] for k in PARAMS] + [f, b], allow_unused=True)
    res = {k: (np.zeros(tuple(v.shape)) if gr is None else gr.double().numpy())
           for k, gr, v in zip(TENSORS, grads, [P[k] for k in PARAMS] + [f, b])}
    res.update(end_objectness_loss=float(out["end_objectness_loss"].detach()), end_box_reg_loss=float(out["end_box_reg_loss"].detach()),
               masked_end=out["masked_end"], total=float(out["total"].detach()))
    return res


# ---- case generators ------------------------------------------------------------------------------------------------------------
def draw_boxes(rng, B, img_h, img_w, h, w, HH=7, WW=7, lo=0.15, hi=0.7, outside=0.0):
    """B boxes xcycwh float32 inside the image (a share `outside` of them straddling its border), each redrawn until no sampling
    coordinate lies within EDGE px of an integer."""
    out = np.zeros((B, 4), F32)
    for r in range(B):
        while True:
            bw, bh = rng.uniform(lo, hi) * img_w, rng.uniform(lo, hi) * img_h
            if rng.uniform() < outside:
                xc, yc = rng.choice([-0.1, 1.1]) * img_w, rng.uniform(0.2, 0.8) * img_h
            else:
                xc, yc = rng.uniform(bw / 2, img_w - bw / 2), rng.uniform(bh / 2, img_h - bh / 2)
            b = np.array([[xc, yc, bw, bh]], F32)
            if edge_distance(b, img_h, img_w, h, w, HH, WW)[0] > EDGE:
                out[r] = b[0]
                break
    return out


def draw_feat(rng, C, h, w):
    return rng.standard_normal((C, h, w)).astype(F32)


def draw_case(W, rng, n, num_pos, img_h, img_w, h, w, masked_rows=(), far_rows=(), opts=None, outside=0.0):
    """(feat, boxes, targets) for the weights W: boxes by draw_boxes; the positive rows' targets are jittered copies of their boxes,
    redrawn until every transform residual is more than EDGE away from the SmoothL1 kink at +-1; masked_rows get a target whose
    transform exceeds 10, far_rows one four times as wide as the box (a residual on SmoothL1's linear branch)."""
    import torch
    feat = draw_feat(rng, 512, h, w)
    boxes = draw_boxes(rng, n, img_h, img_w, h, w, outside=outside)
    targets = np.zeros((num_pos, 4), F32)
    if num_pos == 0:
        return feat, boxes, targets
    with torch.no_grad():
        P = _torch_params(W, torch.float64, requires_grad=False)
        f, b = torch.tensor(feat.astype(np.float64)), torch.tensor(boxes.astype(np.float64))
    for attempt in range(200):
        for r in range(num_pos):
            if attempt == 0 or bad[r]:
                j = rng.uniform(-1, 1, 4)
                targets[r] = boxes[r] * (1 + np.array([0.05, 0.05, 0.3, 0.3]) * j)
                if r in far_rows:
                    targets[r, 2] = 4.0 * boxes[r, 2]
                if r in masked_rows:
                    targets[r, 0] = boxes[r, 0] + 12.0 * boxes[r, 2]
        with torch.no_grad():
            res = forward(P, f, b, num_pos, torch.tensor(targets.astype(np.float64)), None, img_h, img_w, opts)["residual"].numpy()
        bad = (np.abs(np.abs(res) - 1.0) <= EDGE).any(1)
        bad[list(masked_rows)] = False
        if not bad.any():
            return feat, boxes, targets
    raise RuntimeError("draw_case: no targets found away from the SmoothL1 kink")
