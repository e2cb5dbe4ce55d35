"""The backward through conv_net2 -- VGG layers 11..30: the convolutions conv3_1 .. conv5_3 (indices 4..12 of the thirteen), their
in-place ReLUs, pool3 behind conv3_3 and pool4 behind conv4_3 -- restated in numpy / torch (docs/SEMANTICS.md, "CNN gradients").

pool_relu_grad and relu_grad are exact selections: nothing is added or multiplied, so a device result is compared bit for bit.
chain is the backward given FIXED activations: the masks and the pools' arg-maxes are taken from the arrays passed in, never
recomputed, so that a device run and a float64 evaluation route every gradient through the same elements; the convolutions'
gradients are tests/rpn_grad_rules.conv3x3_grad's.  Maps are (C, h, w) numpy arrays.

variant= gives WRONG restatements for the teeth tests: "tie_last" (a tie inside a window goes to its last maximum),
"mask_ge" (the ReLU's mask is output >= 0) and "edge_not_clipped" (a window at the right edge runs on into the next map row)."""
import numpy as np

from tests import rpn_grad_rules as R

F32 = np.float32
CONVS = tuple(range(4, 13))
POOL_AFTER = (6, 9)
CHANNELS = {4: (128, 256), 5: (256, 256), 6: (256, 256), 7: (256, 512), 8: (512, 512), 9: (512, 512), 10: (512, 512),
            11: (512, 512), 12: (512, 512)}
VARIANTS = ("tie_last", "mask_ge", "edge_not_clipped")
# the model around the nine convolutions is as small as the library takes: only conv_w / conv_b matter here
SMALL_MODEL = dict(vocab_size=5, seq_length=1, rpn_hidden=32, enc_size=32, rnn_size=32, fc_dim=256,
                   anchors=np.array([[96], [80]], F32))
# (h4, w4): 5x7 -> 3x4 -> 2x2 clips windows at both pools; 9x15 = 135 pixels -> 5x8 -> 3x4: conv3's weight gradients share their
# pixels between two slices (a slice sums at least 64), odd maps at both pools
CHAIN_SHAPES = [(1, 1), (2, 3), (5, 7), (8, 8), (9, 15)]


def pool_relu_grad(y, dpool, variant=None):
    """y (C, H, W) the map the pool read (the ReLU's output), dpool (C, ceil(H/2), ceil(W/2)) -> dy (C, H, W) in dpool's dtype: a
    window's gradient goes to its first maximum in scan order, if that is > 0; everything else is +0.0."""
    y, g = np.asarray(y), np.asarray(dpool)
    C, H, W = y.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert g.shape == (C, Ho, Wo), (y.shape, g.shape)
    out = np.zeros((C, H * W), g.dtype)
    fy, ch = y.reshape(C, -1), np.arange(C)
    for yo in range(Ho):
        for xo in range(Wo):
            cand = []
            for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
                yy, xx = 2 * yo + a, 2 * xo + b
                if variant == "edge_not_clipped":
                    if yy * W + xx < H * W:
                        cand.append(yy * W + xx)
                elif yy < H and xx < W:
                    cand.append(yy * W + xx)
            cand = np.asarray(cand)
            vals = fy[:, cand]
            arg = len(cand) - 1 - np.argmax(vals[:, ::-1], 1) if variant == "tie_last" else np.argmax(vals, 1)
            best = vals[ch, arg]
            live = np.flatnonzero(best >= 0 if variant == "mask_ge" else best > 0)
            out[live, cand[arg[live]]] = g[live, yo, xo]
    return out.reshape(C, H, W)


def relu_grad(y, dy, variant=None):
    y, dy = np.asarray(y), np.asarray(dy)
    return np.where(y >= 0 if variant == "mask_ge" else y > 0, dy, np.zeros((), dy.dtype)).astype(dy.dtype)


def sizes(h4, w4):
    """{i: (h, w)} of the nine convolutions' maps, and conv5_3's map size."""
    out, h, w = {}, h4, w4
    for i in CONVS:
        out[i] = (h, w)
        if i in POOL_AFTER:
            h, w = (h + 1) // 2, (w + 1) // 2
    return out, (h, w)


def chain(acts, prepool, weights, dfeat, dtype="float64", variant=None):
    """The backward of dfeat (512, h6, w6) given fixed activations.  acts: {i: the input of convolution i (Cin, h, w)} for
    i = 4..12 and acts[13] = conv5_3's output after its ReLU; prepool: {6: conv3_3's output, 9: conv4_3's} after their ReLUs;
    weights: {i: (Cout, Cin, 3, 3)}.  Every product is evaluated in `dtype`.  Returns float64 arrays: "conv_w<i>", "conv_b<i>",
    "dy<i>" (the gradient at convolution i's own output) and "x" (at conv3_1's input)."""
    dt = np.dtype(dtype)
    out, g = {}, np.asarray(dfeat).astype(dt)
    for i in reversed(CONVS):
        if i in POOL_AFTER:
            dy = pool_relu_grad(prepool[i], g, variant)
        else:
            dy = relu_grad(acts[i + 1], g, variant)
        r = R.conv3x3_grad(acts[i], weights[i], dy, dtype=dtype)
        out["dy%d" % i], out["conv_w%d" % i], out["conv_b%d" % i] = dy.astype(np.float64), r["dw"], r["db"]
        g = r["dx"].astype(dt)
    out["x"] = g.astype(np.float64)
    return out


def forward(x4, weights, biases, dtype="float64", leaves=False):
    """torch's own forward of the nine layers: (acts, prepool) as chain takes them, numpy in `dtype`.  leaves: also the torch
    tensors (x, {i: w}, {i: b}, feat) with requires_grad, for autograd."""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.enable_grad():
        x = torch.tensor(np.asarray(x4), dtype=dt).requires_grad_(leaves)
        wt = {i: torch.tensor(np.asarray(weights[i]), dtype=dt).requires_grad_(leaves) for i in CONVS}
        bt = {i: torch.tensor(np.asarray(biases[i]), dtype=dt).requires_grad_(leaves) for i in CONVS}
        acts, prepool, cur = {}, {}, x
        for i in CONVS:
            acts[i] = cur.detach().numpy().copy()
            cur = Fn.relu(Fn.conv2d(cur[None], wt[i], bt[i], padding=1)[0])
            if i in POOL_AFTER:
                prepool[i] = cur.detach().numpy().copy()
                cur = Fn.max_pool2d(cur[None], 2, 2, ceil_mode=True)[0]
        acts[13] = cur.detach().numpy().copy()
    return (acts, prepool, (x, wt, bt, cur)) if leaves else (acts, prepool)


def autograd(x4, weights, biases, dfeat):
    """The 18 gradients and "x" of <dfeat, conv_net2(x4)> by float64 torch autograd, with the activations they were taken at."""
    import torch
    acts, prepool, (x, wt, bt, feat) = forward(x4, weights, biases, "float64", leaves=True)
    with torch.enable_grad():
        (feat * torch.tensor(np.asarray(dfeat), dtype=torch.float64)).sum().backward()
    out = {"x": x.grad.numpy().copy()}
    for i in CONVS:
        out["conv_w%d" % i], out["conv_b%d" % i] = wt[i].grad.numpy().copy(), bt[i].grad.numpy().copy()
    return out, acts, prepool


_weights = {}


def model_weights(seed=41):
    """make_synthetic_weights at SMALL_MODEL's sizes with every convolution He-scaled, std = sqrt(2 / (9 Cin)) (feat_rms = 1:
    conv5_3 is not scaled down), so that the nine layers neither die nor blow up.  Made once per process."""
    if seed not in _weights:
        from densecap_amd.weights import make_synthetic_weights
        _weights[seed] = make_synthetic_weights(seed=seed, feat_rms=1.0, **SMALL_MODEL)
    return _weights[seed]


def conv_params(W):
    return ({i: np.asarray(W["conv_w"][i], F32) for i in CONVS}, {i: np.asarray(W["conv_b"][i], F32) for i in CONVS})


def make_chain_case(h4, w4, seed):
    """x4 (128, h4, w4) float32, shaped like a pool2 map (a ReLU's output, unit mean square), and dfeat (512, h6, w6) with
    per-channel scales spread over a decade."""
    rng = np.random.default_rng(seed)
    x4 = (np.maximum(rng.standard_normal((128, h4, w4)), 0) * np.sqrt(2.0)).astype(F32)
    _, (fh, fw) = sizes(h4, w4)
    dfeat = (rng.standard_normal((512, fh, fw)) * rng.uniform(0.3, 3.0, (512, 1, 1))).astype(F32)
    return x4, dfeat


def make_pool_case(C, H, W, seed, n=1):
    """y (n, C, H, W) and dpool float32 for the pool kernel: a ReLU's output (half of it zeros) with, at seeded places, positive
    ties inside windows at each of the four positions, all-zero windows, and windows whose maximum is -0.0 or negative (what a
    map taken before the ReLU would hold; they must give zero); dpool carries a NaN and an infinity."""
    rng = np.random.default_rng(seed)
    y = np.maximum(rng.standard_normal((n, C, H, W)), 0).astype(F32)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    kinds = rng.integers(0, 8, (n, C, Ho, Wo))
    for idx in np.ndindex(n, C, Ho, Wo):
        k = kinds[idx]
        if k > 4:
            continue
        m, c, yo, xo = idx
        win = y[m, c, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2]             # (a view, clipped at the edge)
        if k == 0:
            win[...] = 0
        elif k == 1:
            win[...] = F32(-0.0)
        elif k == 2:
            win[...] = -np.abs(rng.standard_normal(win.shape)).astype(F32) - F32(0.5)
        else:                                                            # a positive tie: the maximum written to two or all places
            top = F32(1.5) + F32(rng.integers(0, 4))
            places = rng.permutation(win.size)[:max(2, win.size) if k == 3 else 2]
            vals = win.copy().reshape(-1)
            vals[places] = top
            win[...] = vals.reshape(win.shape)
    dpool = (rng.standard_normal((n, C, Ho, Wo)) * 3).astype(F32)
    dpool.reshape(-1)[rng.integers(0, dpool.size)] = np.nan
    dpool.reshape(-1)[rng.integers(0, dpool.size)] = np.inf
    return y, dpool

