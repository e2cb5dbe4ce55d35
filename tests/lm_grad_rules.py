"""The language-model gradient definition (docs/SEMANTICS.md, "Language-model gradients") restated with torch autograd, in
float64 on the float32 weights and codes: an LSTM step of its own (gate order i,f,o,g; (b + x.Wx) + h.Wh), log_softmax and
masking of finished rows.  Inputs of a row [image vector, START, w_1 .. w_L], targets [null, w_1 .. w_L, END]; END = START = V+1;
loss = weight * (-sum_r rowlik_r) / (n (L+2)).  Used by tests/test_lm_grad_rules_cpu.py, test_gpu_wgrad.py and
test_gpu_lm_grad.py.

`variant` makes the deliberately wrong restatements the teeth tests need: "swap_fo" (f and o gates swapped), "div_L1" (divisor
n (L+1)), "image_step" (the image step's output scored against END as well)."""
import numpy as np

PARAMS = ("lm_enc_w", "lm_enc_b", "lm_emb", "lstm_w", "lstm_b", "lm_out_w", "lm_out_b")
TENSORS = PARAMS + ("codes",)


def draw_labels(n, L, V, rng):
    """(n, L) int32 rows of words then zeros: row 0 is full width; with n >= 2 row 1 is empty; with L >= 2 row 0 repeats a word;
    with n >= 3 row 2 starts with row 0's first word (a word fed in two rows)."""
    lab = np.zeros((n, L), np.int32)
    for r in range(n):
        k = int(rng.integers(0, L + 1))
        lab[r, :k] = rng.integers(1, V + 1, k)
    lab[0] = rng.integers(1, V + 1, L)
    if L >= 2:
        lab[0, L - 1] = lab[0, 0]
    if n >= 2:
        lab[1] = 0
    if n >= 3:
        lab[2, 0] = lab[0, 0]
    return lab


def draw_codes(n, D, rng):
    return np.maximum(rng.standard_normal((n, D)), 0).astype(np.float32)


def _t(a, dtype):
    import torch
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return a.detach().to(dtype).clone()


def forward(P, codes, labels, weight=1.0, variant=None):
    """loss (0-d tensor) and rowlik (n,) from a dict of tensors P (any dtype) and codes."""
    import torch
    lab = np.asarray(labels)
    n, L = lab.shape
    Hd = P["lstm_w"].shape[1] // 4
    E = P["lstm_w"].shape[0] - Hd
    Wx, Wh = P["lstm_w"][:E], P["lstm_w"][E:]
    V1 = P["lm_out_w"].shape[0]
    lens = (lab != 0).sum(1)

    def step(xpre, h, c):
        a = xpre + h @ Wh
        i, f, o, g = a[:, :Hd], a[:, Hd:2 * Hd], a[:, 2 * Hd:3 * Hd], a[:, 3 * Hd:]
        if variant == "swap_fo":
            f, o = o, f
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        c2 = f * c + i * g
        return o * torch.tanh(c2), c2

    def logp(h):
        return torch.log_softmax(h @ P["lm_out_w"].t() + P["lm_out_b"], dim=1)

    enc = torch.relu(codes @ P["lm_enc_w"].t() + P["lm_enc_b"])
    zero = torch.zeros(n, Hd, dtype=codes.dtype)
    h, c = step(P["lstm_b"] + enc @ Wx, zero, zero)                          # the image step: its output is not scored
    rowlik = torch.zeros(n, dtype=codes.dtype)
    if variant == "image_step":
        rowlik = rowlik + logp(h)[:, V1 - 1]
    h, c = step(P["lstm_b"] + P["lm_emb"][V1 - 1][None] @ Wx, h, c)          # START (id V+1)
    for j in range(1, L + 2):
        act = np.nonzero(lens + 1 >= j)[0]                                    # rows with a target at this position
        if len(act) == 0:
            break
        tgt = np.array([lab[r, j - 1] if j <= lens[r] else V1 for r in act])
        lp = logp(h[act])
        add = torch.zeros(n, dtype=codes.dtype).index_put((torch.from_numpy(act),), lp[torch.arange(len(act)), torch.from_numpy(tgt - 1)])
        rowlik = rowlik + add
        fed = np.nonzero(lens >= j)[0]                                        # rows whose target is a word: it is fed next
        if len(fed) == 0:
            break
        x = P["lm_emb"][torch.from_numpy(lab[fed, j - 1].astype(np.int64) - 1)]
        h2, c2 = step(P["lstm_b"] + x @ Wx, h[fed], c[fed])
        idx = (torch.from_numpy(fed),)
        h = h.index_put(idx, h2)
        c = c.index_put(idx, c2)
    div = n * (L + 1) if variant == "div_L1" else n * (L + 2)
    return weight * (-rowlik.sum()) / div, rowlik


def lm_grad(W, codes, labels, weight=1.0, dtype=None, variant=None):
    """dict: the eight gradients as numpy float64 arrays, `loss` (float) and `rowlik` (n,) float64."""
    import torch
    dtype = dtype or torch.float64
    with torch.enable_grad():                       # (the oracle switches autograd off for the whole process)
        P = {k: _t(W[k], dtype).requires_grad_() for k in PARAMS}
        x = _t(codes, dtype).requires_grad_()
        loss, rowlik = forward(P, x, labels, weight, variant)
        loss.backward()
    out = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).double().numpy() for k in PARAMS}
    out["codes"] = x.grad.double().numpy()
    out["loss"] = float(loss.detach())
    out["rowlik"] = rowlik.detach().double().numpy()
    return out


def loss_only(W, codes, labels, weight=1.0, variant=None):
    """The float64 loss alone, no graph (finite differences, line searches)."""
    import torch
    with torch.no_grad():
        P = {k: _t(W[k], torch.float64) for k in PARAMS}
        return float(forward(P, _t(codes, torch.float64), labels, weight, variant)[0])


def fed_rows(labels, V):
    """0-based rows of lm_emb that receive a gradient: every word of the labels, and START."""
    return sorted(set(int(w) - 1 for w in np.asarray(labels).ravel() if w != 0) | {V})
