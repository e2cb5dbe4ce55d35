"""The selection rule of the screened greedy decode, restated in torch for the tests.

Scores s_j = fp16(bias_j + sum_k bf16(h_k) bf16(w_jk)); bound b_j = c |h|_2 |w_j|_2 + 2^-10 |s_j| + 2^-100 |w_j|_2 + 2^-24 with
both norms rounded up; L = max_j (s_j - b_j); column j is a candidate iff s_j + b_j >= L.  A row with more than MAX_CAND
candidates, or with a non-finite score or bound, is scanned exactly (`full`)."""
import math

import numpy as np
import torch

MAX_CAND = 64


def bound_c(K):
    """The constant c for K terms, as densecap.hip::screen_bound_c forms it (double, then rounded up to float)."""
    u = 2.0 ** -8
    g = K * 2.0 ** -24
    c = ((2 * u + u * u) + (K / 16.0) * 2.0 ** -18 * (1 + u) * (1 + u) + g / (1 - g)) * (1 + 2.0 ** -8)
    return np.nextafter(np.float32(c), np.float32(np.inf))


def row_norms_up(w):
    """|w_j|_2 of every row in double, rounded up to fp16 (the loader's wnorm), as float32."""
    nr = torch.sqrt((w.double() ** 2).sum(1)) * (1.0 + 1e-9)
    f = nr.half()
    return torch.where(f.double() < nr, torch.nextafter(f, torch.full_like(f, math.inf)), f).float()


def h_norms_up(h):
    """|h_m|_2 as the row tail forms it: fp32 sum of squares, root, times 1.001."""
    return torch.sqrt((h * h).sum(1)) * np.float32(1.001)


def scores_bf16(h, w, bias):
    """The screen's scores with bf16 by casting: products of bf16 values are exact in fp32, the sum is torch's fp32 sum."""
    acc = h.bfloat16().float() @ w.bfloat16().float().t()
    return (acc + bias).half()


def bf16_rne_bits(x):
    """The bf16 bit patterns (uint16 numpy array) of float32 values, rounded to nearest even with integer arithmetic only:
    the 16 bits cut off are compared with half a unit, a tie goes to the even pattern, a carry may run into the exponent
    (up to inf).  Zeros, subnormals and infinities need no case of their own; a NaN becomes 0x7fc0, as torch.bfloat16 makes it."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7fffffff) > 0x7f800000, np.uint16(0x7fc0), r)


def bf16_values(x):
    """bf16(x) as float64 (torch tensor), through bf16_rne_bits."""
    bits = bf16_rne_bits(x).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).astype(np.float64))


def scores_ref64(h, w, bias):
    """bias + sum_k bf16(h_k) bf16(w_jk) in float64: every product of two bf16 values is exact (16 bits), so only the float64
    sum rounds (2^-53 per addition).  What the screen would store with an exact accumulator, before the round to fp16."""
    return bf16_values(h) @ bf16_values(w).t() + torch.as_tensor(bias).double()


def score_tol(h, w, bias, K):
    """How far a stored score may lie from scores_ref64 under the model of DESIGN.md §4.1c, term by term with the exact
    S_j = sum_k |bf16(h_k) bf16(w_jk)| where the proof bounds it by Cauchy-Schwarz:
      (K/16) 2^-18 S_j   the chain of K/16 bf16 MFMA instructions, each off by less than 2^-18 of the sum of magnitudes
      2^-10 |ref|        the bias addition in fp32 and the round to fp16 (2^-11 of the magnitude)
      2^-24              the round to fp16 among its subnormals (2^-25)."""
    S = bf16_values(h).abs() @ bf16_values(w).abs().t()
    return (K / 16.0) * 2.0 ** -18 * S + 2.0 ** -10 * scores_ref64(h, w, bias).abs() + 2.0 ** -24


def cand_bracket(s, hn, wn, c):
    """(lo, hi): the candidate count of every row under `candidates` with the norm hn (1 - 2^-13) and hn (1 + 2^-13).  The
    device sums the Hd <= 2^11 squares in fp32 in an order of its own: the sum moves by less than 2^11 2^-24 = 2^-13 of
    itself, its root by half that, the root's and the 1.001 factor's roundings by 2^-23 more.  Every b_j grows with hn,
    L = max (s - b) falls and s + b rises: the count is monotone in hn, so the device's count lies in [lo, hi]."""
    d = np.float32(2.0 ** -13)
    out = []
    for f in (np.float32(1) - d, np.float32(1) + d):
        mask, _ = candidates(s, bounds(s, hn * f, wn, c))
        out.append(mask.sum(1))
    return out[0], out[1]


def bounds(s, hn, wn, c):
    """b (rows, V1) in fp32, evaluated in the row tail's order."""
    s = s.float()
    ch = (np.float32(c) * hn)[:, None]
    return ch * wn[None, :] + (np.float32(2.0 ** -10) * s.abs() + (np.float32(2.0 ** -100) * wn[None, :] + np.float32(2.0 ** -24)))


def candidates(s, b):
    """(mask (rows, V1), full (rows,)): the candidate columns of every row and whether the row is scanned exactly.  The upper
    end s + b is compared as the row tail keeps it: moved up by 2^-10 of its magnitude + 2^-24, then rounded to fp16."""
    s = s.float()
    bad = ~(torch.isfinite(s).all(1) & torch.isfinite(b).all(1))
    lo = torch.where(torch.isnan(s - b), torch.full_like(s, -math.inf), s - b)
    L = lo.max(1).values
    hi = ((s + b) + ((s + b).abs() * np.float32(2.0 ** -10) + np.float32(2.0 ** -24))).half().float()
    mask = hi >= L[:, None]
    return mask, bad | (mask.sum(1) > MAX_CAND)


def pick(z, mask, full):
    """Token (1-based; 0 = no word) of every row: the largest exact logit among the candidates (all columns where `full`), the
    lower column on ties; NaN and -inf are never entries."""
    use = mask | full[:, None]
    zz = torch.where(use & (z > -math.inf), z, torch.full_like(z, -math.inf))
    tok = torch.argmax(zz, 1) + 1                      # first max
    return torch.where((zz > -math.inf).any(1), tok, torch.zeros_like(tok))
