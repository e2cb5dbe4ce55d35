"""Gradient clipping's rules, restated (docs/SEMANTICS.md, "Gradient clipping"); not a test file.

    sumsq = sum over every element of every segment of (double)g * (double)g
    norm  = sqrt(sumsq);  c = max_norm / (norm + 1e-6);  scale = c < 1 ? (float)c : 1.0f
    a sumsq that is not finite, and max_norm = 0, give scale = 1.0f
    Adam reads g * scale (one rounded fp32 multiply) where it read g

`sumsq_ref` is `math.fsum` of the exact double squares: the correctly rounded sum.

THE BAR of the device's sumsq.  The reduction as built (optim.hip): a lane of grad_sumsq_kernel adds at most 18 squares of its
chunk (one in front of the first 16-byte aligned element, four vectors of four, one behind the last whole vector), a fixed tree
over the 256 lanes adds 8 levels (six inside a wave, two across the four waves), lane l of grad_norm_finish_kernel adds the
partials l, l + 256, .. (ceil(chunks / 256) of them) and the same tree adds 8 more.  `chain_length(sizes)` is that longest chain
of additions, L.  All terms are non-negative and every addition is off by at most 2^-53 relative, so the result is within
(1 + 2^-53)^L - 1 <= (L + 1) * 2^-53 of the exact sum (L * 2^-53 << 1), and fsum adds half a unit of its own: the bar is
(L + 1) * 2^-53 relative.  Nothing in it looks at a device result.  L <= 64 + ceil(chunks / 256) is asserted, so that an
inflated L cannot hide a fault.

`emulate_sumsq` walks the kernels' order in numpy float64 (tests/test_clip_rules_cpu.py holds it against the bar).
"""
import math

import numpy as np

from tests import optim_rules as R

CHUNK = 4096
U53 = 2.0 ** -53
F32 = np.float32


def sumsq_ref(segments):
    """math.fsum of the exact double squares of every element of every segment (a NaN or inf in g: what IEEE gives)"""
    sq = [np.asarray(g, np.float64).reshape(-1) ** 2 for g in segments]
    allsq = np.concatenate(sq) if sq else np.zeros(0)
    if not np.isfinite(allsq).all():
        return float(allsq.sum())
    return math.fsum(allsq.tolist())


def scale_rule(sumsq, max_norm):
    """the fp32 scale of the rule, and the double norm: (np.float32, float)"""
    if max_norm < 0 or math.isnan(max_norm):
        raise ValueError("max_norm must be >= 0 or inf")
    norm = math.sqrt(sumsq) if sumsq >= 0 and not math.isnan(sumsq) else float("nan")
    if max_norm == 0 or not math.isfinite(sumsq):
        return F32(1.0), norm
    c = max_norm / (norm + 1e-6)
    return (F32(c) if c < 1.0 else F32(1.0)), norm


def scaled(g, scale):
    """g * scale, one rounded fp32 multiply an element"""
    with np.errstate(all="ignore"):
        out = np.asarray(g, F32) * F32(scale)
    assert out.dtype == F32
    return out


def adam_step32_scaled(p, g, m, v, t, scale, **kw):
    """optim_rules.adam_step32 on g * scale"""
    return R.adam_step32(p, scaled(g, scale), m, v, t, **kw)


def total_chunks(sizes):
    return sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


def chain_length(sizes):
    """L: the longest chain of additions from an element to the record, for segments of these sizes in one or two tables"""
    lane = 0
    for n in sizes:
        vecs = (min(int(n), CHUNK) + 3) // 4                      # whole vectors a chunk of this segment can hold, at most
        lane = max(lane, min(18, 4 * ((vecs + 255) // 256) + 2))
    T = total_chunks(sizes)
    L = lane + 8 + (T + 255) // 256 + 8
    assert L <= 64 + (T + 255) // 256
    return L


def sumsq_bar(sizes):
    """relative"""
    return (chain_length(sizes) + 1) * U53


def within_bar(got, want, sizes):
    return abs(got - want) <= sumsq_bar(sizes) * want


def ulps32(a, b):
    """distance of two finite fp32 values of one sign in units in the last place"""
    ia, ib = (int(np.asarray(x, F32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def _tree256(x):
    """block_sum256: a butterfly over the 64 lanes of each wave (xor 32, 16, .., 1), then (w0 + w1) + (w2 + w3)"""
    x = np.asarray(x, np.float64).reshape(4, 64).copy()
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lanes ^ d]
    return (x[0, 0] + x[1, 0]) + (x[2, 0] + x[3, 0])


def emulate_sumsq(segments, offsets=None):
    """The two kernels' order of additions in float64.  offsets[i]: floats by which segment i's g is off 16-byte alignment."""
    offsets = offsets or [0] * len(segments)
    partials = []
    for g, off in zip(segments, offsets):
        sq = np.asarray(g, np.float64).reshape(-1) ** 2
        n = len(sq)
        head = (4 - off) % 4
        for lo in range(0, n, CHUNK):
            hi = min(lo + CHUNK, n)
            first = head if lo <= head else head + (lo - head + 3) // 4 * 4
            first = min(first, hi)
            nvec = (hi - first) // 4
            acc = np.zeros(256)
            for i in range(lo, first):
                acc[i - lo] += sq[i]
            for u in range((nvec + 255) // 256):
                for e in range(4):
                    idx = first + 4 * (u * 256 + np.arange(256)) + e
                    ok = (u * 256 + np.arange(256)) < nvec
                    acc[ok] += sq[idx[ok]]
            tail = first + 4 * nvec
            for i in range(tail, hi):
                acc[i - tail] += sq[i]
            partials.append(_tree256(acc))
    acc = np.zeros(256)
    for i, x in enumerate(partials):
        acc[i % 256] += x
    return float(_tree256(acc))


# ---- four wrong rules: each must be rejected by the comparisons the GPU tests make (tests/test_clip_rules_cpu.py) ----
def wrong_scale_after_decay(p, g, m, v, t, scale, **kw):
    """(g + wd * p) * scale in place of g * scale + wd * p"""
    b1, c1, b2, c2, eps, wd, nstep = R.scalars32(t, **kw)
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    if wd > 0:
        g = g + wd * p
    g = g * F32(scale)
    m = b1 * m + c1 * g
    v = b2 * v + (c2 * g) * g
    return p + (nstep * m) / (np.sqrt(v) + eps), m, v


def wrong_per_tensor_scales(segments, max_norm):
    """a norm and a scale per tensor"""
    return [scale_rule(sumsq_ref([g]), max_norm)[0] for g in segments]


def wrong_scale_without_sqrt(sumsq, max_norm):
    c = max_norm / (sumsq + 1e-6)
    return F32(c) if c < 1.0 else F32(1.0)


def wrong_sum_abs(segments):
    return math.fsum(np.abs(np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in segments])).tolist())


def trial_gradient(n, seed):
    """n float32 values, magnitudes log-uniform over 1e-6 .. 10 with random signs, a tenth exactly zero, a few denormals"""
    rng = np.random.RandomState(seed)
    g = (10.0 ** rng.uniform(-6, 1, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    g[rng.rand(n) < 0.1] = 0.0
    den = np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1e-38], F32)
    idx = rng.permutation(n)[:min(n, len(den))]
    g[idx] = den[:len(idx)]
    return g
