"""The optimiser's rules, twice (docs/SEMANTICS.md, "Training step").

`adam_step32` is the float32 restatement the device kernel is compared with BIT FOR BIT: the seven scalars are computed in
double and cast to float once per step, then every element goes through one correctly rounded fp32 operation at a time, no FMA,
in the order TH evaluates train.lua's `grad_params:add(weight_decay, params)` and optim_updates.lua:56-84's `mul`, `add(value,
x)`, `addcmul`, `sqrt`, `add`, `addcdiv`:

    g' = wd > 0 ? g + wd * p : g
    m  = b1 * m + c1 * g'
    v  = b2 * v + (c2 * g') * g'
    p  = p + ((-step) * m) / (sqrt(v) + eps)

`adam_step64` is the same formula in float64 with the scalars left in double: what the reference computes up to rounding.

`Adam64WithBound` runs the float64 rule and carries, element by element, a bound on how far ANY float32 evaluation of the rule
in the order above can be from it: the standard model (every fp32 operation and every scalar's cast is off by at most
u = 2^-24 relative, plus one denormal step 2^-149 absolute), propagated to first order through the recurrences with the
constants rounded up, times FACTOR = 2 for the second-order terms.  Nothing in it looks at a float32 result: the bar comes from
the float64 reference alone (the derivation tests/grad_bars.py uses: bar = a fixed factor times an error the reference itself
supplies).
"""
import math

import numpy as np

DEFAULTS = dict(learning_rate=1e-5, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=1e-6)     # train_opts.lua
U = 2.0 ** -24
ETA = 2.0 ** -149
FACTOR = 2.0


def _opts(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown option(s): %s" % sorted(unknown))
    return dict(DEFAULTS, **kw)


def step_size(o, t):
    """optim_updates.lua:78-80 in double: lr * sqrt(1 - beta2^t) / (1 - beta1^t), t counting from 1"""
    return o["learning_rate"] * math.sqrt(1.0 - o["beta2"] ** t) / (1.0 - o["beta1"] ** t)


def scalars32(t, **kw):
    """(b1, c1, b2, c2, eps, wd, nstep) as np.float32: each computed in double, cast to float once"""
    o = _opts(kw)
    f = np.float32
    return (f(o["beta1"]), f(1.0 - o["beta1"]), f(o["beta2"]), f(1.0 - o["beta2"]), f(o["epsilon"]), f(o["weight_decay"]),
            -f(step_size(o, t)))


def adam_step32(p, g, m, v, t, **kw):
    """One step of the float32 restatement on float32 arrays; returns new (p, m, v).  The inputs are not changed."""
    b1, c1, b2, c2, eps, wd, nstep = scalars32(t, **kw)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if wd > 0:
            g = g + wd * p
        m = b1 * m + c1 * g
        v = b2 * v + (c2 * g) * g
        p = p + (nstep * m) / (np.sqrt(v) + eps)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adam_step64(p, g, m, v, t, **kw):
    """One step of optim_updates.lua's formula in float64 (scalars in double); returns new (p, m, v)."""
    o = _opts(kw)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if o["weight_decay"] > 0:
        g = g + o["weight_decay"] * p
    m = o["beta1"] * m + (1.0 - o["beta1"]) * g
    v = o["beta2"] * v + (1.0 - o["beta2"]) * g * g
    p = p - step_size(o, t) * m / (np.sqrt(v) + o["epsilon"])
    return p, m, v


class Adam64WithBound:
    """The float64 rule from (p0, m = 0, v = 0) with the running error bound described in the module's docstring.  After any
    number of `step(g)` calls: p, m, v (float64) and bar_p, bar_m, bar_v, the per-element bars a float32 evaluation must meet."""

    def __init__(self, p0, **kw):
        self.o = _opts(kw)
        self.p = np.asarray(p0, np.float64).copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.ep = np.zeros_like(self.p)      # p0 is a float32 array: no error yet
        self.em = np.zeros_like(self.p)
        self.ev = np.zeros_like(self.p)
        self.t = 0

    def step(self, g):
        o, u = self.o, U
        b1, b2, eps, wd = o["beta1"], o["beta2"], o["epsilon"], o["weight_decay"]
        c1, c2 = 1.0 - b1, 1.0 - b2
        self.t += 1
        step = step_size(o, self.t)
        g = np.asarray(g, np.float64)
        eg = np.zeros_like(g)
        if wd > 0:                                            # g' = g + wd * p: wd's cast, the product, the sum
            eg = wd * self.ep + 2 * u * np.abs(wd * self.p) + u * np.abs(g + wd * self.p) + 2 * ETA
            g = g + wd * self.p
        # m = b1 m + c1 g': two casts, two products, one sum
        self.em = b1 * self.em + c1 * eg + 3 * u * (np.abs(b1 * self.m) + np.abs(c1 * g)) + 3 * ETA
        self.m = b1 * self.m + c1 * g
        # v = b2 v + (c2 g') g': two casts, three products, one sum; d(g'^2) = 2 |g'| eg + eg^2
        self.ev = b2 * self.ev + c2 * (2 * np.abs(g) * eg + eg * eg) + 4 * u * (np.abs(b2 * self.v) + c2 * g * g) + 4 * ETA
        self.v = b2 * self.v + c2 * g * g
        # D = sqrt(v) + eps: |sqrt(a) - sqrt(b)| <= min(|a - b| / (2 sqrt(min(a, b))), sqrt(|a - b|))
        root = np.sqrt(self.v)
        low = np.sqrt(np.maximum(self.v - self.ev, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            es = np.where(low > 0, np.minimum(self.ev / (2 * low), np.sqrt(self.ev)), np.sqrt(self.ev))
        D = root + eps
        eD = es + u * root + 2 * u * D + 2 * ETA              # sqrt's rounding, eps' cast, the sum
        # N = (-step) m: step's cast and the product
        N = step * self.m
        eN = step * self.em + 2 * u * np.abs(N) + ETA
        # delta = N / D
        delta = N / D
        room = D - eD
        with np.errstate(divide="ignore", invalid="ignore"):
            ed = np.where(room > 0, (eN + np.abs(delta) * eD) / room, np.inf) + u * np.abs(delta) + ETA
        self.p = self.p - delta
        self.ep = self.ep + ed + u * np.abs(self.p) + ETA
        return self

    @property
    def bar_p(self):
        return FACTOR * self.ep

    @property
    def bar_m(self):
        return FACTOR * self.em

    @property
    def bar_v(self):
        return FACTOR * self.ev


# ---- three wrong rules: each must fall outside the bar (tests/test_optim_rules_cpu.py) ----
def wrong_eps_inside_sqrt32(p, g, m, v, t, **kw):
    b1, c1, b2, c2, eps, wd, nstep = scalars32(t, **kw)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    if wd > 0:
        g = g + wd * p
    m = b1 * m + c1 * g
    v = b2 * v + (c2 * g) * g
    return p + (nstep * m) / np.sqrt(v + eps), m, v


def wrong_no_bias_correction32(p, g, m, v, t, **kw):
    o = _opts(kw)
    b1, c1, b2, c2, eps, wd, _ = scalars32(t, **kw)
    nstep = -np.float32(o["learning_rate"])
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    if wd > 0:
        g = g + wd * p
    m = b1 * m + c1 * g
    v = b2 * v + (c2 * g) * g
    return p + (nstep * m) / (np.sqrt(v) + eps), m, v


def wrong_decay_after_moments32(p, g, m, v, t, **kw):
    """the decay outside the moments (a decoupled decay): m and v see the raw gradient, p loses lr * wd * p beside the step"""
    o = _opts(kw)
    b1, c1, b2, c2, eps, wd, nstep = scalars32(t, **kw)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    m = b1 * m + c1 * g
    v = b2 * v + (c2 * g) * g
    return p + (nstep * m) / (np.sqrt(v) + eps) - np.float32(o["learning_rate"]) * wd * p, m, v


def run32(rule, p0, grads, **kw):
    """`rule` for len(grads) steps from (p0, 0, 0); returns (p, m, v) float32"""
    p = np.asarray(p0, np.float32).copy()
    m = np.zeros_like(p); v = np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        p, m, v = rule(p, g, m, v, t, **kw)
    return p, m, v


# ---- the decode screen's operands, restated (dc_load_weights' host loop) ----
def bf16_bits_host_rule(x):
    """float32 array -> uint16 bf16 bits: round to nearest even; a NaN keeps its top 16 bits with the quiet bit set"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    rne = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return np.where(nan, (u >> 16) | 0x40, rne).astype(np.uint16)


def trial_data(n, steps, seed):
    """p0 (n) float32 around 1 in size, both signs; grads (steps, n) float32 with magnitudes log-uniform over 1e-6 .. 1 and
    random signs, a tenth of them exactly zero"""
    rng = np.random.RandomState(seed)
    p0 = (rng.randn(n) * 0.5).astype(np.float32)
    mag = 10.0 ** rng.uniform(-6, 0, size=(steps, n))
    g = (mag * rng.choice([-1.0, 1.0], size=(steps, n))).astype(np.float32)
    g[rng.rand(steps, n) < 0.1] = 0.0
    return p0, g
