"""tests/optim_rules.py against itself (no GPU): the float32 restatement of the Adam step -- the one the device kernel must equal
bit for bit -- agrees with a float64 evaluation of optim_updates.lua's formula within a bar that the float64 run supplies, and
that bar has teeth: three plausible wrong rules fall outside it."""
import os
import re

import numpy as np
import pytest

from tests import optim_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# an lr at which a step is far above p's own rounding, and a decay large enough to matter beside the gradients
OPTS = dict(learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=1e-2)
N = 4096


def _reference(p0, grads, **opts):
    ref = R.Adam64WithBound(p0, **opts)
    for g in grads:
        ref.step(g)
    return ref


def _miss(x, ref64, bar):
    """fraction of elements outside the bar"""
    return float((np.abs(np.asarray(x, np.float64) - ref64) > bar).mean())


@pytest.mark.parametrize("steps", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_float32_restatement_meets_the_float64_bar(steps, wd):
    opts = dict(OPTS, weight_decay=wd)
    p0, grads = R.trial_data(N, steps, seed=steps)
    ref = _reference(p0, grads, **opts)
    p, m, v = R.run32(R.adam_step32, p0, grads, **opts)
    for name, x, r, bar in (("p", p, ref.p, ref.bar_p), ("m", m, ref.m, ref.bar_m), ("v", v, ref.v, ref.bar_v)):
        err = np.abs(x.astype(np.float64) - r)
        print("%s after %d steps: worst err / bar %.3f, bar / |step| median %.2e" % (
            name, steps, float(np.max(err / np.maximum(bar, 1e-300))), float(np.median(ref.bar_p) / opts["learning_rate"])))
        assert np.isfinite(bar).all()
        assert (err <= bar).all(), (name, steps, float(err.max()))
    # the bar is small beside what a step does: it checks the update, not only p
    moved = np.abs(ref.p - p0.astype(np.float64))
    assert np.median(ref.bar_p / np.maximum(moved, 1e-300)) < 1e-2


@pytest.mark.parametrize("steps", [1, 2, 1000])
@pytest.mark.parametrize("rule", [R.wrong_eps_inside_sqrt32, R.wrong_no_bias_correction32, R.wrong_decay_after_moments32])
def test_wrong_rules_fall_outside_the_bar(rule, steps):
    p0, grads = R.trial_data(N, steps, seed=steps)
    ref = _reference(p0, grads, **OPTS)
    p, _m, _v = R.run32(rule, p0, grads, **OPTS)
    miss = _miss(p, ref.p, ref.bar_p)
    print("%s, %d steps: %.1f%% of the elements outside the bar" % (rule.__name__, steps, 100 * miss))
    assert miss > 0.25


def test_scalars_are_double_then_one_cast():
    b1, c1, b2, c2, eps, wd, nstep = R.scalars32(3, **OPTS)
    assert c1 == np.float32(1.0 - 0.9) and c1 != np.float32(1.0) - np.float32(0.9)       # 1 - beta1 in double, not in float
    assert c2 == np.float32(1.0 - 0.999)
    want = 1e-3 * np.sqrt(1.0 - 0.999 ** 3) / (1.0 - 0.9 ** 3)
    assert nstep == -np.float32(want) and nstep.dtype == np.float32


def test_zero_gradient_keeps_decaying_moments_and_moves_p():
    p = np.ones(4, np.float32); m = np.full(4, 0.5, np.float32); v = np.full(4, 0.25, np.float32)
    p2, m2, v2 = R.adam_step32(p, np.zeros(4, np.float32), m, v, 5, **dict(OPTS, weight_decay=0.0))
    assert (m2 == np.float32(0.9) * np.float32(0.5)).all() and (v2 == np.float32(0.999) * np.float32(0.25)).all()
    assert (p2 < p).all()


def test_bf16_host_rule():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 0.0, np.inf, 1e-40], np.float32)      # ties to even both ways
    b = R.bf16_bits_host_rule(x)
    assert list(b[:3]) == [0x3f80, 0x3f80, 0x3f82] and b[5] == 0x7f80
    nan = np.array([0x7f800001, 0xffc00000, 0x7fbfffff], np.uint32).view(np.float32)
    assert list(R.bf16_bits_host_rule(nan)) == [0x7fc0, 0xffc0, 0x7fff]


def test_hooks_of_the_optimiser_header_are_bound():
    from densecap_amd import _lib
    src = open(os.path.join(ROOT, "include", "densecap_debug_optim.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    hooks = sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))
    assert hooks == sorted(_lib._OPTIM_HOOK_SIGS) and len(hooks) == 3
    for name in ("dc_train_begin", "dc_train_step", "dc_train_end", "dc_get_weights", "dc_op_adam"):
        assert name in _lib._SIGS
