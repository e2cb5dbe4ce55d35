"""Gradient clipping and Adam's saved state without a GPU: tests/clip_rules.py on typed-in cases; the emulation of the kernels'
order against the bar; four wrong rules that the comparisons of tests/test_gpu_grad_clip.py must reject; the new prototypes in
the header, the binding and the Lua cdef; the hook header; train.py's flags; the .npz key scheme."""
import math
import os
import re

import numpy as np

from tests import clip_rules as K
from tests import optim_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OPTS = dict(learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the rules on typed-in cases ---------------------------------------------------------------------------------------------------
def test_sumsq_norm_and_scale_on_typed_in_cases():
    g = [np.array([3.0, -4.0], F32), np.array([12.0], F32)]
    assert K.sumsq_ref(g) == 169.0
    s, norm = K.scale_rule(169.0, 6.5)
    assert norm == 13.0 and s == F32(6.5 / (13.0 + 1e-6)) and s < F32(0.5)
    assert K.scale_rule(169.0, 13.0)[0] == F32(13.0 / (13.0 + 1e-6)) < F32(1.0)      # the 1e-6 clips a norm AT the limit by an ulp or so
    assert K.scale_rule(169.0, 14.0)[0] == F32(1.0)
    assert K.scale_rule(169.0, float("inf")) == (F32(1.0), 13.0)
    assert K.scale_rule(169.0, 0.0)[0] == F32(1.0)
    assert K.scale_rule(0.0, 1.0) == (F32(1.0), 0.0)                                    # c = 1e6
    for bad in (float("nan"), float("inf")):
        s, norm = K.scale_rule(bad, 1.0)
        assert s == F32(1.0) and not math.isfinite(norm)
    for bad in (-1.0, float("nan")):
        try:
            K.scale_rule(1.0, bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    assert K.sumsq_ref([np.array([1e-45, 0.0, -0.0], F32)]) == float(F32(1e-45)) ** 2   # a denormal's square is exact in double
    assert math.isnan(K.sumsq_ref([np.array([1.0, np.nan], F32)])) and math.isinf(K.sumsq_ref([np.array([1.0, np.inf], F32)]))


def test_scaled_adam_is_adam_on_the_rounded_product():
    p, g = R.trial_data(257, 1, 3)
    g = g[0]
    m = np.zeros_like(p); v = np.zeros_like(p)
    s = F32(0.3)
    a = K.adam_step32_scaled(p, g, m, v, 2, s, weight_decay=1e-2, **OPTS)
    b = R.adam_step32(p, (g.astype(F32) * s).astype(F32), m, v, 2, weight_decay=1e-2, **OPTS)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    one = K.adam_step32_scaled(p, g, m, v, 2, F32(1.0), weight_decay=1e-2, **OPTS)
    for x, y in zip(one, R.adam_step32(p, g, m, v, 2, weight_decay=1e-2, **OPTS)):
        assert np.array_equal(_bits(x), _bits(y))                                       # scale = 1 is the unclipped step's bits


def test_chain_length_and_its_cap():
    assert K.chain_length([1]) == 6 + 8 + 1 + 8
    assert K.chain_length([4096]) == 18 + 8 + 1 + 8
    assert K.chain_length([4096 * 257]) == 18 + 8 + 2 + 8
    real = [256 * 512 * 9, 256, 72 * 256, 72, 4096 * 25088, 4096, 4096 * 4096, 4096, 5 * 4096, 5, 512 * 4096, 512, 10499 * 512,
            1024 * 2048, 2048, 10498 * 512, 10498]                                      # the 17 segments at the real dimensions
    T = K.total_chunks(real)
    assert K.chain_length(real) == 34 + (T + 255) // 256 <= 64 + (T + 255) // 256
    assert K.sumsq_bar(real) < 2e-14                                                    # the norm is good to 1e-14 at the real model


def test_the_emulated_reduction_sits_inside_the_bar():
    """the kernels' order of additions in float64 (clip_rules.emulate_sumsq) on test_gpu_adam's kind of data"""
    worst = 0.0
    for n, off in ((1, 0), (5, 3), (257, 1), (4095, 2), (4097, 3), (2 * 4096 + 5, 1), (65541, 0), (300000, 2)):
        g = K.trial_gradient(n, seed=n)
        want, got = K.sumsq_ref([g]), K.emulate_sumsq([g], [off])
        assert K.within_bar(got, want, [n]), (n, off, got, want)
        worst = max(worst, abs(got - want) / want / K.U53)
        ones = np.ones(n, F32)
        assert K.emulate_sumsq([ones], [off]) == float(n)                               # every element once
    print("worst error of the emulation: %.2f units of 2^-53" % worst)
    sizes = [(1, 4, 7, 64, 4099)[i % 5] for i in range(21)]
    segs = [K.trial_gradient(n, seed=100 + i) for i, n in enumerate(sizes)]
    assert K.within_bar(K.emulate_sumsq(segs, [i % 4 for i in range(21)]), K.sumsq_ref(segs), sizes)
    # the fp32 scale of the emulated sum is the reference's, to the ulp the GPU test allows
    for frac in (0.5, 0.9, 0.999):
        want = K.sumsq_ref(segs)
        mx = frac * math.sqrt(want)
        assert K.ulps32(K.scale_rule(K.emulate_sumsq(segs), mx)[0], K.scale_rule(want, mx)[0]) <= 1


# ---- four wrong rules --------------------------------------------------------------------------------------------------------------
def _case():
    sizes = (5, 64, 257)
    segs = []
    for i, n in enumerate(sizes):
        p, g = R.trial_data(n, 1, 20 + i)
        segs.append((p, (g[0] * F32(10.0 ** i)).astype(F32), (p * F32(0.1)).astype(F32), np.abs(p * F32(0.01)).astype(F32)))
    return segs


def _differs(a, b):
    return any(not np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_scale_applied_after_the_weight_decay_is_rejected():
    segs = _case()
    sumsq = K.sumsq_ref([s[1] for s in segs])
    scale, norm = K.scale_rule(sumsq, 0.5 * math.sqrt(sumsq))
    assert scale < F32(0.51)
    opts = dict(OPTS, weight_decay=1e-2)
    for p, g, m, v in segs:
        assert _differs(K.wrong_scale_after_decay(p, g, m, v, 3, scale, **opts), K.adam_step32_scaled(p, g, m, v, 3, scale, **opts))
    # (without decay the two are one rule: the case above needs wd > 0, which is why the GPU test runs wd = 1e-2)
    p, g, m, v = segs[0]
    none = dict(OPTS, weight_decay=0.0)
    assert not _differs(K.wrong_scale_after_decay(p, g, m, v, 3, scale, **none), K.adam_step32_scaled(p, g, m, v, 3, scale, **none))


def test_a_per_tensor_norm_is_rejected():
    segs = _case()
    gs = [s[1] for s in segs]
    sumsq = K.sumsq_ref(gs)
    mx = 0.5 * math.sqrt(sumsq)
    scale = K.scale_rule(sumsq, mx)[0]
    per = K.wrong_per_tensor_scales(gs, mx)
    assert all(K.ulps32(s, scale) > 1 for s in per)                                     # the scale comparison (1 ulp) rejects each
    assert any(s == F32(1.0) for s in per)                                              # a small tensor would not be clipped at all
    for (p, g, m, v), s in zip(segs, per):
        assert _differs(K.adam_step32_scaled(p, g, m, v, 1, s, **OPTS), K.adam_step32_scaled(p, g, m, v, 1, scale, **OPTS))


def test_sumsq_without_the_square_root_is_rejected():
    gs = [s[1] for s in _case()]
    sumsq = K.sumsq_ref(gs)
    assert sumsq > 4.0
    mx = 0.5 * math.sqrt(sumsq)
    assert K.ulps32(K.wrong_scale_without_sqrt(sumsq, mx), K.scale_rule(sumsq, mx)[0]) > 1


def test_a_sum_of_absolute_values_is_rejected():
    gs = [s[1] for s in _case()]
    sizes = [len(g) for g in gs]
    assert not K.within_bar(K.wrong_sum_abs(gs), K.sumsq_ref(gs), sizes)
    ones = [np.full(7, 2.0, F32)]                                                       # (on ones the two sums agree: the seams test
    assert K.wrong_sum_abs(ones) != K.sumsq_ref(ones) == 28.0                           # alone would not tell them apart, twos do)


# ---- the three copies of the C ABI ---------------------------------------------------------------------------------------------------
def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"\bint\s+(dc_[a-z0-9_]+)\s*\([^;]*?\)\s*;", text)}


NEW = (("dc_train_set_grad_clip", 2), ("dc_train_grad_norm", 3), ("dc_op_grad_norm", 7), ("dc_train_get_state", 5),
       ("dc_train_set_state", 5))


def test_prototypes_are_in_the_header_the_binding_and_the_lua_cdef():
    from densecap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "densecap.h")).read()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    hp, lp = _prototypes(hdr), _prototypes(cdef)
    for name, nargs in NEW:
        assert name in hp and lp.get(name) == hp[name], name
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGS[name][1]) == hp[name].count(",") + 1 == nargs, name
    shim = open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()
    assert "dc_train_set_grad_clip" in shim and "grad_clip" in shim


def test_the_hook_header_is_bound_exported_and_not_in_lua():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "densecap_amd", "lib", "libdensecap_hip.so")):
        g.build()
    from densecap_amd import _lib
    src = open(os.path.join(ROOT, "include", "densecap_debug_clip.h")).read()
    hooks = sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))
    assert hooks == sorted(_lib._CLIP_HOOK_SIGS) == ["dc_debug_adam_multi_clip"]
    lib = _lib.lib()
    for name, _ in NEW:
        assert hasattr(lib, name), name
    for name in hooks:
        assert hasattr(lib, name) and name not in _lib.EXPORTED_SYMBOLS
        proto = _prototypes(src)[name]
        assert len(_lib._CLIP_HOOK_SIGS[name][1]) == proto.count(",") + 1 == 13
    for f in ("densecap_hip.lua", "DenseCapModelHIP.lua"):
        assert "dc_debug_adam_multi_clip" not in open(os.path.join(ROOT, "lua", f)).read()
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "densecap_debug_clip.h":
            assert "dc_debug_adam_multi_clip" not in open(os.path.join(ROOT, "include", other)).read(), other


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_the_new_flags_parse_with_their_defaults():
    from densecap_amd import train as T
    o = T.build_parser().parse_args([])
    assert o.grad_clip == 0.0 and o.save_optim_state == 0 and o.resume_optim_state == ""
    o = T.build_parser().parse_args(["-grad_clip", "inf", "-save_optim_state", "1", "-resume_optim_state", "a.optim.npz"])
    assert o.grad_clip == float("inf") and o.save_optim_state == 1 and o.resume_optim_state == "a.optim.npz"
    assert T.optim_state_path("out/checkpoint.t7") == os.path.join("out", "checkpoint.optim.npz")
    src = open(os.path.join(ROOT, "densecap_amd", "train.py")).read()
    assert src.index("not reference flags") < src.index('"-grad_clip"') and "1.1 GB" in src
    assert "are not saved" not in T.__doc__ and "-resume_optim_state" in T.__doc__
    assert "--grad_clip" in open(os.path.join(ROOT, "tools", "train_step_bench.py")).read()


def test_the_documents_describe_clipping_and_the_saved_state():
    sem = open(os.path.join(ROOT, "docs", "SEMANTICS.md")).read()
    assert "\n## Gradient clipping" in sem and "dc_train_set_state" in sem
    assert "`m`, `v` and `t` are not saved" not in sem
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "grad_sumsq_kernel" in design and "dc_train_get_state" in design


# ---- the .npz key scheme ---------------------------------------------------------------------------------------------------------------
def test_the_npz_key_scheme_round_trips(tmp_path):
    from densecap_amd import ops
    from densecap_amd.model import flatten_train_state, unflatten_train_state
    from tests.test_gpu_dims import set_weights
    W = set_weights("minimal")
    rng = np.random.default_rng(0)
    names = list(ops.WEIGHT_KEYS) + list(ops.cnn_state_keys())
    assert len(ops.WEIGHT_KEYS) == 21 and len(ops.cnn_state_keys()) == 18

    def shape(k):
        if k.startswith("conv_"):
            return tuple(W[k[:6]][int(k[6:])].shape)
        return tuple(W[k].shape)

    state = {mom: {k: rng.standard_normal(shape(k)).astype(F32) for k in names} for mom in ("m", "v")}
    state.update(t=50000, cnn_t=49000)
    flat = flatten_train_state(state)
    assert sorted(flat) == sorted(["t", "cnn_t"] + ["%s/%s" % (mom, k) for mom in "mv" for k in names])
    path = str(tmp_path / "ckpt.optim.npz")
    np.savez(path, **flat)
    assert os.path.exists(path)                                                         # (no second .npz is appended)
    with np.load(path) as z:
        back = unflatten_train_state(z)
    assert back["t"] == 50000 and back["cnn_t"] == 49000
    for mom in ("m", "v"):
        assert sorted(back[mom]) == sorted(names)
        for k in names:
            assert back[mom][k].shape == state[mom][k].shape and np.array_equal(_bits(back[mom][k]), _bits(state[mom][k])), (mom, k)
    try:
        unflatten_train_state(dict(flat, **{"w/fc7_w": np.zeros(1, F32)}))
    except ValueError:
        pass
    else:
        raise AssertionError("a key outside the scheme was accepted")
