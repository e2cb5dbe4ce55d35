"""The row kernel of truncated sampling alone (sample_trunc.hip through dc_debug_sample_trunc_rows, the production launcher in
its selection-only mode) on host-made rows: the kept count and the score of the last kept rank against the float64 definition
(tests/sample_trunc_rules.py) -- exactly, but for nucleus rows whose cumulative mass sits within 1e-9 Z of the cut --, the word
against the arg-max over the kept set, the two log-probabilities, the rows without a word, and the hook's refusals."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STAGE, NOISE = 1e-4, 1e-5
P_NEAR_ONE = float(np.float32(1) - np.float32(2.0 ** -24))
SEED = (0x299f31d0 << 32) | 0xa4093822


@pytest.fixture(scope="module")
def ctx():
    from densecap_amd import Context
    c = Context(0)
    yield c
    c.close()


def _rows(V1, seed):
    """64 rows: 40 random, 4 constant, 8 two-valued (the duplicates straddle most ranks), 4 with NaNs (fewer candidates than
    the larger top_k), 2 of all NaN, 1 with +Inf, 3 with -Inf entries, 2 quantised (many exact ties)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((64, V1)) * 3).astype(np.float32)
    X[40], X[41], X[42], X[43] = 0.0, -2.5, 1e30, -0.0
    X[43, ::2] = 0.0                                            # -0 and +0 are equal values: one tie class
    for j, n_hi in enumerate((1, 2, 254, 255, 256, 257, V1 // 2, V1 - 1)):
        hi = rng.permutation(V1)[:min(max(n_hi, 1), V1 - 1)]
        X[44 + j] = -1.0
        X[44 + j, hi] = 1.5
    for j in range(4):
        X[52 + j, rng.permutation(V1)[:V1 - max(3, V1 // (2 + 30 * j))]] = np.nan        # V1/2 ... 3 candidates left
    X[56], X[57] = np.nan, np.nan
    X[57, :] = -np.nan
    X[58, V1 // 3] = np.inf
    X[59, ::3] = -np.inf
    X[60, 1:] = -np.inf                                         # one candidate with mass
    X[61, rng.permutation(V1)[:V1 // 2]] = -np.inf
    X[61, 0] = np.nan
    X[62] = np.round(X[62] * 2) / 2
    X[63] = np.round(X[63])
    return X


def _check(ctx, X, t, temperature, top_k, top_p, stats):
    from densecap_amd import ops
    from tests import sample_restatement as R
    from tests import sample_trunc_rules as TR
    rows, V1 = X.shape
    keys = np.stack([np.arange(rows) * 7 + 3, np.arange(rows) % 5], 1).astype(np.int32)          # (r, s)
    out = ops.sample_trunc_rows(ctx, X, keys, t, SEED, temperature, top_k, top_p)
    for i in range(rows):
        ref = TR.row_reference(X[i], temperature, top_k, top_p)
        kept, tok = int(out["kept"][i]), int(out["tok"][i])
        if ref["kept"] < 0:
            assert kept == -1 and tok == 0 and np.isnan(out["theta"][i]) and np.isnan(out["lp"][i]) and np.isnan(out["lq"][i]), i
            continue
        if top_p < 1.0:
            stats["nucleus"] += 1
        if kept != ref["kept"]:
            lo, hi = ref["band"]
            assert top_p < 1.0 and lo <= kept <= hi, (i, kept, ref["kept"], ref["band"], temperature, top_k, top_p)
            stats["excused"] += 1
        cols = ref["order"][:kept]
        assert out["theta"][i] == X[i, cols[-1]], (i, out["theta"][i], X[i, cols[-1]], kept, temperature, top_k, top_p)
        pert = TR.scaled(X[i], temperature) + R.gumbel(R.noise_bits(SEED, keys[i, 1], keys[i, 0], t, np.arange(V1)))
        ks = np.sort(cols)
        best = int(ks[np.argmax(pert[ks])])
        assert 1 <= tok <= V1 and (tok - 1) in set(cols.tolist()), (i, tok, kept)
        if tok - 1 != best:
            gap = pert[best] - pert[tok - 1]
            stats["near"] += 1
            assert gap <= 2 * NOISE, (i, tok, best + 1, gap)
        lp, lq = TR.log_softmax_at(X[i], tok - 1), TR.log_q_at(X[i], temperature, cols, tok - 1)
        assert abs(out["lp"][i] - lp) <= STAGE * max(abs(lp), 1e-3), (i, out["lp"][i], lp)
        assert abs(out["lq"][i] - lq) <= STAGE * max(abs(lq), 1e-3), (i, out["lq"][i], lq, kept)
        stats["rows"] += 1


def _cases(V1):
    ks = [k for k in (1, 2, 255, 256, 257, V1 - 1, V1) if 1 <= k <= V1]
    ps = [1e-6, 0.5, 0.9, P_NEAR_ONE, 1.0]
    cases = [(1.0, k, 1.0) for k in ks]                                   # every top_k, the nucleus off
    cases += [(temp, 0, p) for temp in (0.1, 1.0, 2.0) for p in ps]       # every top_p at every temperature, top_k off
    cases += [(0.1, ks[min(2, len(ks) - 1)], 0.9), (2.0, ks[-2], 0.5), (2.0, 2, P_NEAR_ONE), (0.1, ks[-1], 1e-6)]   # both
    return cases


@pytest.mark.parametrize("V1", [33, 201, 10498])
def test_rows_against_the_definition(ctx, V1):
    X = _rows(V1, V1)
    stats = dict(rows=0, nucleus=0, excused=0, near=0)
    for n, (temp, k, p) in enumerate(_cases(V1)):
        _check(ctx, X, 1 + n % 15, temp, k, p, stats)
    print("V1 %d: %d row checks, %d nucleus rows of which %d excused (cumulative mass within 1e-9 Z of the cut), %d words at a "
          "near-tie" % (V1, stats["rows"], stats["nucleus"], stats["excused"], stats["near"]))
    assert stats["rows"] > 500 and stats["excused"] <= 0.01 * stats["nucleus"]


def test_a_row_above_64_kib(ctx):
    """V1 = 20,001: the 80 KB row needs the LDS opt-in of the launcher."""
    X = _rows(20001, 5)[[0, 1, 40, 44, 47, 52, 56, 58, 59, 63]]
    stats = dict(rows=0, nucleus=0, excused=0, near=0)
    for temp, k, p in ((1.0, 0, 1.0), (1.0, 256, 1.0), (0.5, 0, 0.9), (2.0, 20000, 0.5), (1.0, 20001, P_NEAR_ONE)):
        _check(ctx, X, 3, temp, k, p, stats)
    assert stats["rows"] >= 35 and stats["excused"] <= 0.01 * stats["nucleus"]


def test_rows_do_not_depend_on_the_launch(ctx):
    """A row's outputs are a function of the row, its keys and the options: a repeat, a subset and another order give the
    same bits (no floating-point sum of the kernel has an order that depends on the launch)."""
    from densecap_amd import ops
    X = _rows(201, 9)
    keys = np.stack([np.arange(64), np.arange(64) % 3], 1).astype(np.int32)
    a = ops.sample_trunc_rows(ctx, X, keys, 2, 11, 0.7, 40, 0.9)
    b = ops.sample_trunc_rows(ctx, X, keys, 2, 11, 0.7, 40, 0.9)
    sub = np.array([63, 5, 44, 0, 59])
    c = ops.sample_trunc_rows(ctx, X[sub], keys[sub], 2, 11, 0.7, 40, 0.9)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])
        np.testing.assert_array_equal(a[name][sub], c[name])
    d = ops.sample_trunc_rows(ctx, X, keys, 3, 11, 0.7, 40, 0.9)          # another step: other noise, the same cut
    np.testing.assert_array_equal(d["kept"], a["kept"])
    np.testing.assert_array_equal(d["theta"], a["theta"])
    assert (d["tok"] != a["tok"]).any()


def test_hook_refusals(ctx):
    from densecap_amd import ops
    lib = ctx.lib
    X = _rows(33, 1)
    keys = np.zeros((64, 2), np.int32)
    xd, kd = ctx.to_device(X), ctx.to_device(keys)
    tok, kept = ctx.empty((64,), np.int32), ctx.empty((64,), np.int32)
    theta, lp, lq = ctx.empty((64,), np.float32), ctx.empty((64,), np.float64), ctx.empty((64,), np.float64)
    tok_before = tok.numpy().copy()

    def call(V1=33, k=0, p=1.0, temp=1.0, logits=xd.ptr, lq_ptr=lq.ptr, rows=64):
        return lib.dc_debug_sample_trunc_rows(ctx.h, logits, rows, V1, V1, kd.ptr, 1, 0, temp, k, p, tok.ptr, kept.ptr, theta.ptr,
                                              lp.ptr, lq_ptr)
    for kw, code, msg in ((dict(k=34), -1, "top_k must be"), (dict(k=-1), -1, "top_k must be"), (dict(p=0.0), -1, "top_p must be"),
                          (dict(p=float("nan")), -1, "top_p must be"), (dict(p=1.5), -1, "top_p must be"),
                          (dict(temp=0.0), -1, "temperature must be"), (dict(logits=None), -1, "null pointer"),
                          (dict(lq_ptr=None), -1, "null pointer"), (dict(rows=0), -1, "rows"),
                          (dict(V1=70000), -5, "does not fit")):
        assert call(**kw) == code, (kw, lib.dc_last_error(ctx.h))
        assert msg in lib.dc_last_error(ctx.h).decode(), lib.dc_last_error(ctx.h)
    np.testing.assert_array_equal(tok.numpy(), tok_before)                 # nothing was launched
    assert call(k=5, p=0.9) == 0                                           # the ctx still works
    assert (kept.numpy()[:40] >= 1).all() and (kept.numpy()[:40] <= 5).all()
