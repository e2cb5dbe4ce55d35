"""The screened greedy decode's selection rule on the CPU (no GPU): tests/decode_screen_rules.py on the benchmark's synthetic
weights, bf16 emulated by casting.  512 rows of random ReLU codes decoded greedily for 15 steps with the oracle's lstm_step.
Then the helpers of the kernel tests (tests/test_gpu_decode_screen_kernels.py): the bf16 rounding, the sharp score tolerance --
with the faults it catches and the bound check does not -- and the bracket of the candidate count."""
import math

import numpy as np
import pytest
import torch

from tests import decode_screen_rules as R

ROWS = 512


@pytest.fixture(scope="module")
def decoded():
    """Per step: (h, fp32 logits, scores, bounds) of the 512 rows -- computed once, read by every test."""
    from densecap_amd.weights import make_synthetic_weights
    from oracle import densecap_oracle as O
    torch.manual_seed(0)
    W = make_synthetic_weights(seed=1234)
    T, V1 = int(W["seq_length"]), W["lm_out_w"].shape[0]
    Hd = W["lstm_w"].shape[1] // 4
    E = W["lstm_w"].shape[0] - Hd
    Wx, Wh = W["lstm_w"][:E], W["lstm_w"][E:]
    codes = torch.relu(torch.randn(ROWS, W["lm_enc_w"].shape[1], generator=torch.Generator().manual_seed(5)))
    enc = torch.relu(codes @ W["lm_enc_w"].t() + W["lm_enc_b"])
    h, c = O.lstm_step(W["lstm_b"] + enc @ Wx, torch.zeros(ROWS, Hd), torch.zeros(ROWS, Hd), Wh)
    tok = torch.full((ROWS,), V1, dtype=torch.int64)
    wn, cc = R.row_norms_up(W["lm_out_w"]), R.bound_c(Hd)
    steps = []
    for _ in range(T):
        h, c = O.lstm_step(W["lstm_b"] + W["lm_emb"][tok - 1] @ Wx, h, c, Wh)
        z = h @ W["lm_out_w"].t() + W["lm_out_b"]
        s = R.scores_bf16(h, W["lm_out_w"], W["lm_out_b"])
        steps.append((h, z, s, R.bounds(s, R.h_norms_up(h), wn, cc)))
        tok = torch.argmax(z, 1) + 1
    return steps


def test_bound_holds_everywhere(decoded):
    worst = 0.0
    for h, z, s, b in decoded:
        ratio = ((s.double() - z.double()).abs() / b.double()).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0
    print("max |s - z| / b over %d rows x %d steps: %.4f" % (ROWS, len(decoded), worst))


def test_argmax_is_a_candidate_and_the_cap_holds(decoded):
    counts = []
    for h, z, s, b in decoded:
        mask, full = R.candidates(s, b)
        top = torch.argmax(z, 1)
        assert mask[torch.arange(ROWS), top].all()
        assert ((z == z.max(1).values[:, None]) <= mask).all()          # every column tied with the winner, too
        assert not full.any()
        assert (R.pick(z, mask, full) == top + 1).all()
        counts.append(mask.sum(1))
    counts = torch.cat(counts).float()
    print("candidates per row and step: mean %.2f, p99 %d, max %d" % (counts.mean(), np.percentile(counts.numpy(), 99), counts.max()))
    assert counts.max() <= R.MAX_CAND


def _select(h, w, bias):
    z = h @ w.t() + bias
    s = R.scores_bf16(h, w, bias)
    b = R.bounds(s, R.h_norms_up(h), R.row_norms_up(w), R.bound_c(h.shape[1]))
    mask, full = R.candidates(s, b)
    return z, mask, full, R.pick(z, mask, full)


def test_adversarial_rows():
    g = torch.Generator().manual_seed(3)
    Hd, V1 = 64, 300
    w = torch.randn(V1, Hd, generator=g) * 0.4
    bias = torch.randn(V1, generator=g) * 0.1
    h = torch.tanh(torch.randn(8, Hd, generator=g))
    # two identical rows of Wout that win: both are candidates, the lower index is the word
    z0 = h @ w.t() + bias
    top = int(torch.argmax(z0[0]))
    other = (top + 117) % V1
    w2, b2 = w.clone(), bias.clone()
    w2[other], b2[other] = w2[top], b2[top]
    z, mask, full, tok = _select(h, w2, b2)
    assert mask[0, top] and mask[0, other] and not full[0]
    assert int(tok[0]) == min(top, other) + 1
    assert (tok == torch.argmax(z, 1) + 1).all()
    # all-equal columns: every column is a candidate, the row is scanned exactly and takes column 0
    w3, b3 = w[:1].repeat(V1, 1), torch.full((V1,), 0.25)
    z, mask, full, tok = _select(h, w3, b3)
    assert mask.all() and full.all() and (tok == 1).all()
    # h = 0: the scores are fp16(bias), the winner is the largest bias
    z, mask, full, tok = _select(torch.zeros(2, Hd), w, bias)
    assert not full.any() and (tok == torch.argmax(bias) + 1).all()
    # a NaN in h: non-finite scores, exact scan, no entry -> no word; the other rows are untouched
    hn = h.clone(); hn[1, 5] = math.nan
    z, mask, full, tok = _select(hn, w, bias)
    assert full[1] and int(tok[1]) == 0 and not full[0] and int(tok[0]) == top + 1


# ---- the sharp tolerance of the kernel tests (tests/test_gpu_decode_screen_kernels.py) -----------------------------------------
def _f32(bits):
    return torch.from_numpy(np.asarray(bits, np.uint32).view(np.float32).copy())


def test_bf16_helper_agrees_with_torch():
    """R.bf16_rne_bits against torch.bfloat16: random values over every exponent, random bit patterns, and the special cases --
    ties (to the even pattern, in both directions, with the carry into the exponent and into inf), +-0, subnormals, inf, NaN.
    A NaN must stay a NaN (which one is not compared: torch's vector and scalar conversions do not agree on it)."""
    rng = np.random.default_rng(0)
    ties = [(hi << 16) | 0x8000 for hi in (0x3f80, 0x3f81, 0xbf80, 0xbf81, 0x3fff, 0x7f7f, 0xff7f, 0x0000, 0x0001, 0x007f, 0x8001)]
    near = [t + d for t in ties for d in (-1, 1)]
    special = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00008001, 0x007fffff, 0x00800000,
               0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f7fffff, 0xff7fffff]
    x = torch.cat([_f32(rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)),
                   torch.randn(100000, generator=torch.Generator().manual_seed(1)) * 2.0 ** torch.randint(-140, 120, (100000,)).float(),
                   _f32(ties + near + special)])
    got = R.bf16_rne_bits(x)
    want = x.bfloat16().view(torch.int16).numpy().view(np.uint16)
    nan = torch.isnan(x).numpy()
    assert nan.sum() > 100 and (~nan).sum() > 250000
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7fff) > 0x7f80).all() and ((want[nan] & 0x7fff) > 0x7f80).all()
    # the ties themselves, spelled out: 1.0 + half a unit stays 1.0 (even), the next pattern up goes up; the largest finite
    # float goes to inf; half the smallest bf16 subnormal goes to zero, one and a half of it to two
    t = R.bf16_rne_bits(_f32([0x3f808000, 0x3f818000, 0x7f7f8000, 0x00008000, 0x00018000, 0x80018000]))
    assert t.tolist() == [0x3f80, 0x3f82, 0x7f80, 0x0000, 0x0002, 0x8002]
    np.testing.assert_array_equal(R.bf16_values(x[~torch.isnan(x)]).float().numpy(), x[~torch.isnan(x)].bfloat16().float().numpy())


def test_emulated_scores_within_the_sharp_tolerance(decoded):
    """torch's fp32 sum of the exact products is one of the chains the model of R.score_tol covers."""
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    w, bias = W["lm_out_w"], W["lm_out_b"]
    worst, rel = 0.0, []
    for h, z, s, b in decoded[::4]:
        h = h[:128]
        ref, tol = R.scores_ref64(h, w, bias), R.score_tol(h, w, bias, h.shape[1])
        ratio = ((s[:128].double() - ref).abs() / tol).max().item()
        worst = max(worst, ratio)
        rel.append((tol / b[:128].double()).median().item())
        assert ratio <= 1.0
    print("emulated scores: worst err/tol %.3f; median tol / b %.4f" % (worst, float(np.median(rel))))
    assert float(np.median(rel)) < 1 / 30                  # what makes it sharp: far finer than the bound of the proof


def test_seeded_errors_exceed_the_sharp_tolerance(decoded):
    """Three faults a screen kernel could have, emulated on 128 rows of step 3: hb formed by truncation, one k left out, two k
    of h exchanged.  Each is over R.score_tol on most elements -- while the first still passes |s - z| <= b, the one property
    the route tests assert of the scores (it breaks the premise u = 2^-8 of the proof all the same)."""
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    w, bias = W["lm_out_w"], W["lm_out_b"]
    h, z, s, b = (x[:128] for x in decoded[3])
    ref, tol = R.scores_ref64(h, w, bias), R.score_tol(h, w, bias, h.shape[1])
    wb = w.bfloat16().float()

    def emulate(hb):
        return (hb @ wb.t() + bias).half()

    hb = h.bfloat16().float()
    trunc = _f32(h.numpy().view(np.uint32) & np.uint32(0xffff0000))
    drop = hb.clone(); drop[:, 77] = 0
    swap = hb.clone(); swap[:, [40, 41]] = swap[:, [41, 40]]
    over = {}
    for name, x in (("truncated", trunc), ("dropped k", drop), ("swapped k", swap)):
        e = (emulate(x).double() - ref).abs() / tol
        over[name] = ((e > 1).double().mean().item(), e.median().item())
    print("share of elements over the tolerance (median err/tol):", {k: "%.2f (%.1f)" % v for k, v in over.items()})
    assert ((emulate(hb).double() - ref).abs() <= tol).all()
    for name, (share, _) in over.items():
        assert share > 0.5, name
    st = emulate(trunc)
    bt = R.bounds(st, R.h_norms_up(h), R.row_norms_up(w), R.bound_c(h.shape[1]))
    ratio = ((st.double() - z.double()).abs() / bt.double()).max().item()
    print("truncated hb: max |s - z| / b = %.3f" % ratio)
    assert ratio <= 1.0                                    # the gap: the bound check does not see it


def test_candidate_bracket_is_almost_always_exact(decoded):
    """R.cand_bracket on 256 rows x 15 steps: lo <= the count at the host's own norm <= hi, and lo == hi on >= 95 % -- the
    share the device test may ask for as well."""
    from densecap_amd.weights import make_synthetic_weights
    W = make_synthetic_weights(seed=1234)
    wn = R.row_norms_up(W["lm_out_w"])
    exact = total = widest = 0
    for h, z, s, b in decoded:
        h, s, b = h[:256], s[:256], b[:256]
        lo, hi = R.cand_bracket(s, R.h_norms_up(h), wn, R.bound_c(h.shape[1]))
        mid = R.candidates(s, b)[0].sum(1)
        assert (lo <= mid).all() and (mid <= hi).all()
        exact += int((lo == hi).sum()); total += len(lo); widest = max(widest, int((hi - lo).max()))
    print("bracket exact on %.2f %% of %d (row, step)s, widest gap %d" % (100.0 * exact / total, total, widest))
    assert exact >= 0.95 * total
