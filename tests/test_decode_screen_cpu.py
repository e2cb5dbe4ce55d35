"""The screened greedy decode's selection rule on the CPU (no GPU): tests/decode_screen_rules.py on the benchmark's synthetic
weights, bf16 emulated by casting.  512 rows of random ReLU codes decoded greedily for 15 steps with the oracle's lstm_step."""
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
