"""Scoring captions (dc_score_captions / dc_op_lm_score), the parts that need no GPU: query encoding, the ABI surface,
and the CPU restatement of the definition pinned against the oracle's greedy decode."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = {1: "a", 2: "red", 3: "car", 4: "cafe", 5: "<UNK>", 6: "12", 7: "half"}


def test_encode_captions_normalises_like_preprocess():
    from densecap_amd.model import encode_captions, words_preprocess
    assert words_preprocess(u"A  Red, CAR!") == ["a", "red", "car"]
    assert words_preprocess(u"café") == ["cafe"]
    assert words_preprocess(u"½ a car…") == ["half", "a", "car"]
    q = encode_captions(["A red car.", "car", "", u"café ½"], VOCAB, 4)
    assert q.dtype == np.int32 and q.shape == (4, 4)
    np.testing.assert_array_equal(q, [[1, 2, 3, 0], [3, 0, 0, 0], [0, 0, 0, 0], [4, 7, 0, 0]])


def test_encode_captions_unknown_words_and_errors():
    from densecap_amd.model import encode_captions
    np.testing.assert_array_equal(encode_captions(["a blue car"], VOCAB, 3), [[1, 5, 3]])
    no_unk = {k: v for k, v in VOCAB.items() if v != "<UNK>"}
    with pytest.raises(ValueError, match="'blue'"):
        encode_captions(["a blue car"], no_unk, 3)
    with pytest.raises(ValueError, match="at most 2"):
        encode_captions(["a red car"], VOCAB, 2)
    # id rows pass through, trailing zeros dropped, padded to the width
    np.testing.assert_array_equal(encode_captions([[3, 1, 0], [2]], VOCAB, 4), [[3, 1, 0, 0], [2, 0, 0, 0]])


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densecap.h")).read(), flags=re.S)


def test_new_symbols_in_header_exports_and_cdef():
    hdr = _header()
    lua = open(os.path.join(ROOT, "lua", "densecap_hip.lua")).read()
    from densecap_amd import _lib
    for name in ("dc_score_captions", "dc_op_lm_score"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r"int dc_score_captions\(dc_ctx\* ctx, const float\* img_chw, int H, int W, int img_on_device,\s+"
                     r"const int32_t\* queries, int Q, int Tq, dc_result\* out, float\* loglik\);", lua)
    assert "function Model:scoreCaptions" in open(os.path.join(ROOT, "lua", "DenseCapModelHIP.lua")).read()


def test_library_exports_the_scoring_entry_points():
    if not os.path.exists(os.path.join(ROOT, "densecap_amd", "lib", "libdensecap_hip.so")):
        import __graft_entry__ as g
        g.build()
    from densecap_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "dc_score_captions") and hasattr(lib, "dc_op_lm_score")


def test_restatement_matches_the_greedy_decode():
    """For the greedy caption of a row (cut at its first END, or its first T-1 words when it has none), loglik of that
    caption must be the sum of the per-step maxima of the log-softmax (plus log p(END) at the last step when the caption
    never produced END): this pins the START input, the target shift and the END term."""
    import torch
    from oracle import densecap_oracle as O
    from densecap_amd.weights import make_synthetic_weights
    from tests import score_restatement
    W = make_synthetic_weights(seed=7, vocab_size=300, seq_length=8)
    T, V = 8, 300
    codes = torch.randn(24, W["fc7_w"].shape[0], generator=torch.Generator().manual_seed(3)) * 2
    seq, logits = O.lm_sample(codes, W, T, return_logits=True)
    lps = [O._log_softmax_thnn(l.numpy()).astype(np.float64) for l in logits]
    queries = np.zeros((len(seq), T), np.int32)
    expected = np.zeros(len(seq))
    ended = 0
    for r in range(len(seq)):
        ends = np.nonzero(seq[r] == V + 1)[0]
        L = int(ends[0]) if len(ends) else T - 1
        ended += bool(len(ends))
        queries[r, :L] = seq[r, :L]
        expected[r] = sum(lps[t][r].max() for t in range(L)) + lps[L][r][V]
        if len(ends):
            assert lps[L][r][V] == lps[L][r].max()
    got = score_restatement.lm_score(codes.numpy(), W, queries)
    np.testing.assert_allclose(np.diag(got), expected, rtol=1e-6, atol=1e-5)
