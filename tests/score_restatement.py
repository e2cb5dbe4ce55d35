"""The teacher-forced scoring definition (docs/SEMANTICS.md, "Scoring captions") restated on the CPU from the oracle's own
pieces: O.lstm_step for the LSTM (torch-rnn's step as the oracle computes it) and O._log_softmax_thnn for the scores; the
L+1 log-probabilities of a query are summed in float64.  Used by tests/test_score_captions_cpu.py and test_gpu_score.py."""
import numpy as np


def lm_score(codes, Wt, queries):
    """codes (n, D) float32, queries (Q, Tq) int 1-based ids, zero-padded -> loglik (n, Q) float64.
    Inputs [image vector, START, w_1 .. w_L], targets [w_1 .. w_L, END]; END = START = V+1."""
    import torch
    from oracle import densecap_oracle as O
    codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float32))
    n = codes.shape[0]
    Hd = Wt["lstm_w"].shape[1] // 4
    E = Wt["lstm_w"].shape[0] - Hd
    Wx, Wh = Wt["lstm_w"][:E], Wt["lstm_w"][E:]
    V1 = Wt["lm_out_w"].shape[0]
    enc = torch.relu(codes @ Wt["lm_enc_w"].t() + Wt["lm_enc_b"])
    h, c = O.lstm_step(Wt["lstm_b"] + enc @ Wx, torch.zeros(n, Hd), torch.zeros(n, Hd), Wh)    # image step
    h, c = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][V1 - 1][None] @ Wx, h, c, Wh)              # START (id V+1)
    q = np.asarray(queries)
    out = np.zeros((n, q.shape[0]), np.float64)
    for qi in range(q.shape[0]):
        words = [int(w) for w in q[qi] if w != 0]
        hq, cq = h, c
        for j, y in enumerate(words + [V1]):
            lp = O._log_softmax_thnn((hq @ Wt["lm_out_w"].t() + Wt["lm_out_b"]).numpy())
            out[:, qi] += lp[:, y - 1].astype(np.float64)
            if j < len(words):
                hq, cq = O.lstm_step(Wt["lstm_b"] + Wt["lm_emb"][y - 1][None] @ Wx, hq, cq, Wh)
    return out
