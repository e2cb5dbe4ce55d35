"""The rules of the multi-order NMS (dc_op_nms_multi; docs/SEMANTICS.md, "Localising phrases") restated on the CPU, and the box
and score sets its tests run on.

Reference: for each score column, take the candidate rows (valid, score not NaN), run the oracle's box_utils.nms on them with
max_boxes = M and map the picks back to the rows of the full list.  A row that is no candidate is thereby never picked and never
suppresses -- it is not there."""
import numpy as np

from oracle import densecap_oracle as O


def nms_multi_ref(boxes, scores, thresh, max_picks, valid=None, nms=O.nms):
    """boxes (n,4) x1y1x2y2, scores (n,Q), valid (n) or None -> list of Q pick lists (0-based rows, best first)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    s = np.ascontiguousarray(scores, dtype=np.float32)
    if s.ndim == 1:
        s = s[:, None]
    n, Q = s.shape
    v = np.ones((n,), bool) if valid is None else np.asarray(valid).astype(bool)
    out = []
    for q in range(Q):
        cand = np.flatnonzero(v & ~np.isnan(s[:, q]))
        if len(cand) == 0:
            out.append([])
            continue
        p = nms(np.concatenate([b[cand], s[cand, q:q + 1]], 1), thresh, int(max_picks))
        out.append([int(cand[i]) for i in p])
    return out


def as_lists(picks, counts):
    """(Q,M) picks padded with -1 and (Q) counts, as the library returns them -> list of Q pick lists; the padding is checked."""
    picks, counts = np.asarray(picks), np.asarray(counts)
    out = []
    for q in range(len(counts)):
        c = int(counts[q])
        assert 0 <= c <= picks.shape[1], (q, c)
        assert (picks[q, c:] == -1).all(), "query %d: entries past the count must be -1: %s" % (q, picks[q, c:][:8])
        out.append([int(x) for x in picks[q, :c]])
    return out


def first_difference(got, ref):
    """None when the two lists of pick lists are equal, else a message naming the first query and position that differ."""
    if len(got) != len(ref):
        return "%d queries, expected %d" % (len(got), len(ref))
    for q, (g, r) in enumerate(zip(got, ref)):
        if g != r:
            k = next((i for i, (x, y) in enumerate(zip(g, r)) if x != y), min(len(g), len(r)))
            return "query %d: %d picks, expected %d; first difference at pick %d: got %s, expected %s" % (
                q, len(g), len(r), k, g[k:k + 4], r[k:k + 4])
    return None


# ---- box sets --------------------------------------------------------------------------------------------------------------
def clustered_boxes(rng, n, per):
    """near-duplicate clusters of `per` boxes: a pick suppresses rows far down any score order"""
    ncl = (n + per - 1) // per
    cxy = rng.uniform(0, 3000, (ncl, 1, 2)); wh = rng.uniform(30, 80, (ncl, 1, 2))
    xy = cxy + rng.uniform(-6, 6, (ncl, per, 2))
    b = np.concatenate([xy, xy + wh + rng.uniform(-6, 6, (ncl, per, 2))], 2).reshape(-1, 4)[:n]
    return b.astype(np.float32)


def identical_boxes(n):
    return np.tile(np.array([[10, 20, 50, 70]], np.float32), (n, 1))


def disjoint_boxes(n):
    """a grid of 20x20 boxes 40 apart: no pair overlaps"""
    i = np.arange(n)
    x = (i % 64) * 40.0; y = (i // 64) * 40.0
    return np.stack([x, y, x + 20, y + 20], 1).astype(np.float32)


def with_non_finite(rng, boxes, count=5):
    """a few rows with a NaN or infinite coordinate (a NaN area makes every IoU with the row NaN: it is suppressed by any pick)"""
    b = boxes.copy()
    rows = rng.choice(len(b), min(count, len(b)), replace=False)
    for k, r in enumerate(rows):
        b[r, k % 4] = (np.nan, np.inf, -np.inf)[k % 3]
    return b


# ---- score columns ---------------------------------------------------------------------------------------------------------
def score_columns(rng, n, Q):
    """(n,Q): independent uniform columns; column 1 (if any) rounded to 3 digits (ties); the last column constant (index order);
    with Q >= 4, column 2 a copy of column 0."""
    s = rng.uniform(0, 1, (n, Q)).astype(np.float32)
    if Q >= 2:
        s[:, 1] = np.round(s[:, 1], 3)
    if Q >= 3:
        s[:, Q - 1] = 0.25
    if Q >= 4:
        s[:, 2] = s[:, 0]
    return s
