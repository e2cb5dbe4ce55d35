"""The single-order NMS (boxes.hip: launch_nms, nms_hist_kernel .. nms_scan_band_kernel) on crafted operands: the arithmetic that
decides which path a row takes, restated in numpy, and builders of cases that reach a named path by construction.

Restated: sort_key and its 16-bit bucket, the bucket table the in-bucket rank walks (start, count, the three loops of
nms_bucket_rank_kernel), the window ladder (win_start, graded and not).  Every builder returns (boxes5, expected picks, facts):
boxes5 (n, 5) x1 y1 x2 y2 score, the picks in closed form where the construction gives one (tests/test_nms_rules_cpu.py holds
every closed form against the oracle's nms and nms_py), and the facts the case is named for, computed from the restated
arithmetic.  Everything is integer-exact: every comparison is list equality.

Sorted POSITION p means the p-th row of the sorted list; builders lay boxes out by position, give position p a score that
decreases in p, and scatter positions to original rows through a permutation (perm[p] = the row of position p)."""
import collections

import numpy as np

from oracle import densecap_oracle as O

F32_FILL = 0x7fc5a5a5          # ops.GLUE_F32_FILL / GLUE_I32_FILL: what output buffers hold before a call
I32_FILL = 0x5a5a5a5a
CHUNK = 64                     # rows a scan step resolves (one mask word)
WIN0, WIN_MID, WIN_BIG = 4096, 8192, 32768
BUCKET_BITS = 16


# ---- the sort ---------------------------------------------------------------------------------------------------------------------
def sort_key(scores, valid=None):
    """sort_key of boxes.hip: ascending key = (valid first, NaN first, decreasing score); -0 and +0 share a key."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[s == 0] = 0                                                     # -0 == +0
    m = np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000))
    key = (~m).astype(np.uint32)
    key[np.isnan(s)] = 0
    if valid is not None:
        key[np.asarray(valid) == 0] = 0xffffffff
    return key


def bucket(key):
    return (np.asarray(key, np.uint32) >> np.uint32(32 - BUCKET_BITS)).astype(np.int64)


def live_rows(n, n_dev=None):
    """rows that take part under a device-side count: the first max(0, min(n_dev, n))"""
    return n if n_dev is None else max(0, min(int(n_dev), n))


def sorted_order(scores, valid=None, n_dev=None):
    """the workspace's `order`, nvalid entries: live valid rows by (key, index)"""
    s = np.asarray(scores, np.float32)
    nl = live_rows(len(s), n_dev)
    key = sort_key(s[:nl], None if valid is None else np.asarray(valid)[:nl])
    rows = np.arange(nl) if valid is None else np.flatnonzero(np.asarray(valid)[:nl] != 0)
    return rows[np.lexsort((rows, key[rows]))].tolist()


Bucket = collections.namedtuple("Bucket", "bucket lo cnt prologue wide rest")


def bucket_table(scores, valid=None, n_dev=None):
    """every occupied bucket of the histogram (invalid live rows included: they fill the last bucket): its start `lo` in the
    scattered list, its count, and the iterations of the three loops of nms_bucket_rank_kernel -- single keys up to the first
    16-byte aligned slot, four keys a load, single keys again."""
    s = np.asarray(scores, np.float32)
    nl = live_rows(len(s), n_dev)
    b = bucket(sort_key(s[:nl], None if valid is None else np.asarray(valid)[:nl]))
    ub, cnt = np.unique(b, return_counts=True)
    lo = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    out = []
    for bb, l, c in zip(ub.tolist(), lo.tolist(), cnt.tolist()):
        pro = min(c, (-l) % 4)
        out.append(Bucket(bb, l, c, pro, (c - pro) // 4, (c - pro) % 4))
    return out


# ---- the window ladder ------------------------------------------------------------------------------------------------------------
def win_start(k, graded=False):
    if k == 0:
        return 0
    if not graded:
        return WIN0 + (k - 1) * WIN_BIG
    return WIN0 if k == 1 else WIN0 + WIN_MID + (k - 2) * WIN_BIG


def is_graded(n, max_boxes):
    return max_boxes is not None and max_boxes > 1024 and n > WIN0 + WIN_MID


def windows(n, max_boxes=None):
    """[(r0, r1)] of the windows launch_nms walks over n sorted rows"""
    g, out, k = is_graded(n, max_boxes), [], 0
    while win_start(k, g) < n:
        out.append((win_start(k, g), min(n, win_start(k + 1, g))))
        k += 1
    return out


def window_of(pos, n, max_boxes=None):
    return next(k for k, (r0, r1) in enumerate(windows(n, max_boxes)) if r0 <= pos < r1)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def reference(boxes5, thresh, max_boxes=None, valid=None, n_dev=None, nms=O.nms):
    """the oracle's picks on the rows that take part (live and valid), as rows of the full list"""
    b = np.ascontiguousarray(boxes5, dtype=np.float32)
    nl = live_rows(len(b), n_dev)
    rows = np.arange(nl) if valid is None else np.flatnonzero(np.asarray(valid)[:nl] != 0)
    if len(rows) == 0 or (max_boxes is not None and max_boxes <= 0):
        return []
    return rows[nms(b[rows], thresh, max_boxes)].tolist()


def as_result(picks, order, n, cap, guard_rows=2):
    """what ops.nms_debug returns for these picks and this sorted order: sentinel-filled buffers with guard rows"""
    g = guard_rows
    r = dict(picks=np.full((cap + g,), I32_FILL, np.int32), count=np.full((1 + g,), I32_FILL, np.int32),
             order=np.full((n + g,), I32_FILL, np.int32), nvalid=np.full((1 + g,), I32_FILL, np.int32), rc=0)
    r["picks"][:len(picks)] = list(picks)[:cap + g]                  # (a list longer than the buffer shows in the count)
    r["count"][0] = len(picks)
    r["order"][:len(order)] = order
    r["nvalid"][0] = len(order)
    return r


def first_difference(res, expected, order, n, cap, guard_rows=2):
    """None when the buffers of ops.nms_debug hold exactly these picks and this sorted order -- count, picks below it, nvalid,
    order below it, and the sentinel everywhere a call must not write (picks from the count on, every guard row; `order` is a
    copy of n workspace entries, so only its guard rows are held to it) -- else a message naming the first thing that differs."""
    g = guard_rows
    if res["rc"] != 0:
        return "rc = %d" % res["rc"]
    if res["picks"].shape != (cap + g,) or res["order"].shape != (n + g,):
        return "buffer shapes %s %s" % (res["picks"].shape, res["order"].shape)
    nv, cnt = int(res["nvalid"][0]), int(res["count"][0])
    for name in ("count", "nvalid"):
        if (res[name][1:] != I32_FILL).any():
            return "%s: a guard entry was written: %s" % (name, res[name][1:])
    if (res["order"][n:] != I32_FILL).any():
        return "order: a guard entry was written"
    if nv != len(order):
        return "nvalid = %d, expected %d" % (nv, len(order))
    got = res["order"][:nv].tolist()
    if got != list(order):
        k = next(i for i, (x, y) in enumerate(zip(got, order)) if x != y)
        return "sort: order differs first at position %d: got %s, expected %s" % (k, got[k:k + 4], list(order)[k:k + 4])
    if cnt != len(expected):
        return "scan: count = %d, expected %d" % (cnt, len(expected))
    got = res["picks"][:cnt].tolist()
    if got != list(expected):
        k = next(i for i, (x, y) in enumerate(zip(got, expected)) if x != y)
        return "scan: picks differ first at pick %d: got %s, expected %s" % (k, got[k:k + 4], list(expected)[k:k + 4])
    if (res["picks"][cnt:] != I32_FILL).any():
        k = cnt + int(np.flatnonzero(res["picks"][cnt:] != I32_FILL)[0])
        return "picks[%d] past the count %d was written: %d" % (k, cnt, res["picks"][k])
    return None


# ---- wrong variants of the rule (what the comparison must catch) -------------------------------------------------------------------
VARIANTS = ("higher_index_first", "lt_at_threshold", "nan_last", "neg_zero_below_zero", "rows_past_count", "budget_off_by_one")


def nms_variant(boxes5, thresh, max_boxes=None, valid=None, n_dev=None, variant=None):
    """(picks, order) of a greedy NMS in plain numpy: the rule itself (variant None) or one of VARIANTS."""
    b = np.ascontiguousarray(boxes5, dtype=np.float32)
    n = len(b)
    nl = n if variant == "rows_past_count" else live_rows(n, n_dev)
    v = np.ones((n,), bool) if valid is None else np.asarray(valid) != 0
    rows = np.flatnonzero(v[:nl])
    s = b[rows, 4]
    isn = np.isnan(s)
    s64 = np.where(isn, 0.0, s.astype(np.float64))
    if variant == "neg_zero_below_zero":
        s64 = np.where((s == 0) & np.signbit(s), -1e-300, s64)
    tie = -rows if variant == "higher_index_first" else rows
    nan_rank = isn if variant == "nan_last" else ~isn
    order = rows[np.lexsort((tie, -s64, nan_rank))]
    budget = None if max_boxes is None else max_boxes + (1 if variant == "budget_off_by_one" else 0)
    thr = np.float32(thresh)
    x1, y1, x2, y2 = (b[order, k] for k in range(4))
    area = (x2 - x1 + np.float32(1)) * (y2 - y1 + np.float32(1))
    dead = np.zeros((len(order),), bool)
    picks = []
    with np.errstate(all="ignore"):
        for r in range(len(order)):
            if budget is not None and len(picks) >= budget:
                break
            if dead[r]:
                continue
            picks.append(int(order[r]))
            w = np.maximum(np.minimum(x2, x2[r]) - np.maximum(x1, x1[r]) + np.float32(1), np.float32(0))
            h = np.maximum(np.minimum(y2, y2[r]) - np.maximum(y1, y1[r]) + np.float32(1), np.float32(0))
            inter = w * h
            iou = inter / ((area + area[r]) - inter)
            keep = (iou < thr) if variant == "lt_at_threshold" else (iou <= thr)
            keep[:r + 1] = True
            dead |= ~keep
    return picks, order.tolist()


# ---- boxes by position ----------------------------------------------------------------------------------------------------------
def grid_boxes(n):
    """20 x 20 boxes 40 apart, 256 a row: no pair overlaps (coordinates exact in float32)"""
    i = np.arange(n)
    x = (i % 256) * 40.0
    y = (i // 256) * 40.0
    return np.stack([x, y, x + 20, y + 20], 1).astype(np.float32)


def stair_boxes(n, y0=0.0):
    """[2i, y0, 2i + 9, y0 + 9]: adjacent IoU 80 / 120 = 2/3, next but one 60 / 140 = 3/7, four apart and more 0"""
    i = np.arange(n, dtype=np.float64)
    return np.stack([2 * i, np.full(n, y0), 2 * i + 9, np.full(n, y0 + 9)], 1).astype(np.float32)


def position_scores(n):
    """strictly decreasing in the position, exact in float32, positive and finite negative: n / 2 - p + 0.25"""
    return (np.float32(n // 2) - np.arange(n, dtype=np.float32) + np.float32(0.25)).astype(np.float32)


def scatter(pos_boxes, pos_scores=None, perm_seed=None):
    """(boxes5, perm): position p's box and score at row perm[p] (perm_seed None: the identity)"""
    n = len(pos_boxes)
    s = position_scores(n) if pos_scores is None else np.asarray(pos_scores, np.float32)
    perm = np.arange(n) if perm_seed is None else np.random.default_rng(perm_seed).permutation(n)
    b5 = np.zeros((n, 5), np.float32)
    b5[perm, :4] = pos_boxes
    b5[perm, 4] = s
    return b5, perm


def disjoint(n, scores=None, perm_seed=None):
    """no pair overlaps: the picks are the sorted order itself (cut by a budget)"""
    b5, perm = scatter(grid_boxes(n), scores, perm_seed)
    return b5, perm.tolist(), dict(n=n)


def sort_case(scores, valid=None):
    """disjoint boxes in row order under the given scores: picks == sorted order, from the restated key"""
    s = np.asarray(scores, np.float32)
    b5 = np.concatenate([grid_boxes(len(s)), s[:, None]], 1).astype(np.float32)
    order = sorted_order(s, valid)
    return b5, order, dict(n=len(s), nvalid=len(order), buckets=bucket_table(s, valid))


def staircase(n, perm_seed=None, thresh=0.5):
    """Every box overlaps its neighbours by 2/3 and the next but one by 3/7: at 0.5 the even positions stay -- each one's fate hangs
    on the position before it, a dependency chain as long as the list (the band scan's triangular solve settles one row a sweep,
    the chunk scan walks one pick a step).  At thresh = float32(2/3) exactly nothing is suppressed (iou <= thresh keeps)."""
    b5, perm = scatter(stair_boxes(n), None, perm_seed)
    keeps_all = np.float32(thresh) >= np.float32(80.0) / np.float32(120.0)
    pos = list(range(n)) if keeps_all else list(range(0, n, 2))
    return b5, perm[pos].tolist(), dict(n=n, chain=n, picks_per_full_chunk=CHUNK if keeps_all else CHUNK // 2)


def twins(n, pairs, perm_seed=None, max_boxes=None):
    """Disjoint boxes, with position `later` of every (earlier, later) pair overwritten by a copy of position `earlier`'s box
    (IoU 1): the picks are every position but the later twins.  facts: per pair the distance in rows and in 64-row chunks and
    the window of each member; per chunk its number of picks; `far_chunks`: chunks all of whose picks have a twin four or more
    chunks on (what a helper wave of the band scan fetches for it)."""
    pairs = [(int(e), int(l)) for e, l in pairs]
    later = {l for _, l in pairs}
    assert all(0 <= e < l < n for e, l in pairs) and not later & {e for e, _ in pairs} and len(later) == len(pairs)
    pb = grid_boxes(n)
    for e, l in pairs:
        pb[l] = pb[e]
    b5, perm = scatter(pb, None, perm_seed)
    pos = [p for p in range(n) if p not in later]
    picks_in = collections.Counter(p // CHUNK for p in pos)
    far = collections.defaultdict(set)
    for e, l in pairs:
        if l // CHUNK - e // CHUNK >= 4:
            far[e // CHUNK].add(e)
    facts = dict(n=n, row_dist=[l - e for e, l in pairs], chunk_dist=[l // CHUNK - e // CHUNK for e, l in pairs],
                 windows=[(window_of(e, n, max_boxes), window_of(l, n, max_boxes)) for e, l in pairs],
                 chunk_picks={c: picks_in.get(c, 0) for c in range((n + CHUNK - 1) // CHUNK)},
                 far_chunks={c: len(v) for c, v in far.items() if len(v) == picks_in.get(c, 0)},
                 pick_index={e: i for i, e in enumerate(pos)})
    return b5, perm[pos].tolist(), facts


def far_twin_chunks(perm_seed=None):
    """768 rows: chunk 0 keeps 64 picks, chunk 1 33, chunk 2 17 (the three load depths of a helper wave), each pick with a twin
    five chunks on; the rest of chunks 1 and 2 are twins of chunk 0 (near words); chunk 5 -- the twins of chunk 0 -- has no pick
    at all and live chunks after it."""
    pairs = [(r, 5 * CHUNK + r) for r in range(64)]
    pairs += [(CHUNK + r, 6 * CHUNK + r) for r in range(33)] + [(r, CHUNK + r) for r in range(33, 64)]
    pairs += [(2 * CHUNK + r, 7 * CHUNK + r) for r in range(17)] + [(r, 2 * CHUNK + r) for r in range(17, 64)]
    return twins(12 * CHUNK, pairs, perm_seed)


def nan_box(n, at, perm_seed=None):
    """One box with a NaN corner at position `at`: its area is NaN, so !(iou <= thresh) holds against every box.  At position 0
    it is picked and suppresses all the rest; later, the first pick suppresses it and nothing else changes."""
    pb = grid_boxes(n)
    pb[at, 0] = np.nan
    b5, perm = scatter(pb, None, perm_seed)
    pos = [0] if at == 0 else [p for p in range(n) if p != at]
    return b5, perm[pos].tolist(), dict(n=n, at=at)


def degenerate_boxes(n, perm_seed=None):
    """Zero-extent boxes (x2 = x1 - 1: area 0), negative-extent boxes (area below 0) and copies of both among disjoint ones and
    inside them.  No closed form: the oracle's picks (0 / 0 and negative unions decide there as they do on the device)."""
    rng = np.random.default_rng(n)
    pb = grid_boxes(n)
    rows = rng.choice(n, n // 4, replace=False)
    for k, r in enumerate(rows):
        x, y = pb[r, 0], pb[r, 1]
        pb[r] = ((x + 5, y + 5, x + 4, y + 9), (x + 5, y + 5, x + 1, y + 9), (x + 5, y + 5, x + 4, y + 4), (x + 9, y + 9, x + 2, y + 2),
                 (x, y, x + 20, y - 1), (x + 3, y + 3, x + 3, y + 3))[k % 6]
    src = rng.choice(rows, n // 8, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), rows), n // 8, replace=False)
    pb[dst] = pb[src]                                                 # copies of degenerate boxes
    b5, perm = scatter(pb, None, perm_seed)
    return b5, reference(b5, 0.5), dict(n=n, zero_area=int((((pb[:, 2] - pb[:, 0] + 1) * (pb[:, 3] - pb[:, 1] + 1)) == 0).sum()),
                                        negative_area=int((((pb[:, 2] - pb[:, 0] + 1) * (pb[:, 3] - pb[:, 1] + 1)) < 0).sum()))


def layered(n, fresh, stairs=(), max_boxes=None, perm_seed=None, source=None):
    """The window cases.  Positions in `fresh` hold disjoint boxes of their own; every other position is a copy of a fresh
    position before it (source(p, earlier fresh positions) -> one of them; default: cycling through them, which pairs rows of
    later windows with picks of window 0).  stairs: (start, length) runs of fresh positions that hold a staircase instead, each
    on a row of its own far from the grid; its odd members go.  The picks are the fresh positions but those, cut by the budget.
    facts: the windows, picks before each border, and for every copy the windows of (source, copy)."""
    fresh = np.asarray(sorted(set(int(p) for p in fresh)))
    isf = np.zeros((n,), bool)
    isf[fresh] = True
    assert isf[0]
    pb = grid_boxes(n)
    gone = np.zeros((n,), bool)
    for k, (st, ln) in enumerate(stairs):
        assert isf[st:st + ln].all()
        sb = stair_boxes(ln, y0=20000.0 + 40.0 * k)
        pb[st:st + ln] = sb
        gone[st + 1:st + ln:2] = True
    src_of = {}
    nf = np.cumsum(isf)                                               # fresh positions up to and including p
    plain = fresh[~np.isin(fresh, [p for st, ln in stairs for p in range(st, st + ln)])]
    for p in np.flatnonzero(~isf):
        before = plain[:np.searchsorted(plain, p)]
        e = int(before[p % len(before)]) if source is None else int(source(int(p), before))
        src_of[int(p)] = e
        pb[p] = pb[e]
    b5, perm = scatter(pb, None, perm_seed)
    pos = [int(p) for p in fresh if not gone[p]]
    cut = pos if max_boxes is None else pos[:max_boxes]
    wins = windows(n, max_boxes)
    index = {e: i for i, e in enumerate(pos)}
    facts = dict(n=n, windows=wins, graded=is_graded(n, max_boxes),
                 picks_before={r0: int(np.searchsorted(pos, r0)) for r0, _ in wins},
                 pair_windows=sorted({(window_of(e, n, max_boxes), window_of(p, n, max_boxes)) for p, e in src_of.items()}),
                 cross_residues={w: sorted({index[e] % 16 for p, e in src_of.items() if window_of(p, n, max_boxes) == w
                                            and window_of(e, n, max_boxes) < w}) for w in range(1, len(wins))},
                 stairs_cross=[(st, st + ln) for st, ln in stairs])
    return b5, perm[cut].tolist(), facts


def window_case(n, max_boxes=None, perm_seed=None):
    """n rows laid over the ladder of (n, max_boxes): about one fresh position in eight (so that a budget of 2000 is not met before
    the last window), two copies in three paired with a fresh position of an EARLIER window, a 12-row staircase across every border
    whose sixth member is the window's first row (an odd member: the last pick of the window before suppresses it), and the last
    row of every window fresh."""
    wins = windows(n, max_boxes)
    fresh = set(range(0, n, 8))
    stairs = []
    for r0, r1 in wins:
        fresh |= {r0, r1 - 1}
        if r0 > 0:
            stairs.append((r0 - 5, min(n, r0 + 7) - (r0 - 5)))       # (cut short where the list ends inside it)
            fresh |= set(range(r0 - 5, min(n, r0 + 7)))

    def source(p, before):
        r0 = wins[window_of(p, n, max_boxes)][0]
        early = before[:np.searchsorted(before, r0)]                  # fresh positions of earlier windows
        pool = early if len(early) and p % 3 else before
        return pool[(p * 7) % len(pool)]
    return layered(n, fresh, stairs, max_boxes, perm_seed, source)


def many_picks_before_the_border(perm_seed=None):
    """37,000 rows, no budget: window 0 all fresh (4096 picks), window 1 one fresh row in 16, and the 136 rows of window 2 copies
    of picks whose pick indices cover every residue mod 16 -- nms_cross_kernel's 4 waves x 4 splits each find a suppressor."""
    n = WIN0 + WIN_BIG + 136
    fresh = set(range(WIN0)) | set(range(WIN0, WIN0 + WIN_BIG, 16)) | {WIN0 + WIN_BIG}

    def source(p, before):
        if p < WIN0 + WIN_BIG:
            return before[(p * 5) % len(before)]
        k = p - (WIN0 + WIN_BIG)                                      # 1 .. 135: pick indices 4000 + 3k straddle the border of window 0
        return before[4000 + 3 * k]
    return layered(n, fresh, (), None, perm_seed, source)


# ---- score sets of the sort cases -----------------------------------------------------------------------------------------------
def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


ALIGN_COUNTS = (1, 2, 3, 4, 5, 6, 7, 9, 1, 1, 13, 2, 8, 3, 64, 65, 1, 130, 11, 10)


def alignment_scores(seed=3):
    """Bucket j (decreasing score) holds ALIGN_COUNTS[j] rows whose keys differ in the low 16 bits only, a few of them equal (ties
    by index), rows shuffled: the bucket starts run through every lo % 4 and the counts through every mix of the rank kernel's
    three loops."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.uint32((0x3f80 - j) << 16) | rng.integers(0, max(2, c // 2 + 1), c).astype(np.uint32) * np.uint32(257)
                        for j, c in enumerate(ALIGN_COUNTS)])
    return _bits(rng.permutation(u))


def score_sets():
    """name -> (scores, valid or None) of the sort cases that are not plain sizes"""
    rng = np.random.default_rng(23)
    out = {}
    out["one_bucket_distinct_keys"] = (_bits(np.uint32(0x3f000000) | rng.permutation(65536)[:3000].astype(np.uint32)), None)
    out["alignment_table"] = (alignment_scores(), None)
    out["negative_logits"] = (np.round(-np.abs(rng.standard_normal(5000)) * 4 - 0.01, 2).astype(np.float32), None)
    out["mixed_signs"] = (np.round(rng.standard_normal(5000) * 3, 2).astype(np.float32), None)
    z = np.where(rng.uniform(0, 1, 700) < 0.5, 0.0, -0.0).astype(np.float32)
    z[rng.choice(700, 40, replace=False)] = 1.0
    z[rng.choice(700, 40, replace=False)] = -1.0
    out["signed_zeros"] = (z, None)
    d = np.concatenate([rng.integers(1, 1 << 23, 150), rng.integers(1, 9, 50)]).astype(np.uint32)      # denormal magnitudes
    d = np.concatenate([d, d | np.uint32(0x80000000), np.uint32([0, 0x80000000, 0x00800000, 0x80800000, 1, 0x80000001] * 5)])
    out["denormals"] = (_bits(rng.permutation(d)), None)
    f = np.round(rng.standard_normal(600), 1).astype(np.float32)
    f[rng.choice(600, 30, replace=False)] = np.inf
    f[rng.choice(600, 30, replace=False)] = -np.inf
    out["infinities"] = (f.copy(), None)
    f[rng.choice(600, 45, replace=False)] = np.nan
    f[::97] = _bits(np.uint32(0xffc00001))                            # a NaN with the sign bit set
    out["nan_first"] = (f, None)
    for nv in (0, 1, 63, 64, 65, 4095, 4096, 4097):
        n = 5000
        v = np.zeros((n,), np.uint8)
        v[rng.choice(n, nv, replace=False)] = 1
        out["valid_%d_of_%d" % (nv, n)] = (np.round(rng.standard_normal(n), 2).astype(np.float32), v)
    return out


def clustered_boxes5(rng, n, per, scores=None):
    """near-duplicate clusters of `per` boxes under random scores rounded to 3 digits (ties): picks suppress rows far down the
    order.  No closed form."""
    ncl = (n + per - 1) // per
    cxy = rng.uniform(0, 3000, (ncl, 1, 2))
    wh = rng.uniform(30, 80, (ncl, 1, 2))
    xy = cxy + rng.uniform(-6, 6, (ncl, per, 2))
    b = np.concatenate([xy, xy + wh + rng.uniform(-6, 6, (ncl, per, 2))], 2).reshape(-1, 4)[:n]
    s = np.round(rng.standard_normal(n) * 3, 3) if scores is None else scores
    return np.concatenate([b, np.asarray(s).reshape(n, 1)], 1).astype(np.float32)


def poison_tail(boxes5, valid, n_dev):
    """rows past the device count: NaN boxes, +inf scores, valid = 1 -- anything that takes part from there shows"""
    b = np.array(boxes5, np.float32)
    nl = live_rows(len(b), n_dev)
    b[nl:, :4] = np.nan
    b[nl:, 4] = np.inf
    v = None
    if valid is not None:
        v = np.array(valid, np.uint8)
        v[nl:] = 1
    return b, v


# ---- the case tables (tests/test_nms_rules_cpu.py and tests/test_gpu_nms_kernels.py walk the same ones) ---------------------------
Case = collections.namedtuple("Case", "boxes5 thresh max_boxes valid expected facts")
EQUAL_SIZES = (1, 63, 64, 65, 4097, 20520)       # (all-equal scores: the in-bucket rank is quadratic, 20,520 is the RPN list)
_SCORE_SETS = None


def sort_names():
    global _SCORE_SETS
    if _SCORE_SETS is None:
        _SCORE_SETS = score_sets()
    return ["equal_%d" % n for n in EQUAL_SIZES] + list(_SCORE_SETS)


def sort_build(name):
    if name.startswith("equal_"):
        s, v = np.full((int(name[6:]),), 0.25, np.float32), None
    else:
        sort_names()
        s, v = _SCORE_SETS[name]
    b5, order, facts = sort_case(s, v)
    return Case(b5, 0.5, None, v, order, facts)


_T23 = np.float32(80.0) / np.float32(120.0)      # the staircase's adjacent IoU as the device computes it: float32(2/3)
SCAN = {
    "staircase_64": lambda: staircase(64, 64),
    "staircase_65": lambda: staircase(65, 65),
    "staircase_130": lambda: staircase(130, 130),
    "staircase_4096": lambda: staircase(4096, 4096),
    "twins_rows_1_63_64": lambda: twins(700, [(10, 11), (64, 127), (200, 264)], 1),
    "twins_exactly_3_chunks": lambda: twins(1024, [(133, 329), (255, 384), (0, 254)], 2),
    "twins_exactly_4_chunks": lambda: twins(1024, [(133, 390), (63, 256), (0, 319)], 3),
    "twins_4_chunks_less_a_row": lambda: twins(1024, [(63, 318), (64, 319), (200, 455)], 4),
    "twins_first_to_last_chunk": lambda: twins(4096, [(3, 4095), (0, 4032), (63, 4090), (59 * 64 + 1, 4094)], 5),
    "far_twin_chunks_17_33_64": lambda: far_twin_chunks(6),
    "nan_box_first": lambda: nan_box(700, 0, 7),
    "nan_box_later": lambda: nan_box(700, 300, 8),
    "degenerate_boxes": lambda: degenerate_boxes(600, 9),
    "threshold_exact": lambda: staircase(130, 10, _T23) + (_T23,),
    "threshold_one_ulp_below": lambda: staircase(130, 11, np.nextafter(_T23, np.float32(0))) + (np.nextafter(_T23, np.float32(0)),),
}


def scan_build(name):
    r = SCAN[name]()
    return Case(r[0], r[3] if len(r) > 3 else 0.5, None, None, r[1], r[2])


WINDOWS = collections.OrderedDict(
    [("n%d_ungraded" % n, (n, None)) for n in (4095, 4096, 4097, 12288, 12289, 12290)] +
    [("n%d_budget_2000" % n, (n, 2000)) for n in (12288, 12289, 12290)] + [("many_picks_before_the_border", None)])


def window_build(name):
    if WINDOWS[name] is None:
        b5, exp, facts = many_picks_before_the_border(12)
        return Case(b5, 0.5, None, None, exp, facts)
    n, mb = WINDOWS[name]
    b5, exp, facts = window_case(n, mb, perm_seed=n)
    return Case(b5, 0.5, mb, None, exp, facts)


BUDGET_N = 12400
BUDGETS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 12288, BUDGET_N + 1)


def budget_build(kind, max_boxes):
    """disjoint: pick k is position k - 1, the budget is met on the last row of a chunk (64), of window 0 (4096) and of the
    graded ladder's middle window (12,288); staircase: 32 picks a chunk, so the same budgets cut inside a chunk's pick set."""
    b5, exp, facts = disjoint(BUDGET_N, None, 13) if kind == "disjoint" else staircase(BUDGET_N, 14)
    return Case(b5, 0.5, max_boxes, None, exp[:max_boxes], dict(facts, windows=windows(BUDGET_N, max_boxes), uncut=len(exp)))


DEV_N = 1000
DEV_COUNTS = (0, 1, 64, DEV_N - 1, DEV_N, DEV_N + 5, -3)


def device_count_build(n_dev, with_valid, max_boxes, seed=0, n=DEV_N):
    """clustered boxes, the rows past the count poisoned; expected: the oracle on the live (and valid) rows"""
    rng = np.random.default_rng(1000 + seed)
    b5 = clustered_boxes5(rng, n, 8)
    valid = (rng.uniform(0, 1, n) < 0.8).astype(np.uint8) if with_valid else None
    b5, valid = poison_tail(b5, valid, n_dev)
    return Case(b5, 0.3, max_boxes, valid, reference(b5, 0.3, max_boxes, valid, n_dev), dict(live=live_rows(n, n_dev)))
