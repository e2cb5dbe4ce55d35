"""The rules of the evaluation (dc_op_eval_match, densecap_amd.evaluate; docs/SEMANTICS.md, "Evaluation") restated on the CPU:
the reference's evaluator (eval/eval_utils.lua:136-312, box_utils.lua:565-612) in numpy float64 with literal loops, both claim
modes, and the literal 0.01-step loop of the recall thresholds.  Also the box and score sets the tests run on.

Boxes arrive as xcycwh float32; the conversion to corners is float32 (the arithmetic of dc_op_xcycwh_to_x1y1x2y2); everything
after it is float64 on those float32 values.  `fast=True` replaces the two innermost loops (IoU of one box against a list) by the
same operations on numpy float64 arrays -- element for element the same IEEE operations in the same order; the CPU tests
compare the two forms."""
import numpy as np

F, D = np.float32, np.float64
MIN_OVERLAPS = (0.3, 0.4, 0.5, 0.6, 0.7)
MIN_SCORES = (-1, 0, 0.05, 0.1, 0.15, 0.2, 0.25)
MAX_GT = 512                      # the documented limit of dc_op_eval_match
MAX_DET = 4096


def corners(xcycwh):
    """xcycwh float32 -> x1y1x2y2 float32: x1 = -((w-1)/2) + xc, x2 = (w-1)/2 + xc, every operation rounded to float32."""
    b = np.asarray(xcycwh, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        hw = (b[:, 2] - F(1)) / F(2)
        hh = (b[:, 3] - F(1)) / F(2)
        return np.stack([-hw + b[:, 0], -hh + b[:, 1], hw + b[:, 0], hh + b[:, 1]], 1).astype(F)


def to_xcycwh(x1y1x2y2):
    """Test helper: integer-valued corners -> the xcycwh whose float32 conversion gives those corners back exactly (odd or even
    extents up to 2^20 are exact in float32 halves)."""
    c = np.asarray(x1y1x2y2, D).reshape(-1, 4)
    w = c[:, 2] - c[:, 0] + 1; h = c[:, 3] - c[:, 1] + 1
    return np.stack([c[:, 0] + (w - 1) / 2, c[:, 1] + (h - 1) / 2, w, h], 1).astype(F)


def merge_threshold(thresh):
    """The C ABI carries the threshold as a float, the reference compares against the double 0.7: the threshold used is the double
    with the shortest decimal form that reads back as the float (0.7f -> 0.7)."""
    t = F(thresh)
    for p in range(1, 10):
        d = float("%.*g" % (p, float(t)))
        if F(d) == t:
            return d
    return float(t)


def _max(a, b):                   # Lua 5.1 math.max(a, b): starts from a, takes b when b > a (a NaN in a stays, in b is skipped)
    return b if b > a else a


def _min(a, b):
    return b if b < a else a


def iou(a, b):
    """One pair, a first (the detection, or the lower-indexed ground-truth box): float64, +1 on every extent."""
    a = [float(v) for v in a]; b = [float(v) for v in b]
    with np.errstate(all="ignore"):
        iw = D(_min(a[2], b[2])) - D(_max(a[0], b[0])) + D(1)
        ih = D(_min(a[3], b[3])) - D(_max(a[1], b[1])) + D(1)
        if iw > 0 and ih > 0:
            ua = (D(a[2]) - D(a[0]) + D(1)) * (D(a[3]) - D(a[1]) + D(1)) + (D(b[2]) - D(b[0]) + D(1)) * (D(b[3]) - D(b[1]) + D(1)) - iw * ih
            return float(iw * ih / ua)
    return 0.0


def iou_row(a, bs):
    """iou(a, b) for every row b of bs (float64 (n,4)), as one array expression."""
    a = np.asarray(a, D); bs = np.asarray(bs, D).reshape(-1, 4)
    with np.errstate(all="ignore"):
        x1 = np.where(bs[:, 0] > a[0], bs[:, 0], a[0]); y1 = np.where(bs[:, 1] > a[1], bs[:, 1], a[1])
        x2 = np.where(bs[:, 2] < a[2], bs[:, 2], a[2]); y2 = np.where(bs[:, 3] < a[3], bs[:, 3], a[3])
        iw = x2 - x1 + 1.0; ih = y2 - y1 + 1.0
        ua = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0) + (bs[:, 2] - bs[:, 0] + 1.0) * (bs[:, 3] - bs[:, 1] + 1.0) - iw * ih
        ov = iw * ih / ua
        return np.where((iw > 0) & (ih > 0), ov, 0.0)


def iou_matrix(boxes, fast=False):
    """box_utils.iou_matrix: diagonal 1, entry (i, j) = (j, i) = iou(box i, box j) for i < j."""
    b = np.asarray(boxes, D).reshape(-1, 4)
    n = len(b)
    Dm = np.zeros((n, n), D)
    for i in range(n):
        Dm[i, i] = 1.0
        if fast:
            Dm[i, i + 1:] = iou_row(b[i], b[i + 1:]); Dm[i + 1:, i] = Dm[i, i + 1:]
        else:
            for j in range(i + 1, n):
                Dm[i, j] = Dm[j, i] = iou(b[i], b[j])
    return Dm


def merge_boxes(corners32, thr, fast=False):
    """box_utils.merge_boxes: the list of groups (ascending member lists) in order of creation.  The column with the most alive
    entries >= thr wins a round, the lowest index among equals."""
    Dm = iou_matrix(corners32, fast)
    n = len(Dm)
    groups = []
    while True:
        with np.errstate(invalid="ignore"):
            good = Dm >= thr
        counts = good.sum(axis=0)                         # per column
        col = int(np.argmax(counts)) if n else -1         # the first of the largest
        if n == 0 or counts[col] == 0:
            break
        members = [int(j) for j in range(n) if good[j, col]]
        groups.append(members)
        Dm[members, :] = 0.0
        Dm[:, members] = 0.0
    return groups


def merged_box(corners32, members):
    """The mean of the members' float32 corners as TH takes it: a sequential float64 sum in member order, rounded to float32,
    divided by n in float32, widened to float64."""
    c = np.asarray(corners32, F).reshape(-1, 4)
    out = np.zeros((4,), D)
    with np.errstate(all="ignore"):
        for k in range(4):
            s = D(0)
            for j in members:
                s = s + D(c[j, k])
            out[k] = D(F(s) / F(len(members)))
    return out


def score_order(scores):
    """Decreasing score; ties (and -0 against +0) to the lower index; NaN last."""
    s = np.asarray(scores, D).reshape(-1)
    return sorted(range(len(s)), key=lambda i: (1, 0.0, i) if np.isnan(s[i]) else (0, -s[i], i))


def match_image(det_xcycwh, scores, gt_xcycwh, thresh=0.7, claim_last=True, fast=False):
    """DenseCaptioningEvaluator:addResult for one image -> what dc_op_eval_match writes for it."""
    det = corners(det_xcycwh); gt = corners(gt_xcycwh)
    B, M = len(det), len(gt)
    groups = merge_boxes(gt, merge_threshold(thresh), fast)
    G = len(groups)
    merged = np.zeros((G, 4), D)
    gt_group = np.full((M,), -1, np.int32)
    for g, members in enumerate(groups):
        merged[g] = merged_box(gt, members)
        gt_group[members] = g
    order = score_order(scores)
    used = [0] * G
    ov_out, grp_out, ok_out = np.zeros((B,), D), np.full((B,), -1, np.int32), np.zeros((B,), np.uint8)
    for d, ii in enumerate(order):
        bb = det[ii].astype(D)
        ovmax, jmax = 0.0, -1
        if fast and G:
            ovs = iou_row(bb, merged)
            ovs = np.where(np.isnan(ovs), 0.0, ovs)
            j = int(np.argmax(ovs))                       # the first of the largest: what a strict `>` from 0 keeps
            if ovs[j] > 0:
                ovmax, jmax = float(ovs[j]), j
        else:
            for j in range(G):
                ov = iou(bb, merged[j])
                if ov > ovmax:
                    ovmax, jmax = ov, j
        target = jmax
        if jmax == -1:
            target = G - 1 if (claim_last and G > 0) else -1     # used[-1]: the last group under from-the-end indexing
        ok = 0
        if target >= 0 and used[target] == 0:
            used[target] = 1
            ok = 1
        ov_out[d], grp_out[d], ok_out[d] = ovmax, jmax, ok
    return dict(order=np.asarray(order, np.int32).reshape(-1), ov=ov_out, group=grp_out, ok=ok_out, gt_group=gt_group, n_groups=G,
                merged=merged, groups=groups)


# ---- split level -------------------------------------------------------------------------------------------------------------
def recall_thresholds():
    """`for t=0,1,0.01`: the step is accumulated, a hundred additions of 0.01 overshoot 1, so the loop body runs 100 times."""
    out, t = [], 0.0
    while t <= 1:
        out.append(t)
        t = t + 0.01
    return out


def lua_number(x):
    return "%.14g" % x


def average_precision(tp, fp, npos, thresholds):
    n = len(tp)
    if n == 0:
        return 0.0
    tpc, fpc = np.cumsum(np.asarray(tp, D)), np.cumsum(np.asarray(fp, D))
    with np.errstate(all="ignore"):
        rec = tpc / D(npos)
        prec = tpc / (fpc + tpc)
    ap, apn = 0.0, 0
    for t in thresholds:
        p = 0.0
        for i in range(n):
            with np.errstate(invalid="ignore"):
                m = 1.0 if rec[i] >= t else 0.0
            v = prec[i] * m
            if v > p:
                p = v
        ap += p
        apn += 1
    return ap / apn


def evaluate(scores, ok, ov, npos, caption_scores=None, thresholds=None):
    """DenseCaptioningEvaluator:evaluate on the concatenated records (each image's already in its score order): a stable sort by
    decreasing score, then per (min_overlap, min_score) tp / fp, cumulative sums and the max-interpolated AP.  Without caption
    scores only the min_score == -1 rows exist (a METEOR score is never below 0, so `score > -1` holds for every record)."""
    thresholds = recall_thresholds() if thresholds is None else thresholds
    ix = score_order(scores)
    det, ap = {}, {}
    for mo in MIN_OVERLAPS:
        for ms in MIN_SCORES:
            if ms != -1 and caption_scores is None:
                continue
            tp, fp = [], []
            for ii in ix:
                cs = 0.0 if caption_scores is None else caption_scores[ii]
                hit = ov[ii] >= mo and ok[ii] == 1 and cs > ms
                tp.append(1.0 if hit else 0.0); fp.append(0.0 if hit else 1.0)
            a = average_precision(tp, fp, npos, thresholds)
            if ms == -1:
                det["ov" + lua_number(mo)] = a
            else:
                ap["ov" + lua_number(mo) + "_score" + lua_number(ms)] = a
    mean = lambda d: sum(d.values()) / len(d)
    if caption_scores is None:
        return dict(map=None, ap_breakdown=None, detmap=mean(det), det_breakdown=det)
    return dict(map=mean(ap), ap_breakdown=ap, detmap=mean(det), det_breakdown=det)


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def first_difference(got, ref):
    """None when two match results (dicts as match_image returns; `got` may lack `groups`) are equal bit for bit, else a message."""
    for k in ("n_groups",):
        if int(got[k]) != int(ref[k]):
            return "%s: got %d, expected %d" % (k, got[k], ref[k])
    for k in ("order", "group", "ok", "gt_group"):
        g, r = np.asarray(got[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)
        if g.shape != r.shape or not np.array_equal(g, r):
            i = next((i for i in range(min(len(g), len(r))) if g[i] != r[i]), min(len(g), len(r)))
            return "%s differs at %d: got %s, expected %s" % (k, i, g[i:i + 4], r[i:i + 4])
    for k in ("ov", "merged"):
        g, r = np.asarray(got[k], D), np.asarray(ref[k], D)
        if g.shape != r.shape or g.tobytes() != r.tobytes():
            if g.shape != r.shape:
                return "%s: shape %s, expected %s" % (k, g.shape, r.shape)
            i = int(np.flatnonzero(g.reshape(-1).view(np.uint64) != r.reshape(-1).view(np.uint64))[0])
            return "%s differs at %d: got %r, expected %r" % (k, i, g.reshape(-1)[i], r.reshape(-1)[i])
    return None


# ---- box and score sets --------------------------------------------------------------------------------------------------------
def clustered_gt(rng, M, per):
    """xcycwh ground truth in clusters of `per` near-duplicates with integer-valued corners: merges are frequent and chained
    (members a few pixels apart: some pairs on one side of 0.7, some on the other)."""
    ncl = (M + per - 1) // per
    x1 = rng.integers(0, 600, (ncl, 1)); y1 = rng.integers(0, 600, (ncl, 1))
    w = rng.integers(20, 60, (ncl, 1)); h = rng.integers(20, 60, (ncl, 1))
    j = rng.integers(-4, 5, (ncl, per, 4))
    c = np.stack([x1 + j[:, :, 0], y1 + j[:, :, 1], x1 + w + j[:, :, 2], y1 + h + j[:, :, 3]], 2).reshape(-1, 4)[:M]
    return to_xcycwh(c)


def on_threshold_gt(M):
    """Integer boxes whose IoU is exactly 70/100: a 10x10 box and the 10x7 box nested in it, pair after pair, 100 px apart."""
    c = []
    for k in range((M + 1) // 2):
        x = 100 * (k % 30); y = 100 * (k // 30)
        c.append([x, y, x + 9, y + 9]); c.append([x, y, x + 9, y + 6])
    return to_xcycwh(np.asarray(c[:M], D).reshape(-1, 4))


def detections_for(rng, gt_xcycwh, B, far=0.2):
    """B detections: jittered copies of random ground-truth boxes, and a share `far` of boxes that overlap nothing."""
    gt = np.asarray(gt_xcycwh, F).reshape(-1, 4)
    out = np.zeros((B, 4), F)
    for i in range(B):
        if len(gt) == 0 or rng.uniform() < far:
            out[i] = [5000 + 50 * (i % 64), 5000 + 50 * (i // 64), 20, 20]
        else:
            g = gt[rng.integers(0, len(gt))]
            out[i] = g + np.asarray([rng.integers(-3, 4), rng.integers(-3, 4), rng.integers(-4, 5), rng.integers(-4, 5)], F)
    return out


def special_scores(rng, B):
    """Rounded (tied) scores with +-inf, NaN and signed zeros mixed in."""
    s = np.round(rng.uniform(-1, 1, B), 2).astype(F)
    for val in (np.inf, -np.inf, np.nan, 0.0, -0.0):
        if B:
            s[rng.choice(B, max(1, B // 12), replace=False)] = val
    return s
