"""The validation losses restated in numpy (docs/SEMANTICS.md, "Validation losses"): the box sampler with its counter-based draws,
InvertBoxTransform, the five criteria in float64 and getTarget.  tests/test_loss_rules_cpu.py ties it to the reference's own test
vectors; the GPU tests compare the library against it."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(batch_size=256, high_thresh=0.7, low_thresh=0.3, remove_outbounds=1, mid_box_reg_weight=0.05,
                mid_objectness_weight=0.1, end_box_reg_weight=0.1, end_objectness_weight=0.1, captioning_weight=1.0, seed=0)
FLAG_NO_NEGATIVES, FLAG_NEG_REPLACEMENT = 1, 2
LOSS_KEYS = ("mid_objectness_loss", "mid_box_reg_loss", "end_objectness_loss", "end_box_reg_loss", "captioning_loss", "total_loss")


# ---- Philox4x32-10 (the Random123 function), plain Python integers ---------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3, k0, k1 = (int(v) & MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_w0(c0, c1, c2, seed):
    """Word 0 of philox4x32_10(c0, c1, c2, 0, seed & 0xffffffff, seed >> 32) for an array of c0 (uint64 arithmetic)."""
    M0, M1, MASK, S = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF), np.uint64(32)
    a = np.asarray(c0).astype(np.uint64) & MASK
    b = np.full_like(a, int(c1) & 0xFFFFFFFF)
    c = np.full_like(a, int(c2) & 0xFFFFFFFF)
    d = np.zeros_like(a)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * a, M1 * c
        a, b, c, d = (p1 >> S) ^ b ^ np.uint64(k0), p1 & MASK, (p0 >> S) ^ d ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return a.astype(np.uint32)


def sample_key(i, cls, seed):
    """Candidate i of class cls (0 positive, 1 negative): philox4x32_10(i, 0, cls, 0, seed).w[0]."""
    return philox_w0(i, 0, cls, seed)


# ---- the sampler (BoxSampler.lua:64-167) -------------------------------------------------------------------------------------------
def corners(b):
    """box_utils.xcycwh_to_x1y1x2y2 in float32: x0 = ((w-1)/2)*-1 + xc, x1 = (w-1)/2 + xc."""
    b = np.asarray(b, F32)
    hw, hh = (b[:, 2] - F32(1)) / F32(2), (b[:, 3] - F32(1)) / F32(2)
    return np.stack([-hw + b[:, 0], -hh + b[:, 1], hw + b[:, 0], hh + b[:, 1]], 1).astype(F32)


def match(boxes, gt, convention="boxiou_module", tie="lower"):
    """(max_iou (A) float32 -- NaN where no number was seen --, arg (A), target_idx (G) with -1 = no number in the column).
    A NaN never wins; ties go to the lower index (tie="higher": the other way, for the tests that show the rule matters)."""
    from oracle import densecap_oracle as O
    with np.errstate(all="ignore"):
        iou = O.box_iou(np.asarray(boxes, F32), np.asarray(gt, F32), convention)
    nan = np.isnan(iou)
    m = np.where(nan, F32(-np.inf), iou)
    m = np.where(m == 0, F32(0), m)                                   # -0 == +0
    if tie == "lower":
        arg, tgt = m.argmax(1), m.argmax(0)
    else:
        arg, tgt = m.shape[1] - 1 - m[:, ::-1].argmax(1), m.shape[0] - 1 - m[::-1].argmax(0)
    max_iou = m[np.arange(len(m)), arg].astype(F32)
    none = nan.all(1)
    max_iou[none] = np.nan
    arg = np.where(none, 0, arg)
    tgt = np.where(nan.all(0), -1, tgt)
    return max_iou, arg.astype(np.int32), tgt.astype(np.int64)


def box_sampler(boxes, gt, batch_size=256, high_thresh=0.7, low_thresh=0.3, bounds=None, seed=0, forced_pos=None,
                forced_neg=None, convention="boxiou_module", tie="lower", scatter=True):
    """bounds: None or (x_min, y_min, x_max, y_max) -- the library's remove_outbounds is (1, 1, W, H).  forced_pos / forced_neg:
    0-based ranks in the class's ascending candidate list (the reference's debug_*_sample_idx, 1-based there)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    A = len(boxes)
    max_iou, arg, tgt = match(boxes, gt, convention, tie)
    with np.errstate(invalid="ignore"):
        pos, neg = max_iou > F32(high_thresh), max_iou < F32(low_thresh)
        if bounds is not None:
            c = corners(boxes)
            out = (c[:, 0] < F32(bounds[0])) | (c[:, 1] < F32(bounds[1])) | (c[:, 2] > F32(bounds[2])) | (c[:, 3] > F32(bounds[3]))
            pos, neg = pos & ~out, neg & ~out
    if scatter:
        t = tgt[tgt >= 0]
        pos[t] = True
        neg[t] = False
    flags = 0
    if not neg.any():
        neg = ~pos
        flags |= FLAG_NO_NEGATIVES
    pos_list, neg_list = np.nonzero(pos)[0], np.nonzero(neg)[0]
    total_pos, total_neg = len(pos_list), len(neg_list)
    num_pos = min(batch_size // 2, total_pos)
    num_neg = batch_size - num_pos if total_neg > 0 else 0
    replace = total_neg < num_neg
    if replace:
        flags |= FLAG_NEG_REPLACEMENT

    def draw(cands, num, cls, with_replacement):
        if num == 0:
            return np.zeros(0, np.int64)
        if with_replacement:
            r = (philox_w0(np.arange(num), 1, cls, seed).astype(np.uint64) * np.uint64(len(cands))) >> np.uint64(32)
            return cands[r.astype(np.int64)]
        comp = (sample_key(cands, cls, seed).astype(np.uint64) << np.uint64(32)) | cands.astype(np.uint64)
        return cands[np.argsort(comp, kind="stable")[:num]]
    pi = pos_list[np.asarray(forced_pos, np.int64)] if forced_pos is not None else draw(pos_list, num_pos, 0, False)
    ni = neg_list[np.asarray(forced_neg, np.int64)] if forced_neg is not None else draw(neg_list, num_neg, 1, replace)
    return dict(pos_input_idx=pi.astype(np.int32), pos_target_idx=arg[pi].astype(np.int32), neg_input_idx=ni.astype(np.int32),
                num_pos=len(pi), num_neg=len(ni), total_pos=total_pos, total_neg=total_neg, flags=flags,
                max_iou=max_iou, arg=arg, pos_mask=pos, neg_mask=neg, target_idx=tgt)


# ---- box transforms -------------------------------------------------------------------------------------------------------------
def invert_box_transform(anchors, targets):
    """InvertBoxTransform.lua:36-60 in float64 on the float32 inputs: ((xt-xa)/wa, (yt-ya)/ha, log(wt/wa), log(ht/ha))."""
    a, t = np.asarray(anchors, F32).astype(np.float64), np.asarray(targets, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([(t[:, 0] - a[:, 0]) / a[:, 2], (t[:, 1] - a[:, 1]) / a[:, 3], np.log(t[:, 2] / a[:, 2]),
                         np.log(t[:, 3] / a[:, 3])], 1)


def apply_box_transform(anchors, trans):
    """ApplyBoxTransform.lua:63-90 in float64."""
    a, t = np.asarray(anchors, np.float64), np.asarray(trans, np.float64)
    return np.stack([t[:, 0] * a[:, 2] + a[:, 0], t[:, 1] * a[:, 3] + a[:, 1], np.exp(t[:, 2]) * a[:, 2], np.exp(t[:, 3]) * a[:, 3]], 1)


# ---- the criteria, float64 over float32 inputs ----------------------------------------------------------------------------------------
def box_reg_rows(anchors, pred, targets, mask_rows=True):
    """Per-row SmoothL1 sums against InvertBoxTransform(anchors, targets) and the mask of the rows whose largest |target| exceeds
    10 (prediction and target zeroed: they add nothing).  mask_rows=False: no masking (shows the rule matters)."""
    t = invert_box_transform(anchors, targets)
    p = np.asarray(pred, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        mx = np.abs(t[:, 0])
        for d in range(1, 4):
            v = np.abs(t[:, d])
            mx = np.where(v > mx, v, mx)
        masked = (mx > 10.0) if mask_rows else np.zeros(len(t), bool)
        z = np.abs(p - t)
        rows = np.where(z < 1.0, 0.5 * z * z, z - 0.5).sum(1) if len(t) else np.zeros(0)
    return np.where(masked, 0.0, rows), masked


def nll2(scores, c):
    """-LogSoftMax(s)[c] of two-class rows, the formula of the kernel: log(exp(a - m) + exp(b - m)) + m - s_c."""
    s = np.asarray(scores, F32).astype(np.float64).reshape(-1, 2)
    m = np.where(s[:, 1] > s[:, 0], s[:, 1], s[:, 0])
    with np.errstate(all="ignore"):
        return np.log(np.exp(s[:, 0] - m) + np.exp(s[:, 1] - m)) + m - s[:, c]


def logistic_rows(x, num_pos):
    """LogisticCriterion.lua:85-92 per row: log(exp(a) + exp(a - x)) - a with a = min(0, x), plus x for the rows labelled 0."""
    x = np.asarray(x, F32).astype(np.float64).reshape(-1)
    a = np.where(x < 0, x, 0.0)
    with np.errstate(all="ignore"):
        v = np.log(np.exp(a) + np.exp(a - x)) - a
    v[num_pos:] = v[num_pos:] + x[num_pos:]
    return v


def losses(pos_scores, neg_scores, pos_anchors, pos_trans, pos_targets, obj, pos_roi_boxes, final_trans, rowlik, L, opts=None,
           mask_rows=True, masked_in_denominator=True):
    """The five terms and their total from the sampled rows' float32 arrays and the rows' caption log-likelihoods (float64).
    obj: all num_pos + num_neg recognition logits, positives first; final_trans: the positive rows'."""
    o = dict(DEFAULTS, **(opts or {}))
    np_, nn_ = len(pos_scores), len(neg_scores)
    w = {k: float(F32(o[k])) for k in o if k.endswith("weight")}
    mo = (nll2(pos_scores, 0).sum() / np_ if np_ else 0.0) + (nll2(neg_scores, 1).sum() / nn_ if nn_ else 0.0)
    mid_rows, mid_mask = box_reg_rows(pos_anchors, pos_trans, pos_targets, mask_rows)
    end_rows, end_mask = box_reg_rows(pos_roi_boxes, final_trans, pos_targets, mask_rows)
    den_mid = 4.0 * (np_ if masked_in_denominator else np_ - mid_mask.sum())
    den_end = 4.0 * (np_ if masked_in_denominator else np_ - end_mask.sum())
    n = np_ + nn_
    out = dict(mid_objectness_loss=w["mid_objectness_weight"] * mo,
               mid_box_reg_loss=w["mid_box_reg_weight"] * (mid_rows.sum() / den_mid) if np_ else 0.0,
               end_objectness_loss=w["end_objectness_weight"] * (logistic_rows(obj, np_).sum() / n) if n else 0.0,
               end_box_reg_loss=w["end_box_reg_weight"] * (end_rows.sum() / den_end) if np_ else 0.0,
               captioning_loss=w["captioning_weight"] * (-np.asarray(rowlik, np.float64).sum() / (np_ * (L + 2.0))) if np_ else 0.0)
    out["total_loss"] = (((out["mid_objectness_loss"] + out["mid_box_reg_loss"]) + out["end_objectness_loss"]) +
                         out["end_box_reg_loss"]) + out["captioning_loss"]
    out["masked_mid"], out["masked_end"] = int(mid_mask.sum()), int(end_mask.sum())
    return out


def get_target(gt_sequence, vocab_size):
    """LanguageModel:getTarget (LanguageModel.lua:148-164): (N, T) -> (N, T + 2), a null for the image step, the words, END
    (= V + 1) in the place of the first null."""
    g = np.asarray(gt_sequence, np.int64)
    t = np.zeros((g.shape[0], g.shape[1] + 2), np.int64)
    t[:, 1:-1] = g
    for i in range(len(t)):
        z = np.nonzero(t[i, 1:] == 0)[0]
        t[i, 1 + z[0]] = vocab_size + 1
    return t


# ---- fixtures of the GPU tests: inputs built by jittering copies of the ground truth ------------------------------------------------
def make_case(seed, A, G, img=(600, 720), hits=0.5, dup=True, zero_col=True):
    """boxes (A,4), gt (G,4) xcycwh float32 inside an img = (H, W) frame.  About `hits` of the inputs are jittered copies of
    ground-truth boxes (IoU from ~0.2 to 1), the rest are scattered; some leave the image.  dup: ground-truth box 1 repeats box 0
    and input 1 repeats input 0; zero_col: the last ground-truth box lies far outside, so its IoU column is all zero."""
    rng = np.random.default_rng(seed)
    H, W = img
    gt = np.stack([rng.uniform(40, W - 40, G), rng.uniform(40, H - 40, G), rng.uniform(20, 200, G), rng.uniform(20, 200, G)], 1)
    boxes = np.stack([rng.uniform(-20, W + 20, A), rng.uniform(-20, H + 20, A), rng.uniform(10, 300, A), rng.uniform(10, 300, A)], 1)
    n_hit = int(round(A * hits))
    if n_hit:
        src = rng.integers(0, G, n_hit)
        jit = rng.choice([0.0, 0.02, 0.1, 0.3], n_hit)[:, None]
        b = gt[src] * (1.0 + jit * rng.uniform(-1, 1, (n_hit, 4)))
        boxes[rng.permutation(A)[:n_hit]] = b
    if zero_col and G >= 3:
        gt[-1] = [5 * W, 5 * H, 30, 30]
    if dup and G >= 2:
        gt[1] = gt[0]
    if dup and A >= 2:
        boxes[1] = boxes[0]
    return boxes.astype(F32), gt.astype(F32)


def branch_cases():
    """name -> (boxes, gt, (H, W), opts): small cases that between them reach every branch of the sampler (asserted by
    tests/test_loss_rules_cpu.py, run on the GPU by tests/test_gpu_box_sampler.py)."""
    img = (600, 720)
    cases = {}
    b, g = make_case(1, 700, 9, img, hits=0.6)
    cases["many_positives"] = (b, g, img, dict(batch_size=64))                     # total_pos above batch / 2
    b, g = make_case(2, 700, 9, img, hits=0.0)
    cases["few_positives"] = (b, g, img, dict(batch_size=64))                      # total_pos below batch / 2
    b, g = make_case(3, 40, 5, img, hits=0.3)
    cases["neg_replacement"] = (b, g, img, dict(batch_size=256))                   # total_neg below num_neg
    b, g = make_case(4, 300, 7, img, hits=0.5)
    cases["no_negatives"] = (b, g, img, dict(batch_size=64, low_thresh=0.0, high_thresh=0.5))    # max < 0 never holds
    b, g = make_case(5, 1, 1, img, hits=1.0, dup=False, zero_col=False)
    cases["single_input"] = (b, g, img, dict(batch_size=2))                        # the one input is positive: no candidate negative
    return cases
