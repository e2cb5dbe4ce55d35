"""The reference's DenseCaptioningEvaluator (eval/eval_utils.lua:136-312) on this path; rules in docs/SEMANTICS.md, "Evaluation".

`add_result` matches the detections of an image -- or of a whole group of images in one dc_op_eval_match call -- to the merged
ground truth on the device.  `records()` is the list eval/meteor_bridge.py reads as input.json.  `evaluate` is host float64: the
detection mAP (`detmap`, `det_breakdown`) needs no caption scorer; the caption mAP (`map`, `ap_breakdown`) needs the METEOR
scores of the records, one per record, as meteor_bridge.py writes them to output.json under `scores`.
"""
from __future__ import annotations

import json
import os

import numpy as np

MIN_OVERLAPS = (0.3, 0.4, 0.5, 0.6, 0.7)
MIN_SCORES = (-1, 0, 0.05, 0.1, 0.15, 0.2, 0.25)


def recall_thresholds():
    """`for t=0,1,0.01 do`: Lua accumulates the step, and a hundred additions of 0.01 give 1.0000000000000007 -- the body runs
    for 100 values of t, 0 .. ~0.99, not 101."""
    out, t = [], 0.0
    while t <= 1:
        out.append(t)
        t = t + 0.01
    return np.asarray(out, np.float64)


def _lua_number(x):
    return "%.14g" % x        # tostring(number) of Lua 5.1: the keys of ap_breakdown ("ov0.3_score0.05")


def _score_order(scores):
    """Stable, decreasing; NaN last."""
    s = np.asarray(scores, np.float64).reshape(-1)
    nan = np.isnan(s)
    return np.lexsort((np.where(nan, 0.0, -s), nan))


def evaluate_records(scores, ok, ov, npos, caption_scores=None):
    """DenseCaptioningEvaluator:evaluate on the state add_result collected: scores (each image's in its own score order,
    images concatenated), ok, ov per record, npos = merged ground-truth boxes over all images.  caption_scores: one number per
    record or None.  Returns {map, ap_breakdown, detmap, det_breakdown}; without caption scores map and ap_breakdown are None."""
    scores = np.asarray(scores, np.float64).reshape(-1)
    ok = np.asarray(ok).reshape(-1); ov = np.asarray(ov, np.float64).reshape(-1)
    n = len(scores)
    if len(ok) != n or len(ov) != n:
        raise ValueError("evaluate: %d scores, %d ok, %d ov" % (n, len(ok), len(ov)))
    if caption_scores is not None:
        caption_scores = np.asarray(caption_scores, np.float64).reshape(-1)
        if len(caption_scores) != n:
            raise ValueError("evaluate: %d caption scores for %d records" % (len(caption_scores), n))
    ix = _score_order(scores)
    ok_s, ov_s = ok[ix] == 1, ov[ix]
    cs_s = None if caption_scores is None else caption_scores[ix]
    thresholds = recall_thresholds()
    denom = np.arange(1, n + 1, dtype=np.float64)                 # fp + tp after the cumulative sums
    det, ap = {}, {}
    for mo in MIN_OVERLAPS:
        with np.errstate(invalid="ignore"):
            base = (ov_s >= mo) & ok_s
        for ms in MIN_SCORES:
            if ms != -1 and cs_s is None:
                continue
            with np.errstate(invalid="ignore"):
                hit = base if cs_s is None else base & (cs_s > ms)   # (a METEOR score is never below 0: `score > -1` always holds)
            a = 0.0
            if n:
                tpc = np.cumsum(hit.astype(np.float64))
                with np.errstate(all="ignore"):
                    rec, prec = tpc / np.float64(npos), tpc / denom
                rec = np.where(np.isnan(rec), -np.inf, rec)       # npos = 0: 0/0 passes no `rec >= t`
                # the largest precision among the records with rec >= t: rec never decreases, so they are a suffix
                smax = np.maximum.accumulate(prec[::-1])[::-1]
                first = np.searchsorted(rec, thresholds, side="left")
                p = np.where(first < n, smax[np.minimum(first, n - 1)], 0.0)
                a = float(np.cumsum(p)[-1] / len(thresholds))     # (cumsum: the loop's own left-to-right sum)
            if ms == -1:
                det["ov" + _lua_number(mo)] = a
            else:
                ap["ov" + _lua_number(mo) + "_score" + _lua_number(ms)] = a
    mean = lambda d: sum(d.values()) / len(d)
    if cs_s is None:
        return dict(map=None, ap_breakdown=None, detmap=mean(det), det_breakdown=det)
    return dict(map=mean(ap), ap_breakdown=ap, detmap=mean(det), det_breakdown=det)


class DenseCaptioningEvaluator:
    def __init__(self, ctx, claim_last=True, merge_thresh=0.7):
        """ctx: an ops.Context (a model's `ctx`).  claim_last: the reference's used[-1] rule (docs/SEMANTICS.md)."""
        self.ctx, self.claim_last, self.merge_thresh = ctx, bool(claim_last), merge_thresh
        self._records, self._scores = [], []
        self.n, self.npos = 1, 0

    def add_result(self, scores, boxes, captions, gt_boxes, gt_captions):
        """One image -- scores (B,) or (B,1), boxes (B,4) xcycwh, captions (B strings), gt_boxes (M,4) xcycwh, gt_captions
        (M strings) -- or a group of images: every argument a list with one such entry per image (one device call)."""
        from . import ops
        if not isinstance(scores, (list, tuple)):
            scores, boxes, captions, gt_boxes, gt_captions = [scores], [boxes], [captions], [gt_boxes], [gt_captions]
        n = len(scores)
        if not (len(boxes) == len(captions) == len(gt_boxes) == len(gt_captions) == n):
            raise ValueError("add_result: every argument needs one entry per image")
        scores = [np.asarray(s, np.float32).reshape(-1) for s in scores]
        boxes = [np.asarray(b, np.float32).reshape(-1, 4) for b in boxes]
        gt_boxes = [np.asarray(b, np.float32).reshape(-1, 4) for b in gt_boxes]
        for i in range(n):
            if not (len(scores[i]) == len(boxes[i]) == len(captions[i])):
                raise ValueError("add_result: image %d has %d scores, %d boxes, %d captions" % (
                    i, len(scores[i]), len(boxes[i]), len(captions[i])))
            if len(gt_boxes[i]) != len(gt_captions[i]):
                raise ValueError("add_result: image %d has %d ground-truth boxes, %d captions" % (
                    i, len(gt_boxes[i]), len(gt_captions[i])))
        if n == 0:
            return
        res = ops.eval_match(self.ctx, boxes, scores, gt_boxes, self.merge_thresh, self.claim_last)
        for i, r in enumerate(res):
            refs = [[] for _ in range(r["n_groups"])]
            for j, g in enumerate(r["gt_group"]):             # ascending member order
                refs[int(g)].append(gt_captions[i][j])
            for d in range(len(r["order"])):
                g = int(r["group"][d])
                self._records.append(dict(ok=int(r["ok"][d]), ov=float(r["ov"][d]), candidate=captions[i][int(r["order"][d])],
                                          references=list(refs[g]) if g >= 0 else [], imgid=self.n))
            self._scores.append(scores[i][r["order"]].astype(np.float64))
            self.n += 1
            self.npos += r["n_groups"]

    def num_added(self):
        return self.n - 1

    def records(self):
        return self._records

    def state(self):
        """The minimum evaluate needs: sorted scores, ok, ov, npos (what the CLI keeps in eval_state.json)."""
        s = np.concatenate(self._scores) if self._scores else np.zeros((0,), np.float64)
        return dict(scores=[float(v) for v in s], ok=[r["ok"] for r in self._records], ov=[r["ov"] for r in self._records],
                    npos=int(self.npos))

    def evaluate(self, caption_scores=None):
        st = self.state()
        return evaluate_records(st["scores"], st["ok"], st["ov"], st["npos"], caption_scores)


# ---- the file protocol of eval/meteor_bridge.py --------------------------------------------------------------------------------
def write_records(directory, evaluator, loss_results=None):
    """input.json (the records, what meteor_bridge.py reads) and eval_state.json (the state above) into `directory`.
    loss_results: the averaged validation losses of the run, kept in the state under that key so that the second phase reports
    them again; None: the state is what it was without them."""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "input.json"), "w") as f:
        json.dump(evaluator.records(), f)
    st = evaluator.state()
    if loss_results is not None:
        st["loss_results"] = loss_results
    with open(os.path.join(directory, "eval_state.json"), "w") as f:
        json.dump(st, f)                      # (Python's json writes and reads NaN / Infinity, which a score may be)


def dict_average(dicts):
    """utils.dict_average (densecap/utils.lua): the mean of every key over a list of dicts with the same keys."""
    if not dicts:
        return {}
    return {k: sum(float(d[k]) for d in dicts) / len(dicts) for k in dicts[0]}


def evaluate_from_files(directory, caption_scores_path=None):
    """The second phase, without a GPU: eval_state.json of `directory` and, if given, the output.json meteor_bridge.py wrote
    (key `scores`, one per record).  A score list of another length than the records is an error."""
    with open(os.path.join(directory, "eval_state.json")) as f:
        st = json.load(f)
    cs = None
    if caption_scores_path:
        with open(caption_scores_path) as f:
            cs = json.load(f)["scores"]
        if len(cs) != len(st["ok"]):
            raise ValueError("%s holds %d scores, %s has %d records" % (caption_scores_path, len(cs), directory, len(st["ok"])))
    res = evaluate_records([float(v) for v in st["scores"]], st["ok"], st["ov"], st["npos"], cs)
    if "loss_results" in st:
        res["loss_results"] = st["loss_results"]
    return res
