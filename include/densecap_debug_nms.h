/* densecap_debug_nms.h -- test hooks of the two NMS launchers of boxes.hip: launch_nms (nms_hist_kernel ... nms_scan_band_kernel,
 * the single-order NMS the forward runs twice per image) and launch_nms_multi (the per-query NMS of dc_localize).
 *
 * Like densecap_debug_glue.h, NOT part of the drop-in boundary and in a header of its own because the list of hooks in
 * densecap_debug.h is pinned by tests/test_abi_and_host.py.  dc_op_nms and dc_op_nms_multi pass no device-side row count and bind
 * the workspace for exactly the rows they sort; the forward's final NMS passes n_dev = its count, no valid bytes and
 * max_boxes = -1 on a workspace bound for the 20,520 rows of the RPN NMS before it, and dc_localize passes the same count to the
 * multi-order NMS.  These hooks reach those forms: one production launcher per call, argument for argument, no arithmetic of
 * their own.  All pointers are device pointers; no hook needs loaded weights; every hook synchronises before it returns.
 * Refused with DC_E_INVALID, before any launch: a null pointer the call needs and what is listed per hook.
 */
#ifndef DENSECAP_DEBUG_NMS_H
#define DENSECAP_DEBUG_NMS_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* launch_nms: boxes (n, 4) x1y1x2y2, scores (n), valid_or_null (n) bytes, n_dev_or_null one int32: the rows that take part are
 * the first max(0, min(*n_dev, n)) (the kernels clamp it; it may hold anything).  thresh, max_boxes (-1: no budget) as dc_op_nms;
 * the scan is the ctx's "nms_band" setting (dc_debug_set), the fault word is checked as dc_op_nms checks it.
 * The workspace is bound for ws_rows >= n rows on a buffer the ctx keeps between calls and that only grows: a call after a larger
 * one with the same ws_rows finds that call's mask, near band and bucket pairs where its own will be.
 * picks: min(n, max_boxes) entries (n without a budget), written below *count only; count: one int32.
 * order_or_null (n): a copy of the workspace's sorted permutation, the first *nvalid entries meaningful (the rest is whatever
 * the buffer held); nvalid_or_null: one int32, the rows that are live, valid and therefore sorted.
 * Refused: n < 1, ws_rows < n, max_boxes < -1. */
int dc_debug_nms(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n,
                 const int32_t* n_dev_or_null, int ws_rows, float thresh, int max_boxes, int32_t* picks, int32_t* count,
                 int32_t* order_or_null, int32_t* nvalid_or_null);

/* launch_nms_multi: dc_op_nms_multi with n_dev_or_null (one int32; the live rows are the first max(0, min(*n_dev, n))), on that
 * call's scratch and with its checks: n in 1..4096 (above: DC_E_UNSUPPORTED), Q >= 1, max_picks in 1..4096.
 * picks (Q, max_picks), -1 from the count on; counts (Q). */
int dc_debug_nms_multi(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n,
                       const int32_t* n_dev_or_null, int Q, float thresh, int max_picks, int32_t* picks, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_NMS_H */
