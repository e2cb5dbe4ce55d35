/* densecap_debug_glue.h -- test hooks of the forward path's glue kernels, the ones between the trunk and the language model in
 * enqueue_forward: boxes_ingest_kernel, survivor_compact_kernel, gather_rows_kernel / gather_rows_i32_kernel, final_pack_kernel
 * (boxes.hip), bilinear_roi_pool_kernel in its group form (roipool.hip), recog_heads_kernel and iota_count_kernel
 * (elementwise.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use them to run one launch of one kernel alone on the caller's
 * device buffers, through the launcher the forward calls, with no arithmetic of their own.  They live in a header of their own
 * because the list of hooks in densecap_debug.h is pinned by tests/test_abi_and_host.py.  All pointers are device pointers; no hook
 * needs loaded weights; every hook synchronises before it returns.
 *
 * These kernels trust their callers: picks, gather indices and counts become addresses.  So that no test can make one read or write
 * out of bounds, a hook first copies the count and index arrays to the host and refuses with DC_E_INVALID, before any launch,
 * unless every value a kernel would use as a row index is inside the buffer it indexes (the rules are stated per hook).  The
 * ingest's in_n, the pooling's B_dev and a gather's count may be anything: those kernels clamp them to [0, P] (or [0, cap]).  The
 * compaction and the record kernel clamp their counts from above only -- min(count, P) goes into the row offsets of the later
 * images as it is, since the NMS that writes the counts never goes below 0 -- so a negative count is refused there.  Also refused
 * with DC_E_INVALID: a null pointer the call needs, a shape below 1, a stride below what it strides over.  What a launcher itself
 * refuses (C % 4, HH * WW > 256, a pick list without source boxes, D % 256 of the heads, D % 4 of the compaction) comes back as
 * DC_E_HIP.  A refused call has launched nothing.
 */
#ifndef DENSECAP_DEBUG_GLUE_H
#define DENSECAP_DEBUG_GLUE_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* boxes_ingest_kernel: in_boxes (nimg * P, 4) xcycwh, image i's list in rows [i * P, i * P + n_i), n_i = max(0, min(in_n[i], P));
 * clip != 0: box_utils.clip_boxes to {1, 1, img_w, img_h}, rows that come out invalid are dropped.  roi_boxes (nimg * P, 4): the rows
 * that stay, in order, zeros from the count on; box_src (nimg * P): the list row behind each, -1 from the count on;
 * count[i * count_stride]: their number.  count_stride >= 1. */
int dc_debug_boxes_ingest(dc_ctx* ctx, const float* in_boxes, const int32_t* in_n, int nimg, int P, int clip, int img_h, int img_w,
                          float* roi_boxes, int32_t* box_src, int32_t* count, int count_stride);

/* bilinear_roi_pool_kernel over a group (launch_bilinear_roi_pool_group, argument for argument): image i's map is feat_hwc +
 * i * feat_stride floats, (h, w, C) channels last; boxes (nimg * B, 4); out (nimg * B, C, HH, WW) for out_layout 0 or
 * (nimg * B, HH, WW, C) for 1.  B_dev (null: every row is live): image i's live count is min(B_dev[i * bdev_stride], B); rows from
 * it on are zero-filled.  pick (null: `boxes` is read): row b of image i is src_boxes[i * src_stride + 4 * pick[i * B + b]]
 * (src_stride in floats) and is also written to boxes, zeros from the live count on.
 * Refused here: nimg, B, h, w, C < 1, HH or WW < 2, img_h or img_w < 2, out_layout not 0 or 1, feat_stride < h * w * C or
 * src_stride < 4 * src_rows with more than one image, bdev_stride < 1 with B_dev, src_rows < 1 with pick, a pick of a live row
 * outside [0, src_rows). */
typedef struct dc_glue_roi_pool {
  const float* feat_hwc;
  size_t feat_stride;
  int32_t nimg, h, w, C;
  float* boxes;
  int32_t B;
  const int32_t* B_dev;
  int32_t bdev_stride;
  const int32_t* pick;
  const float* src_boxes;
  size_t src_stride;
  int32_t src_rows;
  int32_t img_h, img_w, HH, WW;
  float* out;
  int32_t out_layout;
} dc_glue_roi_pool;
int dc_debug_roi_pool_group(dc_ctx* ctx, const dc_glue_roi_pool* a);

/* recog_heads_kernel: codes (n, D), w5 (5, D) rows objectness then the four box-regression rows, b5 (5), roi (n, 4) -> obj (n),
 * trans (n, 4), fin (n, 4) = ApplyBoxTransform(roi, trans), fin_xyxy_or_null (n, 4) = its corners. */
int dc_debug_recog_heads(dc_ctx* ctx, const float* codes, const float* w5, const float* b5, const float* roi, float* obj,
                         float* trans, float* fin, float* fin_xyxy_or_null, int n, int D);

/* iota_count_kernel: idx[i] = i for i < cap, *count_out = *count_in. */
int dc_debug_iota_count(dc_ctx* ctx, int32_t* idx, int32_t* count_out, const int32_t* count_in, int cap);

/* gather_rows_kernel (is_i32 = 0: float rows) or gather_rows_i32_kernel (int32 rows): out (cap, width), row i = src row idx[i] for
 * i < *count, zeros from there on.  src has src_rows rows; refused unless idx[i] lies in [0, src_rows) for every i < min(*count, cap). */
int dc_debug_gather_rows(dc_ctx* ctx, const void* src, int src_rows, const int32_t* idx, const int32_t* count, int cap, int width,
                         void* out, int is_i32);

/* survivor_compact_kernel: codes (nimg * P, D), picks (nimg * P), count[i * count_stride] >= 0; K_i = min(count, P).  out: image
 * i's rows codes[i * P + picks[i * P + r]], r < K_i, at rows [off_i, off_i + K_i), off_i the sum of the
 * earlier K; *total = their sum; rows from *total on are not written.  Refused unless picks[i * P + r] lies in [0, P) for every
 * r < K_i. */
int dc_debug_survivor_compact(dc_ctx* ctx, const float* codes, const int32_t* picks, const int32_t* count, int count_stride,
                              int nimg, int P, int D, float* out, int32_t* total);

/* final_pack_kernel: image i's record at pack + i * stride bytes: int32 K_i at byte 0, the fault word (*fault, 0 when null) at
 * byte 68, and from byte 256 boxes (P, 4), scores (P), P rows of `words` 4-byte values -- int32 tokens (T) or, with codes, fc7
 * codes (D) -- and, with box_src, P int32: box_src[i * P + pick].  Only rows below K_i are written.  Exactly one of tokens and codes.
 * tok_gather (tokens only): 0 = token rows in final order, image i's at [i * P, i * P + K_i); 1 = token row of the pick;
 * 2 = final order, packed over the group as dc_debug_survivor_compact packs rows.  final_boxes (nimg * P, 4), obj (nimg * P),
 * tokens (nimg * P, T), codes (nimg * P, D), picks, box_src (nimg * P).
 * Refused: stride below 256 + 4 P (5 + words [+ 1 with box_src]) or no multiple of 4, tok_gather outside 0 .. 2, a count below 0,
 * a pick of a row below K_i outside [0, P). */
typedef struct dc_glue_final_pack {
  const float* final_boxes;
  const float* obj;
  const int32_t* tokens;
  int32_t tok_gather;
  const float* codes;
  const int32_t* picks;
  const int32_t* count;
  int32_t count_stride;
  const uint32_t* fault;
  int32_t nimg, P, T, D;
  void* pack;
  size_t stride;
  const int32_t* box_src;
} dc_glue_final_pack;
int dc_debug_final_pack(dc_ctx* ctx, const dc_glue_final_pack* a);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_GLUE_H */
