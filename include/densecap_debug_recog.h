/* densecap_debug_recog.h -- test hooks of the recognition net's backward kernels (recog_grad.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use them to run each kernel alone, through its production
 * launcher.  They live in a header of their own because the list of hooks in densecap_debug.h is pinned by
 * tests/test_abi_and_host.py.  Device pointers throughout unless a parameter says otherwise; every hook synchronises before it returns.
 */
#ifndef DENSECAP_DEBUG_RECOG_H
#define DENSECAP_DEBUG_RECOG_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tap list and the inverted index of dc_op_roi_pool_grad, alone: boxes (B, 4) on an h x w map.  With P = HH * WW and
 * T = B * P * 4, tap t = (row * P + point) * 4 + k (k = tl, tr, bl, br) lands on pixel tap_pix[t] = y * w + x, or -1 outside the
 * map, with weight tap_w[t]; the taps of pixel i are list[start[i] .. start[i + 1]) in ascending order.  tap_pix (T) int32,
 * tap_w (T) float, start (h * w + 1) int32, list (T) int32 (entries from start[h * w] on are not written). */
int dc_debug_roi_tap_index(dc_ctx* ctx, const float* boxes, int B, int h, int w, int img_h, int img_w, int HH, int WW,
                           int32_t* tap_pix, float* tap_w, int32_t* start, int32_t* list);
/* The two end criteria's gradients: obj (n), trans (n, 4), anchors (n, 4), target (num_pos, 4) -> dobj (n), dtrans (num_pos, 4),
 * danchor (num_pos, 4), masked (one int32: the rows whose target transform exceeds 10). */
int dc_debug_end_crit_grad(dc_ctx* ctx, const float* obj, const float* trans, const float* anchors, const float* target, int n,
                           int num_pos, float w_obj, float w_box, float* dobj, float* dtrans, float* danchor, int32_t* masked);
/* The recognition heads' backward: codes (n, D), w5 (5, D) rows obj then the four box-regression rows, dobj (n), dtrans
 * (num_pos, 4), g_or_null (num_pos, D) -> dcodes (n, D), dw5 (5, D), db5 (5). */
int dc_debug_heads_bwd(dc_ctx* ctx, const float* codes, const float* w5, const float* dobj, const float* dtrans,
                       const float* g_or_null, int n, int num_pos, int D, float* dcodes, float* dw5, float* db5);
/* in (N, HW * C) with k' = p * C + c -> out (N, C * HW) with k = c * HW + p.  C % 64 == 0, HW <= 64. */
int dc_debug_permute_fc6_back(dc_ctx* ctx, const float* in, float* out, int N, int C, int HW);
/* The library's own event split of the last dc_op_recog_grad or dc_loss_gradients, HOST, four floats in ms: the criteria, the
 * heads, fc7 and fc6 backward with their weight gradients; the gradient of the pooled features (the GEMM on the transposed fc6
 * weight); the RoI index and the scatter sum; the box gradient and the roi_boxes rows.  Returns 4, or DC_E_STATE before the
 * first call. */
int dc_debug_recog_grad_stage_ms(dc_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_RECOG_H */
