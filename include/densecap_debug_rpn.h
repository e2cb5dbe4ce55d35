/* densecap_debug_rpn.h -- test hooks of the RPN backward's kernels (rpn_grad.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ and tools/ use them to run a kernel alone, through its
 * production launcher.  They live in a header of their own because the lists of hooks in the other debug headers are pinned by
 * tests.  Device pointers throughout; every hook synchronises before it returns.  No weights needed.
 */
#ifndef DENSECAP_DEBUG_RPN_H
#define DENSECAP_DEBUG_RPN_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight-gradient kernel of dc_op_conv3x3_grad with an explicit slice count: x (h, w, Cin), dy (h, w, Cout) -> dw (Cout,
 * Cin, 3, 3).  slices = 0: the production choice; 1..64: that many slices of ceil(h * w / slices) pixels, rounded up to 16 (a
 * slice past the last pixel adds zeros).  Cin % 32 == 0, h * w <= 65536. */
int dc_debug_conv3x3_wgrad(dc_ctx* ctx, const float* x, const float* dy, int h, int w_px, int Cin, int Cout, int slices, float* dw);
/* The gradient at the RPN's head outputs, alone (docs/SEMANTICS.md, "RPN gradients"): trans, anchors, boxes (A, 4) and scores
 * (A, 2) the training forward's rows, A = k * h * w; the sampler's lists and gt (G, 4); droi_or_null (num_pos + num_neg, 4) ->
 * dheads (h * w, 6k) in the layout of the heads.  num_pos + num_neg <= 1024; the lists are checked. */
int dc_debug_rpn_dheads(dc_ctx* ctx, const float* trans, const float* scores, const float* anchors, const float* boxes, int h, int w_px,
                        int k, const int32_t* pos_input_idx, const int32_t* pos_target_idx, int num_pos, const int32_t* neg_input_idx,
                        int num_neg, const float* gt, int G, const float* droi_or_null, float w_mid_obj, float w_mid_box, float decay,
                        float* dheads);
/* The heads' data gradient with the ReLU mask, alone: dhidden (P, R) = (hidden > 0) * (dheads (P, K6) . heads_w (K6, R)). */
int dc_debug_rpn_heads_bwd(dc_ctx* ctx, const float* dheads, const float* heads_w, const float* hidden, int P, int K6, int R,
                           float* dhidden);
/* What the last dc_op_rpn_grad or dc_forward_backward left: the RPN's share of the feature map's gradient (pixels, 512) to
 * feat_rpn (DEVICE, or NULL), and the library's own event split, HOST, four floats in ms: the head outputs' gradient, the heads,
 * the convolution's weight gradient, its data gradient. */
int dc_debug_rpn_grad_kept(dc_ctx* ctx, float* feat_rpn, int pixels, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_RPN_H */
