/* densecap_debug_grad.h -- test hooks of the language model's backward kernels (lm_grad.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use them to run each kernel alone, through its production
 * launcher.  They live in a header of their own because the list of hooks in densecap_debug.h is pinned by
 * tests/test_abi_and_host.py.  Device pointers throughout unless a parameter says otherwise; every hook synchronises before it returns.
 */
#ifndef DENSECAP_DEBUG_GRAD_H
#define DENSECAP_DEBUG_GRAD_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight-gradient kernel: C (N, K) = sum_m A[m][n] * B[m][k] for A (M, N) and B (M, K), all dense row-major, fp32 MFMA.
 * M, N, K >= 1.  No weights needed. */
int dc_debug_wgrad(dc_ctx* ctx, const float* A, const float* B, int M, int N, int K, float* C);
/* The embedding segment sum: demb (rows_out, E) is zeroed, then for every distinct token t of tok (HOST, count int32 in
 * [1, rows_out]) row t - 1 receives the sum of the dx rows (count, E) it was fed at, in ascending row order. */
int dc_debug_embed_segsum(dc_ctx* ctx, const float* dx, const int32_t* tok_host, int count, int E, int rows_out, float* demb);
/* The softmax cross-entropy gradient rows, in place: x (rows, ld) holds V1 <= ld logits per row, tgt (rows) the 1-based target
 * columns; x becomes (softmax - onehot) * scale, columns past V1 zero.  lse_out_or_null (rows) double. */
int dc_debug_softmax_grad(dc_ctx* ctx, float* x, int rows, int V1, int ld, const int32_t* tgt, float scale, double* lse_out_or_null);
/* The LSTM cell backward: gates_pre (rows, 4Hd) full pre-activations in gate order i,f,o,g; c_prev, c, dh, dc (rows, Hd);
 * dgates (rows, 4Hd) and dc_prev (rows, Hd) out. */
int dc_debug_lstm_cell_bwd(dc_ctx* ctx, const float* gates_pre, const float* c_prev, const float* c, const float* dh,
                           const float* dc, int rows, int Hd, float* dgates, float* dc_prev);
/* The library's own event split of the last dc_op_lm_grad, HOST, four floats in ms: the forward that keeps its state; the
 * recomputed projection, its softmax gradient and the loop back through the steps; the stacked weight, bias and input
 * gradients; the embedding gradient and the codes' rows.  Returns 4, or DC_E_STATE before the first call. */
int dc_debug_lm_grad_stage_ms(dc_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_GRAD_H */
