/* densecap_debug_bwd.h -- test hooks of the backward kernels on the operand forms the backward passes use (lm_grad.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use them to run each kernel alone, through its production
 * launcher.  They live in a header of their own because the lists of hooks in densecap_debug.h and densecap_debug_grad.h are
 * pinned by tests.  Device pointers throughout; every hook synchronises before it returns.  No weights needed.
 */
#ifndef DENSECAP_DEBUG_BWD_H
#define DENSECAP_DEBUG_BWD_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight-gradient kernel with leading dimensions: C[n * ldc + k] = sum_m A[m * lda + n] * B[m * ldb + k] for n < N, k < K.
 * M, N, K >= 1, lda >= N, ldb >= K, ldc >= K.  Columns [N, lda) of A and [K, ldb) of B are not read, columns [K, ldc) of C are
 * not written.  (dc_op_lm_grad's lm_out_w gradient is the call with lda = V1pad > N = V + 1.) */
int dc_debug_wgrad_ld(dc_ctx* ctx, const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc);
/* The column sums behind every bias gradient: out[c] = sum_m X[m * ldx + c] for c < N.  M, N >= 1, ldx >= N. */
int dc_debug_colsum(dc_ctx* ctx, const float* X, int ldx, int M, int N, float* out);
/* The LSTM cell backward with every operand the launcher takes: gates_pre (rows, 4Hd) in gate order i,f,o,g; tok (rows) int32
 * with xg (xg_rows, 4Hd): a row with tok[r] in [1, xg_rows] has xg[tok[r] - 1] added to its pre-activation, tok[r] == 0 adds
 * nothing (both null: no row adds anything); c_prev (rows, Hd) or null (the cell started from c = 0); c (rows, Hd);
 * dh = dh_a + dh_b, either (rows, Hd) or null, not both null; dc_in (rows, Hd) or null (zero); dgates (rows, 4Hd) and dc_prev
 * (rows, Hd) out.  dc_prev may be the buffer passed as dc_in. */
int dc_debug_lstm_cell_bwd_ex(dc_ctx* ctx, const float* gates_pre, const int32_t* tok, const float* xg, int xg_rows,
                              const float* c_prev, const float* c, const float* dh_a, const float* dh_b, const float* dc_in,
                              int rows, int Hd, float* dgates, float* dc_prev);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_BWD_H */
