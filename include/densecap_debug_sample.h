/* densecap_debug_sample.h -- test hook of the truncated sampler's row kernel (sample_trunc.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use it to run the selection alone.  It lives in a header of its
 * own because the list of hooks in densecap_debug.h is pinned by tests/test_abi_and_host.py.
 */
#ifndef DENSECAP_DEBUG_SAMPLE_H
#define DENSECAP_DEBUG_SAMPLE_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The selection of dc_op_lm_sample_n_trunc alone, on the caller's logits and without weights: the production kernel through the
 * production launcher in its selection-only mode (no LSTM update).  Device pointers; synchronises before it returns.
 * logits (rows, ld) fp32, V1 <= ld columns of each row are scores; keys (rows, 2) int32: the (r, s) of every row's noise
 * counter; t >= 1 the step, seed and temperature (0.01..100) as in dc_sample_opts, top_k 0..V1, top_p in (0, 1].
 * Per row: tok_out = the word (1-based; 0 = no word), kept_out = the number of words kept (-1 = no word), theta_out = the raw
 * score of the last kept rank (kept, theta and the tie rule -- lower column first -- determine the kept set), lp_out =
 * LogSoftMax(x)[tok - 1], lq_out = the log-probability of tok under the truncated distribution at the temperature; NaN where
 * there is no word.  Refused with nothing launched: a null pointer, rows < 1, top_k / top_p / temperature out of range
 * (DC_E_INVALID); a V1 whose row does not fit a workgroup's LDS beside the kernel's workspace (DC_E_UNSUPPORTED). */
int dc_debug_sample_trunc_rows(dc_ctx* ctx, const float* logits, int rows, int V1, int ld, const int32_t* keys, int t,
                               uint64_t seed, float temperature, int top_k, float top_p, int32_t* tok_out, int32_t* kept_out,
                               float* theta_out, double* lp_out, double* lq_out);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_SAMPLE_H */
