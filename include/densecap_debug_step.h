/* densecap_debug_step.h -- test hooks of the classic decode step: the vocabulary-projection GEMM with its fused row epilogues
 * (mfma_gemm.hip, v2_tile<.., AMAX, BF3, LSE>) and the one-workgroup-per-row tails that follow it (elementwise.hip:
 * lstm_step_tail_kernel, lse_step_tail_kernel, sample_step_tail_kernel).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ use them to run one launch alone on the caller's operands.  They
 * live in a header of their own because the list of hooks in densecap_debug.h is pinned by tests/test_abi_and_host.py.  All
 * pointers are device pointers unless said otherwise; neither hook needs loaded weights; both synchronise before they return, and
 * both go through the production path: the GEMM through the function every contraction of a decode goes through (so the ctx's
 * dc_debug_set "force_cfg", "v2_stages", "walk", "epi_wide" and dc_set_math_mode apply as they do in a decode), the tails through
 * their launchers.  The hooks only validate on the host and launch; a refused call has launched nothing.
 */
#ifndef DENSECAP_DEBUG_STEP_H
#define DENSECAP_DEBUG_STEP_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one GEMM of a decode step -------------------------------------------------------------------------------------------------
 * out = A (M, K) . W (N, K)^T, K % 32 == 0, bias (N floats, at least amax_n of them with a prefix) or null, plan_M as in a decode
 * (rows of one image when M covers a group, 0 = M).  The epilogue:
 *   DC_STEP_STORE    C[m * ldc + n] = act(product + bias) for every column (relu: 0 / 1); no prefix (amax_cols must be 0).
 *   DC_STEP_ARGMAX   per row and 32-column slot the first maximum among the real columns: part[m * part_ld + slot] = value,
 *                    part_idx[m * part_ld + slot] = column; a slot without an entry (an entry needs v > -inf) holds
 *                    (-inf, 0x7fffffff).  part_ld >= 2 * ceil(columns / 64).
 *   DC_STEP_LSE      part[m * part_ld + 2 * slot + {0, 1}] = (max v, sum exp(v - max)) over the slot's real columns, (-inf, 0) for
 *                    a slot without one; rowidx[m] = the row's 1-based target, whose biased logit goes to
 *                    part[m * part_ld + part_ld - 1].  part_ld >= 4 * ceil(columns / 64) + 1.
 *   DC_STEP_SAMPLE   part[m * part_ld + 5 * slot + 0..4] = the log-sum-exp pair, then the slot's best perturbed entry (score, column
 *                    as int bits, logit there); rowidx[2m], rowidx[2m + 1] = the row's (r, s) of the noise counter, t >= 1 the step,
 *                    seed the key, inv_temp = 1 / temperature in fp32 (0: no noise, no scaling).  part_ld >= 10 * ceil(columns / 64).
 * `columns` is amax_cols with a prefix and N without.  A prefix (amax_cols > 0, a multiple of 64, <= N): columns [0, amax_cols)
 * take the epilogue, [0, amax_n) of them are real; columns [amax_cols, N) are stored raw -- no bias, no activation -- to
 * C[m * ldc + n - amax_cols], ldc >= N - amax_cols.  m_dev_or_null: a device-side row count; rows from min(M, *m_dev) on are not
 * computed and nothing of theirs is written.
 *
 * The descriptor is filled as the decode fills it.  What the launchers refuse (amax_cols not a multiple of 64 or past N,
 * amax_n > amax_cols, a part_ld below the minimum of the log-sum-exp or the sampling epilogue, the sampling epilogue with a row
 * count) comes back as DC_E_HIP with nothing launched.  The hook itself refuses with DC_E_INVALID: a null operand or output of the
 * epilogue, M, N, K < 1, K % 32, plan_M outside [0, M], an unknown epilogue, ldc below the stored columns, a prefix on
 * DC_STEP_STORE, t < 1 for sampling, a negative amax_cols, amax_n or *m_dev, and -- the arg-max launcher does not check it -- an arg-max part_ld below
 * its minimum. */
enum { DC_STEP_STORE = 0, DC_STEP_ARGMAX = 1, DC_STEP_LSE = 2, DC_STEP_SAMPLE = 3 };
typedef struct dc_step_gemm {
  const float* A;
  const float* W;
  const float* bias;
  int32_t M, N, K, plan_M;
  int32_t epilogue;
  int32_t relu;
  float* C;
  int32_t ldc;
  int32_t part_ld;
  float* part;
  int32_t* part_idx;
  const int32_t* rowidx;
  int32_t t;
  float inv_temp;
  uint64_t seed;
  int32_t amax_cols, amax_n;
  const int32_t* m_dev_or_null;
} dc_step_gemm;
int dc_debug_step_gemm(dc_ctx* ctx, const dc_step_gemm* g);

/* ---- one launch of one row tail ------------------------------------------------------------------------------------------------
 * n rows, one workgroup each, on the caller's partials (layouts as above: nslots slots per row, ld floats apart) and state: c, h
 * (n, Hd) updated in place, gates_pre (n, 4 Hd) or null (no LSTM update), xg the table of xg_rows rows of 4 Hd input-gate terms a
 * word id selects (word w reads row w - 1).
 *   DC_STEP_TAIL_GREEDY  part / part_idx (ld >= nslots) or both null: then fixed_tok (0 = no row of xg) is the word.  seq[m * T + t] =
 *                        the word, 0 for a row whose slots are all sentinels; n_dev_or_null: rows from the count on are left alone;
 *                        zero_c: the update starts from c = 0.
 *   DC_STEP_TAIL_SCORE   part (ld >= 2 nslots + 1), tgt[m] the row's target: acc[m] += target logit - lse; a row whose target is
 *                        end_tok adds its term and keeps c, h.
 *   DC_STEP_TAIL_SAMPLE  part (ld >= 5 nslots): the word drawn is the best perturbed entry, a column >= end_tok is no entry;
 *                        acc, fin, seq as dc_op_lm_sample_n keeps them.
 * A tail turns a word into an address of xg.  The sampling tail bounds its column itself; the GREEDY TAIL DOES NOT: it trusts
 * the GEMM's epilogue, which only writes columns below amax_n or the sentinel.  So that no test can make a kernel read out of
 * bounds, the hook first copies to the host every value that would become an address -- the arg-max columns, the column bits of
 * the sampling partials, the targets, fixed_tok -- and refuses with DC_E_INVALID, before any launch, unless each column is
 * 0x7fffffff or in [0, xg_rows), each target in [1, xg_rows] or end_tok, fixed_tok in [0, xg_rows] and the sampling tail's end_tok in [1, xg_rows].
 * Also refused: null pointers the kind needs, n, Hd, T < 1, nslots < 0, ld below the layout, t outside [0, T). */
enum { DC_STEP_TAIL_GREEDY = 0, DC_STEP_TAIL_SCORE = 1, DC_STEP_TAIL_SAMPLE = 2 };
typedef struct dc_step_tail {
  int32_t kind;
  int32_t nslots, ld;
  int32_t xg_rows;
  const float* part;
  const int32_t* part_idx;
  const float* xg;
  const float* gates_pre;
  float* c;
  float* h;
  int32_t n, Hd;
  const int32_t* n_dev_or_null;
  int32_t zero_c, fixed_tok;
  const int32_t* tgt;
  int32_t end_tok;
  int32_t T, t;
  double* acc;
  uint8_t* fin;
  int32_t* seq;
} dc_step_tail;
int dc_debug_step_tail(dc_ctx* ctx, const dc_step_tail* a);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_STEP_H */
