/* densecap_debug_beam.h -- test hooks of the standard beam search (dc_beam_captions / dc_op_lm_beam_n; beam.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/test_gpu_beam_std.py uses them to run the two row kernels of the
 * standard search alone, and its loop one step at a time.  They live in a header of their own because the list of hooks in
 * densecap_debug.h is pinned by tests/test_abi_and_host.py.  All pointers are device pointers; every hook synchronises before it
 * returns DC_OK or a negative code (dc_last_error has the text).  None of them reads dc_set_beam_size or the math mode.
 */
#ifndef DENSECAP_DEBUG_BEAM_H
#define DENSECAP_DEBUG_BEAM_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The merge of step t (0-based column t of the T-column rows) of the standard search: under a live parent b (fin_in == 0) the
 * candidates top_lp[b][j] + beam_lp_in[b], under a finished one the single candidate (b, 0) with beam_lp_in[b] itself; the best
 * `beam` of them (lower flat index b * beam + j first among equal sums; NaN is no candidate) -> beam_lp_out, beams_out (the
 * parent's row with column t = the word, 0 under a finished parent), len_out (the parent's, + 1 with a word), parent, cur_tok
 * (the word fed next; 1 where there is none), fin_out.  beam in [1, 32]; fin_in and fin_out may be the same buffer. */
int dc_debug_beam_std_merge(dc_ctx* ctx, const float* top_lp, const int32_t* top_idx, const float* beam_lp_in,
                            const int32_t* beams_in, const int32_t* len_in, const uint8_t* fin_in, int nprop, int beam, int T, int t,
                            int END, float* beam_lp_out, int32_t* beams_out, int32_t* len_out, int32_t* parent, int32_t* cur_tok,
                            uint8_t* fin_out);
/* The final ranking: beam_lp, len (nprop x beam), beams (nprop x beam x T) -> the n_best first hypotheses of every proposal by
 * beam_lp / pen[len], pen[l] = (float)pow(l, length_alpha) tabulated on the host (length_alpha == 0: no division, the order of
 * the input); captions (nprop x n_best x T), logprob (nprop x n_best): the unnormalised beam_lp.  length_alpha in [0, 2]. */
int dc_debug_beam_std_finish(dc_ctx* ctx, const float* beam_lp, const int32_t* beams, const int32_t* len, int nprop, int beam, int T,
                             int n_best, float length_alpha, int32_t* captions, float* logprob);
/* dc_beam_state (densecap_debug.h) plus len: the number of words every hypothesis holds. */
typedef struct dc_beam_std_state {
  float* h;
  float* c;
  float* beam_lp;
  int32_t* beams;
  int32_t* tok;
  int32_t* parent;
  uint8_t* fin;
  int32_t* len;
} dc_beam_std_state;
/* The standard search up to its loop for nprop rows of codes at beam width `beam`: image step, START step, first expansion ->
 * the state the iteration t = 1 reads and the top-k lists of the first step (top_lp, top_idx: nprop x beam).  Runs the code
 * dc_op_lm_beam_n runs, on lane 0's scratch.  nprop must fit one chunk (see "beam_chunk_floats"): the hook does not chunk. */
int dc_debug_beam_std_start(dc_ctx* ctx, const float* codes, int nprop, int beam, const dc_beam_std_state* state_out, float* top_lp,
                            int32_t* top_idx);
/* Iteration t (1 <= t < seq_length) of the loop from the caller's state -> the state the iteration t + 1 reads and the top-k
 * lists of the step (top_lp, top_idx: nprop x beam x beam; the lists of finished rows are zeros / 1..beam and the merge does
 * not read them).  state_in->parent is not read; state_in->tok must hold ids in [1, V+1]. */
int dc_debug_beam_std_step(dc_ctx* ctx, int nprop, int beam, int t, const dc_beam_std_state* state_in,
                           const dc_beam_std_state* state_out, float* top_lp, int32_t* top_idx);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_BEAM_H */
