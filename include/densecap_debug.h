/* densecap_debug.h -- measurement and test hooks of libdensecap_hip.so.
 *
 * NOT part of the drop-in boundary: nothing here replaces a reference interface and a maintainer of jcjohnson/densecap
 * binds none of it (the LuaJIT cdef in lua/densecap_hip.lua does not).  bench.py, tools/ and tests/ use these entry
 * points to time kernels, to read intermediate tensors for stage-wise parity, and to pin the contraction planner
 * without a GPU.  No setting changes a result except where a hook says it picks among deterministic fp32 summation
 * orders (tail_mode, force_cfg).
 */
#ifndef DENSECAP_DEBUG_H
#define DENSECAP_DEBUG_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Accumulated [contraction count, total ms, total algorithmic FLOPs] of the MFMA contraction kernel family
 * (HIP events around every contraction, including its split-K finish).  reset = 1 (re)starts the
 * measurement, reset = -1 stops it, 0 just reads.  Used by bench.py for the live roofline figure. */
int dc_mfma_profile(dc_ctx* ctx, int reset, int64_t* launches, double* total_ms, double* total_flops);
/* Copy an intermediate of the most recent forward to the host for stage-wise parity:
 * name in {"feat_hwc","rpn_heads","rpn_boxes","rpn_x1y1x2y2","rpn_p","rpn_valid",
 * "rpn_nms_idx","rpn_nms_count","roi_boxes","roi_feats","codes","obj","final_trans","final_boxes",
 * "final_x1y1x2y2" (the corners of "final_boxes" as the final NMS and dc_localize_captions read them),
 * "seq","final_nms_idx","final_nms_count"} (lane 0; "seq" is only filled in the reference caption order),
 * "box_src" (int32, P: after a forward on caller-supplied boxes, the caller's row behind every row of "roi_boxes", -1 past
 * "rpn_nms_count" -- the map before the final NMS),
 * "lm_enc","lm_h","lm_c" (image encoder output and final LSTM state, P rows: row = RoI in the reference caption order,
 * row = final rank with captions after the final NMS -- rows past "survivor_rows" (int32) are then undefined), or
 * "fault_word" (int32: the ctx's sticky device fault word, which the NMS band scan and stream-K report through and every
 * packed result carries -- 0 after a clean forward, -1 if it does not exist), or
 * "arena_allocs" (int32: how many times a lane workspace has been (re)allocated -- it only grows), or
 * "scratch" (3 x int64, no forward needed: the call-scoped device blocks alive now -- 0 between calls, whatever way the last
 * call ended; the bytes held by the context's seven grow-only buffers, those of dc_preprocess_u8, dc_forward_losses and the
 * gradient passes; how many times one of those buffers has been (re)allocated -- unchanged by a call whose shapes fit), or
 * "host_enqueue_us" (int32: host microseconds per image spent enqueueing in the last dc_forward_batch).
 * "decode_screen_cand" (int32, group x P x T: the screened greedy decode's candidate count of every (row, step) of lane 0's
 * last group -- -1 = a non-finite score or bound, above 64 = the row scanned every column exactly; rows the route did not
 * decode are undefined), "decode_screen_routes" (2 x int32: the parts of the last greedy decode that was enqueued -- 2 when
 * a single-image forward cuts its rows over two streams, else 1 -- and a mask, bit i set if part i took the screened step;
 * a replayed graph keeps the routes of its capture), or, after a dc_op_lm_sample under "lm_op_keep" (no forward needed), what that call left behind:
 * "lm_op_h", "lm_op_c" (final LSTM state, n x rnn_size), and on the screened route "lm_op_scores" (fp16, n x V1pad: the last
 * step's screen scores, V1pad = V + 1 rounded up to 64; columns past V are undefined), "lm_op_cand" (int32, n x T, as above),
 * "lm_op_best" (n: the last step's winning fp32 logit).
 * The noise of caption sampling as the device computes it (docs/SEMANTICS.md, "Sampling captions"; no forward needed):
 * "sample_gumbel@<first>" fills host_buf with capacity_bytes / 4 floats, g = -log(-log(u)) of the 23-bit indices first, first + 1,
 * ... (u = (index + 0.5) * 2^-23; at most 2^23 values a call); "sample_bits@<seed>" reads capacity_bytes / 16 rows of int32
 * (s, r, t, v) from host_buf and writes the uint32 noise bits of those coordinates under that seed to the front of host_buf.
 * Returns the number of elements copied (or <0). */
int64_t dc_debug_fetch(dc_ctx* ctx, const char* name, void* host_buf, int64_t capacity_bytes);
/* Test hooks (never needed for correct results; every setting gives the same outputs bit for bit):
 *   "beam_chunk_floats"  cap, in floats, of the beam search's full-logits buffer (default 2^28): proposals advance in
 *                        chunks of max(64, cap / (beam * (V+1))) -- lets a test walk the chunk loop with few rows;
 *   "sample_rows_cap"    rows (region x draw) one chunk of dc_sample_captions / dc_op_lm_sample_n may hold; 0 (default) =
 *                        about 512 MiB of scratch.  Chunks are whole draws; lets a test walk the chunk loop with few rows.
 *   "decode_route"       0 / 1 = the GEMM decode (default), 2 = the persistent LDS-resident decode (one launch for all
 *                        T+1 LSTM steps, [Wout; Wh^T] resident in LDS) wherever it applies: greedy decode of <= 64 rows,
 *                        rnn_size 512.  Tokens are bit-identical on both routes; measured no faster.
 *   "tail_mode"          single-image mode (dc_set_lanes(1)), layers whose 128x128 tile count is not a multiple of the CU
 *                        count: 0 = per layer, whichever of stream-K over the last round / K-split tail plan / whole tiles
 *                        was measured fastest for that shape class (default), 1 = never stream-K, 2 = whole tiles only.
 *                        The routes differ in the fp32 summation order of the affected rows (each one deterministic).
 *   "force_cfg"          measurement hook for tools/route_sweep.py: 0 = planned (default), 1 / 2 / 3 = plain launches use
 *                        128x128 / 128x64 / 64x64 tiles and no split-K, 4 = planned tiles, no split-K, 5 = 128x128 tiles on the 2x2-wave kernel
 *                        with a two-stage ring (two workgroups per CU), 6 = the K-split 128x128 kernel whatever K.  Changes the fp32
 *                        summation order with the kernel family; never set by the product path.
 *   "plan_mode"          -1 (default) = contraction planning follows dc_set_lanes (1 lane = single-image planning: stream-K /
 *                        tail plans over partial last rounds); 0 / 1 force multi-lane / single-image planning whatever the lane
 *                        count -- lets a one-stream profiler pass run exactly the kernels of the multi-lane schedule.
 *   "stagger"            0 (default) .. 4096: every workgroup of a contraction launch first sleeps a pseudo-random number (below
 *                        this value) of 64-cycle periods.  Measurement only (profiles/r04_kernel_lab.md).
 *   "epi_wide"           1 (default) / 0: interior tiles of the plain epilogues leave as 16-byte stores staged through the wave's
 *                        own 4 KB of LDS (8 full lines per instruction) / as dword stores.  Same values, same addresses.
 *   "walk"               0 (default) / 1: 128x64-tile launches run one workgroup per slot that walks its tiles (same XCD, same
 *                        tile order) instead of one workgroup per tile.  Bit-identical; measurement only (no gain measured).
 *   "v2_stages"          LDS ring depth of the 128x64-tile contraction kernel: 0 = by tile count (default: two stages, three
 *                        workgroups per CU, once a launch has >= 3 tiles per CU; three stages otherwise), 2 or 3 forced.
 *                        Same K order either way: bit-identical results.
 *   "decode_screen"      greedy decode step (fp32 math mode): 0 = the fused fp32 step (vocabulary projection with its row
 *                        arg-max in the epilogue), 1 = screen + re-score wherever the row tail's LDS fits: bf16 scores of every
 *                        column, then the exact fp32 logits of the few columns a proven error bound cannot rule out
 *                        (DESIGN.md 4.1c), -1 (default) = by the row count of the launch (measured crossover).  Tokens and
 *                        LSTM state are bit-identical on both routes (tests/test_gpu_decode_screen.py).
 *   "lm_op_keep"         1 / 0 (default): dc_op_lm_sample (greedy) copies its final state to the host before it frees its
 *                        scratch, for dc_debug_fetch "lm_op_*".  Not a setting of the forward.
 *   "nms_band"           1 (default) / 0, per context: NMS windows of <= 4096 sorted rows are scanned by nms_scan_band_kernel (the
 *                        near-diagonal words of the suppression mask resident in LDS) / every window by nms_scan_kernel (one
 *                        memory round trip per 64-row chunk).  Identical picks (tests/test_gpu_ops.py); A/B measurement only.
 * Returns DC_OK or DC_E_INVALID for an unknown name / bad value. */
int dc_debug_set(dc_ctx* ctx, const char* name, int64_t value);
/* Planning query -- pure (no context, no GPU: a missing device counts as 256 CUs; the environment variable DC_PLAN_CU_COUNT,
 * read by the planners, lets a test ask what a part with another CU count would be given): how the contraction engine carries out
 * C[M,N] = A[M,K] . W[N,K]^T (conv_cin != 0: the implicit GEMM of a 3x3 convolution with that many input channels,
 * K = 9*conv_cin; argmax != 0: the vocabulary projection with its fused row arg-max; plan_M = rows of ONE image when M
 * holds a group of images, 0 = M; serial_mode = the dc_set_lanes(1) scheduling).  out8 = {kind, route, stages, splitk,
 * m_split, sk_workgroups, sk_units, tail_splitk}: kind 0 plain launch, 1 split-K + reduce, 2 stream-K over the last
 * round, 3 K-split tail plan; route 0 K-split 128x128, 1 128x64 tiles, 2 128x128 tiles, 3 64x64 tiles; stages = LDS ring
 * depth of a 128x64 launch.  Exists so that the policy (and its invariance under image groups) is pinned by tests that
 * need no GPU.  Returns DC_OK or DC_E_INVALID. */
int dc_debug_plan_gemm(int64_t M, int64_t N, int64_t K, int64_t plan_M, int conv_cin, int argmax, int serial_mode,
                       int32_t* out8);

/* ---- beam search test hooks (tests/test_gpu_beam.py) ---------------------------------------------------------------------
 * The row kernels of LM:beamsearch one at a time, and the production loop one step at a time.  All pointers are device
 * pointers; every hook synchronises before it returns DC_OK or a negative code (dc_last_error has the text). */

/* LogSoftMax + top-k of `rows` rows of V1 logits, `ld` floats apart (finished_or_null[r] != 0: k zeros, indices 1..k) ->
 * top_lp, top_idx (rows x k; 1-based word ids, lower index first among equal values; a row of NaNs gives NaN / 0).
 * V1 beyond the kernel's LDS row on this device or k outside [1, V1]: refused, nothing is launched. */
int dc_debug_beam_topk(dc_ctx* ctx, const float* logits, int rows, int V1, int ld, const uint8_t* finished_or_null, int k,
                       float* top_lp, int32_t* top_idx);
/* The beam x beam merge of step t (0-based column t of the T-column beams): candidates top_lp (nprop x beam x beam) +
 * beam_lp_in (nprop x beam), the best `beam` of them (lower flat index first among equal sums) -> beam_lp_out, beams_out (the
 * parent's row with column t = the word), parent, cur_tok, finished (the row contains END).  beam in [1, 32]. */
int dc_debug_beam_merge(dc_ctx* ctx, const float* top_lp, const int32_t* top_idx, const float* beam_lp_in, const int32_t* beams_in,
                        int nprop, int beam, int T, int t, int END, float* beam_lp_out, int32_t* beams_out, int32_t* parent,
                        int32_t* cur_tok, uint8_t* finished);
/* The state of nprop proposals between two steps of the search, nprop x beam rows at the ctx's beam size (dc_set_beam_size):
 * LSTM state h, c (rnn_size floats a row), beam_lp, beams (seq_length ids a row), tok (the word every row feeds to the next
 * step), parent (the beam of the previous step a row continues) and fin (the row contains END or has no word). */
typedef struct dc_beam_state {
  float* h;
  float* c;
  float* beam_lp;
  int32_t* beams;
  int32_t* tok;
  int32_t* parent;
  uint8_t* fin;
} dc_beam_state;
/* The search up to its loop for nprop rows of codes: image step, START step, first expansion -> the state the iteration t = 1
 * reads, and the top-k lists of the first step (top_lp, top_idx: nprop x beam).  Runs the code dc_op_lm_sample runs at that beam
 * size, on lane 0's scratch.  nprop must fit one chunk (see "beam_chunk_floats"): the hook does not chunk. */
int dc_debug_beam_start(dc_ctx* ctx, const float* codes, int nprop, const dc_beam_state* state_out, float* top_lp,
                        int32_t* top_idx);
/* Iteration t (1 <= t < seq_length) of the loop from the caller's state: LSTM step on tok, vocabulary projection, LogSoftMax +
 * top-k under the finished mask, merge, states by parent -> the state the iteration t + 1 reads and the top-k lists the merge
 * consumed (top_lp, top_idx: nprop x beam x beam).  state_in->parent is not read; state_in->tok must hold ids in [1, V+1]. */
int dc_debug_beam_step(dc_ctx* ctx, int nprop, int t, const dc_beam_state* state_in, const dc_beam_state* state_out,
                       float* top_lp, int32_t* top_idx);

/* ---- screened greedy decode test hooks (tests/test_gpu_decode_screen_kernels.py) -----------------------------
 * The three kernels of the screened step one at a time, through the launchers the decode itself calls, on the loaded weights
 * (Wout in bf16, its row norms, bias, the bound's constant, the xg table).  All pointers are device pointers; both hooks
 * synchronise before they return.  DC_E_STATE without weights, DC_E_UNSUPPORTED where the route does not exist for the loaded
 * dimensions (the row tail's LDS does not fit: the decode then never takes it); nothing is launched in either case.
 * n_dev_or_null: a device-side row count, as the packed survivor decode passes one; rows from min(n, *n_dev) on are not
 * computed and every output row of theirs keeps what the caller put there.  Kp = rnn_size rounded up to 64, V1pad = V + 1
 * rounded up to 64. */

/* h (n x rnn_size fp32) -> what the operand kernel writes: hb_out (n x Kp bf16 bit patterns, zero from rnn_size on), hnorm_out
 * (n floats, >= |h|_2) -- and what the screen kernel then writes from them: scores_out (n x V1pad fp16; columns past V are
 * not written). */
int dc_debug_screen_scores(dc_ctx* ctx, const float* h, int n, const int32_t* n_dev_or_null, uint16_t* hb_out, float* hnorm_out,
                           void* scores_out);
/* One launch of the row tail on the caller's scores (n x V1pad fp16), state h (n x rnn_size) and norms hnorm (n) ->
 * tok_out (n: 1-based word, 0 = no word), cand_out (n: the candidate count, -1 = a non-finite score or bound), best_out (n:
 * the winner's fp32 logit).  gates_pre_or_null == null is the last step: selection only, c and the four outputs below are
 * not used and may be null.  Otherwise gates_pre (n x 4 rnn_size: h.Wh, to which the tail adds the word's xg row) and c
 * (n x rnn_size) give the LSTM update: h_out, c_out (n x rnn_size) and the operands of the next step hb_out (n x Kp),
 * hnorm_out (n).  The caller's h, c and hnorm are not modified (the tail updates copies in scratch of the hook's own). */
int dc_debug_rescore_tail(dc_ctx* ctx, const void* scores, const float* h, const float* c, const float* hnorm,
                          const float* gates_pre_or_null, int n, const int32_t* n_dev_or_null, int32_t* tok_out,
                          int32_t* cand_out, float* best_out, float* h_out, float* c_out, uint16_t* hb_out, float* hnorm_out);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_H */
