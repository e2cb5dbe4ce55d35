/* densecap.h -- C ABI of libdensecap_hip.so
 *
 * MI355X (gfx950) native replacement for the test-time hot path of
 * jcjohnson/densecap:  image -> (boxes, scores, caption tokens), i.e. what
 * `DenseCapModel:forward_test()` (densecap/DenseCapModel.lua:319-327) computes
 * when driven by `run_model.lua:64-87`.
 *
 * The reference has no FFI/plugin registry: its "operator API" is the duck-typed
 * Lua nn.Module protocol.  Each entry point below names the reference interface
 * it replaces (file:line, relative to the reference repo).  The library has no
 * Lua, Python or torch dependency: plain pointers and sizes only.  Host-side
 * mirrors of the reference classes live in lua/ (LuaJIT FFI) and densecap_amd/
 * (Python ctypes); see INTEGRATION.md.
 *
 * Conventions
 *  - all tensors fp32, row-major; token ids int32, 1-based (END = START = V+1)
 *    exactly as the reference's LongTensor `seq` (LanguageModel.lua:30-33);
 *  - box coordinates are 1-based image pixels like the reference; INDEX outputs
 *    (NMS picks) are 0-based;
 *  - every function returns DC_OK (0) or a negative DC_E_* code and never aborts;
 *    dc_last_error() returns the message (replaces Lua assert/error());
 *  - a dc_ctx is bound to one HIP device, owns its stream(s), weights and
 *    workspaces, and is NOT thread-safe (the reference is single-threaded Lua);
 *  - "dev" pointers are HIP device pointers on the ctx's device.  Per-op entry
 *    points (dc_op_*) run on the ctx's primary stream and are synchronous on
 *    return unless stated.
 */
#ifndef DENSECAP_H
#define DENSECAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_OK 0
#define DC_E_INVALID (-1)     /* bad argument / shape            */
#define DC_E_HIP (-2)         /* HIP runtime error               */
#define DC_E_STATE (-3)       /* call order (e.g. no weights)    */
#define DC_E_NOMEM (-4)
#define DC_E_UNSUPPORTED (-5)

#define DC_NUM_VGG_CONVS 13

typedef struct dc_ctx dc_ctx;

/* Weights in the checkpoint's (Torch7) layouts, HOST pointers, fp32.
 * Shapes follow DenseCapModel.lua:61-67,93-100, LocalizationLayer.lua:627-673,
 * LanguageModel.lua:27-61.  The library repacks them into kernel layouts. */
typedef struct dc_weights {
  const float* conv_w[DC_NUM_VGG_CONVS]; /* OIHW (Cout,Cin,3,3): VGG-16 conv1_1..conv5_3 */
  const float* conv_b[DC_NUM_VGG_CONVS]; /* (Cout)                                         */
  const float* rpn_conv_w;  /* (R,512,3,3)  R = rpn_hidden (256)                           */
  const float* rpn_conv_b;  /* (R)                                                         */
  const float* rpn_box_w;   /* (4k,R,1,1)  channel = a*4+d                                 */
  const float* rpn_box_b;   /* (4k)                                                        */
  const float* rpn_score_w; /* (2k,R,1,1)  channel = a*2+{pos,neg}                         */
  const float* rpn_score_b; /* (2k)                                                        */
  const float* fc6_w;       /* (4096, 512*7*7) input index c*49+i*7+j                      */
  const float* fc6_b;
  const float* fc7_w;       /* (4096,4096) */
  const float* fc7_b;
  const float* obj_w;       /* (1,4096)  objectness_branch */
  const float* obj_b;       /* (1) */
  const float* boxreg_w;    /* (4,4096)  box_reg_branch */
  const float* boxreg_b;    /* (4) */
  const float* lm_enc_w;    /* (E,4096)  image_encoder Linear, E = 512 */
  const float* lm_enc_b;    /* (E) */
  const float* lm_emb;      /* (V+2,E)   LookupTable */
  const float* lstm_w;      /* (E+Hd,4*Hd) torch-rnn nn.LSTM weight, gate order i,f,o,g */
  const float* lstm_b;      /* (4*Hd) */
  const float* lm_out_w;    /* (V+1,Hd) */
  const float* lm_out_b;    /* (V+1) */
  const float* anchors;     /* (2,k): row 0 widths, row 1 heights (LocalizationLayer.lua:613-619) */
  float field_centers[4];   /* x0,y0,sx,sy (net_utils.lua:106-140) = 8.5,8.5,16,16 for VGG-16 */
  int32_t num_anchors;      /* k  */
  int32_t rpn_hidden;       /* R  */
  int32_t vocab_size;       /* V  */
  int32_t seq_length;       /* T  */
  int32_t enc_size;         /* E  */
  int32_t rnn_size;         /* Hd */
  int32_t fc_dim;           /* 4096 */
} dc_weights;

/* Result of one image.  Caller owns the buffers (HOST memory) and sets
 * `capacity` >= num_proposals; the library writes K <= capacity rows.
 * Replaces the three return values of DenseCapModel:forward_test
 * (DenseCapModel.lua:319-327): final_boxes (K,4) xcycwh, objectness_scores (K,1)
 * raw logits in decreasing order, and the token matrix `seq` (K,T) that
 * LanguageModel:decodeSequence (LanguageModel.lua:86-103) turns into strings. */
typedef struct dc_result {
  int32_t capacity;  /* in  */
  int32_t K;         /* out */
  int32_t T;         /* out */
  float* boxes;      /* out (capacity,4) xc,yc,w,h */
  float* scores;     /* out (capacity)   */
  int32_t* tokens;   /* out (capacity,T) */
} dc_result;

/* ---- lifecycle ---------------------------------------------------------- */
/* utils.setup_gpus(gpu, use_cudnn) (densecap/utils.lua:22-36): bind to a device. */
int dc_create(dc_ctx** out, int hip_device);
void dc_destroy(dc_ctx* ctx);
/* Lua error()/assert message equivalent. ctx may be NULL (last global error). */
const char* dc_last_error(const dc_ctx* ctx);
/* torch.load(checkpoint).model + model:convert(dtype) (run_model.lua:146-148,
 * DenseCapModel.lua:198-208): upload + repack weights for the kernels. */
int dc_load_weights(dc_ctx* ctx, const dc_weights* w);
/* DenseCapModel:setTestArgs{rpn_nms_thresh,final_nms_thresh,num_proposals}
 * (DenseCapModel.lua:185-191). num_proposals = -1 = uncapped RPN NMS (capacity = all anchors of the image,
 * LocalizationLayer.lua:322-324); final_nms_thresh <= 0 = no final NMS (DenseCapModel.lua:261). */
int dc_set_test_args(dc_ctx* ctx, float rpn_nms_thresh, float final_nms_thresh, int num_proposals);
/* LocalizationLayer:setTestArgs{clip_boxes=, nms_thresh=, max_proposals=} (LocalizationLayer.lua:233-238), which
 * train.lua:139-142 calls directly.  clip_boxes = 0: the RPN boxes are neither clipped to the image nor masked
 * (LocalizationLayer.lua:272-300 is skipped) -- every anchor stays a candidate of the RPN NMS.
 * dc_set_test_args IS this call with clip_boxes = 1 plus the final threshold: the reference's DenseCapModel:setTestArgs
 * passes no `clip_boxes` key, so every call of it turns clipping back on. */
int dc_set_localization_test_args(dc_ctx* ctx, int clip_boxes, float nms_thresh, int max_proposals);

/* ---- the hot path ------------------------------------------------------- */
/* DenseCapModel:forward_test(input) (DenseCapModel.lua:319-327) for one image
 * (3,H,W) BGR, mean-subtracted (run_model.lua:67-74).  img_on_device != 0 means
 * `img_chw` is a device pointer (inputs resident in HBM).  Synchronous. */
int dc_forward_test(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, dc_result* out);
/* Score query phrases against the image's regions: log p(query | region) by the language model, teacher-forced
 * (LanguageModel:updateOutput with a gt_sequence, LanguageModel.lua:106-127; targets of getTarget, :148-167; the
 * captioning loss reads the same scores, DenseCapModel.lua:120,440-445).  For region code c and query w_1..w_L the LSTM
 * reads [image vector, START, w_1 .. w_L] and loglik = sum of log LogSoftMax(scores)[y] over the targets
 * [w_1 .. w_L, END] (L+1 terms, natural log).  The regions are the K rows dc_forward_test returns for the same image and
 * settings, in the same order; `out` is filled as dc_forward_test fills it.  out->tokens == NULL: the forward runs without
 * the caption decode (boxes, scores and loglik are the same bits either way).
 * queries: host (Q, Tq) int32, each row 1-based ids in [1, V] followed by zeros (an all-zero row is the empty query),
 * 1 <= Tq <= 64, Q >= 1.  loglik: host (out->capacity, Q), entry k*Q + q.  fp32 MFMA whatever dc_set_math_mode says,
 * never graph-replayed; results do not depend on Q, the query order or the chunking.  K > out->capacity is refused. */
int dc_score_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                      const int32_t* queries, int Q, int Tq, dc_result* out, float* loglik);
/* Localise phrases (docs/SEMANTICS.md, "Localising phrases"): for every query, the best-fitting boxes among ALL proposals of the
 * image -- not only the rows the objectness-ordered final NMS kept.  nms_thresh in [0, 1]: the IoU threshold of the per-query
 * NMS; max_regions = M in 1..4096: picks returned per query; min_objectness: proposals whose raw objectness is below it (or NaN)
 * are no candidates, -INFINITY = all are.  Anything else (a NaN included) is DC_E_INVALID before any work. */
typedef struct dc_localize_opts { float nms_thresh; int32_t max_regions; float min_objectness; } dc_localize_opts;
/* The forward of dc_forward_test (`out` as there; out->tokens == NULL skips the caption decode), then every proposal row is
 * scored against the queries (rules of dc_score_captions) and, per query, a greedy NMS ordered by that query's log-likelihood
 * (decreasing; ties: the lower proposal row; a NaN log-likelihood is no candidate) runs over the final boxes of all proposals.
 * Host outputs, query q's j-th pick (best first) at q*M + j: count (Q); boxes (Q, M, 4) xcycwh in the frame of dc_result.boxes;
 * loglik (Q, M): the number dc_score_captions returns for that proposal and query under final_nms_thresh = 0, bit for bit;
 * objectness (Q, M): the raw score; region (Q, M): the row of `out` that is the same proposal, -1 if the final NMS dropped it.
 * Entries from count[q] on are not written.  The result does not depend on final_nms_thresh, the caption order, lanes or
 * groups, nor a query's rows on the other queries.  fp32 language model whatever dc_set_math_mode says, never graph-replayed.
 * DC_E_UNSUPPORTED when a forward of this size has more than 4096 proposal rows (num_proposals = -1 on a large image);
 * K > out->capacity is refused.  No proposals: every count is 0. */
int dc_localize_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                         const int32_t* queries, int Q, int Tq, const dc_localize_opts* opts, dc_result* out,
                         int32_t* count, float* boxes, float* loglik, float* objectness, int32_t* region);
/* Sample captions: LanguageModel:sample with sample_argmax = false (LanguageModel.lua:40-41,328-333).  num_samples = S draws
 * per region (1..256); every word is drawn from SoftMax(scores / temperature), temperature in [0.01, 100], or with
 * temperature 0 (S must then be 1) taken by the greedy rule; seed selects the noise, which is counter-based: a draw depends on
 * (seed, draw s, region row r, step, word) and on nothing else.  Definition and rules: docs/SEMANTICS.md, "Sampling captions". */
typedef struct dc_sample_opts {
  int32_t num_samples; float temperature; uint64_t seed;
} dc_sample_opts;
/* The forward of dc_forward_test, then S draws for each of the K regions it returns, in its order (r = output row).  `out` is
 * filled as dc_forward_test fills it; out->tokens == NULL skips the greedy decode (boxes, scores, samples and logprob are the
 * same bits either way).  samples: host (out->capacity, S, T) int32, entry (k*S + s)*T + t: 1-based word ids up to and
 * including the first END (= V+1), zeros after it.  logprob: host (out->capacity, S): the model's own natural-log probability
 * (temperature 1) of the words written, END included; for a row that contains END it is the number dc_op_lm_score returns for
 * that caption on that region.  fp32 MFMA whatever dc_set_math_mode says, never graph-replayed, beam size ignored.  Options
 * outside the ranges above are refused with DC_E_INVALID before anything is enqueued; K > out->capacity is refused. */
int dc_sample_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                       dc_result* out, int32_t* samples, float* logprob);
/* Truncation of the sampling distribution, at every step of every draw (docs/SEMANTICS.md, "Truncation: top-k and nucleus"):
 * top_k = 0 (off) or 1..V+1 keeps the top_k best-scoring words; top_p = 1 (off) or in (0, 1) then keeps the smallest prefix of
 * those, best first, whose renormalised probability at the call's temperature reaches top_p.  {0, 1.0f} = no truncation.
 * Ties: the lower word id first.  Any truncation needs temperature > 0. */
typedef struct dc_sample_trunc { int32_t top_k; float top_p; } dc_sample_trunc;
/* dc_sample_captions with truncation.  trunc == NULL or {0, 1.0f} together with sample_logprob == NULL IS dc_sample_captions
 * (the same code path, the same bits); anything else runs on the row route (full logits per step, one row kernel), whose words
 * follow the same definition but may differ from the fused route's at near-ties.  logprob keeps its meaning (the model's own
 * probability at temperature 1, untruncated; on the row route within the stage bound of dc_op_lm_score, not bit-equal).
 * sample_logprob: NULL, or host (out->capacity, S): the natural-log probability of the draw under the distribution it was
 * drawn from (temperature and truncation applied).  A top_k outside 0..V+1, a top_p outside (0, 1] or truncation at
 * temperature 0 is refused with DC_E_INVALID, a vocabulary whose row does not fit a workgroup's LDS with DC_E_UNSUPPORTED, both
 * before anything is enqueued. */
int dc_sample_captions_trunc(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                             const dc_sample_trunc* trunc_or_null, dc_result* out, int32_t* samples, float* logprob,
                             float* sample_logprob_or_null);
/* Standard beam search (docs/SEMANTICS.md, "Standard beam search"): the N best captions of every region with the model's
 * log-probability of each.  Unlike the reference-rule search of dc_set_beam_size -- which stays what it is -- a finished
 * hypothesis is set aside (it competes as ONE candidate with its score unchanged, and adds no word), every hypothesis starts from
 * the true (h, c) of the START step, and all n_best <= beam_size hypotheses leave the library, ranked by
 * logprob / len^length_alpha (len = words written, END included; length_alpha 0 = by log-probability).
 * beam_size in 1..32 and <= V+1, n_best in 1..beam_size, length_alpha in [0, 2]: anything else is DC_E_INVALID before any work;
 * a vocabulary whose row does not fit the top-k kernel's LDS is DC_E_UNSUPPORTED.  Always fp32, never graph-replayed, and
 * independent of dc_set_beam_size. */
typedef struct dc_beam_opts { int32_t beam_size; int32_t n_best; float length_alpha; } dc_beam_opts;
/* The forward of dc_forward_test (out as there; out->tokens == NULL skips the greedy decode), then the search on the K regions it
 * returns, in its order.  captions: host (out->capacity, n_best, T) int32 -- word ids up to and including END, zeros after it,
 * best first; logprob: host (out->capacity, n_best) -- the UNNORMALISED natural-log probability of the words written.  Rows
 * from K on are not written.  K > out->capacity is refused.  A region whose scores are NaN (non-finite codes) has all-zero
 * rows and NaN log-probabilities. */
int dc_beam_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_beam_opts* opts, dc_result* out,
                     int32_t* captions, float* logprob);
/* ---- validation losses (docs/SEMANTICS.md, "Validation losses") ----
 * The six numbers DenseCapModel:forward_backward returns (DenseCapModel.lua:401-474, LocalizationLayer.lua:383-527) and
 * eval_utils.eval_split averages (eval/eval_utils.lua:54-59,78-81): the forward half only, the two Dropout layers of
 * recog_base by dc_set_dropout (0, the default: the identity).  The sampler's rules: see dc_op_box_sampler. */
/* Settings of the training forward (train_opts.lua:18-40).  The sampler reads batch_size (even, 2..1024), high_thresh and
 * low_thresh (numbers in [0, 1], low <= high), remove_outbounds (0 / 1) and seed; the five weights belong to the loss terms.
 * Defaults of the reference: 256, 0.7, 0.3, 1, mid_box_reg 0.05, mid_objectness 0.1, end_box_reg 0.1, end_objectness 0.1,
 * captioning 1.0. */
typedef struct dc_loss_opts {
  int32_t batch_size; float high_thresh; float low_thresh; int32_t remove_outbounds;
  float mid_box_reg_weight; float mid_objectness_weight; float end_box_reg_weight; float end_objectness_weight;
  float captioning_weight; uint64_t seed;
} dc_loss_opts;
/* The reference's debug_pos_sample_idx / debug_neg_sample_idx (BoxSampler.lua:154-159): HOST lists that take the place of a
 * class's draws.  Entry q is the 0-based rank, in the class's ascending list of candidates, of the q-th sampled row; a non-NULL
 * list sets that class's count to its length (0 .. batch_size), a NULL list leaves the class to the rule. */
typedef struct dc_sampler_forced {
  const int32_t* pos_sample_idx; int32_t num_pos;
  const int32_t* neg_sample_idx; int32_t num_neg;
} dc_sampler_forced;
#define DC_SAMPLER_NO_NEGATIVES 1       /* flags: no input was negative, the negatives are the non-positives            */
#define DC_SAMPLER_NEG_REPLACEMENT 2    /*        fewer negatives than wanted: they were drawn with replacement         */
typedef struct dc_losses {
  double mid_objectness_loss; double mid_box_reg_loss; double end_objectness_loss; double end_box_reg_loss;
  double captioning_loss; double total_loss;
  int32_t num_pos; int32_t num_neg; int32_t total_pos; int32_t total_neg;
  int32_t masked_mid; int32_t masked_end;   /* positive rows whose box-regression target exceeded 10 (zeroed, still counted) */
  int32_t flags;                            /* DC_SAMPLER_NO_NEGATIVES | DC_SAMPLER_NEG_REPLACEMENT */
} dc_losses;
/* The sampler's three lists of a dc_forward_losses call (the reference's dump_vars): HOST buffers of batch_size int32 each,
 * 0-based; num_pos / num_pos / num_neg entries are written. */
typedef struct dc_loss_dump { int32_t* pos_input_idx; int32_t* pos_target_idx; int32_t* neg_input_idx; } dc_loss_dump;
/* One image (3,H,W) as dc_forward_test takes it.  gt_boxes: HOST (G,4) xc,yc,w,h in the frame of the resized image, finite,
 * w > 0, h > 0; gt_labels: HOST (G,L) int32, each row words in [1, V] followed by zeros; 1 <= G <= 512, 1 <= L <= 64.
 * opts_or_null: NULL = the reference's defaults with seed 0.  forced_or_null: caller-forced sample lists.
 * RPN in training form (all k*h*w rows, boxes not clipped, raw two-class scores), the sampler, RoI pooling + fc6 / fc7 + the
 * recognition heads on the num_pos + num_neg sampled rows (positives first), the language model teacher-forced on every
 * positive row against the labels of its ground-truth box, then the five criteria in double and their sum.
 * Eager, on lane 0, fp32 whatever dc_set_math_mode says, never graph-replayed; the dense GEMMs are planned on batch_size rows.
 * The result does not depend on num_proposals, lanes, groups, caption order or beam size, and the call leaves every setting
 * as it found it.  Anything outside the ranges above is refused (DC_E_INVALID; G > 512: DC_E_UNSUPPORTED) before anything is
 * enqueued; forced lists that give more than batch_size rows in all are DC_E_INVALID.
 * Stage-wise test hooks, read with dc_debug_fetch after a call that completed its forward (dc_loss_gradients and
 * dc_forward_backward run the same one and leave the same): "loss_rpn_boxes", "loss_rpn_anchors", "loss_rpn_trans" (A,4),
 * "loss_rpn_scores" (A,2) float; "loss_obj" (n), "loss_final_trans" (n,4), "loss_roi_boxes" (n,4), "loss_codes" (n,fc_dim),
 * "loss_fc6_out" (n,fc_dim) float of the n sampled rows (the last two as fc7 and the heads read them: after Dropout); "loss_rowlik" (num_pos) double, every positive row's caption log-likelihood; "loss_stage_ms" 5 float: trunk + RPN, match + assign + draw,
 * RoI pool + fc, paired scoring, loss terms. */
int dc_forward_losses(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts_or_null,
                      const dc_sampler_forced* forced_or_null, dc_losses* out, const dc_loss_dump* dump_or_null);
/* run_model.lua:160-180 host loop over images, n images of identical size laid out
 * back to back; images are software-pipelined over the ctx's lanes (streams). */
int dc_forward_batch(dc_ctx* ctx, const float* imgs, int n, int H, int W, int imgs_on_device,
                     dc_result* outs);
/* The same loop over images of DIFFERENT sizes (a directory of photographs: run_model.lua -input_dir): imgs[i] is
 * image i, (3, H[i], W[i]); images are pipelined over the lanes exactly like dc_forward_batch, each lane's workspace
 * growing to the largest size it meets.  Results are those of dc_forward_test on each image. */
int dc_forward_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                      dc_result* outs);
/* Number of lanes (HIP streams with private workspaces, 1..4, default 3) dc_forward_batch
 * pipelines images over.  1 = single-image mode (lowest latency for one image at a time): a layer's last
 * partial round of tiles may be shared along K by the idle CUs (a different but fixed fp32 summation order) and the decode
 * rows advance as two blocks on two streams (same arithmetic per row); per-kernel profiling (dc_mfma_profile)
 * keeps every kernel on one stream.  Results are bit-identical for a given lanes setting however images are batched. */
int dc_set_lanes(dc_ctx* ctx, int lanes);
/* Images per GROUP inside dc_forward_batch, 1 .. 8 (0 or 1 = every image on its own, the default; up to 4 through round 5): the images of a
 * group share the launches of the dense stages (the convolutions run over all of them, fc6 / fc7 and the decode over all
 * their RoI rows: fuller tile rounds, a fraction of the launches per image) and of the batched per-image kernels (RPN
 * decode, RoI pooling, gathers); the NMS runs follow each other.  Every decision that changes a sum's order (kernel
 * route, split-K factor) is planned on ONE image's problem, so an image's results do not depend on the group it travels
 * in (bit-identical, like the lane count; tests/fuzz_groups.py).  In single-image mode (dc_set_lanes(1)) the setting is
 * ignored and images travel alone: that mode shares a layer's partial last tile round along K, a plan made for one
 * image's tile count.  Measured at 720x600 / 1000 proposals: 183 images/s with groups of four on two or four lanes against
 * 182 ungrouped; 317 against 285 at 300 proposals; round 6: groups of eight on two lanes 184 against 181 with groups of four,
 * with captions after the final NMS 239-240 against 238 (a packed decode of ~1800 rows a launch). */
int dc_set_group(dc_ctx* ctx, int images);
/* Caption order. 0 (default) = the reference's order: LanguageModel:sample runs on all num_proposals
 * RoIs and the final NMS then keeps K rows (DenseCapModel.lua:127-162,261-275).  1 = run the final NMS
 * first and decode only the K surviving rows: LSTM rows are independent, so boxes, scores and tokens
 * are bit-identical, with ~K/num_proposals of the decode work. */
int dc_set_caption_order(dc_ctx* ctx, int after_final_nms);
/* Dropout of the training forward (docs/SEMANTICS.md, "Dropout"): p of the two nn.Dropout layers of recog_base, after fc6's
 * ReLU (layer 1) and after fc7's (layer 2); models.lua's drop_prob, 0.5 in train_opts.lua.  0 (the default) = none: every call
 * issues the launches and gives the bits it gives without the setting.  A float in [0, 1); NaN, p < 0 and p >= 1 are
 * DC_E_INVALID, as nn.Dropout refuses them.  Read by dc_forward_losses, dc_loss_gradients, dc_forward_backward,
 * dc_forward_backward_cnn, dc_train_step and dc_op_recog_grad, whose masks follow dc_loss_opts.seed; by nothing else:
 * dc_forward_test, scoring, sampling, beam search, dc_forward_boxes and feature extraction never drop. */
int dc_set_dropout(dc_ctx* ctx, float p);
int dc_get_dropout(dc_ctx* ctx, float* p);
/* Arithmetic of the dense contractions (convolutions, nn.Linear, LSTM / vocabulary products).
 *   DC_MATH_FP32 (0, the default): fp32 MFMA, v_mfma_f32_32x32x2_f32 -- an exact fp32 multiply-add chain, the arithmetic the
 *     reference computes in (DenseCapModel.lua:73-76,133) and the only mode whose results are compared bit for bit.
 *   DC_MATH_SPLIT_BF16 (1, opt-in): every fp32 operand is split, in registers, into three bf16 values that sum to it
 *     exactly; six of the nine partial products (all but those below 2^-26 of the product) are accumulated in fp32 on
 *     v_mfma_f32_32x32x16_bf16, which runs at 16x the fp32 MFMA rate -- 2.67x the matrix throughput.  Error against an fp64
 *     result is of the fp32 path's size (tests: <= 1.5x), but the bits differ: NMS / arg-max decisions that hang on the
 *     last ulp may fall the other way, as between any two fp32 summation orders.  Non-finite operands give NaN where fp32
 *     gives inf.  Inputs, outputs and everything between the contractions stay fp32; conv1_1 (3 input channels), the
 *     objectness / box-regression heads and every contraction too small to fill the chip with whole tiles (one image's
 *     conv5_x, RPN conv, LM encoder; everything at webcam sizes) stay on the fp32 path -- the mode is taken layer by
 *     layer, by a rule that depends on ONE image's problem only (results do not depend on lanes or groups).
 * May be changed between forwards; weights need no reloading. */
#define DC_MATH_FP32 0
#define DC_MATH_SPLIT_BF16 1
int dc_set_math_mode(dc_ctx* ctx, int mode);
/* Graph replay (0 = off, the default).  1: a lane that is handed the same work again -- same image size, proposal
 * capacity, group size and settings -- captures its forward once (the second time the key is seen; the first runs
 * eagerly so that every lazy allocation has happened) and relaunches it afterwards as one hipGraph: ~95 kernel launches
 * and copies of an image become one call, the gaps between dependent kernels shrink.  A scheduling knob like the lane
 * count: the kernels and their arguments are the captured ones, results are bit-identical.  Pays in the latency regime
 * (one image in flight, small proposal counts: the webcam daemon); with two or more lanes the other lane already fills
 * the gaps.  Stage times (dc_stage_times) are not available for replayed forwards; beam search and per-launch
 * profiling stay eager.  A forward that this runtime cannot capture turns replay off for the ctx: the forward still runs
 * (eagerly, DC_OK), one warning goes to stderr, and dc_debug_fetch(ctx, "graph_replay_on") reads 0 with the reason
 * left in dc_last_error. */
int dc_set_graph_replay(dc_ctx* ctx, int on);
/* LanguageModel.beam_size (LanguageModel.lua:129-131): 0 (default) = greedy LM:sample; 1..32 = LM:beamsearch
 * (LanguageModel.lua:170-290) with that many beams.  Ties in torch.topk (unspecified in the reference; they occur for
 * finished beams, whose next-word log-probabilities are zeroed) resolve to the lower index. */
int dc_set_beam_size(dc_ctx* ctx, int beam_size);
/* DenseCapModel:extractFeatures (DenseCapModel.lua:285-304): boxes (K,4) and fc7
 * codes (K,fc_dim) after the final NMS; the LSTM decode is skipped. Host outputs. */
int dc_extract_features(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                        int capacity, float* boxes, float* feats, int32_t* K);

/* extract_features.lua's loop (extract_features.lua:79-91) over n images of possibly different sizes, pipelined over
 * the lanes like dc_forward_images: image i writes K[i] rows to boxes + i*capacity*4 and feats + i*capacity*fc_dim. */
int dc_extract_features_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n,
                               int imgs_on_device, int capacity, float* boxes, float* feats, int32_t* K);

/* ---- caller-supplied boxes ------------------------------------------------ */
/* DenseCapModel:updateOutput's test path (DenseCapModel.lua:242-275) with the caller's boxes in the place of the
 * localisation layer's roi_boxes: bilinear RoI pooling on conv5_3, fc6 / fc7, objectness and box regression,
 * final_boxes = ApplyBoxTransform(boxes, final_trans), the language model and the final NMS (final_nms_thresh > 0).  The
 * RPN convolution, its heads, the anchor decode and the RPN NMS are not run; everything after them behaves as in
 * dc_forward_test under the same settings (caption order, beam size, math mode, lanes, groups, graph replay).  It is the
 * inference form of LocalizationLayer:_forward_train's ground-truth path (LocalizationLayer.lua:383-527).
 *  - boxes: HOST memory, (n,4) fp32 xc,yc,w,h, 1-based pixels of the RESIZED image handed to the call -- the frame
 *    dc_result.boxes is written in: an output of the library is a valid input;
 *  - 1 <= n <= P, the row capacity of a forward of that image size (num_proposals of dc_set_test_args; every GEMM is
 *    planned as for a forward whose RPN NMS kept n boxes).  More boxes are refused: raise num_proposals;
 *  - a non-finite coordinate, w <= 0 or h <= 0 in any box refuses the whole call (DC_E_INVALID, dc_last_error names the
 *    first bad box) before anything is enqueued;
 *  - flags = 0: the boxes are used as given, like the ground-truth boxes of _forward_train.  DC_BOXES_CLIP:
 *    box_utils.clip_boxes(boxes, {1,1,W,H}, 'xcycwh') first (box_utils.lua:486-523, the RPN path's clip: every box loses
 *    one pixel of w and h, so do NOT set it for boxes that came out of the library), boxes that come out invalid are
 *    dropped and the rest keep their order (LocalizationLayer.lua:272-300); all dropped: K = 0, DC_OK;
 *  - src (optional, per list): src[r] = 0-based index, into the caller's array and counted before any drop, of the box
 *    behind result row r.  Rows come back in input order when final_nms_thresh <= 0 (DenseCapModel.lua:261), else in
 *    decreasing objectness -- the raw logits of the recognition net, which say how box-like the model finds a region: a
 *    caller who wants EVERY box described sets final_nms_thresh to 0;
 *  - the matching result needs capacity >= n; out->tokens == NULL (in every result of the call) skips the caption decode,
 *    as in dc_score_captions. */
#define DC_BOXES_CLIP 1
typedef struct dc_box_list {
  const float* boxes; /* in  (n,4) xc,yc,w,h, host memory */
  int32_t n;          /* in  */
  int32_t* src;       /* out (capacity of the matching result) or NULL */
} dc_box_list;
int dc_forward_boxes(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_box_list* bl, int flags,
                     dc_result* out);
/* The loop over n images of possibly different sizes, bl[i] the boxes of image i (each its own n); pipelined over the lanes
 * and grouped (dc_set_group) like dc_forward_images.  Results are those of dc_forward_boxes image by image. */
int dc_forward_boxes_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                            const dc_box_list* bl, int flags, dc_result* outs);
/* dc_extract_features_images on the caller's boxes: image i writes K[i] rows (box after regression, fc7 code) to
 * boxes + i*capacity*4 and feats + i*capacity*fc_dim, capacity >= every n.  The final NMS runs as in extractFeatures
 * (DenseCapModel.lua:285-304) EXCEPT that final_nms_thresh <= 0 means no NMS here: all rows, in input order -- a caller of
 * this function wants the codes of the boxes it passed. */
int dc_extract_features_boxes(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                              const dc_box_list* bl, int flags, int capacity, float* boxes, float* feats, int32_t* K);
/* run_model.lua:67-74 (`run_image` before the forward) on the device: image.load's byte -> float conversion (byte / 255),
 * image.scale(img, image_size) -- torch/image's scaleBilinear: scaleLinear_rowcol along the width, then the height; linear
 * interpolation where a side grows, area averaging where it shrinks; the longer side becomes image_size --, RGB -> BGR,
 * x 255, minus the VGG mean (103.939, 116.779, 123.68).  rgb_hwc: (H0, W0, 3) bytes as a JPEG decoder delivers them, host or
 * device memory (on_device); out_chw_dev: (3, H, W) fp32 on the device with (H, W) from dc_preprocess_size -- the tensor
 * dc_forward_test / dc_forward_images take with img_on_device = 1; scaled_rgb_dev (optional, device): the scaled image as
 * (H, W, 3) bytes, what run_model.lua:184 saves for the visualiser.  Every sample is the same chain of fp32 operations as the
 * library's C loops (bit-equal to the host restatement in densecap_amd/run_model.py).  Synchronous. */
int dc_preprocess_size(int H0, int W0, int image_size, int* H, int* W);
int dc_preprocess_u8(dc_ctx* ctx, const uint8_t* rgb_hwc, int H0, int W0, int on_device, int image_size, float* out_chw_dev,
                     uint8_t* scaled_rgb_dev);

/* Per-stage GPU time of the most recent dc_forward_test on this ctx, measured with
 * HIP events on the ctx's stream (replaces LocalizationLayer:timeit,
 * LocalizationLayer.lua:219-230).  names[i] are static strings.  Returns the
 * number of stages written (<= max_stages). */
int dc_stage_times(dc_ctx* ctx, const char** names, float* ms, int max_stages);
/* ---- multi-GPU: image shards + ONE gather ------------------------------------ */
/* The reference binds one device (densecap/utils.lua:22-36) and loops over images on it
 * (run_model.lua:160-180).  Here images shard by index over ranks (one process or thread and one
 * dc_ctx per GPU, weights replicated, no data-path exchange); the only communication is one gather
 * of the per-image results on rank 0: RCCL point-to-point over xGMI, rank 0 posting world-1 receives
 * and every peer one send inside a single group.  librccl is dlopen()ed by dc_comm_create (world > 1)
 * or dc_comm_unique_id; the single-GPU path does not depend on it. */
#define DC_COMM_ID_BYTES 128
#define DC_COMM_SELF_TRANSPORT 1 /* dc_comm_create_ex flag */
typedef struct dc_comm dc_comm;
/* Rank 0 creates the 128-byte rendezvous id (ncclUniqueId) and hands it to the other ranks out of
 * band (file, environment, launcher). */
int dc_comm_unique_id(void* id_out);
/* Collective over all ranks (blocks until everyone has joined).  world == 1 needs no id and no RCCL. */
int dc_comm_create(dc_comm** out, dc_ctx* ctx, const void* id, int rank, int world);
/* The same with flags.  DC_COMM_SELF_TRANSPORT (world == 1 only; ignored otherwise): build the carrier for the single
 * rank as well -- ncclCommInitRank with one rank (id may be NULL: the library makes one) -- and route every gather through
 * the staging buffers and one ncclGroupStart / ncclRecv / ncclSend / ncclGroupEnd with rank 0 as its own peer, the calls a
 * multi-GPU gather makes.  Lets the RCCL path be executed and checked byte for byte on a one-GPU machine.
 * dc_comm_create behaves like this when the environment holds DC_COMM_FORCE_RCCL=1. */
int dc_comm_create_ex(dc_comm** out, dc_ctx* ctx, const void* id, int rank, int world, int flags);
/* What carries this communicator's gathers: "host copy" (world == 1, no carrier), "rccl", "rccl, self", "loopback",
 * "loopback, self".  Static string. */
const char* dc_comm_transport(const dc_comm* comm);
void dc_comm_destroy(dc_comm* comm);
const char* dc_comm_last_error(const dc_comm* comm);
/* Gather `n_local` results (as filled by dc_forward_test / dc_forward_batch: same capacity and T on
 * every rank) from every rank on rank 0.  gathered: rank 0 passes world*n_local caller-allocated
 * results (capacity >= the senders'); entry r*n_local + i receives image i of rank r.  Other ranks
 * pass NULL.  One record per image travels as {K, T, capacity; boxes; scores; int32 tokens}. */
int dc_gather_results(dc_comm* comm, const dc_result* local, int n_local, dc_result* gathered);

/* ---- device memory helpers (for hosts without a GPU allocator, e.g. LuaJIT) -- */
int dc_malloc(dc_ctx* ctx, void** dev_ptr, size_t bytes);
int dc_free(dc_ctx* ctx, void* dev_ptr);
int dc_memcpy_h2d(dc_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int dc_memcpy_d2h(dc_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int dc_synchronize(dc_ctx* ctx);

/* ---- per-op entry points (device pointers) ------------------------------ */
/* layout changes: the kernels keep activations channels-last (HWC). */
int dc_op_chw_to_hwc(dc_ctx* ctx, const float* in_chw, float* out_hwc, int C, int H, int W);
int dc_op_hwc_to_chw(dc_ctx* ctx, const float* in_hwc, float* out_chw, int C, int H, int W);
/* Repack OIHW (Cout,Cin,3,3) -> (Cout, 9*Cin) with k = (kh*3+kw)*Cin + c. */
int dc_op_pack_conv3x3_weights(dc_ctx* ctx, const float* w_oihw, float* w_packed, int Cout, int Cin);
/* nn.SpatialConvolution(Cin,Cout,3,3,1,1,1,1) [+ nn.ReLU] (VGG layers,
 * DenseCapModel.lua:73-76; RPN conv LocalizationLayer.lua:627-636), fp32 MFMA
 * implicit GEMM.  in: (n_img,H,W,Cin) HWC, Cin % 32 == 0; w_packed from
 * dc_op_pack_conv3x3_weights; out (n_img,H,W,Cout). */
int dc_op_conv3x3(dc_ctx* ctx, const float* in_hwc, const float* w_packed, const float* bias,
                  float* out_hwc, int n_img, int H, int W, int Cin, int Cout, int relu);
/* The same conv + ReLU followed by nn.SpatialMaxPooling(2,2,2,2):ceil() (VGG conv1_2, conv2_2, conv3_3, conv4_3 ->
 * pool1..4, DenseCapModel.lua:61-76) in ONE launch: the pool is taken in the conv's epilogue, the full-resolution
 * activation never reaches HBM.  out (ceil(H/2), ceil(W/2), Cout); bit-identical to dc_op_conv3x3 + dc_op_maxpool2x2_ceil. */
int dc_op_conv3x3_relu_pool(dc_ctx* ctx, const float* in_hwc, const float* w_packed, const float* bias,
                            float* out_hwc, int H, int W, int Cin, int Cout);
/* conv1_1: Cin = 3, reads the (3,H,W) CHW boundary image, writes (H,W,Cout) HWC. */
int dc_op_conv3x3_c3(dc_ctx* ctx, const float* in_chw, const float* w_oihw, const float* bias,
                     float* out_hwc, int H, int W, int Cout, int relu);
/* nn.SpatialMaxPooling(2,2,2,2):ceil() as loadcaffe builds it: (H,W,C)->(ceil(H/2),ceil(W/2),C). */
int dc_op_maxpool2x2_ceil(dc_ctx* ctx, const float* in_hwc, float* out_hwc, int n_img, int H, int W, int C);
/* nn.Linear [+ReLU]: C(M,N) = A(M,K) . W(N,K)^T + bias(N); K % 32 == 0. fp32 MFMA. */
int dc_op_linear(dc_ctx* ctx, const float* A, const float* W, const float* bias, float* C,
                 int M, int N, int K, int relu);
/* nn.MakeAnchors (MakeAnchors.lua:40-67) + nn.ReshapeBoxFeatures order: out (k*h*w,4). */
int dc_op_make_anchors(dc_ctx* ctx, float* out, int h, int w, float x0, float y0, float sx, float sy,
                       const float* anchors_dev /*(2,k)*/, int k);
/* nn.ApplyBoxTransform (ApplyBoxTransform.lua:63-90): (n,4),(n,4)->(n,4). */
int dc_op_apply_box_transform(dc_ctx* ctx, const float* boxes, const float* trans, float* out, int n);
/* box_utils.clip_boxes(boxes,{x_min=1,y_min=1,x_max=W,y_max=H},'xcycwh') (box_utils.lua:486-523). */
int dc_op_clip_boxes(dc_ctx* ctx, const float* boxes, float* clipped, uint8_t* valid, int n,
                     float x_min, float y_min, float x_max, float y_max);
/* box_utils.xcycwh_to_x1y1x2y2 (box_utils.lua:270-298). */
int dc_op_xcycwh_to_x1y1x2y2(dc_ctx* ctx, const float* boxes, float* out, int n);
/* nn.BoxIoU (BoxIoU.lua:40-73): (B1,4),(B2,4) xcycwh -> (B1,B2).  convention:
 * DC_IOU_BOXIOU_MODULE (0) the module as written ((w-1)/2 corners, area w*h, no +1);
 * DC_IOU_NMS_PLUS1 (1) box_utils.nms inline form (box_utils.lua:178-181,219-227: +1 on every extent);
 * DC_IOU_LEGACY_HALF_W (2) the module's original converter (BoxIoU.lua:15-37, xc -/+ w/2), the one
 * test/BoxIoU_test.lua:13-94 was written for. */
#define DC_IOU_BOXIOU_MODULE 0
#define DC_IOU_NMS_PLUS1 1
#define DC_IOU_LEGACY_HALF_W 2
int dc_op_box_iou(dc_ctx* ctx, const float* b1, const float* b2, float* out, int B1, int B2, int convention);
/* Fused LocalizationLayer._forward_test lines 265-308 after the head convs: heads (h,w,6k)
 * HWC with channels [0,4k) box (a*4+d) and [4k,6k) score (a*2+d) -> per anchor-row
 * b = a*h*w + y*w + x: boxes (clipped xcycwh), anchors, trans, x1y1x2y2, p, valid. Any out may be NULL. */
int dc_op_rpn_decode(dc_ctx* ctx, const float* heads_hwc, int h, int w, int k, const float* anchors_dev,
                     float x0, float y0, float sx, float sy, int img_h, int img_w,
                     float* boxes, float* anchors_out, float* trans, float* x1y1x2y2, float* p, uint8_t* valid);
/* box_utils.nms (box_utils.lua:154-256).  boxes (n,4) x1y1x2y2, scores (n), valid (n) or
 * NULL; max_boxes < 0 = uncapped.  Writes 0-based picks (capacity >= min(n,max_boxes))
 * in decreasing score order (ties: lower index first) and their count (device int32). */
int dc_op_nms(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid, int n,
              float thresh, int max_boxes, int32_t* picks, int32_t* count);
/* The per-query NMS of dc_localize_captions: dc_op_nms on ONE box list under Q score columns in one pass.  boxes (n,4)
 * x1y1x2y2, scores (n, Q) entry r*Q + q (the layout dc_op_lm_score writes), valid (n) or NULL.  For every column q the picks of
 * dc_op_nms with max_boxes = max_picks on the candidates of q -- the rows with valid[r] != 0 whose score in column q is not
 * NaN; a row that is no candidate is never picked and never suppresses (dc_op_nms ranks a NaN first instead).  picks
 * (Q, max_picks) int32 0-based, -1 past counts[q]; counts (Q).  1 <= n <= 4096 (more: DC_E_UNSUPPORTED), 1 <= max_picks <= 4096,
 * Q >= 1.  A column's result does not depend on Q, the other columns or their order.  Device pointers; synchronous. */
int dc_op_nms_multi(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n, int Q,
                    float thresh, int max_picks, int32_t* picks, int32_t* counts);
/* DenseCaptioningEvaluator:addResult (eval/eval_utils.lua:148-221) for n_images images in one launch; rules in docs/SEMANTICS.md,
 * "Evaluation".  Ragged: image i's detections are rows det_off[i] .. det_off[i+1]-1 of det_boxes (xcycwh) / det_scores, its
 * ground truth rows gt_off[i] .. gt_off[i+1]-1 of gt_boxes (xcycwh); both offset lists have n_images + 1 entries, start at >= 0
 * and do not decrease.  The ground truth is merged (IoU >= merge_thresh, the reference's 0.7), the detections are taken in
 * decreasing score (ties: lower index; NaN last) and claim the merged box they overlap most.  Per image, d = rank in score
 * order, at det_off[i] + d: order (the detection's index within the image), ov (float64), group (0-based merged box, -1 = none),
 * ok (1 = the claimed group was still free).  At gt_off[i] + j: gt_group (the group of ground-truth box j); at gt_off[i] + g:
 * merged_boxes (4 float64 x1y1x2y2 of group g; rows from n_groups[i] on are zero).  n_groups (n_images).
 * flags: DC_EVAL_CLAIM_LAST = a detection that overlaps nothing claims the LAST group (the reference's used[-1]); without it
 * such a detection claims nothing and has ok = 0.  <= 4096 detections and <= 512 ground-truth boxes per image
 * (DC_E_UNSUPPORTED beyond); n_images < 1, merge_thresh NaN or outside (0, 1], unknown flag bits, offsets that are negative or
 * decrease: DC_E_INVALID.  All refusals come before any launch.  Device pointers; synchronous. */
#define DC_EVAL_CLAIM_LAST 1
int dc_op_eval_match(dc_ctx* ctx, const float* det_boxes, const float* det_scores, const int32_t* det_off,
                     const float* gt_boxes, const int32_t* gt_off, int n_images, float merge_thresh, int flags,
                     int32_t* order, double* ov, int32_t* group, uint8_t* ok,
                     int32_t* gt_group, int32_t* n_groups, double* merged_boxes);
/* nn.BoxSampler:updateOutput (BoxSampler.lua:64-167) for one image: boxes (A,4) xcycwh against gt (G,4) xcycwh, IoU in the
 * DC_IOU_BOXIOU_MODULE convention, bit for bit what dc_op_box_iou writes.  max / arg-max per input over the ground truth and per
 * ground-truth box over the inputs (ties: the lower index; a NaN never wins; an input whose IoUs are all NaN is neither positive
 * nor negative); positive = max > high_thresh, negative = max < low_thresh; with remove_outbounds both are cleared for inputs
 * whose (w-1)/2 corners leave [1, img_w] x [1, img_h]; every ground-truth box's best input is then positive whatever its IoU or
 * bounds; no negatives left: the negatives are the non-positives (DC_SAMPLER_NO_NEGATIVES).  num_pos = min(batch_size / 2,
 * total_pos), num_neg = batch_size - num_pos (0 if there is no candidate at all, where the reference stops with an error).
 * Draws are counter-based: candidate i of class c (0 positive, 1 negative) has the key philox4x32_10(i, 0, c, 0, seed).w[0]; the
 * num smallest (key, i) are taken, in that order; with fewer negatives than num_neg (DC_SAMPLER_NEG_REPLACEMENT) draw j takes
 * entry (philox4x32_10(j, 1, 1, 0, seed).w[0] * total_neg) >> 32 of the ascending list.
 * Outputs (device, int32, 0-based): pos_input_idx, pos_target_idx (the arg-max ground-truth box of the sampled input),
 * neg_input_idx, each with room for batch_size entries; counts (8): num_pos, num_neg, total_pos, total_neg, flags, then the number
 * of forced positive / negative ranks outside the candidate list (their rows hold -1 and the call returns DC_E_INVALID), 0.
 * max_iou_or_null (A) float and arg_or_null (A) int32: the per-input max (NaN: no number seen) and arg-max.
 * A < 1, a bad batch size or threshold (NaN included), a forced list longer than batch_size: DC_E_INVALID; G < 1 or G > 512:
 * DC_E_UNSUPPORTED; all before any launch.  Device pointers but for opts and forced; synchronous. */
int dc_op_box_sampler(dc_ctx* ctx, const float* boxes, const float* gt, int A, int G, int img_h, int img_w,
                      const dc_loss_opts* opts, const dc_sampler_forced* forced_or_null, int32_t* pos_input_idx,
                      int32_t* pos_target_idx, int32_t* neg_input_idx, int32_t* counts, float* max_iou_or_null,
                      int32_t* arg_or_null);
/* nn.BilinearRoiPooling forward (BilinearRoiPooling.lua:42-60): feat (h,w,C) HWC, boxes (B,4)
 * xcycwh image px -> out.  out_layout 0: (B,C,HH,WW) as the reference; 1: (B,HH,WW,C). */
int dc_op_bilinear_roi_pool(dc_ctx* ctx, const float* feat_hwc, int h, int w, int C, const float* boxes,
                            int B, int img_h, int img_w, int HH, int WW, float* out, int out_layout);
/* LanguageModel:sample, greedy (LanguageModel.lua:293-348) with the ctx's loaded language
 * model: codes (n,fc_dim) -> tokens (n,T) int32 1-based.  With dc_set_beam_size > 0: LanguageModel:beamsearch. */
int dc_op_lm_sample(dc_ctx* ctx, const float* codes, int n, int32_t* tokens);
/* The scoring of dc_score_captions on given fc7 codes (n, fc_dim): loglik (n, Q), entry r*Q + q.  Device pointers
 * throughout (codes, queries, loglik); synchronous.  Same rules for the queries. */
int dc_op_lm_score(dc_ctx* ctx, const float* codes, int n, const int32_t* queries, int Q, int Tq, float* loglik);
/* Language-model gradients (docs/SEMANTICS.md, "Language-model gradients"): the captioning loss of n (code, caption) pairs and its
 * gradient with respect to the seven language-model tensors and the codes.  codes: DEVICE (n, fc_dim); labels: HOST (n, L) int32,
 * each row words in [1, V] followed by zeros (an all-zero row is an empty caption); loss = weight * (-sum_r rowlik_r) / (n (L+2)),
 * rowlik_r the number dc_op_lm_score gives for the pair (code r, caption r).  out: DEVICE buffers in the layouts of dc_weights --
 * lm_enc_w (E, fc_dim), lm_enc_b (E), lm_emb (V+2, E), lstm_w (E+Hd, 4Hd) gate order i,f,o,g, lstm_b (4Hd), lm_out_w (V+1, Hd),
 * lm_out_b (V+1) -- and codes (n, fc_dim), which may be NULL; all are overwritten.  loss: HOST, one double; rowlik_or_null: HOST
 * (n) doubles.  fp32 whatever dc_set_math_mode says, eager on lane 0, no float atomics (two identical calls give identical
 * bits); the settings and the loaded weights are left as they were.  Synchronous.  Refused with DC_E_INVALID before anything
 * is enqueued: n outside 1..1024, L outside 1..64, a label outside [0, V], a word after a zero, a non-finite weight; with
 * DC_E_UNSUPPORTED: a call whose kept state would exceed 8 GiB of scratch. */
typedef struct dc_lm_grads {
  float* lm_enc_w; float* lm_enc_b; float* lm_emb; float* lstm_w; float* lstm_b; float* lm_out_w; float* lm_out_b; float* codes;
} dc_lm_grads;
int dc_op_lm_grad(dc_ctx* ctx, const float* codes, int n, const int32_t* labels, int L, float weight, const dc_lm_grads* out,
                  double* loss, double* rowlik_or_null);
/* nn.BilinearRoiPooling backward (docs/SEMANTICS.md, "Recognition-net gradients"): feat (h, w, C) HWC, boxes (B, 4) xcycwh image
 * px and dout (B, HH, WW, C) -> dfeat (h, w, C), the scatter of weight * dout over the four taps of every point (out-of-map taps
 * give nothing; every pixel is written, an untouched one is +0.0), and dboxes_or_null (B, 4), the derivatives of sum(dout *
 * pooled) with the floors held constant.  Positions and weights are the forward's bits.  No float atomics: every sum has a fixed
 * order and two identical calls give identical bits.  C % 4 == 0, B >= 1, HH, WW >= 2: DC_E_INVALID otherwise; HH * WW > 256,
 * or h * w > 65536 pixels (the list offsets are scanned by one workgroup; 65536 is the trunk's output for the largest image the
 * forward admits): DC_E_UNSUPPORTED.  The index's scratch is kept by the ctx and only grows.  Device pointers; synchronous. */
int dc_op_roi_pool_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, int C, const float* boxes, int B, int img_h, int img_w,
                        int HH, int WW, const float* dout, float* dfeat, float* dboxes_or_null);
/* Recognition-net gradients (docs/SEMANTICS.md, "Recognition-net gradients"): the gradient of end_objectness + end_box_reg (+ a
 * caller's gradient of the positive codes) through the two recognition heads, fc7, fc6 and RoI pooling.  feat (h, w, 512) HWC,
 * roi_boxes (n, 4) the sampled rows, positives first; target_boxes (num_pos, 4); dcodes_or_null (num_pos, fc_dim): all DEVICE.
 * out: DEVICE buffers, all overwritten -- fc6_w (fc_dim, 512*49) in the checkpoint's (c, i, j) input order, fc6_b, fc7_w
 * (fc_dim, fc_dim), fc7_b, obj_w (fc_dim), obj_b (1), boxreg_w (4, fc_dim), boxreg_b (4), feat (h, w, 512) -- RoI pooling's share
 * of the feature map's gradient -- and roi_boxes (n, 4).  opts_or_null: batch_size (the rows the forward GEMMs are planned on) and
 * the two end weights are read.  The losses (HOST doubles) and masked_end (HOST) are what dc_forward_losses reports for these rows.
 * fp32 whatever dc_set_math_mode says, eager on lane 0, no float atomics; settings and weights are left as they were.
 * Synchronous.  h and w are taken on trust: they are NOT checked against dc_feature_size(img_h, img_w), and only the caller's own
 * feat buffers are indexed by them (the lane's buffers are sized from img_h, img_w and batch_size).  DC_E_INVALID before any
 * launch: n outside 1..1024, num_pos outside 0..n, n > batch_size, a null output, positive rows without target boxes, an image
 * side below 32 px, bad sampler options; DC_E_UNSUPPORTED: h * w > 65536, or scratch above 8 GiB.  The scratch (0.45 GB at the
 * real model) and the two transposed weights (0.48 GB) are kept by the ctx after the first call.  Not here: the CNN's backward (dc_op_cnn_grad, a call of its own). */
typedef struct dc_recog_grads {
  float* fc6_w; float* fc6_b; float* fc7_w; float* fc7_b; float* obj_w; float* obj_b; float* boxreg_w; float* boxreg_b; float* feat; float* roi_boxes;
} dc_recog_grads;
int dc_op_recog_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const float* roi_boxes, int n, int num_pos,
                     const float* target_boxes, const float* dcodes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null,
                     const dc_recog_grads* out, double* end_objectness_loss, double* end_box_reg_loss, int32_t* masked_end);
/* dc_forward_losses (same arguments, the same dc_losses bit for bit), then the gradient of end_objectness + end_box_reg +
 * captioning with respect to every parameter downstream of the RPN: dc_op_lm_grad on the positive rows' codes and the labels of
 * their ground-truth boxes with weight = captioning_weight (lg: its seven tensors, all required; lg->codes may be NULL), then
 * dc_op_recog_grad's backward with those code gradients (rg: all ten required; feat is (h, w, 512) for dc_feature_size(H, W),
 * roi_boxes (num_pos + num_neg, 4) -- batch_size rows of room).  With no sampled row (num_pos + num_neg == 0) or no positive the
 * corresponding gradients are zero.  Every argument, dc_forward_losses' included, is refused before anything is allocated or
 * launched, with dc_forward_losses' codes and texts; the message begins with this function's name (dc_forward_backward: with
 * its own), not with "dc_forward_losses:".  Synchronous. */
int dc_loss_gradients(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                      dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg);
/* The size of the trunk's output map for an H x W image (four ceil-mode 2x2 pools). */
int dc_feature_size(int H, int W, int* h, int* w);
/* The backward of a 3x3 / stride 1 / pad 1 convolution on an HWC map (docs/SEMANTICS.md, "Convolution gradients"), the brick of
 * the RPN's and a CNN's backward: x (h, w, Cin) the layer's input, w (Cout, Cin, 3, 3) its weights in the checkpoint's OIHW order,
 * dy (h, w, Cout) the gradient at the convolution's own output (a ReLU's mask is the caller's) -> dw (Cout, Cin, 3, 3),
 * db (Cout) and dx (h, w, Cin).  Each output may be NULL to skip it; x may be NULL when dw is, w when dx is.  dw is the sum over
 * the pixels of dy times the shifted x, zero outside the map, on the fp32 MFMA with no im2col buffer; dx is the convolution of dy
 * with the flipped, transposed weights on the forward's engine.  fp32 whatever dc_set_math_mode says, no float atomics: every
 * sum has a fixed order and two identical calls give identical bits.  DC_E_INVALID before any launch: Cin % 32, Cout % 32, a
 * non-positive size, a missing input, no output at all; DC_E_UNSUPPORTED: h * w > 65536, or (dx only) a dy the engine's 32-bit
 * operand offsets do not take (Cout > 2048).  Device pointers; synchronous. */
int dc_op_conv3x3_grad(dc_ctx* ctx, const float* x, const float* w, const float* dy, int h, int w_px, int Cin, int Cout, float* dw,
                       float* db, float* dx);
/* ---- CNN gradients (docs/SEMANTICS.md, "CNN gradients") ----
 * The two point-wise kernels of the CNN's backward, alone, on DEVICE pointers; synchronous.
 * dc_op_maxpool2x2_grad: the backward of nn.SpatialMaxPooling(2,2,2,2):ceil() fused with the mask of the in-place nn.ReLU in
 * front of it.  y (n, H, W, C): the map the pool read (the ReLU's output); dpool (n, ceil(H/2), ceil(W/2), C) -> dy (n, H, W, C),
 * every element written: a window is clipped at the map's edge, its gradient goes to its first maximum in scan order (row, then
 * column; `>` is strict) and only if that value is > 0; every other element is +0.0.  No atomics.  C % 4 != 0 or a non-positive
 * size, or a pointer that is not 16-byte aligned (the kernel moves four channels at a time): DC_E_INVALID before any launch.  A NaN
 * in y is never a maximum (every comparison with it is false): y is a ReLU's output, where the forward would have put the NaN
 * into every later map; THNN, which takes a NaN as the maximum, is not followed there. */
int dc_op_maxpool2x2_grad(dc_ctx* ctx, const float* y, const float* dpool, int n, int H, int W, int C, float* dy);
/* dc_op_relu_grad: dy[i] = y[i] > 0 ? dy[i] : +0.0 in place, n_floats of them, any 4-byte alignment.  n_floats < 1: DC_E_INVALID. */
int dc_op_relu_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats);
/* dc_op_dropout: nn.Dropout's forward in place on the DEVICE matrix x (rows, cols), any 4-byte alignment.  Element (row, col) is
 * kept iff (uint64) philox4x32_10(col >> 2, row, layer, 1, seed_lo, seed_hi).w[col & 3] < floor((1 - (double)p) * 2^32); a
 * kept element becomes x * s, s = 1.0f / (1.0f - p) in fp32, one fp32 multiply; a dropped one becomes +0.0 whatever x was (the
 * reference multiplies by 0: a dropped inf or NaN stays NaN there).  p = 0: the identity, nothing is launched.  rows < 1,
 * cols < 1, layer outside 0..255, p outside [0, 1) or NaN: DC_E_INVALID, x untouched. */
int dc_op_dropout(dc_ctx* ctx, float* x, int rows, int cols, int layer, float p, uint64_t seed);
/* dc_op_relu_dropout_grad: the backward of nn.ReLU(true) followed by an in-place nn.Dropout, on the dropped activation y:
 * dy[i] = y[i] > 0 ? dy[i] * s : +0.0 in place (NaN y: 0), n_floats of them, any 4-byte alignment.  p = 0: dc_op_relu_grad. */
int dc_op_relu_dropout_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats, float p);
/* The backward through conv_net2 (DenseCapModel.lua:338-376 with model.finetune_cnn): VGG layers 11..30, that is the nine
 * convolutions conv3_1 .. conv5_3 (index 4..12 of the thirteen; entry i here is convolution 4 + i), their in-place ReLUs, pool3
 * and pool4.  dc_cnn_grads: DEVICE buffers, all overwritten -- conv_w[i] (Cout, Cin, 3, 3) in the checkpoint's OIHW order,
 * conv_b[i] (Cout), all eighteen required; x (h4, w4, 128), the gradient at conv3_1's input, or NULL (conv_net1 is never trained:
 * that product is then not computed).  dc_cnn_dump: optional DEVICE buffers, each filled if not NULL -- act[i] the input of
 * convolution 4 + i, prepool[0] / prepool[1] conv3_3's / conv4_3's output after its ReLU (what pool3 / pool4 read), feat conv5_3's
 * output after its ReLU, dy[i] the gradient at convolution 4 + i's own output, after the mask. */
#define DC_NUM_CNN_GRAD_CONVS 9
typedef struct dc_cnn_grads { float* conv_w[9]; float* conv_b[9]; float* x; } dc_cnn_grads;
typedef struct dc_cnn_dump { float* act[9]; float* prepool[2]; float* feat; float* dy[9]; } dc_cnn_dump;
/* conv_net2's forward from a caller-supplied pool2 map x4_hwc (h4, w4, 128) with the loaded weights, keeping the nine layer
 * inputs and the two pre-pool maps on the device (the ctx keeps them between calls, grow only: 145 MB at 720 x 600, and 0.5 GB
 * of scratch, 400 MiB of it the engine's split-K scratch), then the backward
 * of dfeat_hwc (h6, w6, 512), h6 = ceil(ceil(h4 / 2) / 2): per layer, from conv5_3 down, the ReLU's mask (dc_op_relu_grad; at
 * conv4_3 and conv3_3 dc_op_maxpool2x2_grad), then dc_op_conv3x3_grad's launches for dw, db and dx.  The forward is
 * dc_op_conv3x3 with relu = 1 and dc_op_maxpool2x2_ceil, layer by layer.  fp32 whatever dc_set_math_mode says, eager on lane 0,
 * no float atomics: two identical calls give identical bits; settings and weights are left as they were.  Device pointers;
 * synchronous.  Without weights: DC_E_STATE.  DC_E_INVALID before any launch: a null input or gradient buffer, a non-positive
 * size; DC_E_UNSUPPORTED: h4 * w4 > 65536, in dc_op_conv3x3_grad's words.  Not here: Dropout (conv_net2 has none; the recognition net's is
 * dc_set_dropout), the optimiser (dc_train_step trains the 21 tensors outside the CNN only). */
int dc_op_cnn_grad(dc_ctx* ctx, const float* x4_hwc, int h4, int w4, const float* dfeat_hwc, const dc_cnn_grads* out,
                   const dc_cnn_dump* dump_or_null);
/* RPN gradients (docs/SEMANTICS.md, "RPN gradients"): DEVICE buffers for the gradients of the RPN's six tensors in checkpoint
 * layouts -- rpn_conv_w (rpn_hidden, 512, 3, 3), rpn_conv_b, rpn_box_w (4k, rpn_hidden), rpn_box_b, rpn_score_w (2k, rpn_hidden),
 * rpn_score_b -- and feat (h, w, 512), a gradient of the feature map.  All required, all overwritten. */
typedef struct dc_rpn_grads {
  float* rpn_conv_w; float* rpn_conv_b; float* rpn_box_w; float* rpn_box_b; float* rpn_score_w; float* rpn_score_b; float* feat;
} dc_rpn_grads;
/* The RPN half of the training step on caller-supplied data, as dc_op_recog_grad is the recognition half: the gradient of
 * mid_objectness + mid_box_reg + 0.5 * box_reg_decay * |transforms|^2 + <droi_boxes, sampled boxes> through the sampler's
 * backward, the two 1x1 heads and the RPN's 3x3 convolution.  feat_hwc (h, w, 512); pos_input_idx, pos_target_idx (num_pos) and
 * neg_input_idx (num_neg): rows of the k * h * w RPN outputs and of gt_boxes (G, 4), as dc_forward_losses dumps them;
 * droi_boxes_or_null (num_pos + num_neg, 4), positives first: all DEVICE.  The sampler's backward COPIES: where several sampled
 * rows name one input row, the last one wins (negatives after positives).  The RPN's training forward runs through the same calls
 * as dc_forward_losses; the two mid losses (HOST doubles) and masked_mid (HOST) are what that call reports for these rows.
 * opts_or_null: batch_size and the two mid weights are read.  out->feat is the RPN's share of the feature map's gradient.
 * fp32 whatever dc_set_math_mode says, eager on lane 0, no float atomics (two identical calls give identical bits); settings and
 * weights are left as they were.  h and w are taken on trust, as dc_op_recog_grad takes them.  Synchronous.  DC_E_INVALID before
 * any launch: an index outside [0, k h w) or [0, G), num_pos + num_neg > 1024, a negative or non-finite box_reg_decay, a null
 * output, G outside 1..512, a ground-truth box that is not finite with w, h > 0, an image side below 32 px;
 * DC_E_UNSUPPORTED: h * w > 65536, or an rpn_hidden the engine's conv descriptor does not take (not a multiple of 32, above 2048). */
int dc_op_rpn_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const int32_t* pos_input_idx, const int32_t* pos_target_idx,
                   int num_pos, const int32_t* neg_input_idx, int num_neg, const float* gt_boxes, int G,
                   const float* droi_boxes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null, float box_reg_decay,
                   const dc_rpn_grads* out, double* mid_objectness_loss, double* mid_box_reg_loss, int32_t* masked_mid);
/* DenseCapModel:forward_backward with the reference's default -finetune_cnn_after -1: dc_loss_gradients (same arguments; out, rg
 * and lg are that call's bits), then dc_op_rpn_grad's backward on what the forward left on the device -- lane 0's feature map
 * and RPN hidden map, the RPN rows, the sampler's lists, the ground truth -- and rg->roi_boxes as droi_boxes.  pg: the six RPN tensors and feat (h, w, 512), the TOTAL
 * grad_cnn_features = rg->feat + the RPN's share, one fp32 add per element (LocalizationLayer.lua:550,581,601); rg->feat keeps RoI
 * pooling's share.  box_reg_decay: train_opts.lua's -box_reg_decay (5e-5 there).  With no sampled row the RPN gradients are the
 * decay term's alone.  Together the three structs hold the gradient of all five criteria and the decay with respect to all 21
 * tensors outside the CNN.  Not here: the CNN's backward (dc_forward_backward_cnn) and the optimiser (dc_train_step).
 * Synchronous. */
int dc_forward_backward(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                        const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                        dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg, float box_reg_decay,
                        const dc_rpn_grads* pg);
/* dc_forward_backward (same arguments; out, dump, rg, lg and pg are that call's bits) with conv_net2's activations kept by the
 * forward -- conv1_1 .. pool2 as ever, then dc_op_cnn_grad's forward on the pool2 map, whose conv5_3 map is the fused trunk's bit
 * for bit --, and then dc_op_cnn_grad's backward of pg->feat, the complete grad_cnn_features: cg, the 18 gradients of conv3_1 ..
 * conv5_3 (cg->x may be NULL).  DenseCapModel:forward_backward with model.finetune_cnn.  The refusals of dc_forward_backward and
 * of dc_op_cnn_grad, before anything is allocated or launched.  Not here: the optimiser (dc_train_step, dc_train_set_cnn).
 * Synchronous. */
int dc_forward_backward_cnn(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                            const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                            dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg,
                            float box_reg_decay, const dc_rpn_grads* pg, const dc_cnn_grads* cg);
/* ---- training step (docs/SEMANTICS.md, "Training step") ----
 * The other half of train.lua's loop body (train.lua:163-185) on the device: grad_params:add(weight_decay, params), then
 * adam(params, grad_params, learning_rate, beta1, beta2, epsilon) (optim_updates.lua:56-84) on the 21 tensors outside the CNN, in
 * place, in one launch.  train_opts.lua's defaults: 1e-5, 0.9, 0.999, 1e-8, weight_decay 1e-6. */
typedef struct dc_train_opts { double learning_rate, beta1, beta2, epsilon, weight_decay; } dc_train_opts;
/* Needs loaded weights (DC_E_STATE).  Allocates the two moments, zeroed, and a gradient arena for the 21 tensors (three times the
 * trained parameters' bytes; fc6's three live in the engine's (i, j, c) input order), makes an OIHW master of the RPN convolution,
 * sets t = 0.  DC_E_INVALID before anything is allocated: a negative or non-finite learning_rate, beta1 or beta2 outside [0, 1),
 * epsilon <= 0 or non-finite, a negative or non-finite weight_decay.  A second begin without dc_train_end: DC_E_STATE. */
int dc_train_begin(dc_ctx* ctx, const dc_train_opts* opts);
/* One iteration on one image: dc_forward_backward into the arena (same arguments, checked by the same checker; out and dump are
 * that call's bits for the weights as they were BEFORE the step), t += 1, the Adam launch, then every operand the library derives
 * from a trained weight is remade on the device (the list: DESIGN.md section 19), so that every later call -- forward, scoring,
 * sampling, either math mode, a captured graph: weight pointers do not move -- computes what a fresh ctx loaded with
 * dc_get_weights' arrays computes.  A refused step changes no weight and no t.  Before dc_train_begin: DC_E_STATE.  Dropout is
 * dc_set_dropout's, as in dc_forward_backward; the CNN is trained only after dc_train_set_cnn.  Eager on lane 0, synchronous. */
int dc_train_step(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                  const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                  dc_losses* out, const dc_loss_dump* dump, float box_reg_decay);
/* The CNN's share of the step, train.lua's -finetune_cnn_after (docs/SEMANTICS.md, "CNN gradients").  Valid between dc_train_begin
 * and dc_train_end (else DC_E_STATE); a mode outside 0..2: DC_E_INVALID.  mode 0, the default: dc_train_step is the step above,
 * bit for bit.  mode 1, the step train.lua takes at iter == finetune_cnn_after: the CNN's gradient is zero (model.finetune_cnn is
 * still false there), weight_decay * cnn_params is added and Adam steps on conv3_1 .. conv5_3 and their biases.  mode 2: the
 * step runs dc_forward_backward_cnn, then decay and Adam on those 18 tensors too.  The first non-zero mode allocates the OIHW
 * masters of the nine convolutions, zeroed moments and a gradient arena; the CNN has its own Adam step count, from 0, which
 * counts the steps taken in mode 1 or 2 only (cnn_optim_state, train.lua:115), with dc_train_begin's learning rate and betas, in
 * a second launch of the Adam kernel; the 21 other tensors' update is the same launch with the same bits in every mode.  After a
 * CNN step the nine packed convolutions and their split-bf16 planes are remade from the masters (pointers do not move).
 * conv1_1 .. conv2_2 are never trained.  dc_train_end frees this state too. */
int dc_train_set_cnn(dc_ctx* ctx, int mode);
/* Frees the moments, the arena and the master; the weights stay as trained.  Without a begin: DC_E_STATE. */
int dc_train_end(dc_ctx* ctx);
/* The current weights in the checkpoint's layouts: every non-null tensor pointer of `out` (HOST memory, the sizes of
 * dc_load_weights) is filled -- fc6 permuted back, the fused heads split, the packed convolutions unpacked; a null pointer is
 * skipped (conv_w[i] / conv_b[i] may be: the CNN is not trained).  The dimension fields and field_centers of `out` are ignored.
 * Straight after dc_load_weights it returns the loaded arrays bit for bit. */
int dc_get_weights(dc_ctx* ctx, const dc_weights* out);
/* The Adam kernel alone on caller-supplied DEVICE buffers of n floats as one segment: step t >= 1 of the update above; p, m and
 * v are updated in place, g is read only.  Any alignment (4-byte).  The same refusals for opts as dc_train_begin; n < 1 or
 * t < 1: DC_E_INVALID.  Synchronous. */
int dc_op_adam(dc_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, int t, const dc_train_opts* opts);
/* ---- gradient clipping (docs/SEMANTICS.md, "Gradient clipping") ----
 * Clipping by the global L2 norm of the gradient, between the backward and grad_params:add(weight_decay, params): sumsq = the sum
 * of (double)g * (double)g over every element the step's Adam launches read (the 21 tensors; in CNN mode 2 the CNN's 18 too: one
 * norm), norm = sqrt(sumsq), c = max_norm / (norm + 1e-6), scale = c < 1 ? (float)c : 1, and Adam reads g * scale (one rounded
 * fp32 multiply) in place of g; the arena is not rewritten and the scale never visits the host.  A sumsq that is not finite
 * gives scale = 1 and is reported as it is.  max_norm = +inf: the norm is computed and reported, scale is exactly 1.
 * max_norm = 0, the default (dc_train_begin resets it): off -- dc_train_step issues the launches and gives the bits it gives
 * without this call.  A negative or NaN max_norm: DC_E_INVALID.  Valid between dc_train_begin and dc_train_end, else DC_E_STATE. */
int dc_train_set_grad_clip(dc_ctx* ctx, double max_norm);
/* The norm and the scale of the last completed dc_train_step that ran with clipping on (either pointer may be null); a refused
 * step leaves them as they were.  No such step since dc_train_begin: DC_E_STATE. */
int dc_train_grad_norm(dc_ctx* ctx, double* norm, float* scale);
/* The two norm kernels alone on one caller-supplied DEVICE segment g of n floats, any alignment (4-byte): *sumsq, *norm and
 * *scale (HOST pointers, each may be null) by the rule above; max_norm = 0 leaves scale = 1.  n < 1, a null g, a negative or NaN
 * max_norm: DC_E_INVALID.  Two identical calls give identical bits.  Synchronous. */
int dc_op_grad_norm(dc_ctx* ctx, const float* g, size_t n, double max_norm, double* sumsq, double* norm, float* scale);
/* ---- Adam's state out and in (docs/SEMANTICS.md, "Training step") ----
 * dc_weights as dc_get_weights uses it: HOST pointers, tensors in the checkpoint's layouts (fc6 permuted back, the fused heads
 * split, lm_out_w the first V + 1 rows, rpn_conv_w OIHW), dimension fields ignored.  Both valid only between dc_train_begin and
 * dc_train_end (else DC_E_STATE).
 * get: every non-null pointer among the 21 trained tensors of m / v is filled with the first / second moment (m, v themselves
 * may be null); conv_w[4..12] / conv_b[4..12] with the CNN's moments -- non-null while no CNN state exists (no non-zero
 * dc_train_set_cnn yet): DC_E_STATE; conv_w[0..3], conv_b[0..3] and anchors must be null: DC_E_INVALID.  *t, *cnn_t (may be
 * null): the two step counts (cnn_t = 0 without CNN state). */
int dc_train_get_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int* t, int* cnn_t);
/* set: all 21 tensors are required in both m and v; conv_w[4..12] / conv_b[4..12] are given all 18 in both or not at all --
 * given, the CNN's state is allocated if need be as the first non-zero dc_train_set_cnn allocates it (the mode stays as it is);
 * not given, cnn_t must be 0.  conv_w[0..3], conv_b[0..3] and anchors must be null.  t >= 0, cnn_t >= 0.  Any breach:
 * DC_E_INVALID, and nothing is changed. */
int dc_train_set_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int t, int cnn_t);
/* The sampling of dc_sample_captions on given fc7 codes (n, fc_dim): samples (n, S, T), logprob (n, S).  row_ids (n) int32
 * >= 0 or NULL (= 0..n-1): the region row r of the noise counter for every code row, so that a subset of regions draws what
 * it draws in the full call.  Device pointers throughout (codes, row_ids, samples, logprob); synchronous. */
int dc_op_lm_sample_n(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                      int32_t* samples, float* logprob);
/* The sampling of dc_sample_captions_trunc on given fc7 codes: as dc_op_lm_sample_n, with sample_logprob (n, S) or NULL.
 * Device pointers throughout; synchronous. */
int dc_op_lm_sample_n_trunc(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                            const dc_sample_trunc* trunc_or_null, int32_t* samples, float* logprob,
                            float* sample_logprob_or_null);
/* The search of dc_beam_captions on given fc7 codes (n, fc_dim): captions (n, n_best, T), logprob (n, n_best).  Device pointers
 * throughout (codes, captions, logprob); synchronous.  A row's result does not depend on the other rows. */
int dc_op_lm_beam_n(dc_ctx* ctx, const float* codes, int n, const dc_beam_opts* opts, int32_t* captions, float* logprob);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_H */
