--[[
LuaJIT FFI binding of libdensecap_hip.so (C ABI: include/densecap.h).

This is the binding a maintainer of jcjohnson/densecap adds next to
densecap/DenseCapModel.lua.  It needs only LuaJIT (already required by Torch7);
no cutorch / cunn / cudnn.  NOTE: no Lua runtime exists in the build container,
so this file is written against the header and reviewed by inspection only; the
identical ABI is exercised from Python (densecap_amd/_lib.py), which is what
the parity tests and bench.py execute.
--]]
local ffi = require 'ffi'

ffi.cdef[[
typedef struct dc_ctx dc_ctx;
typedef struct dc_weights {
  const float* conv_w[13]; const float* conv_b[13];
  const float* rpn_conv_w; const float* rpn_conv_b;
  const float* rpn_box_w;  const float* rpn_box_b;
  const float* rpn_score_w; const float* rpn_score_b;
  const float* fc6_w; const float* fc6_b; const float* fc7_w; const float* fc7_b;
  const float* obj_w; const float* obj_b; const float* boxreg_w; const float* boxreg_b;
  const float* lm_enc_w; const float* lm_enc_b; const float* lm_emb;
  const float* lstm_w; const float* lstm_b; const float* lm_out_w; const float* lm_out_b;
  const float* anchors;
  float field_centers[4];
  int32_t num_anchors, rpn_hidden, vocab_size, seq_length, enc_size, rnn_size, fc_dim;
} dc_weights;
typedef struct dc_result {
  int32_t capacity, K, T;
  float* boxes; float* scores; int32_t* tokens;
} dc_result;
int dc_create(dc_ctx** out, int hip_device);
void dc_destroy(dc_ctx* ctx);
const char* dc_last_error(const dc_ctx* ctx);
int dc_load_weights(dc_ctx* ctx, const dc_weights* w);
int dc_set_test_args(dc_ctx* ctx, float rpn_nms_thresh, float final_nms_thresh, int num_proposals);
int dc_set_localization_test_args(dc_ctx* ctx, int clip_boxes, float nms_thresh, int max_proposals);
int dc_set_lanes(dc_ctx* ctx, int lanes);
int dc_set_caption_order(dc_ctx* ctx, int after_final_nms);
int dc_set_math_mode(dc_ctx* ctx, int mode);
int dc_set_graph_replay(dc_ctx* ctx, int on);
int dc_set_beam_size(dc_ctx* ctx, int beam_size);
int dc_set_group(dc_ctx* ctx, int images);
int dc_forward_test(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, dc_result* out);
int dc_score_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                      const int32_t* queries, int Q, int Tq, dc_result* out, float* loglik);
typedef struct dc_localize_opts { float nms_thresh; int32_t max_regions; float min_objectness; } dc_localize_opts;
int dc_localize_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                         const int32_t* queries, int Q, int Tq, const dc_localize_opts* opts, dc_result* out,
                         int32_t* count, float* boxes, float* loglik, float* objectness, int32_t* region);
int dc_op_nms_multi(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n, int Q,
                    float thresh, int max_picks, int32_t* picks, int32_t* counts);
int dc_op_eval_match(dc_ctx* ctx, const float* det_boxes, const float* det_scores, const int32_t* det_off,
                     const float* gt_boxes, const int32_t* gt_off, int n_images, float merge_thresh, int flags,
                     int32_t* order, double* ov, int32_t* group, uint8_t* ok,
                     int32_t* gt_group, int32_t* n_groups, double* merged_boxes);
typedef struct dc_loss_opts {
  int32_t batch_size; float high_thresh; float low_thresh; int32_t remove_outbounds;
  float mid_box_reg_weight; float mid_objectness_weight; float end_box_reg_weight; float end_objectness_weight;
  float captioning_weight; uint64_t seed;
} dc_loss_opts;
typedef struct dc_sampler_forced {
  const int32_t* pos_sample_idx; int32_t num_pos;
  const int32_t* neg_sample_idx; int32_t num_neg;
} dc_sampler_forced;
typedef struct dc_losses {
  double mid_objectness_loss; double mid_box_reg_loss; double end_objectness_loss; double end_box_reg_loss;
  double captioning_loss; double total_loss;
  int32_t num_pos; int32_t num_neg; int32_t total_pos; int32_t total_neg;
  int32_t masked_mid; int32_t masked_end;
  int32_t flags;
} dc_losses;
typedef struct dc_loss_dump { int32_t* pos_input_idx; int32_t* pos_target_idx; int32_t* neg_input_idx; } dc_loss_dump;
int dc_forward_losses(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts_or_null,
                      const dc_sampler_forced* forced_or_null, dc_losses* out, const dc_loss_dump* dump_or_null);
int dc_malloc(dc_ctx* ctx, void** dev_ptr, size_t bytes);
int dc_free(dc_ctx* ctx, void* dev_ptr);
int dc_memcpy_h2d(dc_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int dc_memcpy_d2h(dc_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
typedef struct dc_lm_grads {
  float* lm_enc_w; float* lm_enc_b; float* lm_emb; float* lstm_w; float* lstm_b; float* lm_out_w; float* lm_out_b; float* codes;
} dc_lm_grads;
int dc_op_lm_grad(dc_ctx* ctx, const float* codes, int n, const int32_t* labels, int L, float weight, const dc_lm_grads* out,
                  double* loss, double* rowlik_or_null);
int dc_op_roi_pool_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, int C, const float* boxes, int B, int img_h, int img_w,
                        int HH, int WW, const float* dout, float* dfeat, float* dboxes_or_null);
typedef struct dc_recog_grads {
  float* fc6_w; float* fc6_b; float* fc7_w; float* fc7_b; float* obj_w; float* obj_b; float* boxreg_w; float* boxreg_b; float* feat; float* roi_boxes;
} dc_recog_grads;
int dc_op_recog_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const float* roi_boxes, int n, int num_pos,
                     const float* target_boxes, const float* dcodes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null,
                     const dc_recog_grads* out, double* end_objectness_loss, double* end_box_reg_loss, int32_t* masked_end);
int dc_loss_gradients(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                      dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg);
int dc_feature_size(int H, int W, int* h, int* w);
int dc_op_conv3x3_grad(dc_ctx* ctx, const float* x, const float* w, const float* dy, int h, int w_px, int Cin, int Cout, float* dw,
                       float* db, float* dx);
int dc_op_maxpool2x2_grad(dc_ctx* ctx, const float* y, const float* dpool, int n, int H, int W, int C, float* dy);
int dc_op_relu_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats);
int dc_set_dropout(dc_ctx* ctx, float p);
int dc_get_dropout(dc_ctx* ctx, float* p);
int dc_op_dropout(dc_ctx* ctx, float* x, int rows, int cols, int layer, float p, uint64_t seed);
int dc_op_relu_dropout_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats, float p);
typedef struct dc_cnn_grads { float* conv_w[9]; float* conv_b[9]; float* x; } dc_cnn_grads;
typedef struct dc_cnn_dump { float* act[9]; float* prepool[2]; float* feat; float* dy[9]; } dc_cnn_dump;
int dc_op_cnn_grad(dc_ctx* ctx, const float* x4_hwc, int h4, int w4, const float* dfeat_hwc, const dc_cnn_grads* out,
                   const dc_cnn_dump* dump_or_null);
typedef struct dc_rpn_grads {
  float* rpn_conv_w; float* rpn_conv_b; float* rpn_box_w; float* rpn_box_b; float* rpn_score_w; float* rpn_score_b; float* feat;
} dc_rpn_grads;
int dc_op_rpn_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const int32_t* pos_input_idx, const int32_t* pos_target_idx,
                   int num_pos, const int32_t* neg_input_idx, int num_neg, const float* gt_boxes, int G,
                   const float* droi_boxes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null, float box_reg_decay,
                   const dc_rpn_grads* out, double* mid_objectness_loss, double* mid_box_reg_loss, int32_t* masked_mid);
int dc_forward_backward(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                        const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                        dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg, float box_reg_decay,
                        const dc_rpn_grads* pg);
int dc_forward_backward_cnn(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                            const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                            dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg,
                            float box_reg_decay, const dc_rpn_grads* pg, const dc_cnn_grads* cg);
typedef struct dc_train_opts { double learning_rate, beta1, beta2, epsilon, weight_decay; } dc_train_opts;
int dc_train_begin(dc_ctx* ctx, const dc_train_opts* opts);
int dc_train_set_cnn(dc_ctx* ctx, int mode);
int dc_train_step(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                  const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                  dc_losses* out, const dc_loss_dump* dump, float box_reg_decay);
int dc_train_end(dc_ctx* ctx);
int dc_get_weights(dc_ctx* ctx, const dc_weights* out);
int dc_op_adam(dc_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, int t, const dc_train_opts* opts);
int dc_train_set_grad_clip(dc_ctx* ctx, double max_norm);
int dc_train_grad_norm(dc_ctx* ctx, double* norm, float* scale);
int dc_op_grad_norm(dc_ctx* ctx, const float* g, size_t n, double max_norm, double* sumsq, double* norm, float* scale);
int dc_train_get_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int* t, int* cnn_t);
int dc_train_set_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int t, int cnn_t);
int dc_op_box_sampler(dc_ctx* ctx, const float* boxes, const float* gt, int A, int G, int img_h, int img_w,
                      const dc_loss_opts* opts, const dc_sampler_forced* forced_or_null, int32_t* pos_input_idx,
                      int32_t* pos_target_idx, int32_t* neg_input_idx, int32_t* counts, float* max_iou_or_null,
                      int32_t* arg_or_null);
typedef struct dc_sample_opts {
  int32_t num_samples; float temperature; uint64_t seed;
} dc_sample_opts;
int dc_sample_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                       dc_result* out, int32_t* samples, float* logprob);
int dc_op_lm_sample_n(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                      int32_t* samples, float* logprob);
typedef struct dc_sample_trunc { int32_t top_k; float top_p; } dc_sample_trunc;
int dc_sample_captions_trunc(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                             const dc_sample_trunc* trunc_or_null, dc_result* out, int32_t* samples, float* logprob,
                             float* sample_logprob_or_null);
int dc_op_lm_sample_n_trunc(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                            const dc_sample_trunc* trunc_or_null, int32_t* samples, float* logprob,
                            float* sample_logprob_or_null);
typedef struct dc_beam_opts { int32_t beam_size; int32_t n_best; float length_alpha; } dc_beam_opts;
int dc_beam_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_beam_opts* opts, dc_result* out,
                     int32_t* captions, float* logprob);
int dc_op_lm_beam_n(dc_ctx* ctx, const float* codes, int n, const dc_beam_opts* opts, int32_t* captions, float* logprob);
int dc_forward_batch(dc_ctx* ctx, const float* imgs, int n, int H, int W, int imgs_on_device, dc_result* outs);
int dc_forward_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                      dc_result* outs);
int dc_extract_features(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device,
                        int capacity, float* boxes, float* feats, int32_t* K);
int dc_extract_features_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n,
                               int imgs_on_device, int capacity, float* boxes, float* feats, int32_t* K);
typedef struct dc_box_list {
  const float* boxes; int32_t n; int32_t* src;
} dc_box_list;
int dc_forward_boxes(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_box_list* bl, int flags,
                     dc_result* out);
int dc_forward_boxes_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                            const dc_box_list* bl, int flags, dc_result* outs);
int dc_extract_features_boxes(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int imgs_on_device,
                              const dc_box_list* bl, int flags, int capacity, float* boxes, float* feats, int32_t* K);
int dc_preprocess_size(int H0, int W0, int image_size, int* H, int* W);
int dc_preprocess_u8(dc_ctx* ctx, const uint8_t* rgb_hwc, int H0, int W0, int on_device, int image_size, float* out_chw_dev,
                     uint8_t* scaled_rgb_dev);
int dc_stage_times(dc_ctx* ctx, const char** names, float* ms, int max_stages);
typedef struct dc_comm dc_comm;
int dc_comm_unique_id(void* id_out);
int dc_comm_create(dc_comm** out, dc_ctx* ctx, const void* id, int rank, int world);
int dc_comm_create_ex(dc_comm** out, dc_ctx* ctx, const void* id, int rank, int world, int flags);
const char* dc_comm_transport(const dc_comm* comm);
void dc_comm_destroy(dc_comm* comm);
const char* dc_comm_last_error(const dc_comm* comm);
int dc_gather_results(dc_comm* comm, const dc_result* local, int n_local, dc_result* gathered);
]]

local M = {}
M.C = ffi.load(os.getenv('DENSECAP_HIP_LIB') or 'densecap_hip')

function M.check(ctx, rc, what)
  if rc < 0 then
    error(string.format('%s failed (%d): %s', what or 'densecap_hip', rc,
                        ffi.string(M.C.dc_last_error(ctx))))
  end
  return rc
end

return M
