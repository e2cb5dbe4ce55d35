// libdensecap_hip.so -- C ABI (include/densecap.h) over the gfx950 kernels.
//
// A dc_ctx owns: the repacked weights, `lanes` (stream + workspace for one in-flight image,
// used to software-pipeline run_model.lua's image loop), and the per-stage HIP events.
// The whole forward of one image is enqueued on one stream without host round trips
// (box counts stay on the device); the host waits once, for the result copy.
#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <memory>

#include "common.h"
#include "scratch.h"

namespace {

thread_local std::string g_last_error;

struct VggItem { int cin, cout; bool pool_after; };
const VggItem kVgg[DC_NUM_VGG_CONVS] = {
    {3, 64, false},    {64, 64, true},    {64, 128, false},  {128, 128, true},  {128, 256, false},
    {256, 256, false}, {256, 256, true},  {256, 512, false}, {512, 512, false}, {512, 512, true},
    {512, 512, false}, {512, 512, false}, {512, 512, false}};  // no pool5 (DenseCapModel.lua:61-63)

enum Stage { ST_TRUNK = 0, ST_RPN, ST_NMS1, ST_ROIPOOL, ST_FC, ST_HEADS, ST_LSTM, ST_NMS2, ST_COUNT };
const char* kStageNames[ST_COUNT] = {"vgg16_trunk", "rpn_conv_heads_decode", "rpn_nms",   "bilinear_roi_pool",
                                     "fc6_fc7",     "recog_heads",           "lstm_decode", "final_nms_gather"};

struct DevBuf {          // (a lane's arena: lane_prepare and lane_release own it)
  void* p = nullptr;
  size_t bytes = 0;
};

// A ctx's settings: everything that reaches a kernel argument, a launch decision or the stream layout of a forward
// (enqueue_body, run_gemm).  A captured forward bakes all of it in, so GraphKey holds the whole struct.  4-byte fields only:
// graph keys compare it bytewise.
struct Settings {
  float rpn_nms_thresh = 0.7f, final_nms_thresh = 0.3f;
  int num_proposals = 300;          // LocalizationLayer default (LocalizationLayer.lua:237); run_model sets 1000
  int clip_boxes = 1;               // LocalizationLayer.test_clip_boxes (LocalizationLayer.lua:235)
  int captions_after_final_nms = 0; // dc_set_caption_order
  int serial_mode = 0;              // lanes == 1: idle CUs in a layer's last round are worth a tail split-K (dc_set_lanes)
  int beam_size = 0;                // 0 = greedy LM:sample; > 0 = LM:beamsearch (LanguageModel.lua:129-131)
  int math_mode = 0;                // dc_set_math_mode: 0 = fp32 MFMA (default), 1 = split-bf16 (three planes, six products, fp32 accumulate)
  // dc_debug_set (include/densecap_debug.h)
  int plan_mode = -1;               // -1 = planning follows the lane count, 0 = multi-lane planning, 1 = single-image planning
  int tail_mode = 0;                // partial last round in single-image mode: 0 stream-K, 1 K-split tail plan, 2 whole tiles
  int force_cfg = 0;                // measurement hook: tile configuration of plain launches
  int v2_stages = 0;                // LDS ring depth of the 128x64-tile kernel: 0 by tile count, 2 or 3 forced
  int stagger = 0;                  // measurement hook: start-up stagger of a launch's workgroups
  int walk = 0;                     // measurement hook: 128x64 launches as one workgroup per slot walking its tiles
  int epi_wide = 1;                 // plain interior epilogues as 16-byte stores staged through LDS
  int bf3_presplit = 1;             // 0 = split the weights in registers too (mode 1 of the kernels)
  int bf3_all = 0;                  // 1 = math mode 1 takes EVERY contraction, not only those mfma_gemm_bf3_pays names (test
                                    // hook: small and ragged problems then exercise the split-bf16 kernels)
  int nms_band = 1;                 // launch_nms `band`; dc_create reads the default from DC_NMS_BAND
  int decode_screen = -1;           // greedy decode step: 0 = fused fp32 step, 1 = bf16 screen + exact re-score, -1 = by row count (screen_pays)
  float dropout_p = 0.f;            // dc_set_dropout: the two nn.Dropout layers of the training forward (0 = none; never NaN, so bytewise
                                    // comparison holds); inference never reads it
  // contractions planned for one image alone (stream-K / tail plans over partial last rounds): images then travel alone
  bool serial_planning() const { return plan_mode < 0 ? serial_mode != 0 : plan_mode == 1; }
};
static_assert(sizeof(Settings) == 20 * 4, "Settings has 4-byte fields only (GraphKey compares it bytewise); a new field updates this count");

// Everything a captured forward bakes in: workspace pointers (carve epoch, arena, staging), weights, shape and the settings.
// Bytewise equality up to the end of `set`: 8-byte fields first, then 4-byte ones, so nothing in between is padding.
struct GraphKey {
  uint64_t carve_epoch = 0, weights_epoch = 0;
  const void *fault_dev = nullptr, *arena = nullptr, *host_stage = nullptr, *splitk_ws = nullptr;
  int H = 0, W = 0, P = 0, g = 0, features_only = 0, no_decode = 0;
  int box_src = 0, box_clip = 0;    // the RoI boxes are the caller's (dc_forward_boxes), clipped on the way in (DC_BOXES_CLIP)
  Settings set;
  bool operator==(const GraphKey& o) const { return memcmp(this, &o, offsetof(GraphKey, set) + sizeof(Settings)) == 0; }
};
static_assert(offsetof(GraphKey, set) == 6 * 8 + 8 * 4, "GraphKey is compared bytewise: no padding in front of `set`");

// Where one image's results go: its K rows (at most `capacity`) of boxes, scores and values -- tokens (T per row) or fc7
// codes (D per row, extractFeatures) -- and its K and T; `src` (a forward on caller-supplied boxes): the caller's row each
// result row came from.  Null pointers are skipped.
struct Dest {
  float *boxes = nullptr, *scores = nullptr;
  void* values = nullptr;
  int32_t *K = nullptr, *T = nullptr;
  int capacity = 0;
  int32_t* src = nullptr;
};

// Where a forward's RoI boxes come from: the RPN (bl == nullptr), or the caller -- image i's boxes are bl[i], validated by
// check_box_lists; `clip`: DC_BOXES_CLIP
struct BoxSource {
  const dc_box_list* bl = nullptr;
  bool clip = false;
};

// What a forward computes: boxes, scores and captions; boxes and fc7 codes (extractFeatures); boxes and scores only
enum Mode { MODE_RESULTS, MODE_FEATURES, MODE_NO_DECODE };

struct Lane {
  hipStream_t stream = nullptr;
  hipEvent_t ev[ST_COUNT + 1] = {};
  int H = 0, W = 0, P = 0;  // sizes the workspace is built for
  int G = 1;                // images the workspace holds side by side (group capacity)
  int g = 1;                // images of the group in flight
  int fh = 0, fw = 0, A = 0;
  DevBuf arena;               // one allocation, carved below
  float *img = nullptr, *act[2] = {nullptr, nullptr}, *feat = nullptr, *rpn_hidden = nullptr, *heads = nullptr;
  float *rpn_boxes = nullptr, *rpn_xyxy = nullptr, *rpn_p = nullptr;
  uint8_t* rpn_valid = nullptr;
  NmsWorkspace nms;
  void* nms_base = nullptr;
  int32_t *picks1 = nullptr, *count1 = nullptr, *picks2 = nullptr, *count2 = nullptr;
  float* in_boxes = nullptr;         // caller-supplied boxes of the group (P rows per image) and their counts, as copied in ...
  int32_t *in_n = nullptr, *box_src = nullptr;   // ... and the caller's row behind every row of roi_boxes (boxes_ingest_kernel)
  std::vector<int32_t> in_n_host;    // (source of the asynchronous copy to in_n)
  float *roi_boxes = nullptr, *roi_feats = nullptr, *fc6_out = nullptr, *codes = nullptr;
  float *obj = nullptr, *final_trans = nullptr, *final_boxes = nullptr, *final_xyxy = nullptr;
  float *enc = nullptr, *gates = nullptr, *hstate = nullptr, *cstate = nullptr, *logits = nullptr;
  uint16_t* scr_hb = nullptr;         // screened decode: bf16 h rows, their norms, candidate counts (row x step), winners' logits
  float *scr_hnorm = nullptr, *scr_best = nullptr;
  int32_t* scr_cand = nullptr;
  int32_t *tok = nullptr, *seq = nullptr;
  int32_t* surv_total = nullptr;   // captions after the final NMS: rows the group's final NMS runs kept, all images together
  float* out_feats = nullptr;
  char* out_pack = nullptr;     // the group's packed result records (final_pack_kernel), copied to host_stage in one piece
  float* splitk_ws = nullptr;   // split-K partial tiles (<= 256 tiles of 128x128)
  int32_t* out_tokens = nullptr;
  // pinned host staging
  void* host_stage = nullptr;
  size_t host_stage_bytes = 0;
  bool busy = false;
  const Dest* dst = nullptr;         // where the group in flight goes: dst[0..g)
  bool feats = false;                // ... and its records hold fc7 codes, not tokens
  bool boxes_in = false;             // ... computed on caller-supplied boxes (records carry rec_src; no RPN stages ran)
  float stage_ms[ST_COUNT] = {};
  bool have_times = false;
  // beam search scratch (allocated on first use; beam_chunk() proposals x beam rows at a time)
  void* beam_base = nullptr;
  int beam_rows = 0, beam_chunk = 0, beam_width = 0;   // what the scratch was carved for (rows = chunk x beam)
  float *bm_enc = nullptr, *bm_gates = nullptr, *bm_h[2] = {nullptr, nullptr}, *bm_c[2] = {nullptr, nullptr};
  float *bm_logits = nullptr, *bm_top_lp = nullptr, *bm_lp[2] = {nullptr, nullptr};
  int32_t *bm_top_idx = nullptr, *bm_beams[2] = {nullptr, nullptr}, *bm_parent = nullptr, *bm_tok = nullptr;
  uint8_t* bm_fin = nullptr;
  // what the standard search (dc_beam_captions) adds to it
  int32_t* bs_len[2] = {nullptr, nullptr};
  float* bs_pen = nullptr;
  hipStream_t aux = nullptr;            // single-image mode: second half of the decode rows runs here
  hipStream_t aux2 = nullptr;           // single-image mode: the final NMS runs here, beside the decode
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork2 = nullptr, ev_join2 = nullptr;
  // graph replay (dc_set_graph_replay): the forward of one (shape, settings) key, captured once and relaunched
  uint64_t carve_epoch = 0;             // bumped whenever lane_prepare hands out new workspace pointers
  hipGraphExec_t gexec = nullptr;
  GraphKey gkey, last_key;
  bool last_key_valid = false;          // last_key = the key of the previous (eager) forward on this lane
  bool ran_graph = false;               // the group in flight was a graph launch (no stage events)
  bool nms_before_decode = false;       // the group in flight ran the final NMS before the decode (dc_set_caption_order(1))
};

struct ProfEvt { hipEvent_t a, b; double flops; };

// The record of one training forward: train_forward fills it; the backward stages, the entry points' results and dc_debug_fetch
// "loss_*" read it.  The device rows live in ctx->loss_ws; feat, rpn_hidden and the n = np + nn sampled rows' activations in lane
// 0.  valid: cleared when a forward stage starts, set when it has completed.
struct TrainFwd {
  bool valid = false;
  float *boxes = nullptr, *anchors = nullptr, *trans = nullptr, *scores = nullptr, *gt = nullptr;   // (A,4) x 3, (A,2), (G,4)
  int32_t *pos_idx = nullptr, *pos_tgt = nullptr, *neg_idx = nullptr;                               // the sampler's lists
  double* rowlik = nullptr;                                                                         // (np)
  std::vector<int32_t> lists = std::vector<int32_t>(3 * 1024);      // host copies: pos_idx at 0, pos_tgt at 1024, neg_idx at 2048
  int32_t counts[8] = {0}, masked[2] = {0, 0};                      // the sampler's eight counts; loss_terms' two and its
  double terms[6] = {0};                                            // six doubles
  int A = 0, G = 0, np = 0, nn = 0, h = 0, w = 0, H = 0, W = 0;
  dc_loss_opts opts{};                                              // resolved (the defaults for a null pointer)
  float stage_ms[5] = {0, 0, 0, 0, 0};
  bool kept_feat = false;      // feat is ctx->cnn_feat (dc_forward_backward_cnn's trunk), not lane 0's
};

// The event split of a driver's last call: N events around its N - 1 stages, each made on first use and recorded on the call's
// stream; read() once the stream has drained.  The events die with the clock, that is with the ctx.
template <int N>
struct StageClock {
  hipEvent_t ev[N] = {};
  float ms[N - 1] = {};
  bool ran = false;              // read() has run: ms holds a call's times
  StageClock() = default;  StageClock(const StageClock&) = delete;     // (it owns its events)
  ~StageClock() { for (hipEvent_t e : ev) if (e != nullptr) (void)hipEventDestroy(e); }
  hipError_t record(int i, hipStream_t s) {
    if (ev[i] == nullptr)
      if (const hipError_t e = hipEventCreate(&ev[i]); e != hipSuccess) return e;
    return hipEventRecord(ev[i], s);
  }
  void read() {
    for (int i = 0; i + 1 < N; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    ran = true;
  }
};

}  // namespace

struct dc_ctx {
  int device = 0;
  std::string err;
  bool have_weights = false;
  Settings cfg;
  int max_lanes = 3;
  int group = 0;             // images per lane group (dc_set_group): 0 = default (1), 1 .. kGemmMaxGroup
  int arena_allocs = 0;      // lane workspace (re)allocations so far (dc_debug_fetch "arena_allocs")
  ScratchStats scratch;      // what the Scratch blocks of the calls and the KeptBufs below count (dc_debug_fetch "scratch")
  double host_enqueue_ms = 0;  // host ms per image spent enqueueing in the last forward call (run_images)
  int64_t beam_chunk_floats = (int64_t)1 << 28;   // cap of the beam search's full-logits buffer (dc_debug_set)
  int64_t score_rows_cap = 0;      // rows (region x query) one chunk of dc_score_captions / dc_op_lm_score may hold (dc_debug_set); 0 = ~512 MiB of scratch
  int64_t sample_rows_cap = 0;     // rows (region x draw) one chunk of dc_sample_captions / dc_op_lm_sample_n may hold (dc_debug_set); 0 = ~512 MiB of scratch
  uint32_t* fault_dev = nullptr;   // sticky device word: kFaultStreamK / kFaultNmsBand (common.h), checked with the results
  bool graphs = false;      // dc_set_graph_replay: repeated forwards of one shape are relaunched as a captured hipGraph
  uint64_t weights_epoch = 0;
  int graph_launches = 0, graph_captures = 0;    // dc_debug_fetch "graph_launches" / "graph_captures"
  std::string graph_note;                        // why replay was dropped, if it was (dc_debug_fetch "graph_replay_on" == 0)
  // dims
  int k = 0, R = 0, V = 0, T = 0, E = 0, Hd = 0, D = 0;
  float fc[4] = {0, 0, 0, 0};
  // device weights
  std::vector<void*> owned;
  float* conv_w[DC_NUM_VGG_CONVS] = {};
  float* conv_b[DC_NUM_VGG_CONVS] = {};
  float *rpn_w = nullptr, *rpn_b = nullptr, *heads_w = nullptr, *heads_b = nullptr;
  float *fc6_w = nullptr, *fc6_b = nullptr, *fc7_w = nullptr, *fc7_b = nullptr, *head5_w = nullptr, *head5_b = nullptr;
  float *enc_w = nullptr, *enc_b = nullptr, *wxT = nullptr, *whT = nullptr, *lstm_b = nullptr, *xg = nullptr;
  float *out_w = nullptr, *out_b = nullptr, *anchors = nullptr;
  float* dec_w = nullptr;   // (V1pad + 4Hd, Hd): rows [0,V+1) = lm_out_w, zero rows up to V1pad (multiple of 64), then Wh^T
  int V1pad = 0;
  // language-model gradients (lm_grad): the checkpoint-layout lstm_w (E+Hd, 4Hd) and lm_emb (V+2, E) as uploaded, and the two
  // transposed copies the data gradients need, made on the first gradient call after a dc_load_weights: out_wT (Hd, V1pad; zero
  // columns past V+1) and enc_wT (D, E).  lm_grad_clock: the event split of the last call (dc_debug_lm_grad_stage_ms).
  float *lstm_w_ck = nullptr, *emb = nullptr, *out_wT = nullptr, *enc_wT = nullptr;
  uint64_t grad_epoch = 0;
  StageClock<5> lm_grad_clock;
  // recognition-net gradients (recog_backward): fc7_wT (D, D) and fc6_wT (49*512, D), the transposed copies the data gradients
  // need, made on the first call after a dc_load_weights; the RoI index's scratch (grow only); the event split of the last call
  float *fc7_wT = nullptr, *fc6_wT = nullptr;
  uint64_t recog_epoch = 0;
  KeptBuf roi_grad_ws{scratch}, recog_ws{scratch}, recog_aux_ws{scratch};   // (recog_ws: the backward's scratch; recog_aux_ws: the callers' few rows)
  StageClock<5> recog_clock;
  // RPN gradients (rpn_backward): the RPN convolution's flipped, transposed weights, OIHW and in the engine's packed form (512,
  // 9R), made on first need and again when weights_epoch moves; the backward's scratch and the op's forward rows (grow only);
  // what the last backward left there for the hooks: its event split and the RPN's share of the feature map's gradient
  KeptBuf rpn_wf{scratch}, rpn_ws{scratch}, rpn_aux_ws{scratch};
  uint64_t rpn_epoch = 0;
  StageClock<5> rpn_clock;
  const float* rpn_dfeat = nullptr;
  int rpn_dfeat_pixels = 0;
  // CNN gradients (dc_op_cnn_grad): the activations the forward keeps for the backward and the backward's scratch (grow only);
  // the event split of the last call (kept forward, dump copies, backward; dc_debug_fetch "cnn_grad_ms")
  KeptBuf cnn_kept{scratch}, cnn_ws{scratch};
  KeptBuf train_cnn_kept{scratch};      // ... and the training forward's own kept activations (dc_forward_backward_cnn, the step)
  // the CNN's share of the training step (dc_train_set_cnn): mode, its own step count, the OIHW masters of the nine convolutions,
  // gradient arena and moments of the 18 tensors, the second Adam launch's segment table
  int train_cnn_mode = 0, train_cnn_t = 0, train_cnn_nseg = 0;
  unsigned long long train_cnn_chunks = 0;
  KeptBuf train_cnn_master{scratch}, train_cnn_g{scratch}, train_cnn_m{scratch}, train_cnn_v{scratch}, train_cnn_tab{scratch};
  const float *cnn_x4 = nullptr, *cnn_feat = nullptr;   // the last dc_forward_backward_cnn's kept pool2 map and conv5_3 map (dc_debug_fetch "cnn_x4" / "cnn_feat")
  int cnn_h4 = 0, cnn_w4 = 0;
  StageClock<4> cnn_clock;
  // screened greedy decode (Settings::decode_screen): bf16 copy of Wout (V1pad rows of scr_Kp, zero padded), the rows' 2-norms
  // rounded up to fp16 (V1pad of them), the constant c of the bound.  Part of the weights, made with dec_w.
  uint16_t* scr_w = nullptr;
  uint16_t* scr_wnorm = nullptr;
  float scr_c = 0.f;
  int scr_Kp = 0;
  // dc_debug_set "lm_op_keep": dc_op_lm_sample keeps its final state on the host for dc_debug_fetch "lm_op_*"
  bool lm_op_keep = false;
  std::vector<char> lm_op_h, lm_op_c, lm_op_scores, lm_op_cand, lm_op_best;
  // the last lm_sample_parts enqueued: its parts and which of them (bit i = part i) took the screened step;
  // dc_debug_fetch "decode_screen_routes".  A replayed graph keeps the routes of its capture.
  int lm_parts = 0;
  uint32_t lm_screened = 0;
  std::vector<std::unique_ptr<Lane>> lanes;
  // split-bf16 mode: weight matrices that can take it, and their bf16 planes (made when the mode is first switched on)
  struct PlaneEnt { const float* W; size_t rows; int K; uint16_t* planes; };
  std::vector<PlaneEnt> planes;
  KeptBuf pre_src{scratch}, pre_scratch{scratch};      // dc_preprocess_u8: uploaded bytes, width-pass plane (grow only)
  KeptBuf pre_taps{scratch};        // ... and the tap tables of the sizes in pre_key, kept while the sizes repeat (webcam frames)
  std::vector<char> pre_taps_host;  // (the host copy outlives its asynchronous upload)
  int pre_key[4] = {0, 0, 0, 0};    // H0, W0, oh, ow the tables were made for
  // the training forward: its scratch (grow only) and the record of the last one
  KeptBuf loss_ws{scratch};
  TrainFwd train;
  int32_t* row_ramp = nullptr;           // 0, 1 .. 1023 on the device, made on first need (dc_op_recog_grad's pos_target_idx)
  // the training step (dc_train_begin .. dc_train_end): the options and the step count; the gradient arena and the
  // two moments (one carve list, three blocks: train_arena_carve); the OIHW master of the RPN convolution; the feat / roi_boxes
  // outputs the stages insist on (grow only); the segment table on the device (optim_tab: dc_op_adam's and the hook's own);
  // the event split of the last step (backward, Adam launch, refresh; dc_debug_fetch "train_step_ms")
  bool training = false;
  bool fc6_grad_engine = false;          // recog_backward leaves fc6's weight gradient in the engine's (i, j, c) order (dc_train_step)
  dc_train_opts train_opts{};
  int train_t = 0;
  KeptBuf train_g{scratch}, train_m{scratch}, train_v{scratch}, train_master{scratch}, train_out{scratch}, train_tab{scratch};
  KeptBuf optim_tab{scratch};
  KeptBuf nms_debug_ws{scratch};         // dc_debug_nms's workspace (grow only: a call finds what the larger one before it left)
  int train_nseg = 0;
  unsigned long long train_chunks = 0;
  // gradient clipping (dc_train_set_grad_clip): max_norm (0 = off), the device block of the step's norm pass (the
  // record, then one double per chunk of the two tables), the last completed clipped step's record on the host
  double train_clip = 0;
  bool train_clip_have = false;
  GradNormRec train_clip_rec{};
  KeptBuf train_clip_buf{scratch};
  StageClock<4> train_clock;
  // MFMA profile
  bool prof = false;
  std::vector<ProfEvt> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  int64_t prof_launches = 0;
  double prof_ms = 0, prof_flops = 0;

  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    g_last_error = buf;
    return code;
  }
};

namespace {

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) return ctx->fail(DC_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                           __FILE__, __LINE__);                                      \
  } while (0)
#define DCCHK(expr)            \
  do {                         \
    int _r = (expr);           \
    if (_r != DC_OK) return _r; \
  } while (0)

#define KCHK(expr)                                                                                      \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return ctx->fail(DC_E_HIP, "%s: %s", #expr, hipGetErrorString(_e));           \
  } while (0)

int dev_alloc(dc_ctx* ctx, void** p, size_t bytes) {
  HIPCHK(hipMalloc(p, bytes ? bytes : 16));
  ctx->owned.push_back(*p);
  return DC_OK;
}
int upload(dc_ctx* ctx, float** dst, const float* host, size_t n) {
  if (!host) return ctx->fail(DC_E_INVALID, "dc_load_weights: null weight pointer");
  DCCHK(dev_alloc(ctx, reinterpret_cast<void**>(dst), n * sizeof(float)));
  HIPCHK(hipMemcpy(*dst, host, n * sizeof(float), hipMemcpyHostToDevice));
  return DC_OK;
}

hipEvent_t prof_event(dc_ctx* ctx) {
  if (!ctx->prof_pool.empty()) {
    hipEvent_t e = ctx->prof_pool.back();
    ctx->prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

// every MFMA contraction goes through here (optionally bracketed by HIP events).  `ws` (optional) is a
// scratch buffer of ws_floats floats on the same stream: problems with few tiles and a long K are split
// along K over several workgroups per tile and finished by a small reduce kernel.
// Scratch of one stream's contractions: partial tiles of split-K launches and tail plans, stream-K slots.
struct Ws {
  float* p = nullptr;
  size_t floats = 0;
};

// the ctx's sticky device fault word (stream-K owners and the NMS band scan report a hand-off that never arrived there; the
// packed results carry it to the host): made on first need, before any capture of the forward
static void ensure_fault_word(dc_ctx* ctx) {
  if (ctx->fault_dev == nullptr && hipMalloc(reinterpret_cast<void**>(&ctx->fault_dev), 64) == hipSuccess) {
    ctx->owned.push_back(ctx->fault_dev);
    (void)hipMemset(ctx->fault_dev, 0, 64);
  }
}

int run_gemm(dc_ctx* ctx, const GemmDesc& d_in, hipStream_t s, const Ws& w = Ws()) {
  float* const ws = w.p;
  const size_t ws_floats = w.floats;
  const Settings& c = ctx->cfg;
  GemmDesc d = d_in;
  d.stages = c.v2_stages;
  d.force_cfg = c.force_cfg;
  d.stagger = c.stagger;
  d.walk = c.walk;
  d.epi_wide = c.epi_wide;
  d.bf3 = c.math_mode == 1 && (c.bf3_all || mfma_gemm_bf3_pays(d)) ? 1 : 0;
  if (d.bf3 && c.bf3_presplit) {
    const uint16_t* pp = d_in.sk_slots != nullptr ? reinterpret_cast<const uint16_t*>(d_in.sk_slots) : nullptr;    // a caller's own planes (per-op entry points)
    int prow = d_in.sk_np;
    if (pp == nullptr)
      for (const auto& e : ctx->planes)
        if (e.W == d.W && e.K == d.K && e.planes != nullptr) { pp = e.planes; prow = (int)e.rows; break; }
    if (pp != nullptr) { d.bf3 = 2; d.sk_slots = reinterpret_cast<float*>(const_cast<uint16_t*>(pp)); d.sk_np = prow; }
  }
  if (d.bf3 != 2) { d.sk_slots = nullptr; d.sk_np = 0; }            // (a caller's planes mean nothing to the other routes)
  ProfEvt pe{nullptr, nullptr, gemm_flops(d)};
  if (ctx->prof) {
    pe.a = prof_event(ctx); pe.b = prof_event(ctx);
    (void)hipEventRecord(pe.a, s);
  }
  hipError_t e = hipSuccess;
  GemmPlan pl;                                                // mfma_gemm_plan decides; this function only acts on it
  mfma_gemm_plan(d, c.serial_planning(), c.tail_mode, ws != nullptr ? ws_floats : 0, &pl);
  const int m_split = pl.m_split;
  if (pl.kind == GEMM_PLAN_SPLITK) {
    // few tiles, long K: every tile is shared by `splitk` workgroups
    d.splitk = pl.splitk; d.splitk_ws = ws;
    e = launch_mfma_gemm(d, s);
    if (e == hipSuccess)
      e = d.pool ? launch_splitk_reduce_pool(ws, pl.splitk, d.bias, d.C, 0, d.M, d.N, d.ldc, d.H, d.Wd, d.relu, s)
                 : launch_splitk_reduce(ws, pl.splitk, d.bias, d.C, d.M, d.N, d.ldc, d.relu, s, d.m_dev);
  } else if (pl.kind == GEMM_PLAN_STREAMK) {
    // tile count not a multiple of the CU count: whole tiles for the full rounds, the last partial round shared evenly
    // along K by all CUs (stream-K with in-kernel fix-up: no reduce launch, one partial tile per cut)
    if (m_split > 0) {
      GemmDesc a = d;
      a.M = m_split; a.a_rows = d.M;
      e = launch_mfma_gemm_ks(a, s);
    }
    if (e == hipSuccess) {
      GemmDesc b = d;
      b.m_begin = m_split; b.a_rows = d.M;
      ensure_fault_word(ctx);
      b.sk_fault = ctx->fault_dev;
      e = launch_mfma_gemm_sk(b, pl.sk_wgs, pl.sk_np, ws, s);
    }
  } else if (pl.kind == GEMM_PLAN_TAIL) {
    // tile count not a multiple of the CU count: whole tiles for the full rounds, K-split for the last one
    const int tail_sp = pl.tail_splitk;
    if (m_split > 0) {
      GemmDesc a = d;
      a.M = m_split; a.a_rows = d.M;
      e = launch_mfma_gemm_ks(a, s);
    }
    if (e == hipSuccess) {
      GemmDesc b = d;
      b.m_begin = m_split; b.a_rows = d.M; b.splitk = tail_sp; b.splitk_ws = ws;
      e = launch_mfma_gemm_ks(b, s);
      if (e == hipSuccess)
        e = d.pool ? launch_splitk_reduce_pool(ws, tail_sp, d.bias, d.C, m_split, d.M - m_split, d.N, d.ldc, d.H, d.Wd, d.relu, s)
                   : launch_splitk_reduce(ws, tail_sp, d.bias, d.C + (size_t)m_split * d.ldc, d.M - m_split, d.N, d.ldc, d.relu, s);
    }
  } else {
    e = launch_mfma_gemm(d, s);
  }
  if (ctx->prof) {
    (void)hipEventRecord(pe.b, s);
    ctx->prof_pending.push_back(pe);
  }
  if (e != hipSuccess)
    return ctx->fail(DC_E_HIP, "mfma gemm launch failed: %s (M=%d N=%d K=%d conv=%d)", hipGetErrorString(e), d.M,
                     d.N, d.K, d.conv);
  return DC_OK;
}
void prof_collect(dc_ctx* ctx) {
  for (auto& pe : ctx->prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
      ctx->prof_ms += ms;
      ctx->prof_flops += pe.flops;
      ctx->prof_launches += 1;
    }
    ctx->prof_pool.push_back(pe.a);
    ctx->prof_pool.push_back(pe.b);
  }
  ctx->prof_pending.clear();
}

int fail_on_fault(dc_ctx* ctx, uint32_t fault, const char* who);
// the fault word after a synchronised per-op call
int check_fault_word(dc_ctx* ctx, const char* who) {
  if (ctx->fault_dev == nullptr) return DC_OK;
  uint32_t f = 0;
  if (hipMemcpy(&f, ctx->fault_dev, 4, hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(DC_E_HIP, "%s: fault word read failed", who);
  return f == 0 ? DC_OK : fail_on_fault(ctx, f, who);
}
// How a synchronous call that enqueued on `s` ends, with rc the status of what it enqueued: drain, collect the MFMA profile,
// then report -- rc first, the drain's error next and (fault: the calls that check it) the fault word last.  A Scratch the
// caller holds is still alive here: what the call copies out of it goes between this and its return.
int call_finish(dc_ctx* ctx, hipStream_t s, int rc, const char* who, bool fault = false) {
  const hipError_t e = hipStreamSynchronize(s);
  prof_collect(ctx);
  if (rc != DC_OK) return rc;
  if (e != hipSuccess) return ctx->fail(DC_E_HIP, "%s: %s", who, hipGetErrorString(e));
  return fault ? check_fault_word(ctx, who) : DC_OK;
}

// `planes` (optional): the caller's own bf16 planes of W for the split-bf16 mode (per-op entry points; the model's weights
// are looked up in ctx->planes)
int linear(dc_ctx* ctx, hipStream_t s, const float* A, const float* W, const float* bias, float* C, int M, int N,
           int K, int relu, const Ws& ws = Ws(), int plan_M = 0, const uint16_t* planes = nullptr) {
  GemmDesc d;
  d.A = A; d.W = W; d.bias = bias; d.C = C; d.M = M; d.N = N; d.K = K; d.ldc = N; d.relu = relu; d.plan_M = plan_M;
  d.sk_slots = reinterpret_cast<float*>(const_cast<uint16_t*>(planes)); d.sk_np = planes ? N : 0;
  return run_gemm(ctx, d, s, ws);
}
int conv3x3(dc_ctx* ctx, hipStream_t s, const float* in, const float* w, const float* b, float* out, int nimg, int H,
            int W, int Cin, int Cout, int relu, const Ws& ws = Ws(), const uint16_t* planes = nullptr) {
  GemmDesc d;
  d.sk_slots = reinterpret_cast<float*>(const_cast<uint16_t*>(planes)); d.sk_np = planes ? Cout : 0;
  d.A = in; d.W = w; d.bias = b; d.C = out; d.M = nimg * H * W; d.N = Cout; d.K = 9 * Cin; d.ldc = Cout;
  d.relu = relu; d.conv = 1; d.H = H; d.Wd = W; d.Cin = Cin; d.plan_M = H * W;
  return run_gemm(ctx, d, s, ws);
}
// conv3x3 + ReLU + nn.SpatialMaxPooling(2,2,2,2):ceil() (VGG layers conv1_2, conv2_2, conv3_3, conv4_3,
// DenseCapModel.lua:61-76): the pool rides in the conv's epilogue -- the full-resolution activation never reaches HBM
// (conv1_2: 110 MB store -> 28 MB) and four launches disappear.  out: (ceil(H/2), ceil(W/2), Cout).
int conv3x3_pool(dc_ctx* ctx, hipStream_t s, const float* in, const float* w, const float* b, float* out, int nimg, int H,
                 int W, int Cin, int Cout, int relu, const Ws& ws, const uint16_t* planes = nullptr) {
  GemmDesc d;
  d.sk_slots = reinterpret_cast<float*>(const_cast<uint16_t*>(planes)); d.sk_np = planes ? Cout : 0;
  const int slots = 4 * ((H + 1) / 2) * ((W + 1) / 2);          // window slots of one image
  d.A = in; d.W = w; d.bias = b; d.C = out; d.M = nimg * slots; d.N = Cout; d.K = 9 * Cin; d.plan_M = slots;
  d.ldc = Cout; d.relu = relu; d.conv = 1; d.H = H; d.Wd = W; d.Cin = Cin; d.pool = 1;
  if (!mfma_gemm_can_pool(d))
    return ctx->fail(DC_E_UNSUPPORTED, "conv3x3_pool: %dx%dx%d activation exceeds the kernels' 32-bit operand offsets", H, W, Cin);
  return run_gemm(ctx, d, s, ws);
}

// num_proposals = -1 (LocalizationLayer.lua:322-324: uncapped RPN NMS): capacity = every anchor of this image size
int effective_proposals(const dc_ctx* ctx, int H, int W);
constexpr size_t kSplitkWsFloats = (size_t)6400 * 128 * 128;  // 400 MiB per lane: split-K partial outputs (up to 8 x an eight-image group's 8 x 384 x 4096 fc6 rows), tail plans, stream-K slots

Ws lane_ws(const Lane& L) { return Ws{L.splitk_ws, L.splitk_ws ? kSplitkWsFloats : 0}; }

int effective_proposals(const dc_ctx* ctx, int H, int W) {
  if (ctx->cfg.num_proposals != -1) return ctx->cfg.num_proposals;
  int fh = H, fw = W;
  for (int i = 0; i < DC_NUM_VGG_CONVS; ++i)
    if (kVgg[i].pool_after) { fh = (fh + 1) / 2; fw = (fw + 1) / 2; }
  return ctx->k * fh * fw;
}

// bytes of one image's packed result record: tokens, or fc7 codes (extractFeatures)
// (with_src: a forward on caller-supplied boxes, one more word per row)
size_t pack_words(const dc_ctx* ctx, bool feats) { return feats ? ctx->D : ctx->T; }
size_t pack_stride(const dc_ctx* ctx, int P, bool feats, bool with_src = false) { return rec_stride(P, pack_words(ctx, feats) + (with_src ? 1 : 0)); }
// bytes per image of a lane's record buffers (out_pack, host_stage), which hold any kind (T + D >= max(T, D) + 1)
size_t host_stage_stride(const dc_ctx* ctx, int P) { return rec_stride(P, (size_t)ctx->T + ctx->D); }

// A lane's streams and events, made on first use.
int lane_streams(dc_ctx* ctx, Lane& L) {
  if (L.stream != nullptr) return DC_OK;
  HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&L.aux, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&L.aux2, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&L.ev_fork2, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&L.ev_join2, hipEventDisableTiming));
  for (auto& e : L.ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventCreateWithFlags(&L.ev_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&L.ev_join, hipEventDisableTiming));
  return DC_OK;
}

// Everything a lane owns, released (the device is idle).
void lane_release(Lane& L) {
  if (L.arena.p) (void)hipFree(L.arena.p);
  if (L.beam_base) (void)hipFree(L.beam_base);
  if (L.gexec) (void)hipGraphExecDestroy(L.gexec);
  if (L.host_stage) (void)hipHostFree(L.host_stage);
  for (auto& ev : L.ev) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {L.ev_fork, L.ev_join, L.ev_fork2, L.ev_join2}) if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : {L.aux, L.aux2, L.stream}) if (st) (void)hipStreamDestroy(st);
}

// floats per row of the buffer that holds, by route, a row's full logits, its arg-max partials or its fp16 screen scores
size_t lm_amax_floats(const dc_ctx* ctx) { return (size_t)std::max(std::max(ctx->V + 1, ctx->V1pad / 16), ctx->V1pad / 2); }

// (Re)build a lane's workspace for G images of size (H,W) side by side and proposal capacity P each.
int lane_prepare(dc_ctx* ctx, Lane& L, int H, int W, int P, int G) {
  DCCHK(lane_streams(ctx, L));
  if (L.H == H && L.W == W && L.P == P && L.G == G && L.arena.p) return DC_OK;
  int fh = H, fw = W;
  for (int i = 0; i < DC_NUM_VGG_CONVS; ++i)
    if (kVgg[i].pool_after) { fh = (fh + 1) / 2; fw = (fw + 1) / 2; }
  const int A = ctx->k * fh * fw;
  const int Tn = ctx->T, Dm = ctx->D, E = ctx->E, Hd = ctx->Hd;
  const int nms_n = std::max(A, P);
  const size_t act_bytes = (size_t)G * H * W * 64 * sizeof(float);
  const size_t GP = (size_t)G * P;          // rows of the per-RoI tensors: image i owns rows [i*P, (i+1)*P)
  const std::vector<Carve> cv = {
      {(void**)&L.img, (size_t)G * 3 * H * W * 4},
      {(void**)&L.act[0], act_bytes},
      {(void**)&L.act[1], act_bytes},
      {(void**)&L.rpn_hidden, (size_t)G * fh * fw * ctx->R * 4},
      {(void**)&L.heads, (size_t)G * fh * fw * 6 * ctx->k * 4},
      {(void**)&L.rpn_boxes, (size_t)G * A * 16},
      {(void**)&L.rpn_xyxy, (size_t)G * A * 16},
      {(void**)&L.rpn_p, (size_t)G * A * 4},
      {(void**)&L.rpn_valid, (size_t)G * A},
      {(void**)&L.nms_base, nms_workspace_bytes(nms_n)},          // one: the images' NMS runs follow each other on the stream
      {(void**)&L.picks1, GP * 4},
      {(void**)&L.count1, (size_t)G * kCountStride * 4},
      {(void**)&L.picks2, GP * 4},
      {(void**)&L.count2, (size_t)G * kCountStride * 4},
      {(void**)&L.surv_total, 256},
      {(void**)&L.in_boxes, GP * 16},
      {(void**)&L.in_n, (size_t)G * 4},
      {(void**)&L.box_src, GP * 4},
      {(void**)&L.roi_boxes, GP * 16},
      {(void**)&L.roi_feats, GP * 49 * 512 * 4},
      {(void**)&L.fc6_out, GP * Dm * 4},
      {(void**)&L.codes, GP * Dm * 4},
      {(void**)&L.obj, GP * 4},
      {(void**)&L.final_trans, GP * 16},
      {(void**)&L.final_boxes, GP * 16},
      {(void**)&L.final_xyxy, GP * 16},
      {(void**)&L.enc, GP * E * 4},
      {(void**)&L.gates, GP * 4 * Hd * 4},
      {(void**)&L.hstate, GP * Hd * 4},
      {(void**)&L.cstate, GP * Hd * 4},
      {(void**)&L.logits, GP * lm_amax_floats(ctx) * 4},   // full logits (beam), 2 x V1pad/32 arg-max partials or V1pad fp16 scores per row
      {(void**)&L.scr_hb, GP * (size_t)ctx->scr_Kp * 2},
      {(void**)&L.scr_hnorm, GP * 4},
      {(void**)&L.scr_best, GP * 4},
      {(void**)&L.scr_cand, GP * Tn * 4},
      {(void**)&L.tok, GP * 4},
      {(void**)&L.seq, GP * Tn * 4},
      {(void**)&L.out_pack, (size_t)G * host_stage_stride(ctx, P)},   // packed result records of the group (either kind)
      {(void**)&L.out_tokens, GP * Tn * 4},
      {(void**)&L.out_feats, GP * Dm * 4},
      {(void**)&L.splitk_ws, kSplitkWsFloats * 4},
  };
  const size_t total = carve(cv, nullptr);
  // The arena only grows: a directory of mixed sizes (720x480, 720x540, 480x720 ... the normal case for
  // run_model -input_dir) re-carves the existing allocation instead of a free + malloc of ~0.5 GB per image.
  if (L.arena.p == nullptr || total > L.arena.bytes) {
    if (L.arena.p) {
      HIPCHK(hipStreamSynchronize(L.stream));
      HIPCHK(hipFree(L.arena.p));
      L.arena = DevBuf();
    }
    HIPCHK(hipMalloc(&L.arena.p, total));
    L.arena.bytes = total;
    ctx->arena_allocs += 1;
  }
  carve(cv, L.arena.p);
  L.carve_epoch += 1;                  // every captured pointer is stale now
  nms_workspace_bind(L.nms, L.nms_base, nms_n);
  const size_t hs = (size_t)G * host_stage_stride(ctx, P);
  if (L.host_stage_bytes < hs) {
    if (L.host_stage) HIPCHK(hipHostFree(L.host_stage));
    HIPCHK(hipHostMalloc(&L.host_stage, hs, hipHostMallocDefault));
    L.host_stage_bytes = hs;
  }
  L.H = H; L.W = W; L.P = P; L.G = G; L.fh = fh; L.fw = fw; L.A = A;
  return DC_OK;
}


// One contiguous block of decode rows and the stream it runs on.  LSTM rows are independent, so a batch may be cut
// into blocks that advance on different streams: every row sees exactly the same arithmetic (the K order of a GEMM
// element does not depend on the tile it falls in), only the kernels of the blocks overlap in time.
struct LmPart { hipStream_t s; int r0, n; Ws ws; };

// The buffers of one greedy decode, one row per code row: encoder output (E), gate pre-activations (4 Hd), LSTM state (Hd
// each) and the step GEMM's arg-max partials (2 x V1pad/32).  The forward passes its lane's, dc_op_lm_sample a carve of its own.
// Screened route: amax holds the rows' fp16 scores instead (V1pad each); hb, hnorm, cand, best as in RescoreTail.
// A part that starts at row r0 owns amax from r0 * lm_part_stride floats on BOTH routes: the route is chosen per part, and
// parts on different streams run at the same time, so a screened and a fused part must not share a byte.
struct LmBufs { float *enc, *gates, *h, *c, *amax; uint16_t* hb; float* hnorm; int32_t* cand; float* best; };
LmBufs lane_lm_bufs(const Lane& L) { return LmBufs{L.enc, L.gates, L.hstate, L.cstate, L.logits, L.scr_hb, L.scr_hnorm, L.scr_cand, L.scr_best}; }

// Whether `rows` decode rows of one launch take the screened step (Settings::decode_screen).  Greedy decode in fp32 mode only;
// the row tail keeps a row of h in LDS.  The rule of -1 is measured: the screen wins from a few hundred rows.
size_t lm_part_stride(const dc_ctx* ctx) { return (size_t)ctx->V1pad / 2; }   // floats per row: V1pad fp16 scores >= 2 x V1pad/32 partials
static_assert(sizeof(_Float16) * 2 == sizeof(float), "lm_part_stride counts a row of fp16 scores in floats");
constexpr int kScreenMinRows = 400;
// (the part of the rule that depends on the loaded dimensions alone: the test hooks of the route's kernels ask for it)
bool screen_fits(const dc_ctx* ctx) { return screen_tail_lds_bytes(ctx->Hd, ctx->V1pad) <= kScreenTailMaxLds; }
bool screen_pays(const dc_ctx* ctx, int rows) {
  const Settings& c = ctx->cfg;
  if (c.math_mode != 0 || c.decode_screen == 0 || !screen_fits(ctx)) return false;
  return c.decode_screen == 1 || rows >= kScreenMinRows;
}

// From fc7 codes to the state after the START token: the first five launches of the schedule in lm_sample_parts (there is the
// description), for n rows.  Every schedule of the language model but the reference-rule beam search starts here.  Only enqueues
// (capture-safe).  `plan`: GemmDesc::plan_M; m_dev: optional device-side row count; enc_ws: scratch of the encoder GEMM
// (K = 4096), the only one of the three that may take a split-K route.
int lm_start_state(dc_ctx* ctx, hipStream_t s, const float* codes, int n, float* enc, float* gates, float* c, float* h, int plan,
                   const int32_t* m_dev, const Ws& enc_ws) {
  const int E = ctx->E, Hd = ctx->Hd, V1 = ctx->V + 1;
  GemmDesc g;                // image_encoder: Linear(4096,E)+ReLU (:27-30)
  g.A = codes; g.W = ctx->enc_w; g.bias = ctx->enc_b; g.C = enc; g.M = n; g.N = E; g.K = ctx->D; g.ldc = E; g.relu = 1;
  g.m_dev = m_dev; g.plan_M = plan;
  DCCHK(run_gemm(ctx, g, s, enc_ws));
  g = GemmDesc();            // step 0: gates = (b + enc.Wx) + 0.Wh ; c0 = 0 (output ignored, no vocab projection needed)
  g.A = enc; g.W = ctx->wxT; g.bias = ctx->lstm_b; g.C = gates; g.M = n; g.N = 4 * Hd; g.K = E; g.ldc = 4 * Hd;
  g.m_dev = m_dev; g.plan_M = plan;
  DCCHK(run_gemm(ctx, g, s));
  KCHK(launch_lstm_step_tail(nullptr, nullptr, 0, 0, 0, nullptr, gates, c, h, n, m_dev, Hd, 1, nullptr, 1, 0, s));
  g = GemmDesc();            // h_0.Wh, then the START token's xg row (:32,320) joins it in the tail
  g.A = h; g.W = ctx->whT; g.C = gates; g.M = n; g.N = 4 * Hd; g.K = Hd; g.ldc = 4 * Hd; g.m_dev = m_dev; g.plan_M = plan;
  DCCHK(run_gemm(ctx, g, s));
  KCHK(launch_lstm_step_tail(nullptr, nullptr, 0, 0, V1, ctx->xg, gates, c, h, n, m_dev, Hd, 0, nullptr, 1, 0, s));
  return DC_OK;
}

// The GEMM of one decode step on `rows` rows of h: the vocabulary projection, whose epilogue reduces every row to partials
// (the logits never reach HBM), and -- except after the last step -- in the same launch G = h.Wh for the next step's gates
// (W = [Wout; pad; Wh]).  The caller adds the fields of its epilogue: amax_val / amax_idx / amax_ld, rowidx, samp_*.
GemmDesc decode_step_desc(const dc_ctx* ctx, const float* h, int rows, int plan, bool last, float* gates) {
  const int V1 = ctx->V + 1, Hd = ctx->Hd;
  GemmDesc v;
  v.A = h; v.W = ctx->dec_w; v.bias = ctx->out_b; v.M = rows; v.K = Hd; v.plan_M = plan;
  if (last) {
    v.N = V1; v.ldc = V1;
  } else {
    v.N = ctx->V1pad + 4 * Hd; v.amax_cols = ctx->V1pad; v.amax_n = V1; v.C = gates; v.ldc = 4 * Hd;
  }
  return v;
}

// LanguageModel:sample greedy decode (LanguageModel.lua:293-348) for the rows of `codes` covered by `parts`, on the buffers `b`
// (n_dev: optional device-side row count <= n of a single part starting at row 0; rows past it are not computed).
int lm_sample_parts(dc_ctx* ctx, const LmBufs& b, const float* codes, const LmPart* parts, int nparts, const int32_t* n_dev,
                    int32_t* seq_out, int plan = 0) {
  // Schedule of one decode (h_t = LSTM state after t steps past the image step, tok_0 = START):
  //   enc = ReLU(codes.Wenc^T + b)                      GEMM   (:27-30)
  //   G   = (b + enc.Wx)                                GEMM   step 0 of LM:sample: the image code is the first input
  //   tail: c_0, h_0 from G (c = 0)                     row kernel
  //   G   = h_0.Wh                                      GEMM
  //   tail: h_1 from xg[START] + G                      row kernel
  //   for t = 1..T-1:  [arg-max partials of h_t.Wout^T + b | G = h_t.Wh]   ONE GEMM launch (W = [Wout; pad; Wh])
  //                    tail: tok_t = arg-max; h_{t+1} from xg[tok_t] + G   row kernel
  //   arg-max partials of h_T.Wout^T + b                GEMM;  tail: tok_T
  // Launches of screen_pays() rows run the screened step instead, 3 launches:
  //                    s = fp16(bf16(h_t).bf16(Wout)^T + b)                  bf16 screen, every column
  //                    G = h_t.Wh                                            GEMM (not after the last step)
  //                    tail: tok_t = arg-max of the EXACT fp32 logits of the columns s cannot rule out; h_{t+1}; bf16(h_{t+1}), |h_{t+1}|
  // Otherwise 2 launches per step.  The h.Wh product of the NEXT step rides in the vocabulary projection's launch (both
  // only need h_t) and fills its partial last round of tiles; the token-dependent half of the gates (a row of the
  // precomputed xg = b + Emb.Wx table) is added where the token is produced.  Per element the arithmetic and its order
  // are those of torch-rnn's nn.LSTM: (b + x.Wx) + h.Wh, sigmoid/tanh, c' = f*c + i*g, h' = o*tanh(c').
  // The first five lines are lm_start_state, the GEMM of a step is decode_step_desc: lm_score and lm_sample_n share both.
  const int E = ctx->E, Hd = ctx->Hd, T = ctx->T, D = ctx->D;
  const int ntn = ctx->V1pad / 32;       // arg-max partials per row: one (value, column) per 32-column half of a 64-column tile
  if (nparts > 32) return ctx->fail(DC_E_INVALID, "lm_sample_parts: at most 32 parts");
  ctx->lm_parts = nparts; ctx->lm_screened = 0;
  for (int pi = 0; pi < nparts; ++pi)
    if (screen_pays(ctx, parts[pi].n)) ctx->lm_screened |= 1u << pi;
  for (int pi = 0; pi < nparts; ++pi) {
    const LmPart& p = parts[pi];
    const size_t r0 = p.r0;
    DCCHK(lm_start_state(ctx, p.s, codes + r0 * D, p.n, b.enc + r0 * E, b.gates + r0 * 4 * Hd, b.c + r0 * Hd, b.h + r0 * Hd,
                         plan, n_dev, p.ws));
  }
  for (int t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    for (int pi = 0; pi < nparts; ++pi) {
      const LmPart& p = parts[pi];
      const size_t r0 = p.r0;
      float* gates = b.gates + r0 * 4 * Hd;
      float* hstate = b.h + r0 * Hd;
      float* amax = b.amax + r0 * lm_part_stride(ctx);      // the part's own region, whichever route it takes
      if (ctx->lm_screened >> pi & 1) {
        // screened step: bf16 scores of every column, h_t.Wh on the fp32 family (as lm_start_state forms h_0.Wh: the same bits
        // as the fused launch's, the K order of an element does not depend on the launch), then the re-scoring tail
        const int Kp = ctx->scr_Kp, V1pad = ctx->V1pad;
        uint16_t* hb = b.hb + r0 * Kp;
        _Float16* scores = reinterpret_cast<_Float16*>(amax);
        if (t == 0) KCHK(launch_screen_operands(hstate, p.n, n_dev, Hd, Kp, hb, b.hnorm + r0, p.s));
        KCHK(launch_decode_screen(hb, ctx->scr_w, ctx->out_b, scores, p.n, n_dev, ctx->V + 1, V1pad, Kp, p.s));
        if (!last) {
          GemmDesc g;
          g.A = hstate; g.W = ctx->whT; g.C = gates; g.M = p.n; g.N = 4 * Hd; g.K = Hd; g.ldc = 4 * Hd; g.m_dev = n_dev; g.plan_M = plan;
          DCCHK(run_gemm(ctx, g, p.s));
        }
        RescoreTail a{};
        a.scores = scores; a.ld = V1pad; a.wnorm = reinterpret_cast<const _Float16*>(ctx->scr_wnorm); a.W = ctx->out_w; a.bias = ctx->out_b; a.V1 = ctx->V + 1;
        a.cbound = ctx->scr_c; a.xg = ctx->xg; a.gates_pre = last ? nullptr : gates; a.c = b.c + r0 * Hd; a.h = hstate;
        a.n = p.n; a.n_dev = n_dev; a.Hd = Hd; a.seq = seq_out + r0 * T; a.T = T; a.t = t;
        a.hb = hb; a.Kp = Kp; a.hnorm = b.hnorm + r0; a.cand = b.cand + r0 * T; a.bestv = b.best + r0;
        KCHK(launch_lstm_rescore_tail(a, p.s));
        continue;
      }
      GemmDesc v = decode_step_desc(ctx, hstate, p.n, plan, last, gates);     // epilogue: the row arg-max
      v.m_dev = n_dev;
      v.amax_val = amax;
      v.amax_idx = reinterpret_cast<int32_t*>(v.amax_val + (size_t)p.n * ntn);
      v.amax_ld = ntn;
      DCCHK(run_gemm(ctx, v, p.s));
      KCHK(launch_lstm_step_tail(v.amax_val, v.amax_idx, ntn, ntn, 0, ctx->xg, last ? nullptr : gates, b.c + r0 * Hd, hstate,
                                 p.n, n_dev, Hd, 0, seq_out + r0 * T, T, t, p.s));
    }
  }
  return DC_OK;
}

// `plan`: rows of one image when n covers a group (0 = n); see GemmDesc::plan_M
int lm_sample(dc_ctx* ctx, hipStream_t s, const LmBufs& b, const Ws& ws, const float* codes, int n, int plan, const int32_t* n_dev,
              int32_t* seq_out) {
  const LmPart whole{s, 0, n, ws};
  return lm_sample_parts(ctx, b, codes, &whole, 1, n_dev, seq_out, plan);
}
// ---- beam search: both rules ----------------------------------------------------------------------------------------------------
// Reference rule: LanguageModel:beamsearch (LanguageModel.lua:170-290), dispatched by LM:updateOutput when self.beam_size is set
// (:129-131; no reference script sets it).  The reference walks the proposals one by one with the beams in the
// minibatch dimension; here ALL proposals advance together (rows = proposals x beams; beam_chunk), row for row the same
// arithmetic: LSTM step (MFMA GEMM + point-wise), vocabulary projection (full logits this time), LogSoftMax + top-k per
// beam, beam x beam merge, states re-indexed by parent.  Ties: lower index first (docs/SEMANTICS.md).
// Standard search (docs/SEMANTICS.md, "Standard beam search"): the same dense steps, lists and state gather; what
// differs is how the first state is formed, the bookkeeping kernel between the lists and the gather (beam_std_init /
// beam_std_merge, which carry a length per hypothesis), and the read-out (beam_std_finish ranks n_best of them).
// One run's width and rule travel as a BeamRun: no function of the search reads the dc_set_beam_size setting.
struct BeamRun { int beam; bool standard; };
// Proposals that advance together: all of them (rows = P x beam, one GEMM per step over every proposal) unless the
// full-logits buffer rows x (V+1) would pass 2^28 floats (1 GiB) -- e.g. 5,114 proposals at beam 5 / V = 10,497.
int beam_chunk(const dc_ctx* ctx, BeamRun run, int n) {
  const long cap = (long)(ctx->beam_chunk_floats / ((int64_t)run.beam * (ctx->V + 1)));
  return (int)std::max<long>(1, std::min<long>(n, std::max<long>(64, cap)));
}
int beam_prepare(dc_ctx* ctx, Lane& L, BeamRun run, int chunk) {
  const int beam = run.beam, rows = chunk * beam;
  // bm_enc is sized by the chunk, bm_top_lp / bm_top_idx by rows x beam: the scratch is reusable only when NONE of the
  // three grew (beam 2 x 1000 proposals and beam 20 x 100 have the same row count but not the same carve)
  if (L.beam_base && L.beam_rows >= rows && L.beam_chunk >= chunk && L.beam_width >= beam) return DC_OK;
  if (L.beam_base) { HIPCHK(hipStreamSynchronize(L.stream)); HIPCHK(hipFree(L.beam_base)); L.beam_base = nullptr; }
  const int E = ctx->E, Hd = ctx->Hd, V1 = ctx->V + 1, T = ctx->T;
  L.beam_base = nullptr; L.beam_rows = L.beam_chunk = L.beam_width = 0;
  const std::vector<Carve> cv = {
      {(void**)&L.bm_enc, (size_t)chunk * E * 4},      {(void**)&L.bm_gates, (size_t)rows * 4 * Hd * 4},
      {(void**)&L.bm_h[0], (size_t)rows * Hd * 4},     {(void**)&L.bm_h[1], (size_t)rows * Hd * 4},
      {(void**)&L.bm_c[0], (size_t)rows * Hd * 4},     {(void**)&L.bm_c[1], (size_t)rows * Hd * 4},
      {(void**)&L.bm_logits, (size_t)rows * V1 * 4},   {(void**)&L.bm_top_lp, (size_t)rows * beam * 4},
      {(void**)&L.bm_top_idx, (size_t)rows * beam * 4}, {(void**)&L.bm_lp[0], (size_t)rows * 4},
      {(void**)&L.bm_lp[1], (size_t)rows * 4},         {(void**)&L.bm_beams[0], (size_t)rows * T * 4},
      {(void**)&L.bm_beams[1], (size_t)rows * T * 4},  {(void**)&L.bm_parent, (size_t)rows * 4},
      {(void**)&L.bm_tok, (size_t)rows * 4},           {(void**)&L.bm_fin, (size_t)rows},
      // the standard search's: carved for either rule (a few bytes per row beside the logits' rows x (V+1) x 4)
      {(void**)&L.bs_len[0], (size_t)rows * 4},        {(void**)&L.bs_len[1], (size_t)rows * 4},
      {(void**)&L.bs_pen, ((size_t)T + 1) * 4},
  };
  HIPCHK(hipMalloc(&L.beam_base, carve(cv, nullptr)));
  carve(cv, L.beam_base);
  L.beam_rows = rows; L.beam_chunk = chunk; L.beam_width = beam;
  return DC_OK;
}

// One LSTM step of the beam search on the words in bm_tok, in place on (h, c)
static int beam_lstm_step(dc_ctx* ctx, Lane& L, float* h, float* c, int rows, hipStream_t s) {
  const int Hd = ctx->Hd;
  GemmDesc d;
  d.A = h; d.W = ctx->whT; d.C = L.bm_gates; d.M = rows; d.N = 4 * Hd; d.K = Hd; d.ldc = 4 * Hd;
  d.rowterm = ctx->xg; d.rowidx = L.bm_tok; d.rowterm_ld = 4 * Hd;      // bm_tok: always a valid id (beam.hip, "No word")
  DCCHK(run_gemm(ctx, d, s));
  KCHK(launch_lstm_pointwise(L.bm_gates, c, h, rows, nullptr, Hd, 0, s));
  return DC_OK;
}

// The beam search keeps its state in two ping-pong sets: iteration t (1 <= t < T) reads the LSTM state in bm_h / bm_c[t & 1] and
// the beams in bm_lp / bm_beams[(t & 1) ^ 1], and writes the other set of each (the standard search's bs_len rides with bm_lp and
// bm_beams).  beam_start leaves what t = 1 reads.
static int beam_state_set(int t) { return t & 1; }
static int beam_beams_set(int t) { return (t & 1) ^ 1; }

// Everything before the t loop for the c proposals of one chunk: image step (:198-201), START step (:203-206), one state row per
// proposal, then the first expansion to c x beam rows (top-k lists of the first step in bm_top_lp / bm_top_idx, c x beam).
int beam_start(dc_ctx* ctx, Lane& L, BeamRun run, const float* codes, int c, hipStream_t s) {
  const int beam = run.beam, E = ctx->E, Hd = ctx->Hd, V1 = ctx->V + 1, T = ctx->T, D = ctx->D;
  if (run.standard) {         // lm_start_state: h AND c of the START step
    DCCHK(lm_start_state(ctx, s, codes, c, L.bm_enc, L.bm_gates, L.bm_c[0], L.bm_h[0], 0, nullptr, Ws()));
  } else {
    DCCHK(linear(ctx, s, codes, ctx->enc_w, ctx->enc_b, L.bm_enc, c, E, D, 1));
    DCCHK(linear(ctx, s, L.bm_enc, ctx->wxT, ctx->lstm_b, L.bm_gates, c, 4 * Hd, E, 0));
    KCHK(launch_lstm_pointwise(L.bm_gates, L.bm_c[0], L.bm_h[0], c, nullptr, Hd, 1, s));
    KCHK(launch_fill_i32(L.bm_tok, V1, c, s));
    DCCHK(beam_lstm_step(ctx, L, L.bm_h[0], L.bm_c[0], c, s));
  }
  DCCHK(linear(ctx, s, L.bm_h[0], ctx->out_w, ctx->out_b, L.bm_logits, c, V1, Hd, 0));
  KCHK(launch_beam_logsoftmax_topk(L.bm_logits, c, V1, V1, nullptr, beam, L.bm_top_lp, L.bm_top_idx, s));
  if (run.standard)
    KCHK(launch_beam_std_init(L.bm_top_lp, L.bm_top_idx, c, beam, T, V1, L.bm_lp[0], L.bm_beams[0], L.bs_len[0], L.bm_parent,
                              L.bm_tok, L.bm_fin, s));
  else
    KCHK(launch_beam_init(L.bm_top_lp, L.bm_top_idx, c, beam, T, V1, L.bm_lp[0], L.bm_beams[0], L.bm_parent, L.bm_tok,
                          L.bm_fin, s));
  // Reference rule: LanguageModel.lua:221-226 duplicates the states for the beams with
  // `layer.output = layer.cell:expand(...):clone()`: BOTH the cell and the hidden state of every beam start from the CELL state
  // of the START step (torch-rnn's nn.LSTM with remember_states reads h0 from self.output).  Replicated as written: h rows := c rows.
  // Standard search: every hypothesis of a proposal starts from the proposal's (h, c).
  KCHK(launch_beam_gather_state(run.standard ? L.bm_h[0] : L.bm_c[0], L.bm_c[0], L.bm_parent, c * beam, beam, 1, Hd, L.bm_h[1],
                                L.bm_c[1], s));
  return DC_OK;
}

// Iteration t of the loop (:228-278) on the c x beam rows of one chunk: LSTM step on bm_tok, vocabulary projection, LogSoftMax +
// top-k per row with the finished mask (lists in bm_top_lp / bm_top_idx, rows x beam), beam x beam merge, states by parent.
int beam_iter(dc_ctx* ctx, Lane& L, BeamRun run, int c, int t, hipStream_t s) {
  const int beam = run.beam, Hd = ctx->Hd, V1 = ctx->V + 1, T = ctx->T, rows = c * beam;
  const int cur = beam_state_set(t), bcur = beam_beams_set(t);
  DCCHK(beam_lstm_step(ctx, L, L.bm_h[cur], L.bm_c[cur], rows, s));
  DCCHK(linear(ctx, s, L.bm_h[cur], ctx->out_w, ctx->out_b, L.bm_logits, rows, V1, Hd, 0));
  KCHK(launch_beam_logsoftmax_topk(L.bm_logits, rows, V1, V1, L.bm_fin, beam, L.bm_top_lp, L.bm_top_idx, s));
  if (run.standard)
    KCHK(launch_beam_std_merge(L.bm_top_lp, L.bm_top_idx, L.bm_lp[bcur], L.bm_beams[bcur], L.bs_len[bcur], L.bm_fin, c, beam, T, t,
                               V1, L.bm_lp[bcur ^ 1], L.bm_beams[bcur ^ 1], L.bs_len[bcur ^ 1], L.bm_parent, L.bm_tok, L.bm_fin, s));
  else
    KCHK(launch_beam_merge(L.bm_top_lp, L.bm_top_idx, L.bm_lp[bcur], L.bm_beams[bcur], c, beam, T, t, V1,
                           L.bm_lp[bcur ^ 1], L.bm_beams[bcur ^ 1], L.bm_parent, L.bm_tok, L.bm_fin, s));
  KCHK(launch_beam_gather_state(L.bm_h[cur], L.bm_c[cur], L.bm_parent, rows, beam, beam, Hd, L.bm_h[cur ^ 1],
                                L.bm_c[cur ^ 1], s));
  return DC_OK;
}

// pen[l] = (float)pow(l, alpha) for l = 0..T (pen[0] = 1: a hypothesis without a word has a NaN score already)
std::vector<float> beam_std_pen(int T, float alpha) {
  std::vector<float> pen((size_t)T + 1, 1.f);
  for (int l = 1; l <= T; ++l) pen[l] = (float)pow((double)l, (double)alpha);
  return pen;
}
// Where a search leaves its result (DEVICE buffers).  Reference rule: seq (n, T), the tokens of every proposal's best beam.
// Standard search: seq (n, n_best, T) and logprob (n, n_best), ranked under length_alpha.
struct BeamOut { int32_t* seq; float* logprob = nullptr; int n_best = 1; float length_alpha = 0.f; };
// The whole search on n code rows, chunk by chunk.  Eager: the scratch is allocated on first use, and the length-penalty table goes
// up with a blocking copy before the first launch (every caller has synchronised its previous call: nothing on the stream still
// reads bs_pen); the launches themselves are only enqueued.
int beam_search(dc_ctx* ctx, Lane& L, hipStream_t s, BeamRun run, const float* codes, int n, const BeamOut& out) {
  const int chunk = beam_chunk(ctx, run, n);
  DCCHK(beam_prepare(ctx, L, run, chunk));
  const int beam = run.beam, T = ctx->T, D = ctx->D, N = out.n_best, bs = beam_beams_set(T);
  const int has_pen = run.standard && out.length_alpha != 0.f;
  if (has_pen) HIPCHK(hipMemcpy(L.bs_pen, beam_std_pen(T, out.length_alpha).data(), ((size_t)T + 1) * 4, hipMemcpyHostToDevice));
  for (int p0 = 0; p0 < n; p0 += chunk) {
    const int c = std::min(chunk, n - p0);
    DCCHK(beam_start(ctx, L, run, codes + (size_t)p0 * D, c, s));
    for (int t = 1; t < T; ++t) DCCHK(beam_iter(ctx, L, run, c, t, s));
    if (run.standard)
      KCHK(launch_beam_std_finish(L.bm_lp[bs], L.bm_beams[bs], L.bs_len[bs], L.bs_pen, has_pen, c, beam, T, N,
                                  out.seq + (size_t)p0 * N * T, out.logprob + (size_t)p0 * N, s));
    else
      KCHK(launch_beam_best(L.bm_beams[bs], c, beam, T, out.seq + (size_t)p0 * T, s));
  }
  return DC_OK;
}

constexpr int kScorePlanRows = 4096;    // lm_score: rows its per-region GEMMs are planned on, at most (see there)

// ---- what lm_score and lm_sample_n share ------------------------------------------------------------------------------------
// Both run `items` (queries / draws) on n region codes: rows = item * n + region, in chunks of whole items under a row cap, on
// scratch of their own, eager, and always with the fp32 MFMA kernels (their epilogues have no split-bf16 variant).
struct Fp32Guard {        // math_mode = 0 while one lives, whatever dc_set_math_mode says
  Settings& c; int saved;
  explicit Fp32Guard(Settings& cfg) : c(cfg), saved(cfg.math_mode) { c.math_mode = 0; }
  ~Fp32Guard() { c.math_mode = saved; }
};
struct LmRows {
  int n = 0, plan = 0, chunk = 0;       // region rows; rows every GEMM is planned on; whole items per chunk
  size_t rmax = 0;                      // rows of a full chunk
  float *enc = nullptr, *g0 = nullptr, *h0 = nullptr, *c0 = nullptr;          // per region: encoder output, gates, START state
  float *h = nullptr, *c = nullptr, *gates = nullptr, *part = nullptr;        // per row: state, gates, the step GEMM's partials
  double* acc = nullptr;                // per row: the sum of its log-probability terms
  std::vector<double> acc_host;         // acc of the chunk just run (lm_chunk_end)
  Scratch block;                        // what the pointers above are carved from (lm_rows_alloc)
  LmRows(dc_ctx* ctx, hipStream_t s) : block(ctx->scratch, s) {}
};
// The chunk: as many whole items as `rows_cap` rows hold (the caller's dc_debug_set knob; 0 = ~512 MiB of scratch at row_bytes a
// row), at least one.  The per-region GEMMs are planned on min(n, kScorePlanRows) rows: every plan then stays on the
// sequential-K v2 kernels (the image encoder, K = 4096, would take the K-split kernel -- another summation order -- from about
// 6,300 planned rows on), and a v2 element's K order does not depend on its tile, so a region's numbers do not depend on the
// other regions in the call.
void lm_rows_plan(LmRows& w, int n, int items, int64_t rows_cap, size_t row_bytes) {
  const int64_t cap = rows_cap > 0 ? rows_cap : (int64_t)(((size_t)512 << 20) / row_bytes);
  w.n = n;
  w.chunk = (int)std::max<int64_t>(1, std::min<int64_t>(items, cap / n));
  w.plan = std::min(n, kScorePlanRows);
  w.rmax = (size_t)w.chunk * n;
}
// One allocation for the shared pieces (ld: floats of partials per row) and the caller's `extra` ones; it dies with w.
int lm_rows_alloc(dc_ctx* ctx, LmRows& w, int ld, const std::vector<Carve>& extra) {
  const size_t n = w.n, E = ctx->E, Hd = ctx->Hd;
  std::vector<Carve> cv = {
      {(void**)&w.enc, n * E * 4},            {(void**)&w.g0, n * 4 * Hd * 4},        {(void**)&w.h0, n * Hd * 4},
      {(void**)&w.c0, n * Hd * 4},            {(void**)&w.h, w.rmax * Hd * 4},        {(void**)&w.c, w.rmax * Hd * 4},
      {(void**)&w.gates, w.rmax * 4 * Hd * 4}, {(void**)&w.part, w.rmax * ld * 4},    {(void**)&w.acc, w.rmax * 8},
  };
  cv.insert(cv.end(), extra.begin(), extra.end());
  HIPCHK(w.block.alloc(cv));
  return DC_OK;
}
// A chunk of ni items begins: the rows' integers go up (`ints` to `ints_dev`), acc -- and `flags`, one byte per row, where the
// caller keeps some -- are zeroed, and every item's row block starts from the regions' START state.
int lm_chunk_begin(dc_ctx* ctx, hipStream_t s, LmRows& w, int ni, int32_t* ints_dev, const std::vector<int32_t>& ints,
                   uint8_t* flags = nullptr) {
  const size_t rows = (size_t)ni * w.n;
  HIPCHK(hipMemcpyAsync(ints_dev, ints.data(), ints.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(w.acc, 0, rows * 8, s));
  if (flags != nullptr) HIPCHK(hipMemsetAsync(flags, 0, rows, s));
  KCHK(launch_repeat_rows2(w.h0, w.c0, (size_t)w.n * ctx->Hd, ni, w.h, w.c, s));
  return DC_OK;
}
// ... and ends: acc comes back into w.acc_host (row = item * n + region) and the stream is drained
int lm_chunk_end(dc_ctx* ctx, hipStream_t s, LmRows& w, int ni) {
  w.acc_host.resize((size_t)ni * w.n);
  HIPCHK(hipMemcpyAsync(w.acc_host.data(), w.acc, w.acc_host.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return DC_OK;
}

// Teacher-forced scoring: LanguageModel:updateOutput with a gt_sequence (LanguageModel.lua:106-127) and the targets of
// getTarget (:148-167) -- for region code r and query w_1..w_L the inputs [image vector, START, w_1 .. w_L], targets
// [null, w_1 .. w_L, END], loglik = sum over positions 2..L+2 of LogSoftMax(h_p.Wout^T + b)[y_p] (L+1 terms, END included).
// Schedule:
//   per region (n rows): lm_start_state -- enc, image step, h_0.Wh, START step, as lm_sample_parts describes them
//   per chunk of whole queries (rows = q * n + r, queries sorted by length, longest first): copy the START state to every row,
//   then for projection j = 1 .. Lmax+1: [log-sum-exp partials of h.Wout^T + b | G = h.Wh] ONE GEMM over the rows still alive
//   (a prefix: their queries have >= j - 1 words; the last projection has no Wh half) + lse_step_tail (log p of the target
//   added to the row's double sum; rows whose target is a word take the LSTM step with that word fed).
// Every GEMM is planned on min(n, kScorePlanRows) rows (plan_M) without split-K workspace, every element's arithmetic is a
// function of its row alone, and the per-row sums run in step order: a row's loglik does not depend on Q, the query order,
// the chunking or the other regions scored.
// `qry` (Q, Tq) host, validated; out[r * ldo + q].
int lm_score(dc_ctx* ctx, hipStream_t s, const float* codes, int n, const int32_t* qry, int Q, int Tq, float* out, int ldo) {
  const int Hd = ctx->Hd, V1 = ctx->V + 1;
  const int nslots = ctx->V1pad / 32, ld = 2 * nslots + 1;
  std::vector<int> len(Q), order(Q);
  for (int q = 0; q < Q; ++q) {
    int L = 0;
    while (L < Tq && qry[(size_t)q * Tq + L] != 0) ++L;
    len[q] = L;
    order[q] = q;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
  const int steps_max = len[order[0]] + 1;
  Fp32Guard fp32(ctx->cfg);
  LmRows w(ctx, s);
  lm_rows_plan(w, n, Q, ctx->score_rows_cap, (size_t)Hd * 6 * 4 + (size_t)ld * 4 + 8 + (size_t)steps_max * 4);
  int32_t* tgt = nullptr;       // the rows' targets, step by step
  DCCHK(lm_rows_alloc(ctx, w, ld, {{(void**)&tgt, w.rmax * steps_max * 4}}));
  auto body = [&]() -> int {
    DCCHK(lm_start_state(ctx, s, codes, n, w.enc, w.g0, w.c0, w.h0, w.plan, nullptr, Ws()));
    std::vector<int32_t> th;
    for (int a = 0; a < Q; a += w.chunk) {
      const int nq = std::min(w.chunk, Q - a), steps = len[order[a]] + 1;
      const size_t rows = (size_t)nq * n;
      th.assign(rows * steps, 0);
      for (int j = 1; j <= steps; ++j)
        for (int i = 0; i < nq; ++i) {
          const int q = order[a + i];
          if (len[q] + 1 < j) break;
          const int32_t tok = j <= len[q] ? qry[(size_t)q * Tq + j - 1] : V1;
          std::fill(th.begin() + (j - 1) * rows + (size_t)i * n, th.begin() + (j - 1) * rows + (size_t)(i + 1) * n, tok);
        }
      DCCHK(lm_chunk_begin(ctx, s, w, nq, tgt, th));
      int alive = nq;
      for (int j = 1; j <= steps; ++j) {
        while (alive > 0 && len[order[a + alive - 1]] + 1 < j) --alive;
        const bool last = j == steps;
        const int m = alive * n;
        GemmDesc v = decode_step_desc(ctx, w.h, m, w.plan, last, w.gates);     // epilogue: log-sum-exp partials, target's logit
        v.amax_val = w.part; v.amax_ld = ld; v.rowidx = tgt + (size_t)(j - 1) * rows;
        DCCHK(run_gemm(ctx, v, s));
        KCHK(launch_lse_step_tail(w.part, nslots, ld, v.rowidx, V1, ctx->xg, last ? nullptr : w.gates, w.c, w.h, w.acc, m, Hd, s));
      }
      DCCHK(lm_chunk_end(ctx, s, w, nq));
      for (int i = 0; i < nq; ++i)
        for (int r = 0; r < n; ++r) out[(size_t)r * ldo + order[a + i]] = (float)w.acc_host[(size_t)i * n + r];
    }
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "lm_score");
}

// Paired teacher-forced scoring (dc_forward_losses): n rows, row r scored against ITS OWN label row lab[r*L .. r*L+L) (words, then
// zeros), out[r] = the row's double sum -- the number lm_score forms for that (code, caption) pair, from the same pieces: the rows
// are permuted by caption length, longest first (stable), their codes gathered in that order, so that the rows still alive at a
// step are a prefix as lm_score's queries are; one item of n rows, tgt[(j-1)*n + row] the row's own target.  `plan`: the rows
// every GEMM is planned on (<= kScorePlanRows: the sequential-K kernels, see lm_rows_plan).  `lab` host, validated.
int lm_score_paired(dc_ctx* ctx, hipStream_t s, const float* codes, int n, int plan, const int32_t* lab, int L, double* out) {
  const int Hd = ctx->Hd, V1 = ctx->V + 1, D = ctx->D;
  const int nslots = ctx->V1pad / 32, ld = 2 * nslots + 1;
  std::vector<int> len(n), order(n);
  for (int r = 0; r < n; ++r) {
    int l = 0;
    while (l < L && lab[(size_t)r * L + l] != 0) ++l;
    len[r] = l;
    order[r] = r;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
  const int steps = len[order[0]] + 1;
  Fp32Guard fp32(ctx->cfg);
  LmRows w(ctx, s);
  lm_rows_plan(w, n, 1, 0, (size_t)Hd * 6 * 4 + (size_t)ld * 4 + 8 + (size_t)steps * 4);
  w.plan = std::min(plan, kScorePlanRows);
  int32_t* ints = nullptr;      // the rows' targets step by step, then the permutation and the row count
  float* gcodes = nullptr;
  const size_t n_tgt = (size_t)n * steps;
  DCCHK(lm_rows_alloc(ctx, w, ld, {{(void**)&ints, (n_tgt + n + 1) * 4}, {(void**)&gcodes, (size_t)n * D * 4}}));
  std::vector<int32_t> th(n_tgt + n + 1, 0);
  auto body = [&]() -> int {
    for (int j = 1; j <= steps; ++j)
      for (int i = 0; i < n; ++i) {
        const int r = order[i];
        if (len[r] + 1 < j) break;
        th[(size_t)(j - 1) * n + i] = j <= len[r] ? lab[(size_t)r * L + j - 1] : V1;
      }
    for (int i = 0; i < n; ++i) th[n_tgt + i] = order[i];
    th[n_tgt + n] = n;
    HIPCHK(hipMemcpyAsync(ints, th.data(), th.size() * 4, hipMemcpyHostToDevice, s));
    KCHK(launch_gather_rows(codes, ints + n_tgt, ints + n_tgt + n, n, D, gcodes, s));
    DCCHK(lm_start_state(ctx, s, gcodes, n, w.enc, w.g0, w.c0, w.h0, w.plan, nullptr, Ws()));
    DCCHK(lm_chunk_begin(ctx, s, w, 1, ints, th));
    int alive = n;
    for (int j = 1; j <= steps; ++j) {
      while (alive > 0 && len[order[alive - 1]] + 1 < j) --alive;
      const bool last = j == steps;
      GemmDesc v = decode_step_desc(ctx, w.h, alive, w.plan, last, w.gates);
      v.amax_val = w.part; v.amax_ld = ld; v.rowidx = ints + (size_t)(j - 1) * n;
      DCCHK(run_gemm(ctx, v, s));
      KCHK(launch_lse_step_tail(w.part, nslots, ld, v.rowidx, V1, ctx->xg, last ? nullptr : w.gates, w.c, w.h, w.acc, alive, Hd, s));
    }
    DCCHK(lm_chunk_end(ctx, s, w, 1));
    for (int i = 0; i < n; ++i) out[order[i]] = w.acc_host[i];
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "lm_score_paired");
}

// Language-model gradients (docs/SEMANTICS.md, "Language-model gradients"): the forward of lm_score_paired with
// every step's state kept, then the backward through it.  Rows are permuted longest caption first, as there.  The kept state
// lives in SLOTS of rows, slot q at row off[q] of every buffer:
//   slot 0 (n rows): the image cell -- X = enc, G = its full pre-activation, DG = its gate gradient
//   slot 1 (n rows): h_0, c_0;  G = h_0.Wh (the START cell's pre-activation less xg[START]);  X = Emb[START]
//   slot 1 + j (alive_j rows, j = 1 .. steps): h_j, c_j, the state projection j reads;  G = h_j.Wh;  X = Emb[w_j] -- the input
//     of the cell that consumes h_j, whose gate gradient DG sits in the same slot (zero rows where the caption has ended)
// so that X, H and DG are each ONE row-major matrix for the stacked weight gradients.  Launch list (lane 0's stream, eager):
//   forward : gather codes; lm_start_state; the image cell once more into slots 0 / 1 (same descriptor, same bits); per step the
//             GEMM of decode_step_desc + a copy of c into the next slot + lse_step_tail there
//   backward: logits of all steps in one storing GEMM; softmax_grad rows; dH = dlogits.Wout (GEMM on out_wT);
//             per step, last first: lstm_cell_bwd, then dh_prev = dgates.Wh^T (GEMM on the checkpoint lstm_w); the image cell
//   stacked : dWout, dWx, dWh, dWenc (wgrad), the three bias column sums, dX = DG.Wx^T (GEMM), ReLU mask, dcodes (GEMM on enc_wT)
//   rows    : embedding rows of the fed tokens for X (before `stacked`), the segment sum, the codes' rows back in caller order
constexpr size_t kLmGradMaxScratch = (size_t)8 << 30;
int lm_grad(dc_ctx* ctx, hipStream_t s, const float* codes, int n, const int32_t* lab, int L, float weight, const dc_lm_grads& out,
            double* loss, double* rowlik) {
  const int Hd = ctx->Hd, E = ctx->E, D = ctx->D, V = ctx->V, V1 = V + 1, V1pad = ctx->V1pad;
  const int nslots = V1pad / 32, ld = 2 * nslots + 1;
  // the two transposed weights, once per loaded checkpoint
  if (ctx->out_wT == nullptr || ctx->grad_epoch != ctx->weights_epoch) {
    if (ctx->out_wT == nullptr) {
      DCCHK(dev_alloc(ctx, (void**)&ctx->out_wT, (size_t)Hd * V1pad * 4));
      DCCHK(dev_alloc(ctx, (void**)&ctx->enc_wT, (size_t)D * E * 4));
    }
    KCHK(launch_transpose2d(ctx->out_w, ctx->out_wT, V1pad, Hd, s));     // the rows of dec_w past V+1 are zero up to V1pad
    KCHK(launch_transpose2d(ctx->enc_w, ctx->enc_wT, E, D, s));
    ctx->grad_epoch = ctx->weights_epoch;
  }
  std::vector<int> len(n), order(n);
  for (int r = 0; r < n; ++r) {
    int l = 0;
    while (l < L && lab[(size_t)r * L + l] != 0) ++l;
    len[r] = l;
    order[r] = r;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
  const int steps = len[order[0]] + 1;
  // alive[j], j = 1 .. steps: rows projection j covers (caption length + 1 >= j); off[q]: first row of slot q
  std::vector<int> alive(steps + 2, 0), off(steps + 3, 0);
  for (int j = 1; j <= steps; ++j) {
    int a = 0;
    while (a < n && len[order[a]] + 1 >= j) ++a;
    alive[j] = a;
  }
  off[0] = 0; off[1] = n; off[2] = 2 * n;
  for (int j = 1; j <= steps; ++j) off[2 + j] = off[1 + j] + alive[j];
  const int P = off[2 + steps], Mp = P - 2 * n;            // all rows; rows of the projections
  // host tables: tgt (Mp) the projections' targets; fed (P) the token fed to the cell that consumes a slot's state (0: none);
  // the permutation; the embedding gradient's sorted row list
  std::vector<int32_t> tgt(Mp, 0), fed(P, 0);
  for (int i = 0; i < n; ++i) fed[off[1] + i] = V1;         // START
  for (int j = 1; j <= steps; ++j)
    for (int i = 0; i < alive[j]; ++i) {
      const int r = order[i];
      tgt[off[1 + j] - 2 * n + i] = j <= len[r] ? lab[(size_t)r * L + j - 1] : V1;
      fed[off[1 + j] + i] = j <= len[r] ? lab[(size_t)r * L + j - 1] : 0;
    }
  std::vector<int32_t> erow;
  for (int r = n; r < P; ++r)
    if (fed[r] > 0) erow.push_back(r);
  std::stable_sort(erow.begin(), erow.end(), [&](int32_t a, int32_t b) { return fed[a] < fed[b]; });
  std::vector<int32_t> eseg, eid;
  for (size_t i = 0; i < erow.size(); ++i)
    if (i == 0 || fed[erow[i]] != fed[erow[i - 1]]) { eseg.push_back((int32_t)i); eid.push_back(fed[erow[i]]); }
  eseg.push_back((int32_t)erow.size());
  const int ntok = (int)eid.size();
  // ints on the device: [tgt (Mp) | fed (P) | order (n) | n | erow | eseg | eid]
  std::vector<int32_t> ih;
  ih.insert(ih.end(), tgt.begin(), tgt.end());
  const size_t o_fed = ih.size();   ih.insert(ih.end(), fed.begin(), fed.end());
  const size_t o_ord = ih.size();   for (int i = 0; i < n; ++i) ih.push_back(order[i]);
  const size_t o_n = ih.size();     ih.push_back(n);
  const size_t o_erow = ih.size();  ih.insert(ih.end(), erow.begin(), erow.end());
  const size_t o_eseg = ih.size();  ih.insert(ih.end(), eseg.begin(), eseg.end());
  const size_t o_eid = ih.size();   ih.insert(ih.end(), eid.begin(), eid.end());
  // scratch
  const size_t ws_floats = std::max(std::max(wgrad_ws_floats(Mp, V1, Hd), wgrad_ws_floats(P, E, 4 * Hd)),
                                    std::max(wgrad_ws_floats(P - n, Hd, 4 * Hd), wgrad_ws_floats(n, E, D)));
  float *gcodes, *Hb, *Cb, *Gb, *DGb, *Xb, *dXb, *part, *logits, *dHp, *dhc, *dcc, *dcodes, *ws;
  double* acc;
  int32_t* ints;
  const std::vector<Carve> cv = {
      {(void**)&gcodes, (size_t)n * D * 4},     {(void**)&Hb, (size_t)P * Hd * 4},       {(void**)&Cb, (size_t)P * Hd * 4},
      {(void**)&Gb, (size_t)P * 4 * Hd * 4},    {(void**)&DGb, (size_t)P * 4 * Hd * 4},  {(void**)&Xb, (size_t)P * E * 4},
      {(void**)&dXb, (size_t)P * E * 4},        {(void**)&part, (size_t)n * ld * 4},     {(void**)&logits, (size_t)Mp * V1pad * 4},
      {(void**)&dHp, (size_t)Mp * Hd * 4},      {(void**)&dhc, (size_t)n * Hd * 4},      {(void**)&dcc, (size_t)n * Hd * 4},
      {(void**)&dcodes, (size_t)n * D * 4},     {(void**)&ws, ws_floats * 4},            {(void**)&acc, (size_t)n * 8},
      {(void**)&ints, ih.size() * 4},
  };
  const size_t bytes = carve(cv, nullptr);
  if (bytes > kLmGradMaxScratch)
    return ctx->fail(DC_E_UNSUPPORTED, "dc_op_lm_grad: n = %d rows of %d steps need %.2f GiB of kept state and scratch, more than the %d GiB "
                     "a call may take; pass fewer rows per call", n, steps, (double)bytes / (double)((size_t)1 << 30),
                     (int)(kLmGradMaxScratch >> 30));
  Fp32Guard fp32(ctx->cfg);
  const int plan = std::min(n, kScorePlanRows);
  Scratch base(ctx->scratch, s);
  HIPCHK(base.alloc(cv));
  auto& clock = ctx->lm_grad_clock;
  std::vector<double> acc_host(n);
  auto slot = [&](float* b, int q, int width) { return b + (size_t)off[q] * width; };
  auto body = [&]() -> int {
    const int32_t *d_tgt = ints, *d_fed = ints + o_fed;
    HIPCHK(hipMemcpyAsync(ints, ih.data(), ih.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(clock.record(0, s));
    // ---- forward ----
    KCHK(launch_gather_rows(codes, ints + o_ord, ints + o_n, n, D, gcodes, s));
    DCCHK(lm_start_state(ctx, s, gcodes, n, slot(Xb, 0, E), slot(Gb, 1, 4 * Hd), slot(Cb, 2, Hd), slot(Hb, 2, Hd), plan, nullptr, Ws()));
    {                          // the image cell again, kept: its pre-activation, c_0 and h_0 (lm_start_state's first GEMM and tail)
      GemmDesc g;
      g.A = slot(Xb, 0, E); g.W = ctx->wxT; g.bias = ctx->lstm_b; g.C = slot(Gb, 0, 4 * Hd); g.M = n; g.N = 4 * Hd; g.K = E; g.ldc = 4 * Hd;
      g.plan_M = plan;
      DCCHK(run_gemm(ctx, g, s));
      KCHK(launch_lstm_step_tail(nullptr, nullptr, 0, 0, 0, nullptr, slot(Gb, 0, 4 * Hd), slot(Cb, 1, Hd), slot(Hb, 1, Hd), n, nullptr, Hd, 1,
                                 nullptr, 1, 0, s));
    }
    HIPCHK(hipMemsetAsync(acc, 0, (size_t)n * 8, s));
    for (int j = 1; j <= steps; ++j) {
      const bool last = j == steps;
      GemmDesc v = decode_step_desc(ctx, slot(Hb, 1 + j, Hd), alive[j], plan, last, slot(Gb, 1 + j, 4 * Hd));
      v.amax_val = part; v.amax_ld = ld; v.rowidx = d_tgt + (off[1 + j] - 2 * n);
      DCCHK(run_gemm(ctx, v, s));
      if (!last)               // the rows that go on take their step in the next slot: c is updated in place there
        HIPCHK(hipMemcpyAsync(slot(Cb, 2 + j, Hd), slot(Cb, 1 + j, Hd), (size_t)alive[j + 1] * Hd * 4, hipMemcpyDeviceToDevice, s));
      KCHK(launch_lse_step_tail(part, nslots, ld, v.rowidx, V1, ctx->xg, last ? nullptr : slot(Gb, 1 + j, 4 * Hd), slot(Cb, 2 + j, Hd),
                                slot(Hb, 2 + j, Hd), acc, alive[j], Hd, s));
    }
    HIPCHK(hipMemcpyAsync(acc_host.data(), acc, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(clock.record(1, s));
    // ---- backward: projections, then the steps ----
    const float scale = (float)((double)weight / ((double)n * (double)(L + 2)));
    {
      GemmDesc g;              // the logits of every step, stored (the scorer's fused epilogue never writes them)
      g.A = slot(Hb, 2, Hd); g.W = ctx->out_w; g.bias = ctx->out_b; g.C = logits; g.M = Mp; g.N = V1; g.K = Hd; g.ldc = V1pad;
      DCCHK(run_gemm(ctx, g, s));
      KCHK(launch_softmax_grad(logits, V1pad, V1, d_tgt, scale, nullptr, Mp, s));
      g = GemmDesc();          // dH = dlogits.Wout
      g.A = logits; g.W = ctx->out_wT; g.C = dHp; g.M = Mp; g.N = Hd; g.K = V1pad; g.ldc = Hd;
      DCCHK(run_gemm(ctx, g, s));
    }
    HIPCHK(hipMemsetAsync(DGb, 0, (size_t)P * 4 * Hd * 4, s));
    HIPCHK(hipMemsetAsync(dhc, 0, (size_t)n * Hd * 4, s));
    HIPCHK(hipMemsetAsync(dcc, 0, (size_t)n * Hd * 4, s));
    for (int j = steps; j >= 1; --j) {       // the cell that made h_j: kept in slot j, consumed h_{j-1}
      KCHK(launch_lstm_cell_bwd(slot(Gb, j, 4 * Hd), d_fed + off[j], ctx->xg, slot(Cb, j, Hd), slot(Cb, 1 + j, Hd),
                                dHp + (size_t)(off[1 + j] - 2 * n) * Hd, dhc, dcc, slot(DGb, j, 4 * Hd), dcc, alive[j], Hd, s));
      GemmDesc g;              // dh_{j-1} = dgates.Wh^T: the checkpoint's Wh rows are (Hd, 4Hd), K contiguous
      g.A = slot(DGb, j, 4 * Hd); g.W = ctx->lstm_w_ck + (size_t)E * 4 * Hd; g.C = dhc; g.M = alive[j]; g.N = Hd; g.K = 4 * Hd; g.ldc = Hd;
      DCCHK(run_gemm(ctx, g, s));
    }
    KCHK(launch_lstm_cell_bwd(slot(Gb, 0, 4 * Hd), nullptr, nullptr, nullptr, slot(Cb, 1, Hd), nullptr, dhc, dcc, slot(DGb, 0, 4 * Hd), dcc, n,
                              Hd, s));
    HIPCHK(clock.record(2, s));
    // ---- stacked gradients ----
    KCHK(launch_embed_rows(ctx->emb, d_fed + n, P - n, E, slot(Xb, 1, E), s));
    KCHK(launch_wgrad(logits, V1pad, slot(Hb, 2, Hd), Hd, Mp, V1, Hd, out.lm_out_w, Hd, ws, s));
    KCHK(launch_colsum(logits, V1pad, Mp, V1, out.lm_out_b, s));
    KCHK(launch_wgrad(Xb, E, DGb, 4 * Hd, P, E, 4 * Hd, out.lstm_w, 4 * Hd, ws, s));
    KCHK(launch_wgrad(slot(Hb, 1, Hd), Hd, slot(DGb, 1, 4 * Hd), 4 * Hd, P - n, Hd, 4 * Hd, out.lstm_w + (size_t)E * 4 * Hd, 4 * Hd, ws, s));
    KCHK(launch_colsum(DGb, 4 * Hd, P, 4 * Hd, out.lstm_b, s));
    {
      GemmDesc g;              // dX = DG.Wx^T for every cell: slot 0 is d(enc) before the ReLU, the rest feed the embedding rows
      g.A = DGb; g.W = ctx->lstm_w_ck; g.C = dXb; g.M = P; g.N = E; g.K = 4 * Hd; g.ldc = E;
      DCCHK(run_gemm(ctx, g, s));
    }
    KCHK(launch_relu_mask(dXb, Xb, (size_t)n * E, s));
    KCHK(launch_wgrad(dXb, E, gcodes, D, n, E, D, out.lm_enc_w, D, ws, s));
    KCHK(launch_colsum(dXb, E, n, E, out.lm_enc_b, s));
    if (out.codes != nullptr) {
      GemmDesc g;              // dcodes = d(enc).Wenc
      g.A = dXb; g.W = ctx->enc_wT; g.C = dcodes; g.M = n; g.N = D; g.K = E; g.ldc = D;
      DCCHK(run_gemm(ctx, g, s));
    }
    HIPCHK(clock.record(3, s));
    // ---- rows ----
    HIPCHK(hipMemsetAsync(out.lm_emb, 0, (size_t)(V + 2) * E * 4, s));
    KCHK(launch_embed_segsum(dXb, E, ints + o_erow, ints + o_eseg, ints + o_eid, ntok, out.lm_emb, s));
    if (out.codes != nullptr) KCHK(launch_scatter_rows(dcodes, ints + o_ord, n, D, out.codes, s));
    HIPCHK(clock.record(4, s));
    HIPCHK(hipStreamSynchronize(s));
    clock.read();
    double sum = 0.0;
    for (int r = 0; r < n; ++r) sum += acc_host[r];           // (permuted order: longest caption first)
    *loss = (double)weight * (-sum) / ((double)n * (double)(L + 2));
    if (rowlik != nullptr)
      for (int i = 0; i < n; ++i) rowlik[order[i]] = acc_host[i];
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "dc_op_lm_grad");
}

// the rules of docs/SEMANTICS.md ("Sampling captions") for a dc_sample_opts; nothing is enqueued before they hold
int check_sample_opts(dc_ctx* ctx, const dc_sample_opts* o, const char* who) {
  if (o == nullptr) return ctx->fail(DC_E_INVALID, "%s: null options", who);
  if (o->num_samples < 1 || o->num_samples > 256)
    return ctx->fail(DC_E_INVALID, "%s: num_samples must be in 1..256 (got %d)", who, (int)o->num_samples);
  const float tp = o->temperature;
  if (!(tp == 0.f || (tp >= 0.01f && tp <= 100.f)))
    return ctx->fail(DC_E_INVALID, "%s: temperature must be 0 or in [0.01, 100] (got %g)", who, (double)tp);
  if (tp == 0.f && o->num_samples != 1)
    return ctx->fail(DC_E_INVALID, "%s: temperature 0 is the greedy rule, num_samples must be 1 (got %d)", who, (int)o->num_samples);
  return DC_OK;
}

// ... and for a dc_sample_trunc beside it.  *route = the truncation the row route runs with, or null: the call is the fused one.
int check_sample_trunc(dc_ctx* ctx, const dc_sample_opts* o, const dc_sample_trunc* tr, bool want_q, const char* who,
                       const dc_sample_trunc** route) {
  static const dc_sample_trunc kOff = {0, 1.f};
  *route = nullptr;
  const dc_sample_trunc* t = tr ? tr : &kOff;
  const int V1 = ctx->V + 1;
  if (t->top_k < 0 || t->top_k > V1)
    return ctx->fail(DC_E_INVALID, "%s: top_k must be 0 (off) or in 1..%d (got %d)", who, V1, (int)t->top_k);
  if (!(t->top_p > 0.f && t->top_p <= 1.f))
    return ctx->fail(DC_E_INVALID, "%s: top_p must be in (0, 1] (got %g)", who, (double)t->top_p);
  const bool on = t->top_k != 0 || t->top_p != 1.f;
  if (!on && !want_q) return DC_OK;
  if (o->temperature == 0.f)
    return ctx->fail(DC_E_INVALID, "%s: temperature 0 is the greedy rule: no top_k / top_p / sample_logprob with it", who);
  if ((size_t)V1 > sample_trunc_max_vocab())
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a vocabulary of %d words does not fit the truncation kernel's LDS row on this device (max %zu)",
                     who, V1, sample_trunc_max_vocab());
  *route = t;
  return DC_OK;
}

// Sampling captions: LanguageModel:sample with sample_argmax = false (LanguageModel.lua:40-41,328-333) -- S draws per region, each
// word drawn from SoftMax(scores / temperature) by the Gumbel-max rule with counter-based noise, and the model's own
// log-probability of every draw (definition: docs/SEMANTICS.md, "Sampling captions").
// Schedule (lm_score's shape, on the same shared pieces):
//   per region (n rows): lm_start_state -- the state before the first word does not depend on the draw
//   per chunk of whole draws (rows = s * n + i): copy the START state to every row, then for step t = 1 .. T:
//   [sampling partials of h.Wout^T + b | G = h.Wh] ONE GEMM over all rows of the chunk (the last step without the Wh half) +
//   sample_step_tail (word, log p added to the row's double sum, LSTM step with the word fed).  Finished rows stay in the launch:
//   where a row ends is data-dependent, there is no prefix to cut.
// Planned like lm_score (min(n, kScorePlanRows) rows, no split-K workspace), noise a function of (seed, s, r, t, column) alone
// with r = row_ids[i] (or i): a draw does not depend on S, the chunking, or the other regions in the call.
// row_ids: host (n) or null; samples (n, S, T) and logprob (n, S): host.
//
// The row route (truncation, or a caller who wants sample_logprob): the epilogue's five floats per slot cannot
// carry a top-k or nucleus cut, which needs the whole row before the choice.  Per step then: the logits h.Wout^T + b through
// linear() into rows x (V+1) floats of scratch (w.part: lm_rows_plan counts them in row_bytes, so the 512 MiB chunk rule and
// "sample_rows_cap" hold), G = h.Wh as lm_start_state forms it, and sample_trunc_rows (sample_trunc.hip) in the place of
// sample_step_tail.  The same shared pieces, the same planning, the same noise coordinates: the bit-identities above hold here
// too.  trunc == null and lq == null: the fused route, untouched.
int lm_sample_n(dc_ctx* ctx, hipStream_t s, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts& o,
                int32_t* samples, float* logprob, const dc_sample_trunc* trunc = nullptr, float* sample_logprob = nullptr) {
  const int Hd = ctx->Hd, V1 = ctx->V + 1, T = ctx->T, S = o.num_samples;
  const bool by_rows = trunc != nullptr || sample_logprob != nullptr;
  const int nslots = ctx->V1pad / 32, ld = by_rows ? V1 : 5 * nslots;
  Fp32Guard fp32(ctx->cfg);
  LmRows w(ctx, s);
  lm_rows_plan(w, n, S, ctx->sample_rows_cap,
               (size_t)Hd * 6 * 4 + (size_t)ld * 4 + 8 + (size_t)T * 4 + 8 + 1 + (by_rows ? 8 : 0));
  if (w.rmax > (size_t)INT32_MAX / (size_t)std::max(ld, 4 * Hd))
    return ctx->fail(DC_E_INVALID, "lm_sample_n: %d regions are too many rows for one launch", n);
  int32_t *seq = nullptr, *keys = nullptr;      // the rows' words; their (row id, draw) noise keys
  uint8_t* fin = nullptr;                       // END drawn at an earlier step
  double* acc_q = nullptr;                      // row route: the sum of the draws' log-probabilities under the truncated distribution
  DCCHK(lm_rows_alloc(ctx, w, ld, {{(void**)&seq, w.rmax * T * 4}, {(void**)&keys, w.rmax * 8}, {(void**)&fin, w.rmax},
                                   {(void**)&acc_q, by_rows ? w.rmax * 8 : 0}}));
  auto body = [&]() -> int {
    DCCHK(lm_start_state(ctx, s, codes, n, w.enc, w.g0, w.c0, w.h0, w.plan, nullptr, Ws()));
    std::vector<int32_t> kh, sh;
    std::vector<double> qh;
    for (int a = 0; a < S; a += w.chunk) {
      const int nd = std::min(w.chunk, S - a);
      const size_t rows = (size_t)nd * n;
      kh.resize(rows * 2);
      for (int i = 0; i < nd; ++i)
        for (int r = 0; r < n; ++r) {
          kh[2 * ((size_t)i * n + r)] = row_ids ? row_ids[r] : r;
          kh[2 * ((size_t)i * n + r) + 1] = a + i;
        }
      DCCHK(lm_chunk_begin(ctx, s, w, nd, keys, kh, fin));
      if (by_rows) HIPCHK(hipMemsetAsync(acc_q, 0, rows * 8, s));
      for (int t = 1; by_rows && t <= T; ++t) {
        const bool last = t == T;
        DCCHK(linear(ctx, s, w.h, ctx->out_w, ctx->out_b, w.part, (int)rows, V1, Hd, 0, Ws(), w.plan));
        if (!last) {
          GemmDesc g;              // h_t.Wh for the next step's gates, as lm_start_state forms h_0.Wh
          g.A = w.h; g.W = ctx->whT; g.C = w.gates; g.M = (int)rows; g.N = 4 * Hd; g.K = Hd; g.ldc = 4 * Hd; g.plan_M = w.plan;
          DCCHK(run_gemm(ctx, g, s));
        }
        SampleTruncArgs a = {};
        a.logits = w.part; a.ld = ld; a.V1 = V1; a.keys = keys; a.t = t;
        a.seed_lo = (uint32_t)(o.seed & 0xffffffffu); a.seed_hi = (uint32_t)(o.seed >> 32);
        a.inv_temp = 1.f / o.temperature; a.top_k = trunc ? trunc->top_k : 0; a.top_p = trunc ? trunc->top_p : 1.f;
        a.end_tok = V1; a.xg = ctx->xg; a.gates_pre = last ? nullptr : w.gates; a.c = w.c; a.h = w.h; a.Hd = Hd;
        a.acc = w.acc; a.acc_q = acc_q; a.fin = fin; a.seq = seq; a.T = T; a.tpos = t - 1;
        KCHK(launch_sample_trunc_rows(a, (int)rows, s));
      }
      for (int t = 1; !by_rows && t <= T; ++t) {
        const bool last = t == T;
        GemmDesc v = decode_step_desc(ctx, w.h, (int)rows, w.plan, last, w.gates);     // epilogue: the sampling partials
        v.amax_val = w.part; v.amax_ld = ld; v.rowidx = keys;
        v.samp_t = t; v.samp_seed_lo = (uint32_t)(o.seed & 0xffffffffu); v.samp_seed_hi = (uint32_t)(o.seed >> 32);
        v.samp_inv_temp = o.temperature == 0.f ? 0.f : 1.f / o.temperature;
        DCCHK(run_gemm(ctx, v, s));
        KCHK(launch_sample_step_tail(w.part, nslots, ld, V1, ctx->xg, last ? nullptr : w.gates, w.c, w.h, w.acc, fin, seq, T, t - 1,
                                     (int)rows, Hd, s));
      }
      sh.resize(rows * T);
      HIPCHK(hipMemcpyAsync(sh.data(), seq, rows * T * 4, hipMemcpyDeviceToHost, s));
      if (by_rows) {
        qh.resize(rows);
        HIPCHK(hipMemcpyAsync(qh.data(), acc_q, rows * 8, hipMemcpyDeviceToHost, s));
      }
      DCCHK(lm_chunk_end(ctx, s, w, nd));
      for (int i = 0; i < nd; ++i)
        for (int r = 0; r < n; ++r) {
          logprob[(size_t)r * S + a + i] = (float)w.acc_host[(size_t)i * n + r];
          if (sample_logprob != nullptr) sample_logprob[(size_t)r * S + a + i] = (float)qh[(size_t)i * n + r];
          memcpy(samples + ((size_t)r * S + a + i) * T, sh.data() + ((size_t)i * n + r) * T, (size_t)T * 4);
        }
    }
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "lm_sample_n");
}

// the validity rules of docs/SEMANTICS.md for a (Q, Tq) block of queries in host memory
int check_queries(dc_ctx* ctx, const int32_t* qry, int Q, int Tq, const char* who) {
  if (Q < 1) return ctx->fail(DC_E_INVALID, "%s: Q must be >= 1 (got %d)", who, Q);
  if (Tq < 1 || Tq > 64) return ctx->fail(DC_E_INVALID, "%s: Tq must be in 1..64 (got %d)", who, Tq);
  const int V = ctx->V;
  for (int q = 0; q < Q; ++q) {
    bool ended = false;
    for (int t = 0; t < Tq; ++t) {
      const int32_t w = qry[(size_t)q * Tq + t];
      if (w == 0) { ended = true; continue; }
      if (w < 0 || w > V)
        return ctx->fail(DC_E_INVALID, "%s: query %d, column %d: token %d is outside 1..%d", who, q, t, (int)w, V);
      if (ended)
        return ctx->fail(DC_E_INVALID, "%s: query %d, column %d: a word after a zero (a query is words, then zero padding)", who, q, t);
    }
  }
  return DC_OK;
}

// Single-image mode (lanes == 1): nothing else is in flight, so the small kernels and partial tile rounds of the 15
// decode steps leave the chip idle (~25 % of the decode).  The rows are cut into two blocks on two streams; their
// kernels fill each other's gaps.  Same outputs bit for bit (tests/test_gpu_e2e.py::test_single_lane_mode_parity).
int lm_sample_two_streams(dc_ctx* ctx, Lane& L, const float* codes, int n, int plan, int32_t* seq_out) {
  const int h = std::min(n, ((n / 2 + 127) / 128) * 128);
  if (h >= n || L.aux == nullptr) return lm_sample(ctx, L.stream, lane_lm_bufs(L), lane_ws(L), codes, n, plan, nullptr, seq_out);
  const size_t wsf = L.splitk_ws ? kSplitkWsFloats / 2 : 0;     // each block its own half of the partial-tile scratch
  const LmPart parts[2] = {{L.stream, 0, h, Ws{L.splitk_ws, wsf}},
                           {L.aux, h, n - h, Ws{L.splitk_ws ? L.splitk_ws + wsf : nullptr, wsf}}};
  HIPCHK(hipEventRecord(L.ev_fork, L.stream));
  HIPCHK(hipStreamWaitEvent(L.aux, L.ev_fork, 0));
  DCCHK(lm_sample_parts(ctx, lane_lm_bufs(L), codes, parts, 2, nullptr, seq_out, plan));
  HIPCHK(hipEventRecord(L.ev_join, L.aux));
  HIPCHK(hipStreamWaitEvent(L.stream, L.ev_join, 0));
  return DC_OK;
}

// The VGG-16 trunk (DenseCapModel.lua:73-76) of the g images at L.img, on the lane's stream: L.feat = conv5_3's map, (*fh, *fw)
// its size.  Shared by the test-time forward (enqueue_body) and the training forward of dc_forward_losses.
// nconv: only the first nconv convolutions (the training forward with kept activations stops behind pool2 and goes on in
// cnn_forward_kept); L.feat is then that layer's map.
int enqueue_trunk(dc_ctx* ctx, Lane& L, int g, int* fh, int* fw, int nconv = DC_NUM_VGG_CONVS) {
  hipStream_t s = L.stream;
  int h = L.H, w = L.W, cur = 0;
  KCHK(launch_conv3x3_c3(L.img, ctx->conv_w[0], ctx->conv_b[0], L.act[0], g, h, w, 64, 1, s));
  for (int i = 1; i < nconv; ++i) {
    if (kVgg[i].pool_after) {
      // conv + ReLU + ceil-mode 2x2 pool in one launch
      DCCHK(conv3x3_pool(ctx, s, L.act[cur], ctx->conv_w[i], ctx->conv_b[i], L.act[cur ^ 1], g, h, w, kVgg[i].cin,
                         kVgg[i].cout, 1, lane_ws(L)));
      h = (h + 1) / 2; w = (w + 1) / 2;
    } else {
      DCCHK(conv3x3(ctx, s, L.act[cur], ctx->conv_w[i], ctx->conv_b[i], L.act[cur ^ 1], g, h, w, kVgg[i].cin,
                    kVgg[i].cout, 1, lane_ws(L)));
    }
    cur ^= 1;
  }
  L.feat = L.act[cur];
  *fh = h; *fw = w;
  return DC_OK;
}

// Enqueue the whole forward of a GROUP of g images (laid out back to back at `img`) on the lane's stream (no host
// sync).  The dense stages run once for the whole group -- the convolutions over g images, fc6/fc7, heads and the
// decode over g*P RoI rows -- so their launches carry g times the tiles (fuller last rounds, half the launches per
// image); the per-image stages (RPN decode, NMS, RoI pooling, final NMS, gathers) loop over the images.  Every routing
// decision that changes a sum's order is planned per image (GemmDesc::plan_M), so an image's numbers do not depend on
// the group it travels in.
// `events`: record the stage events (an eager enqueue; a captured graph carries none -- dc_stage_times then has nothing)
// `no_decode`: boxes and scores only, no language model (dc_score_captions without tokens); the records' token rows are then
// stale and must not be read
// `boxes_in`: the RoI boxes are the caller's, already in L.in_boxes / L.in_n (enqueue_forward): the stages between the trunk
// and RoI pooling are replaced by the ingest launch (their events follow each other at once).  `clip_in`: DC_BOXES_CLIP
int enqueue_body(dc_ctx* ctx, Lane& L, int g, bool features_only, bool events, bool no_decode = false, bool boxes_in = false,
                 bool clip_in = false) {
  const Settings& cfg = ctx->cfg;
  hipStream_t s = L.stream;
  const int H = L.H, W = L.W, P = L.P;
#define STAGE_EVENT(i) do { if (events) HIPCHK(hipEventRecord(L.ev[i], s)); } while (0)
  STAGE_EVENT(0);
  // ---- VGG-16 trunk (DenseCapModel.lua:73-76) -------------------------------------------
  int h = H, w = W;
  DCCHK(enqueue_trunk(ctx, L, g, &h, &w));
  const size_t feat_elems = (size_t)h * w * 512;
  STAGE_EVENT(1);
  ensure_fault_word(ctx);            // every forward has an NMS and a final pack that report through it: made before any capture
  if (boxes_in) {
    STAGE_EVENT(2);
    STAGE_EVENT(3);
    // ---- the caller's boxes in the place of the localisation layer's roi_boxes (DenseCapModel.lua:242-275) ----------------
    KCHK(launch_boxes_ingest(L.in_boxes, L.in_n, g, P, clip_in ? 1 : 0, H, W, L.roi_boxes, L.box_src, L.count1, kCountStride, s));
    KCHK(launch_bilinear_roi_pool_group(L.feat, feat_elems, g, h, w, 512, L.roi_boxes, P, L.count1, kCountStride, nullptr, nullptr,
                                        0, H, W, 7, 7, L.roi_feats, 1, s));
  } else {
    // ---- RPN (LocalizationLayer.lua:265, build_rpn :609-690) ----------------------------------
    DCCHK(conv3x3(ctx, s, L.feat, ctx->rpn_w, ctx->rpn_b, L.rpn_hidden, g, h, w, 512, ctx->R, 1, lane_ws(L)));
    DCCHK(linear(ctx, s, L.rpn_hidden, ctx->heads_w, ctx->heads_b, L.heads, g * h * w, 6 * ctx->k, ctx->R, 0, Ws(), h * w));
    KCHK(launch_rpn_decode(L.heads, g, h, w, ctx->k, ctx->anchors, ctx->fc[0], ctx->fc[1], ctx->fc[2], ctx->fc[3], H, W,
                           L.rpn_boxes, nullptr, nullptr, L.rpn_xyxy, L.rpn_p, L.rpn_valid, cfg.clip_boxes, s));   // the whole group in one launch
    STAGE_EVENT(2);
    // ---- RPN NMS (LocalizationLayer.lua:318-338) ------------------------------------------------
    for (int i = 0; i < g; ++i)
      KCHK(launch_nms(L.nms, L.rpn_xyxy + (size_t)i * L.A * 4, L.rpn_p + (size_t)i * L.A, L.rpn_valid + (size_t)i * L.A, L.A,
                      nullptr, cfg.rpn_nms_thresh, P, L.picks1 + (size_t)i * P, L.count1 + i * kCountStride, cfg.nms_band, s, ctx->fault_dev));
    STAGE_EVENT(3);
    // ---- bilinear RoI pooling (LocalizationLayer.lua:338-349) -----------------------------------
    // one launch for the group; the picked RPN boxes are gathered by the kernel itself (and left in roi_boxes for the heads)
    KCHK(launch_bilinear_roi_pool_group(L.feat, feat_elems, g, h, w, 512, L.roi_boxes, P, L.count1, kCountStride, L.picks1, L.rpn_boxes,
                                        (size_t)L.A * 4, H, W, 7, 7, L.roi_feats, 1, s));
  }
  STAGE_EVENT(4);
  // ---- recog_base fc6/fc7 (DenseCapModel.lua:133) ------------------------------------------------
  const int R = g * P;                      // RoI rows of the group
  DCCHK(linear(ctx, s, L.roi_feats, ctx->fc6_w, ctx->fc6_b, L.fc6_out, R, ctx->D, 49 * 512, 1, lane_ws(L), P));
  DCCHK(linear(ctx, s, L.fc6_out, ctx->fc7_w, ctx->fc7_b, L.codes, R, ctx->D, ctx->D, 1, lane_ws(L), P));
  STAGE_EVENT(5);
  // ---- objectness / box regression / final boxes (DenseCapModel.lua:134,139-140) -----------------
  KCHK(launch_recog_heads(L.codes, ctx->head5_w, ctx->head5_b, L.roi_boxes, L.obj, L.final_trans, L.final_boxes,
                          L.final_xyxy, R, ctx->D, s));
  STAGE_EVENT(6);
  const bool survivors_only = cfg.captions_after_final_nms && !features_only;
  // single-image mode, reference order: decode (two row blocks on two streams) and final NMS (a third stream) are
  // independent consumers of the heads' outputs.  Per-launch HIP-event profiling wants kernels that do not overlap:
  // everything stays on one stream while it is on.
  const bool side_streams = cfg.serial_mode && !ctx->prof && !features_only && !survivors_only && R >= 256 &&
                            cfg.beam_size == 0 && !no_decode;
  hipStream_t sn = side_streams ? L.aux2 : s;       // stream of the final NMS
  if (side_streams) {
    HIPCHK(hipEventRecord(L.ev_fork2, s));
    HIPCHK(hipStreamWaitEvent(L.aux2, L.ev_fork2, 0));
  }
  // ---- language model (reference order: all P proposals, DenseCapModel.lua:127-162) -----------------
  if (!features_only && !survivors_only && !no_decode) {
    if (cfg.beam_size > 0) DCCHK(beam_search(ctx, L, s, {cfg.beam_size, false}, L.codes, R, {L.seq}));
    else if (side_streams) DCCHK(lm_sample_two_streams(ctx, L, L.codes, R, P, L.seq));
    else DCCHK(lm_sample(ctx, s, lane_lm_bufs(L), lane_ws(L), L.codes, R, P, nullptr, L.seq));
  }
  if (!survivors_only) STAGE_EVENT(7);
  // ---- final NMS + gather (DenseCapModel.lua:261-275) ----------------------------------------------
  for (int i = 0; i < g; ++i) {
    const size_t r0 = (size_t)i * P;
    // forward_test skips the final NMS when final_nms_thresh <= 0 (DenseCapModel.lua:261); extractFeatures calls
    // box_utils.nms unconditionally (DenseCapModel.lua:285-304)
    // (... on the RPN's boxes; a caller who passes boxes and no threshold wants the codes of those boxes: dc_extract_features_boxes)
    if (cfg.final_nms_thresh > 0.f || (features_only && !boxes_in)) {
      KCHK(launch_nms(L.nms, L.final_xyxy + r0 * 4, L.obj + r0, nullptr, P, L.count1 + i * kCountStride, cfg.final_nms_thresh, -1,
                      L.picks2 + r0, L.count2 + i * kCountStride, cfg.nms_band, sn, ctx->fault_dev));
    } else {
      // DenseCapModel.lua:261: no final NMS when final_nms_thresh <= 0 -> all RoIs, in RPN order
      KCHK(launch_iota_count(L.picks2 + r0, L.count2 + i * kCountStride, L.count1 + i * kCountStride, P, sn));
    }
  }
  if (side_streams) {
    HIPCHK(hipEventRecord(L.ev_join2, L.aux2));
    HIPCHK(hipStreamWaitEvent(s, L.ev_join2, 0));
  }
  // captions after the final NMS: event 7 sits between the two stages here as well, in the order they ran (harvest swaps the names)
  if (survivors_only) STAGE_EVENT(7);
  L.nms_before_decode = survivors_only;
  const bool packed_decode = survivors_only && cfg.beam_size == 0;
  if (no_decode) {
    // no language model in either order
  } else if (packed_decode) {
    // Identical outputs, less work: LSTM rows are independent, so only the rows the final NMS kept are decoded (~a quarter at
    // 1000 proposals / 0.3).  Round 6: ONCE PER GROUP -- the kept fc7 rows of all g images packed into one row block
    // (survivor_compact_kernel), ONE decode over it with the device-side row count (row tiles past it exit at once), routes
    // planned on one image's P rows as in the reference order: an element's arithmetic is the same in either order and in any
    // group (tests/test_gpu_e2e.py::test_caption_order_is_output_invariant).  final_pack reads the packed token rows back
    // image by image.
    KCHK(launch_survivor_compact(L.codes, L.picks2, L.count2, kCountStride, g, P, ctx->D, L.out_feats, L.surv_total, s));
    DCCHK(lm_sample(ctx, s, lane_lm_bufs(L), lane_ws(L), L.out_feats, R, P, L.surv_total, L.out_tokens));
  } else if (survivors_only) {
    // beam search after the final NMS: image by image (the beam rows of one image advance together)
    for (int i = 0; i < g; ++i) {
      const size_t r0 = (size_t)i * P;
      const int32_t *pk = L.picks2 + r0, *cnt = L.count2 + i * kCountStride;
      KCHK(launch_gather_rows(L.codes + r0 * ctx->D, pk, cnt, P, ctx->D, L.out_feats + r0 * ctx->D, s));
      // rows past K: zero codes, ignored
      DCCHK(beam_search(ctx, L, s, {cfg.beam_size, false}, L.out_feats + r0 * ctx->D, P, {L.out_tokens + r0 * ctx->T}));
    }
  }
  // ---- results: ONE gather launch for the group into packed records, ONE copy to the pinned host staging ---------------
  const size_t stride = pack_stride(ctx, P, features_only, boxes_in);
  KCHK(launch_final_pack(L.final_boxes, L.obj, survivors_only ? L.out_tokens : L.seq, packed_decode ? 2 : survivors_only ? 0 : 1,
                         features_only ? L.codes : nullptr, L.picks2, L.count2, kCountStride, ctx->fault_dev, g, P, ctx->T, ctx->D,
                         L.out_pack, stride, s, boxes_in ? L.box_src : nullptr));
  STAGE_EVENT(8);
  HIPCHK(hipMemcpyAsync(L.host_stage, L.out_pack, (size_t)g * stride, hipMemcpyDeviceToHost, s));
#undef STAGE_EVENT
  return DC_OK;
}

GraphKey graph_key(const dc_ctx* ctx, const Lane& L, int g, bool features_only, bool no_decode, const BoxSource& bs) {
  GraphKey k;
  k.carve_epoch = L.carve_epoch; k.weights_epoch = ctx->weights_epoch;
  k.fault_dev = ctx->fault_dev; k.arena = L.arena.p; k.host_stage = L.host_stage; k.splitk_ws = L.splitk_ws;
  k.H = L.H; k.W = L.W; k.P = L.P; k.g = g; k.features_only = features_only; k.no_decode = no_decode;
  k.box_src = bs.bl != nullptr; k.box_clip = bs.bl != nullptr && bs.clip;
  k.set = ctx->cfg;
  return k;
}

// imgs[0..g): the group's images.  `packed`: they are one buffer of the caller, back to back, and arrive in one copy; a list's
// images are copied one by one (two allocations whose addresses happen to follow each other are still not one buffer).
// `bs`: the group's box lists, bs.bl[0..g) (or none): their rows and counts travel to the lane beside the images, outside
// the captured body -- a replayed forward reads them from the lane.
int enqueue_forward(dc_ctx* ctx, Lane& L, const float* const* imgs, int g, int img_on_device, bool packed, Mode mode,
                    const BoxSource& bs) {
  hipStream_t s = L.stream;
  const bool features_only = mode == MODE_FEATURES, no_decode = mode == MODE_NO_DECODE;
  const size_t img_elems = (size_t)3 * L.H * L.W;
  const hipMemcpyKind kind = img_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const int per_copy = packed ? g : 1;
  for (int i = 0; i < g; i += per_copy)
    HIPCHK(hipMemcpyAsync(L.img + (size_t)i * img_elems, imgs[i], per_copy * img_elems * 4, kind, s));
  const bool boxes_in = bs.bl != nullptr, clip_in = boxes_in && bs.clip;
  if (boxes_in) {
    L.in_n_host.resize(g);
    for (int i = 0; i < g; ++i) {
      L.in_n_host[i] = bs.bl[i].n;
      HIPCHK(hipMemcpyAsync(L.in_boxes + (size_t)i * L.P * 4, bs.bl[i].boxes, (size_t)bs.bl[i].n * 16, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(L.in_n, L.in_n_host.data(), (size_t)g * 4, hipMemcpyHostToDevice, s));
  }
  L.g = g;
  const size_t stride = pack_stride(ctx, L.P, features_only, boxes_in);
  for (int i = 0; i < g; ++i) *reinterpret_cast<uint32_t*>(static_cast<char*>(L.host_stage) + i * stride + kRecFault) = 0;
  L.ran_graph = false;
  // Graph replay (dc_set_graph_replay): the FIRST forward of a key runs eagerly (lazy allocations, kernel attributes and
  // the stream-K fault word are all in place afterwards), the second is captured and instantiated, later ones are one
  // hipGraphLaunch.  Per-launch profiling and beam search (which allocates on first use) stay eager.
  const bool eligible = ctx->graphs && !ctx->prof && ctx->cfg.beam_size == 0;
  if (eligible) {
    const auto key = graph_key(ctx, L, g, features_only, no_decode, bs);
    if (L.gexec != nullptr && key == L.gkey) {
      HIPCHK(hipGraphLaunch(L.gexec, s));
      ctx->graph_launches += 1;
      L.ran_graph = true;
    } else if (L.last_key_valid && key == L.last_key) {
      if (L.gexec != nullptr) { (void)hipGraphExecDestroy(L.gexec); L.gexec = nullptr; }
      hipGraph_t graph = nullptr;
      HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
      const int rc = enqueue_body(ctx, L, g, features_only, false, no_decode, boxes_in, clip_in);
      const hipError_t e = hipStreamEndCapture(s, &graph);
      hipError_t e2 = hipSuccess;
      if (rc == DC_OK && e == hipSuccess && graph != nullptr) e2 = hipGraphInstantiate(&L.gexec, graph, nullptr, nullptr, 0);
      if (graph != nullptr) (void)hipGraphDestroy(graph);
      if (rc != DC_OK || e != hipSuccess || e2 != hipSuccess || L.gexec == nullptr) {
        // a forward that cannot be captured on this runtime: say so once (stderr + dc_last_error text, no error code:
        // the forward itself still runs, eagerly), stay eager on this ctx; dc_debug_fetch "graph_replay_on" reads 0 from here on
        const hipError_t why = e != hipSuccess ? e : e2;
        (void)hipGetLastError();
        L.gexec = nullptr;
        ctx->graphs = false;
        char note[256];
        snprintf(note, sizeof note, "dc_set_graph_replay: capture of a %dx%d forward failed (%s); graph replay is now OFF for this ctx",
                 L.W, L.H, rc != DC_OK ? ctx->err.c_str() : hipGetErrorString(why));
        fprintf(stderr, "libdensecap_hip: %s\n", note);
        ctx->graph_note = note;
        if (rc != DC_OK) return rc;
        DCCHK(enqueue_body(ctx, L, g, features_only, true, no_decode, boxes_in, clip_in));
      } else {
        L.gkey = key;
        ctx->graph_captures += 1;
        HIPCHK(hipGraphLaunch(L.gexec, s));
        ctx->graph_launches += 1;
        L.ran_graph = true;
      }
    } else {
      DCCHK(enqueue_body(ctx, L, g, features_only, true, no_decode, boxes_in, clip_in));
      L.last_key = key;
      L.last_key_valid = true;
    }
  } else {
    DCCHK(enqueue_body(ctx, L, g, features_only, true, no_decode, boxes_in, clip_in));
    L.last_key_valid = false;
  }
  L.busy = true;
  L.feats = features_only;
  L.boxes_in = boxes_in;
  return DC_OK;
}


// The ctx's sticky fault word read `fault` (a hand-off between workgroups did not arrive within its spin bound): clear it, turn
// off on this ctx what raised it -- the next forward has new settings, hence a new graph key -- and fail the call.
int fail_on_fault(dc_ctx* ctx, uint32_t fault, const char* who) {
  (void)hipMemset(ctx->fault_dev, 0, 64);
  if (fault == kFaultNmsBand) {
    ctx->cfg.nms_band = 0;          // every NMS window back on the chunk scan
    return ctx->fail(DC_E_HIP, "%s: NMS band scan: a hand-off between the waves of nms_scan_band_kernel did not arrive within the "
                               "spin bound; this ctx now scans every window by chunks -- repeat the call", who);
  }
  ctx->cfg.tail_mode = 1;           // stop sharing tiles between workgroups
  return ctx->fail(DC_E_HIP, "%s: stream-K: a workgroup's partner never published its partial tile within the spin bound (GPU "
                             "shared with another job?); this ctx now uses the K-split tail plan -- repeat the call", who);
}

// Wait for the lane's in-flight group and hand the results to the caller's buffers.
int harvest(dc_ctx* ctx, Lane& L) {
  if (!L.busy) return DC_OK;
  HIPCHK(hipStreamSynchronize(L.stream));
  L.busy = false;
  if (!L.ran_graph) {
    for (int i = 0; i < ST_COUNT; ++i) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]);
      L.stage_ms[i] = ms / (float)std::max(L.g, 1);       // per image of the group
    }
    if (L.nms_before_decode) std::swap(L.stage_ms[ST_LSTM], L.stage_ms[ST_NMS2]);    // events 6..7 timed the NMS, 7..8 the decode
    if (L.boxes_in) L.stage_ms[ST_RPN] = L.stage_ms[ST_NMS1] = 0.f;                   // nothing ran between their events
  }
  L.have_times = !L.ran_graph;                            // a replayed graph carries no stage events
  const int P = L.P;
  const size_t stride = pack_stride(ctx, P, L.feats, L.boxes_in);
  const size_t row_bytes = (size_t)(L.feats ? ctx->D : ctx->T) * 4;      // values of one row: codes or tokens
  for (int i = 0; i < L.g; ++i) {
    const char* hs = static_cast<const char*>(L.host_stage) + i * stride;
    if (const uint32_t fw = *reinterpret_cast<const uint32_t*>(hs + kRecFault); fw != 0u) {
      L.dst = nullptr;
      return fail_on_fault(ctx, fw, "forward");
    }
    const Dest& d = L.dst[i];
    const int K = std::min(*reinterpret_cast<const int32_t*>(hs + kRecK), d.capacity);
    if (d.K) *d.K = K;
    if (d.T) *d.T = ctx->T;
    if (d.boxes) memcpy(d.boxes, hs + kRecPayload, (size_t)K * 16);
    if (d.scores) memcpy(d.scores, hs + rec_scores(P), (size_t)K * 4);
    if (d.values) memcpy(d.values, hs + rec_values(P), K * row_bytes);
    if (d.src && L.boxes_in) memcpy(d.src, hs + rec_src(P, pack_words(ctx, L.feats)), (size_t)K * 4);
  }
  L.dst = nullptr;
  return DC_OK;
}

Lane& lane0(dc_ctx* ctx) {
  if (ctx->lanes.empty()) ctx->lanes.emplace_back(new Lane());
  return *ctx->lanes[0];
}
int lane0_stream(dc_ctx* ctx, hipStream_t* s) {
  Lane& L = lane0(ctx);
  DCCHK(lane_streams(ctx, L));
  *s = L.stream;
  return DC_OK;
}

}  // namespace

int dc_ctx_device(const dc_ctx* ctx) { return ctx->device; }
void dc_ctx_set_error(dc_ctx* ctx, const char* msg) { ctx->err = msg; g_last_error = msg; }

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

int dc_create(dc_ctx** out, int hip_device) {
  if (!out) { g_last_error = "dc_create: null out"; return DC_E_INVALID; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_last_error = std::string("dc_create: no HIP device available (") + hipGetErrorString(e) +
                   "); this library has no CPU fallback";
    return DC_E_HIP;
  }
  if (hip_device < 0 || hip_device >= ndev) { g_last_error = "dc_create: bad device index"; return DC_E_INVALID; }
  e = hipSetDevice(hip_device);
  if (e != hipSuccess) { g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return DC_E_HIP; }
  dc_ctx* ctx = new dc_ctx();
  ctx->device = hip_device;
  const char* band = getenv("DC_NMS_BAND");          // an A/B and bisecting switch: DC_NMS_BAND=0 starts with the band scan off
  ctx->cfg.nms_band = band != nullptr && band[0] == '0' ? 0 : 1;
  *out = ctx;
  return DC_OK;
}

void dc_destroy(dc_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (auto& lp : ctx->lanes) lane_release(*lp);
  for (void* p : ctx->owned) hipFree(p);
  for (auto e : ctx->prof_pool) hipEventDestroy(e);
  delete ctx;                 // (the kept buffers and the stage clocks' events free themselves here)
}

const char* dc_last_error(const dc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

// LocalizationLayer:setTestArgs (LocalizationLayer.lua:233-238)
int dc_set_localization_test_args(dc_ctx* ctx, int clip_boxes, float nms_thresh, int max_proposals) {
  if (!ctx) return DC_E_INVALID;
  if (max_proposals != -1 && (max_proposals <= 0 || max_proposals > (1 << 20)))
    return ctx->fail(DC_E_UNSUPPORTED, "num_proposals must be -1 (uncapped) or in [1,1048576] (got %d)", max_proposals);
  ctx->cfg.clip_boxes = clip_boxes != 0;
  ctx->cfg.rpn_nms_thresh = nms_thresh;
  ctx->cfg.num_proposals = max_proposals;
  return DC_OK;
}

// DenseCapModel:setTestArgs (DenseCapModel.lua:185-191): the layer's setTestArgs WITHOUT a clip_boxes key (-> true) + opt.final_nms_thresh
int dc_set_test_args(dc_ctx* ctx, float rpn_nms_thresh, float final_nms_thresh, int num_proposals) {
  if (!ctx) return DC_E_INVALID;
  DCCHK(dc_set_localization_test_args(ctx, 1, rpn_nms_thresh, num_proposals));
  ctx->cfg.final_nms_thresh = final_nms_thresh;
  return DC_OK;
}

int dc_set_lanes(dc_ctx* ctx, int lanes) {
  if (!ctx) return DC_E_INVALID;
  if (lanes < 1 || lanes > 4) return ctx->fail(DC_E_INVALID, "dc_set_lanes: lanes must be in [1,4]");
  ctx->max_lanes = lanes;
  // numerics depend only on this setting, never on how many images a call happens to carry: with one lane the
  // last partial round of a layer is K-split (different fp32 summation order for those rows)
  ctx->cfg.serial_mode = lanes == 1;
  return DC_OK;
}

int dc_set_group(dc_ctx* ctx, int images) {
  if (!ctx) return DC_E_INVALID;
  if (images < 0 || images > kGemmMaxGroup) return ctx->fail(DC_E_INVALID, "dc_set_group: 0 (default = 1) .. %d images per group", kGemmMaxGroup);
  ctx->group = images;
  return DC_OK;
}

// beam search needs one vocabulary row in the top-k kernel's LDS and at least `beam` words to choose from
static int check_beam_fits(dc_ctx* ctx, int beam_size) {
  if (beam_size <= 0 || !ctx->have_weights) return DC_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(DC_E_HIP, "hipSetDevice failed");
  const size_t vmax = beam_topk_max_vocab();
  if ((size_t)(ctx->V + 1) > vmax)
    return ctx->fail(DC_E_UNSUPPORTED, "beam search: a vocabulary of %d words does not fit the top-k kernel's LDS row on this device (max %zu)",
                     ctx->V, vmax > 0 ? vmax - 1 : 0);
  if (beam_size > ctx->V + 1)
    return ctx->fail(DC_E_UNSUPPORTED, "beam search: beam_size %d exceeds the %d output words", beam_size, ctx->V + 1);
  return DC_OK;
}

int dc_set_beam_size(dc_ctx* ctx, int beam_size) {
  if (!ctx) return DC_E_INVALID;
  if (beam_size < 0 || beam_size > 32) return ctx->fail(DC_E_UNSUPPORTED, "dc_set_beam_size: beam_size must be in [0,32] (got %d)", beam_size);
  DCCHK(check_beam_fits(ctx, beam_size));          // before dc_load_weights the check runs there instead
  ctx->cfg.beam_size = beam_size;
  return DC_OK;
}

// the bf16 planes of every registered weight matrix (once; ~0.85 GB next to the 0.7 GB of fp32 weights)
static int make_weight_planes(dc_ctx* ctx) {
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  for (auto& e : ctx->planes) {
    if (e.planes != nullptr) continue;
    DCCHK(dev_alloc(ctx, reinterpret_cast<void**>(&e.planes), (size_t)3 * e.rows * e.K * 2));
    KCHK(launch_split_planes(e.W, e.planes, e.rows, e.K, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return DC_OK;
}

int dc_set_math_mode(dc_ctx* ctx, int mode) {
  if (!ctx) return DC_E_INVALID;
  if (mode != DC_MATH_FP32 && mode != DC_MATH_SPLIT_BF16)
    return ctx->fail(DC_E_INVALID, "dc_set_math_mode: 0 (fp32 MFMA) or 1 (split-bf16), got %d", mode);
  if (mode == DC_MATH_SPLIT_BF16 && ctx->have_weights) DCCHK(make_weight_planes(ctx));
  ctx->cfg.math_mode = mode;
  return DC_OK;
}

// nn.Dropout's own check (Dropout.lua: "p must be in range [0, 1)"); NaN fails the comparison
int dc_set_dropout(dc_ctx* ctx, float p) {
  if (!ctx) return DC_E_INVALID;
  if (!(p >= 0.f && p < 1.f)) return ctx->fail(DC_E_INVALID, "dc_set_dropout: p must be in [0, 1), got %g", (double)p);
  ctx->cfg.dropout_p = p;
  return DC_OK;
}
int dc_get_dropout(dc_ctx* ctx, float* p) {
  if (!ctx) return DC_E_INVALID;
  if (!p) return ctx->fail(DC_E_INVALID, "dc_get_dropout: null pointer");
  *p = ctx->cfg.dropout_p;
  return DC_OK;
}

int dc_set_graph_replay(dc_ctx* ctx, int on) {
  if (!ctx) return DC_E_INVALID;
  ctx->graphs = on != 0;
  return DC_OK;
}

int dc_set_caption_order(dc_ctx* ctx, int after_final_nms) {
  if (!ctx) return DC_E_INVALID;
  ctx->cfg.captions_after_final_nms = after_final_nms != 0;
  return DC_OK;
}

// the fp16 bit pattern of the smallest fp16 value not below x >= 0 (inf past 65504; NaN stays NaN)
static uint16_t half_bits_up(double x) {
  _Float16 h = (_Float16)x;
  uint16_t u;
  memcpy(&u, &h, 2);
  if ((double)h < x) u += 1;                         // x >= 0: the next pattern up (0x7bff + 1 = inf)
  return u;
}
// The constant c of the screen's bound |s_j - z_j| <= c |h|_2 |W_j|_2 + 2^-10 |s_j| + ... for K = Hd terms:
//   2u + u^2, u = 2^-8        both factors of a product rounded to bf16
//   (K/16) 2^-18 (1 + u)^2    the bf16 MFMA chain: K/16 instructions, each off by less than 2^-18 of the sum of magnitudes
//   K 2^-24 / (1 - K 2^-24)   the fp32 fmaf chain the score is compared with
// times 1 + 2^-8 for the fp32 evaluation of the bound itself; rounded up.
static float screen_bound_c(int K) {
  const double u = 0x1p-8, g = K * 0x1p-24;
  const double c = ((2 * u + u * u) + (K / 16.0) * 0x1p-18 * (1 + u) * (1 + u) + g / (1 - g)) * (1 + 0x1p-8);
  return nextafterf((float)c, INFINITY);
}

// n floats of a checkpoint weight in `stage`, on the device for the one launch that repacks them into the ctx's own layout
static int stage_weight(dc_ctx* ctx, Scratch& stage, const float* host, size_t n, float** dev) {
  HIPCHK(stage.alloc(n * 4));
  *dev = static_cast<float*>(stage.get());
  HIPCHK(hipMemcpy(*dev, host, n * 4, hipMemcpyHostToDevice));
  return DC_OK;
}

int dc_load_weights(dc_ctx* ctx, const dc_weights* w) {
  if (!ctx || !w) return DC_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->have_weights) return ctx->fail(DC_E_STATE, "weights already loaded; create a new ctx");
  // the supported family (docs/SEMANTICS.md, "Supported model dimensions"): every contraction walks K in 32-wide tiles, the
  // recognition heads walk fc_dim 256 columns at a time -- refused here, by field, so that no forward can fail on a dimension
  {
    const struct { const char* name; int v, mult; } dims[] = {
        {"num_anchors", w->num_anchors, 1}, {"rpn_hidden", w->rpn_hidden, 32}, {"fc_dim", w->fc_dim, 256},
        {"enc_size", w->enc_size, 32},      {"rnn_size", w->rnn_size, 32},     {"vocab_size", w->vocab_size, 1},
        {"seq_length", w->seq_length, 1}};
    for (const auto& f : dims)
      if (f.v <= 0 || f.v % f.mult)
        return ctx->fail(DC_E_INVALID, "dc_load_weights: unsupported dimensions: %s = %d must be a positive multiple of %d", f.name,
                         f.v, f.mult);
  }
  ctx->k = w->num_anchors; ctx->R = w->rpn_hidden; ctx->V = w->vocab_size; ctx->T = w->seq_length;
  ctx->E = w->enc_size; ctx->Hd = w->rnn_size; ctx->D = w->fc_dim;
  memcpy(ctx->fc, w->field_centers, sizeof ctx->fc);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  const int k = ctx->k, R = ctx->R, V = ctx->V, E = ctx->E, Hd = ctx->Hd, D = ctx->D;
  // VGG convs: conv1_1 stays OIHW (direct kernel); the rest are repacked to (Cout, 9*Cin)
  DCCHK(upload(ctx, &ctx->conv_w[0], w->conv_w[0], (size_t)64 * 27));
  DCCHK(upload(ctx, &ctx->conv_b[0], w->conv_b[0], 64));
  for (int i = 1; i < DC_NUM_VGG_CONVS; ++i) {
    const size_t n = (size_t)kVgg[i].cout * kVgg[i].cin * 9;
    if (!w->conv_w[i] || !w->conv_b[i]) return ctx->fail(DC_E_INVALID, "null conv weight %d", i);
    Scratch stage(ctx->scratch, s);
    float* tmp = nullptr;
    DCCHK(stage_weight(ctx, stage, w->conv_w[i], n, &tmp));
    DCCHK(dev_alloc(ctx, (void**)&ctx->conv_w[i], n * 4));
    KCHK(launch_pack_conv3x3(tmp, ctx->conv_w[i], kVgg[i].cout, kVgg[i].cin, s));
    HIPCHK(hipStreamSynchronize(s));
    DCCHK(upload(ctx, &ctx->conv_b[i], w->conv_b[i], kVgg[i].cout));
  }
  {  // RPN conv
    const size_t n = (size_t)R * 512 * 9;
    if (!w->rpn_conv_w) return ctx->fail(DC_E_INVALID, "null rpn_conv_w");
    Scratch stage(ctx->scratch, s);
    float* tmp = nullptr;
    DCCHK(stage_weight(ctx, stage, w->rpn_conv_w, n, &tmp));
    DCCHK(dev_alloc(ctx, (void**)&ctx->rpn_w, n * 4));
    KCHK(launch_pack_conv3x3(tmp, ctx->rpn_w, R, 512, s));
    HIPCHK(hipStreamSynchronize(s));
    DCCHK(upload(ctx, &ctx->rpn_b, w->rpn_conv_b, R));
  }
  {  // fused 1x1 heads: rows [0,4k) box, [4k,6k) score
    if (!w->rpn_box_w || !w->rpn_score_w || !w->rpn_box_b || !w->rpn_score_b)
      return ctx->fail(DC_E_INVALID, "null rpn head weight");
    std::vector<float> hw((size_t)6 * k * R), hb((size_t)6 * k);
    memcpy(hw.data(), w->rpn_box_w, (size_t)4 * k * R * 4);
    memcpy(hw.data() + (size_t)4 * k * R, w->rpn_score_w, (size_t)2 * k * R * 4);
    memcpy(hb.data(), w->rpn_box_b, (size_t)4 * k * 4);
    memcpy(hb.data() + 4 * k, w->rpn_score_b, (size_t)2 * k * 4);
    DCCHK(upload(ctx, &ctx->heads_w, hw.data(), hw.size()));
    DCCHK(upload(ctx, &ctx->heads_b, hb.data(), hb.size()));
  }
  {  // fc6: permute K from (c,i,j) to (i,j,c) to match the channels-last RoI features
    const size_t n = (size_t)D * 512 * 49;
    if (!w->fc6_w) return ctx->fail(DC_E_INVALID, "null fc6_w");
    Scratch stage(ctx->scratch, s);
    float* tmp = nullptr;
    DCCHK(stage_weight(ctx, stage, w->fc6_w, n, &tmp));
    DCCHK(dev_alloc(ctx, (void**)&ctx->fc6_w, n * 4));
    KCHK(launch_permute_fc6(tmp, ctx->fc6_w, D, 512, 49, s));
    HIPCHK(hipStreamSynchronize(s));
    DCCHK(upload(ctx, &ctx->fc6_b, w->fc6_b, D));
  }
  DCCHK(upload(ctx, &ctx->fc7_w, w->fc7_w, (size_t)D * D));
  DCCHK(upload(ctx, &ctx->fc7_b, w->fc7_b, D));
  {
    if (!w->obj_w || !w->boxreg_w || !w->obj_b || !w->boxreg_b) return ctx->fail(DC_E_INVALID, "null head weight");
    std::vector<float> h5((size_t)5 * D), b5(5);
    memcpy(h5.data(), w->obj_w, (size_t)D * 4);
    memcpy(h5.data() + D, w->boxreg_w, (size_t)4 * D * 4);
    b5[0] = w->obj_b[0];
    memcpy(b5.data() + 1, w->boxreg_b, 16);
    DCCHK(upload(ctx, &ctx->head5_w, h5.data(), h5.size()));
    DCCHK(upload(ctx, &ctx->head5_b, b5.data(), 5));
  }
  DCCHK(upload(ctx, &ctx->enc_w, w->lm_enc_w, (size_t)E * D));
  DCCHK(upload(ctx, &ctx->enc_b, w->lm_enc_b, E));
  DCCHK(upload(ctx, &ctx->lstm_b, w->lstm_b, (size_t)4 * Hd));
  {  // torch-rnn weight (E+Hd, 4Hd): rows [0,E) = Wx, [E,E+Hd) = Wh; kernels want (N,K)
    float* lw = nullptr;
    DCCHK(upload(ctx, &lw, w->lstm_w, (size_t)(E + Hd) * 4 * Hd));
    DCCHK(dev_alloc(ctx, (void**)&ctx->wxT, (size_t)4 * Hd * E * 4));
    DCCHK(dev_alloc(ctx, (void**)&ctx->whT, (size_t)4 * Hd * Hd * 4));
    ctx->lstm_w_ck = lw;
    KCHK(launch_transpose2d(lw, ctx->wxT, E, 4 * Hd, s));
    KCHK(launch_transpose2d(lw + (size_t)E * 4 * Hd, ctx->whT, Hd, 4 * Hd, s));
    // xg[v] = b + Emb[v].Wx for every token of the LookupTable (V+2 rows): the input half of the
    // gate pre-activation of every decode step becomes a row gather.
    float* emb = nullptr;
    DCCHK(upload(ctx, &emb, w->lm_emb, (size_t)(V + 2) * E));
    ctx->emb = emb;
    DCCHK(dev_alloc(ctx, (void**)&ctx->xg, (size_t)(V + 2) * 4 * Hd * 4));
    DCCHK(linear(ctx, s, emb, ctx->wxT, ctx->lstm_b, ctx->xg, V + 2, 4 * Hd, E, 0));
    HIPCHK(hipStreamSynchronize(s));
  }
  {  // decode-step operand: [Wout (V+1 rows); zero rows to a multiple of 64; Wh^T (4Hd rows)], all with K = Hd -- one GEMM
     // launch per step produces the vocabulary arg-max of h_t and h_t.Wh for the next step's gates
    if (!w->lm_out_w || !w->lm_out_b) return ctx->fail(DC_E_INVALID, "null lm_out weight");
    ctx->V1pad = (V + 1 + 63) / 64 * 64;
    const size_t rows = (size_t)ctx->V1pad + 4 * Hd;
    DCCHK(dev_alloc(ctx, (void**)&ctx->dec_w, rows * Hd * 4));
    HIPCHK(hipMemset(ctx->dec_w, 0, rows * Hd * 4));
    HIPCHK(hipMemcpy(ctx->dec_w, w->lm_out_w, (size_t)(V + 1) * Hd * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->dec_w + (size_t)ctx->V1pad * Hd, ctx->whT, (size_t)4 * Hd * Hd * 4, hipMemcpyDeviceToDevice));
    ctx->out_w = ctx->dec_w;
    // the screen's operands (Settings::decode_screen): Wout in bf16 (round to nearest even), rows padded with zeros to a
    // multiple of 64 columns and to V1pad rows; |Wout_j|_2 in double, rounded up to fp16; the bound's constant
    const int Kp = (Hd + 63) / 64 * 64;
    std::vector<uint16_t> wb((size_t)ctx->V1pad * Kp, 0);
    std::vector<uint16_t> wn((size_t)ctx->V1pad, 0);
    for (int j = 0; j <= V; ++j) {
      double ss = 0.0;
      for (int kk = 0; kk < Hd; ++kk) {
        const float x = w->lm_out_w[(size_t)j * Hd + kk];
        ss += (double)x * (double)x;
        uint32_t u;
        memcpy(&u, &x, 4);
        wb[(size_t)j * Kp + kk] = (u & 0x7fffffffu) > 0x7f800000u ? (uint16_t)((u >> 16) | 0x40) : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
      }
      wn[j] = half_bits_up(sqrt(ss) * (1.0 + 1e-9));   // (NaN / inf stay what they are: the row tail then scans exactly)
    }
    DCCHK(dev_alloc(ctx, (void**)&ctx->scr_w, wb.size() * 2));
    HIPCHK(hipMemcpy(ctx->scr_w, wb.data(), wb.size() * 2, hipMemcpyHostToDevice));
    DCCHK(dev_alloc(ctx, (void**)&ctx->scr_wnorm, wn.size() * 2));
    HIPCHK(hipMemcpy(ctx->scr_wnorm, wn.data(), wn.size() * 2, hipMemcpyHostToDevice));
    ctx->scr_Kp = Kp;
    ctx->scr_c = screen_bound_c(Hd);
  }
  DCCHK(upload(ctx, &ctx->out_b, w->lm_out_b, (size_t)V + 1));
  DCCHK(upload(ctx, &ctx->anchors, w->anchors, (size_t)2 * k));
  HIPCHK(hipStreamSynchronize(s));
  prof_collect(ctx);
  // the matrices the split-bf16 mode can take (one image's problem fills the chip): their planes are made when the mode is on
  for (int i = 1; i < DC_NUM_VGG_CONVS; ++i)
    ctx->planes.push_back({ctx->conv_w[i], (size_t)kVgg[i].cout, 9 * kVgg[i].cin, nullptr});
  ctx->planes.push_back({ctx->fc6_w, (size_t)D, 49 * 512, nullptr});
  ctx->planes.push_back({ctx->fc7_w, (size_t)D, D, nullptr});
  ctx->planes.push_back({ctx->dec_w, (size_t)ctx->V1pad + 4 * Hd, Hd, nullptr});
  if (ctx->cfg.math_mode == DC_MATH_SPLIT_BF16) DCCHK(make_weight_planes(ctx));
  ctx->have_weights = true;
  ctx->weights_epoch += 1;                 // captured graphs hold the old weight pointers
  if (int rc = check_beam_fits(ctx, ctx->cfg.beam_size); rc != DC_OK) {   // dc_set_beam_size came first: validate it now
    ctx->cfg.beam_size = 0;
    return rc;
  }
  return DC_OK;
}

// A failed enqueue/harvest must not leave lanes that still point at the caller's result buffers (the caller frees them
// when the error surfaces) or work in flight on a workspace that the next call may rebuild: wait for every lane and
// forget its pending destination without copying anything out.
static void drain_lanes(dc_ctx* ctx) {
  for (auto& lp : ctx->lanes) {
    Lane& L = *lp;
    if (L.stream) (void)hipStreamSynchronize(L.stream);
    if (L.aux) (void)hipStreamSynchronize(L.aux);
    if (L.aux2) (void)hipStreamSynchronize(L.aux2);
    L.busy = false;
    L.dst = nullptr;
  }
  (void)hipGetLastError();
}
#define DCCHK_DRAIN(expr)                 \
  do {                                    \
    int _r = (expr);                      \
    if (_r != DC_OK) { drain_lanes(ctx); return _r; } \
  } while (0)

// The reference puts no limit on the image size (box_utils.lua:154-256 handles any number of boxes).  What bounds an
// image here is the 32-bit operand addressing of the convolution kernels: the largest activation, conv1_x's
// (H, W, 64) fp32 map, must stay below 4 GiB -- about 16 Mpx.
static int check_image_size(dc_ctx* ctx, int H, int W, const char* who) {
  if ((size_t)H * W * 64 * 4 >= 0xffffe000ull)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a %dx%d image exceeds the conv kernels' 4 GiB activation limit (~16 Mpx)", who, W, H);
  return DC_OK;
}

// Length of the run of equal-sized images starting at i that may travel as one group (dc_set_group).  Single-image planning
// (dc_set_lanes(1)) shares a layer's partial last round along K -- plans made for ONE image's tile count, which a group does
// not have: images travel alone there, so that results never depend on the group.  A group's conv1_x activation shares one
// 32-bit operand offset space; the pooled conv counts window slots (4 per 2x2 window: a pixel more per odd side).
static int group_run(const dc_ctx* ctx, const int* H, const int* W, int i, int n) {
  if (ctx->cfg.serial_planning()) return 1;
  const size_t rows1 = std::max((size_t)H[i] * W[i], (size_t)4 * ((H[i] + 1) / 2) * ((W[i] + 1) / 2));
  int g = 1;
  while (g < ctx->group && i + g < n && H[i + g] == H[i] && W[i + g] == W[i] && (size_t)(g + 1) * rows1 * 64 * 4 < 0xffffe000ull)
    ++g;
  return g;
}

// The driver of every forward entry point, after the entry point's own argument checks: image i is imgs[i], (3, H[i], W[i]),
// and its results go to dst[i].  Runs of consecutive equal-sized images travel as groups (dc_set_group: the dense stages
// share launches), pipelined over the lanes.  A lane that takes a run of g images keeps its group capacity if it already
// holds their size, else it is carved for g; results do not depend on the capacity (every route is planned per image).
// `packed`: the images are one buffer of the caller, back to back (enqueue_forward).
// `bs`: caller-supplied boxes, bs.bl[i] for image i (checked by check_box_lists), or none.
static int run_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int on_dev, bool packed,
                      Mode mode, const Dest* dst, const BoxSource& bs = BoxSource()) {
  HIPCHK(hipSetDevice(ctx->device));
  int runs = 0;
  for (int i = 0; i < n; i += group_run(ctx, H, W, i, n)) ++runs;
  const int nl = std::min(runs, ctx->max_lanes);
  while ((int)ctx->lanes.size() < nl) ctx->lanes.emplace_back(new Lane());
  double enq_ms = 0;
  for (int i = 0, r = 0; i < n; ++r) {
    const int g = group_run(ctx, H, W, i, n);
    Lane& L = *ctx->lanes[r % nl];
    DCCHK_DRAIN(harvest(ctx, L));                 // the lane's previous images leave before its workspace is re-carved
    const int G = L.H == H[i] && L.W == W[i] ? std::max(g, L.G) : g;
    DCCHK_DRAIN(lane_prepare(ctx, L, H[i], W[i], effective_proposals(ctx, H[i], W[i]), G));
    L.dst = dst + i;
    const auto t0 = std::chrono::steady_clock::now();
    DCCHK_DRAIN(enqueue_forward(ctx, L, imgs + i, g, on_dev, packed, mode, BoxSource{bs.bl ? bs.bl + i : nullptr, bs.clip}));
    enq_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    i += g;
  }
  for (int l = 0; l < nl; ++l) DCCHK_DRAIN(harvest(ctx, *ctx->lanes[l]));
  ctx->host_enqueue_ms = enq_ms / n;       // host time spent enqueueing, per image (dc_debug_fetch "host_enqueue_us")
  prof_collect(ctx);
  return DC_OK;
}

static std::vector<Dest> result_dests(dc_result* r, int n) {
  std::vector<Dest> d(n);
  for (int i = 0; i < n; ++i) d[i] = Dest{r[i].boxes, r[i].scores, r[i].tokens, &r[i].K, &r[i].T, r[i].capacity};
  return d;
}

// dc_forward_test, dc_forward_batch and the forward of dc_score_captions: n images of one size, back to back at `imgs`
static int forward_batch(dc_ctx* ctx, const float* imgs, int n, int H, int W, int on_dev, dc_result* outs, Mode mode) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_forward_*: weights not loaded");
  if (!imgs || !outs || n <= 0 || H < 32 || W < 32) return ctx->fail(DC_E_INVALID, "dc_forward_*: bad arguments");
  DCCHK(check_image_size(ctx, H, W, "dc_forward_*"));
  for (int i = 0; i < n; ++i)
    if (outs[i].capacity <= 0) return ctx->fail(DC_E_INVALID, "dc_result.capacity must be > 0");
  std::vector<const float*> ptrs(n);
  for (int i = 0; i < n; ++i) ptrs[i] = imgs + (size_t)3 * H * W * i;
  const std::vector<int> Hs(n, H), Ws(n, W);
  const std::vector<Dest> dst = result_dests(outs, n);
  return run_images(ctx, ptrs.data(), Hs.data(), Ws.data(), n, on_dev, true, mode, dst.data());
}

int dc_forward_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int on_dev, dc_result* outs) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_forward_images: weights not loaded");
  if (!imgs || !H || !W || !outs || n <= 0) return ctx->fail(DC_E_INVALID, "dc_forward_images: bad arguments");
  for (int i = 0; i < n; ++i) {
    if (!imgs[i] || H[i] < 32 || W[i] < 32 || outs[i].capacity <= 0)
      return ctx->fail(DC_E_INVALID, "dc_forward_images: image %d: null pointer, side below 32 px or capacity <= 0", i);
    DCCHK(check_image_size(ctx, H[i], W[i], "dc_forward_images"));
  }
  const std::vector<Dest> dst = result_dests(outs, n);
  return run_images(ctx, imgs, H, W, n, on_dev, false, MODE_RESULTS, dst.data());
}

int dc_forward_test(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, dc_result* out) {
  return forward_batch(ctx, img_chw, 1, H, W, img_on_device, out, MODE_RESULTS);
}
int dc_forward_batch(dc_ctx* ctx, const float* imgs, int n, int H, int W, int imgs_on_device, dc_result* outs) {
  return forward_batch(ctx, imgs, n, H, W, imgs_on_device, outs, MODE_RESULTS);
}

int dc_extract_features(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, int capacity,
                        float* boxes, float* feats, int32_t* K) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_extract_features: weights not loaded");
  if (!img_chw || capacity <= 0 || H < 32 || W < 32) return ctx->fail(DC_E_INVALID, "dc_extract_features: bad arguments");
  DCCHK(check_image_size(ctx, H, W, "dc_extract_features"));
  const Dest dst{boxes, nullptr, feats, K, nullptr, capacity};
  return run_images(ctx, &img_chw, &H, &W, 1, img_on_device, true, MODE_FEATURES, &dst);
}

int dc_extract_features_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int on_dev,
                               int capacity, float* boxes, float* feats, int32_t* K) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_extract_features_images: weights not loaded");
  if (!imgs || !H || !W || n <= 0 || capacity <= 0 || !boxes || !feats || !K)
    return ctx->fail(DC_E_INVALID, "dc_extract_features_images: bad arguments");
  for (int i = 0; i < n; ++i) {
    if (!imgs[i] || H[i] < 32 || W[i] < 32)
      return ctx->fail(DC_E_INVALID, "dc_extract_features_images: image %d: null pointer or side below 32 px", i);
    DCCHK(check_image_size(ctx, H[i], W[i], "dc_extract_features_images"));
  }
  std::vector<Dest> dst(n);
  for (int i = 0; i < n; ++i)      // image i: `capacity` rows further on in each array
    dst[i] = Dest{boxes + (size_t)i * capacity * 4, nullptr, feats + (size_t)i * capacity * ctx->D, K + i, nullptr, capacity};
  return run_images(ctx, imgs, H, W, n, on_dev, false, MODE_FEATURES, dst.data());
}

// The checks every entry point on caller-supplied boxes makes before anything is enqueued (docs/SEMANTICS.md): image i's list
// has 1 .. P boxes (P = the row capacity of a forward of that size) with finite coordinates and w, h > 0, and the rows fit
// `cap(i)`, the capacity of the result that receives them.
static int check_box_lists(dc_ctx* ctx, const char* who, const float* const* imgs, const int* H, const int* W, int n,
                           const dc_box_list* bl, int flags, const std::function<int(int)>& cap) {
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!imgs || !H || !W || !bl || n <= 0) return ctx->fail(DC_E_INVALID, "%s: bad arguments (null pointer or n <= 0)", who);
  if (flags & ~DC_BOXES_CLIP) return ctx->fail(DC_E_INVALID, "%s: unknown flags 0x%x (DC_BOXES_CLIP is the only one)", who, flags);
  for (int i = 0; i < n; ++i) {
    if (!imgs[i] || H[i] < 32 || W[i] < 32) return ctx->fail(DC_E_INVALID, "%s: image %d: null pointer or side below 32 px", who, i);
    DCCHK(check_image_size(ctx, H[i], W[i], who));
    const int P = effective_proposals(ctx, H[i], W[i]);
    if (!bl[i].boxes || bl[i].n < 1) return ctx->fail(DC_E_INVALID, "%s: image %d: a box list needs boxes and n >= 1 (got n = %d)", who, i, (int)bl[i].n);
    if (bl[i].n > P)
      return ctx->fail(DC_E_INVALID, "%s: image %d: %d boxes exceed the row capacity %d of a forward; raise num_proposals with dc_set_test_args",
                       who, i, (int)bl[i].n, P);
    if (cap(i) < bl[i].n)
      return ctx->fail(DC_E_INVALID, "%s: image %d: capacity %d is below its %d boxes", who, i, cap(i), (int)bl[i].n);
    for (int b = 0; b < bl[i].n; ++b) {
      const float* x = bl[i].boxes + (size_t)b * 4;
      if (!(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]) && std::isfinite(x[3]) && x[2] > 0.f && x[3] > 0.f))
        return ctx->fail(DC_E_INVALID, "%s: image %d: box %d (%g, %g, %g, %g) needs finite xc, yc and finite w, h > 0", who, i, b,
                         (double)x[0], (double)x[1], (double)x[2], (double)x[3]);
    }
  }
  return DC_OK;
}

// dc_forward_boxes (one image) and dc_forward_boxes_images; `who` names the entry point in the messages
static int forward_boxes(dc_ctx* ctx, const char* who, const float* const* imgs, const int* H, const int* W, int n, int on_dev,
                         const dc_box_list* bl, int flags, dc_result* outs) {
  if (!ctx) return DC_E_INVALID;
  if (!outs) return ctx->fail(DC_E_INVALID, "%s: null results", who);
  DCCHK(check_box_lists(ctx, who, imgs, H, W, n, bl, flags, [&](int i) { return (int)outs[i].capacity; }));
  std::vector<Dest> dst = result_dests(outs, n);
  bool decode = false;                   // no result wants tokens: the language model is not run (as in dc_score_captions)
  for (int i = 0; i < n; ++i) { dst[i].src = bl[i].src; decode = decode || outs[i].tokens != nullptr; }
  return run_images(ctx, imgs, H, W, n, on_dev, false, decode ? MODE_RESULTS : MODE_NO_DECODE, dst.data(),
                    BoxSource{bl, (flags & DC_BOXES_CLIP) != 0});
}

int dc_forward_boxes_images(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int on_dev,
                            const dc_box_list* bl, int flags, dc_result* outs) {
  return forward_boxes(ctx, "dc_forward_boxes_images", imgs, H, W, n, on_dev, bl, flags, outs);
}
int dc_forward_boxes(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_box_list* bl, int flags,
                     dc_result* out) {
  return forward_boxes(ctx, "dc_forward_boxes", &img_chw, &H, &W, 1, img_on_device, bl, flags, out);
}

int dc_extract_features_boxes(dc_ctx* ctx, const float* const* imgs, const int* H, const int* W, int n, int on_dev,
                              const dc_box_list* bl, int flags, int capacity, float* boxes, float* feats, int32_t* K) {
  if (!ctx) return DC_E_INVALID;
  if (!boxes || !feats || !K) return ctx->fail(DC_E_INVALID, "dc_extract_features_boxes: null output");
  DCCHK(check_box_lists(ctx, "dc_extract_features_boxes", imgs, H, W, n, bl, flags, [&](int) { return capacity; }));
  std::vector<Dest> dst(n);
  for (int i = 0; i < n; ++i)
    dst[i] = Dest{boxes + (size_t)i * capacity * 4, nullptr, feats + (size_t)i * capacity * ctx->D, K + i, nullptr, capacity, bl[i].src};
  return run_images(ctx, imgs, H, W, n, on_dev, false, MODE_FEATURES, dst.data(), BoxSource{bl, (flags & DC_BOXES_CLIP) != 0});
}

// run_model.lua:67-74 on the device.  Synchronous; runs on the ctx's primary stream.
int dc_preprocess_size(int H0, int W0, int image_size, int* H, int* W) {
  if (H0 <= 0 || W0 <= 0 || image_size <= 0 || !H || !W) return DC_E_INVALID;
  preprocess_scaled_size(H0, W0, image_size, H, W);
  return (*H >= 1 && *W >= 1) ? DC_OK : DC_E_INVALID;
}

int dc_preprocess_u8(dc_ctx* ctx, const uint8_t* rgb_hwc, int H0, int W0, int on_device, int image_size, float* out_chw_dev,
                     uint8_t* scaled_rgb_dev) {
  if (!ctx) return DC_E_INVALID;
  if (!rgb_hwc || !out_chw_dev || H0 <= 0 || W0 <= 0 || image_size <= 0 || (size_t)H0 * W0 > ((size_t)1 << 28))
    return ctx->fail(DC_E_INVALID, "dc_preprocess_u8: bad arguments");
  int oh = 0, ow = 0;
  preprocess_scaled_size(H0, W0, image_size, &oh, &ow);
  if (oh < 1 || ow < 1) return ctx->fail(DC_E_INVALID, "dc_preprocess_u8: a %dx%d image scaled to %d leaves no pixels", W0, H0, image_size);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  const uint8_t* src = rgb_hwc;
  if (!on_device) {
    const size_t nb = (size_t)H0 * W0 * 3;
    HIPCHK(ctx->pre_src.grow(nb, s));
    HIPCHK(hipMemcpyAsync(ctx->pre_src.get(), rgb_hwc, nb, hipMemcpyHostToDevice, s));
    src = static_cast<const uint8_t*>(ctx->pre_src.get());
  }
  HIPCHK(ctx->pre_scratch.grow(preprocess_scratch_bytes(H0, W0, oh, ow), s));
  const int key[4] = {H0, W0, oh, ow};
  if (ctx->pre_taps.get() == nullptr || memcmp(key, ctx->pre_key, sizeof key) != 0) {
    // new sizes: rebuild the tables (round-5 advisor finding: they were rebuilt, uploaded from pageable memory and waited
    // for on every frame).  The host copy is replaced only after the stream has drained its previous upload.
    HIPCHK(hipStreamSynchronize(s));
    ctx->pre_taps_host.resize(preprocess_taps_bytes(oh, ow));
    preprocess_make_taps(H0, W0, oh, ow, ctx->pre_taps_host.data());
    HIPCHK(ctx->pre_taps.grow(ctx->pre_taps_host.size(), s));
    HIPCHK(hipMemcpyAsync(ctx->pre_taps.get(), ctx->pre_taps_host.data(), ctx->pre_taps_host.size(), hipMemcpyHostToDevice, s));
    memcpy(ctx->pre_key, key, sizeof key);
  }
  const float mean_bgr[3] = {103.939f, 116.779f, 123.68f};          // run_model.lua:73
  KCHK(launch_preprocess_u8(src, H0, W0, oh, ow, mean_bgr, ctx->pre_scratch.get(), ctx->pre_taps.get(), out_chw_dev, scaled_rgb_dev, s));
  HIPCHK(hipStreamSynchronize(s));
  return DC_OK;
}

int dc_stage_times(dc_ctx* ctx, const char** names, float* ms, int max_stages) {
  if (!ctx) return DC_E_INVALID;
  if (ctx->lanes.empty() || !ctx->lanes[0]->have_times) return 0;
  const int n = std::min(max_stages, (int)ST_COUNT);
  for (int i = 0; i < n; ++i) {
    if (names) names[i] = kStageNames[i];
    if (ms) ms[i] = ctx->lanes[0]->stage_ms[i];
  }
  return n;
}

int dc_mfma_profile(dc_ctx* ctx, int reset, int64_t* launches, double* total_ms, double* total_flops) {
  if (!ctx) return DC_E_INVALID;
  if (launches) *launches = ctx->prof_launches;
  if (total_ms) *total_ms = ctx->prof_ms;
  if (total_flops) *total_flops = ctx->prof_flops;
  if (reset) {
    ctx->prof_launches = 0; ctx->prof_ms = 0; ctx->prof_flops = 0;
    ctx->prof = reset > 0;   // reset=1: (re)start profiling; reset=-1: stop
  }
  return DC_OK;
}

// the noise of caption sampling as the device computes it (dc_debug_fetch "sample_gumbel@..." / "sample_bits@..."):
// what 0: host_out[i] = g of the 23-bit index first + i; what 1: host_out[i] = the Philox word of (s, r, t, v) = srtv[4i..4i+3]
static int64_t sample_noise_debug(dc_ctx* ctx, int what, uint64_t seed, const int32_t* srtv, uint32_t first, int64_t count,
                                  void* host_out) {
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  if (!host_out || count < 0 || count > ((int64_t)1 << 23) || (what != 0 && what != 1) || (what == 1 && !srtv) ||
      (what == 0 && (int64_t)first + count > ((int64_t)1 << 23)))
    return ctx->fail(DC_E_INVALID, "dc_debug_fetch: sample noise: at most 2^23 values, indices below 2^23");
  if (count == 0) return 0;
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc((size_t)count * (what == 1 ? 20 : 4)));
  void* dev = block.get();
  if (what == 0) {
    KCHK(launch_sample_noise_gumbel(first, (size_t)count, static_cast<float*>(dev), s));
  } else {
    int32_t* kd = reinterpret_cast<int32_t*>(static_cast<char*>(dev) + (size_t)count * 4);
    HIPCHK(hipMemcpyAsync(kd, srtv, (size_t)count * 16, hipMemcpyHostToDevice, s));
    KCHK(launch_sample_noise_bits(seed, kd, (size_t)count, static_cast<uint32_t*>(dev), s));
  }
  HIPCHK(hipMemcpyAsync(host_out, dev, (size_t)count * 4, hipMemcpyDeviceToHost, s));
  DCCHK(call_finish(ctx, s, DC_OK, "dc_debug_fetch: sample noise"));
  return count;
}


int64_t dc_debug_fetch(dc_ctx* ctx, const char* name, void* host_buf, int64_t capacity_bytes) {
  if (!ctx || !name || !host_buf) return DC_E_INVALID;
  if (strncmp(name, "sample_gumbel@", 14) == 0 || strncmp(name, "sample_bits@", 12) == 0) {
    // the number behind the '@': decimal digits only, nothing after them, no overflow
    const bool bits = name[7] == 'b';
    const char* num = name + (bits ? 12 : 14);
    char* end = nullptr;
    errno = 0;
    const unsigned long long val = strtoull(num, &end, 10);
    if (*num < '0' || *num > '9' || *end != '\0' || errno != 0 || (!bits && val >= (1ull << 23)))
      return ctx->fail(DC_E_INVALID, "dc_debug_fetch: '%s': a decimal %s must follow the '@'", name, bits ? "64-bit seed" : "index below 2^23");
    if (!bits) return sample_noise_debug(ctx, 0, 0, nullptr, (uint32_t)val, capacity_bytes / 4, host_buf);
    const int64_t count = capacity_bytes / 16;
    std::vector<int32_t> coords(static_cast<const int32_t*>(host_buf), static_cast<const int32_t*>(host_buf) + count * 4);
    return sample_noise_debug(ctx, 1, val, coords.data(), 0, count, host_buf);
  }
  if (strcmp(name, "decode_screen_routes") == 0) {
    if (capacity_bytes < 8) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    static_cast<int32_t*>(host_buf)[0] = ctx->lm_parts;
    static_cast<int32_t*>(host_buf)[1] = (int32_t)ctx->lm_screened;
    return 2;
  }
  if (strcmp(name, "train_step_ms") == 0) {          // the last dc_train_step: backward (the three stages), Adam launch, refresh
    if (capacity_bytes < 12) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    memcpy(host_buf, ctx->train_clock.ms, 12);
    return 3;
  }
  if (strcmp(name, "cnn_grad_ms") == 0) {            // the last dc_op_cnn_grad: the kept-activation forward, the backward
    if (capacity_bytes < 8) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    if (!ctx->cnn_clock.ran) return ctx->fail(DC_E_STATE, "dc_debug_fetch: no dc_op_cnn_grad has run");
    static_cast<float*>(host_buf)[0] = ctx->cnn_clock.ms[0];
    static_cast<float*>(host_buf)[1] = ctx->cnn_clock.ms[2];
    return 2;
  }
  if (strcmp(name, "cnn_x4") == 0 || strcmp(name, "cnn_feat") == 0) {      // what the last dc_forward_backward_cnn kept
    const bool x4 = name[4] == 'x';
    if (ctx->cnn_x4 == nullptr) return ctx->fail(DC_E_STATE, "dc_debug_fetch: no dc_forward_backward_cnn has run");
    int fh = ctx->cnn_h4, fw = ctx->cnn_w4;
    if (!x4) { fh = ((fh + 1) / 2 + 1) / 2; fw = ((fw + 1) / 2 + 1) / 2; }
    const int64_t elems = (int64_t)fh * fw * (x4 ? 128 : 512);
    if (elems * 4 > capacity_bytes) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small (%lld needed)", (long long)elems * 4);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_buf, x4 ? ctx->cnn_x4 : ctx->cnn_feat, elems * 4, hipMemcpyDeviceToHost));
    return elems;
  }
  if (strcmp(name, "train_cnn_t") == 0) {          // the CNN's own step count; -1 before the first non-zero dc_train_set_cnn
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = ctx->training && ctx->train_cnn_nseg > 0 ? ctx->train_cnn_t : -1;
    return 1;
  }
  if (strcmp(name, "train_t") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = ctx->training ? ctx->train_t : -1;
    return 1;
  }
  if (strcmp(name, "scratch") == 0) {
    if (capacity_bytes < 24) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    const int64_t v[3] = {ctx->scratch.live, ctx->scratch.kept_bytes, ctx->scratch.kept_allocs};
    memcpy(host_buf, v, sizeof v);
    return 3;
  }
  if (strncmp(name, "lm_op_", 6) == 0) {            // what the last dc_op_lm_sample kept (dc_debug_set "lm_op_keep")
    const struct { const char* n; const std::vector<char>* v; int esize; } kept[] = {
        {"lm_op_h", &ctx->lm_op_h, 4}, {"lm_op_c", &ctx->lm_op_c, 4}, {"lm_op_scores", &ctx->lm_op_scores, 2},
        {"lm_op_cand", &ctx->lm_op_cand, 4}, {"lm_op_best", &ctx->lm_op_best, 4}};
    for (const auto& e : kept) {
      if (strcmp(name, e.n) != 0) continue;
      if (e.v->empty()) return ctx->fail(DC_E_STATE, "dc_debug_fetch: %s: nothing kept (lm_op_keep, then dc_op_lm_sample)", name);
      if ((int64_t)e.v->size() > capacity_bytes) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small (%lld needed)", (long long)e.v->size());
      memcpy(host_buf, e.v->data(), e.v->size());
      return (int64_t)(e.v->size() / e.esize);
    }
    return ctx->fail(DC_E_INVALID, "dc_debug_fetch: unknown name '%s'", name);
  }
  if (ctx->lanes.empty() || !ctx->lanes[0]->arena.p) return ctx->fail(DC_E_STATE, "no forward has run yet");
  Lane& L = *ctx->lanes[0];
  const int P = L.P;
  if (strncmp(name, "loss_", 5) == 0) {             // the record of the last training forward (include/densecap.h, at dc_forward_losses)
    const TrainFwd& k = ctx->train;
    const int64_t kn = k.np + k.nn;
    if (!k.valid) return ctx->fail(DC_E_STATE, "dc_debug_fetch: %s: no dc_forward_losses call has got that far", name);
    if (strcmp(name, "loss_stage_ms") == 0) {
      if (capacity_bytes < 20) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
      memcpy(host_buf, k.stage_ms, 20);
      return 5;
    }
    const struct { const char* n; const void* p; int64_t elems; int esize; } kept[] = {
        {"loss_rpn_boxes", k.boxes, (int64_t)k.A * 4, 4},     {"loss_rpn_anchors", k.anchors, (int64_t)k.A * 4, 4},
        {"loss_rpn_trans", k.trans, (int64_t)k.A * 4, 4},     {"loss_rpn_scores", k.scores, (int64_t)k.A * 2, 4},
        {"loss_obj", L.obj, kn, 4},                           {"loss_final_trans", L.final_trans, kn * 4, 4},
        {"loss_roi_boxes", L.roi_boxes, kn * 4, 4},           {"loss_codes", L.codes, kn * ctx->D, 4},
        {"loss_fc6_out", L.fc6_out, kn * ctx->D, 4},
        {"loss_rowlik", k.rowlik, (int64_t)k.np, 8},         {"loss_feat", k.kept_feat ? ctx->cnn_feat : L.feat, (int64_t)k.h * k.w * 512, 4}};
    for (const auto& e : kept) {
      if (strcmp(name, e.n) != 0) continue;
      const int64_t bytes = e.elems * e.esize;
      if (bytes > capacity_bytes) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small (%lld needed)", (long long)bytes);
      HIPCHK(hipSetDevice(ctx->device));
      HIPCHK(hipStreamSynchronize(L.stream));
      if (bytes > 0) HIPCHK(hipMemcpy(host_buf, e.p, bytes, hipMemcpyDeviceToHost));
      return e.elems;
    }
    return ctx->fail(DC_E_INVALID, "dc_debug_fetch: unknown name '%s'", name);
  }
  struct Ent { const char* n; const void* p; int64_t elems; int esize; };
  const Ent tab[] = {
      {"feat_hwc", L.feat, (int64_t)L.fh * L.fw * 512, 4},
      {"rpn_heads", L.heads, (int64_t)L.fh * L.fw * 6 * ctx->k, 4},
      {"rpn_boxes", L.rpn_boxes, (int64_t)L.A * 4, 4},
      {"rpn_x1y1x2y2", L.rpn_xyxy, (int64_t)L.A * 4, 4},
      {"rpn_p", L.rpn_p, (int64_t)L.A, 4},
      {"rpn_valid", L.rpn_valid, (int64_t)L.A, 1},
      {"rpn_nms_idx", L.picks1, (int64_t)P, 4},
      {"rpn_nms_count", L.count1, 1, 4},
      {"roi_boxes", L.roi_boxes, (int64_t)P * 4, 4},
      {"roi_feats", L.roi_feats, (int64_t)P * 49 * 512, 4},
      {"codes", L.codes, (int64_t)P * ctx->D, 4},
      {"obj", L.obj, (int64_t)P, 4},
      {"final_trans", L.final_trans, (int64_t)P * 4, 4},
      {"final_boxes", L.final_boxes, (int64_t)P * 4, 4},
      {"final_x1y1x2y2", L.final_xyxy, (int64_t)P * 4, 4},
      {"seq", L.seq, (int64_t)P * ctx->T, 4},
      {"final_nms_idx", L.picks2, (int64_t)P, 4},
      {"final_nms_count", L.count2, 1, 4},
      // language-model state of image 0's rows (reference order: row = RoI; captions after the final NMS: row = final rank)
      {"lm_enc", L.enc, (int64_t)P * ctx->E, 4},
      {"lm_h", L.hstate, (int64_t)P * ctx->Hd, 4},
      {"lm_c", L.cstate, (int64_t)P * ctx->Hd, 4},
      // screened decode: candidate count of every (row, step) of the lane's whole group (-1: non-finite; > 64: scanned exactly)
      {"decode_screen_cand", L.scr_cand, (int64_t)L.G * P * ctx->T, 4},
      {"survivor_rows", L.surv_total, 1, 4},
      {"box_src", L.box_src, (int64_t)P, 4},
  };
  if (strcmp(name, "host_enqueue_us") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = (int32_t)(ctx->host_enqueue_ms * 1000.0);
    return 1;
  }
  if (strcmp(name, "graph_launches") == 0 || strcmp(name, "graph_captures") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = name[6] == 'l' ? ctx->graph_launches : ctx->graph_captures;
    return 1;
  }
  if (strcmp(name, "graph_replay_on") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = ctx->graphs ? 1 : 0;
    if (!ctx->graphs && !ctx->graph_note.empty()) ctx->err = ctx->graph_note;      // readable through dc_last_error
    return 1;
  }
  if (strcmp(name, "fault_word") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    int32_t v = -1;
    if (ctx->fault_dev != nullptr) {
      HIPCHK(hipSetDevice(ctx->device));
      HIPCHK(hipStreamSynchronize(L.stream));
      HIPCHK(hipMemcpy(&v, ctx->fault_dev, 4, hipMemcpyDeviceToHost));
    }
    *static_cast<int32_t*>(host_buf) = v;
    return 1;
  }
  if (strcmp(name, "arena_allocs") == 0) {
    if (capacity_bytes < 4) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small");
    *static_cast<int32_t*>(host_buf) = ctx->arena_allocs;
    return 1;
  }
  for (const Ent& e : tab) {
    if (strcmp(e.n, name) == 0) {
      const int64_t bytes = e.elems * e.esize;
      if (bytes > capacity_bytes) return ctx->fail(DC_E_INVALID, "dc_debug_fetch: buffer too small (%lld needed)", (long long)bytes);
      HIPCHK(hipSetDevice(ctx->device));
      HIPCHK(hipStreamSynchronize(L.stream));
      HIPCHK(hipMemcpy(host_buf, e.p, bytes, hipMemcpyDeviceToHost));
      return e.elems;
    }
  }
  return ctx->fail(DC_E_INVALID, "dc_debug_fetch: unknown name '%s'", name);
}

int dc_debug_plan_gemm(int64_t M, int64_t N, int64_t K, int64_t plan_M, int conv_cin, int argmax, int serial_mode,
                       int32_t* out8) {
  if (!out8 || M <= 0 || N <= 0 || K <= 0 || K % 32 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || plan_M < 0 ||
      plan_M > M || (conv_cin != 0 && (conv_cin % 32 || K != 9 * (int64_t)conv_cin)))
    return DC_E_INVALID;
  GemmDesc d;
  static float dummy;                                        // only the POINTER's presence matters to the planner
  d.M = (int)M; d.N = (int)N; d.K = (int)K; d.ldc = (int)N; d.plan_M = (int)plan_M;
  if (conv_cin) { d.conv = 1; d.Cin = conv_cin; }
  if (argmax) d.amax_val = &dummy;
  GemmPlan pl;
  // (DC_PLAN_CU_COUNT: "what would a part with this many CUs be given" -- honoured by THIS query only, never by a launch)
  int cu_override = 0;
  if (const char* e = getenv("DC_PLAN_CU_COUNT")) {
    const int nc = atoi(e);
    if (nc >= 8 && nc <= 4096) cu_override = nc;
  }
  set_planning_cu_override(cu_override);
  mfma_gemm_plan(d, serial_mode != 0, 0, kSplitkWsFloats, &pl);
  set_planning_cu_override(0);
  const int32_t v[8] = {pl.kind, pl.route, pl.stages, pl.splitk, pl.m_split, pl.sk_wgs, pl.sk_np, pl.tail_splitk};
  memcpy(out8, v, sizeof(v));
  return DC_OK;
}

int dc_debug_set(dc_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return DC_E_INVALID;
  if (strcmp(name, "beam_chunk_floats") == 0) {
    if (value < 1) return ctx->fail(DC_E_INVALID, "dc_debug_set: beam_chunk_floats must be >= 1");
    ctx->beam_chunk_floats = value;
    return DC_OK;
  }
  if (strcmp(name, "sample_rows_cap") == 0) {
    if (value < 0) return ctx->fail(DC_E_INVALID, "dc_debug_set: sample_rows_cap must be >= 0 (0 = the default cap)");
    ctx->sample_rows_cap = value;
    return DC_OK;
  }
  if (strcmp(name, "score_rows_cap") == 0) {
    if (value < 0) return ctx->fail(DC_E_INVALID, "dc_debug_set: score_rows_cap must be >= 0 (0 = the default cap)");
    ctx->score_rows_cap = value;
    return DC_OK;
  }
  if (strcmp(name, "lm_op_keep") == 0) {
    if (value != 0 && value != 1) return ctx->fail(DC_E_INVALID, "dc_debug_set: lm_op_keep must be 0 or 1");
    ctx->lm_op_keep = value != 0;
    return DC_OK;
  }
  // the knobs kept in Settings: accepted values lo..hi, except `hole`
  struct Knob { const char* name; int Settings::*field; int lo, hi; const char* accepted; int hole = INT_MIN; };
  static const Knob kKnobs[] = {
      {"nms_band", &Settings::nms_band, 0, 1, "0 or 1"},
      {"v2_stages", &Settings::v2_stages, 0, 3, "0, 2 or 3", 1},
      {"force_cfg", &Settings::force_cfg, 0, 6, "0..6"},
      {"plan_mode", &Settings::plan_mode, -1, 1, "-1, 0 or 1"},
      {"stagger", &Settings::stagger, 0, 4096, "0..4096 (64-cycle sleeps)"},
      {"epi_wide", &Settings::epi_wide, 0, 1, "0 or 1"},
      {"walk", &Settings::walk, 0, 1, "0 or 1"},
      {"bf3_all", &Settings::bf3_all, 0, 1, "0 or 1"},
      {"bf3_presplit", &Settings::bf3_presplit, 0, 1, "0 or 1"},
      {"tail_mode", &Settings::tail_mode, 0, 2, "0, 1 or 2"},
      {"decode_screen", &Settings::decode_screen, -1, 1, "-1, 0 or 1"},
  };
  for (const Knob& k : kKnobs) {
    if (strcmp(name, k.name) != 0) continue;
    if (value < k.lo || value > k.hi || value == k.hole)
      return ctx->fail(DC_E_INVALID, "dc_debug_set: %s must be %s", k.name, k.accepted);
    ctx->cfg.*k.field = (int)value;
    return DC_OK;
  }
  return ctx->fail(DC_E_INVALID, "dc_debug_set: unknown name '%s'", name);
}

// ---- memory helpers ----------------------------------------------------------------------
int dc_malloc(dc_ctx* ctx, void** dev_ptr, size_t bytes) {
  if (!ctx || !dev_ptr) return DC_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMalloc(dev_ptr, bytes ? bytes : 16));
  return DC_OK;
}
int dc_free(dc_ctx* ctx, void* dev_ptr) {
  if (!ctx) return DC_E_INVALID;
  HIPCHK(hipFree(dev_ptr));
  return DC_OK;
}
int dc_memcpy_h2d(dc_ctx* ctx, void* d, const void* h, size_t bytes) {
  if (!ctx) return DC_E_INVALID;
  HIPCHK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  return DC_OK;
}
int dc_memcpy_d2h(dc_ctx* ctx, void* h, const void* d, size_t bytes) {
  if (!ctx) return DC_E_INVALID;
  HIPCHK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
  return DC_OK;
}
int dc_synchronize(dc_ctx* ctx) {
  if (!ctx) return DC_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipDeviceSynchronize());
  return DC_OK;
}


// split-bf16 mode on a per-op call: the caller's weight matrix gets temporary planes in `pl` (the model's own are made once)
static int op_planes(dc_ctx* ctx, hipStream_t s, const float* W, int N, int K, Scratch& pl) {
  if (ctx->cfg.math_mode != DC_MATH_SPLIT_BF16 || !ctx->cfg.bf3_presplit || K % 32) return DC_OK;
  HIPCHK(pl.alloc((size_t)3 * N * K * 2));
  KCHK(launch_split_planes(W, static_cast<uint16_t*>(pl.get()), (size_t)N, K, s));
  return DC_OK;
}

// ---- per-op entry points --------------------------------------------------------------------
#define OP_PROLOGUE()                         \
  if (!ctx) return DC_E_INVALID;              \
  HIPCHK(hipSetDevice(ctx->device));          \
  hipStream_t s;                              \
  DCCHK(lane0_stream(ctx, &s));
#define OP_EPILOGUE()                 \
  HIPCHK(hipStreamSynchronize(s));    \
  prof_collect(ctx);                  \
  return DC_OK;

int dc_op_chw_to_hwc(dc_ctx* ctx, const float* in, float* out, int C, int H, int W) {
  OP_PROLOGUE(); KCHK(launch_chw_to_hwc(in, out, C, H, W, s)); OP_EPILOGUE();
}
int dc_op_hwc_to_chw(dc_ctx* ctx, const float* in, float* out, int C, int H, int W) {
  OP_PROLOGUE(); KCHK(launch_hwc_to_chw(in, out, C, H, W, s)); OP_EPILOGUE();
}
int dc_op_pack_conv3x3_weights(dc_ctx* ctx, const float* w, float* out, int Cout, int Cin) {
  OP_PROLOGUE(); KCHK(launch_pack_conv3x3(w, out, Cout, Cin, s)); OP_EPILOGUE();
}
// A per-op contraction with the weight `w` (N x K): `run(ws, planes)` on the split-K scratch and (split-bf16 mode) temporary
// planes of `w`, then synchronise and read the fault word.  `who` names the entry point in the messages.
static int op_gemm(dc_ctx* ctx, hipStream_t s, const float* w, int N, int K, const char* who,
                   const std::function<int(const Ws&, const uint16_t*)>& run) {
  Scratch ws(ctx->scratch, s), pl(ctx->scratch, s);
  HIPCHK(ws.alloc(kSplitkWsFloats * 4));
  DCCHK(op_planes(ctx, s, w, N, K, pl));
  return call_finish(ctx, s, run(Ws{static_cast<float*>(ws.get()), kSplitkWsFloats}, static_cast<const uint16_t*>(pl.get())), who, true);
}

int dc_op_conv3x3(dc_ctx* ctx, const float* in, const float* w, const float* b, float* out, int n_img, int H, int W,
                  int Cin, int Cout, int relu) {
  OP_PROLOGUE();
  if (Cin % 32 || n_img <= 0 || H <= 0 || W <= 0 || Cout <= 0)
    return ctx->fail(DC_E_INVALID, "dc_op_conv3x3: need Cin %% 32 == 0 and positive sizes");
  return op_gemm(ctx, s, w, Cout, 9 * Cin, "dc_op_conv3x3", [&](const Ws& ws, const uint16_t* pl) {
    return conv3x3(ctx, s, in, w, b, out, n_img, H, W, Cin, Cout, relu, ws, pl);
  });
}
int dc_op_conv3x3_relu_pool(dc_ctx* ctx, const float* in, const float* w, const float* b, float* out, int H, int W,
                            int Cin, int Cout) {
  OP_PROLOGUE();
  if (Cin % 32 || Cout % 4 || H <= 0 || W <= 0 || Cout <= 0)
    return ctx->fail(DC_E_INVALID, "dc_op_conv3x3_relu_pool: need Cin %% 32 == 0, Cout %% 4 == 0 and positive sizes");
  return op_gemm(ctx, s, w, Cout, 9 * Cin, "dc_op_conv3x3_relu_pool", [&](const Ws& ws, const uint16_t* pl) {
    return conv3x3_pool(ctx, s, in, w, b, out, 1, H, W, Cin, Cout, 1, ws, pl);
  });
}
int dc_op_conv3x3_c3(dc_ctx* ctx, const float* in, const float* w, const float* b, float* out, int H, int W, int Cout,
                     int relu) {
  OP_PROLOGUE();
  if (Cout != 64) return ctx->fail(DC_E_UNSUPPORTED, "dc_op_conv3x3_c3: Cout must be 64");
  KCHK(launch_conv3x3_c3(in, w, b, out, 1, H, W, Cout, relu, s));
  OP_EPILOGUE();
}
int dc_op_maxpool2x2_ceil(dc_ctx* ctx, const float* in, float* out, int n_img, int H, int W, int C) {
  OP_PROLOGUE(); KCHK(launch_maxpool2x2_ceil(in, out, n_img, H, W, C, s)); OP_EPILOGUE();
}
int dc_op_linear(dc_ctx* ctx, const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                 int relu) {
  OP_PROLOGUE();
  if (K % 32 || M <= 0 || N <= 0) return ctx->fail(DC_E_INVALID, "dc_op_linear: need K %% 32 == 0");
  return op_gemm(ctx, s, W, N, K, "dc_op_linear", [&](const Ws& ws, const uint16_t* pl) {
    return linear(ctx, s, A, W, bias, C, M, N, K, relu, ws, 0, pl);
  });
}
int dc_op_make_anchors(dc_ctx* ctx, float* out, int h, int w, float x0, float y0, float sx, float sy,
                       const float* anchors_dev, int k) {
  OP_PROLOGUE(); KCHK(launch_make_anchors(out, h, w, x0, y0, sx, sy, anchors_dev, k, s)); OP_EPILOGUE();
}
int dc_op_apply_box_transform(dc_ctx* ctx, const float* boxes, const float* trans, float* out, int n) {
  OP_PROLOGUE(); KCHK(launch_apply_box_transform(boxes, trans, out, n, s)); OP_EPILOGUE();
}
int dc_op_clip_boxes(dc_ctx* ctx, const float* boxes, float* clipped, uint8_t* valid, int n, float x_min, float y_min,
                     float x_max, float y_max) {
  OP_PROLOGUE(); KCHK(launch_clip_boxes(boxes, clipped, valid, n, x_min, y_min, x_max, y_max, s)); OP_EPILOGUE();
}
int dc_op_xcycwh_to_x1y1x2y2(dc_ctx* ctx, const float* boxes, float* out, int n) {
  OP_PROLOGUE(); KCHK(launch_xcycwh_to_x1y1x2y2(boxes, out, n, s)); OP_EPILOGUE();
}
int dc_op_box_iou(dc_ctx* ctx, const float* b1, const float* b2, float* out, int B1, int B2, int convention) {
  OP_PROLOGUE(); KCHK(launch_box_iou(b1, b2, out, B1, B2, convention, s)); OP_EPILOGUE();
}
int dc_op_rpn_decode(dc_ctx* ctx, const float* heads, int h, int w, int k, const float* anchors_dev, float x0,
                     float y0, float sx, float sy, int img_h, int img_w, float* boxes, float* anchors_out,
                     float* trans, float* x1y1x2y2, float* p, uint8_t* valid) {
  OP_PROLOGUE();
  KCHK(launch_rpn_decode(heads, 1, h, w, k, anchors_dev, x0, y0, sx, sy, img_h, img_w, boxes, anchors_out, trans,
                         x1y1x2y2, p, valid, 1, s));
  OP_EPILOGUE();
}
int dc_op_nms(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid, int n, float thresh,
              int max_boxes, int32_t* picks, int32_t* count) {
  OP_PROLOGUE();
  if (n < 0) return ctx->fail(DC_E_INVALID, "dc_op_nms: n must be >= 0");
  if (n == 0) { HIPCHK(hipMemsetAsync(count, 0, 4, s)); OP_EPILOGUE(); }
  Scratch base(ctx->scratch, s);
  HIPCHK(base.alloc(nms_workspace_bytes(n)));
  NmsWorkspace ws;
  nms_workspace_bind(ws, base.get(), n);
  ensure_fault_word(ctx);
  KCHK(launch_nms(ws, boxes, scores, valid, n, nullptr, thresh, max_boxes, picks, count, ctx->cfg.nms_band, s, ctx->fault_dev));
  return call_finish(ctx, s, DC_OK, "dc_op_nms", true);
}
constexpr int kNmsMultiMax = 4096;       // rows and picks of the multi-order NMS (boxes.hip: one 64-bit word of the removed set per lane)
int dc_op_nms_multi(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n, int Q, float thresh,
                    int max_picks, int32_t* picks, int32_t* counts) {
  OP_PROLOGUE();
  if (!boxes || !scores || !picks || !counts) return ctx->fail(DC_E_INVALID, "dc_op_nms_multi: null pointer");
  if (n < 1) return ctx->fail(DC_E_INVALID, "dc_op_nms_multi: n must be >= 1 (got %d)", n);
  if (Q < 1) return ctx->fail(DC_E_INVALID, "dc_op_nms_multi: Q must be >= 1 (got %d)", Q);
  if (max_picks < 1 || max_picks > kNmsMultiMax)
    return ctx->fail(DC_E_INVALID, "dc_op_nms_multi: max_picks must be in 1..%d (got %d)", kNmsMultiMax, max_picks);
  if (n > kNmsMultiMax)
    return ctx->fail(DC_E_UNSUPPORTED, "dc_op_nms_multi: %d boxes exceed the %d the per-query scan holds", n, kNmsMultiMax);
  Scratch ws(ctx->scratch, s);
  HIPCHK(ws.alloc(nms_multi_workspace_bytes(n)));
  KCHK(launch_nms_multi(ws.get(), boxes, scores, valid_or_null, n, nullptr, Q, thresh, max_picks, picks, counts, s));
  return call_finish(ctx, s, DC_OK, "dc_op_nms_multi");
}
constexpr int kEvalMaxDet = 4096, kEvalMaxGt = 512;   // per image (eval_match.hip: the sort keys and the M x M bit mask live in LDS)
// The ABI carries the merge threshold as a float, the reference compares doubles against the literal 0.7: the double with the
// shortest decimal form that reads back as the float (0.7f -> 0.7; docs/SEMANTICS.md, "Evaluation").
static double eval_merge_threshold(float t) {
  char buf[40];
  for (int p = 1; p <= 9; ++p) {
    snprintf(buf, sizeof buf, "%.*g", p, (double)t);
    const double d = strtod(buf, nullptr);
    if ((float)d == t) return d;
  }
  return (double)t;
}
int dc_op_eval_match(dc_ctx* ctx, const float* det_boxes, const float* det_scores, const int32_t* det_off, const float* gt_boxes,
                     const int32_t* gt_off, int n_images, float merge_thresh, int flags, int32_t* order, double* ov, int32_t* group,
                     uint8_t* ok, int32_t* gt_group, int32_t* n_groups, double* merged_boxes) {
  OP_PROLOGUE();
  if (!det_boxes || !det_scores || !det_off || !gt_boxes || !gt_off || !order || !ov || !group || !ok || !gt_group || !n_groups ||
      !merged_boxes)
    return ctx->fail(DC_E_INVALID, "dc_op_eval_match: null pointer");
  if (n_images < 1) return ctx->fail(DC_E_INVALID, "dc_op_eval_match: n_images must be >= 1 (got %d)", n_images);
  if (!(merge_thresh > 0.f && merge_thresh <= 1.f))
    return ctx->fail(DC_E_INVALID, "dc_op_eval_match: merge_thresh must be in (0, 1] (got %g)", (double)merge_thresh);
  if (flags & ~DC_EVAL_CLAIM_LAST) return ctx->fail(DC_E_INVALID, "dc_op_eval_match: unknown flag bits 0x%x", flags);
  // the offsets decide the launch: read them back first (the call is synchronous anyway)
  std::vector<int32_t> off(2 * ((size_t)n_images + 1));
  HIPCHK(hipMemcpyAsync(off.data(), det_off, ((size_t)n_images + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(off.data() + n_images + 1, gt_off, ((size_t)n_images + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int max_b = 0, max_m = 0;
  for (int which = 0; which < 2; ++which) {
    const int32_t* o = off.data() + (size_t)which * (n_images + 1);
    if (o[0] < 0) return ctx->fail(DC_E_INVALID, "dc_op_eval_match: %s[0] is negative", which ? "gt_off" : "det_off");
    for (int i = 0; i < n_images; ++i) {
      if (o[i + 1] < o[i])
        return ctx->fail(DC_E_INVALID, "dc_op_eval_match: %s decreases at image %d", which ? "gt_off" : "det_off", i);
      int& mx = which ? max_m : max_b;
      mx = std::max(mx, (int)(o[i + 1] - o[i]));
    }
  }
  if (max_b > kEvalMaxDet)
    return ctx->fail(DC_E_UNSUPPORTED, "dc_op_eval_match: %d detections in one image exceed the %d the sort holds", max_b, kEvalMaxDet);
  if (max_m > kEvalMaxGt)
    return ctx->fail(DC_E_UNSUPPORTED, "dc_op_eval_match: %d ground-truth boxes in one image exceed the %d the merge holds", max_m,
                     kEvalMaxGt);
  KCHK(launch_eval_match(det_boxes, det_scores, det_off, gt_boxes, gt_off, n_images, max_b, max_m, eval_merge_threshold(merge_thresh),
                         (flags & DC_EVAL_CLAIM_LAST) ? 1 : 0, order, ov, group, ok, gt_group, n_groups, merged_boxes, s));
  OP_EPILOGUE();
}
// The sampler's settings, checked before anything is enqueued (docs/SEMANTICS.md, "Validation losses")
static int check_sampler_opts(dc_ctx* ctx, const dc_loss_opts* o, const char* who) {
  if (o->batch_size < 2 || o->batch_size > 1024 || (o->batch_size & 1))
    return ctx->fail(DC_E_INVALID, "%s: batch_size must be even and in 2..1024 (got %d)", who, o->batch_size);
  if (!(o->low_thresh >= 0.f && o->low_thresh <= 1.f) || !(o->high_thresh >= 0.f && o->high_thresh <= 1.f) ||
      o->low_thresh > o->high_thresh)
    return ctx->fail(DC_E_INVALID, "%s: thresholds must satisfy 0 <= low <= high <= 1 (got low %g, high %g)", who,
                     (double)o->low_thresh, (double)o->high_thresh);
  if (o->remove_outbounds != 0 && o->remove_outbounds != 1)
    return ctx->fail(DC_E_INVALID, "%s: remove_outbounds must be 0 or 1 (got %d)", who, o->remove_outbounds);
  return DC_OK;
}
// The sampler on s with a call's settings and forced lists (checked by the caller); a: its rows, outputs and scratch; fdev: 2048
// ints of device scratch for the forced lists
static int enqueue_box_sampler(dc_ctx* ctx, hipStream_t s, BoxSamplerArgs a, int img_h, int img_w, const dc_loss_opts& o,
                               const dc_sampler_forced* forced, int32_t* fdev) {
  a.x_max = (float)img_w; a.y_max = (float)img_h; a.bounds = o.remove_outbounds;
  a.high = o.high_thresh; a.low = o.low_thresh; a.batch = o.batch_size;
  a.seed_lo = (uint32_t)(o.seed & 0xffffffffull); a.seed_hi = (uint32_t)(o.seed >> 32);
  if (forced && forced->pos_sample_idx) {
    if (forced->num_pos > 0) HIPCHK(hipMemcpyAsync(fdev, forced->pos_sample_idx, (size_t)forced->num_pos * 4, hipMemcpyHostToDevice, s));
    a.forced_pos = fdev; a.n_forced_pos = forced->num_pos;
  }
  if (forced && forced->neg_sample_idx) {
    if (forced->num_neg > 0) HIPCHK(hipMemcpyAsync(fdev + 1024, forced->neg_sample_idx, (size_t)forced->num_neg * 4, hipMemcpyHostToDevice, s));
    a.forced_neg = fdev + 1024; a.n_forced_neg = forced->num_neg;
  }
  KCHK(launch_box_sampler(a, s));
  return DC_OK;
}
int dc_op_box_sampler(dc_ctx* ctx, const float* boxes, const float* gt, int A, int G, int img_h, int img_w, const dc_loss_opts* opts,
                      const dc_sampler_forced* forced, int32_t* pos_input_idx, int32_t* pos_target_idx, int32_t* neg_input_idx,
                      int32_t* counts, float* max_iou, int32_t* arg) {
  OP_PROLOGUE();
  if (!boxes || !gt || !opts || !pos_input_idx || !pos_target_idx || !neg_input_idx || !counts)
    return ctx->fail(DC_E_INVALID, "dc_op_box_sampler: null pointer");
  if (A < 1) return ctx->fail(DC_E_INVALID, "dc_op_box_sampler: A must be >= 1 (got %d)", A);
  if (G < 1 || G > 512) return ctx->fail(DC_E_UNSUPPORTED, "dc_op_box_sampler: G must be in 1..512 (got %d)", G);
  if (img_h < 1 || img_w < 1) return ctx->fail(DC_E_INVALID, "dc_op_box_sampler: image size %dx%d", img_w, img_h);
  DCCHK(check_sampler_opts(ctx, opts, "dc_op_box_sampler"));
  const int np = forced && forced->pos_sample_idx ? forced->num_pos : 0, nn = forced && forced->neg_sample_idx ? forced->num_neg : 0;
  if (np < 0 || np > opts->batch_size || nn < 0 || nn > opts->batch_size)
    return ctx->fail(DC_E_INVALID, "dc_op_box_sampler: a forced list holds 0..batch_size entries (got %d, %d)", np, nn);
  const size_t ws_bytes = box_sampler_ws_bytes(A, G), forced_bytes = (size_t)2048 * 4;
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(ws_bytes + forced_bytes));
  char* ws = static_cast<char*>(block.get());
  BoxSamplerArgs a{};
  a.boxes = boxes; a.gt = gt; a.A = A; a.G = G;
  a.pos_input_idx = pos_input_idx; a.pos_target_idx = pos_target_idx; a.neg_input_idx = neg_input_idx; a.counts = counts;
  a.max_iou_user = max_iou; a.arg_user = arg; a.ws = ws;
  DCCHK(enqueue_box_sampler(ctx, s, a, img_h, img_w, *opts, forced, reinterpret_cast<int32_t*>(ws + ws_bytes)));
  int32_t c[8] = {0};
  HIPCHK(hipMemcpyAsync(c, counts, sizeof c, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (c[5] || c[6])
    return ctx->fail(DC_E_INVALID, "dc_op_box_sampler: %d forced positive and %d forced negative ranks lie outside the candidate lists (%d, %d)",
                     c[5], c[6], c[2], c[3]);
  OP_EPILOGUE();
}
int dc_op_bilinear_roi_pool(dc_ctx* ctx, const float* feat_hwc, int h, int w, int C, const float* boxes, int B,
                            int img_h, int img_w, int HH, int WW, float* out, int out_layout) {
  OP_PROLOGUE();
  if (C % 4 || B <= 0 || HH < 2 || WW < 2) return ctx->fail(DC_E_INVALID, "dc_op_bilinear_roi_pool: bad shape");
  KCHK(launch_bilinear_roi_pool(feat_hwc, h, w, C, boxes, B, nullptr, img_h, img_w, HH, WW, out, out_layout, s));
  OP_EPILOGUE();
}
int dc_op_lm_sample(dc_ctx* ctx, const float* codes, int n, int32_t* tokens) {
  OP_PROLOGUE();
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_op_lm_sample: weights not loaded");
  if (n <= 0) return ctx->fail(DC_E_INVALID, "dc_op_lm_sample: n must be > 0");
  // private scratch for n rows (the beam search brings its own: beam_prepare)
  const size_t E = ctx->E, Hd = ctx->Hd, rows = n;
  LmBufs b{};               // sized as lane_prepare sizes the lane's
  const std::vector<Carve> cv = {
      {(void**)&b.enc, rows * E * 4},  {(void**)&b.gates, rows * 4 * Hd * 4},       {(void**)&b.h, rows * Hd * 4},
      {(void**)&b.c, rows * Hd * 4},   {(void**)&b.amax, rows * lm_amax_floats(ctx) * 4},
      {(void**)&b.hb, rows * ctx->scr_Kp * 2}, {(void**)&b.hnorm, rows * 4}, {(void**)&b.cand, rows * ctx->T * 4}, {(void**)&b.best, rows * 4},
  };
  Scratch base(ctx->scratch, s);
  HIPCHK(base.alloc(cv));
  DCCHK(call_finish(ctx, s,
                    ctx->cfg.beam_size > 0 ? beam_search(ctx, lane0(ctx), s, {ctx->cfg.beam_size, false}, codes, n, {tokens})
                                           : lm_sample(ctx, s, b, lane_ws(lane0(ctx)), codes, n, 0, nullptr, tokens),
                    "dc_op_lm_sample"));
  if (ctx->lm_op_keep && ctx->cfg.beam_size == 0) {
    const bool scr = ctx->lm_screened & 1;      // lm_sample: one part
    const struct { std::vector<char>* v; const void* p; size_t bytes; } keep[] = {
        {&ctx->lm_op_h, b.h, rows * Hd * 4}, {&ctx->lm_op_c, b.c, rows * Hd * 4},
        {&ctx->lm_op_scores, b.amax, scr ? rows * ctx->V1pad * 2 : 0}, {&ctx->lm_op_cand, b.cand, scr ? rows * ctx->T * 4 : 0},
        {&ctx->lm_op_best, b.best, scr ? rows * 4 : 0}};
    for (const auto& k : keep) {
      k.v->resize(k.bytes);
      if (k.bytes) HIPCHK(hipMemcpy(k.v->data(), k.p, k.bytes, hipMemcpyDeviceToHost));
    }
  }
  return DC_OK;
}


int dc_op_lm_score(dc_ctx* ctx, const float* codes, int n, const int32_t* queries, int Q, int Tq, float* loglik) {
  OP_PROLOGUE();
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_op_lm_score: weights not loaded");
  if (!codes || !queries || !loglik) return ctx->fail(DC_E_INVALID, "dc_op_lm_score: null pointer");
  if (n <= 0) return ctx->fail(DC_E_INVALID, "dc_op_lm_score: n must be > 0");
  if (Q < 1 || Tq < 1 || Tq > 64) return check_queries(ctx, nullptr, Q, Tq, "dc_op_lm_score");
  std::vector<int32_t> qh((size_t)Q * Tq);
  HIPCHK(hipMemcpy(qh.data(), queries, qh.size() * 4, hipMemcpyDeviceToHost));
  DCCHK(check_queries(ctx, qh.data(), Q, Tq, "dc_op_lm_score"));
  std::vector<float> out((size_t)n * Q);
  DCCHK(lm_score(ctx, s, codes, n, qh.data(), Q, Tq, out.data(), Q));
  HIPCHK(hipMemcpy(loglik, out.data(), out.size() * 4, hipMemcpyHostToDevice));
  OP_EPILOGUE();
}

// What dc_score_captions and dc_sample_captions (`who`) do before their language-model pass: the forward of dc_forward_test (one
// image: lane 0; without the greedy decode when no tokens are wanted), then the *K rows it returned, compacted from the lane's
// fc7 codes into L.out_feats, its survivor block (the lane is idle once the forward is harvested).  *K = 0: no rows, nothing enqueued.
static int forward_kept_codes(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, dc_result* out, const char* who,
                              int* K) {
  DCCHK(forward_batch(ctx, img_chw, 1, H, W, img_on_device, out, out->tokens == nullptr ? MODE_NO_DECODE : MODE_RESULTS));
  Lane& L = lane0(ctx);
  *K = *reinterpret_cast<const int32_t*>(static_cast<const char*>(L.host_stage) + kRecK);
  if (*K > out->capacity)
    return ctx->fail(DC_E_INVALID, "%s: the image has %d regions but out->capacity is %d", who, *K, (int)out->capacity);
  if (*K > 0)
    KCHK(launch_survivor_compact(L.codes, L.picks2, L.count2, kCountStride, 1, L.P, ctx->D, L.out_feats, L.surv_total, L.stream));
  return DC_OK;
}

int dc_score_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const int32_t* queries, int Q,
                      int Tq, dc_result* out, float* loglik) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "dc_score_captions: weights not loaded");
  if (!img_chw || !queries || !out || !loglik) return ctx->fail(DC_E_INVALID, "dc_score_captions: null pointer");
  DCCHK(check_queries(ctx, queries, Q, Tq, "dc_score_captions"));
  int K = 0;
  DCCHK(forward_kept_codes(ctx, img_chw, H, W, img_on_device, out, "dc_score_captions", &K));
  if (K == 0) return DC_OK;
  Lane& L = lane0(ctx);
  return lm_score(ctx, L.stream, L.out_feats, K, queries, Q, Tq, loglik, Q);
}

// Localising phrases (docs/SEMANTICS.md): the forward of dc_forward_test, then ALL count1 proposal rows -- not only the K the
// final NMS kept -- scored against the queries (lm_score on L.codes: a row's number does not depend on the rows scored with it,
// so it is the number dc_score_captions gives that proposal under final_nms_thresh = 0), then one NMS per query, ordered by the
// query's own column, on the lane's final boxes (launch_nms_multi on L.final_xyxy with the device row count L.count1).  The
// (n, Q) scores reach the host in lm_score and go up again: n * Q floats, next to nothing beside the scoring itself.
int dc_localize_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const int32_t* queries, int Q, int Tq,
                         const dc_localize_opts* opts, dc_result* out, int32_t* count, float* boxes, float* loglik,
                         float* objectness, int32_t* region) {
  const char* who = "dc_localize_captions";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!img_chw || !queries || !opts || !out || !count || !boxes || !loglik || !objectness || !region)
    return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (!(opts->nms_thresh >= 0.f && opts->nms_thresh <= 1.f))
    return ctx->fail(DC_E_INVALID, "%s: nms_thresh must be in [0, 1] (got %g)", who, (double)opts->nms_thresh);
  if (opts->max_regions < 1 || opts->max_regions > kNmsMultiMax)
    return ctx->fail(DC_E_INVALID, "%s: max_regions must be in 1..%d (got %d)", who, kNmsMultiMax, (int)opts->max_regions);
  if (opts->min_objectness != opts->min_objectness) return ctx->fail(DC_E_INVALID, "%s: min_objectness is NaN", who);
  DCCHK(check_queries(ctx, queries, Q, Tq, who));
  if (H < 32 || W < 32) return ctx->fail(DC_E_INVALID, "%s: image side below 32 px", who);
  const int P = effective_proposals(ctx, H, W);
  if (P > kNmsMultiMax)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a forward of %d proposal rows exceeds the %d the per-query NMS holds; cap num_proposals", who,
                     P, kNmsMultiMax);
  DCCHK(forward_batch(ctx, img_chw, 1, H, W, img_on_device, out, out->tokens == nullptr ? MODE_NO_DECODE : MODE_RESULTS));
  Lane& L = lane0(ctx);
  const int K = *reinterpret_cast<const int32_t*>(static_cast<const char*>(L.host_stage) + kRecK);
  if (K > out->capacity)
    return ctx->fail(DC_E_INVALID, "%s: the image has %d regions but out->capacity is %d", who, K, (int)out->capacity);
  const int M = opts->max_regions;
  std::fill(count, count + Q, 0);
  HIPCHK(hipSetDevice(ctx->device));
  int32_t n1 = 0;
  HIPCHK(hipMemcpy(&n1, L.count1, 4, hipMemcpyDeviceToHost));
  const int n = std::max(0, std::min((int)n1, L.P));
  if (K == 0 || n == 0) return DC_OK;
  std::vector<float> ll((size_t)n * Q);
  DCCHK(lm_score(ctx, L.stream, L.codes, n, queries, Q, Tq, ll.data(), Q));
  std::vector<float> fb((size_t)n * 4), obj(n);
  std::vector<int32_t> inv(n, -1), p2(K);
  HIPCHK(hipMemcpy(fb.data(), L.final_boxes, fb.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(obj.data(), L.obj, obj.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(p2.data(), L.picks2, p2.size() * 4, hipMemcpyDeviceToHost));
  for (int k = 0; k < K; ++k)
    if (p2[k] >= 0 && p2[k] < n) inv[p2[k]] = k;              // region: the row of `out` that is the same proposal
  const bool masked = !(std::isinf(opts->min_objectness) && opts->min_objectness < 0.f);
  std::vector<uint8_t> vh(masked ? n : 0);
  for (size_t r = 0; r < vh.size(); ++r) vh[r] = obj[r] >= opts->min_objectness ? 1 : 0;      // (a NaN objectness: invalid)
  float* sc_d = nullptr; uint8_t* valid_d = nullptr; void* mask_d = nullptr; int32_t *picks_d = nullptr, *counts_d = nullptr;
  const std::vector<Carve> cv = {{(void**)&sc_d, ll.size() * 4}, {(void**)&valid_d, (size_t)L.P},
                                 {(void**)&mask_d, nms_multi_workspace_bytes(L.P)}, {(void**)&picks_d, (size_t)Q * M * 4},
                                 {(void**)&counts_d, (size_t)Q * 4}};
  hipStream_t s = L.stream;
  std::vector<int32_t> pk((size_t)Q * M);
  Scratch base(ctx->scratch, s);                 // (made after pk: the stream is drained before pk dies)
  HIPCHK(base.alloc(cv));
  auto body = [&]() -> int {
    HIPCHK(hipMemcpyAsync(sc_d, ll.data(), ll.size() * 4, hipMemcpyHostToDevice, s));
    if (masked) HIPCHK(hipMemcpyAsync(valid_d, vh.data(), vh.size(), hipMemcpyHostToDevice, s));
    KCHK(launch_nms_multi(mask_d, L.final_xyxy, sc_d, masked ? valid_d : nullptr, L.P, L.count1, Q, opts->nms_thresh, M, picks_d,
                          counts_d, s));
    HIPCHK(hipMemcpyAsync(pk.data(), picks_d, pk.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(count, counts_d, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    return DC_OK;
  };
  DCCHK(call_finish(ctx, s, body(), who));
  for (int q = 0; q < Q; ++q)
    for (int j = 0; j < count[q]; ++j) {
      const int r = j < M ? pk[(size_t)q * M + j] : -1;
      if (r < 0 || r >= n) return ctx->fail(DC_E_HIP, "%s: query %d: pick %d of %d is row %d of %d", who, q, j, (int)count[q], r, n);
      const size_t o = (size_t)q * M + j;
      std::copy(fb.begin() + (size_t)r * 4, fb.begin() + (size_t)r * 4 + 4, boxes + o * 4);
      loglik[o] = ll[(size_t)r * Q + q];
      objectness[o] = obj[r];
      region[o] = inv[r];
    }
  return DC_OK;
}

// ---- validation losses (docs/SEMANTICS.md, "Validation losses") -----------------------------------------------------------------
// The settings a losses call runs under, whatever the ctx holds: fp32 MFMA and multi-lane planning (single-image planning shares a
// layer's last tile round along K, another summation order), so that the numbers depend on neither dc_set_math_mode nor
// dc_set_lanes.  The ctx's own settings come back when the guard dies.
static int train_trunk_kept(dc_ctx* ctx, Lane& L, int* fh, int* fw);      // (with the CNN gradients, below)
struct LossCfgGuard {
  Settings& c; Settings saved;
  explicit LossCfgGuard(Settings& cfg) : c(cfg), saved(cfg) { c.math_mode = 0; c.serial_mode = 0; c.plan_mode = 0; }
  ~LossCfgGuard() { c = saved; }
};
static const dc_loss_opts kLossDefaults = {256, 0.7f, 0.3f, 1, 0.05f, 0.1f, 0.1f, 0.1f, 1.0f, 0};

namespace {
// ---- the training path: dc_forward_losses, dc_loss_gradients and dc_forward_backward (at the end of the RPN gradients' section)
// are one, two and three of the stages train_forward, train_recog_lm_backward and train_rpn_backward, in that order, on one
// TrainFwd record; dc_op_recog_grad and dc_op_rpn_grad run the same pieces on a caller's rows.
struct TrainCall {             // the arguments the three entry points share, as the entry point got them (o: resolved)
  const char* who; const float* img; int H, W, on_device; const float* gt_boxes; const int32_t* gt_labels; int G, Lw;
  dc_loss_opts o; const dc_sampler_forced* forced; dc_losses* out; const dc_loss_dump* dump;
  bool cnn = false;            // the trunk keeps conv_net2's activations (dc_forward_backward_cnn)
};
void feature_size(int H, int W, int* h, int* w) {
  for (int i = 0; i < DC_NUM_VGG_CONVS; ++i)
    if (kVgg[i].pool_after) { H = (H + 1) / 2; W = (W + 1) / 2; }
  *h = H; *w = W;
}
int check_gt_boxes(dc_ctx* ctx, const char* who, const float* host_boxes, int G) {
  for (int j = 0; j < G; ++j) {
    const float* b = host_boxes + (size_t)j * 4;
    if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3])) || !(b[2] > 0.f) || !(b[3] > 0.f))
      return ctx->fail(DC_E_INVALID, "%s: ground-truth box %d (%g, %g, %g, %g) is not finite with w > 0 and h > 0", who, j, (double)b[0],
                       (double)b[1], (double)b[2], (double)b[3]);
  }
  return DC_OK;
}
// lists (host): pos_input_idx at 0, pos_target_idx at 1024, neg_input_idx at 2048; the kernels trust them.  code: DC_E_HIP for
// the sampler's own output, DC_E_INVALID for a caller's lists.
int check_sampled_lists(dc_ctx* ctx, const char* who, int code, const int32_t* lists, int np, int nn, int A, int G) {
  for (int r = 0; r < np + nn; ++r) {
    const int i = r < np ? lists[r] : lists[2048 + r - np], j = r < np ? lists[1024 + r] : 0;
    if (i < 0 || i >= A || j < 0 || j >= G)
      return ctx->fail(code, "%s: sampled row %d names input %d of %d, ground-truth box %d of %d", who, r, i, A, j, G);
  }
  return DC_OK;
}
int check_dump(dc_ctx* ctx, const char* who, const dc_loss_dump* dump) {
  if (dump && (!dump->pos_input_idx || !dump->pos_target_idx || !dump->neg_input_idx))
    return ctx->fail(DC_E_INVALID, "%s: a dump needs all three lists", who);
  return DC_OK;
}
int check_forward_args(dc_ctx* ctx, const TrainCall& c) {
  const char* who = c.who;
  if (!c.img || !c.gt_boxes || !c.gt_labels || !c.out) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (c.H < 32 || c.W < 32) return ctx->fail(DC_E_INVALID, "%s: image side below 32 px", who);
  DCCHK(check_image_size(ctx, c.H, c.W, who));
  if (c.G < 1 || c.G > 512) return ctx->fail(DC_E_UNSUPPORTED, "%s: G must be in 1..512 (got %d)", who, c.G);
  DCCHK(check_queries(ctx, c.gt_labels, c.G, c.Lw, who));
  DCCHK(check_gt_boxes(ctx, who, c.gt_boxes, c.G));
  DCCHK(check_sampler_opts(ctx, &c.o, who));
  const int batch = c.o.batch_size;
  const int fnp = c.forced && c.forced->pos_sample_idx ? c.forced->num_pos : 0, fnn = c.forced && c.forced->neg_sample_idx ? c.forced->num_neg : 0;
  if (fnp < 0 || fnp > batch || fnn < 0 || fnn > batch || fnp + fnn > batch)
    return ctx->fail(DC_E_INVALID, "%s: forced lists hold 0..batch_size entries, batch_size in all (got %d, %d)", who, fnp, fnn);
  return check_dump(ctx, who, c.dump);
}
// memset on s of every {pointer, bytes} entry (the gradients of a call with no sampled or no positive row)
int zero_fill(dc_ctx* ctx, hipStream_t s, std::initializer_list<std::pair<void*, size_t>> tab) {
  for (const auto& e : tab)
    if (e.second > 0) HIPCHK(hipMemsetAsync(e.first, 0, e.second, s));
  return DC_OK;
}
// The RPN's training forward (LocalizationLayer.lua:405-412) from a feature map into the given buffers: all A = k * h * w rows,
// not clipped, raw scores.  Launch list: RPN conv; heads; rpn_decode with clip = 0 (boxes, anchors, trans); rpn_score_rows.
int rpn_train_forward(dc_ctx* ctx, Lane& L, const float* feat, int h, int w, int img_h, int img_w, float* hidden, float* heads,
                      float* boxes, float* anchors, float* trans, float* scores) {
  hipStream_t s = L.stream;
  const int k = ctx->k;
  DCCHK(conv3x3(ctx, s, feat, ctx->rpn_w, ctx->rpn_b, hidden, 1, h, w, 512, ctx->R, 1, lane_ws(L)));
  DCCHK(linear(ctx, s, hidden, ctx->heads_w, ctx->heads_b, heads, h * w, 6 * k, ctx->R, 0, Ws(), h * w));
  KCHK(launch_rpn_decode(heads, 1, h, w, k, ctx->anchors, ctx->fc[0], ctx->fc[1], ctx->fc[2], ctx->fc[3], img_h, img_w, boxes, anchors,
                         trans, nullptr, nullptr, nullptr, 0, s));
  KCHK(launch_rpn_score_rows(heads, h, w, k, scores, s));
  return DC_OK;
}
// fc6, fc7 and the recognition heads on the n pooled rows of L.roi_feats (their boxes in L.roi_boxes), planned for `batch` rows.
// With dc_set_dropout's p > 0: Dropout layer 1 in place on fc6_out and layer 2 on codes, masks by `seed` (docs/SEMANTICS.md,
// "Dropout"); at p = 0 no launch is added.
int recog_rows_forward(dc_ctx* ctx, Lane& L, int n, int batch, uint64_t seed) {
  hipStream_t s = L.stream;
  const int D = ctx->D;
  const float p = ctx->cfg.dropout_p;
  DCCHK(linear(ctx, s, L.roi_feats, ctx->fc6_w, ctx->fc6_b, L.fc6_out, n, D, 49 * 512, 1, lane_ws(L), batch));
  if (p > 0.f) KCHK(launch_dropout_rows(L.fc6_out, n, D, (size_t)D, 1, p, seed, s));
  DCCHK(linear(ctx, s, L.fc6_out, ctx->fc7_w, ctx->fc7_b, L.codes, n, D, D, 1, lane_ws(L), batch));
  if (p > 0.f) KCHK(launch_dropout_rows(L.codes, n, D, (size_t)D, 2, p, seed, s));
  KCHK(launch_recog_heads(L.codes, ctx->head5_w, ctx->head5_b, L.roi_boxes, L.obj, L.final_trans, L.final_boxes, L.final_xyxy, n, D, s));
  return DC_OK;
}
// loss_terms on a record's rows and lists and the sampled rows' recognition outputs; what is null has its term skipped
// (LossTermArgs).  Its six doubles and two counts go through terms / masked (device) into the record.
int enqueue_loss_terms(dc_ctx* ctx, hipStream_t s, TrainFwd& f, const float* roi_boxes, const float* final_trans, const float* obj, int Lw,
                       double* terms, int32_t* masked) {
  const dc_loss_opts& o = f.opts;
  LossTermArgs t{};
  t.scores = f.scores; t.anchors = f.anchors; t.trans = f.trans; t.gt = f.gt; t.roi_boxes = roi_boxes; t.final_trans = final_trans;
  t.obj = obj; t.pos_input_idx = f.pos_idx; t.pos_target_idx = f.pos_tgt; t.neg_input_idx = f.neg_idx; t.rowlik = f.rowlik;
  t.num_pos = f.np; t.num_neg = f.nn; t.L = Lw;
  t.w_mid_box = o.mid_box_reg_weight; t.w_mid_obj = o.mid_objectness_weight; t.w_end_box = o.end_box_reg_weight;
  t.w_end_obj = o.end_objectness_weight; t.w_cap = o.captioning_weight;
  t.out = terms; t.out_masked = masked;
  KCHK(launch_loss_terms(t, s));
  HIPCHK(hipMemcpyAsync(f.terms, terms, sizeof f.terms, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(f.masked, masked, sizeof f.masked, hipMemcpyDeviceToHost, s));
  return DC_OK;
}

// The training forward of one image and its five criteria: LocalizationLayer:_forward_train (LocalizationLayer.lua:383-527) and
// DenseCapModel:forward_backward's forward half (DenseCapModel.lua:401-459).  The caller has checked c, holds LossCfgGuard and
// has prepared lane 0 for (H, W, batch_size).  Launch list (lane 0's stream, eager):
//   image copy; the trunk (enqueue_trunk); rpn_train_forward
//   memset + box_sampler_match + box_sampler_draw; the counts and lists come back (the host sizes the rest by them)
//   bilinear RoI pooling of the n = num_pos + num_neg sampled boxes (gathered by the kernel); recog_rows_forward
//   lm_score_paired on the num_pos positive rows (its own scratch; the row sums come back and go up again: num_pos doubles)
//   loss_terms (one workgroup); six doubles and two counts come back
int train_forward(dc_ctx* ctx, const TrainCall& c, Lane& L, TrainFwd& f) {
  const char* who = c.who;
  const dc_loss_opts& o = c.o;
  const int H = c.H, W = c.W, G = c.G, Lw = c.Lw, batch = o.batch_size, A = L.A;
  hipStream_t s = L.stream;
  f.valid = false;
  // ---- scratch: what the lane does not hold (kept for the later stages and dc_debug_fetch "loss_*" until the next call) ----
  void* samp_ws = nullptr;
  int32_t *fdev = nullptr, *counts = nullptr, *sel = nullptr, *masked = nullptr;
  double* terms = nullptr;
  const std::vector<Carve> cv = {
      {(void**)&f.boxes, (size_t)A * 16},  {(void**)&f.anchors, (size_t)A * 16}, {(void**)&f.trans, (size_t)A * 16},
      {(void**)&f.scores, (size_t)A * 8},  {(void**)&f.gt, (size_t)G * 16},      {(void**)&samp_ws, box_sampler_ws_bytes(A, G)},
      {(void**)&fdev, 2048 * 4},           {(void**)&f.pos_idx, 1024 * 4},       {(void**)&f.pos_tgt, 1024 * 4},
      {(void**)&f.neg_idx, 1024 * 4},      {(void**)&counts, 8 * 4},             {(void**)&sel, 1024 * 4},
      {(void**)&f.rowlik, 1024 * 8},       {(void**)&terms, 6 * 8},              {(void**)&masked, 2 * 4},
  };
  HIPCHK(ctx->loss_ws.grow(carve(cv, nullptr), s));
  carve(cv, ctx->loss_ws.get());
  f.A = A; f.G = G; f.H = H; f.W = W; f.opts = o;
  int32_t* const lists = f.lists.data();
  std::vector<double> rl;
  auto body = [&]() -> int {
    HIPCHK(hipEventRecord(L.ev[0], s));
    HIPCHK(hipMemcpyAsync(L.img, c.img, (size_t)3 * H * W * 4, c.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    f.kept_feat = c.cnn;
    if (c.cnn) DCCHK(train_trunk_kept(ctx, L, &f.h, &f.w));
    else DCCHK(enqueue_trunk(ctx, L, 1, &f.h, &f.w));
    const int h = f.h, w = f.w;
    ensure_fault_word(ctx);
    DCCHK(rpn_train_forward(ctx, L, L.feat, h, w, H, W, L.rpn_hidden, L.heads, f.boxes, f.anchors, f.trans, f.scores));
    HIPCHK(hipEventRecord(L.ev[1], s));
    // ---- the sampler ----
    HIPCHK(hipMemcpyAsync(f.gt, c.gt_boxes, (size_t)G * 16, hipMemcpyHostToDevice, s));
    BoxSamplerArgs a{};
    a.boxes = f.boxes; a.gt = f.gt; a.A = A; a.G = G;
    a.pos_input_idx = f.pos_idx; a.pos_target_idx = f.pos_tgt; a.neg_input_idx = f.neg_idx; a.counts = counts; a.ws = samp_ws;
    DCCHK(enqueue_box_sampler(ctx, s, a, H, W, o, c.forced, fdev));
    HIPCHK(hipMemcpyAsync(f.counts, counts, sizeof f.counts, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lists, f.pos_idx, 1024 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lists + 1024, f.pos_tgt, 1024 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lists + 2048, f.neg_idx, 1024 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(L.ev[2], s));
    HIPCHK(hipStreamSynchronize(s));
    const int np = f.np = f.counts[0], nn = f.nn = f.counts[1];
    if (f.counts[5] || f.counts[6])
      return ctx->fail(DC_E_INVALID, "%s: %d forced positive and %d forced negative ranks lie outside the candidate lists (%d, %d)", who,
                       f.counts[5], f.counts[6], f.counts[2], f.counts[3]);
    const int n = np + nn;
    if (np < 0 || nn < 0 || n > batch)
      return ctx->fail(DC_E_INVALID, "%s: the forced lists give %d + %d sampled rows, more than batch_size = %d", who, np, nn, batch);
    DCCHK(check_sampled_lists(ctx, who, DC_E_HIP, lists, np, nn, A, G));
    if (n > 0) {
      // ---- RoI pooling, fc6 / fc7, recognition heads on the sampled rows, positives first (LocalizationLayer.lua:443-452) ----
      HIPCHK(hipMemcpyAsync(sel, f.pos_idx, (size_t)np * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(sel + np, f.neg_idx, (size_t)nn * 4, hipMemcpyDeviceToDevice, s));
      KCHK(launch_bilinear_roi_pool_group(L.feat, 0, 1, h, w, 512, L.roi_boxes, n, nullptr, 0, sel, f.boxes, 0, H, W, 7, 7, L.roi_feats, 1, s));
      DCCHK(recog_rows_forward(ctx, L, n, batch, o.seed));
    }
    HIPCHK(hipEventRecord(L.ev[3], s));
    // ---- captioning: every positive row against the labels of its ground-truth box ----
    rl.assign(std::max(np, 1), 0.0);
    if (np > 0) {
      std::vector<int32_t> lab((size_t)np * Lw);
      for (int r = 0; r < np; ++r)
        std::copy(c.gt_labels + (size_t)lists[1024 + r] * Lw, c.gt_labels + (size_t)(lists[1024 + r] + 1) * Lw, lab.begin() + (size_t)r * Lw);
      DCCHK(lm_score_paired(ctx, s, L.codes, np, batch, lab.data(), Lw, rl.data()));
      HIPCHK(hipMemcpyAsync(f.rowlik, rl.data(), (size_t)np * 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipEventRecord(L.ev[4], s));
    DCCHK(enqueue_loss_terms(ctx, s, f, L.roi_boxes, L.final_trans, L.obj, Lw, terms, masked));         // the five criteria
    HIPCHK(hipEventRecord(L.ev[5], s));
    HIPCHK(hipStreamSynchronize(s));
    return DC_OK;
  };
  const int rc = body();
  if (rc != DC_OK) { drain_lanes(ctx); prof_collect(ctx); return rc; }
  prof_collect(ctx);
  for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&f.stage_ms[i], L.ev[i], L.ev[i + 1]);
  L.have_times = false;                       // the lane's stage events no longer time a dc_forward_test
  DCCHK(check_fault_word(ctx, who));
  f.valid = true;
  return DC_OK;
}
// dc_losses and the caller's dump from the record
void fill_losses(const TrainFwd& f, dc_losses* out, const dc_loss_dump* dump) {
  out->mid_objectness_loss = f.terms[0]; out->mid_box_reg_loss = f.terms[1]; out->end_objectness_loss = f.terms[2];
  out->end_box_reg_loss = f.terms[3]; out->captioning_loss = f.terms[4]; out->total_loss = f.terms[5];
  out->num_pos = f.np; out->num_neg = f.nn; out->total_pos = f.counts[2]; out->total_neg = f.counts[3];
  out->masked_mid = f.masked[0]; out->masked_end = f.masked[1]; out->flags = f.counts[4];
  if (dump) {
    std::copy(f.lists.begin(), f.lists.begin() + f.np, dump->pos_input_idx);
    std::copy(f.lists.begin() + 1024, f.lists.begin() + 1024 + f.np, dump->pos_target_idx);
    std::copy(f.lists.begin() + 2048, f.lists.begin() + 2048 + f.nn, dump->neg_input_idx);
  }
}
}  // namespace

static int op_lm_sample_n(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                          const dc_sample_trunc* trunc, int32_t* samples, float* logprob, float* sample_logprob, const char* who) {
  OP_PROLOGUE();
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!codes || !samples || !logprob) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n <= 0) return ctx->fail(DC_E_INVALID, "%s: n must be > 0", who);
  DCCHK(check_sample_opts(ctx, opts, who));
  const dc_sample_trunc* route = nullptr;
  DCCHK(check_sample_trunc(ctx, opts, trunc, sample_logprob != nullptr, who, &route));
  std::vector<int32_t> ids;
  if (row_ids != nullptr) {
    ids.resize(n);
    HIPCHK(hipMemcpy(ids.data(), row_ids, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
      if (ids[i] < 0) return ctx->fail(DC_E_INVALID, "%s: row_ids[%d] = %d is negative", who, i, (int)ids[i]);
  }
  const size_t S = (size_t)opts->num_samples;
  std::vector<int32_t> tok((size_t)n * S * ctx->T);
  std::vector<float> lp((size_t)n * S), lq(sample_logprob ? (size_t)n * S : 0);
  DCCHK(lm_sample_n(ctx, s, codes, n, row_ids ? ids.data() : nullptr, *opts, tok.data(), lp.data(), route,
                    sample_logprob ? lq.data() : nullptr));
  HIPCHK(hipMemcpy(samples, tok.data(), tok.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(logprob, lp.data(), lp.size() * 4, hipMemcpyHostToDevice));
  if (sample_logprob) HIPCHK(hipMemcpy(sample_logprob, lq.data(), lq.size() * 4, hipMemcpyHostToDevice));
  OP_EPILOGUE();
}
int dc_op_lm_sample_n_trunc(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                            const dc_sample_trunc* trunc_or_null, int32_t* samples, float* logprob,
                            float* sample_logprob_or_null) {
  return op_lm_sample_n(ctx, codes, n, row_ids, opts, trunc_or_null, samples, logprob, sample_logprob_or_null,
                        "dc_op_lm_sample_n_trunc");
}
int dc_op_lm_sample_n(dc_ctx* ctx, const float* codes, int n, const int32_t* row_ids, const dc_sample_opts* opts,
                      int32_t* samples, float* logprob) {
  return op_lm_sample_n(ctx, codes, n, row_ids, opts, nullptr, samples, logprob, nullptr, "dc_op_lm_sample_n");
}

static int sample_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                           const dc_sample_trunc* trunc, dc_result* out, int32_t* samples, float* logprob, float* sample_logprob,
                           const char* who) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!img_chw || !out || !samples || !logprob) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_sample_opts(ctx, opts, who));
  const dc_sample_trunc* route = nullptr;
  DCCHK(check_sample_trunc(ctx, opts, trunc, sample_logprob != nullptr, who, &route));
  int K = 0;
  DCCHK(forward_kept_codes(ctx, img_chw, H, W, img_on_device, out, who, &K));
  if (K == 0) return DC_OK;
  Lane& L = lane0(ctx);
  return lm_sample_n(ctx, L.stream, L.out_feats, K, nullptr, *opts, samples, logprob, route, sample_logprob);      // r = output row
}
int dc_sample_captions_trunc(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                             const dc_sample_trunc* trunc_or_null, dc_result* out, int32_t* samples, float* logprob,
                             float* sample_logprob_or_null) {
  return sample_captions(ctx, img_chw, H, W, img_on_device, opts, trunc_or_null, out, samples, logprob, sample_logprob_or_null,
                         "dc_sample_captions_trunc");
}
int dc_sample_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_sample_opts* opts,
                       dc_result* out, int32_t* samples, float* logprob) {
  return sample_captions(ctx, img_chw, H, W, img_on_device, opts, nullptr, out, samples, logprob, nullptr, "dc_sample_captions");
}

// The standard search's entry points (the search itself: "beam search: both rules" above).  It always runs in fp32, eagerly.
static int check_beam_opts(dc_ctx* ctx, const dc_beam_opts* o, const char* who) {
  if (!o) return ctx->fail(DC_E_INVALID, "%s: null options", who);
  if (o->beam_size < 1 || o->beam_size > 32 || o->beam_size > ctx->V + 1)
    return ctx->fail(DC_E_INVALID, "%s: beam_size must be in 1..32 and at most the %d output words (got %d)", who, ctx->V + 1,
                     (int)o->beam_size);
  if (o->n_best < 1 || o->n_best > o->beam_size)
    return ctx->fail(DC_E_INVALID, "%s: n_best must be in 1..beam_size = %d (got %d)", who, (int)o->beam_size, (int)o->n_best);
  if (!(o->length_alpha >= 0.f && o->length_alpha <= 2.f))        // NaN fails
    return ctx->fail(DC_E_INVALID, "%s: length_alpha must be in [0, 2] (got %g)", who, (double)o->length_alpha);
  return check_beam_fits(ctx, o->beam_size);
}
// captions (n, n_best, T) and logprob (n, n_best): DEVICE buffers.  Only the launches are enqueued: the caller synchronises.
static int lm_beam_std(dc_ctx* ctx, Lane& L, hipStream_t s, const float* codes, int n, const dc_beam_opts& o, int32_t* captions,
                       float* logprob) {
  Fp32Guard fp32(ctx->cfg);
  return beam_search(ctx, L, s, {o.beam_size, true}, codes, n, {captions, logprob, o.n_best, o.length_alpha});
}
int dc_op_lm_beam_n(dc_ctx* ctx, const float* codes, int n, const dc_beam_opts* opts, int32_t* captions, float* logprob) {
  OP_PROLOGUE();
  const char* who = "dc_op_lm_beam_n";
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!codes || !captions || !logprob) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n <= 0) return ctx->fail(DC_E_INVALID, "%s: n must be > 0", who);
  DCCHK(check_beam_opts(ctx, opts, who));
  return call_finish(ctx, s, lm_beam_std(ctx, lane0(ctx), s, codes, n, *opts, captions, logprob), who);
}
int dc_beam_captions(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const dc_beam_opts* opts, dc_result* out,
                     int32_t* captions, float* logprob) {
  if (!ctx) return DC_E_INVALID;
  const char* who = "dc_beam_captions";
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!img_chw || !out || !captions || !logprob) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_beam_opts(ctx, opts, who));
  int K = 0;
  DCCHK(forward_kept_codes(ctx, img_chw, H, W, img_on_device, out, who, &K));
  if (K == 0) return DC_OK;
  Lane& L = lane0(ctx);
  const size_t N = (size_t)opts->n_best, T = (size_t)ctx->T;
  int32_t* cap_d = nullptr; float* lp_d = nullptr;
  const std::vector<Carve> cv = {{(void**)&cap_d, (size_t)K * N * T * 4}, {(void**)&lp_d, (size_t)K * N * 4}};
  Scratch base(ctx->scratch, L.stream);
  HIPCHK(base.alloc(cv));
  DCCHK(call_finish(ctx, L.stream, lm_beam_std(ctx, L, L.stream, L.out_feats, K, *opts, cap_d, lp_d), who));
  HIPCHK(hipMemcpy(captions, cap_d, (size_t)K * N * T * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(logprob, lp_d, (size_t)K * N * 4, hipMemcpyDeviceToHost));
  return DC_OK;
}

int dc_op_lm_grad(dc_ctx* ctx, const float* codes, int n, const int32_t* labels, int L, float weight, const dc_lm_grads* out,
                  double* loss, double* rowlik_or_null) {
  const char* who = "dc_op_lm_grad";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!codes || !labels || !out || !loss) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (!out->lm_enc_w || !out->lm_enc_b || !out->lm_emb || !out->lstm_w || !out->lstm_b || !out->lm_out_w || !out->lm_out_b)
    return ctx->fail(DC_E_INVALID, "%s: null gradient buffer (only codes may be null)", who);
  if (n < 1 || n > 1024) return ctx->fail(DC_E_INVALID, "%s: n must be in 1..1024 (got %d)", who, n);
  if (L < 1 || L > 64) return ctx->fail(DC_E_INVALID, "%s: L must be in 1..64 (got %d)", who, L);
  if (!std::isfinite(weight)) return ctx->fail(DC_E_INVALID, "%s: weight must be finite", who);
  DCCHK(check_queries(ctx, labels, n, L, who));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  LossCfgGuard guard(ctx->cfg);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  return lm_grad(ctx, s, codes, n, labels, L, weight, *out, loss, rowlik_or_null);
}

// ---- test hooks of the backward kernels (densecap_debug_grad.h) -----------------------------------------------------------------
int dc_debug_wgrad(dc_ctx* ctx, const float* A, const float* B, int M, int N, int K, float* C) {
  OP_PROLOGUE();
  if (!A || !B || !C || M < 1 || N < 1 || K < 1) return ctx->fail(DC_E_INVALID, "dc_debug_wgrad: bad argument");
  Scratch ws(ctx->scratch, s);
  const size_t wf = wgrad_ws_floats(M, N, K);
  if (wf > 0) HIPCHK(ws.alloc(wf * 4));
  KCHK(launch_wgrad(A, N, B, K, M, N, K, C, K, static_cast<float*>(ws.get()), s));
  OP_EPILOGUE();
}
int dc_debug_embed_segsum(dc_ctx* ctx, const float* dx, const int32_t* tok_host, int count, int E, int rows_out, float* demb) {
  OP_PROLOGUE();
  if (!dx || !tok_host || !demb || count < 1 || E < 1 || rows_out < 1) return ctx->fail(DC_E_INVALID, "dc_debug_embed_segsum: bad argument");
  for (int i = 0; i < count; ++i)
    if (tok_host[i] < 1 || tok_host[i] > rows_out) return ctx->fail(DC_E_INVALID, "dc_debug_embed_segsum: token %d outside 1..%d", (int)tok_host[i], rows_out);
  std::vector<int32_t> rows(count), seg, ids;
  for (int i = 0; i < count; ++i) rows[i] = i;
  std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) { return tok_host[a] < tok_host[b]; });
  for (int i = 0; i < count; ++i)
    if (i == 0 || tok_host[rows[i]] != tok_host[rows[i - 1]]) { seg.push_back(i); ids.push_back(tok_host[rows[i]]); }
  seg.push_back(count);
  std::vector<int32_t> ih(rows);
  ih.insert(ih.end(), seg.begin(), seg.end());
  ih.insert(ih.end(), ids.begin(), ids.end());
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(ih.size() * 4));
  int32_t* d = static_cast<int32_t*>(block.get());
  HIPCHK(hipMemcpyAsync(d, ih.data(), ih.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(demb, 0, (size_t)rows_out * E * 4, s));
  KCHK(launch_embed_segsum(dx, E, d, d + count, d + count + seg.size(), (int)ids.size(), demb, s));
  OP_EPILOGUE();
}
int dc_debug_softmax_grad(dc_ctx* ctx, float* x, int rows, int V1, int ld, const int32_t* tgt, float scale, double* lse_out_or_null) {
  OP_PROLOGUE();
  if (!x || !tgt || rows < 1 || V1 < 1 || ld < V1) return ctx->fail(DC_E_INVALID, "dc_debug_softmax_grad: bad argument");
  KCHK(launch_softmax_grad(x, ld, V1, tgt, scale, lse_out_or_null, rows, s));
  OP_EPILOGUE();
}
int dc_debug_lstm_cell_bwd(dc_ctx* ctx, const float* gates_pre, const float* c_prev, const float* c, const float* dh,
                           const float* dc, int rows, int Hd, float* dgates, float* dc_prev) {
  OP_PROLOGUE();
  if (!gates_pre || !c_prev || !c || !dh || !dc || !dgates || !dc_prev || rows < 1 || Hd < 1)
    return ctx->fail(DC_E_INVALID, "dc_debug_lstm_cell_bwd: bad argument");
  KCHK(launch_lstm_cell_bwd(gates_pre, nullptr, nullptr, c_prev, c, dh, nullptr, dc, dgates, dc_prev, rows, Hd, s));
  OP_EPILOGUE();
}
int dc_debug_lm_grad_stage_ms(dc_ctx* ctx, float* ms) {
  if (!ctx) return DC_E_INVALID;
  if (!ms) return ctx->fail(DC_E_INVALID, "dc_debug_lm_grad_stage_ms: null pointer");
  if (!ctx->lm_grad_clock.ran) return ctx->fail(DC_E_STATE, "dc_debug_lm_grad_stage_ms: no dc_op_lm_grad call has completed");
  memcpy(ms, ctx->lm_grad_clock.ms, 16);
  return 4;
}

// ---- the same kernels on the operand forms the backward passes use (densecap_debug_bwd.h) -----------------------------------------
int dc_debug_wgrad_ld(dc_ctx* ctx, const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc) {
  OP_PROLOGUE();
  if (!A || !B || !C || M < 1 || N < 1 || K < 1 || lda < N || ldb < K || ldc < K)
    return ctx->fail(DC_E_INVALID, "dc_debug_wgrad_ld: bad argument");
  Scratch ws(ctx->scratch, s);
  const size_t wf = wgrad_ws_floats(M, N, K);
  if (wf > 0) HIPCHK(ws.alloc(wf * 4));
  KCHK(launch_wgrad(A, lda, B, ldb, M, N, K, C, ldc, static_cast<float*>(ws.get()), s));
  OP_EPILOGUE();
}
int dc_debug_colsum(dc_ctx* ctx, const float* X, int ldx, int M, int N, float* out) {
  OP_PROLOGUE();
  if (!X || !out || M < 1 || N < 1 || ldx < N) return ctx->fail(DC_E_INVALID, "dc_debug_colsum: bad argument");
  KCHK(launch_colsum(X, ldx, M, N, out, s));
  OP_EPILOGUE();
}
int dc_debug_lstm_cell_bwd_ex(dc_ctx* ctx, const float* gates_pre, const int32_t* tok, const float* xg, int xg_rows,
                              const float* c_prev, const float* c, const float* dh_a, const float* dh_b, const float* dc_in,
                              int rows, int Hd, float* dgates, float* dc_prev) {
  OP_PROLOGUE();
  const char* who = "dc_debug_lstm_cell_bwd_ex";
  if (!gates_pre || !c || (!dh_a && !dh_b) || !dgates || !dc_prev || rows < 1 || Hd < 1 || (tok != nullptr) != (xg != nullptr) ||
      (xg != nullptr && xg_rows < 1))
    return ctx->fail(DC_E_INVALID, "%s: bad argument", who);
  if (tok != nullptr) {                          // the kernel trusts its tokens: the caller's are checked here
    std::vector<int32_t> th(rows);
    HIPCHK(hipMemcpy(th.data(), tok, (size_t)rows * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r)
      if (th[r] < 0 || th[r] > xg_rows) return ctx->fail(DC_E_INVALID, "%s: row %d: token %d outside 0..%d", who, r, (int)th[r], xg_rows);
  }
  KCHK(launch_lstm_cell_bwd(gates_pre, tok, xg, c_prev, c, dh_a, dh_b, dc_in, dgates, dc_prev, rows, Hd, s));
  OP_EPILOGUE();
}

// ---- recognition-net gradients (docs/SEMANTICS.md, "Recognition-net gradients") ------------------------------------
int dc_feature_size(int H, int W, int* h, int* w) {
  if (!h || !w || H < 1 || W < 1) return DC_E_INVALID;
  feature_size(H, W, h, w);
  return DC_OK;
}

// The backward of bilinear RoI pooling on stream s (not synchronised): the tap index in the ctx's own scratch (grow only), the
// scatter sum, the box gradient.  clock (optional): its event `mark` is recorded between the scatter sum and the box gradient.
static int roi_pool_grad(dc_ctx* ctx, hipStream_t s, const float* feat, int h, int w, int C, const float* boxes, int B, int img_h,
                         int img_w, int HH, int WW, const float* dout, float* dfeat, float* dboxes, StageClock<5>* clock = nullptr, int mark = 0) {
  const size_t bytes = roi_grad_ws_bytes(B, HH * WW, h * w, C);
  HIPCHK(ctx->roi_grad_ws.grow(bytes, s));
  const RoiGradWs ws = roi_grad_carve(ctx->roi_grad_ws.get(), B, HH * WW, h * w, C);
  KCHK(launch_roi_tap_index(boxes, B, h, w, img_h, img_w, HH, WW, ws, s));
  KCHK(launch_roi_scatter_sum(dout, B, h, w, C, HH, WW, ws, dfeat, s));
  if (clock != nullptr) HIPCHK(clock->record(mark, s));
  if (dboxes != nullptr) KCHK(launch_roi_box_grad(feat, h, w, C, boxes, B, img_h, img_w, HH, WW, dout, dboxes, s));
  return DC_OK;
}
static int check_roi_grad_shape(dc_ctx* ctx, int h, int w, int C, int B, int HH, int WW, const char* who) {
  if (h < 1 || w < 1 || C < 4 || C % 4 || B < 1 || HH < 2 || WW < 2) return ctx->fail(DC_E_INVALID, "%s: bad shape", who);
  if (HH * WW > 256) return ctx->fail(DC_E_UNSUPPORTED, "%s: HH * WW = %d points, more than the 256 a row may have", who, HH * WW);
  if ((long long)h * w > (1 << 16) || (long long)B * HH * WW * 4 > (1 << 30))      // (the offsets are scanned by ONE workgroup)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a map of %d x %d pixels (at most 65536: the trunk's output for the largest image) or %d rows "
                     "are more than the index takes", who, h, w, B);
  return DC_OK;
}
int dc_op_roi_pool_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, int C, const float* boxes, int B, int img_h, int img_w,
                        int HH, int WW, const float* dout, float* dfeat, float* dboxes_or_null) {
  OP_PROLOGUE();
  const char* who = "dc_op_roi_pool_grad";
  if (!feat_hwc || !boxes || !dout || !dfeat) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_roi_grad_shape(ctx, h, w, C, B, HH, WW, who));
  DCCHK(roi_pool_grad(ctx, s, feat_hwc, h, w, C, boxes, B, img_h, img_w, HH, WW, dout, dfeat, dboxes_or_null));
  OP_EPILOGUE();
}

// What the backward reads of the forward: the lane's kept activations of the n sampled rows (or the caller's own).
struct RecogKept {
  const float *feat; int h, w;
  const float *roi_boxes, *roi_feats, *fc6_out, *codes, *obj, *final_trans;
  const float *target, *g;                   // (np, 4) target boxes; (np, D) gradient of the positive codes or null
  int n, np, img_h, img_w;
  float w_obj, w_box;
};
constexpr int kRecogK6 = 49 * 512;
constexpr size_t kRecogGradMaxScratch = (size_t)8 << 30;
// The scratch of one recog_backward call on n rows, and its carve list (in ctx->recog_ws)
struct RecogScratch {
  float *dobj = nullptr, *dtrans = nullptr, *danchor = nullptr, *dcodes = nullptr, *dx7 = nullptr, *dpool = nullptr, *dw6 = nullptr;
  float *dw5 = nullptr, *db5 = nullptr, *dbox = nullptr, *ws = nullptr, *spare = nullptr;
  int32_t* masked = nullptr;
};
static std::vector<Carve> recog_carve(const dc_ctx* ctx, int n, RecogScratch& r) {
  const size_t D = (size_t)ctx->D, N = (size_t)n;
  const size_t ws_floats = std::max(wgrad_ws_floats(n, ctx->D, ctx->D), wgrad_ws_floats(n, ctx->D, kRecogK6));
  return {
      {(void**)&r.dobj, N * 4},        {(void**)&r.dtrans, N * 16},          {(void**)&r.danchor, N * 16},
      {(void**)&r.dcodes, N * D * 4},  {(void**)&r.dx7, N * D * 4},          {(void**)&r.dpool, N * kRecogK6 * 4},
      {(void**)&r.dw6, D * kRecogK6 * 4}, {(void**)&r.dw5, 5 * D * 4},       {(void**)&r.db5, 256},
      {(void**)&r.dbox, N * 16},       {(void**)&r.ws, ws_floats * 4},       {(void**)&r.spare, 2 * 1024 * 4},
      {(void**)&r.masked, 256},
  };
}
// bytes a call takes: the two transposed weights (kept by the ctx) and the call's scratch
static int check_recog_scratch(dc_ctx* ctx, int n, int h, int w, const char* who) {
  RecogScratch r;
  const size_t D = (size_t)ctx->D;
  const size_t bytes = carve(recog_carve(ctx, n, r), nullptr) + (D * D + D * kRecogK6) * 4 + roi_grad_ws_bytes(n, 49, h * w, 512);
  if (bytes > kRecogGradMaxScratch)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: n = %d rows at fc_dim = %d need %.2f GiB of scratch, more than the %d GiB a call may take", who,
                     n, ctx->D, (double)bytes / (double)((size_t)1 << 30), (int)(kRecogGradMaxScratch >> 30));
  return DC_OK;
}
static int check_recog_out(dc_ctx* ctx, const dc_recog_grads* o, const char* who) {
  if (!o || !o->fc6_w || !o->fc6_b || !o->fc7_w || !o->fc7_b || !o->obj_w || !o->obj_b || !o->boxreg_w || !o->boxreg_b || !o->feat ||
      !o->roi_boxes)
    return ctx->fail(DC_E_INVALID, "%s: null recognition gradient buffer", who);
  return DC_OK;
}

// Launch list (lane 0's stream, eager; the caller holds LossCfgGuard):
//   end_crit_grad; heads_bwd; five small copies into the head outputs
//   relu_mask (fc7); wgrad + colsum (fc7); GEMM on fc7_wT; relu_mask (fc6); wgrad + permute_fc6_back + colsum (fc6)
//   (with dc_set_dropout's p > 0 the two relu_mask launches are relu_dropout_mask: in.codes and in.fc6_out carry the masks)
//   GEMM on fc6_wT: dpool (n, 7, 7, 512)
//   memset + roi_taps + roi_index_scan + roi_place + roi_sort_lists; roi_scatter_sum + roi_chunk_reduce
//   roi_box_grad; add_pos_rows4
static int recog_backward(dc_ctx* ctx, hipStream_t s, const RecogKept& in, const dc_recog_grads& out, int32_t* masked_end) {
  const int D = ctx->D, n = in.n, np = in.np;
  const float drop_p = ctx->cfg.dropout_p;
  if (ctx->fc7_wT == nullptr || ctx->recog_epoch != ctx->weights_epoch) {
    if (ctx->fc7_wT == nullptr) {
      DCCHK(dev_alloc(ctx, (void**)&ctx->fc7_wT, (size_t)D * D * 4));
      DCCHK(dev_alloc(ctx, (void**)&ctx->fc6_wT, (size_t)D * kRecogK6 * 4));
    }
    KCHK(launch_transpose2d(ctx->fc7_w, ctx->fc7_wT, D, D, s));
    KCHK(launch_transpose2d(ctx->fc6_w, ctx->fc6_wT, D, kRecogK6, s));       // (the ctx's fc6_w is point-major: so is dpool)
    ctx->recog_epoch = ctx->weights_epoch;
  }
  RecogScratch r;
  const std::vector<Carve> cv = recog_carve(ctx, n, r);
  HIPCHK(ctx->recog_ws.grow(carve(cv, nullptr), s));               // kept by the context: 0.45 GB at the real model
  carve(cv, ctx->recog_ws.get());
  auto& clock = ctx->recog_clock;
  auto body = [&]() -> int {
    HIPCHK(clock.record(0, s));
    KCHK(launch_end_crit_grad(in.obj, in.final_trans, in.roi_boxes, in.target, n, np, in.w_obj, in.w_box, r.dobj, r.dtrans, r.danchor, r.masked, s));
    KCHK(launch_heads_bwd(in.codes, ctx->head5_w, r.dobj, r.dtrans, in.g, n, np, D, r.dcodes, r.dw5, r.db5, s));
    HIPCHK(hipMemcpyAsync(out.obj_w, r.dw5, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.boxreg_w, r.dw5 + D, (size_t)4 * D * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.obj_b, r.db5, 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.boxreg_b, r.db5 + 1, 16, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(masked_end, r.masked, 4, hipMemcpyDeviceToHost, s));
    if (drop_p > 0.f) KCHK(launch_relu_dropout_mask(r.dcodes, in.codes, (size_t)n * D, drop_p, s));
    else KCHK(launch_relu_mask(r.dcodes, in.codes, (size_t)n * D, s));
    KCHK(launch_wgrad(r.dcodes, D, in.fc6_out, D, n, D, D, out.fc7_w, D, r.ws, s));
    KCHK(launch_colsum(r.dcodes, D, n, D, out.fc7_b, s));
    {
      GemmDesc g;              // d(fc6 output) = d(fc7 pre-activation).W7
      g.A = r.dcodes; g.W = ctx->fc7_wT; g.C = r.dx7; g.M = n; g.N = D; g.K = D; g.ldc = D;
      DCCHK(run_gemm(ctx, g, s));
    }
    if (drop_p > 0.f) KCHK(launch_relu_dropout_mask(r.dx7, in.fc6_out, (size_t)n * D, drop_p, s));
    else KCHK(launch_relu_mask(r.dx7, in.fc6_out, (size_t)n * D, s));
    if (ctx->fc6_grad_engine) {        // the training step updates fc6 where it lives: its gradient stays in the engine's order
      KCHK(launch_wgrad(r.dx7, D, in.roi_feats, kRecogK6, n, D, kRecogK6, out.fc6_w, kRecogK6, r.ws, s));
    } else {
      KCHK(launch_wgrad(r.dx7, D, in.roi_feats, kRecogK6, n, D, kRecogK6, r.dw6, kRecogK6, r.ws, s));
      KCHK(launch_permute_fc6_back(r.dw6, out.fc6_w, D, 512, 49, s));
    }
    KCHK(launch_colsum(r.dx7, D, n, D, out.fc6_b, s));
    HIPCHK(clock.record(1, s));
    {
      GemmDesc g;              // dpool = d(fc6 pre-activation).W6, point-major
      g.A = r.dx7; g.W = ctx->fc6_wT; g.C = r.dpool; g.M = n; g.N = kRecogK6; g.K = D; g.ldc = kRecogK6;
      DCCHK(run_gemm(ctx, g, s));
    }
    HIPCHK(clock.record(2, s));
    DCCHK(roi_pool_grad(ctx, s, in.feat, in.h, in.w, 512, in.roi_boxes, n, in.img_h, in.img_w, 7, 7, r.dpool, out.feat, r.dbox, &clock, 3));
    KCHK(launch_add_pos_rows4(r.dbox, r.danchor, n, np, out.roi_boxes, s));
    HIPCHK(clock.record(4, s));
    HIPCHK(hipStreamSynchronize(s));
    clock.read();
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "recognition backward");
}
// RecogKept of the n rows recog_rows_forward left in lane 0, on the feature map `feat`
static RecogKept recog_kept(const Lane& L, const float* feat, int h, int w, int n, int np, const float* target, const float* g, int img_h,
                            int img_w, const dc_loss_opts& o) {
  return {feat, h, w, L.roi_boxes, L.roi_feats, L.fc6_out, L.codes, L.obj, L.final_trans, target, g, n, np, img_h, img_w,
          o.end_objectness_weight, o.end_box_reg_weight};
}

int dc_op_recog_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const float* roi_boxes, int n, int num_pos,
                     const float* target_boxes, const float* dcodes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null,
                     const dc_recog_grads* out, double* end_objectness_loss, double* end_box_reg_loss, int32_t* masked_end) {
  const char* who = "dc_op_recog_grad";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!feat_hwc || !roi_boxes || !end_objectness_loss || !end_box_reg_loss || !masked_end) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_recog_out(ctx, out, who));
  const dc_loss_opts o = opts_or_null ? *opts_or_null : kLossDefaults;
  DCCHK(check_sampler_opts(ctx, &o, who));
  if (n < 1 || n > 1024) return ctx->fail(DC_E_INVALID, "%s: n must be in 1..1024 (got %d)", who, n);
  if (num_pos < 0 || num_pos > n) return ctx->fail(DC_E_INVALID, "%s: num_pos must be in 0..n = %d (got %d)", who, n, num_pos);
  if (n > o.batch_size) return ctx->fail(DC_E_INVALID, "%s: n = %d rows, more than batch_size = %d", who, n, (int)o.batch_size);
  if (num_pos > 0 && !target_boxes) return ctx->fail(DC_E_INVALID, "%s: positive rows need target boxes", who);
  if (img_h < 32 || img_w < 32) return ctx->fail(DC_E_INVALID, "%s: image side below 32 px", who);
  DCCHK(check_image_size(ctx, img_h, img_w, who));
  DCCHK(check_roi_grad_shape(ctx, h, w, 512, n, 7, 7, who));
  DCCHK(check_recog_scratch(ctx, n, h, w, who));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  LossCfgGuard guard(ctx->cfg);
  Lane& L = lane0(ctx);
  DCCHK(lane_prepare(ctx, L, img_h, img_w, o.batch_size, 1));
  hipStream_t s = L.stream;
  const int np = num_pos;
  if (ctx->row_ramp == nullptr) {            // the targets come gathered: row r's is target_boxes[r]
    std::vector<int32_t> ramp(1024);
    for (int r = 0; r < 1024; ++r) ramp[r] = r;
    DCCHK(dev_alloc(ctx, (void**)&ctx->row_ramp, ramp.size() * 4));
    HIPCHK(hipMemcpy(ctx->row_ramp, ramp.data(), ramp.size() * 4, hipMemcpyHostToDevice));
  }
  double* terms = nullptr;
  int32_t* masked = nullptr;
  const std::vector<Carve> cv = {{(void**)&terms, 6 * 8}, {(void**)&masked, 2 * 4}};
  HIPCHK(ctx->recog_aux_ws.grow(carve(cv, nullptr), s));
  carve(cv, ctx->recog_aux_ws.get());
  TrainFwd f;                                // the rows' targets as a record's ground truth; no RPN rows, no row sums
  f.gt = const_cast<float*>(target_boxes); f.pos_tgt = ctx->row_ramp; f.np = np; f.nn = n - np; f.opts = o;
  // ---- the forward half: the training forward's own pieces on the caller's boxes; loss_terms with its two end terms only ----
  auto fwd = [&]() -> int {
    HIPCHK(hipMemcpyAsync(L.roi_boxes, roi_boxes, (size_t)n * 16, hipMemcpyDeviceToDevice, s));
    KCHK(launch_bilinear_roi_pool(feat_hwc, h, w, 512, L.roi_boxes, n, nullptr, img_h, img_w, 7, 7, L.roi_feats, 1, s));
    DCCHK(recog_rows_forward(ctx, L, n, o.batch_size, o.seed));
    DCCHK(enqueue_loss_terms(ctx, s, f, L.roi_boxes, L.final_trans, L.obj, 1, terms, masked));
    HIPCHK(hipStreamSynchronize(s));
    return DC_OK;
  };
  const int rc = fwd();
  L.have_times = false;
  if (rc != DC_OK) { (void)hipStreamSynchronize(s); prof_collect(ctx); return rc; }
  *end_objectness_loss = f.terms[2];
  *end_box_reg_loss = f.terms[3];
  return recog_backward(ctx, s, recog_kept(L, feat_hwc, h, w, n, np, target_boxes, dcodes_or_null, img_h, img_w, o), *out, masked_end);
}

namespace {
int check_recog_lm_args(dc_ctx* ctx, const TrainCall& c, const dc_recog_grads* rg, const dc_lm_grads* lg) {
  const char* who = c.who;
  if (!c.out) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_recog_out(ctx, rg, who));
  if (!lg || !lg->lm_enc_w || !lg->lm_enc_b || !lg->lm_emb || !lg->lstm_w || !lg->lstm_b || !lg->lm_out_w || !lg->lm_out_b)
    return ctx->fail(DC_E_INVALID, "%s: null language-model gradient buffer (only codes may be null)", who);
  if (c.Lw > 64) return ctx->fail(DC_E_INVALID, "%s: L must be in 1..64 (got %d)", who, c.Lw);
  if (c.H >= 32 && c.W >= 32 && c.o.batch_size >= 2 && c.o.batch_size <= 1024) {
    int fh = 0, fw = 0;
    feature_size(c.H, c.W, &fh, &fw);
    DCCHK(check_recog_scratch(ctx, c.o.batch_size, fh, fw, who));
  }
  return check_dump(ctx, who, c.dump);
}
// The backward of the captioning loss and of the two end criteria on the record's sampled rows (their activations in lane 0):
// lm_grad on the np positive rows, its gradient of their codes added in recog_backward on all n.  No positive row: the
// language model's gradients are zero; no sampled row: the recognition net's too.
int train_recog_lm_backward(dc_ctx* ctx, const TrainCall& c, Lane& L, const TrainFwd& f, const dc_recog_grads& rg, const dc_lm_grads& lg) {
  const int np = f.np, n = np + f.nn, Lw = c.Lw;
  const size_t D = ctx->D, E = ctx->E, Hd = ctx->Hd, V = ctx->V;
  hipStream_t s = L.stream;
  float *gcodes = nullptr, *tgt_dev = nullptr;
  const std::vector<Carve> cv = {{(void**)&gcodes, (size_t)std::max(np, 1) * D * 4}, {(void**)&tgt_dev, (size_t)std::max(np, 1) * 16}};
  HIPCHK(ctx->recog_aux_ws.grow(carve(cv, nullptr), s));
  carve(cv, ctx->recog_aux_ws.get());
  auto body = [&]() -> int {
    if (np > 0) {
      std::vector<int32_t> lab((size_t)np * Lw);
      std::vector<float> tgt((size_t)np * 4);                 // (end_crit_grad takes the positives' targets gathered)
      for (int r = 0; r < np; ++r) {
        const int j = f.lists[1024 + r];
        std::copy(c.gt_labels + (size_t)j * Lw, c.gt_labels + (size_t)(j + 1) * Lw, lab.begin() + (size_t)r * Lw);
        std::copy(c.gt_boxes + (size_t)j * 4, c.gt_boxes + (size_t)(j + 1) * 4, tgt.begin() + (size_t)r * 4);
      }
      HIPCHK(hipMemcpyAsync(tgt_dev, tgt.data(), tgt.size() * 4, hipMemcpyHostToDevice, s));     // (lm_grad synchronises before tgt dies)
      dc_lm_grads lgo = lg;
      lgo.codes = gcodes;
      double cap = 0.0;
      // (lm_grad runs its own teacher-forced forward after train_forward's lm_score_paired; its loss value is not used)
      DCCHK(lm_grad(ctx, s, L.codes, np, lab.data(), Lw, f.opts.captioning_weight, lgo, &cap, nullptr));
      if (lg.codes != nullptr) HIPCHK(hipMemcpyAsync(lg.codes, gcodes, (size_t)np * D * 4, hipMemcpyDeviceToDevice, s));
    } else {
      DCCHK(zero_fill(ctx, s, {{lg.lm_enc_w, E * D * 4}, {lg.lm_enc_b, E * 4}, {lg.lm_emb, (V + 2) * E * 4}, {lg.lstm_w, (E + Hd) * 4 * Hd * 4},
                               {lg.lstm_b, 4 * Hd * 4}, {lg.lm_out_w, (V + 1) * Hd * 4}, {lg.lm_out_b, (V + 1) * 4}}));
    }
    if (n == 0) {
      DCCHK(zero_fill(ctx, s, {{rg.fc6_w, D * kRecogK6 * 4}, {rg.fc6_b, D * 4}, {rg.fc7_w, D * D * 4}, {rg.fc7_b, D * 4}, {rg.obj_w, D * 4},
                               {rg.obj_b, 4}, {rg.boxreg_w, 4 * D * 4}, {rg.boxreg_b, 16}, {rg.feat, (size_t)f.h * f.w * 512 * 4}}));
      HIPCHK(hipStreamSynchronize(s));
      return DC_OK;
    }
    int32_t masked_end = 0;
    return recog_backward(ctx, s, recog_kept(L, L.feat, f.h, f.w, n, np, tgt_dev, np > 0 ? gcodes : nullptr, f.H, f.W, f.opts), rg, &masked_end);
  };
  const int rc = body();
  if (rc != DC_OK) (void)hipStreamSynchronize(s);
  return rc;
}
}  // namespace


// ---- test hooks of the recognition backward (densecap_debug_recog.h) -------------------------------------------------------------
int dc_debug_roi_tap_index(dc_ctx* ctx, const float* boxes, int B, int h, int w, int img_h, int img_w, int HH, int WW,
                           int32_t* tap_pix, float* tap_w, int32_t* start, int32_t* list) {
  OP_PROLOGUE();
  const char* who = "dc_debug_roi_tap_index";
  if (!boxes || !tap_pix || !tap_w || !start || !list) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_roi_grad_shape(ctx, h, w, 4, B, HH, WW, who));
  const int npix = h * w;
  const size_t T = (size_t)B * HH * WW * 4;
  Scratch base(ctx->scratch, s);
  HIPCHK(base.alloc(roi_grad_ws_bytes(B, HH * WW, npix, 4)));
  const RoiGradWs ws = roi_grad_carve(base.get(), B, HH * WW, npix, 4);
  KCHK(launch_roi_tap_index(boxes, B, h, w, img_h, img_w, HH, WW, ws, s));
  HIPCHK(hipMemcpyAsync(tap_pix, ws.tap_pix, T * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(tap_w, ws.tap_w, T * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(start, ws.start, ((size_t)npix + 1) * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(list, ws.list, T * 4, hipMemcpyDeviceToDevice, s));
  OP_EPILOGUE();
}
int dc_debug_end_crit_grad(dc_ctx* ctx, const float* obj, const float* trans, const float* anchors, const float* target, int n,
                           int num_pos, float w_obj, float w_box, float* dobj, float* dtrans, float* danchor, int32_t* masked) {
  OP_PROLOGUE();
  if (!obj || !trans || !anchors || !dobj || !dtrans || !danchor || !masked || n < 1 || n > 1024 || num_pos < 0 || num_pos > n ||
      (num_pos > 0 && !target))
    return ctx->fail(DC_E_INVALID, "dc_debug_end_crit_grad: bad argument");
  KCHK(launch_end_crit_grad(obj, trans, anchors, target, n, num_pos, w_obj, w_box, dobj, dtrans, danchor, masked, s));
  OP_EPILOGUE();
}
int dc_debug_heads_bwd(dc_ctx* ctx, const float* codes, const float* w5, const float* dobj, const float* dtrans,
                       const float* g_or_null, int n, int num_pos, int D, float* dcodes, float* dw5, float* db5) {
  OP_PROLOGUE();
  if (!codes || !w5 || !dobj || !dtrans || !dcodes || !dw5 || !db5 || n < 1 || num_pos < 0 || num_pos > n || D < 1)
    return ctx->fail(DC_E_INVALID, "dc_debug_heads_bwd: bad argument");
  KCHK(launch_heads_bwd(codes, w5, dobj, dtrans, g_or_null, n, num_pos, D, dcodes, dw5, db5, s));
  OP_EPILOGUE();
}
int dc_debug_permute_fc6_back(dc_ctx* ctx, const float* in, float* out, int N, int C, int HW) {
  OP_PROLOGUE();
  if (!in || !out) return ctx->fail(DC_E_INVALID, "dc_debug_permute_fc6_back: null pointer");
  KCHK(launch_permute_fc6_back(in, out, N, C, HW, s));
  OP_EPILOGUE();
}
int dc_debug_recog_grad_stage_ms(dc_ctx* ctx, float* ms) {
  if (!ctx) return DC_E_INVALID;
  if (!ms) return ctx->fail(DC_E_INVALID, "dc_debug_recog_grad_stage_ms: null pointer");
  if (!ctx->recog_clock.ran) return ctx->fail(DC_E_STATE, "dc_debug_recog_grad_stage_ms: no recognition backward has completed");
  memcpy(ms, ctx->recog_clock.ms, 16);
  return 4;
}

// ---- the truncated sampler's test hook (densecap_debug_sample.h) ----------------------------------------------------------------
int dc_debug_sample_trunc_rows(dc_ctx* ctx, const float* logits, int rows, int V1, int ld, const int32_t* keys, int t,
                               uint64_t seed, float temperature, int top_k, float top_p, int32_t* tok_out, int32_t* kept_out,
                               float* theta_out, double* lp_out, double* lq_out) {
  OP_PROLOGUE();
  const char* who = "dc_debug_sample_trunc_rows";
  if (!logits || !keys || !tok_out || !kept_out || !theta_out || !lp_out || !lq_out)
    return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (rows < 1 || V1 < 1 || ld < V1 || t < 1) return ctx->fail(DC_E_INVALID, "%s: rows, V1 >= 1, ld >= V1 and t >= 1 wanted", who);
  if (!(temperature >= 0.01f && temperature <= 100.f))
    return ctx->fail(DC_E_INVALID, "%s: temperature must be in [0.01, 100] (got %g)", who, (double)temperature);
  if (top_k < 0 || top_k > V1) return ctx->fail(DC_E_INVALID, "%s: top_k must be 0 (off) or in 1..%d (got %d)", who, V1, top_k);
  if (!(top_p > 0.f && top_p <= 1.f)) return ctx->fail(DC_E_INVALID, "%s: top_p must be in (0, 1] (got %g)", who, (double)top_p);
  if ((size_t)V1 > sample_trunc_max_vocab())
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a row of %d words does not fit the truncation kernel's LDS row on this device (max %zu)", who,
                     V1, sample_trunc_max_vocab());
  SampleTruncArgs a = {};
  a.logits = logits; a.ld = ld; a.V1 = V1; a.keys = keys; a.t = t;
  a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32);
  a.inv_temp = 1.f / temperature; a.top_k = top_k; a.top_p = top_p; a.end_tok = V1;
  a.seq = tok_out; a.T = 1; a.tpos = 0;
  a.kept_out = kept_out; a.theta_out = theta_out; a.lp_out = lp_out; a.lq_out = lq_out;
  KCHK(launch_sample_trunc_rows(a, rows, s));
  OP_EPILOGUE();
}

// ---- the classic decode step's test hooks (densecap_debug_step.h) -----------------------------------------------------------------
// One GEMM of a step on the caller's operands: the descriptor of decode_step_desc and of its three callers (lm_sample_parts,
// lm_score, lm_sample_n), field for field, through run_gemm without scratch, as a step runs it.
int dc_debug_step_gemm(dc_ctx* ctx, const dc_step_gemm* g) {
  OP_PROLOGUE();
  const char* who = "dc_debug_step_gemm";
  if (!g || !g->A || !g->W) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (g->M < 1 || g->N < 1 || g->K < 1 || g->K % 32 || g->plan_M < 0 || g->plan_M > g->M)
    return ctx->fail(DC_E_INVALID, "%s: M, N, K >= 1, K %% 32 == 0 and plan_M in [0, M] wanted", who);
  const int epi = g->epilogue;
  if (epi < DC_STEP_STORE || epi > DC_STEP_SAMPLE) return ctx->fail(DC_E_INVALID, "%s: unknown epilogue %d", who, epi);
  if (g->amax_cols < 0 || g->amax_n < 0) return ctx->fail(DC_E_INVALID, "%s: amax_cols, amax_n >= 0 wanted", who);
  const bool prefix = g->amax_cols > 0;
  if (epi == DC_STEP_STORE) {
    if (prefix || !g->C || g->ldc < g->N) return ctx->fail(DC_E_INVALID, "%s: a store wants C, ldc >= N and no prefix", who);
  } else {
    if (!g->part || (epi == DC_STEP_ARGMAX && !g->part_idx) || (epi != DC_STEP_ARGMAX && !g->rowidx))
      return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
    if (epi == DC_STEP_SAMPLE && g->t < 1) return ctx->fail(DC_E_INVALID, "%s: t >= 1 wanted", who);
    // the stored half's row length is nothing a launcher can judge; a prefix the launchers refuse never gets as far as a store
    if (prefix && g->C != nullptr && g->amax_cols <= g->N && g->ldc < g->N - g->amax_cols)
      return ctx->fail(DC_E_INVALID, "%s: ldc = %d is below the %d stored columns", who, g->ldc, g->N - g->amax_cols);
    // (the log-sum-exp and sampling launches check their part_ld; the arg-max launch trusts its caller)
    const long cols = prefix ? g->amax_cols : g->N;
    if (epi == DC_STEP_ARGMAX && g->part_ld < 2 * ((cols + 63) / 64))
      return ctx->fail(DC_E_INVALID, "%s: part_ld = %d is below the arg-max's 2 x %ld slots", who, g->part_ld, (cols + 63) / 64);
  }
  if (g->m_dev_or_null) {
    int32_t live = 0;
    HIPCHK(hipMemcpy(&live, g->m_dev_or_null, 4, hipMemcpyDeviceToHost));
    if (live < 0) return ctx->fail(DC_E_INVALID, "%s: *m_dev = %d", who, (int)live);
  }
  GemmDesc v;
  v.A = g->A; v.W = g->W; v.bias = g->bias; v.M = g->M; v.K = g->K; v.plan_M = g->plan_M;
  if (!prefix) {
    v.N = g->N; v.ldc = g->N;
  } else {
    v.N = g->N; v.amax_cols = g->amax_cols; v.amax_n = g->amax_n; v.C = g->C; v.ldc = g->ldc;
  }
  switch (epi) {
    case DC_STEP_STORE:
      v.C = g->C; v.ldc = g->ldc; v.relu = g->relu ? 1 : 0;
      break;
    case DC_STEP_ARGMAX:
      v.amax_val = g->part; v.amax_idx = g->part_idx; v.amax_ld = g->part_ld;
      break;
    case DC_STEP_LSE:
      v.amax_val = g->part; v.amax_ld = g->part_ld; v.rowidx = g->rowidx;
      break;
    default:
      v.amax_val = g->part; v.amax_ld = g->part_ld; v.rowidx = g->rowidx;
      v.samp_t = g->t; v.samp_seed_lo = (uint32_t)(g->seed & 0xffffffffu); v.samp_seed_hi = (uint32_t)(g->seed >> 32);
      v.samp_inv_temp = g->inv_temp;
  }
  v.m_dev = g->m_dev_or_null;
  DCCHK(run_gemm(ctx, v, s));
  OP_EPILOGUE();
}

// One launch of one row tail on the caller's partials.  Every value the tail would turn into an address of xg is checked on the
// host first (the greedy tail does not bound its column: densecap_debug_step.h).
int dc_debug_step_tail(dc_ctx* ctx, const dc_step_tail* a) {
  OP_PROLOGUE();
  const char* who = "dc_debug_step_tail";
  constexpr int32_t kSentinel = 0x7fffffff;
  if (!a) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  const int kind = a->kind;
  if (kind < DC_STEP_TAIL_GREEDY || kind > DC_STEP_TAIL_SAMPLE) return ctx->fail(DC_E_INVALID, "%s: unknown kind %d", who, kind);
  if (a->n < 1 || a->Hd < 1 || a->nslots < 0 || a->xg_rows < 0 || a->T < 1 || a->t < 0 || a->t >= a->T)
    return ctx->fail(DC_E_INVALID, "%s: n, Hd, T >= 1, nslots, xg_rows >= 0 and t in [0, T) wanted", who);
  const bool step = a->gates_pre != nullptr;
  if (step && (!a->c || !a->h)) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  const size_t n = a->n, ns = a->nslots;
  const bool has_part = kind != DC_STEP_TAIL_GREEDY || a->part != nullptr || a->part_idx != nullptr;
  const int per = kind == DC_STEP_TAIL_GREEDY ? 1 : kind == DC_STEP_TAIL_SCORE ? 2 : 5;
  if (has_part && (!a->part || a->ld < per * a->nslots + (kind == DC_STEP_TAIL_SCORE ? 1 : 0)))
    return ctx->fail(DC_E_INVALID, "%s: partials wanted, ld >= %d floats a slot%s", who, per, kind == DC_STEP_TAIL_SCORE ? " + 1" : "");
  auto column_ok = [&](int32_t col) { return col == kSentinel || (col >= 0 && col < a->xg_rows); };
  std::vector<int32_t> host;
  if (kind == DC_STEP_TAIL_GREEDY) {
    if (has_part && (!a->part_idx || !a->seq)) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
    if (a->fixed_tok < 0 || a->fixed_tok > a->xg_rows)
      return ctx->fail(DC_E_INVALID, "%s: fixed_tok = %d is not 0 or a word id in [1, %d]", who, a->fixed_tok, a->xg_rows);
    if (step && !a->xg && (has_part || a->fixed_tok > 0)) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
    if (has_part && ns > 0) {
      host.resize(n * a->ld);
      HIPCHK(hipMemcpy(host.data(), a->part_idx, host.size() * 4, hipMemcpyDeviceToHost));
      for (size_t m = 0; m < n; ++m)
        for (size_t j = 0; j < ns; ++j)
          if (!column_ok(host[m * a->ld + j]))
            return ctx->fail(DC_E_INVALID, "%s: part_idx[%zu][%zu] = %d is not a column in [0, %d) or the sentinel", who, m, j,
                             (int)host[m * a->ld + j], a->xg_rows);
    }
  } else if (kind == DC_STEP_TAIL_SCORE) {
    if (!a->tgt || !a->acc || (step && !a->xg)) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
    host.resize(n);
    HIPCHK(hipMemcpy(host.data(), a->tgt, n * 4, hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n; ++m)
      if (host[m] != a->end_tok && (host[m] < 1 || host[m] > a->xg_rows))
        return ctx->fail(DC_E_INVALID, "%s: tgt[%zu] = %d is not a word id in [1, %d] or end_tok", who, m, (int)host[m], a->xg_rows);
  } else {
    if (!a->acc || !a->fin || !a->seq || (step && !a->xg)) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
    if (a->end_tok < 1 || a->end_tok > a->xg_rows)
      return ctx->fail(DC_E_INVALID, "%s: end_tok = %d is not a word id in [1, %d]", who, a->end_tok, a->xg_rows);
    if (ns > 0) {
      host.resize(n * a->ld);
      HIPCHK(hipMemcpy(host.data(), a->part, host.size() * 4, hipMemcpyDeviceToHost));      // the column travels as a float's bits
      for (size_t m = 0; m < n; ++m)
        for (size_t j = 0; j < ns; ++j)
          if (!column_ok(host[m * a->ld + 5 * j + 3]))
            return ctx->fail(DC_E_INVALID, "%s: the column of part[%zu], slot %zu, = %d is not in [0, %d) or the sentinel", who, m, j,
                             (int)host[m * a->ld + 5 * j + 3], a->xg_rows);
    }
  }
  if (kind == DC_STEP_TAIL_GREEDY) {
    KCHK(launch_lstm_step_tail(has_part ? a->part : nullptr, has_part ? a->part_idx : nullptr, a->nslots, a->ld, a->fixed_tok, a->xg,
                               a->gates_pre, a->c, a->h, a->n, a->n_dev_or_null, a->Hd, a->zero_c ? 1 : 0, a->seq, a->T, a->t, s));
  } else if (kind == DC_STEP_TAIL_SCORE) {
    KCHK(launch_lse_step_tail(a->part, a->nslots, a->ld, a->tgt, a->end_tok, a->xg, a->gates_pre, a->c, a->h, a->acc, a->n, a->Hd, s));
  } else {
    KCHK(launch_sample_step_tail(a->part, a->nslots, a->ld, a->end_tok, a->xg, a->gates_pre, a->c, a->h, a->acc, a->fin, a->seq, a->T,
                                 a->t, a->n, a->Hd, s));
  }
  OP_EPILOGUE();
}

// ---- the forward path's glue kernels, one launch each (densecap_debug_glue.h) -------------------------------------------------------
// These kernels trust picks, indices and counts; the hooks read them back and check every value that would become a row index.
// live[i] = max(0, min(count[i * stride], cap)) of nimg images, read from the device.  who: the kernel sums min(count, cap) into
// row offsets without a lower clamp (the NMS that writes the counts never goes below 0), so a negative count is refused.
static int glue_live_counts(dc_ctx* ctx, const int32_t* count, int stride, int nimg, int cap, std::vector<int32_t>& live,
                            const char* who = nullptr) {
  std::vector<int32_t> host((size_t)(nimg - 1) * stride + 1);
  HIPCHK(hipMemcpy(host.data(), count, host.size() * 4, hipMemcpyDeviceToHost));
  live.resize(nimg);
  for (int i = 0; i < nimg; ++i) {
    const int32_t c = host[(size_t)i * stride];
    if (who != nullptr && c < 0) return ctx->fail(DC_E_INVALID, "%s: count[%d] = %d is below 0", who, i, (int)c);
    live[i] = std::max(0, std::min(c, (int32_t)cap));
  }
  return DC_OK;
}
// idx (nimg blocks of `rows` values): block i's first live[i] values must lie in [0, bound)
static int glue_check_rows(dc_ctx* ctx, const int32_t* idx, int nimg, int rows, const std::vector<int32_t>& live, int bound,
                           const char* who, const char* what) {
  std::vector<int32_t> host((size_t)nimg * rows);
  HIPCHK(hipMemcpy(host.data(), idx, host.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < nimg; ++i)
    for (int r = 0; r < live[i]; ++r) {
      const int32_t v = host[(size_t)i * rows + r];
      if (v < 0 || v >= bound) return ctx->fail(DC_E_INVALID, "%s: %s[%d][%d] = %d is not a row in [0, %d)", who, what, i, r, (int)v, bound);
    }
  return DC_OK;
}

int dc_debug_boxes_ingest(dc_ctx* ctx, const float* in_boxes, const int32_t* in_n, int nimg, int P, int clip, int img_h, int img_w,
                          float* roi_boxes, int32_t* box_src, int32_t* count, int count_stride) {
  OP_PROLOGUE();
  const char* who = "dc_debug_boxes_ingest";
  if (!in_boxes || !in_n || !roi_boxes || !box_src || !count) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (nimg < 1 || nimg > 65535 || P < 1 || (long long)nimg * P > (1 << 28) || img_h < 1 || img_w < 1 || count_stride < 1)
    return ctx->fail(DC_E_INVALID, "%s: nimg in [1, 65535], P, img_h, img_w, count_stride >= 1 wanted", who);
  KCHK(launch_boxes_ingest(in_boxes, in_n, nimg, P, clip ? 1 : 0, img_h, img_w, roi_boxes, box_src, count, count_stride, s));
  OP_EPILOGUE();
}

int dc_debug_roi_pool_group(dc_ctx* ctx, const dc_glue_roi_pool* a) {
  OP_PROLOGUE();
  const char* who = "dc_debug_roi_pool_group";
  if (!a || !a->feat_hwc || !a->boxes || !a->out) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (a->nimg < 1 || a->B < 1 || a->h < 1 || a->w < 1 || a->C < 1 || a->HH < 2 || a->WW < 2 || a->img_h < 2 || a->img_w < 2 ||
      (a->out_layout != 0 && a->out_layout != 1))
    return ctx->fail(DC_E_INVALID, "%s: nimg, B, h, w, C >= 1, HH, WW, img_h, img_w >= 2 and out_layout 0 or 1 wanted", who);
  const long long map = (long long)a->h * a->w * a->C;
  if (map >= (1ll << 31) || (long long)a->nimg * a->B > (1 << 24) || (long long)a->HH * a->WW * a->C >= (1ll << 31))
    return ctx->fail(DC_E_INVALID, "%s: the shape is past the kernel's 32-bit indices", who);
  if (a->nimg > 1 && a->feat_stride < (size_t)map)
    return ctx->fail(DC_E_INVALID, "%s: feat_stride = %zu is below the %lld floats of a map", who, a->feat_stride, map);
  if (a->B_dev != nullptr && a->bdev_stride < 1) return ctx->fail(DC_E_INVALID, "%s: bdev_stride >= 1 wanted", who);
  // a pick list without source boxes is the launcher's to refuse; with them, every pick of a live row is checked here
  if (a->pick != nullptr && a->src_boxes != nullptr) {
    if (a->src_rows < 1) return ctx->fail(DC_E_INVALID, "%s: src_rows >= 1 wanted", who);
    if (a->nimg > 1 && a->src_stride < (size_t)a->src_rows * 4)
      return ctx->fail(DC_E_INVALID, "%s: src_stride = %zu is below the %d source rows", who, a->src_stride, a->src_rows);
    std::vector<int32_t> live(a->nimg, a->B);
    if (a->B_dev != nullptr) DCCHK(glue_live_counts(ctx, a->B_dev, a->bdev_stride, a->nimg, a->B, live));
    DCCHK(glue_check_rows(ctx, a->pick, a->nimg, a->B, live, a->src_rows, who, "pick"));
  }
  KCHK(launch_bilinear_roi_pool_group(a->feat_hwc, a->feat_stride, a->nimg, a->h, a->w, a->C, a->boxes, a->B, a->B_dev, a->bdev_stride,
                                      a->pick, a->src_boxes, a->src_stride, a->img_h, a->img_w, a->HH, a->WW, a->out, a->out_layout, s));
  OP_EPILOGUE();
}

int dc_debug_recog_heads(dc_ctx* ctx, const float* codes, const float* w5, const float* b5, const float* roi, float* obj,
                         float* trans, float* fin, float* fin_xyxy_or_null, int n, int D) {
  OP_PROLOGUE();
  const char* who = "dc_debug_recog_heads";
  if (!codes || !w5 || !b5 || !roi || !obj || !trans || !fin) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n < 1 || n > (1 << 28) || D < 1) return ctx->fail(DC_E_INVALID, "%s: n in [1, 2^28] and D >= 1 wanted", who);
  KCHK(launch_recog_heads(codes, w5, b5, roi, obj, trans, fin, fin_xyxy_or_null, n, D, s));
  OP_EPILOGUE();
}

int dc_debug_iota_count(dc_ctx* ctx, int32_t* idx, int32_t* count_out, const int32_t* count_in, int cap) {
  OP_PROLOGUE();
  const char* who = "dc_debug_iota_count";
  if (!idx || !count_out || !count_in) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (cap < 1) return ctx->fail(DC_E_INVALID, "%s: cap >= 1 wanted", who);
  KCHK(launch_iota_count(idx, count_out, count_in, cap, s));
  OP_EPILOGUE();
}

int dc_debug_gather_rows(dc_ctx* ctx, const void* src, int src_rows, const int32_t* idx, const int32_t* count, int cap, int width,
                         void* out, int is_i32) {
  OP_PROLOGUE();
  const char* who = "dc_debug_gather_rows";
  if (!src || !idx || !count || !out) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (src_rows < 1 || cap < 1 || width < 1 || (long long)cap * width >= (1ll << 31))
    return ctx->fail(DC_E_INVALID, "%s: src_rows, cap, width >= 1 and cap * width < 2^31 wanted", who);
  std::vector<int32_t> live;
  DCCHK(glue_live_counts(ctx, count, 1, 1, cap, live));
  DCCHK(glue_check_rows(ctx, idx, 1, cap, live, src_rows, who, "idx"));
  if (is_i32) KCHK(launch_gather_rows_i32(static_cast<const int32_t*>(src), idx, count, cap, width, static_cast<int32_t*>(out), s));
  else KCHK(launch_gather_rows(static_cast<const float*>(src), idx, count, cap, width, static_cast<float*>(out), s));
  OP_EPILOGUE();
}

int dc_debug_survivor_compact(dc_ctx* ctx, const float* codes, const int32_t* picks, const int32_t* count, int count_stride,
                              int nimg, int P, int D, float* out, int32_t* total) {
  OP_PROLOGUE();
  const char* who = "dc_debug_survivor_compact";
  if (!codes || !picks || !count || !out || !total) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (nimg < 1 || nimg > 65535 || P < 1 || D < 1 || count_stride < 1 || (long long)nimg * P > (1 << 28))
    return ctx->fail(DC_E_INVALID, "%s: nimg in [1, 65535], P, D, count_stride >= 1 wanted", who);
  std::vector<int32_t> live;
  DCCHK(glue_live_counts(ctx, count, count_stride, nimg, P, live, who));
  DCCHK(glue_check_rows(ctx, picks, nimg, P, live, P, who, "picks"));
  KCHK(launch_survivor_compact(codes, picks, count, count_stride, nimg, P, D, out, total, s));
  OP_EPILOGUE();
}

int dc_debug_final_pack(dc_ctx* ctx, const dc_glue_final_pack* a) {
  OP_PROLOGUE();
  const char* who = "dc_debug_final_pack";
  if (!a || !a->final_boxes || !a->obj || !a->picks || !a->count || !a->pack) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if ((a->tokens != nullptr) == (a->codes != nullptr)) return ctx->fail(DC_E_INVALID, "%s: exactly one of tokens and codes wanted", who);
  const int words = a->codes != nullptr ? a->D : a->T;
  if (a->nimg < 1 || a->nimg > 65535 || a->P < 1 || words < 1 || a->count_stride < 1 || (long long)a->nimg * a->P > (1 << 28))
    return ctx->fail(DC_E_INVALID, "%s: nimg in [1, 65535], P, count_stride and the row's T or D >= 1 wanted", who);
  if (a->tokens != nullptr && (a->tok_gather < 0 || a->tok_gather > 2))
    return ctx->fail(DC_E_INVALID, "%s: tok_gather = %d is not 0, 1 or 2", who, a->tok_gather);
  const size_t need = (a->box_src != nullptr ? rec_src(a->P, words) + (size_t)a->P * 4 : rec_src(a->P, words));
  if (a->stride < need || a->stride % 4)
    return ctx->fail(DC_E_INVALID, "%s: stride = %zu is below the record's %zu bytes or no multiple of 4", who, a->stride, need);
  std::vector<int32_t> live;
  DCCHK(glue_live_counts(ctx, a->count, a->count_stride, a->nimg, a->P, live, who));
  DCCHK(glue_check_rows(ctx, a->picks, a->nimg, a->P, live, a->P, who, "picks"));
  KCHK(launch_final_pack(a->final_boxes, a->obj, a->tokens, a->tok_gather, a->codes, a->picks, a->count, a->count_stride, a->fault,
                         a->nimg, a->P, a->T, a->D, a->pack, a->stride, s, a->box_src));
  OP_EPILOGUE();
}

// ---- the two NMS launchers with a device-side row count (densecap_debug_nms.h) -----------------------------------------------------
// dc_op_nms binds a workspace of its own for exactly n rows; the forward binds one for the RPN list and runs the final NMS in it.
// The hook's workspace is a buffer the ctx keeps, bound for ws_rows: a small call after a large one reads the large one's leftovers.
int dc_debug_nms(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n,
                 const int32_t* n_dev_or_null, int ws_rows, float thresh, int max_boxes, int32_t* picks, int32_t* count,
                 int32_t* order_or_null, int32_t* nvalid_or_null) {
  OP_PROLOGUE();
  const char* who = "dc_debug_nms";
  if (!boxes || !scores || !picks || !count) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n < 1) return ctx->fail(DC_E_INVALID, "%s: n must be >= 1 (got %d)", who, n);
  if (ws_rows < n) return ctx->fail(DC_E_INVALID, "%s: ws_rows = %d is below the %d rows of the call", who, ws_rows, n);
  if (max_boxes < -1) return ctx->fail(DC_E_INVALID, "%s: max_boxes must be >= -1 (got %d)", who, max_boxes);
  HIPCHK(ctx->nms_debug_ws.grow(nms_workspace_bytes(ws_rows), s));
  NmsWorkspace ws;
  nms_workspace_bind(ws, ctx->nms_debug_ws.get(), ws_rows);
  ensure_fault_word(ctx);
  KCHK(launch_nms(ws, boxes, scores, valid_or_null, n, n_dev_or_null, thresh, max_boxes, picks, count, ctx->cfg.nms_band, s,
                  ctx->fault_dev));
  if (order_or_null != nullptr) HIPCHK(hipMemcpyAsync(order_or_null, ws.order, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (nvalid_or_null != nullptr) HIPCHK(hipMemcpyAsync(nvalid_or_null, ws.nvalid, 4, hipMemcpyDeviceToDevice, s));
  return call_finish(ctx, s, DC_OK, who, true);
}

int dc_debug_nms_multi(dc_ctx* ctx, const float* boxes, const float* scores, const uint8_t* valid_or_null, int n,
                       const int32_t* n_dev_or_null, int Q, float thresh, int max_picks, int32_t* picks, int32_t* counts) {
  OP_PROLOGUE();
  const char* who = "dc_debug_nms_multi";
  if (!boxes || !scores || !picks || !counts) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n < 1) return ctx->fail(DC_E_INVALID, "%s: n must be >= 1 (got %d)", who, n);
  if (Q < 1) return ctx->fail(DC_E_INVALID, "%s: Q must be >= 1 (got %d)", who, Q);
  if (max_picks < 1 || max_picks > kNmsMultiMax)
    return ctx->fail(DC_E_INVALID, "%s: max_picks must be in 1..%d (got %d)", who, kNmsMultiMax, max_picks);
  if (n > kNmsMultiMax)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: %d boxes exceed the %d the per-query scan holds", who, n, kNmsMultiMax);
  Scratch ws(ctx->scratch, s);
  HIPCHK(ws.alloc(nms_multi_workspace_bytes(n)));
  KCHK(launch_nms_multi(ws.get(), boxes, scores, valid_or_null, n, n_dev_or_null, Q, thresh, max_picks, picks, counts, s));
  return call_finish(ctx, s, DC_OK, who);
}

// ---- beam search test hooks, both rules (densecap_debug.h, densecap_debug_beam.h) ----------------------------------------------
int dc_debug_beam_topk(dc_ctx* ctx, const float* logits, int rows, int V1, int ld, const uint8_t* finished_or_null, int k,
                       float* top_lp, int32_t* top_idx) {
  OP_PROLOGUE();
  if (!logits || !top_lp || !top_idx || rows < 0 || V1 < 1 || ld < V1)
    return ctx->fail(DC_E_INVALID, "dc_debug_beam_topk: bad argument");
  KCHK(launch_beam_logsoftmax_topk(logits, rows, V1, ld, finished_or_null, k, top_lp, top_idx, s));
  OP_EPILOGUE();
}
int dc_debug_beam_merge(dc_ctx* ctx, const float* top_lp, const int32_t* top_idx, const float* beam_lp_in, const int32_t* beams_in,
                        int nprop, int beam, int T, int t, int END, float* beam_lp_out, int32_t* beams_out, int32_t* parent,
                        int32_t* cur_tok, uint8_t* finished) {
  OP_PROLOGUE();
  if (!top_lp || !top_idx || !beam_lp_in || !beams_in || !beam_lp_out || !beams_out || !parent || !cur_tok || !finished ||
      nprop < 1 || T < 1 || t < 0 || t >= T || END < 1)
    return ctx->fail(DC_E_INVALID, "dc_debug_beam_merge: bad argument");
  KCHK(launch_beam_merge(top_lp, top_idx, beam_lp_in, beams_in, nprop, beam, T, t, END, beam_lp_out, beams_out, parent, cur_tok,
                         finished, s));
  OP_EPILOGUE();
}

// The four state hooks run one body: the search's own start and iteration on lane 0's scratch under the caller's BeamRun.  A state
// is a dc_beam_std_state inside, `len` null (and not copied) for the reference rule.
static dc_beam_std_state beam_hook_state(const dc_beam_state* st) {
  return st ? dc_beam_std_state{st->h, st->c, st->beam_lp, st->beams, st->tok, st->parent, st->fin, nullptr} : dc_beam_std_state{};
}
// what they check of a state first; on DC_OK the lane's beam scratch holds nprop proposals
static int beam_hook_prepare(dc_ctx* ctx, BeamRun run, int nprop, const dc_beam_std_state* st, const char* who) {
  if (!st || !st->h || !st->c || !st->beam_lp || !st->beams || !st->tok || !st->parent || !st->fin || (run.standard && !st->len))
    return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (nprop < 1 || beam_chunk(ctx, run, nprop) < nprop)
    return ctx->fail(DC_E_INVALID, "%s: %d proposals are not one chunk (the hook does not chunk)", who, nprop);
  return beam_prepare(ctx, lane0(ctx), run, nprop);
}
// the lane's beam state, sets (hs, bs), to or from the caller's buffers (rows = nprop x beam)
static int beam_hook_copy(dc_ctx* ctx, Lane& L, int rows, int hs, int bs, const dc_beam_std_state& st, bool out, hipStream_t s) {
  const size_t Hd = ctx->Hd, T = ctx->T;
  const struct { void* lane; void* user; size_t bytes; } parts[] = {
      {L.bm_h[hs], st.h, rows * Hd * 4}, {L.bm_c[hs], st.c, rows * Hd * 4},   {L.bm_lp[bs], st.beam_lp, (size_t)rows * 4},
      {L.bm_beams[bs], st.beams, rows * T * 4}, {L.bm_tok, st.tok, (size_t)rows * 4}, {L.bm_parent, st.parent, (size_t)rows * 4},
      {L.bm_fin, st.fin, (size_t)rows}, {L.bs_len[bs], st.len, st.len ? (size_t)rows * 4 : 0}};
  for (const auto& p : parts)
    if (p.bytes) HIPCHK(hipMemcpyAsync(out ? p.user : p.lane, out ? p.lane : p.user, p.bytes, hipMemcpyDeviceToDevice, s));
  return DC_OK;
}
// ... and the top-k lists out
static int beam_hook_lists(dc_ctx* ctx, Lane& L, size_t n, float* top_lp, int32_t* top_idx, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(top_lp, L.bm_top_lp, n * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(top_idx, L.bm_top_idx, n * 4, hipMemcpyDeviceToDevice, s));
  return DC_OK;
}
static int beam_hook_start(dc_ctx* ctx, hipStream_t s, BeamRun run, const float* codes, int nprop, const dc_beam_std_state* out,
                           float* top_lp, int32_t* top_idx, const char* who) {
  DCCHK(beam_hook_prepare(ctx, run, nprop, out, who));
  Lane& L = lane0(ctx);
  DCCHK(beam_start(ctx, L, run, codes, nprop, s));
  DCCHK(beam_hook_copy(ctx, L, nprop * run.beam, beam_state_set(1), beam_beams_set(1), *out, true, s));
  return beam_hook_lists(ctx, L, (size_t)nprop * run.beam, top_lp, top_idx, s);
}
static int beam_hook_step(dc_ctx* ctx, hipStream_t s, BeamRun run, int nprop, int t, const dc_beam_std_state* in,
                          const dc_beam_std_state* out, float* top_lp, int32_t* top_idx, const char* who) {
  DCCHK(beam_hook_prepare(ctx, run, nprop, in, who));
  DCCHK(beam_hook_prepare(ctx, run, nprop, out, who));
  if (t < 1 || t >= ctx->T) return ctx->fail(DC_E_INVALID, "%s: t = %d is not in [1, %d)", who, t, ctx->T);
  Lane& L = lane0(ctx);
  const int rows = nprop * run.beam;
  // the word of a row selects an xg row by address in the step GEMM: the caller's are checked here, as the kernels check their own
  std::vector<int32_t> tok(rows);
  HIPCHK(hipMemcpy(tok.data(), in->tok, (size_t)rows * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < rows; ++i)
    if (tok[i] < 1 || tok[i] > ctx->V + 1)
      return ctx->fail(DC_E_INVALID, "%s: tok[%d] = %d is not a word id in [1, %d]", who, i, (int)tok[i], ctx->V + 1);
  DCCHK(beam_hook_copy(ctx, L, rows, beam_state_set(t), beam_beams_set(t), *in, false, s));
  DCCHK(beam_iter(ctx, L, run, nprop, t, s));
  DCCHK(beam_hook_copy(ctx, L, rows, beam_state_set(t + 1), beam_beams_set(t + 1), *out, true, s));
  return beam_hook_lists(ctx, L, (size_t)rows * run.beam, top_lp, top_idx, s);
}

// the reference-rule hooks run at the width dc_set_beam_size set, in the math mode of dc_set_math_mode
static int beam_ref_hook_run(dc_ctx* ctx, const char* who, BeamRun* run) {
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (ctx->cfg.beam_size < 1) return ctx->fail(DC_E_STATE, "%s: dc_set_beam_size first", who);
  *run = {ctx->cfg.beam_size, false};
  return DC_OK;
}
int dc_debug_beam_start(dc_ctx* ctx, const float* codes, int nprop, const dc_beam_state* state_out, float* top_lp,
                        int32_t* top_idx) {
  OP_PROLOGUE();
  const char* who = "dc_debug_beam_start";
  if (!codes || !top_lp || !top_idx) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  BeamRun run;
  DCCHK(beam_ref_hook_run(ctx, who, &run));
  const dc_beam_std_state out = beam_hook_state(state_out);
  DCCHK(beam_hook_start(ctx, s, run, codes, nprop, &out, top_lp, top_idx, who));
  OP_EPILOGUE();
}
int dc_debug_beam_step(dc_ctx* ctx, int nprop, int t, const dc_beam_state* state_in, const dc_beam_state* state_out,
                       float* top_lp, int32_t* top_idx) {
  OP_PROLOGUE();
  const char* who = "dc_debug_beam_step";
  if (!top_lp || !top_idx) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  BeamRun run;
  DCCHK(beam_ref_hook_run(ctx, who, &run));
  const dc_beam_std_state in = beam_hook_state(state_in), out = beam_hook_state(state_out);
  DCCHK(beam_hook_step(ctx, s, run, nprop, t, &in, &out, top_lp, top_idx, who));
  OP_EPILOGUE();
}

int dc_debug_beam_std_merge(dc_ctx* ctx, const float* top_lp, const int32_t* top_idx, const float* beam_lp_in,
                            const int32_t* beams_in, const int32_t* len_in, const uint8_t* fin_in, int nprop, int beam, int T, int t,
                            int END, float* beam_lp_out, int32_t* beams_out, int32_t* len_out, int32_t* parent, int32_t* cur_tok,
                            uint8_t* fin_out) {
  OP_PROLOGUE();
  if (!top_lp || !top_idx || !beam_lp_in || !beams_in || !len_in || !fin_in || !beam_lp_out || !beams_out || !len_out || !parent ||
      !cur_tok || !fin_out || nprop < 1 || beam < 1 || beam > 32 || T < 1 || t < 0 || t >= T || END < 1)
    return ctx->fail(DC_E_INVALID, "dc_debug_beam_std_merge: bad argument");
  KCHK(launch_beam_std_merge(top_lp, top_idx, beam_lp_in, beams_in, len_in, fin_in, nprop, beam, T, t, END, beam_lp_out, beams_out,
                             len_out, parent, cur_tok, fin_out, s));
  OP_EPILOGUE();
}
int dc_debug_beam_std_finish(dc_ctx* ctx, const float* beam_lp, const int32_t* beams, const int32_t* len, int nprop, int beam, int T,
                             int n_best, float length_alpha, int32_t* captions, float* logprob) {
  OP_PROLOGUE();
  if (!beam_lp || !beams || !len || !captions || !logprob || nprop < 1 || beam < 1 || beam > 32 || T < 1 || n_best < 1 ||
      n_best > beam || !(length_alpha >= 0.f && length_alpha <= 2.f))
    return ctx->fail(DC_E_INVALID, "dc_debug_beam_std_finish: bad argument");
  const std::vector<float> pen = beam_std_pen(T, length_alpha);
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(pen.size() * 4));
  float* pen_d = static_cast<float*>(block.get());
  HIPCHK(hipMemcpy(pen_d, pen.data(), pen.size() * 4, hipMemcpyHostToDevice));
  KCHK(launch_beam_std_finish(beam_lp, beams, len, pen_d, length_alpha != 0.f, nprop, beam, T, n_best, captions, logprob, s));
  OP_EPILOGUE();
}
// the standard hooks take their width as an argument, validated like a call's options, and run in fp32 like the search
static int beam_std_hook_opts(dc_ctx* ctx, int beam, const char* who) {
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  const dc_beam_opts o = {beam, 1, 0.f};
  return check_beam_opts(ctx, &o, who);
}
int dc_debug_beam_std_start(dc_ctx* ctx, const float* codes, int nprop, int beam, const dc_beam_std_state* state_out, float* top_lp,
                            int32_t* top_idx) {
  OP_PROLOGUE();
  const char* who = "dc_debug_beam_std_start";
  if (!codes || !top_lp || !top_idx) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(beam_std_hook_opts(ctx, beam, who));
  Fp32Guard fp32(ctx->cfg);
  DCCHK(beam_hook_start(ctx, s, {beam, true}, codes, nprop, state_out, top_lp, top_idx, who));
  OP_EPILOGUE();
}
int dc_debug_beam_std_step(dc_ctx* ctx, int nprop, int beam, int t, const dc_beam_std_state* state_in,
                           const dc_beam_std_state* state_out, float* top_lp, int32_t* top_idx) {
  OP_PROLOGUE();
  const char* who = "dc_debug_beam_std_step";
  if (!top_lp || !top_idx) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(beam_std_hook_opts(ctx, beam, who));
  Fp32Guard fp32(ctx->cfg);
  DCCHK(beam_hook_step(ctx, s, {beam, true}, nprop, t, state_in, state_out, top_lp, top_idx, who));
  OP_EPILOGUE();
}

// ---- screened greedy decode test hooks (densecap_debug.h) ------------------------------------------------------------------------
static int screen_hook_check(dc_ctx* ctx, int n, const char* who) {
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!screen_fits(ctx))
    return ctx->fail(DC_E_UNSUPPORTED, "%s: no screened route at rnn_size %d, V + 1 = %d (the row tail's LDS does not fit)", who,
                     ctx->Hd, ctx->V + 1);
  if (n < 1) return ctx->fail(DC_E_INVALID, "%s: n must be > 0", who);
  return DC_OK;
}
int dc_debug_screen_scores(dc_ctx* ctx, const float* h, int n, const int32_t* n_dev_or_null, uint16_t* hb_out, float* hnorm_out,
                           void* scores_out) {
  OP_PROLOGUE();
  DCCHK(screen_hook_check(ctx, n, "dc_debug_screen_scores"));
  if (!h || !hb_out || !hnorm_out || !scores_out) return ctx->fail(DC_E_INVALID, "dc_debug_screen_scores: null pointer");
  KCHK(launch_screen_operands(h, n, n_dev_or_null, ctx->Hd, ctx->scr_Kp, hb_out, hnorm_out, s));
  KCHK(launch_decode_screen(hb_out, ctx->scr_w, ctx->out_b, scores_out, n, n_dev_or_null, ctx->V + 1, ctx->V1pad, ctx->scr_Kp, s));
  OP_EPILOGUE();
}
int dc_debug_rescore_tail(dc_ctx* ctx, const void* scores, const float* h, const float* c, const float* hnorm,
                          const float* gates_pre_or_null, int n, const int32_t* n_dev_or_null, int32_t* tok_out,
                          int32_t* cand_out, float* best_out, float* h_out, float* c_out, uint16_t* hb_out, float* hnorm_out) {
  OP_PROLOGUE();
  DCCHK(screen_hook_check(ctx, n, "dc_debug_rescore_tail"));
  const bool step = gates_pre_or_null != nullptr;
  if (!scores || !h || !hnorm || !tok_out || !cand_out || !best_out || (step && (!c || !h_out || !c_out || !hb_out || !hnorm_out)))
    return ctx->fail(DC_E_INVALID, "dc_debug_rescore_tail: null pointer");
  // the tail updates h, c and hnorm in place: with gates it runs on copies, and the live rows of the copies go to the caller
  const size_t Hd = ctx->Hd, rows = n;
  float *hs = nullptr, *cs = nullptr, *ns = nullptr;
  const std::vector<Carve> cv = {{(void**)&hs, rows * Hd * 4}, {(void**)&cs, rows * Hd * 4}, {(void**)&ns, rows * 4}};
  Scratch base(ctx->scratch, s);
  int live = n;
  if (step) {
    if (n_dev_or_null) {
      HIPCHK(hipMemcpy(&live, n_dev_or_null, 4, hipMemcpyDeviceToHost));
      live = std::max(0, std::min(n, live));
    }
    HIPCHK(base.alloc(cv));
  }
  RescoreTail a{};
  a.scores = static_cast<const _Float16*>(scores); a.ld = ctx->V1pad; a.wnorm = reinterpret_cast<const _Float16*>(ctx->scr_wnorm);
  a.W = ctx->out_w; a.bias = ctx->out_b; a.V1 = ctx->V + 1; a.cbound = ctx->scr_c; a.xg = ctx->xg; a.gates_pre = gates_pre_or_null;
  a.h = step ? hs : const_cast<float*>(h); a.c = step ? cs : const_cast<float*>(h);       // (selection only: c is not touched)
  a.hnorm = step ? ns : const_cast<float*>(hnorm);
  a.n = n; a.n_dev = n_dev_or_null; a.Hd = ctx->Hd; a.seq = tok_out; a.T = 1; a.t = 0; a.hb = hb_out; a.Kp = ctx->scr_Kp;
  a.cand = cand_out; a.bestv = best_out;
  const struct { void* scratch; const void* in; void* out; size_t row; } st[] = {
      {hs, h, h_out, Hd * 4}, {cs, c, c_out, Hd * 4}, {ns, hnorm, hnorm_out, 4}};
  if (step)
    for (const auto& p : st) HIPCHK(hipMemcpyAsync(p.scratch, p.in, rows * p.row, hipMemcpyDeviceToDevice, s));
  KCHK(launch_lstm_rescore_tail(a, s));
  if (step && live > 0)
    for (const auto& p : st) HIPCHK(hipMemcpyAsync(p.out, p.scratch, (size_t)live * p.row, hipMemcpyDeviceToDevice, s));
  OP_EPILOGUE();
}

// ---- convolution gradients (docs/SEMANTICS.md, "Convolution gradients") --------------------------------------------
// Can the engine run dx = conv3x3(dy, flipped weights)?  Its conv descriptor's own rule (operands within the 32-bit buffer
// offsets, at most 2048 input channels), which mfma_gemm_can_pool states for a conv of these sizes.
static bool conv3x3_dx_fits(int h, int wd, int Cin, int Cout) {
  GemmDesc d;
  d.conv = 1; d.M = h * wd; d.H = h; d.Wd = wd; d.Cin = Cout; d.K = 9 * Cout; d.N = Cin; d.ldc = Cin;
  return mfma_gemm_can_pool(d);
}
static int check_conv3x3_grad_shape(dc_ctx* ctx, int h, int wd, int Cin, int Cout, bool dx, const char* who) {
  if (h < 1 || wd < 1 || Cin < 1 || Cout < 1 || Cin % 32 || Cout % 32)
    return ctx->fail(DC_E_INVALID, "%s: need Cin %% 32 == 0, Cout %% 32 == 0 and positive sizes", who);
  if ((long long)h * wd > (1 << 16))
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a map of %d x %d pixels, more than the 65536 the kernels take", who, h, wd);
  if (dx && !conv3x3_dx_fits(h, wd, Cin, Cout))
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a gradient of %d x %d x %d exceeds the engine's 32-bit operand offsets", who, h, wd, Cout);
  return DC_OK;
}
// What one call carves from its block: the weight gradient's partial tiles, the flipped weights in OIHW and packed, the engine's
// split-K scratch (the last three only where dx is wanted)
struct ConvGradScratch { float *part = nullptr, *wf = nullptr, *wfp = nullptr, *splitk = nullptr; };
static std::vector<Carve> conv3x3_grad_carve(int Cin, int Cout, int S, bool dw, bool dx, ConvGradScratch& r) {
  const size_t wn = (size_t)Cout * Cin * 9 * 4;
  return {{(void**)&r.part, dw ? conv3x3_wgrad_ws_floats(S, Cout, Cin) * 4 : 0},
          {(void**)&r.wf, dx ? wn : 0}, {(void**)&r.wfp, dx ? wn : 0}, {(void**)&r.splitk, dx ? kSplitkWsFloats * 4 : 0}};
}
// Launch list (stream s, eager, not synchronised; the caller holds LossCfgGuard):
//   conv3x3_wgrad + conv3x3_wgrad_finish (dw); colsum (db); conv3x3_flip + pack_conv3x3 + the engine's conv (dx)
// w_packed: w is in launch_pack_conv3x3's form (the ctx's own convolutions), not OIHW
static int conv3x3_grad(dc_ctx* ctx, hipStream_t s, const float* x, const float* w, const float* dy, int h, int wd, int Cin, int Cout,
                        int S, float* dw, float* db, float* dx, const ConvGradScratch& r, int w_packed = 0) {
  if (dw != nullptr) KCHK(launch_conv3x3_wgrad(x, dy, h, wd, Cin, Cout, S, dw, r.part, s));
  if (db != nullptr) KCHK(launch_colsum(dy, Cout, h * wd, Cout, db, s));
  if (dx != nullptr) {
    KCHK(launch_conv3x3_flip(w, Cout, Cin, w_packed, r.wf, s));
    KCHK(launch_pack_conv3x3(r.wf, r.wfp, Cin, Cout, s));
    DCCHK(conv3x3(ctx, s, dy, r.wfp, nullptr, dx, 1, h, wd, Cout, Cin, 0, Ws{r.splitk, kSplitkWsFloats}));
  }
  return DC_OK;
}
int dc_op_conv3x3_grad(dc_ctx* ctx, const float* x, const float* w, const float* dy, int h, int w_px, int Cin, int Cout, float* dw,
                       float* db, float* dx) {
  OP_PROLOGUE();
  const char* who = "dc_op_conv3x3_grad";
  if (!dy || (dw && !x) || (dx && !w)) return ctx->fail(DC_E_INVALID, "%s: null input", who);
  if (!dw && !db && !dx) return ctx->fail(DC_E_INVALID, "%s: no output asked for", who);
  DCCHK(check_conv3x3_grad_shape(ctx, h, w_px, Cin, Cout, dx != nullptr, who));
  drain_lanes(ctx);
  LossCfgGuard guard(ctx->cfg);
  const int S = conv3x3_wgrad_slices(h * w_px, Cout, Cin);
  ConvGradScratch r;
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(conv3x3_grad_carve(Cin, Cout, S, dw != nullptr, dx != nullptr, r)));
  return call_finish(ctx, s, conv3x3_grad(ctx, s, x, w, dy, h, w_px, Cin, Cout, S, dw, db, dx, r), who, dx != nullptr);
}

// ---- CNN gradients (docs/SEMANTICS.md, "CNN gradients") -------------------------------------------------------------
int dc_op_maxpool2x2_grad(dc_ctx* ctx, const float* y, const float* dpool, int n, int H, int W, int C, float* dy) {
  OP_PROLOGUE();
  if (!y || !dpool || !dy) return ctx->fail(DC_E_INVALID, "dc_op_maxpool2x2_grad: null pointer");
  if (n < 1 || H < 1 || W < 1 || C < 1 || C % 4) return ctx->fail(DC_E_INVALID, "dc_op_maxpool2x2_grad: need C %% 4 == 0 and positive sizes");
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dpool) | reinterpret_cast<uintptr_t>(dy)) & 15)
    return ctx->fail(DC_E_INVALID, "dc_op_maxpool2x2_grad: y, dpool and dy must be 16-byte aligned");
  KCHK(launch_maxpool2x2_ceil_relu_grad(y, dpool, dy, n, H, W, C, s));
  OP_EPILOGUE();
}
int dc_op_relu_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats) {
  OP_PROLOGUE();
  if (!y || !dy) return ctx->fail(DC_E_INVALID, "dc_op_relu_grad: null pointer");
  if (n_floats < 1) return ctx->fail(DC_E_INVALID, "dc_op_relu_grad: need n_floats >= 1");
  KCHK(launch_relu_mask(dy, y, (size_t)n_floats, s));
  OP_EPILOGUE();
}

// ---- Dropout (docs/SEMANTICS.md, "Dropout") ---------------------------------------------------------------------------------------
int dc_op_dropout(dc_ctx* ctx, float* x, int rows, int cols, int layer, float p, uint64_t seed) {
  OP_PROLOGUE();
  const char* who = "dc_op_dropout";
  if (!x) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (rows < 1 || cols < 1) return ctx->fail(DC_E_INVALID, "%s: need rows >= 1 and cols >= 1 (got %d, %d)", who, rows, cols);
  if (layer < 0 || layer > 255) return ctx->fail(DC_E_INVALID, "%s: layer must be in 0..255 (got %d)", who, layer);
  if (!(p >= 0.f && p < 1.f)) return ctx->fail(DC_E_INVALID, "%s: p must be in [0, 1), got %g", who, (double)p);
  if (p > 0.f) KCHK(launch_dropout_rows(x, rows, cols, (size_t)cols, layer, p, seed, s));     // (p = 0: the identity, no launch)
  OP_EPILOGUE();
}
int dc_op_relu_dropout_grad(dc_ctx* ctx, const float* y, float* dy, long long n_floats, float p) {
  OP_PROLOGUE();
  const char* who = "dc_op_relu_dropout_grad";
  if (!y || !dy) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (n_floats < 1) return ctx->fail(DC_E_INVALID, "%s: need n_floats >= 1", who);
  if (!(p >= 0.f && p < 1.f)) return ctx->fail(DC_E_INVALID, "%s: p must be in [0, 1), got %g", who, (double)p);
  if (p > 0.f) KCHK(launch_relu_dropout_mask(dy, y, (size_t)n_floats, p, s));
  else KCHK(launch_relu_mask(dy, y, (size_t)n_floats, s));
  OP_EPILOGUE();
}

// conv_net2: convolutions kCnnFirst .. 12 of kVgg.  Layer j = 0..8 is convolution kCnnFirst + j on a map of (h[j], w[j]) pixels.
constexpr int kCnnFirst = DC_NUM_VGG_CONVS - DC_NUM_CNN_GRAD_CONVS;
struct CnnShape {
  int h[DC_NUM_CNN_GRAD_CONVS], w[DC_NUM_CNN_GRAD_CONVS], fh, fw;
  CnnShape(int h4, int w4) {
    for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
      h[j] = h4; w[j] = w4;
      if (kVgg[kCnnFirst + j].pool_after) { h4 = (h4 + 1) / 2; w4 = (w4 + 1) / 2; }
    }
    fh = h4; fw = w4;
  }
  size_t in_floats(int j) const { return (size_t)h[j] * w[j] * kVgg[kCnnFirst + j].cin; }
  size_t out_floats(int j) const { return (size_t)h[j] * w[j] * kVgg[kCnnFirst + j].cout; }
};
// What the forward keeps: out[j] convolution j's output after its ReLU (the mask of layer j; the input of layer j + 1 where no
// pool follows), pooled[j] the pool's output where one does.  in(j): the input of layer j, x4 for the first.
struct CnnKept {
  const float* x4 = nullptr;
  float *out[DC_NUM_CNN_GRAD_CONVS] = {}, *pooled[DC_NUM_CNN_GRAD_CONVS] = {};
  const float* in(int j) const { return j == 0 ? x4 : pooled[j - 1] != nullptr ? pooled[j - 1] : out[j - 1]; }
};
// own_x4: a piece for the pool2 map itself (the training forward's, which the lane's ping-pong buffers would overwrite)
static std::vector<Carve> cnn_kept_carve(const CnnShape& sh, CnnKept& k, float** own_x4 = nullptr) {
  std::vector<Carve> cv;
  if (own_x4 != nullptr) cv.push_back({(void**)own_x4, sh.in_floats(0) * 4});
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
    cv.push_back({(void**)&k.out[j], sh.out_floats(j) * 4});
    if (kVgg[kCnnFirst + j].pool_after) cv.push_back({(void**)&k.pooled[j], sh.in_floats(j + 1) * 4});
  }
  return cv;
}
// The backward's scratch, sized once for the largest layer: two gradient maps (ga, gb) and conv3x3_grad's own pieces
struct CnnScratch { float *ga = nullptr, *gb = nullptr; ConvGradScratch r; int S[DC_NUM_CNN_GRAD_CONVS] = {}; };
static std::vector<Carve> cnn_scratch_carve(const CnnShape& sh, CnnScratch& c) {
  size_t map = 0, part = 0, wn = 0;
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
    const VggItem& v = kVgg[kCnnFirst + j];
    c.S[j] = conv3x3_wgrad_slices(sh.h[j] * sh.w[j], v.cout, v.cin);
    map = std::max(map, std::max(sh.in_floats(j), sh.out_floats(j)));
    part = std::max(part, conv3x3_wgrad_ws_floats(c.S[j], v.cout, v.cin));
    wn = std::max(wn, (size_t)v.cout * v.cin * 9);
  }
  return {{(void**)&c.ga, map * 4},        {(void**)&c.gb, map * 4},        {(void**)&c.r.part, part * 4},
          {(void**)&c.r.wf, wn * 4},       {(void**)&c.r.wfp, wn * 4},      {(void**)&c.r.splitk, kSplitkWsFloats * 4}};
}
static int check_cnn_grad_args(dc_ctx* ctx, int h4, int w4, const dc_cnn_grads* out, const char* who) {
  if (!out) return ctx->fail(DC_E_INVALID, "%s: null CNN gradient struct", who);
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j)
    if (!out->conv_w[j] || !out->conv_b[j]) return ctx->fail(DC_E_INVALID, "%s: null CNN gradient buffer", who);
  if (h4 < 1 || w4 < 1) return ctx->fail(DC_E_INVALID, "%s: need positive sizes", who);
  const CnnShape sh(h4, w4);
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j)
    DCCHK(check_conv3x3_grad_shape(ctx, sh.h[j], sh.w[j], kVgg[kCnnFirst + j].cin, kVgg[kCnnFirst + j].cout, j > 0 || out->x != nullptr, who));
  return DC_OK;
}
// Launch list (stream s, eager, not synchronised; the caller holds LossCfgGuard), per layer: the engine's conv with ReLU
// [+ maxpool2x2_ceil]; every output stays in `k`
static int cnn_forward_kept(dc_ctx* ctx, hipStream_t s, const CnnShape& sh, const CnnKept& k, const Ws& ws) {
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
    const int i = kCnnFirst + j;
    DCCHK(conv3x3(ctx, s, k.in(j), ctx->conv_w[i], ctx->conv_b[i], k.out[j], 1, sh.h[j], sh.w[j], kVgg[i].cin, kVgg[i].cout, 1, ws));
    if (kVgg[i].pool_after) KCHK(launch_maxpool2x2_ceil(k.out[j], k.pooled[j], 1, sh.h[j], sh.w[j], kVgg[i].cout, s));
  }
  return DC_OK;
}
// Launch list, from conv5_3 down: relu_mask in place (maxpool2x2_ceil_relu_grad into the other map where a pool follows the
// layer), then conv3x3_grad's launches; the first layer's dx only where out.x asks for it.  dfeat is copied first: it is read only.
static int cnn_backward(dc_ctx* ctx, hipStream_t s, const CnnShape& sh, const CnnKept& k, const float* dfeat, const dc_cnn_grads& out,
                        const dc_cnn_dump* dump, const CnnScratch& c) {
  const int last = DC_NUM_CNN_GRAD_CONVS - 1;
  float *cur = c.ga, *other = c.gb;            // cur: the gradient at the layer's output map (after the pool, where one follows)
  HIPCHK(hipMemcpyAsync(cur, dfeat, sh.out_floats(last) * 4, hipMemcpyDeviceToDevice, s));
  for (int j = last; j >= 0; --j) {
    const VggItem& v = kVgg[kCnnFirst + j];
    float* dy = cur;
    if (v.pool_after) {
      KCHK(launch_maxpool2x2_ceil_relu_grad(k.out[j], cur, other, 1, sh.h[j], sh.w[j], v.cout, s));
      dy = other;
    } else {
      KCHK(launch_relu_mask(cur, k.out[j], sh.out_floats(j), s));
    }
    if (dump != nullptr && dump->dy[j] != nullptr)
      HIPCHK(hipMemcpyAsync(dump->dy[j], dy, sh.out_floats(j) * 4, hipMemcpyDeviceToDevice, s));
    float* dx = j > 0 ? (dy == cur ? other : cur) : out.x;
    DCCHK(conv3x3_grad(ctx, s, k.in(j), ctx->conv_w[kCnnFirst + j], dy, sh.h[j], sh.w[j], v.cin, v.cout, c.S[j], out.conv_w[j],
                       out.conv_b[j], dx, c.r, 1));
    if (j > 0) { other = dy; cur = dx; }
  }
  return DC_OK;
}
// The training forward's trunk with kept activations (dc_forward_backward_cnn): conv1_1 .. pool2 as enqueue_trunk runs them, the
// pool2 map copied into ctx->train_cnn_kept (only this function grows it: cnn_x4 / cnn_feat stay valid), then cnn_forward_kept on the lane's split-K scratch; L.feat = conv5_3's kept map.
static int train_trunk_kept(dc_ctx* ctx, Lane& L, int* fh, int* fw) {
  hipStream_t s = L.stream;
  int h4 = 0, w4 = 0;
  DCCHK(enqueue_trunk(ctx, L, 1, &h4, &w4, kCnnFirst));
  const CnnShape sh(h4, w4);
  CnnKept k;
  float* x4 = nullptr;
  const std::vector<Carve> kc = cnn_kept_carve(sh, k, &x4);
  HIPCHK(ctx->train_cnn_kept.grow(carve(kc, nullptr), s));
  carve(kc, ctx->train_cnn_kept.get());
  HIPCHK(hipMemcpyAsync(x4, L.feat, sh.in_floats(0) * 4, hipMemcpyDeviceToDevice, s));
  k.x4 = x4;
  DCCHK(cnn_forward_kept(ctx, s, sh, k, lane_ws(L)));
  L.feat = k.out[DC_NUM_CNN_GRAD_CONVS - 1];
  ctx->cnn_x4 = x4; ctx->cnn_feat = L.feat; ctx->cnn_h4 = h4; ctx->cnn_w4 = w4;
  *fh = sh.fh; *fw = sh.fw;
  return DC_OK;
}
// The fourth stage of dc_forward_backward_cnn: the chain on what train_trunk_kept left in ctx->cnn_kept, dfeat = pg->feat
static int train_cnn_backward(dc_ctx* ctx, Lane& L, const float* dfeat, const dc_cnn_grads& cg) {
  hipStream_t s = L.stream;
  const CnnShape sh(ctx->cnn_h4, ctx->cnn_w4);
  CnnKept k;
  CnnScratch c;
  float* x4 = nullptr;
  carve(cnn_kept_carve(sh, k, &x4), ctx->train_cnn_kept.get());
  k.x4 = x4;
  const std::vector<Carve> sc = cnn_scratch_carve(sh, c);
  HIPCHK(ctx->cnn_ws.grow(carve(sc, nullptr), s));
  carve(sc, ctx->cnn_ws.get());
  auto& clock = ctx->cnn_clock;
  auto body = [&]() -> int {
    for (int i = 0; i < 3; ++i) HIPCHK(clock.record(i, s));          // (the forward ran inside train_forward: its time is the trunk stage's)
    DCCHK(cnn_backward(ctx, s, sh, k, dfeat, cg, nullptr, c));
    HIPCHK(clock.record(3, s));
    HIPCHK(hipStreamSynchronize(s));
    clock.read();
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "CNN backward", true);
}
int dc_op_cnn_grad(dc_ctx* ctx, const float* x4_hwc, int h4, int w4, const float* dfeat_hwc, const dc_cnn_grads* out,
                   const dc_cnn_dump* dump) {
  const char* who = "dc_op_cnn_grad";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!x4_hwc || !dfeat_hwc) return ctx->fail(DC_E_INVALID, "%s: null input", who);
  DCCHK(check_cnn_grad_args(ctx, h4, w4, out, who));
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  drain_lanes(ctx);
  LossCfgGuard guard(ctx->cfg);
  const CnnShape sh(h4, w4);
  CnnKept k;
  CnnScratch c;
  k.x4 = x4_hwc;
  const std::vector<Carve> kc = cnn_kept_carve(sh, k), sc = cnn_scratch_carve(sh, c);
  HIPCHK(ctx->cnn_kept.grow(carve(kc, nullptr), s));
  HIPCHK(ctx->cnn_ws.grow(carve(sc, nullptr), s));
  carve(kc, ctx->cnn_kept.get());
  carve(sc, ctx->cnn_ws.get());
  auto& clock = ctx->cnn_clock;
  auto body = [&]() -> int {
    ensure_fault_word(ctx);
    HIPCHK(clock.record(0, s));
    DCCHK(cnn_forward_kept(ctx, s, sh, k, Ws{c.r.splitk, kSplitkWsFloats}));
    HIPCHK(clock.record(1, s));
    if (dump != nullptr) {
      const int last = DC_NUM_CNN_GRAD_CONVS - 1;
      for (int j = 0; j <= last; ++j)
        if (dump->act[j] != nullptr) HIPCHK(hipMemcpyAsync(dump->act[j], k.in(j), sh.in_floats(j) * 4, hipMemcpyDeviceToDevice, s));
      for (int j = 0, p = 0; j <= last; ++j)
        if (kVgg[kCnnFirst + j].pool_after) {
          if (p < 2 && dump->prepool[p] != nullptr)
            HIPCHK(hipMemcpyAsync(dump->prepool[p], k.out[j], sh.out_floats(j) * 4, hipMemcpyDeviceToDevice, s));
          ++p;
        }
      if (dump->feat != nullptr) HIPCHK(hipMemcpyAsync(dump->feat, k.out[last], sh.out_floats(last) * 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(clock.record(2, s));
    DCCHK(cnn_backward(ctx, s, sh, k, dfeat_hwc, *out, dump, c));
    HIPCHK(clock.record(3, s));
    HIPCHK(hipStreamSynchronize(s));
    clock.read();
    return DC_OK;
  };
  return call_finish(ctx, s, body(), who, true);
}

// ---- RPN gradients (docs/SEMANTICS.md, "RPN gradients") -------------------------------------------------------------
// What the backward reads of the forward: the feature map, the RPN's hidden map after its in-place ReLU, the rows rpn_decode and
// rpn_score_rows made of the heads (A = k * h * w each), the sampler's lists and the ground truth on the device, and the
// gradient of the sampled boxes (n, 4) or null.
struct RpnKept {
  const float* feat; int h, w;
  const float *hidden, *trans, *scores, *anchors, *boxes, *gt, *droi;
  const int32_t *pos_idx, *pos_tgt, *neg_idx;
  int np, nn;
  float w_mid_obj, w_mid_box, decay;
};
struct RpnScratch {
  int32_t *win_all = nullptr, *win_pos = nullptr;
  float *dheads = nullptr, *dhidden = nullptr, *dw6 = nullptr, *db6 = nullptr, *ws = nullptr, *part = nullptr, *dfeat = nullptr;
};
static std::vector<Carve> rpn_carve(const dc_ctx* ctx, int h, int w, int S, RpnScratch& r) {
  const size_t hw = (size_t)h * w, K6 = (size_t)6 * ctx->k, R = (size_t)ctx->R, A = hw * ctx->k;
  return {{(void**)&r.win_all, A * 4},         {(void**)&r.win_pos, A * 4},      {(void**)&r.dheads, hw * K6 * 4},
          {(void**)&r.dhidden, hw * R * 4},    {(void**)&r.dw6, K6 * R * 4},     {(void**)&r.db6, K6 * 4},
          {(void**)&r.ws, wgrad_ws_floats((int)hw, (int)K6, (int)R) * 4},
          {(void**)&r.part, conv3x3_wgrad_ws_floats(S, (int)R, 512) * 4},        {(void**)&r.dfeat, hw * 512 * 4}};
}
static int check_rpn_out(dc_ctx* ctx, const dc_rpn_grads* o, const char* who) {
  if (!o || !o->rpn_conv_w || !o->rpn_conv_b || !o->rpn_box_w || !o->rpn_box_b || !o->rpn_score_w || !o->rpn_score_b || !o->feat)
    return ctx->fail(DC_E_INVALID, "%s: null RPN gradient buffer", who);
  return DC_OK;
}
static int check_rpn_grad_shape(dc_ctx* ctx, int h, int w, float decay, const char* who) {
  if (!(decay >= 0.f) || !std::isfinite(decay)) return ctx->fail(DC_E_INVALID, "%s: box_reg_decay must be finite and >= 0", who);
  if (h < 1 || w < 1) return ctx->fail(DC_E_INVALID, "%s: bad map size", who);
  if ((long long)h * w > (1 << 16))
    return ctx->fail(DC_E_UNSUPPORTED, "%s: a map of %d x %d pixels, more than the 65536 the kernels take", who, h, w);
  if (ctx->R % 32 || !conv3x3_dx_fits(h, w, 512, ctx->R) || (size_t)6 * ctx->k * 4 > 48 * 1024)
    return ctx->fail(DC_E_UNSUPPORTED, "%s: rpn_hidden = %d, num_anchors = %d: the hidden map's gradient does not fit the engine's conv "
                     "descriptor (a multiple of 32 channels, 32-bit operand offsets) or a head row the row kernel's LDS", who, ctx->R, ctx->k);
  return DC_OK;
}
// Launch list (lane 0's stream, eager; the caller holds LossCfgGuard; ws: the lane's split-K scratch):
//   [conv3x3_flip + pack_conv3x3 after a dc_load_weights]
//   2 x memset + rpn_winner + rpn_dheads
//   wgrad + colsum on dheads, four copies into the head outputs; rpn_heads_bwd
//   conv3x3_wgrad + conv3x3_wgrad_finish; colsum
//   the engine's conv on the flipped weights: the RPN's share of the feature map's gradient, kept in ctx->rpn_ws
// feat_add == null: out.feat = that share; else out.feat = feat_add + the share, one fp32 add per element.
static int rpn_backward(dc_ctx* ctx, hipStream_t s, const RpnKept& in, const dc_rpn_grads& out, const float* feat_add, const Ws& ws) {
  const int k = ctx->k, R = ctx->R, h = in.h, w = in.w, hw = h * w, K6 = 6 * k;
  const size_t wn = (size_t)R * 512 * 9;
  if (ctx->rpn_wf.get() == nullptr || ctx->rpn_wf.bytes() < 2 * wn * 4 || ctx->rpn_epoch != ctx->weights_epoch) {
    HIPCHK(ctx->rpn_wf.grow(2 * wn * 4, s));
    float* wf = static_cast<float*>(ctx->rpn_wf.get());
    KCHK(launch_conv3x3_flip(ctx->rpn_w, R, 512, 1, wf + wn, s));           // (the ctx keeps rpn_w packed)
    KCHK(launch_pack_conv3x3(wf + wn, wf, 512, R, s));
    ctx->rpn_epoch = ctx->weights_epoch;
  }
  const int S = conv3x3_wgrad_slices(hw, R, 512);
  RpnScratch r;
  const std::vector<Carve> cv = rpn_carve(ctx, h, w, S, r);
  HIPCHK(ctx->rpn_ws.grow(carve(cv, nullptr), s));
  carve(cv, ctx->rpn_ws.get());
  ctx->rpn_dfeat = nullptr;
  auto& clock = ctx->rpn_clock;
  auto body = [&]() -> int {
    HIPCHK(clock.record(0, s));
    RpnDheadsArgs a{};
    a.trans = in.trans; a.scores = in.scores; a.anchors = in.anchors; a.boxes = in.boxes; a.gt = in.gt; a.droi = in.droi;
    a.pos_input_idx = in.pos_idx; a.pos_target_idx = in.pos_tgt; a.neg_input_idx = in.neg_idx;
    a.num_pos = in.np; a.num_neg = in.nn; a.h = h; a.w = w; a.k = k;
    a.w_mid_obj = in.w_mid_obj; a.w_mid_box = in.w_mid_box; a.decay = in.decay;
    a.win_all = r.win_all; a.win_pos = r.win_pos; a.dheads = r.dheads;
    KCHK(launch_rpn_dheads(a, s));
    HIPCHK(clock.record(1, s));
    KCHK(launch_wgrad(r.dheads, K6, in.hidden, R, hw, K6, R, r.dw6, R, r.ws, s));
    KCHK(launch_colsum(r.dheads, K6, hw, K6, r.db6, s));
    HIPCHK(hipMemcpyAsync(out.rpn_box_w, r.dw6, (size_t)4 * k * R * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.rpn_score_w, r.dw6 + (size_t)4 * k * R, (size_t)2 * k * R * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.rpn_box_b, r.db6, (size_t)4 * k * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out.rpn_score_b, r.db6 + 4 * k, (size_t)2 * k * 4, hipMemcpyDeviceToDevice, s));
    KCHK(launch_rpn_heads_bwd(r.dheads, ctx->heads_w, in.hidden, hw, K6, R, r.dhidden, s));
    HIPCHK(clock.record(2, s));
    KCHK(launch_conv3x3_wgrad(in.feat, r.dhidden, h, w, 512, R, S, out.rpn_conv_w, r.part, s));
    KCHK(launch_colsum(r.dhidden, R, hw, R, out.rpn_conv_b, s));
    HIPCHK(clock.record(3, s));
    DCCHK(conv3x3(ctx, s, r.dhidden, static_cast<const float*>(ctx->rpn_wf.get()), nullptr, r.dfeat, 1, h, w, R, 512, 0, ws));
    if (feat_add != nullptr) KCHK(launch_add_pos_rows4(feat_add, r.dfeat, hw * 128, hw * 128, out.feat, s));
    else HIPCHK(hipMemcpyAsync(out.feat, r.dfeat, (size_t)hw * 512 * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(clock.record(4, s));
    HIPCHK(hipStreamSynchronize(s));
    clock.read();
    ctx->rpn_dfeat = r.dfeat; ctx->rpn_dfeat_pixels = hw;
    return DC_OK;
  };
  return call_finish(ctx, s, body(), "RPN backward", true);
}
// RpnKept of a record's rows and lists on the feature map `feat` and the hidden map made of it (droi: (np + nn, 4) or null)
static RpnKept rpn_kept(const TrainFwd& f, const float* feat, const float* hidden, const float* droi, float decay) {
  return {feat, f.h, f.w, hidden, f.trans, f.scores, f.anchors, f.boxes, f.gt, f.np + f.nn > 0 ? droi : nullptr, f.pos_idx, f.pos_tgt,
          f.neg_idx, f.np, f.nn, f.opts.mid_objectness_weight, f.opts.mid_box_reg_weight, decay};
}

int dc_op_rpn_grad(dc_ctx* ctx, const float* feat_hwc, int h, int w, const int32_t* pos_input_idx, const int32_t* pos_target_idx,
                   int num_pos, const int32_t* neg_input_idx, int num_neg, const float* gt_boxes, int G,
                   const float* droi_boxes_or_null, int img_h, int img_w, const dc_loss_opts* opts_or_null, float box_reg_decay,
                   const dc_rpn_grads* out, double* mid_objectness_loss, double* mid_box_reg_loss, int32_t* masked_mid) {
  const char* who = "dc_op_rpn_grad";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (!feat_hwc || !gt_boxes || !mid_objectness_loss || !mid_box_reg_loss || !masked_mid) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  DCCHK(check_rpn_out(ctx, out, who));
  const dc_loss_opts o = opts_or_null ? *opts_or_null : kLossDefaults;
  DCCHK(check_sampler_opts(ctx, &o, who));
  const int np = num_pos, nn = num_neg;
  if (np < 0 || nn < 0 || (long long)np + nn > 1024) return ctx->fail(DC_E_INVALID, "%s: num_pos + num_neg must be in 0..1024 (got %d + %d)", who, np, nn);
  if ((np > 0 && (!pos_input_idx || !pos_target_idx)) || (nn > 0 && !neg_input_idx)) return ctx->fail(DC_E_INVALID, "%s: null list", who);
  if (G < 1 || G > 512) return ctx->fail(DC_E_INVALID, "%s: G must be in 1..512 (got %d)", who, G);
  if (img_h < 32 || img_w < 32) return ctx->fail(DC_E_INVALID, "%s: image side below 32 px", who);
  DCCHK(check_image_size(ctx, img_h, img_w, who));
  DCCHK(check_rpn_grad_shape(ctx, h, w, box_reg_decay, who));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  const int k = ctx->k, R = ctx->R, hw = h * w, A = k * hw;
  TrainFwd f;                                // this call's own rows and lists, as a training forward would have recorded them
  f.np = np; f.nn = nn; f.h = h; f.w = w; f.opts = o;
  // the caller's lists and boxes are checked on the host: the kernels trust them
  std::vector<int32_t>& lists = f.lists;       // (host)
  std::vector<float> gth((size_t)G * 4);
  if (np > 0) {
    HIPCHK(hipMemcpy(lists.data(), pos_input_idx, (size_t)np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lists.data() + 1024, pos_target_idx, (size_t)np * 4, hipMemcpyDeviceToHost));
  }
  if (nn > 0) HIPCHK(hipMemcpy(lists.data() + 2048, neg_input_idx, (size_t)nn * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(gth.data(), gt_boxes, gth.size() * 4, hipMemcpyDeviceToHost));
  DCCHK(check_sampled_lists(ctx, who, DC_E_INVALID, lists.data(), np, nn, A, G));
  DCCHK(check_gt_boxes(ctx, who, gth.data(), G));
  LossCfgGuard guard(ctx->cfg);
  Lane& L = lane0(ctx);
  DCCHK(lane_prepare(ctx, L, img_h, img_w, o.batch_size, 1));
  hipStream_t s = L.stream;
  // ---- the forward half: rpn_train_forward on rows of this call's own; loss_terms with its two mid terms only ----
  float *hidden = nullptr, *heads = nullptr;
  int32_t *idx = nullptr, *masked = nullptr;
  double* terms = nullptr;
  const std::vector<Carve> cv = {
      {(void**)&hidden, (size_t)hw * R * 4}, {(void**)&heads, (size_t)hw * 6 * k * 4}, {(void**)&f.boxes, (size_t)A * 16},
      {(void**)&f.anchors, (size_t)A * 16},  {(void**)&f.trans, (size_t)A * 16},       {(void**)&f.scores, (size_t)A * 8},
      {(void**)&f.gt, (size_t)G * 16},       {(void**)&idx, 3 * 1024 * 4},             {(void**)&masked, 2 * 4},
      {(void**)&terms, 6 * 8}};
  HIPCHK(ctx->rpn_aux_ws.grow(carve(cv, nullptr), s));
  carve(cv, ctx->rpn_aux_ws.get());
  f.pos_idx = idx; f.pos_tgt = idx + 1024; f.neg_idx = idx + 2048;
  auto fwd = [&]() -> int {
    ensure_fault_word(ctx);
    DCCHK(rpn_train_forward(ctx, L, feat_hwc, h, w, img_h, img_w, hidden, heads, f.boxes, f.anchors, f.trans, f.scores));
    HIPCHK(hipMemcpyAsync(idx, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f.gt, gth.data(), gth.size() * 4, hipMemcpyHostToDevice, s));
    DCCHK(enqueue_loss_terms(ctx, s, f, nullptr, nullptr, nullptr, 1, terms, masked));
    HIPCHK(hipStreamSynchronize(s));
    return DC_OK;
  };
  const int rc = fwd();
  L.have_times = false;
  if (rc != DC_OK) { (void)hipStreamSynchronize(s); prof_collect(ctx); return rc; }
  *mid_objectness_loss = f.terms[0];
  *mid_box_reg_loss = f.terms[1];
  *masked_mid = f.masked[0];
  return rpn_backward(ctx, s, rpn_kept(f, feat_hwc, hidden, droi_boxes_or_null, box_reg_decay), *out, nullptr, lane_ws(L));
}

namespace {
int check_rpn_args(dc_ctx* ctx, const TrainCall& c, const dc_rpn_grads* pg, float box_reg_decay) {
  DCCHK(check_rpn_out(ctx, pg, c.who));
  int fh = 1, fw = 1;
  if (c.H >= 1 && c.W >= 1) feature_size(c.H, c.W, &fh, &fw);
  DCCHK(check_rpn_grad_shape(ctx, fh, fw, box_reg_decay, c.who));
  return check_dump(ctx, c.who, c.dump);
}
// The RPN backward on the record's rows, lists and ground truth and lane 0's feat and rpn_hidden; pg.feat = feat_add + its share
int train_rpn_backward(dc_ctx* ctx, Lane& L, const TrainFwd& f, float box_reg_decay, const float* droi, const float* feat_add,
                       const dc_rpn_grads& pg) {
  return rpn_backward(ctx, L.stream, rpn_kept(f, L.feat, L.rpn_hidden, droi, box_reg_decay), pg, feat_add, lane_ws(L));
}
// The three entry points: the first `stages` of the three stages.  Every argument is refused before anything is allocated or
// launched, in the order the refusals have always come in (RPN, recognition / language model, forward; every family ends with
// the dump's); one LossCfgGuard, one drain, one lane_prepare; the stages on ctx->train; dc_losses and the dump from it.
int train_call(dc_ctx* ctx, const TrainCall& c, int stages, const dc_recog_grads* rg, const dc_lm_grads* lg, float box_reg_decay,
               const dc_rpn_grads* pg, const dc_cnn_grads* cg = nullptr) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", c.who);
  if (stages > 3) {
    const int H = std::max(c.H, 1), W = std::max(c.W, 1);
    DCCHK(check_cnn_grad_args(ctx, ((H + 1) / 2 + 1) / 2, ((W + 1) / 2 + 1) / 2, cg, c.who));
  }
  if (stages > 2) DCCHK(check_rpn_args(ctx, c, pg, box_reg_decay));
  if (stages > 1) DCCHK(check_recog_lm_args(ctx, c, rg, lg));
  DCCHK(check_forward_args(ctx, c));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  LossCfgGuard guard(ctx->cfg);
  Lane& L = lane0(ctx);
  DCCHK(lane_prepare(ctx, L, c.H, c.W, c.o.batch_size, 1));
  struct FeatGuard {           // the kept-activation trunk points L.feat into ctx->train_cnn_kept for the stages of this call
    Lane& L; bool on; float* feat;        // only: afterwards the lane's pointer is what it was
    ~FeatGuard() { if (on) L.feat = feat; }
  } feat_guard{L, c.cnn, L.feat};
  DCCHK(train_forward(ctx, c, L, ctx->train));
  fill_losses(ctx->train, c.out, c.dump);
  if (stages > 1) DCCHK(train_recog_lm_backward(ctx, c, L, ctx->train, *rg, *lg));
  if (stages > 2) DCCHK(train_rpn_backward(ctx, L, ctx->train, box_reg_decay, rg->roi_boxes, rg->feat, *pg));
  if (stages > 3) DCCHK(train_cnn_backward(ctx, L, pg->feat, *cg));
  return DC_OK;
}
}  // namespace

#define TRAIN_ARGS(name) {name, img_chw, H, W, img_on_device, gt_boxes, gt_labels, G, L, opts ? *opts : kLossDefaults, forced, out, dump}
int dc_forward_losses(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                      dc_losses* out, const dc_loss_dump* dump) {
  return train_call(ctx, TRAIN_ARGS("dc_forward_losses"), 1, nullptr, nullptr, 0.f, nullptr);
}
int dc_loss_gradients(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                      const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                      dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg) {
  return train_call(ctx, TRAIN_ARGS("dc_loss_gradients"), 2, rg, lg, 0.f, nullptr);
}
int dc_forward_backward(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                        const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                        dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg, float box_reg_decay,
                        const dc_rpn_grads* pg) {
  return train_call(ctx, TRAIN_ARGS("dc_forward_backward"), 3, rg, lg, box_reg_decay, pg);
}
int dc_forward_backward_cnn(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                            const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                            dc_losses* out, const dc_loss_dump* dump, const dc_recog_grads* rg, const dc_lm_grads* lg,
                            float box_reg_decay, const dc_rpn_grads* pg, const dc_cnn_grads* cg) {
  TrainCall c = TRAIN_ARGS("dc_forward_backward_cnn");
  c.cnn = true;
  return train_call(ctx, c, 4, rg, lg, box_reg_decay, pg, cg);
}
// ---- the training step (docs/SEMANTICS.md, "Training step") ----------------------------------------------------------
namespace {
// The trained tensors as the Adam launch sees them: 17 segments for the checkpoint's 21 tensors.  A segment's parameter is the
// ctx's own engine buffer wherever that is the checkpoint layout, a concatenation of checkpoint layouts (the fused heads) or a
// permutation of one tensor (fc6): Adam is elementwise.  The two exceptions: lstm_w lives in lstm_w_ck (the engine reads the
// transposed halves made of it) and the RPN convolution in an OIHW master (the engine reads the packed form made of it).
struct TrainArena {
  float *rpn_conv_w = nullptr, *rpn_conv_b = nullptr, *heads_w = nullptr, *heads_b = nullptr, *fc6_w = nullptr, *fc6_b = nullptr;
  float *fc7_w = nullptr, *fc7_b = nullptr, *head5_w = nullptr, *head5_b = nullptr, *enc_w = nullptr, *enc_b = nullptr, *emb = nullptr;
  float *lstm_w = nullptr, *lstm_b = nullptr, *out_w = nullptr, *out_b = nullptr;
};
struct TrainSeg { float* TrainArena::*slot; float* p; size_t n; };
void train_segments(const dc_ctx* ctx, std::vector<TrainSeg>& out) {
  const size_t k = ctx->k, R = ctx->R, D = ctx->D, E = ctx->E, Hd = ctx->Hd, V = ctx->V;
  out = {{&TrainArena::rpn_conv_w, static_cast<float*>(ctx->train_master.get()), R * 512 * 9},
          {&TrainArena::rpn_conv_b, ctx->rpn_b, R},
          {&TrainArena::heads_w, ctx->heads_w, 6 * k * R},         // rpn_box_w (4k, R), then rpn_score_w (2k, R)
          {&TrainArena::heads_b, ctx->heads_b, 6 * k},
          {&TrainArena::fc6_w, ctx->fc6_w, D * kRecogK6},          // the engine's (i, j, c) input order: gradient and moments too
          {&TrainArena::fc6_b, ctx->fc6_b, D},
          {&TrainArena::fc7_w, ctx->fc7_w, D * D},
          {&TrainArena::fc7_b, ctx->fc7_b, D},
          {&TrainArena::head5_w, ctx->head5_w, 5 * D},             // obj_w (D), then boxreg_w (4, D)
          {&TrainArena::head5_b, ctx->head5_b, 5},
          {&TrainArena::enc_w, ctx->enc_w, E * D},
          {&TrainArena::enc_b, ctx->enc_b, E},
          {&TrainArena::emb, ctx->emb, (V + 2) * E},
          {&TrainArena::lstm_w, ctx->lstm_w_ck, (E + Hd) * 4 * Hd},
          {&TrainArena::lstm_b, ctx->lstm_b, 4 * Hd},
          {&TrainArena::out_w, ctx->dec_w, (V + 1) * Hd},          // the lm_out_w rows of dec_w
          {&TrainArena::out_b, ctx->out_b, V + 1}};
}
// the arena's carve list (the gradients'; the two moments' blocks are carved by the same list): bytes with base == null
size_t train_arena_carve(const std::vector<TrainSeg>& segs, TrainArena& a, void* base) {
  std::vector<Carve> cv;
  for (const TrainSeg& sg : segs) cv.push_back({(void**)&(a.*(sg.slot)), sg.n * 4});
  return carve(cv, base);
}
int check_train_opts(dc_ctx* ctx, const dc_train_opts* o, const char* who) {
  if (!o) return ctx->fail(DC_E_INVALID, "%s: null options", who);
  if (!std::isfinite(o->learning_rate) || o->learning_rate < 0) return ctx->fail(DC_E_INVALID, "%s: learning_rate must be finite and >= 0", who);
  if (!(o->beta1 >= 0 && o->beta1 < 1) || !(o->beta2 >= 0 && o->beta2 < 1)) return ctx->fail(DC_E_INVALID, "%s: beta1 and beta2 must lie in [0, 1)", who);
  if (!std::isfinite(o->epsilon) || !(o->epsilon > 0)) return ctx->fail(DC_E_INVALID, "%s: epsilon must be finite and > 0", who);
  if (!std::isfinite(o->weight_decay) || o->weight_decay < 0) return ctx->fail(DC_E_INVALID, "%s: weight_decay must be finite and >= 0", who);
  return DC_OK;
}
// The scalars of step t >= 1: each computed in double and rounded to float once (optim_updates.lua:56-84 computes them in double too)
AdamScalars adam_scalars(const dc_train_opts& o, int t) {
  const double step = o.learning_rate * std::sqrt(1.0 - std::pow(o.beta2, (double)t)) / (1.0 - std::pow(o.beta1, (double)t));
  return {(float)o.beta1, (float)(1.0 - o.beta1), (float)o.beta2, (float)(1.0 - o.beta2), (float)o.epsilon, (float)o.weight_decay,
          -(float)step};
}
// A segment table on the device (tab grows to hold it): nseg entries and the closing one; *chunks = the launch's work items
int upload_adam_table(dc_ctx* ctx, KeptBuf& tab, hipStream_t s, std::vector<AdamSeg>& segs, unsigned long long* chunks) {
  unsigned long long c = 0;
  for (AdamSeg& e : segs) { e.chunk0 = c; c += adam_chunks(e.n); }
  segs.push_back({nullptr, nullptr, nullptr, nullptr, 0, c});
  HIPCHK(tab.grow(segs.size() * sizeof(AdamSeg), s));
  HIPCHK(hipMemcpy(tab.get(), segs.data(), segs.size() * sizeof(AdamSeg), hipMemcpyHostToDevice));
  *chunks = c;
  return DC_OK;
}
void train_release(dc_ctx* ctx) {
  for (KeptBuf* b : {&ctx->train_g, &ctx->train_m, &ctx->train_v, &ctx->train_master, &ctx->train_out, &ctx->train_tab,
                     &ctx->train_cnn_master, &ctx->train_cnn_g, &ctx->train_cnn_m, &ctx->train_cnn_v, &ctx->train_cnn_tab,
                     &ctx->train_clip_buf}) b->reset();
  ctx->train_cnn_mode = ctx->train_cnn_t = ctx->train_cnn_nseg = 0;
  ctx->train_cnn_chunks = 0;
  ctx->train_clip = 0;
  ctx->train_clip_have = false;
  ctx->training = false;
  ctx->train_t = 0;
  ctx->train_nseg = 0;
  ctx->train_chunks = 0;
}
// Every operand the library derives from a trained weight, remade on s from the updated parameters (the list: DESIGN.md §19).
// Pointers do not move, so a captured forward stays valid and weights_epoch stays where it is; the gradient side's copies
// (out_wT, enc_wT; fc7_wT, fc6_wT; the RPN's flipped weights) are remade by their owners before their next use.  xg comes from
// the GEMM dc_load_weights runs, in fp32 whatever dc_set_math_mode says.
int train_refresh(dc_ctx* ctx, hipStream_t s) {
  const int R = ctx->R, V = ctx->V, E = ctx->E, Hd = ctx->Hd;
  KCHK(launch_pack_conv3x3(static_cast<const float*>(ctx->train_master.get()), ctx->rpn_w, R, 512, s));
  KCHK(launch_transpose2d(ctx->lstm_w_ck, ctx->wxT, E, 4 * Hd, s));
  KCHK(launch_transpose2d(ctx->lstm_w_ck + (size_t)E * 4 * Hd, ctx->whT, Hd, 4 * Hd, s));
  {
    Fp32Guard fp32(ctx->cfg);        // xg as a ctx makes it that loads its weights before the math mode is switched
    DCCHK(linear(ctx, s, ctx->emb, ctx->wxT, ctx->lstm_b, ctx->xg, V + 2, 4 * Hd, E, 0));
  }
  HIPCHK(hipMemcpyAsync(ctx->dec_w + (size_t)ctx->V1pad * Hd, ctx->whT, (size_t)4 * Hd * Hd * 4, hipMemcpyDeviceToDevice, s));
  KCHK(launch_screen_operands(ctx->dec_w, V + 1, Hd, ctx->V1pad, ctx->scr_Kp, ctx->scr_w, ctx->scr_wnorm, s));
  for (const auto& e : ctx->planes)
    if (e.planes != nullptr && (e.W == ctx->fc6_w || e.W == ctx->fc7_w || e.W == ctx->dec_w)) KCHK(launch_split_planes(e.W, e.planes, e.rows, e.K, s));
  ctx->grad_epoch = ctx->recog_epoch = ctx->rpn_epoch = 0;     // (weights_epoch >= 1 once weights are loaded)
  return DC_OK;
}
// The CNN's 18 trained tensors: per convolution kCnnFirst + j the OIHW master (w) and the ctx's own bias.  One carve list serves
// the masters (biases: zero bytes), the gradient arena and the two moments.
struct CnnTrain { float *w[DC_NUM_CNN_GRAD_CONVS] = {}, *b[DC_NUM_CNN_GRAD_CONVS] = {}; };
size_t cnn_train_carve(CnnTrain& a, void* base, bool biases) {
  std::vector<Carve> cv;
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
    const VggItem& v = kVgg[kCnnFirst + j];
    cv.push_back({(void**)&a.w[j], (size_t)v.cout * v.cin * 9 * 4});
    if (biases) cv.push_back({(void**)&a.b[j], (size_t)v.cout * 4});
  }
  return carve(cv, base);
}
// ... and what the library derives from them: the engine's packed convolutions and, where they exist, their split-bf16 planes
int train_refresh_cnn(dc_ctx* ctx, hipStream_t s) {
  CnnTrain p;
  cnn_train_carve(p, ctx->train_cnn_master.get(), false);
  for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
    const int i = kCnnFirst + j;
    KCHK(launch_pack_conv3x3(p.w[j], ctx->conv_w[i], kVgg[i].cout, kVgg[i].cin, s));
    for (const auto& e : ctx->planes)
      if (e.planes != nullptr && e.W == ctx->conv_w[i]) KCHK(launch_split_planes(e.W, e.planes, e.rows, e.K, s));
  }
  return DC_OK;
}
// The CNN's training state as the first non-zero dc_train_set_cnn makes it: masters, zeroed moments and arena, t = 0
int train_cnn_alloc(dc_ctx* ctx) {
  {
    HIPCHK(hipSetDevice(ctx->device));
    drain_lanes(ctx);
    hipStream_t s;
    DCCHK(lane0_stream(ctx, &s));
    auto body = [&]() -> int {
      CnnTrain p, g, m, v;
      HIPCHK(ctx->train_cnn_master.grow(cnn_train_carve(p, nullptr, false), s));
      cnn_train_carve(p, ctx->train_cnn_master.get(), false);
      const size_t bytes = cnn_train_carve(g, nullptr, true);
      for (KeptBuf* b : {&ctx->train_cnn_g, &ctx->train_cnn_m, &ctx->train_cnn_v}) {
        HIPCHK(b->grow(bytes, s));
        HIPCHK(hipMemsetAsync(b->get(), 0, bytes, s));
      }
      cnn_train_carve(g, ctx->train_cnn_g.get(), true);
      cnn_train_carve(m, ctx->train_cnn_m.get(), true);
      cnn_train_carve(v, ctx->train_cnn_v.get(), true);
      std::vector<AdamSeg> tab;
      for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
        const int i = kCnnFirst + j;
        KCHK(launch_unpack_conv3x3(ctx->conv_w[i], p.w[j], kVgg[i].cout, kVgg[i].cin, s));
        tab.push_back({p.w[j], g.w[j], m.w[j], v.w[j], (size_t)kVgg[i].cout * kVgg[i].cin * 9, 0});
        tab.push_back({ctx->conv_b[i], g.b[j], m.b[j], v.b[j], (size_t)kVgg[i].cout, 0});
      }
      const int nseg = (int)tab.size();
      DCCHK(upload_adam_table(ctx, ctx->train_cnn_tab, s, tab, &ctx->train_cnn_chunks));
      HIPCHK(hipStreamSynchronize(s));
      ctx->train_cnn_nseg = nseg;
      ctx->train_cnn_t = 0;
      return DC_OK;
    };
    const int rc = body();
    if (rc != DC_OK) {
      (void)hipStreamSynchronize(s);
      for (KeptBuf* b : {&ctx->train_cnn_master, &ctx->train_cnn_g, &ctx->train_cnn_m, &ctx->train_cnn_v, &ctx->train_cnn_tab}) b->reset();
      ctx->train_cnn_nseg = 0;
      return rc;
    }
  }
  return DC_OK;
}
}  // namespace

int dc_train_set_cnn(dc_ctx* ctx, int mode) {
  const char* who = "dc_train_set_cnn";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "%s: only between dc_train_begin and dc_train_end", who);
  if (mode < 0 || mode > 2) return ctx->fail(DC_E_INVALID, "%s: mode must be 0, 1 or 2 (got %d)", who, mode);
  if (mode != 0 && ctx->train_cnn_nseg == 0) DCCHK(train_cnn_alloc(ctx));
  ctx->train_cnn_mode = mode;
  return DC_OK;
}

int dc_train_begin(dc_ctx* ctx, const dc_train_opts* opts) {
  const char* who = "dc_train_begin";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  if (ctx->training) return ctx->fail(DC_E_STATE, "%s: already training; dc_train_end first", who);
  DCCHK(check_train_opts(ctx, opts, who));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  auto body = [&]() -> int {
    const size_t wn = (size_t)ctx->R * 512 * 9;
    HIPCHK(ctx->train_master.grow(wn * 4, s));
    KCHK(launch_unpack_conv3x3(ctx->rpn_w, static_cast<float*>(ctx->train_master.get()), ctx->R, 512, s));
    std::vector<TrainSeg> segs;
    train_segments(ctx, segs);
    TrainArena g, m, v;
    const size_t bytes = train_arena_carve(segs, g, nullptr);
    HIPCHK(ctx->train_g.grow(bytes, s));
    HIPCHK(ctx->train_m.grow(bytes, s));
    HIPCHK(ctx->train_v.grow(bytes, s));
    HIPCHK(hipMemsetAsync(ctx->train_m.get(), 0, bytes, s));
    HIPCHK(hipMemsetAsync(ctx->train_v.get(), 0, bytes, s));
    train_arena_carve(segs, g, ctx->train_g.get());
    train_arena_carve(segs, m, ctx->train_m.get());
    train_arena_carve(segs, v, ctx->train_v.get());
    std::vector<AdamSeg> tab;
    for (const TrainSeg& sg : segs) tab.push_back({sg.p, g.*(sg.slot), m.*(sg.slot), v.*(sg.slot), sg.n, 0});
    DCCHK(upload_adam_table(ctx, ctx->train_tab, s, tab, &ctx->train_chunks));
    ctx->train_nseg = (int)segs.size();
    HIPCHK(hipStreamSynchronize(s));
    return DC_OK;
  };
  const int rc = body();
  if (rc != DC_OK) { (void)hipStreamSynchronize(s); train_release(ctx); return rc; }
  ctx->train_opts = *opts;
  ctx->train_t = 0;
  ctx->train_clip = 0;
  ctx->train_clip_have = false;
  ctx->training = true;
  return DC_OK;
}

int dc_train_end(dc_ctx* ctx) {
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "dc_train_end: not training");
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  train_release(ctx);
  return DC_OK;
}

int dc_train_step(dc_ctx* ctx, const float* img_chw, int H, int W, int img_on_device, const float* gt_boxes,
                  const int32_t* gt_labels, int G, int L, const dc_loss_opts* opts, const dc_sampler_forced* forced,
                  dc_losses* out, const dc_loss_dump* dump, float box_reg_decay) {
  const char* who = "dc_train_step";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "%s: dc_train_begin first", who);
  TrainCall c = TRAIN_ARGS(who);
  const int cnn_mode = ctx->train_cnn_mode;
  c.cnn = cnn_mode == 2;
  // what sizes the outputs below is checked here; train_call then checks everything, in dc_forward_backward's order
  DCCHK(check_forward_args(ctx, c));
  int fh = 1, fw = 1;
  feature_size(H, W, &fh, &fw);
  DCCHK(check_rpn_grad_shape(ctx, fh, fw, box_reg_decay, who));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  std::vector<TrainSeg> segs;
  train_segments(ctx, segs);
  TrainArena g;
  train_arena_carve(segs, g, ctx->train_g.get());
  float *feat_rg = nullptr, *feat_pg = nullptr, *roi = nullptr;
  const std::vector<Carve> cv = {{(void**)&feat_rg, (size_t)fh * fw * 512 * 4}, {(void**)&feat_pg, (size_t)fh * fw * 512 * 4},
                                 {(void**)&roi, (size_t)c.o.batch_size * 16}};
  HIPCHK(ctx->train_out.grow(carve(cv, nullptr), s));
  carve(cv, ctx->train_out.get());
  const size_t k = ctx->k, R = ctx->R, D = ctx->D;
  const dc_recog_grads rg = {g.fc6_w, g.fc6_b, g.fc7_w, g.fc7_b, g.head5_w, g.head5_b, g.head5_w + D, g.head5_b + 1, feat_rg, roi};
  const dc_lm_grads lg = {g.enc_w, g.enc_b, g.emb, g.lstm_w, g.lstm_b, g.out_w, g.out_b, nullptr};
  const dc_rpn_grads pg = {g.rpn_conv_w, g.rpn_conv_b, g.heads_w, g.heads_b, g.heads_w + 4 * k * R, g.heads_b + 4 * k, feat_pg};
  auto& clock = ctx->train_clock;
  HIPCHK(clock.record(0, s));
  // the CNN's gradients: mode 2 the chain's, into the CNN's arena; mode 1 zero (train.lua:64-66, 83-85: at iter == finetune_cnn_after
  // cnn_grad_params is zeroed and model.finetune_cnn is still false), so that step is weight decay and Adam alone
  dc_cnn_grads cg{};
  if (cnn_mode != 0) {
    CnnTrain ga;
    cnn_train_carve(ga, ctx->train_cnn_g.get(), true);
    for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) { cg.conv_w[j] = ga.w[j]; cg.conv_b[j] = ga.b[j]; }
  }
  ctx->fc6_grad_engine = true;
  const int rc = train_call(ctx, c, cnn_mode == 2 ? 4 : 3, &rg, &lg, box_reg_decay, &pg, cnn_mode == 2 ? &cg : nullptr);
  ctx->fc6_grad_engine = false;
  if (rc != DC_OK) return rc;                      // no weight and no t has changed
  const AdamScalars k1 = adam_scalars(ctx->train_opts, ctx->train_t + 1);
  const AdamScalars kc = adam_scalars(ctx->train_opts, ctx->train_cnn_t + 1);      // (the CNN's own t: it counts CNN steps only)
  // clipping (docs/SEMANTICS.md, "Gradient clipping"): one norm over the table(s) whose gradients the backward filled, its two
  // launches in front of the Adam launch(es), which then read the scale from the device
  const bool clip = ctx->train_clip > 0;
  const AdamSeg* const tab1 = static_cast<const AdamSeg*>(ctx->train_tab.get());
  const AdamSeg* const tabc = static_cast<const AdamSeg*>(ctx->train_cnn_tab.get());
  GradNormRec* rec = nullptr;
  if (clip) {
    HIPCHK(ctx->train_clip_buf.grow(256 + (ctx->train_chunks + ctx->train_cnn_chunks) * sizeof(double), s));
    rec = static_cast<GradNormRec*>(ctx->train_clip_buf.get());
  }
  auto body = [&]() -> int {
    HIPCHK(clock.record(1, s));
    if (clip) {
      double* const partial = reinterpret_cast<double*>(reinterpret_cast<char*>(rec) + 256);
      unsigned long long total = ctx->train_chunks;
      KCHK(launch_grad_sumsq(tab1, ctx->train_nseg, ctx->train_chunks, partial, 0, s));
      if (cnn_mode == 2) {
        KCHK(launch_grad_sumsq(tabc, ctx->train_cnn_nseg, ctx->train_cnn_chunks, partial + total, 0, s));
        total += ctx->train_cnn_chunks;
      }
      KCHK(launch_grad_norm_finish(partial, total, ctx->train_clip, rec, s));
      KCHK(launch_adam_multi_scaled(tab1, ctx->train_nseg, ctx->train_chunks, k1, &rec->scale, 0, s));
    } else {
      KCHK(launch_adam_multi(tab1, ctx->train_nseg, ctx->train_chunks, k1, 0, s));
    }
    if (cnn_mode != 0) {
      if (cnn_mode == 1) HIPCHK(hipMemsetAsync(ctx->train_cnn_g.get(), 0, ctx->train_cnn_g.bytes(), s));
      if (clip && cnn_mode == 2) KCHK(launch_adam_multi_scaled(tabc, ctx->train_cnn_nseg, ctx->train_cnn_chunks, kc, &rec->scale, 0, s));
      else KCHK(launch_adam_multi(tabc, ctx->train_cnn_nseg, ctx->train_cnn_chunks, kc, 0, s));
    }
    HIPCHK(clock.record(2, s));
    DCCHK(train_refresh(ctx, s));
    if (cnn_mode != 0) DCCHK(train_refresh_cnn(ctx, s));
    HIPCHK(clock.record(3, s));
    return DC_OK;
  };
  ctx->train_t += 1;                               // (from the launch on the weights are step t's, whatever fails after it)
  if (cnn_mode != 0) ctx->train_cnn_t += 1;
  const int rc2 = call_finish(ctx, s, body(), who, true);
  if (rc2 != DC_OK) return rc2;
  clock.read();
  if (clip) {                                      // (the stream has drained: this copy waits for nothing)
    HIPCHK(hipMemcpy(&ctx->train_clip_rec, rec, sizeof(GradNormRec), hipMemcpyDeviceToHost));
    ctx->train_clip_have = true;
  }
  return DC_OK;
}

int dc_train_set_grad_clip(dc_ctx* ctx, double max_norm) {
  const char* who = "dc_train_set_grad_clip";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "%s: only between dc_train_begin and dc_train_end", who);
  if (!(max_norm >= 0)) return ctx->fail(DC_E_INVALID, "%s: max_norm must be >= 0 or +inf (0: off)", who);
  ctx->train_clip = max_norm;
  return DC_OK;
}

int dc_train_grad_norm(dc_ctx* ctx, double* norm, float* scale) {
  const char* who = "dc_train_grad_norm";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training || !ctx->train_clip_have) return ctx->fail(DC_E_STATE, "%s: no step has run with clipping on since dc_train_begin", who);
  if (norm) *norm = ctx->train_clip_rec.norm;
  if (scale) *scale = ctx->train_clip_rec.scale;
  return DC_OK;
}

int dc_get_weights(dc_ctx* ctx, const dc_weights* out) {
  const char* who = "dc_get_weights";
  if (!ctx || !out) return DC_E_INVALID;
  if (!ctx->have_weights) return ctx->fail(DC_E_STATE, "%s: weights not loaded", who);
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  const size_t k = ctx->k, R = ctx->R, D = ctx->D, E = ctx->E, Hd = ctx->Hd, V = ctx->V;
  auto d2h = [&](const float* dst, const float* dev, size_t n) -> int {
    if (dst != nullptr) HIPCHK(hipMemcpy(const_cast<float*>(dst), dev, n * 4, hipMemcpyDeviceToHost));
    return DC_OK;
  };
  // a packed convolution through a call's scratch: unpack, then copy
  auto conv_out = [&](const float* dst, const float* packed, int Cout, int Cin) -> int {
    if (dst == nullptr) return DC_OK;
    Scratch tmp(ctx->scratch, s);
    HIPCHK(tmp.alloc((size_t)Cout * Cin * 9 * 4));
    KCHK(launch_unpack_conv3x3(packed, static_cast<float*>(tmp.get()), Cout, Cin, s));
    HIPCHK(hipStreamSynchronize(s));
    return d2h(dst, static_cast<const float*>(tmp.get()), (size_t)Cout * Cin * 9);
  };
  DCCHK(d2h(out->conv_w[0], ctx->conv_w[0], (size_t)64 * 27));
  for (int i = 0; i < DC_NUM_VGG_CONVS; ++i) {
    if (i > 0) DCCHK(conv_out(out->conv_w[i], ctx->conv_w[i], kVgg[i].cout, kVgg[i].cin));
    DCCHK(d2h(out->conv_b[i], ctx->conv_b[i], kVgg[i].cout));
  }
  DCCHK(conv_out(out->rpn_conv_w, ctx->rpn_w, (int)R, 512));
  DCCHK(d2h(out->rpn_conv_b, ctx->rpn_b, R));
  DCCHK(d2h(out->rpn_box_w, ctx->heads_w, 4 * k * R));
  DCCHK(d2h(out->rpn_score_w, ctx->heads_w + 4 * k * R, 2 * k * R));
  DCCHK(d2h(out->rpn_box_b, ctx->heads_b, 4 * k));
  DCCHK(d2h(out->rpn_score_b, ctx->heads_b + 4 * k, 2 * k));
  if (out->fc6_w != nullptr) {
    if (D > 65535) return ctx->fail(DC_E_UNSUPPORTED, "%s: fc_dim = %d: the fc6 permutation takes at most 65535 rows", who, (int)D);
    Scratch tmp(ctx->scratch, s);
    HIPCHK(tmp.alloc(D * kRecogK6 * 4));
    KCHK(launch_permute_fc6_back(ctx->fc6_w, static_cast<float*>(tmp.get()), (int)D, 512, 49, s));
    HIPCHK(hipStreamSynchronize(s));
    DCCHK(d2h(out->fc6_w, static_cast<const float*>(tmp.get()), D * kRecogK6));
  }
  DCCHK(d2h(out->fc6_b, ctx->fc6_b, D));
  DCCHK(d2h(out->fc7_w, ctx->fc7_w, D * D));
  DCCHK(d2h(out->fc7_b, ctx->fc7_b, D));
  DCCHK(d2h(out->obj_w, ctx->head5_w, D));
  DCCHK(d2h(out->obj_b, ctx->head5_b, 1));
  DCCHK(d2h(out->boxreg_w, ctx->head5_w + D, 4 * D));
  DCCHK(d2h(out->boxreg_b, ctx->head5_b + 1, 4));
  DCCHK(d2h(out->lm_enc_w, ctx->enc_w, E * D));
  DCCHK(d2h(out->lm_enc_b, ctx->enc_b, E));
  DCCHK(d2h(out->lm_emb, ctx->emb, (V + 2) * E));
  DCCHK(d2h(out->lstm_w, ctx->lstm_w_ck, (E + Hd) * 4 * Hd));
  DCCHK(d2h(out->lstm_b, ctx->lstm_b, 4 * Hd));
  DCCHK(d2h(out->lm_out_w, ctx->dec_w, (V + 1) * Hd));
  DCCHK(d2h(out->lm_out_b, ctx->out_b, V + 1));
  DCCHK(d2h(out->anchors, ctx->anchors, 2 * k));
  return DC_OK;
}

static int adam_segments_run(dc_ctx* ctx, const char* who, std::vector<AdamSeg>& tab, int t, const dc_train_opts* opts, int grid) {
  DCCHK(check_train_opts(ctx, opts, who));
  if (t < 1) return ctx->fail(DC_E_INVALID, "%s: t counts from 1 (got %d)", who, t);
  for (const AdamSeg& e : tab)
    if (!e.p || !e.g || !e.m || !e.v || e.n < 1) return ctx->fail(DC_E_INVALID, "%s: a segment needs four buffers and n >= 1", who);
  if (grid < 0 || grid > 65535) return ctx->fail(DC_E_INVALID, "%s: grid must be in 0..65535", who);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  const int nseg = (int)tab.size();
  unsigned long long chunks = 0;
  DCCHK(upload_adam_table(ctx, ctx->optim_tab, s, tab, &chunks));
  auto body = [&]() -> int {
    KCHK(launch_adam_multi(static_cast<const AdamSeg*>(ctx->optim_tab.get()), nseg, chunks, adam_scalars(*opts, t), grid, s));
    return DC_OK;
  };
  return call_finish(ctx, s, body(), who);
}

int dc_op_adam(dc_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, int t, const dc_train_opts* opts) {
  if (!ctx) return DC_E_INVALID;
  std::vector<AdamSeg> tab = {{p, g, m, v, n, 0}};
  return adam_segments_run(ctx, "dc_op_adam", tab, t, opts, 0);
}

// The norm pass over `tab` (uploaded into ctx->optim_tab), then, with `adam`, the scaled Adam launch; the record comes back to *out
static int grad_norm_run(dc_ctx* ctx, const char* who, std::vector<AdamSeg>& tab, double max_norm, int grid, const AdamScalars* adam,
                         GradNormRec* out) {
  if (!(max_norm >= 0)) return ctx->fail(DC_E_INVALID, "%s: max_norm must be >= 0 or +inf", who);
  if (grid < 0 || grid > 65535) return ctx->fail(DC_E_INVALID, "%s: grid must be in 0..65535", who);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  const int nseg = (int)tab.size();
  unsigned long long chunks = 0;
  DCCHK(upload_adam_table(ctx, ctx->optim_tab, s, tab, &chunks));
  Scratch block(ctx->scratch, s);
  GradNormRec* rec = nullptr;
  double* partial = nullptr;
  HIPCHK(block.alloc(std::vector<Carve>{{(void**)&rec, sizeof(GradNormRec)}, {(void**)&partial, (size_t)chunks * sizeof(double)}}));
  const AdamSeg* const dev = static_cast<const AdamSeg*>(ctx->optim_tab.get());
  auto body = [&]() -> int {
    KCHK(launch_grad_sumsq(dev, nseg, chunks, partial, grid, s));
    KCHK(launch_grad_norm_finish(partial, chunks, max_norm, rec, s));
    if (adam) KCHK(launch_adam_multi_scaled(dev, nseg, chunks, *adam, &rec->scale, grid, s));
    return DC_OK;
  };
  DCCHK(call_finish(ctx, s, body(), who));
  HIPCHK(hipMemcpy(out, rec, sizeof(GradNormRec), hipMemcpyDeviceToHost));
  return DC_OK;
}

int dc_op_grad_norm(dc_ctx* ctx, const float* g, size_t n, double max_norm, double* sumsq, double* norm, float* scale) {
  const char* who = "dc_op_grad_norm";
  if (!ctx) return DC_E_INVALID;
  if (!g || n < 1) return ctx->fail(DC_E_INVALID, "%s: a segment needs a buffer and n >= 1", who);
  std::vector<AdamSeg> tab = {{nullptr, g, nullptr, nullptr, n, 0}};
  GradNormRec r{};
  DCCHK(grad_norm_run(ctx, who, tab, max_norm, 0, nullptr, &r));
  if (sumsq) *sumsq = r.sumsq;
  if (norm) *norm = r.norm;
  if (scale) *scale = r.scale;
  return DC_OK;
}

// ---- Adam's state out and in (docs/SEMANTICS.md, "Training step") ------------------------------------------------------------------
namespace {
// What both directions check first: the pointers of the untrained tensors must be null; *cnn = how many of the CNN's 18 are given
int train_state_shape(dc_ctx* ctx, const dc_weights* w, const char* who, int* cnn) {
  *cnn = 0;
  if (!w) return DC_OK;
  for (int i = 0; i < DC_NUM_VGG_CONVS; ++i) {
    if (i < kCnnFirst) {
      if (w->conv_w[i] || w->conv_b[i]) return ctx->fail(DC_E_INVALID, "%s: conv_w[%d] / conv_b[%d] are never trained: must be null", who, i, i);
    } else {
      *cnn += (w->conv_w[i] != nullptr) + (w->conv_b[i] != nullptr);
    }
  }
  if (w->anchors) return ctx->fail(DC_E_INVALID, "%s: anchors are not trained: must be null", who);
  return DC_OK;
}
bool train_state_complete(const dc_weights* w) {          // the 21 trained tensors outside the CNN
  for (const float* f : {w->rpn_conv_w, w->rpn_conv_b, w->rpn_box_w, w->rpn_box_b, w->rpn_score_w, w->rpn_score_b, w->fc6_w, w->fc6_b,
                         w->fc7_w, w->fc7_b, w->obj_w, w->obj_b, w->boxreg_w, w->boxreg_b, w->lm_enc_w, w->lm_enc_b, w->lm_emb,
                         w->lstm_w, w->lstm_b, w->lm_out_w, w->lm_out_b})
    if (f == nullptr) return false;
  return true;
}
// One moment block (the arena `base` of the 21 tensors, `cnn_base` of the CNN's or null) <-> w's host tensors, in checkpoint layouts
int train_state_move(dc_ctx* ctx, hipStream_t s, const dc_weights* w, void* base, void* cnn_base, bool to_host, const char* who) {
  const size_t k = ctx->k, R = ctx->R, D = ctx->D, E = ctx->E, Hd = ctx->Hd, V = ctx->V;
  std::vector<TrainSeg> segs;
  train_segments(ctx, segs);
  TrainArena a;
  train_arena_carve(segs, a, base);
  auto mv = [&](const float* host, float* dev, size_t n) -> int {
    if (host == nullptr) return DC_OK;
    if (to_host) HIPCHK(hipMemcpy(const_cast<float*>(host), dev, n * 4, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy(dev, host, n * 4, hipMemcpyHostToDevice));
    return DC_OK;
  };
  DCCHK(mv(w->rpn_conv_w, a.rpn_conv_w, R * 512 * 9));
  DCCHK(mv(w->rpn_conv_b, a.rpn_conv_b, R));
  DCCHK(mv(w->rpn_box_w, a.heads_w, 4 * k * R));
  DCCHK(mv(w->rpn_score_w, a.heads_w + 4 * k * R, 2 * k * R));
  DCCHK(mv(w->rpn_box_b, a.heads_b, 4 * k));
  DCCHK(mv(w->rpn_score_b, a.heads_b + 4 * k, 2 * k));
  if (w->fc6_w != nullptr) {                      // the arena holds fc6 in the engine's (i, j, c) input order
    if (D > 65535) return ctx->fail(DC_E_UNSUPPORTED, "%s: fc_dim = %d: the fc6 permutation takes at most 65535 rows", who, (int)D);
    Scratch tmp(ctx->scratch, s);
    HIPCHK(tmp.alloc(D * kRecogK6 * 4));
    float* const t = static_cast<float*>(tmp.get());
    if (to_host) {
      KCHK(launch_permute_fc6_back(a.fc6_w, t, (int)D, 512, 49, s));
      HIPCHK(hipStreamSynchronize(s));
      DCCHK(mv(w->fc6_w, t, D * kRecogK6));
    } else {
      DCCHK(mv(w->fc6_w, t, D * kRecogK6));
      KCHK(launch_permute_fc6(t, a.fc6_w, (int)D, 512, 49, s));
      HIPCHK(hipStreamSynchronize(s));
    }
  }
  DCCHK(mv(w->fc6_b, a.fc6_b, D));
  DCCHK(mv(w->fc7_w, a.fc7_w, D * D));
  DCCHK(mv(w->fc7_b, a.fc7_b, D));
  DCCHK(mv(w->obj_w, a.head5_w, D));
  DCCHK(mv(w->obj_b, a.head5_b, 1));
  DCCHK(mv(w->boxreg_w, a.head5_w + D, 4 * D));
  DCCHK(mv(w->boxreg_b, a.head5_b + 1, 4));
  DCCHK(mv(w->lm_enc_w, a.enc_w, E * D));
  DCCHK(mv(w->lm_enc_b, a.enc_b, E));
  DCCHK(mv(w->lm_emb, a.emb, (V + 2) * E));
  DCCHK(mv(w->lstm_w, a.lstm_w, (E + Hd) * 4 * Hd));
  DCCHK(mv(w->lstm_b, a.lstm_b, 4 * Hd));
  DCCHK(mv(w->lm_out_w, a.out_w, (V + 1) * Hd));
  DCCHK(mv(w->lm_out_b, a.out_b, V + 1));
  if (cnn_base != nullptr) {
    CnnTrain c;
    cnn_train_carve(c, cnn_base, true);
    for (int j = 0; j < DC_NUM_CNN_GRAD_CONVS; ++j) {
      const VggItem& vg = kVgg[kCnnFirst + j];
      DCCHK(mv(w->conv_w[kCnnFirst + j], c.w[j], (size_t)vg.cout * vg.cin * 9));
      DCCHK(mv(w->conv_b[kCnnFirst + j], c.b[j], (size_t)vg.cout));
    }
  }
  return DC_OK;
}
}  // namespace

int dc_train_get_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int* t, int* cnn_t) {
  const char* who = "dc_train_get_state";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "%s: only between dc_train_begin and dc_train_end", who);
  int cm = 0, cv = 0;
  DCCHK(train_state_shape(ctx, m, who, &cm));
  DCCHK(train_state_shape(ctx, v, who, &cv));
  const bool have_cnn = ctx->train_cnn_nseg > 0;
  if ((cm > 0 || cv > 0) && !have_cnn) return ctx->fail(DC_E_STATE, "%s: the CNN has no training state (no non-zero dc_train_set_cnn yet)", who);
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  HIPCHK(hipStreamSynchronize(s));
  if (m) DCCHK(train_state_move(ctx, s, m, ctx->train_m.get(), have_cnn ? ctx->train_cnn_m.get() : nullptr, true, who));
  if (v) DCCHK(train_state_move(ctx, s, v, ctx->train_v.get(), have_cnn ? ctx->train_cnn_v.get() : nullptr, true, who));
  if (t) *t = ctx->train_t;
  if (cnn_t) *cnn_t = have_cnn ? ctx->train_cnn_t : 0;
  return DC_OK;
}

int dc_train_set_state(dc_ctx* ctx, const dc_weights* m, const dc_weights* v, int t, int cnn_t) {
  const char* who = "dc_train_set_state";
  if (!ctx) return DC_E_INVALID;
  if (!ctx->training) return ctx->fail(DC_E_STATE, "%s: only between dc_train_begin and dc_train_end", who);
  if (!m || !v) return ctx->fail(DC_E_INVALID, "%s: both moments are required", who);
  if (t < 0 || cnn_t < 0) return ctx->fail(DC_E_INVALID, "%s: t and cnn_t must be >= 0 (got %d, %d)", who, t, cnn_t);
  int cm = 0, cv = 0;
  DCCHK(train_state_shape(ctx, m, who, &cm));
  DCCHK(train_state_shape(ctx, v, who, &cv));
  if (!train_state_complete(m) || !train_state_complete(v))
    return ctx->fail(DC_E_INVALID, "%s: all 21 trained tensors are required in m and in v", who);
  const int all = 2 * DC_NUM_CNN_GRAD_CONVS;
  if (cm != cv || (cm != 0 && cm != all)) return ctx->fail(DC_E_INVALID, "%s: the CNN's 18 tensors are given in both moments or in neither", who);
  if (cm == 0 && cnn_t != 0) return ctx->fail(DC_E_INVALID, "%s: cnn_t = %d without the CNN's moments", who, cnn_t);
  if (ctx->D > 65535) return ctx->fail(DC_E_UNSUPPORTED, "%s: fc_dim = %d: the fc6 permutation takes at most 65535 rows", who, (int)ctx->D);
  if (cm == all && ctx->train_cnn_nseg == 0) DCCHK(train_cnn_alloc(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  drain_lanes(ctx);
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  HIPCHK(hipStreamSynchronize(s));
  const bool cnn = cm == all;
  DCCHK(train_state_move(ctx, s, m, ctx->train_m.get(), cnn ? ctx->train_cnn_m.get() : nullptr, false, who));
  DCCHK(train_state_move(ctx, s, v, ctx->train_v.get(), cnn ? ctx->train_cnn_v.get() : nullptr, false, who));
  ctx->train_t = t;
  if (cnn) ctx->train_cnn_t = cnn_t;
  return DC_OK;
}

// ---- test hook of gradient clipping (densecap_debug_clip.h) ---------------------------------------------------------------------------
int dc_debug_adam_multi_clip(dc_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n,
                             int nseg, int t, const dc_train_opts* opts, int grid, double max_norm, double* sumsq, float* scale) {
  const char* who = "dc_debug_adam_multi_clip";
  if (!ctx) return DC_E_INVALID;
  if (!p || !g || !m || !v || !n || nseg < 1 || nseg > 4096) return ctx->fail(DC_E_INVALID, "%s: 1..4096 segments, five lists", who);
  DCCHK(check_train_opts(ctx, opts, who));
  if (t < 1) return ctx->fail(DC_E_INVALID, "%s: t counts from 1 (got %d)", who, t);
  std::vector<AdamSeg> tab;
  for (int i = 0; i < nseg; ++i) {
    if (!p[i] || !g[i] || !m[i] || !v[i] || n[i] < 1) return ctx->fail(DC_E_INVALID, "%s: a segment needs four buffers and n >= 1", who);
    tab.push_back({p[i], g[i], m[i], v[i], n[i], 0});
  }
  const AdamScalars k = adam_scalars(*opts, t);
  GradNormRec r{};
  DCCHK(grad_norm_run(ctx, who, tab, max_norm, grid, &k, &r));
  if (sumsq) *sumsq = r.sumsq;
  if (scale) *scale = r.scale;
  return DC_OK;
}

// ---- test hooks of the optimiser's kernels (densecap_debug_optim.h) ----------------------------------------------------------------
int dc_debug_adam_multi(dc_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n,
                        int nseg, int t, const dc_train_opts* opts, int grid) {
  const char* who = "dc_debug_adam_multi";
  if (!ctx) return DC_E_INVALID;
  if (!p || !g || !m || !v || !n || nseg < 1 || nseg > 4096) return ctx->fail(DC_E_INVALID, "%s: 1..4096 segments, five lists", who);
  std::vector<AdamSeg> tab;
  for (int i = 0; i < nseg; ++i) tab.push_back({p[i], g[i], m[i], v[i], n[i], 0});
  return adam_segments_run(ctx, who, tab, t, opts, grid);
}
int dc_debug_screen_operands(dc_ctx* ctx, const float* W, int V1, int Hd, int V1pad, int Kp, uint16_t* wb, uint16_t* wn) {
  const char* who = "dc_debug_screen_operands";
  if (!ctx) return DC_E_INVALID;
  if (!W || !wb || !wn || V1 < 1 || Hd < 1 || V1pad < V1 || Kp < Hd) return ctx->fail(DC_E_INVALID, "%s: bad argument", who);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  auto body = [&]() -> int { KCHK(launch_screen_operands(W, V1, Hd, V1pad, Kp, wb, wn, s)); return DC_OK; };
  return call_finish(ctx, s, body(), who);
}
int dc_debug_unpack_conv3x3(dc_ctx* ctx, const float* w_packed, float* w_oihw, int Cout, int Cin) {
  const char* who = "dc_debug_unpack_conv3x3";
  if (!ctx) return DC_E_INVALID;
  if (!w_packed || !w_oihw || Cout < 1 || Cin < 1) return ctx->fail(DC_E_INVALID, "%s: bad argument", who);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s;
  DCCHK(lane0_stream(ctx, &s));
  auto body = [&]() -> int { KCHK(launch_unpack_conv3x3(w_packed, w_oihw, Cout, Cin, s)); return DC_OK; };
  return call_finish(ctx, s, body(), who);
}
#undef TRAIN_ARGS


// ---- test hooks of the RPN backward (densecap_debug_rpn.h) ----------------------------------------------------------------------------
int dc_debug_rpn_dheads(dc_ctx* ctx, const float* trans, const float* scores, const float* anchors, const float* boxes, int h, int w_px,
                        int k, const int32_t* pos_input_idx, const int32_t* pos_target_idx, int num_pos, const int32_t* neg_input_idx,
                        int num_neg, const float* gt, int G, const float* droi_or_null, float w_mid_obj, float w_mid_box, float decay,
                        float* dheads) {
  OP_PROLOGUE();
  const char* who = "dc_debug_rpn_dheads";
  if (!trans || !scores || !anchors || !boxes || !gt || !dheads || h < 1 || w_px < 1 || k < 1 || G < 1 || num_pos < 0 || num_neg < 0 ||
      (long long)num_pos + num_neg > 1024 || (long long)h * w_px > (1 << 16) || k > 4096 || (num_pos > 0 && (!pos_input_idx || !pos_target_idx)) ||
      (num_neg > 0 && !neg_input_idx))
    return ctx->fail(DC_E_INVALID, "%s: bad argument", who);
  const int A = k * h * w_px;
  std::vector<int32_t> li(3 * 1024, 0);                       // the kernels trust their lists: the caller's are checked here
  if (num_pos > 0) {
    HIPCHK(hipMemcpy(li.data(), pos_input_idx, (size_t)num_pos * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(li.data() + 1024, pos_target_idx, (size_t)num_pos * 4, hipMemcpyDeviceToHost));
  }
  if (num_neg > 0) HIPCHK(hipMemcpy(li.data() + 2048, neg_input_idx, (size_t)num_neg * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < num_pos; ++r)
    if (li[r] < 0 || li[r] >= A || li[1024 + r] < 0 || li[1024 + r] >= G) return ctx->fail(DC_E_INVALID, "%s: positive row %d out of range", who, r);
  for (int r = 0; r < num_neg; ++r)
    if (li[2048 + r] < 0 || li[2048 + r] >= A) return ctx->fail(DC_E_INVALID, "%s: negative row %d out of range", who, r);
  RpnDheadsArgs a{};
  Scratch block(ctx->scratch, s);
  HIPCHK(block.alloc(std::vector<Carve>{{(void**)&a.win_all, (size_t)A * 4}, {(void**)&a.win_pos, (size_t)A * 4}}));
  a.trans = trans; a.scores = scores; a.anchors = anchors; a.boxes = boxes; a.gt = gt; a.droi = droi_or_null;
  a.pos_input_idx = pos_input_idx; a.pos_target_idx = pos_target_idx; a.neg_input_idx = neg_input_idx;
  a.num_pos = num_pos; a.num_neg = num_neg; a.h = h; a.w = w_px; a.k = k;
  a.w_mid_obj = w_mid_obj; a.w_mid_box = w_mid_box; a.decay = decay; a.dheads = dheads;
  KCHK(launch_rpn_dheads(a, s));
  OP_EPILOGUE();
}
int dc_debug_rpn_heads_bwd(dc_ctx* ctx, const float* dheads, const float* heads_w, const float* hidden, int P, int K6, int R,
                           float* dhidden) {
  OP_PROLOGUE();
  if (!dheads || !heads_w || !hidden || !dhidden || P < 1 || K6 < 1 || R < 1 || K6 > 12288)
    return ctx->fail(DC_E_INVALID, "dc_debug_rpn_heads_bwd: bad argument");
  KCHK(launch_rpn_heads_bwd(dheads, heads_w, hidden, P, K6, R, dhidden, s));
  OP_EPILOGUE();
}
int dc_debug_rpn_grad_kept(dc_ctx* ctx, float* feat_rpn, int pixels, float* ms) {
  OP_PROLOGUE();
  const char* who = "dc_debug_rpn_grad_kept";
  if (!ms) return ctx->fail(DC_E_INVALID, "%s: null pointer", who);
  if (ctx->rpn_dfeat == nullptr) return ctx->fail(DC_E_STATE, "%s: no RPN backward has completed", who);
  if (feat_rpn != nullptr) {
    if (pixels != ctx->rpn_dfeat_pixels) return ctx->fail(DC_E_INVALID, "%s: the kept map has %d pixels (got %d)", who, ctx->rpn_dfeat_pixels, pixels);
    HIPCHK(hipMemcpyAsync(feat_rpn, ctx->rpn_dfeat, (size_t)pixels * 512 * 4, hipMemcpyDeviceToDevice, s));
  }
  memcpy(ms, ctx->rpn_clock.ms, 16);
  OP_EPILOGUE();
}

// ---- test hook of the convolution backward (densecap_debug_rpn.h) ------------------------------------------------------------------
int dc_debug_conv3x3_wgrad(dc_ctx* ctx, const float* x, const float* dy, int h, int w_px, int Cin, int Cout, int slices, float* dw) {
  OP_PROLOGUE();
  const char* who = "dc_debug_conv3x3_wgrad";
  if (!x || !dy || !dw || slices < 0 || slices > 64) return ctx->fail(DC_E_INVALID, "%s: bad argument", who);
  DCCHK(check_conv3x3_grad_shape(ctx, h, w_px, Cin, Cout, false, who));
  const int S = slices > 0 ? slices : conv3x3_wgrad_slices(h * w_px, Cout, Cin);
  Scratch ws(ctx->scratch, s);
  HIPCHK(ws.alloc(conv3x3_wgrad_ws_floats(S, Cout, Cin) * 4));
  KCHK(launch_conv3x3_wgrad(x, dy, h, w_px, Cin, Cout, S, dw, static_cast<float*>(ws.get()), s));
  OP_EPILOGUE();
}

}  // extern "C"
