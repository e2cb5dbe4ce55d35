// Shared declarations for libdensecap_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/densecap.h"
#include "../../include/densecap_debug.h"
#include "../../include/densecap_debug_sample.h"
#include "../../include/densecap_debug_step.h"
#include "../../include/densecap_debug_beam.h"
#include "../../include/densecap_debug_grad.h"
#include "../../include/densecap_debug_recog.h"
#include "../../include/densecap_debug_bwd.h"
#include "../../include/densecap_debug_rpn.h"
#include "../../include/densecap_debug_optim.h"
#include "../../include/densecap_debug_clip.h"
#include "../../include/densecap_debug_glue.h"
#include "../../include/densecap_debug_nms.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// TH / THNN of the reference's era compute exp, sigmoid and tanh of a FloatTensor through the C DOUBLE functions and cast
// the result to float (TH: LAB_IMPLEMENT_BASIC_FUNCTION(exp, exp), TH_sigmoid(double) = 1.0 / (1.0 + exp(-x)), tanh;
// docs/SEMANTICS.md).  Both sides of the parity tests use this form: a double result is within an ulp of the true value
// in any libm, so the float it rounds to is the same on the device and in the oracle (bar one case in ~2^29).
__device__ __forceinline__ float th_expf(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float th_sigmoidf(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
__device__ __forceinline__ float th_tanhf(float x) { return (float)tanh((double)x); }

// ---- the noise of caption sampling (docs/SEMANTICS.md, "Sampling captions") ---------------------------------------------------
// Philox4x32-10 (the Random123 function): counter (c0..c3), key (k0, k1) -> four 32-bit words.  Counter-based: a word is a pure
// function of its coordinates, whichever lane, tile or launch asks for it.
struct Philox4 { uint32_t w[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// Standard Gumbel noise of 32 random bits: u = ((bits >> 9) + 0.5) * 2^-23 lies strictly inside (0, 1) and is exact in fp32, and so
// is w = 1 - u; g = -log(-log(u)) with the inner logarithm taken as log1p(-w), so that u next to 1 loses nothing (log of a number
// next to 1 would).  Within 1e-5 of the double-precision value for all 2^23 values of u
// (tests/test_gpu_sample.py evaluates the copy compiled into mfma_gemm.hip, the one that draws).
__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
  const uint32_t k = bits >> 9;
  const float w = ((float)((1u << 23) - k) - 0.5f) * 0x1p-23f;
  return -logf(-log1pf(-w));
}

__device__ __forceinline__ float sigmoidf_(float x) { return th_sigmoidf(x); }
// ---- what the decode step tails share (elementwise.hip, sample_trunc.hip) ------------------------------------------------------
// The LSTM point-wise half: thread tid owns hidden units j0 + tid + u * 256 (u < kTailUPT) of its row in the pass that starts
// at j0.  tail_load requests a pass's token-independent operands (the h.Wh gates, c); the kernels call it for j0 = 0 before
// their reduction, so the operands travel while the word is being found.  tail_update then runs every pass -- the ones past
// the first (Hd > 512) load in place -- with the word's xg row `x` (null: no embedding row) added: per element
// (x + gates_pre), sigmoid/tanh, c' = f*c + i*g, h' = o*tanh(c'), c and h in place.
constexpr int kTailUPT = 2;                         // hidden units per thread and pass (Hd = 512: one pass)
struct TailRegs { float gpre[kTailUPT][4], cprev[kTailUPT]; };
__device__ __forceinline__ void tail_load(TailRegs& r, const float* __restrict__ g, const float* __restrict__ c_row, int Hd,
                                          int j0, int tid, int zero_c) {
#pragma unroll
  for (int u = 0; u < kTailUPT; ++u) {
    const int j = j0 + tid + u * 256;
    if (j < Hd) {
#pragma unroll
      for (int q = 0; q < 4; ++q) r.gpre[u][q] = g[q * Hd + j];
      r.cprev[u] = zero_c ? 0.f : c_row[j];
    }
  }
}
__device__ __forceinline__ void tail_update(TailRegs& r, const float* __restrict__ g, const float* __restrict__ x,
                                            float* __restrict__ c_row, float* __restrict__ h_row, int Hd, int tid, int zero_c) {
  for (int j0 = 0; j0 < Hd; j0 += 256 * kTailUPT) {
    if (j0 > 0) tail_load(r, g, c_row, Hd, j0, tid, zero_c);
#pragma unroll
    for (int u = 0; u < kTailUPT; ++u) {
      const int j = j0 + tid + u * 256;
      if (j >= Hd) continue;
      float gi = r.gpre[u][0], gf = r.gpre[u][1], go = r.gpre[u][2], gg = r.gpre[u][3];
      if (x != nullptr) { gi = x[j] + gi; gf = x[Hd + j] + gf; go = x[2 * Hd + j] + go; gg = x[3 * Hd + j] + gg; }
      const float ig = sigmoidf_(gi), fg = sigmoidf_(gf), og = sigmoidf_(go);
      const float gt = th_tanhf(gg);
      const float cn = fg * r.cprev[u] + ig * gt;
      c_row[j] = cn;
      h_row[j] = og * th_tanhf(cn);
    }
  }
}

// (shared by boxes.hip and the recognition heads: one definition of the conversion every NMS input goes through)
__device__ __forceinline__ void corners(float xc, float yc, float w, float h, float& x1, float& y1, float& x2,
                                        float& y2) {
  // box_utils.xcycwh_to_x1y1x2y2 (box_utils.lua:288-291): x0 = ((w-1)/2)*-1 + xc ; x1 = (w-1)/2 + xc
  const float hw = __fdiv_rn(__fsub_rn(w, 1.f), 2.f);
  const float hh = __fdiv_rn(__fsub_rn(h, 1.f), 2.f);
  x1 = __fadd_rn(-hw, xc);
  y1 = __fadd_rn(-hh, yc);
  x2 = __fadd_rn(hw, xc);
  y2 = __fadd_rn(hh, yc);
}

// ---- the ctx's sticky device fault word: what raised it ------------------------------------------------------------------
constexpr uint32_t kFaultStreamK = 1u;   // a stream-K owner gave up waiting for a partner's partial tile (mfma_gemm.hip)
constexpr uint32_t kFaultNmsBand = 2u;   // a hand-off between the waves of nms_scan_band_kernel did not arrive (boxes.hip)

// ---- one image's packed result record (final_pack_kernel; the pinned host staging holds the same layout) ------------------
// int32 K at kRecK, uint32 fault word at kRecFault; boxes (P,4) at kRecPayload, scores (P) at rec_scores(P), and from
// rec_values(P) `words` 4-byte values per row: int32 tokens (T) or fc7 codes (D).  rec_stride: bytes of a record, 256-aligned.
constexpr size_t kRecK = 0, kRecFault = 68, kRecPayload = 256;
inline size_t rec_scores(int P) { return kRecPayload + (size_t)P * 16; }
inline size_t rec_values(int P) { return rec_scores(P) + (size_t)P * 4; }
inline size_t rec_stride(int P, size_t words) { return (rec_values(P) + (size_t)P * words * 4 + 255) & ~(size_t)255; }
// a forward on caller-supplied boxes appends int32 src (P) to the values: a record of `words` + 1 words per row
inline size_t rec_src(int P, size_t words) { return rec_values(P) + (size_t)P * words * 4; }
// int32 values between two images' NMS count slots (count1 / count2 of a lane): one 256-byte line per image
constexpr int kCountStride = 64;

// ---- ctx accessors for the other translation units (densecap.hip) ------------------
int dc_ctx_device(const dc_ctx* ctx);
void dc_ctx_set_error(dc_ctx* ctx, const char* msg);

// ---- MFMA contraction engine (mfma_gemm.hip) --------------------------------
struct GemmDesc {
  const float* A = nullptr;   // dense: (M,K) row-major; conv: (nimg,H,W,Cin) HWC activations
  const float* W = nullptr;   // (N,K) row-major, K contiguous
  const float* bias = nullptr;  // (N) or null
  float* C = nullptr;         // (M,ldc)
  int M = 0, N = 0, K = 0, ldc = 0;
  int relu = 0;
  // conv3x3 implicit GEMM (mode 1): M = nimg*H*Wd, K = 9*Cin
  int conv = 0, H = 0, Wd = 0, Cin = 0;
  // conv + fused 2x2/2 ceil-mode max-pool (one image): the M index walks POOL WINDOWS -- m = 4*window + 2*dy + dx with
  // window = wy*ceil(Wd/2) + wx in raster order of the pooled map, pixel (2wy+dy, 2wx+dx) -- so that the four pixels of
  // a window are four consecutive accumulator registers of one lane; M = 4*ceil(H/2)*ceil(Wd/2); slots outside the
  // image (odd H or Wd) read zeros and are left out of the max.  C is the POOLED map: C[window*ldc + n].
  int pool = 0;
  // Rows of ONE image when the launch carries a group of images (0 = M): every routing decision that changes the fp32
  // summation order (K-split kernel vs the sequential-K kernels, split-K factor) and the tile shape are planned on this
  // count, so an image's numbers do not depend on how many images share its launches.
  int plan_M = 0;
  // arithmetic: 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, the default and the only mode results are bit-compared in);
  // 1 = split-bf16 (dc_set_math_mode(1)): both operands split into three bf16 planes in registers, six of the nine partial
  // products accumulated in fp32 on v_mfma_f32_32x32x16_bf16 -- fp32-class accuracy at 2.67x the matrix rate
  // 2 = the same with the B operand (weights) split ONCE into planes in HBM (launch_split_planes): `sk_slots` then carries the
  // planes pointer and `sk_np` the rows of the plane matrix (stream-K, whose fields these are, does not exist in this mode)
  int bf3 = 0;                // (sits in what was the alignment hole in front of `rowterm`: no other field moved)
  // optional gathered row term (LSTM input gates): C[m][n] += rowterm[rowidx[m]*rowterm_ld + n]
  const float* rowterm = nullptr;
  const int32_t* rowidx = nullptr;   // values are 1-based token ids -> row = id-1
  int rowterm_ld = 0;
  // Sampling epilogue (densecap.hip::lm_sample_n; docs/SEMANTICS.md "Sampling captions"): samp_t >= 1 (the step) together with
  // amax_val and rowidx selects it in the place of the log-sum-exp.  rowidx[2m], rowidx[2m + 1] = the row's (r, s) of the noise
  // counter; every (row, 32-column half) writes five floats to amax_val[m * amax_ld + 5 * slot + ..]: the log-sum-exp partial
  // (max v, sum exp(v - max)) exactly as below, then the best perturbed entry (v * samp_inv_temp + g, its column as int bits, v at
  // that column), first maximum on ties; samp_inv_temp == 0: no noise and no scaling (the greedy rule).  amax_ld >= 10 per
  // 64-column tile.  The four fields sit in alignment holes, as `bf3` does: the struct keeps its size, so neither a field nor a
  // kernel argument behind the descriptor moves and no existing kernel's code changes.
  // Where they are (offsets in bytes; the remaining hole is at 196, behind sk_np): samp_t 100 (behind rowterm_ld), samp_seed_lo 132
  // (behind amax_n), samp_seed_hi 148 (behind splitk), samp_inv_temp 180 (behind walk).
  int samp_t = 0;
  // rowidx together with amax_val (and no rowterm): fused row LOG-SUM-EXP instead of the arg-max (teacher-forced scoring,
  // densecap.hip::lm_score).  rowidx[m] = the row's 1-based target token (column rowidx[m] - 1 < amax_n); every (row, 32-column
  // half) writes its partial (max v, sum exp(v - max)) over the real columns to amax_val[m * amax_ld + 2 * slot + {0, 1}] (slot as
  // for the arg-max), the lane holding the target column writes the biased target logit to amax_val[m * amax_ld + amax_ld - 1];
  // amax_ld >= 4 * ceil(amax columns / 64) + 1, amax_idx unused.  Same routes, tiles and amax_cols handling as the arg-max.
  // optional fused row arg-max (vocab projection): instead of storing C, every (row, 32-column half of a 64-column tile)
  // writes its best (value, column) to amax_val/amax_idx[m * amax_ld + 2 * tile_n + half] (columns ascend with the slot);
  // amax_ld >= 2 * ceil(N / 64); C may be null.
  float* amax_val = nullptr;
  int32_t* amax_idx = nullptr;
  int amax_ld = 0;
  // arg-max over a PREFIX of the columns (decode step: W = [vocab rows; pad; Wh rows], both products share A = h_t):
  // columns [0, amax_cols) (a multiple of 64) get the arg-max epilogue, of which [0, amax_n) are real vocabulary
  // entries; columns [amax_cols, N) are stored raw to C[m*ldc + (n - amax_cols)].  amax_cols = 0: every column.
  int amax_cols = 0;
  int amax_n = 0;
  uint32_t samp_seed_lo = 0;  // sampling epilogue: the noise key (seed & 0xffffffff, seed >> 32) ...
  // optional device-side row count: effective M = min(M, *m_dev); workgroups past it exit at once
  const int32_t* m_dev = nullptr;
  // split-K (K-split 128x128 kernel only): `splitk` workgroups share one tile, each sums a contiguous K range
  // and writes its raw partial tile to splitk_ws[(slice*M + m)*N + n]; launch_splitk_reduce finishes the job
  int splitk = 1;
  uint32_t samp_seed_hi = 0;  // ... its upper half
  float* splitk_ws = nullptr;
  // stream-K over the tiles of rows [m_begin, M) (K-split kernel, launch_mfma_gemm_sk): sk_lo[0..sk_wgs] = unit offsets
  // of the workgroups on the line of K units (unit = 2 K-tiles, sk_np units per tile, tiles n-fastest); sk_slots =
  // sk_wgs partial tiles of 128x128 floats; sk_flags[0..sk_wgs) zeroed before the launch; sk_fault = sticky device word
  // raised when an owner gives up waiting for a partner (checked by the host with the results)
  int stages = 0;             // LDS ring depth of the 128x64-tile kernel: 0 = by tile count, 3 (two workgroups per CU) or 2 (three per CU)
  int force_cfg = 0;          // measurement hook (dc_debug_set "force_cfg"): 0 = planned, 1 = 128x128, 2 = 128x64, 3 = 64x64 tiles; 4 = planned tiles, no split-K;
                              // 5 = 128x128 tiles on the v2 kernel with a two-stage ring (two workgroups per CU); 6 = the K-split 128x128 kernel whatever K
  int stagger = 0;            // measurement hook (dc_debug_set "stagger"): workgroups start after a pseudo-random pause of up to this many 64-cycle sleeps
  int epi_wide = 1;           // interior tiles of plain epilogues leave as 16-byte stores staged through the wave's LDS (dc_debug_set "epi_wide": 0 = dword stores)
  int walk = 0;               // measurement hook (dc_debug_set "walk"): 128x64 launches run one workgroup per slot that walks its tiles
  float samp_inv_temp = 0.f;  // sampling epilogue: 1 / temperature in fp32, 0 = the greedy rule
  const int* sk_lo = nullptr;
  int sk_np = 0;
  float* sk_slots = nullptr;
  unsigned* sk_flags = nullptr;
  unsigned* sk_fault = nullptr;
  // row window (K-split kernel only): tiles cover rows [m_begin, M); a_rows = rows of the whole A operand
  // (extent of the conv input for the buffer descriptor) when M is only a prefix, 0 = M
  int m_begin = 0;
  int a_rows = 0;
};
static_assert(offsetof(GemmDesc, samp_t) == 100 && offsetof(GemmDesc, samp_seed_lo) == 132 && offsetof(GemmDesc, samp_seed_hi) == 148 &&
              offsetof(GemmDesc, samp_inv_temp) == 180, "the sampling fields sit in the alignment holes listed at samp_t");
static_assert(sizeof(GemmDesc) == 232, "GemmDesc is a kernel argument: a new field goes into an alignment hole or every kernel's argument offsets move");
// C = act(sum_s ws[s] + bias): fixed summation order s = 0..S-1
// m_dev (optional): device-side row count, rows >= *m_dev are left alone (their partials were never written)
hipError_t launch_splitk_reduce(const float* ws, int S, const float* bias, float* C, int M, int N, int ldc, int relu,
                                hipStream_t s, const int32_t* m_dev = nullptr);
// same for a pooled conv (GemmDesc::pool): ws rows are window-ordered slots [m_begin, m_begin+M); C_pooled is the base
// of the whole pooled map
hipError_t launch_splitk_reduce_pool(const float* ws, int S, const float* bias, float* C_pooled, int m_begin, int M, int N,
                                     int ldc, int H, int Wd, int relu, hipStream_t s);
// can this conv problem take GemmDesc::pool (operands within the kernels' 32-bit buffer offsets)?
bool mfma_gemm_can_pool(const GemmDesc& d);
// Largest image group a launch may carry (dc_set_group).  Split-K factors are functions of ONE image's problem, so the
// partial-output workspace test assumes a group of this size: an image gets the same factor in every group.
constexpr int kGemmMaxGroup = 8;
// split factor launch_mfma_gemm would like for this problem (1 = none)
int mfma_gemm_splitk(const GemmDesc& d, size_t ws_floats);      // ws_floats: capacity of the partial-output workspace
// Tail plan for problems whose 128x128 tile count is not a multiple of the 256 CUs: rows [0, m_split) run as
// whole tiles (full rounds), rows [m_split, M) are split `tail_splitk` ways along K so the last partial round
// fills the chip.  Returns false when it does not pay.
bool mfma_gemm_tail_plan(const GemmDesc& d, int* m_split, int* tail_splitk);
// Stream-K plan for the last, partial round of 128x128 tiles: rows [0, m_split) as whole tiles, the tiles of rows
// [m_split, M) shared along K by `wgs` workgroups (np = K units per tile).  false when it does not pay.
bool mfma_gemm_sk_plan(const GemmDesc& d, int* m_split, int* wgs, int* np);
size_t mfma_gemm_sk_ws_floats(int wgs);
hipError_t launch_mfma_gemm_sk(const GemmDesc& d, int wgs, int np, float* ws, hipStream_t stream);
// force the K-split 128x128 kernel (honours m_begin / a_rows / splitk)
hipError_t launch_mfma_gemm_ks(const GemmDesc& d, hipStream_t stream);
// How a contraction is carried out (mfma_gemm_plan): kind = what run_gemm does around the launch, route = the kernel family.
enum { GEMM_PLAN_PLAIN = 0, GEMM_PLAN_SPLITK = 1, GEMM_PLAN_STREAMK = 2, GEMM_PLAN_TAIL = 3 };
enum { GEMM_ROUTE_KS = 0, GEMM_ROUTE_V2_128x64 = 1, GEMM_ROUTE_V2_128x128 = 2, GEMM_ROUTE_V2_64x64 = 3 };
struct GemmPlan {
  int kind = GEMM_PLAN_PLAIN, route = GEMM_ROUTE_KS;
  int stages = 0;            // LDS ring depth of a 128x64 launch (2 or 3), 0 otherwise
  int splitk = 1;            // GEMM_PLAN_SPLITK
  int m_split = 0;           // GEMM_PLAN_STREAMK / GEMM_PLAN_TAIL: rows [0, m_split) run as whole tiles
  int sk_wgs = 0, sk_np = 0; // GEMM_PLAN_STREAMK
  int tail_splitk = 1;       // GEMM_PLAN_TAIL
};
// Pure function of the problem, the scheduling mode and the workspace size (no device needed beyond its CU count).
void mfma_gemm_plan(const GemmDesc& d, bool serial_mode, int tail_mode, size_t ws_floats, GemmPlan* plan);
// Launches the fp32 MFMA kernel on `stream`; returns hipSuccess or the launch error.
hipError_t launch_mfma_gemm(const GemmDesc& d, hipStream_t stream);
double gemm_flops(const GemmDesc& d);
// does the split-bf16 mode pay for this contraction (enough tiles for ONE image to fill the chip without K sharing)?
bool mfma_gemm_bf3_pays(const GemmDesc& d);

// ---- element-wise / layout kernels (elementwise.hip) ---------------------------
hipError_t launch_chw_to_hwc(const float* in, float* out, int C, int H, int W, hipStream_t s);
hipError_t launch_hwc_to_chw(const float* in, float* out, int C, int H, int W, hipStream_t s);
hipError_t launch_pack_conv3x3(const float* w_oihw, float* w_packed, int Cout, int Cin, hipStream_t s);
int device_cu_count();      // compute units of the current device (256 on MI355X); cached per device
void set_planning_cu_override(int cus);   // dc_debug_plan_gemm only: this thread's planners see `cus` CUs until reset with 0
hipError_t launch_conv3x3_c3(const float* in_chw, const float* w_oihw, const float* bias, float* out_hwc, int nimg,
                             int H, int W, int Cout, int relu, hipStream_t s);
hipError_t launch_maxpool2x2_ceil(const float* in, float* out, int nimg, int H, int W, int C, hipStream_t s);
hipError_t launch_transpose2d(const float* in, float* out, int rows, int cols, hipStream_t s);
// fc6 weight (N, C*HH*WW) with k = c*HW + p  ->  k' = p*C + c
hipError_t launch_permute_fc6(const float* in, float* out, int N, int C, int HW, hipStream_t s);
// LSTM pointwise: gates (n,4Hd) [i f o g], c (n,Hd) in/out, h (n,Hd) out
hipError_t launch_lstm_pointwise(const float* gates, float* c, float* h, int n, const int32_t* n_dev, int Hd,
                                  int zero_c, hipStream_t s);
hipError_t launch_fill_i32(int32_t* p, int32_t v, int n, hipStream_t s);
// idx[i] = i for i < cap, *count_out = *count_in
hipError_t launch_iota_count(int32_t* idx, int32_t* count_out, const int32_t* count_in, int cap, hipStream_t s);
// One decode step's row-wise tail (LanguageModel.lua:316-335 between two GEMMs), one workgroup per row
// (a wave per row was measured slower: 11.4 vs 8.3 us -- the row's 2048 gate values want 256 lanes in flight):
//   pval != null: tok = 1 + argmax over the row's `ntiles` partials (first max on ties), seq[m*T+t] = tok;
//                 else tok = fixed_tok (START, or 0 = no input-gate row term);
//   gates = (tok ? xg[(tok-1)*4Hd ..] : 0) + gates_pre[m]  (same association as torch-rnn: (b + x.Wx) + h.Wh);
//   [i f o g] -> c' = f*c + i*g (c = 0 if zero_c), h' = o*tanh(c').  gates_pre == null: arg-max only.
hipError_t launch_lstm_step_tail(const float* pval, const int32_t* pidx, int ntiles, int ld, int fixed_tok,
                                 const float* xg, const float* gates_pre, float* c, float* h, int n,
                                 const int32_t* n_dev, int Hd, int zero_c, int32_t* seq, int T, int t, hipStream_t s);
// ---- screened greedy decode (Settings::decode_screen) ----
// Screen (decode_screen.hip): scores[m*V1pad + j] = fp16(bias[j] + sum_k hb[m][k] * wb[j][k]) in bf16 MFMA arithmetic, for rows
// below the live count (m_dev as in GemmDesc) and columns j < V1.  hb: (M, Kp) bf16, wb: (V1pad, Kp) bf16, Kp % 64 == 0.
hipError_t launch_decode_screen(const uint16_t* hb, const uint16_t* wb, const float* bias, void* scores, int M,
                                const int32_t* m_dev, int V1, int V1pad, int Kp, hipStream_t s);
// hb[m] = bf16(h[m]) (zero from Hd to Kp), hnorm[m] >= |h[m]|_2, for the rows below the live count
hipError_t launch_screen_operands(const float* h, int n, const int32_t* n_dev, int Hd, int Kp, uint16_t* hb, float* hnorm,
                                  hipStream_t s);
// The step tail of the screened route, one workgroup per row: tok = 1 + the arg-max of the fp32 logits h.W^T + bias exactly as
// the fused step forms them, found among the columns the scores cannot rule out (or among all: see the kernel);
// seq[m*T + t] = tok; cand[m*T + t] = the row's candidate count (-1: a non-finite score or bound); bestv[m] = the winner's
// logit.  Then, gates_pre != null, the LSTM update of launch_lstm_step_tail with tok fed, and hb / hnorm of the new h.
struct RescoreTail {
  const _Float16* scores; int ld;                 // (n, ld) fp16
  const _Float16* wnorm;                          // |W_j|_2 rounded up to fp16 (ld of them, zero past V1)
  const float *W, *bias; int V1;                  // W (V1, Hd) fp32; bias (V1)
  float cbound;                                   // c of the bound b_j = c |h| |W_j| + ...
  const float *xg, *gates_pre;
  float *c, *h; int n; const int32_t* n_dev; int Hd;
  int32_t* seq; int T, t;
  uint16_t* hb; int Kp; float* hnorm;             // hnorm: read for this step, rewritten for the next
  int32_t* cand; float* bestv;
};
hipError_t launch_lstm_rescore_tail(const RescoreTail& a, hipStream_t s);
// dynamic LDS the tail needs for rows of Hd and ld scores; the route exists where it fits kScreenTailMaxLds (the kernel's 560
// bytes of static LDS come on top: 66,096 bytes at the edge launch on gfx950 as they are -- DESIGN.md §4.1c, test set lds_last)
size_t screen_tail_lds_bytes(int Hd, int ld);
constexpr size_t kScreenTailMaxLds = 64 * 1024;
// Teacher-forced scoring step tail (densecap.hip::lm_score), one workgroup per row m < n: lse = log-sum-exp of the row's
// `nslots` partials (part[m*ld + 2s], part[m*ld + 2s + 1]: max, sum), combined in double in a fixed order; the target logit
// part[m*ld + ld - 1]; acc[m] += (double)tlogit - lse.  Then, if the row's target tgt[m] is not `end_tok` and gates_pre != null,
// the LSTM point-wise update of lstm_step_tail with the target fed: gates = xg[tgt - 1] + gates_pre[m], c, h in place.
// dst_a / dst_b = `copies` back-to-back repeats of src_a / src_b (len floats each, len % 4 == 0)
hipError_t launch_repeat_rows2(const float* src_a, const float* src_b, size_t len, int copies, float* dst_a, float* dst_b,
                               hipStream_t s);
hipError_t launch_lse_step_tail(const float* part, int nslots, int ld, const int32_t* tgt, int end_tok, const float* xg,
                                const float* gates_pre, float* c, float* h, double* acc, int n, int Hd, hipStream_t s);
// Sampling step tail (densecap.hip::lm_sample_n), one workgroup per row m < n, on the partials of the sampling epilogue
// (GemmDesc::samp_t; part[m*ld + 5s + 0..4] = max, sum, best perturbed score, its column, the logit there): tok = 1 + column of
// the best perturbed entry over the slots (first maximum on ties); lse as launch_lse_step_tail forms it; with fin[m] == 0:
// seq[m*T + t] = tok, acc[m] += (double)logit - lse, and fin[m] = 1 if tok == end_tok; with fin[m] != 0: seq[m*T + t] = 0.
// Then, gates_pre != null, the LSTM point-wise update of lstm_step_tail with tok fed, finished or not (every row runs all T steps).
hipError_t launch_sample_step_tail(const float* part, int nslots, int ld, int end_tok, const float* xg, const float* gates_pre,
                                   float* c, float* h, double* acc, uint8_t* fin, int32_t* seq, int T, int t, int n, int Hd,
                                   hipStream_t s);
// ---- truncated sampling (sample_trunc.hip; docs/SEMANTICS.md, "Truncation: top-k and nucleus") ----
// One workgroup per row m < rows on the row's V1 logits (logits + m*ld) held in LDS: the kept set of (top_k, top_p) at 1/inv_temp,
// tok = 1 + the Gumbel-max over it with the noise of (seed, keys[2m + 1] = s, keys[2m] = r, t), lower column on ties; then, as
// launch_sample_step_tail: with fin[m] == 0 seq[m*T + tpos] = tok, acc[m] += log p(tok) (temperature 1, untruncated), acc_q[m] +=
// log q(tok) (under the truncated distribution), fin[m] = 1 at end_tok; with fin[m] != 0 seq = 0.  A row without a word writes 0,
// NaN to both sums and ends.  gates_pre != null: the LSTM point-wise update with tok fed, finished or not.  acc, acc_q, fin and
// the four per-row outputs of the test hook (kept: words kept, -1 = no word; theta: raw score of the last kept rank; lp, lq: this
// step's two terms) may each be null.
struct SampleTruncArgs {
  const float* logits; int ld, V1;
  const int32_t* keys; int t; uint32_t seed_lo, seed_hi;
  float inv_temp; int top_k; float top_p;
  int end_tok;
  const float *xg, *gates_pre; float *c, *h; int Hd;
  double *acc, *acc_q; uint8_t* fin;
  int32_t* seq; int T, tpos;
  int32_t* kept_out; float* theta_out; double *lp_out, *lq_out;
};
size_t sample_trunc_max_vocab();    // largest V+1 whose row and the kernel's workspace fit the LDS of the current device
hipError_t launch_sample_trunc_rows(const SampleTruncArgs& a, int rows, hipStream_t s);
// test hooks of the sampling noise (mfma_gemm.hip, so that the build that draws the words is the one tested; dc_debug_fetch): out[i] = gumbel_from_bits((first + i) << 9), i < count;
// bits[i] = the Philox word of the coordinates srtv[4i..4i+3] = (s, r, t, v) under `seed`
hipError_t launch_sample_noise_gumbel(uint32_t first, size_t count, float* out, hipStream_t s);
hipError_t launch_sample_noise_bits(uint64_t seed, const int32_t* srtv, size_t count, uint32_t* bits, hipStream_t s);
// split-bf16 mode: W (N, K) fp32 -> 3 x N x K bf16 planes, k permuted per 32-tile as the kernels read them (elementwise.hip)
hipError_t launch_split_planes(const float* W, uint16_t* planes, size_t N, int K, hipStream_t s);
// objectness + box regression heads + final ApplyBoxTransform (DenseCapModel.lua:134,139-140)
// final_xyxy (optional): the final boxes as corners too (box_utils.xcycwh_to_x1y1x2y2), what the final NMS reads
hipError_t launch_recog_heads(const float* codes, const float* w5 /*(5,D): obj, 4 boxreg*/, const float* b5,
                              const float* roi_boxes, float* obj, float* trans, float* final_boxes, float* final_xyxy,
                              int n, int D, hipStream_t s);

// hipFuncAttributeMaxDynamicSharedMemorySize per (device, kernel) -- mfma_gemm.hip
hipError_t ensure_dyn_lds(const void* fn, size_t bytes);

// ---- beam search row kernels (beam.hip; LanguageModel.lua:170-290) --------------------------
size_t beam_topk_max_vocab();     // largest V+1 whose row fits the top-k kernel's LDS on the current device
hipError_t launch_beam_logsoftmax_topk(const float* logits, int rows, int V1, int ld, const uint8_t* finished, int k,
                                       float* top_lp, int32_t* top_idx, hipStream_t s);
hipError_t launch_beam_init(const float* top_lp, const int32_t* top_idx, int nprop, int beam, int T, int END,
                            float* beam_lp, int32_t* beams, int32_t* parent, int32_t* cur_tok, uint8_t* finished,
                            hipStream_t s);
hipError_t launch_beam_merge(const float* top_lp, const int32_t* top_idx, const float* beam_lp_in,
                             const int32_t* beams_in, int nprop, int beam, int T, int t, int END, float* beam_lp_out,
                             int32_t* beams_out, int32_t* parent, int32_t* cur_tok, uint8_t* finished, hipStream_t s);
hipError_t launch_beam_gather_state(const float* h_in, const float* c_in, const int32_t* parent, int rows, int beam,
                                    int src_per_prop, int Hd, float* h_out, float* c_out, hipStream_t s);
hipError_t launch_beam_best(const int32_t* beams, int nprop, int beam, int T, int32_t* seq, hipStream_t s);
// the standard search (docs/SEMANTICS.md, "Standard beam search"): first expansion, merge, final ranking
hipError_t launch_beam_std_init(const float* top_lp, const int32_t* top_idx, int nprop, int beam, int T, int END, float* beam_lp,
                                int32_t* beams, int32_t* len, int32_t* parent, int32_t* cur_tok, uint8_t* finished,
                                hipStream_t s);
hipError_t launch_beam_std_merge(const float* top_lp, const int32_t* top_idx, const float* beam_lp_in, const int32_t* beams_in,
                                 const int32_t* len_in, const uint8_t* fin_in, int nprop, int beam, int T, int t, int END,
                                 float* beam_lp_out, int32_t* beams_out, int32_t* len_out, int32_t* parent, int32_t* cur_tok,
                                 uint8_t* fin_out, hipStream_t s);
hipError_t launch_beam_std_finish(const float* beam_lp, const int32_t* beams, const int32_t* len, const float* pen, int has_pen,
                                  int nprop, int beam, int T, int n_best, int32_t* captions, float* logprob, hipStream_t s);

// ---- box pipeline (boxes.hip) ------------------------------------------------------
hipError_t launch_make_anchors(float* out, int h, int w, float x0, float y0, float sx, float sy,
                               const float* anchors, int k, hipStream_t s);
hipError_t launch_apply_box_transform(const float* boxes, const float* trans, float* out, int n, hipStream_t s);
hipError_t launch_clip_boxes(const float* boxes, float* clipped, uint8_t* valid, int n, float x_min, float y_min,
                             float x_max, float y_max, hipStream_t s);
hipError_t launch_xcycwh_to_x1y1x2y2(const float* boxes, float* out, int n, hipStream_t s);
hipError_t launch_box_iou(const float* b1, const float* b2, float* out, int B1, int B2, int convention,
                          hipStream_t s);
// (nimg images of a group side by side: every per-image tensor follows the previous image's)
hipError_t launch_rpn_decode(const float* heads, int nimg, int h, int w, int k, const float* anchors, float x0, float y0,
                             float sx, float sy, int img_h, int img_w, float* boxes, float* anchors_out,
                             float* trans, float* x1y1x2y2, float* p, uint8_t* valid, int clip, hipStream_t s);
struct NmsWorkspace {
  // device scratch, sized for n_cap boxes (see boxes.hip)
  int n_cap = 0;
  uint32_t* keys = nullptr;       // (n) order-preserving sort keys
  int32_t* tmp_idx = nullptr;     // (n) bucketed (unordered inside a bucket) indices
  uint32_t* tmp_key = nullptr;    // (n) their keys, same order
  int32_t* order = nullptr;       // (n) sorted position -> original index
  float* sboxes = nullptr;        // (n,4) boxes in sorted order
  float* sarea = nullptr;         // (n)
  int32_t* pick_pos = nullptr;    // (n) sorted positions of the picks so far
  int32_t* hist = nullptr;        // (NMS_BUCKETS)
  int32_t* cursor = nullptr;      // (NMS_BUCKETS)
  int32_t* off = nullptr;         // (NMS_BUCKETS)
  int32_t* state = nullptr;       // {count, done}
  int32_t* nvalid = nullptr;      // (1)
  unsigned long long* removed0 = nullptr;  // (ceil(n/64)) bits suppressed by picks of earlier windows
  unsigned long long* mask = nullptr;      // window bit mask
  unsigned long long* nearband = nullptr;  // (4096, 4) words c, c-1, c-2, c-3 of every row of a window of <= 4096 rows
  size_t mask_words = 0;
  size_t zero_bytes = 0;          // hist..removed0 are contiguous and zeroed per call
};
size_t nms_workspace_bytes(int n);
hipError_t nms_workspace_bind(NmsWorkspace& ws, void* base, int n);
// n_dev (optional device int32) overrides n at run time (n is then the capacity)
// fault (optional): the ctx's sticky device word; nms_scan_band_kernel stores kFaultNmsBand there when a hand-off between its
// waves did not arrive within the spin bound (the host then fails the call and switches the band scan off)
// band: windows of <= NMS_BAND_ROWS rows take nms_scan_band_kernel (false: every window through nms_scan_kernel -- an A/B and
// bisecting switch, the picks are the same)
hipError_t launch_nms(NmsWorkspace& ws, const float* boxes, const float* scores, const uint8_t* valid, int n,
                      const int32_t* n_dev, float thresh, int max_boxes, int32_t* picks, int32_t* count, bool band,
                      hipStream_t s, uint32_t* fault);
// Multi-order NMS (boxes.hip): the greedy NMS of launch_nms on ONE box list (n <= 4096 rows, x1y1x2y2) under the Q score columns
// of scores (n, Q), entry r*Q + q, side by side: picks (Q, max_picks) int32, -1 past counts[q].  Rows with valid[r] == 0 (valid
// may be null) or a NaN score in column q are no candidates of q.  ws: nms_multi_workspace_bytes(n) of device scratch (the shared
// suppression bit mask).  n_dev (optional device int32) overrides n at run time (n is then the capacity).
size_t nms_multi_workspace_bytes(int n);
hipError_t launch_nms_multi(void* ws, const float* boxes, const float* scores, const uint8_t* valid, int n,
                            const int32_t* n_dev, int Q, float thresh, int max_picks, int32_t* picks, int32_t* counts,
                            hipStream_t s);
// Evaluation (eval_match.hip): per image, the detections in score order against the merged ground truth; one workgroup an image.
// max_b / max_m: the largest detection / ground-truth count of any image (<= 4096 / 512), which size the dynamic LDS.  thr: the
// merge threshold as the double it is compared in.  Outputs are ragged like the inputs (see dc_op_eval_match).
hipError_t launch_eval_match(const float* det_boxes, const float* det_scores, const int32_t* det_off, const float* gt_boxes,
                             const int32_t* gt_off, int n_images, int max_b, int max_m, double thr, int claim_last,
                             int32_t* order, double* ov, int32_t* group, uint8_t* ok, int32_t* gt_group, int32_t* n_groups,
                             double* merged_boxes, hipStream_t s);
// nn.BoxSampler (train_losses.hip; docs/SEMANTICS.md, "Validation losses"): match the A inputs against the G <= 512 ground-truth
// boxes, assign positives and negatives, draw.  Outputs as dc_op_box_sampler documents them; ws: box_sampler_ws_bytes(A, G) of
// device scratch.  forced_pos / forced_neg: device lists of 0-based ranks in the class's ascending candidate list, or null.
struct BoxSamplerArgs {
  const float* boxes; const float* gt; int A, G;
  float x_max, y_max; int bounds;
  float high, low; int batch; uint32_t seed_lo, seed_hi;
  const int32_t* forced_pos; int n_forced_pos;
  const int32_t* forced_neg; int n_forced_neg;
  int32_t *pos_input_idx, *pos_target_idx, *neg_input_idx, *counts;
  float* max_iou_user; int32_t* arg_user;
  void* ws;
};
size_t box_sampler_ws_bytes(int A, int G);
hipError_t launch_box_sampler(const BoxSamplerArgs& a, hipStream_t s);
// The RPN's raw two-class scores as (k*h*w, 2) rows in ReshapeBoxFeatures order, read from the heads buffer (channel 4k + 2a + d)
hipError_t launch_rpn_score_rows(const float* heads, int h, int w, int k, float* out, hipStream_t s);
// The five criteria and their total (train_losses.hip), one workgroup, every sum a fixed tree of doubles over the sampled rows:
// scores (A,2), anchors / trans (A,4) of the RPN; the sampler's lists; gt (G,4); roi_boxes / final_trans (n,4) and obj (n) of the
// n = num_pos + num_neg <= 1024 sampled rows, positives first; rowlik (num_pos) the rows' caption log-likelihoods; L the label
// width.  out: six doubles (mid objectness, mid box, end objectness, end box, captioning, total); out_masked: rows masked in the
// two box terms.  A term is computed only if its input is non-null -- mid objectness: scores; mid box: anchors; end objectness:
// obj; end box: roi_boxes; captioning: rowlik -- and is 0.0, with no masked row, otherwise; it reads its own inputs only.
struct LossTermArgs {
  const float *scores, *anchors, *trans, *gt, *roi_boxes, *final_trans, *obj;
  const int32_t *pos_input_idx, *pos_target_idx, *neg_input_idx;
  const double* rowlik;
  int num_pos, num_neg, L;
  float w_mid_box, w_mid_obj, w_end_box, w_end_obj, w_cap;
  double* out; int32_t* out_masked;
};
hipError_t launch_loss_terms(const LossTermArgs& a, hipStream_t s);
// out[i] = src[idx[i]] rows of `width` floats for i < *count (rows >= *count zero-filled up to cap)
hipError_t launch_gather_rows(const float* src, const int32_t* idx, const int32_t* count, int cap, int width,
                              float* out, hipStream_t s);
hipError_t launch_gather_rows_i32(const int32_t* src, const int32_t* idx, const int32_t* count, int cap, int width,
                                  int32_t* out, hipStream_t s);

// ---- language-model gradients (lm_grad.hip; docs/SEMANTICS.md, "Language-model gradients") ----
// Weight gradient C(N,K) = sum_m A(m,N) * B(m,K) (rows of lda / ldb / ldc floats) on the fp32 MFMA, both operands read as they
// lie in memory.  The rows are shared by wgrad_slices(M, N, K) workgroups per tile (a function of the sizes and the device
// alone); with more than one, `ws` holds wgrad_ws_floats floats of partial tiles that a second launch adds in slice order.
int wgrad_slices(int M, int N, int K);
size_t wgrad_ws_floats(int M, int N, int K);
hipError_t launch_wgrad(const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc, float* ws,
                        hipStream_t s);
// out[c] = sum_m X[m][c] for c < N, a fixed tree of doubles
hipError_t launch_colsum(const float* X, int ldx, int M, int N, float* out, hipStream_t s);
// rows of logits (ld floats, V1 real columns) to rows of (softmax - onehot(tgt - 1)) * scale in place, columns past V1 zeroed;
// lse_out (optional): the rows' log-sum-exp
hipError_t launch_softmax_grad(float* x, int ld, int V1, const int32_t* tgt, float scale, double* lse_out, int rows, hipStream_t s);
// LSTM cell backward on `rows` rows (see the kernel): dgates (rows, 4Hd) in gate order i, f, o, g and dc_prev (rows, Hd)
hipError_t launch_lstm_cell_bwd(const float* gates_pre, const int32_t* tok, const float* xg, const float* c_prev, const float* c,
                                const float* dh_a, const float* dh_b, const float* dc_in, float* dgates, float* dc_prev, int rows,
                                int Hd, hipStream_t s);
hipError_t launch_embed_rows(const float* emb, const int32_t* tok, int rows, int E, float* out, hipStream_t s);
hipError_t launch_scatter_rows(const float* src, const int32_t* perm, int rows, int width, float* out, hipStream_t s);
// demb[ids[t] - 1] = sum of dx[rows[i]] for i in [seg[t], seg[t + 1]), in that order, for t < ntok
hipError_t launch_embed_segsum(const float* dx, int E, const int32_t* rows, const int32_t* seg, const int32_t* ids, int ntok,
                               float* demb, hipStream_t s);

// the fc7 rows the final NMS kept, of all images of a group, packed into one row block in pick order; *total = their number
hipError_t launch_survivor_compact(const float* codes, const int32_t* picks, const int32_t* count, int count_stride, int nimg,
                                   int P, int D, float* out, int32_t* total, hipStream_t s);

// the results of a group of images gathered by their final-NMS picks into packed records (see final_pack_kernel);
// tok_gather: 1 = token rows are per RoI (gathered by pick), 0 = already in final order per image, 2 = final order, packed over the group
// box_src != null (a forward on caller-supplied boxes): every record also carries int32 box_src[pick] per row, at rec_src
hipError_t launch_final_pack(const float* final_boxes, const float* obj, const int32_t* tokens, int tok_gather,
                             const float* codes, const int32_t* picks, const int32_t* count, int count_stride,
                             const uint32_t* fault, int nimg, int P, int T, int D, void* pack, size_t stride, hipStream_t s,
                             const int32_t* box_src = nullptr);

// Caller-supplied boxes in the place of the RPN's: image i of the group has in_n[i] (device) rows at in + i*P*4; the rows that
// stay (all of them, or with `clip` those that box_utils.clip_boxes leaves valid, clipped) go to roi_boxes in their order,
// their caller-side row index to box_src, their number to count[i * count_stride] (boxes_ingest_kernel)
hipError_t launch_boxes_ingest(const float* in, const int32_t* in_n, int nimg, int P, int clip, int img_h, int img_w,
                               float* roi_boxes, int32_t* box_src, int32_t* count, int count_stride, hipStream_t s);

// ---- bilinear RoI pooling (roipool.hip) ---------------------------------------------
// group form: nimg feature maps feat_stride floats apart, B rows of boxes / output per image, live counts
// B_dev[image * bdev_stride]; pick != null: box b of an image = src_boxes[image * src_stride + pick[b]], also written to boxes
hipError_t launch_bilinear_roi_pool_group(const float* feat_hwc, size_t feat_stride, int nimg, int h, int w, int C,
                                          float* boxes, int B, const int32_t* B_dev, int bdev_stride,
                                          const int32_t* pick, const float* src_boxes, size_t src_stride, int img_h,
                                          int img_w, int HH, int WW, float* out, int out_layout, hipStream_t s);
hipError_t launch_bilinear_roi_pool(const float* feat_hwc, int h, int w, int C, const float* boxes, int B,
                                    const int32_t* B_dev, int img_h, int img_w, int HH, int WW, float* out,
                                    int out_layout, hipStream_t s);

// ---- backward of bilinear RoI pooling (recog_grad.hip; docs/SEMANTICS.md, "Recognition-net gradients") ----
// The tap list and the inverted index of B rows of HH x WW points on an h x w map (npix = h * w, T = B * HH * WW * 4 taps):
// tap t = (row * HH * WW + point) * 4 + k lands on pixel tap_pix[t] (-1: outside the map) with weight tap_w[t]; pixel i's taps
// are list[start[i] .. start[i + 1]) in ascending order.  count, cursor, chunk0, item_pix and part belong to the kernels.
struct RoiGradWs {
  int32_t *tap_pix, *list, *count, *start, *cursor, *chunk0, *item_pix;
  float *tap_w, *part;
};
size_t roi_grad_ws_bytes(int B, int P, int npix, int C);
RoiGradWs roi_grad_carve(void* base, int B, int P, int npix, int C);
hipError_t launch_roi_tap_index(const float* boxes, int B, int h, int w, int img_h, int img_w, int HH, int WW, const RoiGradWs& ws,
                                hipStream_t s);
// dfeat (h, w, C) = the scatter sum of dout (B, HH, WW, C) over the index (every pixel is written; an untouched one is +0.0)
hipError_t launch_roi_scatter_sum(const float* dout, int B, int h, int w, int C, int HH, int WW, const RoiGradWs& ws, float* dfeat,
                                  hipStream_t s);
// dboxes (B, 4): d/d(xc, yc, w, h) of sum(dout * pooled) with the floors held constant
hipError_t launch_roi_box_grad(const float* feat_hwc, int h, int w, int C, const float* boxes, int B, int img_h, int img_w, int HH,
                               int WW, const float* dout, float* dboxes, hipStream_t s);

// the two end criteria's gradients in one launch (see end_crit_grad_kernel): dobj (n), dtrans and danchor (np, 4), *masked
hipError_t launch_end_crit_grad(const float* obj, const float* trans, const float* anchors, const float* target, int n, int np,
                                float w_obj, float w_box, float* dobj, float* dtrans, float* danchor, int32_t* masked, hipStream_t s);
// the recognition heads' backward: dcodes (n, D), dw5 (5, D) and db5 (5) in the order obj, 4 boxreg; g (np, D) or null
hipError_t launch_heads_bwd(const float* codes, const float* w5, const float* dobj, const float* dtrans, const float* g, int n, int np,
                            int D, float* dcodes, float* dw5, float* db5, hipStream_t s);
// (N, HW*C) with k' = p*C + c  ->  k = c*HW + p, the inverse of launch_permute_fc6; C % 64 == 0, HW <= 64, N <= 65535
hipError_t launch_permute_fc6_back(const float* in, float* out, int N, int C, int HW, hipStream_t s);
// out[r] = a[r] + (r < np ? b[r] : 0), n rows of four floats
hipError_t launch_add_pos_rows4(const float* a, const float* b, int n, int np, float* out, hipStream_t s);

// ---- backward of a 3x3 / stride 1 / pad 1 convolution (rpn_grad.hip; docs/SEMANTICS.md, "Convolution gradients") ----
// dw (Cout, Cin, 3, 3) = sum over the pixels of dy (h, w, Cout) times the nine shifted copies of x (h, w, Cin), zero outside the
// map, on the fp32 MFMA; no im2col buffer.  The pixels are shared by S slices per tile (1..64; conv3x3_wgrad_slices is the
// production choice, a function of the sizes and the device alone); `ws` holds conv3x3_wgrad_ws_floats(S, ..) floats of partial
// tiles, added in slice order.  Cin % 32 == 0, h * w <= 65536.
int conv3x3_wgrad_slices(int P, int Cout, int Cin);
size_t conv3x3_wgrad_ws_floats(int S, int Cout, int Cin);
hipError_t launch_conv3x3_wgrad(const float* x, const float* dy, int h, int w, int Cin, int Cout, int S, float* dw, float* ws,
                                hipStream_t s);
// wf (Cin, Cout, 3, 3) with wf[c][o][tap] = w[o][c][8 - tap]: dx = conv3x3(dy, wf).  w: OIHW, or (packed) launch_pack_conv3x3's form
hipError_t launch_conv3x3_flip(const float* w, int Cout, int Cin, int packed, float* wf, hipStream_t s);

// ---- CNN gradients (cnn_grad.hip; docs/SEMANTICS.md, "CNN gradients") ----
// dy (n, H, W, C), every element written: dpool (n, ceil(H/2), ceil(W/2), C) routed to the first maximum of each clipped 2x2
// window of y (n, H, W, C) where that maximum is > 0, +0.0 elsewhere.  C % 4 == 0; 16-byte aligned pointers.
hipError_t launch_maxpool2x2_ceil_relu_grad(const float* y, const float* dpool, float* dy, int nimg, int H, int W, int C,
                                            hipStream_t s);
// dy[i] = y[i] > 0 ? dy[i] : +0.0 in place, n floats; any 4-byte alignment (16-byte accesses where both pointers allow them)
hipError_t launch_relu_mask(float* dy, const float* y, size_t n, hipStream_t s);

// ---- Dropout of the training forward (dropout.hip; docs/SEMANTICS.md, "Dropout") ----
// T = floor((1 - p) 2^32) in double (2^32 where 1 - p rounds to 1); s = 1 / (1 - p) in fp32
unsigned long long dropout_threshold(float p);
float dropout_scale(float p);
// In place on x (rows, cols), row stride ld >= cols floats: element (row, col) is kept, as x * s, iff word col & 3 of
// philox4x32_10(col >> 2, row, layer, 1, seed) < T, and is +0.0 otherwise.  0 < p < 1, layer in 0..255; any 4-byte alignment
// (16-byte accesses where x is 16-byte aligned and ld % 4 == 0).
hipError_t launch_dropout_rows(float* x, int rows, int cols, size_t ld, int layer, float p, uint64_t seed, hipStream_t s);
// dy[i] = y[i] > 0 ? dy[i] * s : +0.0 in place, n floats, y the dropped activation; 0 < p < 1; alignment as launch_relu_mask
hipError_t launch_relu_dropout_mask(float* dy, const float* y, size_t n, float p, hipStream_t s);

// ---- RPN gradients (rpn_grad.hip; docs/SEMANTICS.md, "RPN gradients") ----
// The gradient at the RPN's head outputs, dheads (h * w, 6k) in the layout of the heads: the two mid criteria on the sampled rows,
// ApplyBoxTransform:backward of droi (n, 4) or null, scattered by the sampler's copy rule (the last sampled row that names an
// input row wins), plus decay * trans on every box element.  trans, anchors, boxes (A, 4) and scores (A, 2) are the training
// forward's rows, A = k * h * w; win_all / win_pos: A int32 each of scratch.  n = num_pos + num_neg <= 1024; the lists are trusted.
struct RpnDheadsArgs {
  const float *trans, *scores, *anchors, *boxes, *gt, *droi;
  const int32_t *pos_input_idx, *pos_target_idx, *neg_input_idx;
  int num_pos, num_neg, h, w, k;
  float w_mid_obj, w_mid_box, decay;
  int32_t *win_all, *win_pos;
  float* dheads;
};
hipError_t launch_rpn_dheads(const RpnDheadsArgs& a, hipStream_t s);
// dhidden (P, R) = (hidden > 0) * (dheads (P, K6) . W (K6, R)), fp32 in ascending K6 order; K6 <= 12288
hipError_t launch_rpn_heads_bwd(const float* dheads, const float* W, const float* hidden, int P, int K6, int R, float* dhidden,
                                hipStream_t s);

// ---- the optimiser (optim.hip; docs/SEMANTICS.md, "Training step") ----
// One segment of an Adam launch: p, m, v (n floats each) are updated in place from g; chunk0 = adam_chunks of the segments in
// front of it.  The table on the device holds nseg + 1 entries: the last one carries the total in chunk0 and nothing else.
struct AdamSeg {
  float* p; const float* g; float* m; float* v;
  size_t n;
  unsigned long long chunk0;
};
// The step's scalars, each computed in double on the host and rounded to float once: b1 = beta1, c1 = 1 - beta1, b2 = beta2,
// c2 = 1 - beta2, eps, wd = weight_decay, nstep = -(lr * sqrt(1 - beta2^t) / (1 - beta1^t))
struct AdamScalars { float b1, c1, b2, c2, eps, wd, nstep; };
unsigned long long adam_chunks(size_t n);
// grid_or_0: 0 = the production grid (min(chunks, 2048) workgroups); > 0: that many (a test hook: the result does not depend on it)
hipError_t launch_adam_multi(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, const AdamScalars& k, int grid_or_0,
                             hipStream_t s);
// ---- the global gradient norm (docs/SEMANTICS.md, "Gradient clipping") ----
// What grad_norm_finish_kernel leaves on the device: the sum of squares, its root, and the factor the scaled Adam launch reads
struct GradNormRec { double sumsq, norm; float scale, pad_; };
// partial[c] = the sum of squares of chunk c of the table's gradients (one double per chunk of the launch_adam_multi list,
// `chunks` of them, whatever the grid); only the g pointers and n of the table are read
hipError_t launch_grad_sumsq(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, double* partial, int grid_or_0,
                             hipStream_t s);
// One workgroup: the `total` partials (of one table, or of two laid end to end) in a fixed order -> *rec.  max_norm >= 0 or +inf;
// 0 reports the norm and leaves scale = 1
hipError_t launch_grad_norm_finish(const double* partial, unsigned long long total, double max_norm, GradNormRec* rec, hipStream_t s);
// launch_adam_multi with every gradient element multiplied by *scale_dev (a device float, read by the kernel) first
hipError_t launch_adam_multi_scaled(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, const AdamScalars& k,
                                    const float* scale_dev, int grid_or_0, hipStream_t s);
// The decode screen's operands from W (V1, Hd) fp32: wb (V1pad, Kp) bf16 bits, zero padded; wn (V1pad) the rows' 2-norms rounded
// up to fp16, zero past V1
hipError_t launch_screen_operands(const float* W, int V1, int Hd, int V1pad, int Kp, uint16_t* wb, uint16_t* wn, hipStream_t s);
// launch_pack_conv3x3's inverse: (Cout, 9 Cin) with k = tap * Cin + c -> OIHW
hipError_t launch_unpack_conv3x3(const float* packed, float* oihw, int Cout, int Cin, hipStream_t s);

// ---- image preprocessing (preprocess.hip; run_model.lua:67-74) -------------------------------------------------------
void preprocess_scaled_size(int H0, int W0, int image_size, int* oh, int* ow);
size_t preprocess_scratch_bytes(int H0, int W0, int oh, int ow);     // the width pass's double plane
size_t preprocess_taps_bytes(int oh, int ow);                        // the tap tables of a (H0, W0) -> (oh, ow) scaling ...
void preprocess_make_taps(int H0, int W0, int oh, int ow, void* host_out);   // ... built on the host (they depend on the sizes only)
hipError_t launch_preprocess_u8(const uint8_t* src_dev, int H0, int W0, int oh, int ow, const float mean_bgr[3],
                                void* scratch, const void* taps_dev, float* out_chw, uint8_t* rgb_hwc, hipStream_t s);
