// Kernels of the RPN's backward pass (densecap.hip::rpn_backward; docs/SEMANTICS.md, "RPN gradients") and of the brick it and a
// CNN's backward are built from, the backward of a 3x3 / stride 1 / pad 1 convolution on an HWC map (densecap.hip::conv3x3_grad;
// "Convolution gradients").
// Everything here is fp32 with fixed summation orders and no atomics: two identical calls give identical bits.
#include "common.h"

#include <algorithm>

namespace {

// ---- weight gradient: dW(Cout, 9*Cin) = sum_p dY(p, Cout) * im2col(X)(p, 9*Cin) on v_mfma_f32_32x32x2_f32 ---------------------
// The sibling of lm_grad.hip's wgrad_kernel: the summed index is the pixel p = y * w + x, the ROW of both operands, so both are
// staged in LDS row-major, kCwBM pixels at a time, and nothing is transposed.  dY is read as it lies in memory.  The second
// operand is never materialised: column k = tap * Cin + c of pixel p is X[(y + tap / 3 - 1, x + tap % 3 - 1)][c], zero outside
// the map, fetched from the HWC map itself.  A thread stages the same column in every round (256 threads = 2 rows of 128
// columns), so its tap and channel are found once; 128 neighbouring threads read 128 consecutive floats of one pixel, or of two
// taps' pixels where a tile straddles taps (Cin % 128 != 0; Cin % 32 == 0 keeps a 32-column group inside one tap).
// One workgroup (4 waves) owns a 128 x 128 tile of dW, each wave a 64 x 64 quarter as 2 x 2 MFMA tiles.  gridDim.z = S slices
// share the pixels: slice z sums pixels [z * rows_per, (z + 1) * rows_per) and writes its raw tile to part[(z * N + n) * K + k];
// conv3x3_wgrad_finish_kernel adds the slices in the order z = 0 .. S-1 and writes the checkpoint layout (Cout, Cin, 3, 3).
constexpr int kCwTile = 128;      // tile edge in both output dimensions
constexpr int kCwBM = 16;         // pixels staged per round
constexpr int kCwLd = kCwTile + 32;   // LDS row stride: rows m and m + 1 (the two halves of a wave) fall into different bank halves
constexpr int kCwPerThread = kCwBM * kCwTile / 256;   // floats of one operand a thread stages per round

__device__ __forceinline__ void cw_fetch_dy(const float* __restrict__ dY, int Cout, int m0, int m_end, int n, bool n_ok, int tid,
                                            float (&r)[kCwPerThread]) {
#pragma unroll
  for (int u = 0; u < kCwPerThread; ++u) {
    const int row = m0 + (tid >> 7) + 2 * u;
    r[u] = (n_ok && row < m_end) ? dY[(size_t)row * Cout + n] : 0.f;
  }
}
// the thread's column of the im2col operand: channel c of the pixel (dyo, dxo) away, for the rows m0 + (tid >> 7) + 2u
__device__ __forceinline__ void cw_fetch_x(const float* __restrict__ X, int h, int w, int Cin, int m0, int m_end, int dyo, int dxo,
                                           int c, bool k_ok, int tid, float (&r)[kCwPerThread]) {
#pragma unroll
  for (int u = 0; u < kCwPerThread; ++u) {
    const int row = m0 + (tid >> 7) + 2 * u;
    float v = 0.f;
    if (k_ok && row < m_end) {
      const int y = row / w, x = row - y * w;
      const int yy = y + dyo, xx = x + dxo;
      if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = X[((size_t)yy * w + xx) * Cin + c];
    }
    r[u] = v;
  }
}
__device__ __forceinline__ void cw_stage(float* __restrict__ sh, int tid, const float (&r)[kCwPerThread]) {
#pragma unroll
  for (int u = 0; u < kCwPerThread; ++u) sh[((tid >> 7) + 2 * u) * kCwLd + (tid & (kCwTile - 1))] = r[u];
}

__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ dY, int h, int w,
                                                            int Cin, int Cout, int rows_per, float* __restrict__ part) {
  __shared__ float shA[kCwBM * kCwLd];
  __shared__ float shB[kCwBM * kCwLd];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int M = h * w, N = Cout, K = 9 * Cin;
  const int n0 = blockIdx.y * kCwTile, k0 = blockIdx.x * kCwTile;
  const int m_begin = blockIdx.z * rows_per, m_end = min(M, m_begin + rows_per);
  const int wn = (wid >> 1) * 64, wk = (wid & 1) * 64;
  const int lr = lane >> 5, lc = lane & 31;
  // what this thread stages: column n of dY, column k = tap * Cin + c of the im2col operand
  const int sn = n0 + (tid & (kCwTile - 1)), sk = k0 + (tid & (kCwTile - 1));
  const bool n_ok = sn < N, k_ok = sk < K;
  const int tap = k_ok ? sk / Cin : 0, sc = k_ok ? sk - tap * Cin : 0;
  const int dyo = tap / 3 - 1, dxo = tap % 3 - 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  float ra[kCwPerThread], rb[kCwPerThread];
  cw_fetch_dy(dY, Cout, m_begin, m_end, sn, n_ok, tid, ra);
  cw_fetch_x(X, h, w, Cin, m_begin, m_end, dyo, dxo, sc, k_ok, tid, rb);
  for (int m0 = m_begin; m0 < m_end; m0 += kCwBM) {
    __syncthreads();                                   // the previous round's reads are done
    cw_stage(shA, tid, ra);
    cw_stage(shB, tid, rb);
    __syncthreads();
    if (m0 + kCwBM < m_end) {                          // the next round travels while this one is multiplied
      cw_fetch_dy(dY, Cout, m0 + kCwBM, m_end, sn, n_ok, tid, ra);
      cw_fetch_x(X, h, w, Cin, m0 + kCwBM, m_end, dyo, dxo, sc, k_ok, tid, rb);
    }
#pragma unroll
    for (int mm = 0; mm < kCwBM; mm += 2) {
      const float* pa = shA + (mm + lr) * kCwLd + wn + lc;
      const float* pb = shB + (mm + lr) * kCwLd + wk + lc;
      const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float* out = part + (size_t)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk + j * 32 + lc;
      if (k >= K) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = n0 + wn + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * lr;
        if (n < N) out[(size_t)n * K + k] = acc[i][j][q];
      }
    }
}

// dw[o][c][tap] = sum_z part[z][o][tap * Cin + c], z ascending: the slice sum and the inverse of pack_conv3x3_kernel in one pass
__global__ __launch_bounds__(256) void conv3x3_wgrad_finish_kernel(const float* __restrict__ part, int S, int Cout, int Cin,
                                                                   float* __restrict__ dw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, NK = (size_t)Cout * Cin * 9;
  if (i >= NK) return;
  float v = part[i];
  for (int z = 1; z < S; ++z) v += part[(size_t)z * NK + i];
  const int c = (int)(i % Cin);
  const size_t t = i / Cin;
  const int tap = (int)(t % 9);
  const size_t o = t / 9;
  dw[(o * Cin + c) * 9 + tap] = v;
}

// wf[c][o][tap] = w[o][c][8 - tap]: the weights of the convolution that takes dY to dX, OIHW (Cin, Cout, 3, 3).  w is OIHW
// (Cout, Cin, 3, 3), or with `packed` the engine's (Cout, 9 * Cin) with k = tap * Cin + c (what a context keeps of its own weights).
__global__ __launch_bounds__(256) void conv3x3_flip_kernel(const float* __restrict__ w, int Cout, int Cin, int packed,
                                                           float* __restrict__ wf) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)Cout * Cin * 9;
  if (i >= total) return;
  const int tap = (int)(i % 9);
  const size_t t = i / 9;
  const size_t o = t % Cout;
  const size_t c = t / Cout;
  wf[i] = packed ? w[(o * 9 + (8 - tap)) * Cin + c] : w[(o * Cin + c) * 9 + (8 - tap)];
}

// ---- the gradient at the RPN's head outputs (docs/SEMANTICS.md, "RPN gradients") ------------------------------------------------
// The sampler's backward is a COPY (BoxSamplerHelper.lua:166-177): the positive rows' gradients are copied to their input rows
// first, then the negative rows', each list in order, so of the sampled rows that name one input row the last one wins -- a
// negative beats a positive, the largest r among equals.  Row r (positives first) is the last writer of its input row for the
// boxes and the scores when no row after it names the same input; for the transforms, which only positives carry, when no
// positive after it does.  One workgroup, n <= 1024 rows; the winners are unique, so the two tables do not depend on store order.
__global__ __launch_bounds__(1024) void rpn_winner_kernel(const int32_t* __restrict__ pos_input_idx,
                                                          const int32_t* __restrict__ neg_input_idx, int np, int nn,
                                                          int32_t* __restrict__ win_all, int32_t* __restrict__ win_pos) {
  __shared__ int32_t idx[1024];
  const int r = threadIdx.x, n = np + nn;
  if (r < n) idx[r] = r < np ? pos_input_idx[r] : neg_input_idx[r - np];
  __syncthreads();
  if (r >= n) return;
  const int i = idx[r];
  bool last_all = true, last_pos = r < np;
  for (int q = r + 1; q < n; ++q)
    if (idx[q] == i) {
      last_all = false;
      if (q < np) last_pos = false;
    }
  if (last_all) win_all[i] = r;
  if (last_pos) win_pos[i] = r;
}

// One thread per RPN row b = a * h * w + y * w + x writes the row's six elements of dheads (h * w, 6k): box channels a * 4 + d,
// score channels 4k + a * 2 + d (the layout rpn_decode_kernel and rpn_score_rows_kernel read).  Per-row terms in double on the
// fp32 inputs, cast once:
//   scores: w_mid_obj * (softmax(s) - e_c) / count of the winning row, c = 0 and count = num_pos for a positive, c = 1 and
//           count = num_neg for a negative, softmax in loss_terms' form exp(s - max) / sum; no winner: +0.0
//   mid   : w_mid_box * clamp(trans - target, -1, 1) / (4 num_pos) of the winning POSITIVE row, target = InvertBoxTransform(anchor,
//           gt[pos_target_idx[r]]) as lt_box_row forms it; zero for a row whose largest |target| exceeds 10
//   abt   : ApplyBoxTransform:backward of the winning row's droi: (g_x * wa, g_y * ha, g_w * box_w, g_h * box_h)
// and every box element is decay * trans + (abt + mid) in fp32 (RegularizeLayer.lua:18-22).
__global__ __launch_bounds__(256) void rpn_dheads_kernel(RpnDheadsArgs a) {
  const int hw = a.h * a.w, A = a.k * hw;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= A) return;
  const int an = b / hw, cell = b - an * hw;
  const int ra = a.win_all[b], rp = a.win_pos[b], np = a.num_pos;
  const float* t = a.trans + (size_t)b * 4;
  float mid[4] = {0.f, 0.f, 0.f, 0.f}, abt[4] = {0.f, 0.f, 0.f, 0.f}, ds[2] = {0.f, 0.f};
  if (rp >= 0) {
    const float* anc = a.anchors + (size_t)b * 4;
    const float* tg = a.gt + (size_t)a.pos_target_idx[rp] * 4;
    const double xa = anc[0], ya = anc[1], wa = anc[2], ha = anc[3];
    const double xt = tg[0], yt = tg[1], wt = tg[2], ht = tg[3];
    double tt[4];
    tt[0] = (xt - xa) / wa; tt[1] = (yt - ya) / ha; tt[2] = log(wt / wa); tt[3] = log(ht / ha);
    double mx = fabs(tt[0]);
    for (int d = 1; d < 4; ++d) { const double v = fabs(tt[d]); if (v > mx) mx = v; }
    if (!(mx > 10.0)) {
      for (int d = 0; d < 4; ++d) {
        double z = (double)t[d] - tt[d];
        z = z < -1.0 ? -1.0 : (z > 1.0 ? 1.0 : z);
        mid[d] = (float)((double)a.w_mid_box * z / (4.0 * (double)np));
      }
    }
  }
  if (ra >= 0) {
    if (a.droi != nullptr) {
      const float* g = a.droi + (size_t)ra * 4;
      const float* anc = a.anchors + (size_t)b * 4;
      const float* bx = a.boxes + (size_t)b * 4;
      abt[0] = __fmul_rn(g[0], anc[2]); abt[1] = __fmul_rn(g[1], anc[3]);
      abt[2] = __fmul_rn(g[2], bx[2]);  abt[3] = __fmul_rn(g[3], bx[3]);
    }
    const int c = ra < np ? 0 : 1;
    const double cnt = c == 0 ? (double)np : (double)a.num_neg;
    const double s0 = (double)a.scores[(size_t)b * 2], s1 = (double)a.scores[(size_t)b * 2 + 1], m = s1 > s0 ? s1 : s0;
    const double e0 = exp(s0 - m), e1 = exp(s1 - m), sum = e0 + e1;
    ds[0] = (float)((double)a.w_mid_obj * (e0 / sum - (c == 0 ? 1.0 : 0.0)) / cnt);
    ds[1] = (float)((double)a.w_mid_obj * (e1 / sum - (c == 1 ? 1.0 : 0.0)) / cnt);
  }
  float* row = a.dheads + (size_t)cell * 6 * a.k;
#pragma unroll
  for (int d = 0; d < 4; ++d) row[an * 4 + d] = __fadd_rn(__fmul_rn(a.decay, t[d]), __fadd_rn(abt[d], mid[d]));
  row[4 * a.k + an * 2] = ds[0];
  row[4 * a.k + an * 2 + 1] = ds[1];
}

// ---- the two 1x1 heads' data gradient with the in-place ReLU's mask ----------------------------------------------------------------
// dhidden[p][j] = hidden[p][j] > 0 ? sum_c dheads[p][c] * W[c][j] : +0.0, one workgroup per pixel, the row of dheads in LDS,
// c ascending on one fmaf chain.  K6 = 6k is tens of columns: a row kernel, not the engine.
__global__ __launch_bounds__(256) void rpn_heads_bwd_kernel(const float* __restrict__ dheads, const float* __restrict__ W,
                                                            const float* __restrict__ hidden, int K6, int R,
                                                            float* __restrict__ dhidden) {
  extern __shared__ float row[];
  const size_t p = blockIdx.x;
  for (int c = threadIdx.x; c < K6; c += 256) row[c] = dheads[p * K6 + c];
  __syncthreads();
  for (int j = threadIdx.x; j < R; j += 256) {
    float v = 0.f;
    for (int c = 0; c < K6; ++c) v = __fmaf_rn(row[c], W[(size_t)c * R + j], v);
    dhidden[p * R + j] = hidden[p * R + j] > 0.f ? v : 0.f;
  }
}

}  // namespace

int conv3x3_wgrad_slices(int P, int Cout, int Cin) { return wgrad_slices(P, Cout, 9 * Cin); }
size_t conv3x3_wgrad_ws_floats(int S, int Cout, int Cin) { return (size_t)S * Cout * Cin * 9; }
hipError_t launch_conv3x3_wgrad(const float* x, const float* dy, int h, int w, int Cin, int Cout, int S, float* dw, float* ws,
                                hipStream_t s) {
  if (h < 1 || w < 1 || Cin < 32 || Cin % 32 || Cout < 1 || S < 1 || S > 64 || (size_t)h * w > 65536 || ws == nullptr)
    return hipErrorInvalidValue;
  const int M = h * w, K = 9 * Cin;
  int rows_per = (M + S - 1) / S;
  rows_per = (rows_per + kCwBM - 1) / kCwBM * kCwBM;
  const dim3 grid((K + kCwTile - 1) / kCwTile, (Cout + kCwTile - 1) / kCwTile, S);
  hipLaunchKernelGGL(conv3x3_wgrad_kernel, grid, dim3(256), 0, s, x, dy, h, w, Cin, Cout, rows_per, ws);
  const size_t NK = (size_t)Cout * K;
  hipLaunchKernelGGL(conv3x3_wgrad_finish_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, s, ws, S, Cout, Cin, dw);
  return hipGetLastError();
}
hipError_t launch_conv3x3_flip(const float* w, int Cout, int Cin, int packed, float* wf, hipStream_t s) {
  const size_t total = (size_t)Cout * Cin * 9;
  hipLaunchKernelGGL(conv3x3_flip_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, Cout, Cin, packed, wf);
  return hipGetLastError();
}
hipError_t launch_rpn_dheads(const RpnDheadsArgs& a, hipStream_t s) {
  const int n = a.num_pos + a.num_neg;
  const long long A = (long long)a.k * a.h * a.w;
  if (a.num_pos < 0 || a.num_neg < 0 || n > 1024 || a.k < 1 || a.h < 1 || a.w < 1 || A > (1ll << 30)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.win_all, 0xff, (size_t)A * 4, s);            // -1: no sampled row names the input row
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.win_pos, 0xff, (size_t)A * 4, s);
  if (e != hipSuccess) return e;
  if (n > 0)
    hipLaunchKernelGGL(rpn_winner_kernel, dim3(1), dim3(1024), 0, s, a.pos_input_idx, a.neg_input_idx, a.num_pos, a.num_neg, a.win_all,
                       a.win_pos);
  hipLaunchKernelGGL(rpn_dheads_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_rpn_heads_bwd(const float* dheads, const float* W, const float* hidden, int P, int K6, int R, float* dhidden,
                                hipStream_t s) {
  if (P < 1 || K6 < 1 || R < 1 || (size_t)K6 * 4 > 48 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rpn_heads_bwd_kernel, dim3(P), dim3(256), (size_t)K6 * 4, s, dheads, W, hidden, K6, R, dhidden);
  return hipGetLastError();
}
