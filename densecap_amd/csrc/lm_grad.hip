// Kernels of the language model's backward pass (densecap.hip::lm_grad; docs/SEMANTICS.md, "Language-model gradients").
// Everything here is fp32 with fixed summation orders and no atomics: two identical calls give identical bits.
#include "common.h"

#include <algorithm>

namespace {

// ---- weight gradient: C(N,K) = sum_m A(m,N) * B(m,K) on v_mfma_f32_32x32x2_f32 -----------------------------------------------
// The summed index is the ROW of both operands, so the MFMA's inner index walks rows: lane l of a wave feeds A[m + (l>>5)][n + (l&31)]
// and B[m + (l>>5)][k + (l&31)] -- 32 neighbouring lanes read 32 consecutive floats of one row.  Both operands are therefore staged
// in LDS row-major, exactly as they lie in memory, kWgBM rows at a time; nothing is transposed anywhere.
// One workgroup (4 waves) owns a 128 x 128 tile of C, each wave a 64 x 64 quarter as 2 x 2 MFMA tiles (64 accumulator registers).
// gridDim.z = S slices share the rows: slice z sums rows [z * rows_per, (z + 1) * rows_per) and, with S > 1, writes its raw tile
// to part[(z * N + n) * K + k]; wgrad_reduce_kernel adds the slices in the order z = 0 .. S-1.
constexpr int kWgTile = 128;      // tile edge in both output dimensions
constexpr int kWgBM = 16;         // rows of A and B staged per round
constexpr int kWgLd = kWgTile + 32;   // LDS row stride: rows m and m + 1 (the two halves of a wave) fall into different bank halves
constexpr int kWgPerThread = kWgBM * kWgTile / 256;   // floats of one operand a thread stages per round

__device__ __forceinline__ void wgrad_fetch(const float* __restrict__ X, int ldx, int m0, int m_end, int c0, int C, int tid,
                                            float (&r)[kWgPerThread]) {
#pragma unroll
  for (int u = 0; u < kWgPerThread; ++u) {
    const int idx = tid + u * 256, row = m0 + (idx >> 7), col = c0 + (idx & (kWgTile - 1));
    r[u] = (row < m_end && col < C) ? X[(size_t)row * ldx + col] : 0.f;
  }
}
__device__ __forceinline__ void wgrad_stage(float* __restrict__ sh, int tid, const float (&r)[kWgPerThread]) {
#pragma unroll
  for (int u = 0; u < kWgPerThread; ++u) {
    const int idx = tid + u * 256;
    sh[(idx >> 7) * kWgLd + (idx & (kWgTile - 1))] = r[u];
  }
}

__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                    int M, int N, int K, int rows_per, float* __restrict__ C, int ldc,
                                                    float* __restrict__ part) {
  __shared__ float shA[kWgBM * kWgLd];
  __shared__ float shB[kWgBM * kWgLd];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.y * kWgTile, k0 = blockIdx.x * kWgTile;
  const int m_begin = blockIdx.z * rows_per, m_end = min(M, m_begin + rows_per);
  const int wn = (wid >> 1) * 64, wk = (wid & 1) * 64;
  const int lr = lane >> 5, lc = lane & 31;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  float ra[kWgPerThread], rb[kWgPerThread];
  wgrad_fetch(A, lda, m_begin, m_end, n0, N, tid, ra);
  wgrad_fetch(B, ldb, m_begin, m_end, k0, K, tid, rb);
  for (int m0 = m_begin; m0 < m_end; m0 += kWgBM) {
    __syncthreads();                                   // the previous round's reads are done
    wgrad_stage(shA, tid, ra);
    wgrad_stage(shB, tid, rb);
    __syncthreads();
    if (m0 + kWgBM < m_end) {                          // the next round travels while this one is multiplied
      wgrad_fetch(A, lda, m0 + kWgBM, m_end, n0, N, tid, ra);
      wgrad_fetch(B, ldb, m0 + kWgBM, m_end, k0, K, tid, rb);
    }
#pragma unroll
    for (int mm = 0; mm < kWgBM; mm += 2) {
      const float* pa = shA + (mm + lr) * kWgLd + wn + lc;
      const float* pb = shB + (mm + lr) * kWgLd + wk + lc;
      const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float* out = part != nullptr ? part + (size_t)blockIdx.z * N * K : C;
  const int ldo = part != nullptr ? K : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk + j * 32 + lc;
      if (k >= K) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = n0 + wn + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * lr;
        if (n < N) out[(size_t)n * ldo + k] = acc[i][j][q];
      }
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int S, int N, int K, float* __restrict__ C,
                                                           int ldc) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, NK = (size_t)N * K;
  if (i >= NK) return;
  float v = part[i];
  for (int z = 1; z < S; ++z) v += part[(size_t)z * NK + i];
  C[(i / K) * ldc + (i % K)] = v;
}

// ---- column sums (bias gradients): out[c] = sum_m X[m][c], a fixed tree ------------------------------------------------------
// A workgroup owns 32 columns; thread (g = tid >> 5, c = tid & 31) adds rows g, g + 8, ... in ascending order in double, the eight
// partial sums are then added in the order g = 0 .. 7.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int ldx, int M, int N, float* __restrict__ out) {
  __shared__ double sh[8][32];
  const int g = threadIdx.x >> 5, c = blockIdx.x * 32 + (threadIdx.x & 31);
  double v = 0.0;
  if (c < N)
    for (int m = g; m < M; m += 8) v += (double)X[(size_t)m * ldx + c];
  sh[g][threadIdx.x & 31] = v;
  __syncthreads();
  if (g == 0 && c < N) {
    double t = sh[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < 8; ++q) t += sh[q][threadIdx.x];
    out[c] = (float)t;
  }
}

// ---- softmax cross-entropy gradient, one workgroup per row of logits, in place ---------------------------------------------------
// lse = max + log(sum exp(v - max)) with TH's exp (double, cast to float) summed in double: per thread in ascending column order,
// the 64 lanes of a wave by a butterfly, the four waves in order.  x[c] = (exp(v[c] - lse) - [c == tgt - 1]) * scale, the
// exponential taken in double and cast; columns [V1, ld) are set to +0.0 (they are K padding of the products that follow).
__global__ __launch_bounds__(256) void softmax_grad_kernel(float* __restrict__ x, int ld, int V1, const int32_t* __restrict__ tgt,
                                                           float scale, double* __restrict__ lse_out) {
  __shared__ float smx[4];
  __shared__ double ssum[4];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float* row = x + (size_t)m * ld;
  float mx = -INFINITY;
  for (int c = tid; c < V1; c += 256) { const float v = row[c]; mx = v > mx ? v : mx; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float ov = __shfl_xor(mx, o, 64); mx = ov > mx ? ov : mx; }
  if (lane == 0) smx[wid] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  double sum = 0.0;
  for (int c = tid; c < V1; c += 256) sum += (double)th_expf(row[c] - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) ssum[wid] = sum;
  __syncthreads();
  const double lse = (double)mx + log(((ssum[0] + ssum[1]) + ssum[2]) + ssum[3]);
  if (tid == 0 && lse_out != nullptr) lse_out[m] = lse;
  const int t = tgt[m] - 1;
  for (int c = tid; c < ld; c += 256) {
    float g = 0.f;
    if (c < V1) {
      const float p = (float)exp((double)row[c] - lse);
      g = (p - (c == t ? 1.f : 0.f)) * scale;
    }
    row[c] = g;
  }
}

// ---- LSTM cell backward, one workgroup per row ---------------------------------------------------------------------------------
// The cell's activations are formed again from what the forward kept, exactly as tail_update forms them: pre-activation =
// xg[tok - 1] + gates_pre (tok == null or 0: gates_pre alone), i, f, o = sigmoid, g = tanh, and tanh(c) from the kept c.
// dh = dh_a + dh_b (either may be null); dc_t = dc_in + dh * o * (1 - tanh(c)^2); d(pre) in gate order i, f, o, g;
// dc_prev = dc_t * f.  c_prev == null: the cell started from c = 0.  dc_in and dc_prev may be the same buffer.
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ gates_pre, const int32_t* __restrict__ tok,
                                                            const float* __restrict__ xg, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c, const float* __restrict__ dh_a,
                                                            const float* __restrict__ dh_b, const float* dc_in,
                                                            float* __restrict__ dgates, float* dc_prev, int Hd) {
  const int m = blockIdx.x;
  const float* gp = gates_pre + (size_t)m * 4 * Hd;
  const int t = tok != nullptr ? tok[m] : 0;
  const float* x = t > 0 ? xg + (size_t)(t - 1) * 4 * Hd : nullptr;
  float* dg = dgates + (size_t)m * 4 * Hd;
  for (int j = threadIdx.x; j < Hd; j += 256) {
    float gi = gp[j], gf = gp[Hd + j], go = gp[2 * Hd + j], gg = gp[3 * Hd + j];
    if (x != nullptr) { gi = x[j] + gi; gf = x[Hd + j] + gf; go = x[2 * Hd + j] + go; gg = x[3 * Hd + j] + gg; }
    const float ig = th_sigmoidf(gi), fg = th_sigmoidf(gf), og = th_sigmoidf(go), gt = th_tanhf(gg);
    const size_t e = (size_t)m * Hd + j;
    const float cp = c_prev != nullptr ? c_prev[e] : 0.f;
    const float tc = th_tanhf(c[e]);
    const float dh = (dh_a != nullptr ? dh_a[e] : 0.f) + (dh_b != nullptr ? dh_b[e] : 0.f);
    const float dct = (dc_in != nullptr ? dc_in[e] : 0.f) + dh * og * (1.f - tc * tc);
    dg[j] = dct * gt * (ig * (1.f - ig));
    dg[Hd + j] = dct * cp * (fg * (1.f - fg));
    dg[2 * Hd + j] = dh * tc * (og * (1.f - og));
    dg[3 * Hd + j] = dct * ig * (1.f - gt * gt);
    dc_prev[e] = dct * fg;
  }
}

// out[r] = tok[r] > 0 ? emb[tok[r] - 1] : 0, rows of E floats (the inputs the token cells were fed)
__global__ __launch_bounds__(256) void embed_rows_kernel(const float* __restrict__ emb, const int32_t* __restrict__ tok, int E,
                                                         float* __restrict__ out) {
  const int r = blockIdx.x, t = tok[r];
  for (int j = threadIdx.x; j < E; j += 256) out[(size_t)r * E + j] = t > 0 ? emb[(size_t)(t - 1) * E + j] : 0.f;
}

// out[perm[i]] = src[i], rows of `width` floats
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ perm, int width,
                                                           float* __restrict__ out) {
  const int i = blockIdx.x;
  const size_t o = (size_t)perm[i] * width;
  for (int j = threadIdx.x; j < width; j += 256) out[o + j] = src[(size_t)i * width + j];
}

// ---- embedding gradient: one workgroup per distinct token --------------------------------------------------------------------
// rows[seg[t] .. seg[t + 1]) are the dx rows that token ids[t] was fed at, in the host's order; they are added in that order.
__global__ __launch_bounds__(256) void embed_segsum_kernel(const float* __restrict__ dx, int E, const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ seg, const int32_t* __restrict__ ids,
                                                           float* __restrict__ demb) {
  const int t = blockIdx.x, b = seg[t], e = seg[t + 1];
  float* out = demb + (size_t)(ids[t] - 1) * E;
  for (int j = threadIdx.x; j < E; j += 256) {
    float v = dx[(size_t)rows[b] * E + j];
    for (int i = b + 1; i < e; ++i) v += dx[(size_t)rows[i] * E + j];
    out[j] = v;
  }
}

}  // namespace

int wgrad_slices(int M, int N, int K) {
  const int tiles = ((N + kWgTile - 1) / kWgTile) * ((K + kWgTile - 1) / kWgTile);
  const int want = std::max(1, 2 * device_cu_count() / tiles);          // two workgroups per CU fill the chip
  const int most = std::max(1, (M + 63) / 64);                          // a slice sums at least 64 rows
  return std::min(std::min(want, most), 64);
}
size_t wgrad_ws_floats(int M, int N, int K) {
  const int S = wgrad_slices(M, N, K);
  return S > 1 ? (size_t)S * N * K : 0;
}
hipError_t launch_wgrad(const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc, float* ws,
                        hipStream_t s) {
  if (M < 1 || N < 1 || K < 1 || lda < N || ldb < K || ldc < K) return hipErrorInvalidValue;
  const int S = wgrad_slices(M, N, K);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  int rows_per = (M + S - 1) / S;
  rows_per = (rows_per + kWgBM - 1) / kWgBM * kWgBM;
  const dim3 grid((K + kWgTile - 1) / kWgTile, (N + kWgTile - 1) / kWgTile, S);
  hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, s, A, lda, B, ldb, M, N, K, rows_per, C, ldc, S > 1 ? ws : nullptr);
  if (S > 1) {
    const size_t NK = (size_t)N * K;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, s, ws, S, N, K, C, ldc);
  }
  return hipGetLastError();
}
hipError_t launch_colsum(const float* X, int ldx, int M, int N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 31) / 32), dim3(256), 0, s, X, ldx, M, N, out);
  return hipGetLastError();
}
hipError_t launch_softmax_grad(float* x, int ld, int V1, const int32_t* tgt, float scale, double* lse_out, int rows, hipStream_t s) {
  hipLaunchKernelGGL(softmax_grad_kernel, dim3(rows), dim3(256), 0, s, x, ld, V1, tgt, scale, lse_out);
  return hipGetLastError();
}
hipError_t launch_lstm_cell_bwd(const float* gates_pre, const int32_t* tok, const float* xg, const float* c_prev, const float* c,
                                const float* dh_a, const float* dh_b, const float* dc_in, float* dgates, float* dc_prev, int rows,
                                int Hd, hipStream_t s) {
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(rows), dim3(256), 0, s, gates_pre, tok, xg, c_prev, c, dh_a, dh_b, dc_in, dgates,
                     dc_prev, Hd);
  return hipGetLastError();
}
hipError_t launch_embed_rows(const float* emb, const int32_t* tok, int rows, int E, float* out, hipStream_t s) {
  hipLaunchKernelGGL(embed_rows_kernel, dim3(rows), dim3(256), 0, s, emb, tok, E, out);
  return hipGetLastError();
}
hipError_t launch_scatter_rows(const float* src, const int32_t* perm, int rows, int width, float* out, hipStream_t s) {
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(rows), dim3(256), 0, s, src, perm, width, out);
  return hipGetLastError();
}
hipError_t launch_embed_segsum(const float* dx, int E, const int32_t* rows, const int32_t* seg, const int32_t* ids, int ntok,
                               float* demb, hipStream_t s) {
  hipLaunchKernelGGL(embed_segsum_kernel, dim3(ntok), dim3(256), 0, s, dx, E, rows, seg, ids, demb);
  return hipGetLastError();
}
