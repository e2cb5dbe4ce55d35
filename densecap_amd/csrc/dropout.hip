// Dropout of the recognition net's training forward and its backward (docs/SEMANTICS.md, "Dropout"): the two nn.Dropout layers of
// recog_base, after fc6's ReLU and after fc7's.  The mask is counter-based: element (row, col) of layer l is kept iff word col & 3
// of philox4x32_10(col >> 2, row, l, 1, seed) is below T = floor((1 - p) 2^32), a pure function of its coordinates.  Applied in
// place, so the activation itself carries the mask into the backward (y > 0 iff ReLU-alive and kept): nothing is stored and
// nothing is drawn twice.  No atomics, every element written once.
#include "common.h"

namespace {

// ---- nn.Dropout forward, in place on x (rows, cols) with row stride ld ------------------------------------------------------------
// One thread owns one run of four columns (col >> 2 = g) of one row and draws one Philox block for it.  vec: x is 16-byte aligned
// and ld % 4 == 0, so a whole run is one 16-byte access; the run that crosses cols (cols % 4 != 0) and every run of a misaligned
// matrix go float by float.  A kept element is x * s in one fp32 multiply; a dropped one is +0.0 whatever x was.
__global__ __launch_bounds__(256) void dropout_rows_kernel(float* __restrict__ x, int rows, int cols, size_t ld, uint32_t layer,
                                                           unsigned long long T, float s, uint32_t k0, uint32_t k1, int vec) {
  const size_t c4 = ((size_t)cols + 3) / 4, total = (size_t)rows * c4;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t row = i / c4;
  const uint32_t g = (uint32_t)(i - row * c4);
  const Philox4 z = philox4x32_10(g, (uint32_t)row, layer, 1u, k0, k1);
  float* const p = x + row * ld + (size_t)g * 4;
  const int left = cols - (int)(g * 4u);               // columns of this run inside the matrix: 1..4 in the last run, 4 elsewhere
  if (vec && left >= 4) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (unsigned long long)z.w[e] < T ? v[e] * s : 0.f;
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < left) p[e] = (unsigned long long)z.w[e] < T ? p[e] * s : 0.f;
  }
}

// ---- nn.ReLU(true) followed by nn.Dropout, backward, in place: dy[i] = y[i] > 0 ? dy[i] * s : +0.0 ---------------------------------
// y is the dropped activation.  relu_mask_kernel's access pattern (cnn_grad.hip): n4 vectors of four floats (both pointers
// 16-byte aligned), then the n - 4 * n4 floats behind them one by one
__global__ __launch_bounds__(256) void relu_dropout_mask_kernel(const float* __restrict__ y, float* __restrict__ dy, size_t n4, size_t n,
                                                                float s) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n4; i += stride) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + i * 4);
    f32x4 d = *reinterpret_cast<const f32x4*>(dy + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = a[e] > 0.f ? d[e] * s : 0.f;
    *reinterpret_cast<f32x4*>(dy + i * 4) = d;
  }
  for (size_t i = n4 * 4 + t0; i < n; i += stride) dy[i] = y[i] > 0.f ? dy[i] * s : 0.f;
}

inline int grid_of(size_t total, int cap) {
  const size_t b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : b > (size_t)cap ? (size_t)cap : b);
}

}  // namespace

unsigned long long dropout_threshold(float p) { return (unsigned long long)floor((1.0 - (double)p) * 4294967296.0); }
float dropout_scale(float p) { return 1.0f / (1.0f - p); }

hipError_t launch_dropout_rows(float* x, int rows, int cols, size_t ld, int layer, float p, uint64_t seed, hipStream_t s) {
  if (rows < 1 || cols < 1 || ld < (size_t)cols || layer < 0 || layer > 255 || !(p > 0.f && p < 1.f)) return hipErrorInvalidValue;
  const size_t blocks = ((size_t)rows * (((size_t)cols + 3) / 4) + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const int vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld % 4 == 0;
  hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, cols, ld, (uint32_t)layer, dropout_threshold(p),
                     dropout_scale(p), (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), vec);
  return hipGetLastError();
}

hipError_t launch_relu_dropout_mask(float* dy, const float* y, size_t n, float p, hipStream_t s) {
  if (n < 1 || !(p > 0.f && p < 1.f)) return hipErrorInvalidValue;
  const bool aligned = ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  hipLaunchKernelGGL(relu_dropout_mask_kernel, dim3(grid_of(aligned ? n4 + 3 : n, 256 * 16)), dim3(256), 0, s, y, dy, n4, n, dropout_scale(p));
  return hipGetLastError();
}
