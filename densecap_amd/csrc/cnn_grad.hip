// Point-wise kernels of the CNN's backward pass (densecap.hip::cnn_backward; docs/SEMANTICS.md, "CNN gradients"): the backward of
// the ceil-mode 2x2 / stride 2 max pool fused with the mask of the in-place ReLU in front of it, and that mask alone for the
// convolutions no pool follows (the fully connected layers' ReLUs in lm_grad and recog_backward take the same kernel).  Both are
// selections: no arithmetic, no atomics, every output element written once.
#include "common.h"

namespace {

// ---- nn.SpatialMaxPooling(2,2,2,2):ceil() backward + nn.ReLU(true) backward, HWC ------------------------------------------------
// y (n, H, W, C): the map the pool read, that is the ReLU's output; dpool (n, ceil(H/2), ceil(W/2), C).  One thread owns a window
// of four channels (the windows do not overlap): the window is clipped at the map's edge, the gradient goes to the FIRST maximum
// in scan order (row, then column; `>` is strict, as THNN's SpatialMaxPooling_updateOutput keeps its index) and only where that
// value is > 0 (the ReLU's mask by its output); every other element of the window gets +0.0.  A select, not a product: a NaN in
// dpool lands where the rule puts it and nowhere else.
__global__ __launch_bounds__(256) void maxpool2x2_ceil_relu_grad_kernel(const float* __restrict__ y, const float* __restrict__ dpool,
                                                                        float* __restrict__ dy, int nimg, int H, int W, int C) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, C4 = C / 4;
  const size_t total = (size_t)nimg * Ho * Wo * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    size_t t = i / C4;
    const int xo = (int)(t % Wo); t /= Wo;
    const int yo = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const int y0 = 2 * yo, x0 = 2 * xo;
    const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
    const size_t img = ((size_t)n * H * W) * C + (size_t)c4 * 4;
    const size_t o00 = img + ((size_t)y0 * W + x0) * C, o01 = o00 + C, o10 = o00 + (size_t)W * C, o11 = o10 + C;
    const f32x4 g = *reinterpret_cast<const f32x4*>(dpool + i * 4);
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(y + o00);
    f32x4 v01 = v00, v10 = v00, v11 = v00;                       // (a clipped position never beats the first: `>` is strict)
    if (hx) v01 = *reinterpret_cast<const f32x4*>(y + o01);
    if (hy) v10 = *reinterpret_cast<const f32x4*>(y + o10);
    if (hx && hy) v11 = *reinterpret_cast<const f32x4*>(y + o11);
    f32x4 d00, d01, d10, d11;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float best = v00[e];
      int pos = 0;
      if (v01[e] > best) { best = v01[e]; pos = 1; }
      if (v10[e] > best) { best = v10[e]; pos = 2; }
      if (v11[e] > best) { best = v11[e]; pos = 3; }
      const bool live = best > 0.f;
      d00[e] = live && pos == 0 ? g[e] : 0.f;
      d01[e] = live && pos == 1 ? g[e] : 0.f;
      d10[e] = live && pos == 2 ? g[e] : 0.f;
      d11[e] = live && pos == 3 ? g[e] : 0.f;
    }
    *reinterpret_cast<f32x4*>(dy + o00) = d00;
    if (hx) *reinterpret_cast<f32x4*>(dy + o01) = d01;
    if (hy) *reinterpret_cast<f32x4*>(dy + o10) = d10;
    if (hx && hy) *reinterpret_cast<f32x4*>(dy + o11) = d11;
  }
}

// ---- nn.ReLU(true) backward, in place: dy[i] = y[i] > 0 ? dy[i] : +0.0 ------------------------------------------------------------
// n4 vectors of four floats (both pointers 16-byte aligned), then the n - 4 * n4 floats behind them one by one
__global__ __launch_bounds__(256) void relu_mask_kernel(const float* __restrict__ y, float* __restrict__ dy, size_t n4, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < n4; i += stride) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + i * 4);
    f32x4 d = *reinterpret_cast<const f32x4*>(dy + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = a[e] > 0.f ? d[e] : 0.f;
    *reinterpret_cast<f32x4*>(dy + i * 4) = d;
  }
  for (size_t i = n4 * 4 + t0; i < n; i += stride) dy[i] = y[i] > 0.f ? dy[i] : 0.f;
}

inline int grid_of(size_t total, int cap) {
  const size_t b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : b > (size_t)cap ? (size_t)cap : b);
}

}  // namespace

hipError_t launch_maxpool2x2_ceil_relu_grad(const float* y, const float* dpool, float* dy, int nimg, int H, int W, int C,
                                            hipStream_t s) {
  if (nimg < 1 || H < 1 || W < 1 || C < 4 || C % 4) return hipErrorInvalidValue;
  const size_t total = (size_t)nimg * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_ceil_relu_grad_kernel, dim3(grid_of(total, 256 * 16)), dim3(256), 0, s, y, dpool, dy, nimg, H, W, C);
  return hipGetLastError();
}

hipError_t launch_relu_mask(float* dy, const float* y, size_t n, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  const bool aligned = ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_of(aligned ? n4 + 3 : n, 256 * 16)), dim3(256), 0, s, y, dy, n4, n);
  return hipGetLastError();
}
