// Backward of bilinear RoI pooling (docs/SEMANTICS.md, "Recognition-net gradients"; nn.BilinearRoiPooling:backward,
// LocalizationLayer.lua:574-582).  fp32 data, fixed summation orders, no float atomics: two identical calls give identical bits.
//
// The gradient of the feature map is a scatter: tap t = (row * P + point) * 4 + k (k = tl, tr, bl, br) adds
// weight_t * dpool[row][point][:] to one pixel.  It is computed as "store once, sum per destination", and the contribution rows
// are the dpool rows themselves, so nothing is stored twice:
//   roi_taps_kernel       one workgroup per row: every tap's pixel (or -1) and weight, from the forward's own position helper,
//                         and an INTEGER-atomic histogram of taps per pixel
//   roi_index_scan_kernel one workgroup: the pixels' list offsets, their chunk counts and the (pixel, chunk) work items
//   roi_place_kernel      one thread per tap: a slot of its pixel's list from an integer cursor (any order) ...
//   roi_sort_lists_kernel ... one workgroup per pixel puts the list in ascending tap id (bitonic; LDS, or in place for a long list)
//   roi_scatter_sum_kernel one workgroup per (pixel, chunk of kRoiChunk list entries): a left-to-right sum from +0.0
//   roi_chunk_reduce_kernel the pixels with several chunks: their partial sums added in chunk order
// kRoiChunk is a constant, so the order of every sum depends on the sizes and the boxes alone, never on the device.
// The gradient of the boxes (roi_box_grad_kernel) is one workgroup per row: stnbhwd's updateGradInput, AffineGridGenerator's
// and BoxToAffine's backward (BoxToAffine.lua:107-110), the channel dot products and the sum over points in double.
#include "common.h"

#include <algorithm>

#pragma clang fp contract(off)

#include "roi_sample.h"

namespace {

constexpr int kRoiMaxPts = 256;     // HH * WW, as the forward
constexpr int kRoiChunk = 128;      // list entries one work item sums
constexpr int kRoiSortLds = 4096;   // the longest list sorted in LDS
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(256) void roi_taps_kernel(const float* __restrict__ boxes, int h, int w, float img_h, float img_w,
                                                       int HH, int WW, int32_t* __restrict__ tap_pix, float* __restrict__ tap_w,
                                                       int32_t* __restrict__ count) {
  const int b = blockIdx.x, p = threadIdx.x, P = HH * WW;
  if (p >= P) return;
  const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + (size_t)b * 4);
  const RoiPoint pt = roi_point(bx, img_h, img_w, HH, WW, p / WW, p % WW, h, w);
  int pix[4];
  float wt[4];
  roi_tap_pixels(pt.x0, pt.y0, h, w, pix);
  roi_tap_weights(pt.wx, pt.wy, wt);
  const size_t t0 = ((size_t)b * P + p) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tap_pix[t0 + k] = pix[k];
    tap_w[t0 + k] = wt[k];
    if (count != nullptr && pix[k] >= 0) atomicAdd(&count[pix[k]], 1);
  }
}

// start[i] = taps of the pixels before i (start[npix] = all); cursor = start; chunk0[i] = work items before pixel i, a pixel
// having max(1, ceil(count / kRoiChunk)) of them (an empty pixel's one item writes its zeros); item_pix[item] = its pixel
__global__ __launch_bounds__(kScanThreads) void roi_index_scan_kernel(const int32_t* __restrict__ count, int npix,
                                                                      int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                                      int32_t* __restrict__ chunk0, int32_t* __restrict__ item_pix) {
  __shared__ int s_wave[2][kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int per = (npix + kScanThreads - 1) / kScanThreads;
  const int i0 = min(npix, tid * per), i1 = min(npix, i0 + per);
  int c = 0, q = 0;
  for (int i = i0; i < i1; ++i) { const int n = count[i]; c += n; q += max(1, (n + kRoiChunk - 1) / kRoiChunk); }
  int ic = c, iq = q;
  for (int off = 1; off < 64; off <<= 1) {
    const int oc = __shfl_up(ic, off, 64), oq = __shfl_up(iq, off, 64);
    if (lane >= off) { ic += oc; iq += oq; }
  }
  if (lane == 63) { s_wave[0][wid] = ic; s_wave[1][wid] = iq; }
  __syncthreads();
  int bc = 0, bq = 0;
  for (int v = 0; v < wid; ++v) { bc += s_wave[0][v]; bq += s_wave[1][v]; }
  int rc = bc + ic - c, rq = bq + iq - q;            // taps and items in front of this thread's pixels
  for (int i = i0; i < i1; ++i) {
    const int n = count[i], m = max(1, (n + kRoiChunk - 1) / kRoiChunk);
    start[i] = rc; cursor[i] = rc; chunk0[i] = rq;
    for (int k = 0; k < m; ++k) item_pix[rq + k] = i;
    rc += n; rq += m;
  }
  if (tid == kScanThreads - 1) { start[npix] = rc; chunk0[npix] = rq; }
}

__global__ __launch_bounds__(256) void roi_place_kernel(const int32_t* __restrict__ tap_pix, int T, int32_t* __restrict__ cursor,
                                                        int32_t* __restrict__ list) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int pix = tap_pix[t];
  if (pix >= 0) list[atomicAdd(&cursor[pix], 1)] = t;
}

// ascending bitonic sort of a[0 .. n) by one workgroup; the network is the all-ascending one (first step of a stage mirrors,
// the others shift), so the virtual padding up to a power of two (+inf at indices >= n) never moves and is simply skipped
__device__ __forceinline__ void roi_sort_block(int32_t* a, int n, int tid) {
  int npad = 2;
  while (npad < n) npad <<= 1;
  for (int k = 2; k <= npad; k <<= 1) {
    const int hk = k >> 1;
    for (int t = tid; t < (npad >> 1); t += 256) {
      const int blk = t / hk, off = t - blk * hk;
      const int l = blk * k + off, r = blk * k + k - 1 - off;
      if (r < n) { const int32_t x = a[l], y = a[r]; if (x > y) { a[l] = y; a[r] = x; } }
    }
    __syncthreads();
    for (int j = k >> 2; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += 256) {
        const int l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), r = l | j;
        if (r < n) { const int32_t x = a[l], y = a[r]; if (x > y) { a[l] = y; a[r] = x; } }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void roi_sort_lists_kernel(const int32_t* __restrict__ start, int npix, int32_t* list) {
  __shared__ int32_t s_a[kRoiSortLds];
  const int tid = threadIdx.x;
  for (int pix = blockIdx.x; pix < npix; pix += gridDim.x) {
    const int b = start[pix], n = start[pix + 1] - b;
    if (n < 2) continue;                                    // (n is the same for the whole workgroup)
    if (n <= kRoiSortLds) {
      for (int i = tid; i < n; i += 256) s_a[i] = list[b + i];
      __syncthreads();
      roi_sort_block(s_a, n, tid);
      for (int i = tid; i < n; i += 256) list[b + i] = s_a[i];
      __syncthreads();
    } else {
      roi_sort_block(list + b, n, tid);
    }
  }
}

// work item (pixel, chunk): out[c] = ((0 + w_0 d_0[c]) + w_1 d_1[c]) + ... over the chunk's list entries in their order
__global__ __launch_bounds__(128) void roi_scatter_sum_kernel(const float* __restrict__ dout, int C, const int32_t* __restrict__ list,
                                                              const float* __restrict__ tap_w, const int32_t* __restrict__ start,
                                                              const int32_t* __restrict__ chunk0, const int32_t* __restrict__ item_pix,
                                                              int npix, float* __restrict__ dfeat, float* __restrict__ part) {
  __shared__ int32_t s_src[kRoiChunk];      // the dpool row: tap >> 2 = row * P + point
  __shared__ float s_w[kRoiChunk];
  const int it = blockIdx.x, tid = threadIdx.x;
  if (it >= chunk0[npix]) return;
  const int pix = item_pix[it], c = it - chunk0[pix], nch = chunk0[pix + 1] - chunk0[pix];
  const int s0 = start[pix] + c * kRoiChunk, cnt = min(start[pix + 1] - s0, kRoiChunk);
  if (tid < cnt) {
    const int t = list[s0 + tid];
    s_src[tid] = t >> 2;
    s_w[tid] = tap_w[t];
  }
  __syncthreads();
  float* out = nch == 1 ? dfeat + (size_t)pix * C : part + (size_t)it * C;
  const int C4 = C >> 2;
  for (int c4 = tid; c4 < C4; c4 += 128) {
    const float* src = dout + (size_t)c4 * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 4 <= cnt; k += 4) {                          // four rows travel together; they are added one after the other
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (size_t)s_src[k] * C);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + (size_t)s_src[k + 1] * C);
      const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + (size_t)s_src[k + 2] * C);
      const f32x4 v3 = *reinterpret_cast<const f32x4*>(src + (size_t)s_src[k + 3] * C);
      const float w0 = s_w[k], w1 = s_w[k + 1], w2 = s_w[k + 2], w3 = s_w[k + 3];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc[e] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc[e], __fmul_rn(w0, v0[e])), __fmul_rn(w1, v1[e])), __fmul_rn(w2, v2[e])),
                           __fmul_rn(w3, v3[e]));
    }
    for (; k < cnt; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)s_src[k] * C);
      const float wv = s_w[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(wv, v[e]));
    }
    *reinterpret_cast<f32x4*>(out + (size_t)c4 * 4) = acc;
  }
}

__global__ __launch_bounds__(128) void roi_chunk_reduce_kernel(const float* __restrict__ part, int C, const int32_t* __restrict__ chunk0,
                                                               float* __restrict__ dfeat) {
  const int pix = blockIdx.x, i0 = chunk0[pix], nch = chunk0[pix + 1] - i0;
  if (nch < 2) return;
  const int C4 = C >> 2;
  for (int c4 = threadIdx.x; c4 < C4; c4 += 128) {
    f32x4 acc = *reinterpret_cast<const f32x4*>(part + (size_t)i0 * C + (size_t)c4 * 4);
    for (int k = 1; k < nch; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(part + (size_t)(i0 + k) * C + (size_t)c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], v[e]);
    }
    *reinterpret_cast<f32x4*>(dfeat + (size_t)pix * C + (size_t)c4 * 4) = acc;
  }
}

// One workgroup per row.  A wave takes the points wid, wid + 4, ...: every lane adds its channels' products feat[tap][c] *
// dout[c] (c ascending, four doubles, an out-of-map tap reading zero), the 64 lanes are added by a butterfly; lane 0 forms
//   d/dycoord = -wx TL + wx BL - (1 - wx) TR + (1 - wx) BR,  d/dxcoord = -wy TL + wy TR - (1 - wy) BL + (1 - wy) BR
// (the floor held constant), times (h - 1) / 2 and (w - 1) / 2.  Thread 0 then adds over the points in ascending order:
// dtheta = sum dgrid (x) base grid, and BoxToAffine's backward gives (dxc, dyc, dw, dh).
__global__ __launch_bounds__(256) void roi_box_grad_kernel(const float* __restrict__ feat, int h, int w, int C,
                                                           const float* __restrict__ boxes, float img_h, float img_w, int HH, int WW,
                                                           const float* __restrict__ dout, float* __restrict__ dboxes) {
  __shared__ int s_x0[kRoiMaxPts], s_y0[kRoiMaxPts];
  __shared__ float s_wx[kRoiMaxPts], s_wy[kRoiMaxPts];
  __shared__ double s_dg[kRoiMaxPts][2];              // d/dgy, d/dgx
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, P = HH * WW, C4 = C >> 2;
  if (tid < P) {
    const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + (size_t)b * 4);
    const RoiPoint pt = roi_point(bx, img_h, img_w, HH, WW, tid / WW, tid % WW, h, w);
    s_x0[tid] = pt.x0; s_y0[tid] = pt.y0; s_wx[tid] = pt.wx; s_wy[tid] = pt.wy;
  }
  __syncthreads();
  for (int p = wid; p < P; p += 4) {
    int pix[4];
    roi_tap_pixels(s_x0[p], s_y0[p], h, w, pix);
    const float* g = dout + ((size_t)b * P + p) * C;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int c4 = lane; c4 < C4; c4 += 64) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (size_t)c4 * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 tv = pix[k] >= 0 ? *reinterpret_cast<const f32x4*>(feat + (size_t)pix[k] * C + (size_t)c4 * 4) : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[k] = d[k] + (double)tv[e] * (double)gv[e];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) d[k] = d[k] + __shfl_xor(d[k], o, 64);
    if (lane == 0) {
      const double wx = (double)s_wx[p], wy = (double)s_wy[p];
      const double ux = (double)__fsub_rn(1.f, s_wx[p]), uy = (double)__fsub_rn(1.f, s_wy[p]);
      const double dy = ((-(wx * d[0]) + wx * d[2]) - ux * d[1]) + ux * d[3];
      const double dx = ((-(wy * d[0]) + wy * d[1]) - uy * d[2]) + uy * d[3];
      s_dg[p][0] = dy * (double)(h - 1) / 2.0;
      s_dg[p][1] = dx * (double)(w - 1) / 2.0;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double th11 = 0.0, th13 = 0.0, th22 = 0.0, th23 = 0.0;
    for (int p = 0; p < P; ++p) {
      const double yb = (double)roi_base_coord(p / WW, HH), xb = (double)roi_base_coord(p % WW, WW);
      th11 = th11 + s_dg[p][0] * yb;
      th13 = th13 + s_dg[p][0];
      th22 = th22 + s_dg[p][1] * xb;
      th23 = th23 + s_dg[p][1];
    }
    const f32x4 o = {(float)(th23 * (2.0 / ((double)img_w - 1.0))), (float)(th13 * (2.0 / ((double)img_h - 1.0))),
                     (float)(th22 * (1.0 / (double)img_w)), (float)(th11 * (1.0 / (double)img_h))};
    *reinterpret_cast<f32x4*>(dboxes + (size_t)b * 4) = o;
  }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

static size_t roi_grad_items_max(int B, int P, int npix) { return (size_t)B * P * 4 / kRoiChunk + (size_t)npix + 1; }

size_t roi_grad_ws_bytes(int B, int P, int npix, int C) {
  const size_t T = (size_t)B * P * 4, items = roi_grad_items_max(B, P, npix);
  return 3 * up256(T * 4) + 4 * up256(((size_t)npix + 1) * 4) + up256(items * 4) + up256(items * C * 4);
}

RoiGradWs roi_grad_carve(void* base, int B, int P, int npix, int C) {
  const size_t T = (size_t)B * P * 4, items = roi_grad_items_max(B, P, npix), np1 = up256(((size_t)npix + 1) * 4);
  char* p = static_cast<char*>(base);
  RoiGradWs ws;
  ws.tap_pix = reinterpret_cast<int32_t*>(p); p += up256(T * 4);
  ws.tap_w = reinterpret_cast<float*>(p); p += up256(T * 4);
  ws.list = reinterpret_cast<int32_t*>(p); p += up256(T * 4);
  ws.count = reinterpret_cast<int32_t*>(p); p += np1;
  ws.start = reinterpret_cast<int32_t*>(p); p += np1;
  ws.cursor = reinterpret_cast<int32_t*>(p); p += np1;
  ws.chunk0 = reinterpret_cast<int32_t*>(p); p += np1;
  ws.item_pix = reinterpret_cast<int32_t*>(p); p += up256(items * 4);
  ws.part = reinterpret_cast<float*>(p);
  return ws;
}

static bool roi_grad_shape_ok(int h, int w, int B, int HH, int WW) {
  return h >= 1 && w >= 1 && B >= 1 && HH >= 2 && WW >= 2 && HH * WW <= kRoiMaxPts && (long long)h * w <= (1 << 16) &&
         (long long)B * HH * WW * 4 <= (1 << 30);
}

hipError_t launch_roi_tap_index(const float* boxes, int B, int h, int w, int img_h, int img_w, int HH, int WW, const RoiGradWs& ws,
                                hipStream_t s) {
  if (!roi_grad_shape_ok(h, w, B, HH, WW)) return hipErrorInvalidValue;
  const int npix = h * w, T = B * HH * WW * 4;
  hipError_t e = hipMemsetAsync(ws.count, 0, (size_t)npix * 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(roi_taps_kernel, dim3(B), dim3(256), 0, s, boxes, h, w, (float)img_h, (float)img_w, HH, WW, ws.tap_pix, ws.tap_w,
                     ws.count);
  hipLaunchKernelGGL(roi_index_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.count, npix, ws.start, ws.cursor, ws.chunk0,
                     ws.item_pix);
  hipLaunchKernelGGL(roi_place_kernel, dim3((T + 255) / 256), dim3(256), 0, s, ws.tap_pix, T, ws.cursor, ws.list);
  hipLaunchKernelGGL(roi_sort_lists_kernel, dim3(std::min(npix, 65535)), dim3(256), 0, s, ws.start, npix, ws.list);
  return hipGetLastError();
}

hipError_t launch_roi_scatter_sum(const float* dout, int B, int h, int w, int C, int HH, int WW, const RoiGradWs& ws, float* dfeat,
                                  hipStream_t s) {
  if (!roi_grad_shape_ok(h, w, B, HH, WW) || C < 4 || (C & 3)) return hipErrorInvalidValue;
  const int npix = h * w;
  const unsigned items = (unsigned)roi_grad_items_max(B, HH * WW, npix);
  hipLaunchKernelGGL(roi_scatter_sum_kernel, dim3(items), dim3(128), 0, s, dout, C, ws.list, ws.tap_w, ws.start, ws.chunk0, ws.item_pix,
                     npix, dfeat, ws.part);
  hipLaunchKernelGGL(roi_chunk_reduce_kernel, dim3(npix), dim3(128), 0, s, ws.part, C, ws.chunk0, dfeat);
  return hipGetLastError();
}

hipError_t launch_roi_box_grad(const float* feat_hwc, int h, int w, int C, const float* boxes, int B, int img_h, int img_w, int HH,
                               int WW, const float* dout, float* dboxes, hipStream_t s) {
  if (!roi_grad_shape_ok(h, w, B, HH, WW) || C < 4 || (C & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(roi_box_grad_kernel, dim3(B), dim3(256), 0, s, feat_hwc, h, w, C, boxes, (float)img_h, (float)img_w, HH, WW, dout,
                     dboxes);
  return hipGetLastError();
}

// ---- the two end criteria and the recognition heads ---------------------------------------------------------------------------
namespace {

// One launch for both criteria (LogisticCriterion.lua:124-130, BoxRegressionCriterion.lua:50-79, InvertBoxTransform.lua:63-98).
// Row r of n, the first np positive.  All in double on the fp32 inputs, cast once:
//   dobj[r]    = w_obj * (-exp(-(x + log_den)) + [r >= np]) / n,  log_den = log(1 + exp(-x)) formed as the loss forms it
//   dtrans[r]  = w_box * clamp(trans - t, -1, 1) / (4 np) for r < np, t = InvertBoxTransform(anchor, target); a row with
//                max |t| > 10 has trans and t zeroed: zero gradient, counted in *masked
//   danchor[r] = (dtx / wa, dty / ha, (tx dtx + dtw) / wa, (ty dty + dth) / ha), tx and ty read after the masking
__global__ __launch_bounds__(256) void end_crit_grad_kernel(const float* __restrict__ obj, const float* __restrict__ trans,
                                                            const float* __restrict__ anchors, const float* __restrict__ target,
                                                            int n, int np, float w_obj, float w_box, float* __restrict__ dobj,
                                                            float* __restrict__ dtrans, float* __restrict__ danchor,
                                                            int32_t* __restrict__ masked) {
  __shared__ int s_masked;
  if (threadIdx.x == 0) s_masked = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < n; r += 256) {
    const double x = (double)obj[r], off = x < 0.0 ? x : 0.0;
    const double log_den = log(exp(off) + exp(off - x)) - off;
    double g = -exp(-(x + log_den));
    if (r >= np) g = g + 1.0;
    dobj[r] = (float)((double)w_obj * (g / (double)n));
    if (r < np) {
      const double xa = anchors[r * 4 + 0], ya = anchors[r * 4 + 1], wa = anchors[r * 4 + 2], ha = anchors[r * 4 + 3];
      const double xt = target[r * 4 + 0], yt = target[r * 4 + 1], wt = target[r * 4 + 2], ht = target[r * 4 + 3];
      double t[4] = {(xt - xa) / wa, (yt - ya) / ha, log(wt / wa), log(ht / ha)};
      double mx = fabs(t[0]);
      for (int d = 1; d < 4; ++d) { const double v = fabs(t[d]); if (v > mx) mx = v; }
      double dt[4] = {0.0, 0.0, 0.0, 0.0};
      if (mx > 10.0) {
        atomicAdd(&s_masked, 1);
        t[0] = 0.0; t[1] = 0.0;
      } else {
        for (int d = 0; d < 4; ++d) {
          const double z = (double)trans[r * 4 + d] - t[d];
          dt[d] = (double)w_box * ((z < -1.0 ? -1.0 : (z > 1.0 ? 1.0 : z)) / (4.0 * (double)np));
        }
      }
      for (int d = 0; d < 4; ++d) dtrans[r * 4 + d] = (float)dt[d];
      danchor[r * 4 + 0] = (float)(dt[0] / wa);
      danchor[r * 4 + 1] = (float)(dt[1] / ha);
      danchor[r * 4 + 2] = (float)((t[0] * dt[0] + dt[2]) / wa);
      danchor[r * 4 + 3] = (float)((t[1] * dt[1] + dt[3]) / ha);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *masked = s_masked;
}

// Workgroups [0, n): row r of dcodes = dobj_r * w5[0] + [r < np] (sum_d dtrans_{r,d} w5[1 + d] + g_r), in double, cast once.
// Workgroups from n on: 256 of the 5 * D weight-gradient entries each -- dw5[k][j] = sum_r dhead_{r,k} codes_{r,j} in double in
// ascending r (dhead_{r,0} = dobj_r, dhead_{r,1+d} = dtrans_{r,d} for r < np); the first five threads of workgroup n also give
// db5[k] = sum_r dhead_{r,k}.
__global__ __launch_bounds__(256) void heads_bwd_kernel(const float* __restrict__ codes, const float* __restrict__ w5,
                                                        const float* __restrict__ dobj, const float* __restrict__ dtrans,
                                                        const float* __restrict__ g, int n, int np, int D, float* __restrict__ dcodes,
                                                        float* __restrict__ dw5, float* __restrict__ db5) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < n) {
    const int r = blk;
    const double a = (double)dobj[r];
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < np)
      for (int d = 0; d < 4; ++d) b[d] = (double)dtrans[r * 4 + d];
    for (int j = tid; j < D; j += 256) {
      double v = a * (double)w5[j];
      if (r < np) {
        for (int d = 0; d < 4; ++d) v = v + b[d] * (double)w5[(size_t)(1 + d) * D + j];
        if (g != nullptr) v = v + (double)g[(size_t)r * D + j];
      }
      dcodes[(size_t)r * D + j] = (float)v;
    }
    return;
  }
  const int e = (blk - n) * 256 + tid;
  if (e < 5 * D) {
    const int k = e / D, j = e - k * D, rows = k == 0 ? n : np;
    double v = 0.0;
    for (int r = 0; r < rows; ++r) v = v + (double)(k == 0 ? dobj[r] : dtrans[r * 4 + k - 1]) * (double)codes[(size_t)r * D + j];
    dw5[e] = (float)v;
  }
  if (blk == n && tid < 5) {
    const int k = tid, rows = k == 0 ? n : np;
    double v = 0.0;
    for (int r = 0; r < rows; ++r) v = v + (double)(k == 0 ? dobj[r] : dtrans[r * 4 + k - 1]);
    db5[k] = (float)v;
  }
}

// out[n][c * HW + p] = in[n][p * C + c]: the inverse of permute_fc6_kernel.  One workgroup per (row, 64 channels): the tile is
// read along c and written as one run of 64 * HW floats.
constexpr int kPermMaxHW = 64;
__global__ __launch_bounds__(256) void permute_fc6_back_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int HW) {
  __shared__ float tile[kPermMaxHW][65];
  const size_t row = (size_t)blockIdx.y * C * HW;
  const int c0 = blockIdx.x * 64;
  for (int i = threadIdx.x; i < HW * 64; i += 256) {
    const int p = i >> 6, cc = i & 63;
    tile[p][cc] = in[row + (size_t)p * C + c0 + cc];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HW * 64; i += 256) {
    const int cc = i / HW, p = i - cc * HW;
    out[row + (size_t)c0 * HW + i] = tile[p][cc];
  }
}

// out[r] = a[r] + (r < np ? b[r] : 0), rows of four floats
__global__ __launch_bounds__(256) void add_pos_rows4_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int np,
                                                            float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n * 4) out[i] = i < np * 4 ? __fadd_rn(a[i], b[i]) : a[i];
}

}  // namespace

hipError_t launch_end_crit_grad(const float* obj, const float* trans, const float* anchors, const float* target, int n, int np,
                                float w_obj, float w_box, float* dobj, float* dtrans, float* danchor, int32_t* masked, hipStream_t s) {
  if (n < 1 || np < 0 || np > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(end_crit_grad_kernel, dim3(1), dim3(256), 0, s, obj, trans, anchors, target, n, np, w_obj, w_box, dobj, dtrans,
                     danchor, masked);
  return hipGetLastError();
}
hipError_t launch_heads_bwd(const float* codes, const float* w5, const float* dobj, const float* dtrans, const float* g, int n, int np,
                            int D, float* dcodes, float* dw5, float* db5, hipStream_t s) {
  if (n < 1 || np < 0 || np > n || D < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(heads_bwd_kernel, dim3(n + (5 * D + 255) / 256), dim3(256), 0, s, codes, w5, dobj, dtrans, g, n, np, D, dcodes, dw5,
                     db5);
  return hipGetLastError();
}
hipError_t launch_permute_fc6_back(const float* in, float* out, int N, int C, int HW, hipStream_t s) {
  if (N < 1 || N > 65535 || C < 64 || (C & 63) || HW < 1 || HW > kPermMaxHW) return hipErrorInvalidValue;
  hipLaunchKernelGGL(permute_fc6_back_kernel, dim3(C / 64, N), dim3(256), 0, s, in, out, C, HW);
  return hipGetLastError();
}
hipError_t launch_add_pos_rows4(const float* a, const float* b, int n, int np, float* out, hipStream_t s) {
  hipLaunchKernelGGL(add_pos_rows4_kernel, dim3((n * 4 + 255) / 256), dim3(256), 0, s, a, b, n, np, out);
  return hipGetLastError();
}
