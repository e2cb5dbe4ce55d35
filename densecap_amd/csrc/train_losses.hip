// Validation losses, first stage: nn.BoxSampler on the device (dc_op_box_sampler; docs/SEMANTICS.md, "Validation losses";
// BoxSampler.lua:64-167).  A translation unit of its own, compiled with -ffp-contract=off: every decision is exact.
//
// Two launches:
//   * box_sampler_match_kernel, 256 inputs a workgroup: the ground truth's corners and areas are staged once in LDS, every thread
//     keeps its input's running max / arg-max over the G ground-truth boxes in registers (strict >, so the lower index wins a tie;
//     a NaN never wins) -- the A x G matrix is never written.  The other direction, every ground-truth box's best input, is an
//     INTEGER max of (ordered IoU bits << 32 | ~input index): first into a per-workgroup LDS slab (a plain read filters out the
//     entries that cannot win, so few atomics are issued), then one 64-bit atomicMax per box and workgroup into global memory.
//     Integer max does not depend on the order of arrival; no float atomics anywhere.
//   * box_sampler_draw_kernel, one workgroup of 1024 per class (0 = positives, 1 = negatives), each on its own copy of the mask
//     bytes so that the two never wait for each other: thresholds and the bounds rule, the forced positives, the counts (integer
//     adds), the no-negatives fallback; then the class's draws.  Without replacement: the `num` smallest (key << 32 | index) by a
//     radix select over the 64-bit composite (eight 8-bit passes of an LDS histogram; composites are distinct, so the threshold
//     is one element and exactly `num` pass it), sorted bitonically in LDS.  With replacement, and for caller-forced lists: the
//     r-th candidate in ascending order, found through per-thread chunk counts, their scan and a walk of one chunk.
#include "common.h"

typedef unsigned long long u64;

constexpr int BS_MAX_GT = 512;
constexpr int BS_MAX_BATCH = 1024;
constexpr int BS_DRAW_THREADS = 1024;

// the IoU of box_iou_kernel (boxes.hip) under convention 0, operation for operation: p = the input, q = the ground-truth box
__device__ __forceinline__ float bs_iou(float px1, float py1, float px2, float py2, float a1, float qx1, float qy1, float qx2,
                                        float qy2, float a2) {
  const float x0 = fmaxf(px1, qx1), y0 = fmaxf(py1, qy1), x1 = fminf(px2, qx2), y1 = fminf(py2, qy2);
  float w = __fadd_rn(__fsub_rn(x1, x0), 0.f), h = __fadd_rn(__fsub_rn(y1, y0), 0.f);
  w = w > 0.f ? w : 0.f;
  h = h > 0.f ? h : 0.f;
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fsub_rn(__fadd_rn(a1, a2), inter));
}

// bits that order as the floats do (NaN excluded by the caller; -0 == +0)
__device__ __forceinline__ uint32_t bs_ordered_bits(float v) {
  if (v == 0.f) v = 0.f;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void box_sampler_match_kernel(const float* __restrict__ boxes, const float* __restrict__ gt, int A,
                                                                int G, float* __restrict__ max_iou, int32_t* __restrict__ arg,
                                                                float* __restrict__ max_iou_user, int32_t* __restrict__ arg_user,
                                                                u64* __restrict__ gbest) {
  __shared__ float s_gt[BS_MAX_GT * 5];          // x1 y1 x2 y2 area
  __shared__ u64 s_best[BS_MAX_GT];
  const int tid = threadIdx.x;
  for (int j = tid; j < G; j += 256) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(gt + (size_t)j * 4);
    float x1, y1, x2, y2;
    corners(q[0], q[1], q[2], q[3], x1, y1, x2, y2);
    s_gt[j * 5 + 0] = x1; s_gt[j * 5 + 1] = y1; s_gt[j * 5 + 2] = x2; s_gt[j * 5 + 3] = y2;
    s_gt[j * 5 + 4] = __fmul_rn(q[2], q[3]);
    s_best[j] = 0ull;
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  if (i < A) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
    float px1, py1, px2, py2;
    corners(p[0], p[1], p[2], p[3], px1, py1, px2, py2);
    const float a1 = __fmul_rn(p[2], p[3]);
    const u64 low = (u64)(~(uint32_t)i);
    float best = __uint_as_float(0x7fc00000u);   // NaN until a number is seen
    int jbest = 0;
    for (int j = 0; j < G; ++j) {
      const float v = bs_iou(px1, py1, px2, py2, a1, s_gt[j * 5 + 0], s_gt[j * 5 + 1], s_gt[j * 5 + 2], s_gt[j * 5 + 3], s_gt[j * 5 + 4]);
      if (v != v) continue;
      if (best != best || v > best) { best = v; jbest = j; }
      const u64 key = ((u64)bs_ordered_bits(v) << 32) | low;
      if (key > s_best[j]) atomicMax(&s_best[j], key);           // (the read only filters: the slab grows monotonically)
    }
    max_iou[i] = best;
    arg[i] = jbest;
    if (max_iou_user) max_iou_user[i] = best;
    if (arg_user) arg_user[i] = jbest;
  }
  __syncthreads();
  for (int j = tid; j < G; j += 256)
    if (s_best[j] != 0ull) atomicMax(&gbest[j], s_best[j]);
}

__device__ __forceinline__ bool bs_member(uint8_t b, int cls, int noneg) {
  return cls == 0 ? (b & 1) != 0 : (noneg ? (b & 1) == 0 : (b & 2) != 0);
}
__device__ __forceinline__ u64 bs_composite(uint32_t i, int cls, uint32_t k0, uint32_t k1) {
  return ((u64)philox4x32_10(i, 0u, (uint32_t)cls, 0u, k0, k1).w[0] << 32) | (u64)i;
}

__global__ __launch_bounds__(BS_DRAW_THREADS) void box_sampler_draw_kernel(BoxSamplerArgs a, const float* __restrict__ max_iou,
                                                                           const int32_t* __restrict__ arg,
                                                                           const u64* __restrict__ gbest, uint8_t* __restrict__ mask) {
  __shared__ u64 s_buf[BS_MAX_BATCH];
  __shared__ int s_off[BS_DRAW_THREADS + 1];
  __shared__ int s_hist[256];
  __shared__ int s_wave[BS_DRAW_THREADS / 64];
  __shared__ int s_cnt[2], s_n, s_bad, s_digit, s_k;
  const int cls = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int A = a.A;
  uint8_t* m = mask + (size_t)cls * A;
  if (tid == 0) { s_cnt[0] = 0; s_cnt[1] = 0; s_n = 0; s_bad = 0; }
  // ---- thresholds and bounds ----
  for (int i = tid; i < A; i += BS_DRAW_THREADS) {
    const float v = max_iou[i];
    bool pos = v > a.high, neg = v < a.low;
    if (a.bounds) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(a.boxes + (size_t)i * 4);
      float x1, y1, x2, y2;
      corners(p[0], p[1], p[2], p[3], x1, y1, x2, y2);
      if (x1 < 1.f || y1 < 1.f || x2 > a.x_max || y2 > a.y_max) { pos = false; neg = false; }
    }
    m[i] = (uint8_t)((pos ? 1 : 0) | (neg ? 2 : 0));
  }
  __syncthreads();
  // ---- every ground-truth box's best input is positive, whatever its IoU or bounds ----
  for (int j = tid; j < a.G; j += BS_DRAW_THREADS) {
    const u64 k = gbest[j];
    if (k != 0ull) m[~(uint32_t)k] = 1;           // (several boxes may name one input: they store the same byte)
  }
  __syncthreads();
  // ---- counts ----
  {
    int cp = 0, cn = 0;
    for (int i = tid; i < A; i += BS_DRAW_THREADS) { const uint8_t b = m[i]; cp += b & 1; cn += (b >> 1) & 1; }
    for (int off = 32; off > 0; off >>= 1) { cp += __shfl_xor(cp, off, 64); cn += __shfl_xor(cn, off, 64); }
    if (lane == 0) { atomicAdd(&s_cnt[0], cp); atomicAdd(&s_cnt[1], cn); }
  }
  __syncthreads();
  const int total_pos = s_cnt[0];
  int total_neg = s_cnt[1], flags = 0;
  const int noneg = total_neg == 0;
  if (noneg) { flags |= 1; total_neg = A - total_pos; }
  int num_pos = min(a.batch / 2, total_pos);
  int num_neg = total_neg > 0 ? a.batch - num_pos : 0;
  const bool replace = total_neg < num_neg;
  if (replace) flags |= 2;
  if (a.forced_pos) num_pos = a.n_forced_pos;
  if (a.forced_neg) num_neg = a.n_forced_neg;
  const int total = cls ? total_neg : total_pos, num = cls ? num_neg : num_pos;
  const int32_t* forced = cls ? a.forced_neg : a.forced_pos;
  int32_t* out_idx = cls ? a.neg_input_idx : a.pos_input_idx;
  if (forced != nullptr || (cls == 1 && replace)) {
    // ---- the r-th candidate in ascending order ----
    const int chunk = (A + BS_DRAW_THREADS - 1) / BS_DRAW_THREADS;
    const int i0 = min(A, tid * chunk), i1 = min(A, i0 + chunk);
    int c = 0;
    for (int i = i0; i < i1; ++i) c += bs_member(m[i], cls, noneg) ? 1 : 0;
    int incl = c;
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wid; ++w) base += s_wave[w];
    s_off[tid] = base + incl - c;                 // candidates in front of this thread's chunk
    if (tid == BS_DRAW_THREADS - 1) s_off[BS_DRAW_THREADS] = base + incl;
    __syncthreads();
    for (int q = tid; q < num; q += BS_DRAW_THREADS) {
      long long r = forced ? (long long)forced[q]
                           : (long long)(((u64)philox4x32_10((uint32_t)q, 1u, (uint32_t)cls, 0u, a.seed_lo, a.seed_hi).w[0] * (u64)total) >> 32);
      int found = -1;
      if (r >= 0 && r < total) {
        int lo = 0, hi = BS_DRAW_THREADS - 1;     // the last chunk whose offset is <= r
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_off[mid] <= (int)r) lo = mid; else hi = mid - 1;
        }
        int left = (int)r - s_off[lo];
        const int e0 = min(A, lo * chunk), e1 = min(A, e0 + chunk);
        for (int i = e0; i < e1; ++i)
          if (bs_member(m[i], cls, noneg)) { if (left == 0) { found = i; break; } --left; }
      }
      if (found < 0) atomicAdd(&s_bad, 1);
      out_idx[q] = found;
      if (cls == 0) a.pos_target_idx[q] = found >= 0 ? arg[found] : -1;
    }
  } else if (num > 0) {
    // ---- the num smallest (key, index): radix select on the 64-bit composite, most significant digit first ----
    u64 prefix = 0ull;
    int k = num;
    for (int pass = 7; pass >= 0; --pass) {
      const int shift = pass * 8;
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < A; i += BS_DRAW_THREADS) {
        if (!bs_member(m[i], cls, noneg)) continue;
        const u64 comp = bs_composite((uint32_t)i, cls, a.seed_lo, a.seed_hi);
        if (pass == 7 || (comp >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((comp >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int acc = 0, d = 0;
        for (; d < 255; ++d) {
          if (acc + s_hist[d] >= k) break;
          acc += s_hist[d];
        }
        s_digit = d;
        s_k = k - acc;
      }
      __syncthreads();
      prefix |= (u64)s_digit << shift;
      k = s_k;
    }
    for (int i = tid; i < A; i += BS_DRAW_THREADS) {
      if (!bs_member(m[i], cls, noneg)) continue;
      const u64 comp = bs_composite((uint32_t)i, cls, a.seed_lo, a.seed_hi);
      if (comp <= prefix) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < BS_MAX_BATCH) s_buf[slot] = comp;
      }
    }
    __syncthreads();
    int npad = 2;
    while (npad < num) npad <<= 1;
    for (int t = tid; t < npad; t += BS_DRAW_THREADS)
      if (t >= num) s_buf[t] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= npad; kk <<= 1)
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (npad >> 1); t += BS_DRAW_THREADS) {
          const int l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), r = l | j;
          const u64 x = s_buf[l], y = s_buf[r];
          if ((x > y) == ((l & kk) == 0)) { s_buf[l] = y; s_buf[r] = x; }
        }
        __syncthreads();
      }
    for (int q = tid; q < num; q += BS_DRAW_THREADS) {
      const int i = (int)(uint32_t)s_buf[q];
      out_idx[q] = i;
      if (cls == 0) a.pos_target_idx[q] = arg[i];
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (cls == 0) { a.counts[0] = num_pos; a.counts[2] = total_pos; a.counts[5] = s_bad; }
    else { a.counts[1] = num_neg; a.counts[3] = total_neg; a.counts[4] = flags; a.counts[6] = s_bad; a.counts[7] = 0; }
  }
}

// workspace: gbest u64 [G] | max_iou float [A] | arg int32 [A] | mask bytes [2 A]
size_t box_sampler_ws_bytes(int A, int G) {
  return (((size_t)G * 8 + (size_t)A * 4 + (size_t)A * 4 + (size_t)A * 2) + 255) & ~(size_t)255;
}

hipError_t launch_box_sampler(const BoxSamplerArgs& a, hipStream_t s) {
  if (a.A < 1 || a.G < 1 || a.G > BS_MAX_GT || a.batch < 2 || a.batch > BS_MAX_BATCH || (a.batch & 1)) return hipErrorInvalidValue;
  if ((a.forced_pos && (a.n_forced_pos < 0 || a.n_forced_pos > BS_MAX_BATCH)) ||
      (a.forced_neg && (a.n_forced_neg < 0 || a.n_forced_neg > BS_MAX_BATCH)))
    return hipErrorInvalidValue;
  u64* gbest = reinterpret_cast<u64*>(a.ws);
  float* max_iou = reinterpret_cast<float*>(gbest + a.G);
  int32_t* arg = reinterpret_cast<int32_t*>(max_iou + a.A);
  uint8_t* mask = reinterpret_cast<uint8_t*>(arg + a.A);
  hipError_t e = hipMemsetAsync(gbest, 0, (size_t)a.G * 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(box_sampler_match_kernel, dim3((a.A + 255) / 256), dim3(256), 0, s, a.boxes, a.gt, a.A, a.G, max_iou, arg,
                     a.max_iou_user, a.arg_user, gbest);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(box_sampler_draw_kernel, dim3(2), dim3(BS_DRAW_THREADS), 0, s, a, max_iou, arg, gbest, mask);
  return hipGetLastError();
}

// ---- the five loss terms (docs/SEMANTICS.md, "Validation losses") ----------------------------------------------------------------
// The RPN's raw two-class scores as rows: out[b * 2 + d] = heads[(y * w + x) * 6k + 4k + 2a + d] for row b = a * h * w + y * w + x
// (ReshapeBoxFeatures order; column 0 is the positive class)
__global__ void rpn_score_rows_kernel(const float* __restrict__ heads, int h, int w, int k, float* __restrict__ out) {
  const int total = k * h * w;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  const int a = b / (h * w), cell = b - a * h * w;
  const float* p = heads + (size_t)cell * 6 * k + 4 * k + 2 * a;
  out[(size_t)b * 2 + 0] = p[0];
  out[(size_t)b * 2 + 1] = p[1];
}
hipError_t launch_rpn_score_rows(const float* heads, int h, int w, int k, float* out, hipStream_t s) {
  const int total = k * h * w;
  hipLaunchKernelGGL(rpn_score_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, s, heads, h, w, k, out);
  return hipGetLastError();
}

constexpr int LT_THREADS = 256;
constexpr int LT_ROWS = 1024;          // rows of a term's summand table (batch_size <= 1024), the leaves of its fixed tree

// sum of buf[0 .. LT_ROWS) by a tree whose shape depends on nothing: strides 512, 256 .. 1 (all threads call it)
__device__ __forceinline__ double lt_tree_sum(double* buf, int tid) {
  __syncthreads();
  for (int stride = LT_ROWS / 2; stride > 0; stride >>= 1) {
    for (int t = tid; t < stride; t += LT_THREADS) buf[t] = buf[t] + buf[t + stride];
    __syncthreads();
  }
  const double r = buf[0];
  __syncthreads();
  return r;
}
// -LogSoftMax(s)[c] of a two-class row, in double
__device__ __forceinline__ double lt_nll2(float s0, float s1, int c) {
  const double a = (double)s0, b = (double)s1, m = b > a ? b : a;
  const double lse = log(exp(a - m) + exp(b - m)) + m;
  return lse - (c == 0 ? a : b);
}
// SmoothL1 over the four transform parameters of one row against InvertBoxTransform(anchor, target), all in double on the
// fp32 inputs; a row whose largest |target| exceeds 10 contributes zero (prediction and target zeroed) and is counted
__device__ __forceinline__ double lt_box_row(const float* anchor, const float* pred, const float* target, int* masked) {
  const double xa = anchor[0], ya = anchor[1], wa = anchor[2], ha = anchor[3];
  const double xt = target[0], yt = target[1], wt = target[2], ht = target[3];
  double t[4];
  t[0] = (xt - xa) / wa; t[1] = (yt - ya) / ha; t[2] = log(wt / wa); t[3] = log(ht / ha);
  double mx = fabs(t[0]);
  for (int d = 1; d < 4; ++d) { const double v = fabs(t[d]); if (v > mx) mx = v; }      // (torch max: a NaN entry is not > 10)
  if (mx > 10.0) { *masked = 1; return 0.0; }
  double sum = 0.0;
  for (int d = 0; d < 4; ++d) {
    const double z = fabs((double)pred[d] - t[d]);
    sum = sum + (z < 1.0 ? 0.5 * z * z : z - 0.5);
  }
  return sum;
}

__global__ __launch_bounds__(LT_THREADS) void loss_terms_kernel(LossTermArgs a) {
  __shared__ double buf[LT_ROWS];
  __shared__ int s_masked[2];
  const int tid = threadIdx.x;
  if (tid < 2) s_masked[tid] = 0;
  __syncthreads();
  const int np = a.num_pos, nn = a.num_neg, n = np + nn;
  double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // (a term whose input is null is skipped by every thread: 0.0, no masked row)
  // mid objectness: mean over the positives of -LogSoftMax(s)[0] + mean over the negatives of -LogSoftMax(s)[1]
  if (a.scores != nullptr) {
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) {
      double v = 0.0;
      if (r < np) { const int i = a.pos_input_idx[r]; v = lt_nll2(a.scores[(size_t)i * 2], a.scores[(size_t)i * 2 + 1], 0); }
      buf[r] = v;
    }
    const double mo_pos = lt_tree_sum(buf, tid);
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) {
      double v = 0.0;
      if (r < nn) { const int i = a.neg_input_idx[r]; v = lt_nll2(a.scores[(size_t)i * 2], a.scores[(size_t)i * 2 + 1], 1); }
      buf[r] = v;
    }
    const double mo_neg = lt_tree_sum(buf, tid);
    out[0] = (double)a.w_mid_obj * ((np > 0 ? mo_pos / (double)np : 0.0) + (nn > 0 ? mo_neg / (double)nn : 0.0));
  }
  // mid box regression: the RPN's transforms of the positive rows against their anchors' inverse transform
  if (a.anchors != nullptr) {
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) {
      double v = 0.0;
      if (r < np) {
        const int i = a.pos_input_idx[r];
        int m = 0;
        v = lt_box_row(a.anchors + (size_t)i * 4, a.trans + (size_t)i * 4, a.gt + (size_t)a.pos_target_idx[r] * 4, &m);
        if (m) atomicAdd(&s_masked[0], 1);
      }
      buf[r] = v;
    }
    const double mb = lt_tree_sum(buf, tid);
    out[1] = np > 0 ? (double)a.w_mid_box * (mb / (4.0 * (double)np)) : 0.0;
  }
  // end objectness: the binary logistic loss of every row's recognition logit, the first num_pos rows labelled 1
  if (a.obj != nullptr) {
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) {
      double v = 0.0;
      if (r < n) {
        const double x = (double)a.obj[r], off = x < 0.0 ? x : 0.0;
        v = log(exp(off) + exp(off - x)) - off;
        if (r >= np) v = v + x;
      }
      buf[r] = v;
    }
    const double eo = lt_tree_sum(buf, tid);
    out[2] = n > 0 ? (double)a.w_end_obj * (eo / (double)n) : 0.0;
  }
  // end box regression: the final transforms of the positive rows against their RoI boxes' inverse transform
  if (a.roi_boxes != nullptr) {
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) {
      double v = 0.0;
      if (r < np) {
        int m = 0;
        v = lt_box_row(a.roi_boxes + (size_t)r * 4, a.final_trans + (size_t)r * 4, a.gt + (size_t)a.pos_target_idx[r] * 4, &m);
        if (m) atomicAdd(&s_masked[1], 1);
      }
      buf[r] = v;
    }
    const double eb = lt_tree_sum(buf, tid);
    out[3] = np > 0 ? (double)a.w_end_box * (eb / (4.0 * (double)np)) : 0.0;
  }
  // captioning: -sum of the rows' log-likelihoods over num_pos * (L + 2) (batch and time average)
  if (a.rowlik != nullptr) {
    for (int r = tid; r < LT_ROWS; r += LT_THREADS) buf[r] = r < np ? -a.rowlik[r] : 0.0;
    const double cap = lt_tree_sum(buf, tid);
    out[4] = np > 0 ? (double)a.w_cap * (cap / ((double)np * (double)(a.L + 2))) : 0.0;
  }
  out[5] = (((out[0] + out[1]) + out[2]) + out[3]) + out[4];
  if (tid == 0) {
    for (int d = 0; d < 6; ++d) a.out[d] = out[d];
    a.out_masked[0] = s_masked[0];
    a.out_masked[1] = s_masked[1];
  }
}
hipError_t launch_loss_terms(const LossTermArgs& a, hipStream_t s) {
  if (a.num_pos < 0 || a.num_neg < 0 || a.num_pos > LT_ROWS || a.num_neg > LT_ROWS || a.num_pos + a.num_neg > LT_ROWS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(loss_terms_kernel, dim3(1), dim3(LT_THREADS), 0, s, a);
  return hipGetLastError();
}
