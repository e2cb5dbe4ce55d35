// Evaluation: match one image's detections to its merged ground truth (dc_op_eval_match; docs/SEMANTICS.md, "Evaluation";
// eval/eval_utils.lua:148-221, box_utils.lua:565-612).  A translation unit of its own: boxes.hip's code generation stays as it is.
//
// One workgroup of 256 per image, everything in LDS:
//   * keys: (score key << 32) | row for every detection, bitonic-sorted as in nms_multi_scan_kernel: decreasing score, the lower
//     index first among equals, -0 == +0, NaN behind every number.
//   * the ground truth's corners (float32) and its M x M ">= thr" relation as a bit mask (W = ceil(M / 64) words a row), IoU in
//     float64 on the float32 corners, argument order (lower index, higher index) for both halves: the mask is symmetric.
//   * the merge, by wave 0 alone (no barrier inside the loop): a round is a masked popcount of every alive column, an arg-max over
//     the wave ((count << 16) | (0xffff - column): the most members, then the lowest index), the group = column & alive.
//   * the match, all threads: rank d's best group (strict > from 0) does not depend on the claims, so it is computed in parallel;
//     the claim "first come, first served in score order" is first[target] = min over d of the ranks that claim target
//     (an LDS atomicMin), ok[d] = (first[target] == d).
// Every float64 expression keeps the reference's order of operations; the file is compiled with -ffp-contract=off.
#include "common.h"

typedef unsigned long long u64;

constexpr int EVM_MAX_DET = 4096;
constexpr int EVM_MAX_GT = 512;

__device__ __forceinline__ uint32_t evm_score_key(float s) {
  if (s != s) return 0xfffffffeu;        // NaN: behind -inf (0xff800000), in front of the padding (all ones)
  if (s == 0.f) s = 0.f;                 // -0 == +0
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

// math.max(a, b) / math.min(a, b) of Lua 5.1: start from a, take b when it compares greater / less (a NaN in a stays)
__device__ __forceinline__ double evm_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double evm_min(double a, double b) { return b < a ? b : a; }

// a: the detection (or the lower-indexed ground-truth box), b: the (merged) ground-truth box
__device__ __forceinline__ double evm_iou(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
  const double iw = evm_min(a2, b2) - evm_max(a0, b0) + 1.0;
  const double ih = evm_min(a3, b3) - evm_max(a1, b1) + 1.0;
  if (iw > 0.0 && ih > 0.0) {
    const double ua = (a2 - a0 + 1.0) * (a3 - a1 + 1.0) + (b2 - b0 + 1.0) * (b3 - b1 + 1.0) - iw * ih;
    return iw * ih / ua;
  }
  return 0.0;
}

__global__ __launch_bounds__(256) void eval_match_kernel(const float* __restrict__ det_boxes, const float* __restrict__ det_scores,
                                                         const int32_t* __restrict__ det_off, const float* __restrict__ gt_boxes,
                                                         const int32_t* __restrict__ gt_off, double thr, int claim_last,
                                                         int npad_cap, int m_cap, int32_t* __restrict__ order,
                                                         double* __restrict__ ov_out, int32_t* __restrict__ group_out,
                                                         uint8_t* __restrict__ ok_out, int32_t* __restrict__ gt_group,
                                                         int32_t* __restrict__ n_groups, double* __restrict__ merged_out) {
  // keys [npad_cap] u64 | merged [m_cap * 4] double | mask [m_cap * w_cap] u64 | gtc [m_cap * 4] float | first [m_cap] int
  extern __shared__ __attribute__((aligned(16))) u64 evm_lds[];
  const int w_cap = (m_cap + 63) >> 6;
  u64* keys = evm_lds;
  double* merged = reinterpret_cast<double*>(keys + npad_cap);
  u64* mask = reinterpret_cast<u64*>(merged + (size_t)m_cap * 4);
  float* gtc = reinterpret_cast<float*>(mask + (size_t)m_cap * w_cap);
  int* first = reinterpret_cast<int*>(gtc + (size_t)m_cap * 4);
  __shared__ int s_G;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int d0 = det_off[img], B = det_off[img + 1] - d0;
  const int g0 = gt_off[img], M = gt_off[img + 1] - g0;
  const int W = (M + 63) >> 6;
  int npad = 64;
  while (npad < B) npad <<= 1;                                   // <= npad_cap (the host pads the largest B the same way)

  // ---- keys, ground-truth corners ----
  for (int i = tid; i < npad; i += 256)
    keys[i] = i < B ? (((u64)evm_score_key(det_scores[d0 + i]) << 32) | (u64)(uint32_t)i) : ~0ull;
  for (int j = tid; j < M; j += 256) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(gt_boxes + (size_t)(g0 + j) * 4);
    float c0, c1, c2, c3;
    corners(b[0], b[1], b[2], b[3], c0, c1, c2, c3);
    gtc[j * 4 + 0] = c0; gtc[j * 4 + 1] = c1; gtc[j * 4 + 2] = c2; gtc[j * 4 + 3] = c3;
    first[j] = 0x7fffffff;
  }
  __syncthreads();
  // ---- bitonic sort, ascending (distinct keys but for the padding) ----
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += 256) {
        const int l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), r = l | j;
        const u64 a = keys[l], b = keys[r];
        if ((a > b) == ((l & k) == 0)) { keys[l] = b; keys[r] = a; }
      }
      __syncthreads();
    }
  // ---- the ">= thr" relation: word (i, w), bit j <=> D[i][64w + j] >= thr, D's diagonal 1 ----
  for (int t = tid; t < M * W; t += 256) {
    const int i = t / W, w = t - i * W;
    const double i0 = gtc[i * 4 + 0], i1 = gtc[i * 4 + 1], i2 = gtc[i * 4 + 2], i3 = gtc[i * 4 + 3];
    const int jn = min(64, M - w * 64);
    u64 word = 0ull;
    for (int jj = 0; jj < jn; ++jj) {
      const int j = w * 64 + jj;
      const double j0 = gtc[j * 4 + 0], j1 = gtc[j * 4 + 1], j2 = gtc[j * 4 + 2], j3 = gtc[j * 4 + 3];
      const double dv = i == j ? 1.0 : (i < j ? evm_iou(i0, i1, i2, i3, j0, j1, j2, j3) : evm_iou(j0, j1, j2, j3, i0, i1, i2, i3));
      if (dv >= thr) word |= (1ull << jj);
    }
    mask[t] = word;
  }
  __syncthreads();
  // ---- merge (wave 0) ----
  if (wid == 0) {
    u64 alive[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int left = M - w * 64;
      alive[w] = left >= 64 ? ~0ull : (left > 0 ? ((1ull << left) - 1ull) : 0ull);
    }
    int G = 0;
    while (true) {
      uint32_t best = 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        if (c < M && ((alive[k] >> lane) & 1ull)) {
          int cnt = 0;
#pragma unroll
          for (int w = 0; w < 8; ++w)
            if (w < W) cnt += __builtin_popcountll(mask[c * W + w] & alive[w]);
          const uint32_t key = ((uint32_t)cnt << 16) | (uint32_t)(0xffff - c);
          best = key > best ? key : best;
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, off, 64);
        best = o > best ? o : best;
      }
      if ((best >> 16) == 0u) break;                              // (an alive column counts itself: none is alive)
      const int col = 0xffff - (int)(best & 0xffffu);
      u64 grp[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) grp[w] = w < W ? (mask[col * W + w] & alive[w]) : 0ull;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if ((grp[k] >> lane) & 1ull) gt_group[g0 + 64 * k + lane] = G;
      if (lane < 4) {                                             // lane c: the mean of corner c, members in ascending order
        double s = 0.0;
        int n = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          u64 m = grp[k];
          while (m != 0ull) {
            const int j = 64 * k + __builtin_ctzll(m);
            m &= m - 1ull;
            s = s + (double)gtc[j * 4 + lane];
            ++n;
          }
        }
        const double mean = (double)__fdiv_rn((float)s, (float)n);
        merged[G * 4 + lane] = mean;
        merged_out[(size_t)(g0 + G) * 4 + lane] = mean;
      }
#pragma unroll
      for (int w = 0; w < 8; ++w) alive[w] &= ~grp[w];
      ++G;
    }
    if (lane == 0) { s_G = G; n_groups[img] = G; }
    for (int t = G * 4 + lane; t < M * 4; t += 64) merged_out[(size_t)g0 * 4 + t] = 0.0;   // rows past the last group
  }
  __syncthreads();
  const int G = s_G;
  // ---- match: rank d's best group, and the claims ----
  for (int d = tid; d < B; d += 256) {
    const int idx = (int)(uint32_t)keys[d];
    const f32x4 b = *reinterpret_cast<const f32x4*>(det_boxes + (size_t)(d0 + idx) * 4);
    float c0, c1, c2, c3;
    corners(b[0], b[1], b[2], b[3], c0, c1, c2, c3);
    const double a0 = c0, a1 = c1, a2 = c2, a3 = c3;
    double ovmax = 0.0;
    int jmax = -1;
    for (int j = 0; j < G; ++j) {
      const double ov = evm_iou(a0, a1, a2, a3, merged[j * 4 + 0], merged[j * 4 + 1], merged[j * 4 + 2], merged[j * 4 + 3]);
      if (ov > ovmax) { ovmax = ov; jmax = j; }
    }
    order[d0 + d] = idx;
    ov_out[d0 + d] = ovmax;
    group_out[d0 + d] = jmax;
    const int target = jmax >= 0 ? jmax : ((claim_last && G > 0) ? G - 1 : -1);
    if (target >= 0) atomicMin(&first[target], d);
  }
  __syncthreads();
  for (int d = tid; d < B; d += 256) {
    const int jmax = group_out[d0 + d];                           // (this thread's own store above)
    const int target = jmax >= 0 ? jmax : ((claim_last && G > 0) ? G - 1 : -1);
    ok_out[d0 + d] = (target >= 0 && first[target] == d) ? 1 : 0;
  }
}

size_t eval_match_lds_bytes(int max_b, int max_m, int* npad_cap, int* m_cap) {
  int npad = 64;
  while (npad < max_b) npad <<= 1;
  const int mc = max_m < 1 ? 1 : max_m;
  const int wc = (mc + 63) >> 6;
  *npad_cap = npad;
  *m_cap = mc;
  return (size_t)npad * 8 + (size_t)mc * 4 * 8 + (size_t)mc * wc * 8 + (size_t)mc * 4 * 4 + (size_t)mc * 4;
}

hipError_t launch_eval_match(const float* det_boxes, const float* det_scores, const int32_t* det_off, const float* gt_boxes,
                             const int32_t* gt_off, int n_images, int max_b, int max_m, double thr, int claim_last,
                             int32_t* order, double* ov, int32_t* group, uint8_t* ok, int32_t* gt_group, int32_t* n_groups,
                             double* merged_boxes, hipStream_t s) {
  if (max_b > EVM_MAX_DET || max_m > EVM_MAX_GT) return hipErrorInvalidValue;
  int npad_cap = 0, m_cap = 0;
  const size_t lds = eval_match_lds_bytes(max_b, max_m, &npad_cap, &m_cap);
  const void* fn = reinterpret_cast<const void*>(&eval_match_kernel);
  hipError_t e = ensure_dyn_lds(fn, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eval_match_kernel, dim3(n_images), dim3(256), lds, s, det_boxes, det_scores, det_off, gt_boxes, gt_off, thr,
                     claim_last, npad_cap, m_cap, order, ov, group, ok, gt_group, n_groups, merged_boxes);
  return hipGetLastError();
}
