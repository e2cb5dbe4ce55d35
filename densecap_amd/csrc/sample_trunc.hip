// Sampling captions with top-k / nucleus truncation (docs/SEMANTICS.md, "Truncation: top-k and nucleus") -- the
// row kernel of densecap.hip::lm_sample_n's row route.  The fused sampling epilogue of the step GEMM reduces a row to five
// floats per 32-column slot; truncation needs the whole row before the choice, so this route writes the logits to memory and
// one workgroup (256 threads) per row keeps them in dynamic LDS:
//   1. row max (fp32 compares) and log-sum-exp (double) over the candidates -- a NaN is never one;
//   2. the rank cut: a radix select over the order-preserving 32-bit keys of the raw scores, four passes of a 256-bin LDS
//      histogram (integer atomics), then an ordered count over columns for the ties at the cut (lower column first);
//   3. the nucleus: the same walk on per-bin MASSES.  A mass is q = exp(y - y_first) in double, rounded once to a multiple of
//      2^-47 and summed as a 64-bit integer: integer sums are exact, so they have no order at all -- a row's cut is the same
//      from run to run and from launch shape to launch shape without a floating-point atomic anywhere.  The rounding moves a
//      cumulative mass by at most (V+1) * 2^-48 <= 1.5e-10 (Z >= 1: the first rank has q = 1) for every row that fits the LDS;
//   4. Gumbel-max over the kept columns with the noise of the fused route (one philox4x32_10 call per run of four columns,
//      counter (v >> 2, t, r, s)), the two log-probability terms, finished / no-word handling and the LSTM point-wise update
//      with the word fed (tail_load / tail_update of common.h, as sample_step_tail_kernel).
// Every loop has a trip count fixed by V+1, the pass count or the bin count; there is no spin wait and no retry.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBins = 256;
constexpr int kNoColumn = 0x7fffffff;                 // no entry yet (elementwise.hip's kNoCol)
constexpr double kMassOne = 140737488355328.0;      // 2^47: q = 1 as a fixed-point mass; (V+1) * 2^47 < 2^63 for V+1 < 65536

// order-preserving key: a larger score has the larger key; -0 and +0 (equal values) share one
__device__ __forceinline__ uint32_t score_key(float x) {
  const uint32_t u = x == 0.f ? 0u : __builtin_bit_cast(uint32_t, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// is (key, col) at or above the cut (theta, tie)?  Ranks: key descending, the lower column first among equal keys.
__device__ __forceinline__ bool above_cut(uint32_t key, int col, uint32_t theta, int tie) {
  return key > theta || (key == theta && col <= tie);
}
__device__ __forceinline__ unsigned long long mass_of(float x, float inv_temp, float y_first) {
  const float y = __fmul_rn(x, inv_temp);
  return __double2ull_rn(exp((double)y - (double)y_first) * kMassOne);
}

struct Cut { uint32_t theta; int tie; };

__global__ __launch_bounds__(256) void sample_trunc_row_kernel(SampleTruncArgs a) {
  extern __shared__ float row[];                     // V1 raw scores
  __shared__ int hist[kBins];
  __shared__ unsigned long long mass[kBins];
  __shared__ float smx[4], sv[4];
  __shared__ int si[4], scnt[4];
  __shared__ double ssum[4];
  __shared__ uint32_t sel_digit;
  __shared__ int sel_rem, sel_tie;
  __shared__ unsigned long long sel_mrem;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V1 = a.V1, Hd = a.Hd;
  // the token-independent operands of the LSTM update are requested first: they travel while the word is being found
  TailRegs r;
  const float* g = a.gates_pre ? a.gates_pre + (size_t)m * 4 * Hd : nullptr;
  float* c_row = a.c ? a.c + (size_t)m * Hd : nullptr;
  if (g != nullptr) tail_load(r, g, c_row, Hd, 0, tid, 0);

  // ---- 1. the row into LDS; candidates, row max, log-sum-exp --------------------------------------------------------------------
  const float* x = a.logits + (size_t)m * a.ld;
  float mx = -INFINITY;
  int nc = 0;
  for (int j = tid; j < V1; j += 256) {
    const float v = x[j];
    row[j] = v;
    if (v == v) { ++nc; mx = v > mx ? v : mx; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    mx = ov > mx ? ov : mx;
    nc += __shfl_xor(nc, o, 64);
  }
  if (lane == 0) { smx[wid] = mx; scnt[wid] = nc; }
  __syncthreads();
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  nc = scnt[0] + scnt[1] + scnt[2] + scnt[3];
  const float inv_temp = a.inv_temp;
  const float y_first = __fmul_rn(mx, inv_temp);
  // No word: no candidate, or a first-ranked score that is not finite, raw or scaled (docs/SEMANTICS.md).  Uniform over the block.
  const bool none = nc == 0 || !(fabsf(mx) < INFINITY) || !(fabsf(y_first) < INFINITY);
  int tok = 0, kept = -1;
  float theta_score = NAN;
  double lp = (double)NAN, lq = (double)NAN;
  if (!none) {
    double sum = 0.0;
    for (int j = tid; j < V1; j += 256) {
      const float v = row[j];
      if (v == v) sum += exp((double)v - (double)mx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) ssum[wid] = sum;
    __syncthreads();
    const double lse = (double)mx + log(((ssum[0] + ssum[1]) + ssum[2]) + ssum[3]);

    // ---- 2. the rank cut: the key of rank K and how many of its equals stay -----------------------------------------------------
    const int K = a.top_k > 0 && a.top_k < nc ? a.top_k : nc;
    Cut cut = {0u, 0};
    int eq_keep = 0;           // ranks kept among the columns whose key equals cut.theta
    {
      uint32_t prefix = 0u;
      int rem = K;
#pragma unroll 1
      for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < V1; j += 256) {
          const float v = row[j];
          const uint32_t key = score_key(v);
          if (v == v && ((key ^ prefix) & himask) == 0u) atomicAdd(&hist[(key >> shift) & 0xffu], 1);
        }
        __syncthreads();
        int above = 0;         // entries in the bins above this thread's
        for (int b = kBins - 1; b >= 0; --b) { const int hb = hist[b]; if (b > tid) above += hb; }
        const int own = hist[tid];
        if (above < rem && rem <= above + own) { sel_digit = (uint32_t)tid; sel_rem = rem - above; }
        __syncthreads();
        prefix |= sel_digit << shift;
        rem = sel_rem;
        __syncthreads();
      }
      cut.theta = prefix;
      eq_keep = rem;
    }

    // ---- 3. the nucleus among the top-k survivors: the walk on masses -----------------------------------------------------------
    // (the tie column of the top-k cut is needed first: survivors are the ranks above it)
    auto tie_column = [&](uint32_t theta, int keep) -> int {     // the column of the keep-th lowest column with key == theta
      const int ch = (V1 + 255) / 256, j0 = tid * ch, j1 = min(V1, j0 + ch);
      int cnt = 0;
      for (int j = j0; j < j1; ++j) { const float v = row[j]; cnt += (v == v && score_key(v) == theta) ? 1 : 0; }
      hist[tid] = cnt;
      __syncthreads();
      int below = 0;
      for (int b = 0; b < kBins; ++b) { const int hb = hist[b]; if (b < tid) below += hb; }
      if (below < keep && keep <= below + cnt) {
        int seen = below, col = j0;
        for (int j = j0; j < j1; ++j) {
          const float v = row[j];
          if (v == v && score_key(v) == theta && ++seen == keep) col = j;
        }
        sel_tie = col;
      }
      __syncthreads();
      const int col = sel_tie;
      __syncthreads();
      return col;
    };
    cut.tie = tie_column(cut.theta, eq_keep);
    if (a.top_p < 1.f) {
      const Cut kcut = cut;
      uint32_t prefix = 0u;
      unsigned long long mrem = 0ull;
#pragma unroll 1
      for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        mass[tid] = 0ull;
        __syncthreads();
        for (int j = tid; j < V1; j += 256) {
          const float v = row[j];
          const uint32_t key = score_key(v);
          if (v == v && ((key ^ prefix) & himask) == 0u && above_cut(key, j, kcut.theta, kcut.tie))
            atomicAdd(&mass[(key >> shift) & 0xffu], mass_of(v, inv_temp, y_first));
        }
        __syncthreads();
        unsigned long long above = 0ull, total = 0ull;
        for (int b = kBins - 1; b >= 0; --b) { const unsigned long long hb = mass[b]; total += hb; if (b > tid) above += hb; }
        if (shift == 24) {
          // Z = total; the target: the smallest integer mass >= top_p * Z, at least one unit, at most Z
          const double want = ceil((double)a.top_p * (double)total);
          unsigned long long tgt = want >= 1.0 ? __double2ull_rz(want) : 1ull;
          mrem = tgt < total ? tgt : total;
        }
        const unsigned long long own = mass[tid];
        if (above < mrem && mrem <= above + own) { sel_digit = (uint32_t)tid; sel_mrem = mrem - above; }
        __syncthreads();
        prefix |= sel_digit << shift;
        mrem = sel_mrem;
        __syncthreads();
      }
      // every column of key `prefix` carries the same mass; the ranks among them that reach the target, lower columns first
      const unsigned long long each = mass_of(key_score(prefix), inv_temp, y_first);      // > 0: its bin's mass reached mrem >= 1
      const unsigned long long need = each > 0ull ? (mrem + each - 1ull) / each : 1ull;
      cut.theta = prefix;
      cut.tie = tie_column(prefix, (int)need);
    }

    // ---- 4. the draw over the kept columns; the kept count and mass ---------------------------------------------------------------
    float best = -INFINITY;
    int bi = kNoColumn, cnt = 0;
    double qsum = 0.0;
    const uint32_t step = (uint32_t)a.t, kr = (uint32_t)a.keys[2 * m], ks = (uint32_t)a.keys[2 * m + 1];
    for (int j4 = tid * 4; j4 < V1; j4 += 1024) {
      bool in[4];
      bool any = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j4 + q;
        const float v = j < V1 ? row[j] : NAN;
        in[q] = v == v && above_cut(score_key(v), j, cut.theta, cut.tie);
        any = any || in[q];
      }
      if (!any) continue;
      const Philox4 nz = philox4x32_10((uint32_t)j4 >> 2, step, kr, ks, a.seed_lo, a.seed_hi);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!in[q]) continue;
        const float y = __fmul_rn(row[j4 + q], inv_temp);
        const float pv = __fadd_rn(y, gumbel_from_bits(nz.w[q]));
        ++cnt;
        qsum += exp((double)y - (double)y_first);
        if (bi == kNoColumn || pv > best) { best = pv; bi = j4 + q; }       // ascending column: the first maximum stays
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != kNoColumn && (bi == kNoColumn || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
      cnt += __shfl_xor(cnt, o, 64);
      qsum += __shfl_xor(qsum, o, 64);
    }
    __syncthreads();           // ssum, scnt: read above by every thread
    if (lane == 0) { sv[wid] = best; si[wid] = bi; scnt[wid] = cnt; ssum[wid] = qsum; }
    __syncthreads();
    best = sv[0]; bi = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (si[w] != kNoColumn && (bi == kNoColumn || sv[w] > best || (sv[w] == best && si[w] < bi))) { best = sv[w]; bi = si[w]; }
    kept = scnt[0] + scnt[1] + scnt[2] + scnt[3];
    theta_score = key_score(cut.theta);
    // The word is the only value that turns device data into an address: checked before use.  A kept set always holds the first
    // rank, so a column outside [0, V1) cannot come out of the reduction; anything else is no word all the same.
    if (bi >= 0 && bi < V1) {
      tok = bi + 1;
      const float xt = row[bi];
      lp = (double)xt - lse;
      lq = ((double)__fmul_rn(xt, inv_temp) - (double)y_first) - log(((ssum[0] + ssum[1]) + ssum[2]) + ssum[3]);
    } else {
      kept = -1;
      theta_score = NAN;
    }
  }
  if (tid == 0) {
    const bool done = a.fin != nullptr && a.fin[m] != 0;
    a.seq[(size_t)m * a.T + a.tpos] = done ? 0 : tok;
    if (!done) {
      if (a.acc != nullptr) { if (tok == 0) a.acc[m] = (double)NAN; else a.acc[m] += lp; }
      if (a.acc_q != nullptr) { if (tok == 0) a.acc_q[m] = (double)NAN; else a.acc_q[m] += lq; }
      if (a.fin != nullptr && (tok == 0 || tok == a.end_tok)) a.fin[m] = 1;
    }
    if (a.kept_out != nullptr) a.kept_out[m] = kept;
    if (a.theta_out != nullptr) a.theta_out[m] = theta_score;
    if (a.lp_out != nullptr) a.lp_out[m] = lp;
    if (a.lq_out != nullptr) a.lq_out[m] = lq;
  }
  if (g == nullptr) return;
  tail_update(r, g, tok > 0 ? a.xg + (size_t)(tok - 1) * 4 * Hd : nullptr, c_row, a.h + (size_t)m * Hd, Hd, tid, 0);
}

constexpr size_t kStaticLds = 4096;      // the kernel's static LDS (histograms, reduction scratch: ~3.2 KiB), rounded up

}  // namespace

// The row kernel keeps one vocabulary row in dynamic LDS beside its static workspace: both must fit what the CURRENT device
// grants a workgroup (the rule of beam_topk_max_vocab).  Below 65,536 columns the fixed-point masses cannot overflow either.
size_t sample_trunc_max_vocab() {
  int dev = 0, lds = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
  const size_t fit = (size_t)lds > kStaticLds ? ((size_t)lds - kStaticLds) / sizeof(float) : 0;
  return fit < 65535 ? fit : 65535;
}

hipError_t launch_sample_trunc_rows(const SampleTruncArgs& a, int rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (a.V1 < 1 || (size_t)a.V1 > sample_trunc_max_vocab() || a.ld < a.V1 || a.top_k < 0 || a.top_k > a.V1 ||
      !(a.top_p > 0.f && a.top_p <= 1.f) || !(a.inv_temp > 0.f) || a.logits == nullptr || a.keys == nullptr || a.seq == nullptr ||
      (a.gates_pre != nullptr && (a.c == nullptr || a.h == nullptr || a.xg == nullptr)))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)a.V1 * sizeof(float);
  if (lds + kStaticLds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_trunc_row_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sample_trunc_row_kernel, dim3(rows), dim3(256), lds, s, a);
  return hipGetLastError();
}
