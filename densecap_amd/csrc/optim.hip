// The optimiser's kernels (docs/SEMANTICS.md, "Training step", "Gradient clipping"): Adam over a table of
// segments in one launch, the global gradient norm over the same table in two, the decode screen's operands from the fp32 lm_out_w rows, and the RPN convolution's engine layout back to OIHW.
// Built with -ffp-contract=off; every operation of the update is spelled as one rounded fp32 operation all the same.
#include "common.h"

namespace {

// The table's pointers come out of memory, so the compiler cannot know their address space: said here, the accesses are global ones
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) const f32x4 gcf32x4;

constexpr int kAdamChunk = 4096;          // elements of one segment a workgroup takes at a time: 256 lanes x 4 x 16 bytes per array

// One element of optim_updates.lua:56-84 after train.lua's grad_params:add(weight_decay, params), in TH's order of evaluation:
// mul, add(value, x), addcmul, addcdiv.  sqrt and / are the correctly rounded ones (no fast-math, no contraction).
// kScaled (gradient clipping): the gradient element is g * scale, one rounded multiply, before anything else reads it.
template <bool kScaled>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& k, float scale) {
  if (kScaled) g = __fmul_rn(g, scale);
  if (k.wd > 0.f) g = __fadd_rn(g, __fmul_rn(k.wd, p));
  m = __fadd_rn(__fmul_rn(k.b1, m), __fmul_rn(k.c1, g));
  v = __fadd_rn(__fmul_rn(k.b2, v), __fmul_rn(__fmul_rn(k.c2, g), g));
  // (sqrtf and /, not __fsqrt_rn: that intrinsic is the 1-ulp v_sqrt_f32 here; the plain calls are the correctly rounded expansions)
  p = __fadd_rn(p, __fmul_rn(k.nstep, m) / __fadd_rn(sqrtf(v), k.eps));
}

template <bool kScaled>
__device__ __forceinline__ void adam_vec(f32x4& p, const f32x4 g, f32x4& m, f32x4& v, const AdamScalars& k, float scale) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], me = m[e], ve = v[e];
    adam_one<kScaled>(pe, g[e], me, ve, k, scale);
    p[e] = pe; m[e] = me; v[e] = ve;
  }
}

template <bool kScaled>
__device__ __forceinline__ void adam_scalar_range(const AdamSeg& sg, size_t lo, size_t hi, const AdamScalars& k, float scale) {
  gfloat* const P = (gfloat*)sg.p;
  gcfloat* const G = (gcfloat*)sg.g;
  gfloat* const M = (gfloat*)sg.m;
  gfloat* const V = (gfloat*)sg.v;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
    float p = P[i], m = M[i], v = V[i];
    adam_one<kScaled>(p, G[i], m, v, k, scale);
    P[i] = p; M[i] = m; V[i] = v;
  }
}

// Work = the flat list of kAdamChunk-element chunks of all segments (seg[i].chunk0 = chunks of the segments before i; seg[nseg]
// closes the list), walked grid-stride: a 103 M-element matrix and a 4-element bias share the same workgroups.  Every element is
// read and written by exactly one lane, so the result does not depend on the grid.  Where the four pointers of a segment sit at
// the same offset from 16-byte alignment, the elements from the first aligned one on move as 16-byte accesses and what is left
// at the two ends of a chunk goes one float at a time; a segment whose pointers disagree goes one float at a time throughout.
// kScaled: the launch passes one more argument, a device pointer to the scale (grad_norm_finish_kernel's, on the same stream),
// read once per workgroup.  The unscaled instantiation has no such argument -- the pack is empty -- so that its signature, its
// kernel arguments and its code are the kernel's as it was before clipping existed.
template <bool kScaled, typename... ScalePtr>
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamSeg* __restrict__ seg, int nseg, AdamScalars k, ScalePtr... scale_dev) {
  static_assert(sizeof...(ScalePtr) == (kScaled ? 1 : 0), "the scaled launch passes the scale's address, the unscaled one nothing");
  float scale = 1.f;
  if constexpr (kScaled) scale = *(scale_dev, ...);
  const unsigned long long total = seg[nseg].chunk0;
  for (unsigned long long c = blockIdx.x; c < total; c += gridDim.x) {
    int lo_s = 0, hi_s = nseg - 1;                       // the segment of chunk c: the last one with chunk0 <= c (workgroup-uniform)
    while (lo_s < hi_s) {
      const int mid = (lo_s + hi_s + 1) >> 1;
      if (seg[mid].chunk0 <= c) lo_s = mid; else hi_s = mid - 1;
    }
    const AdamSeg sg = seg[lo_s];
    const size_t lo = (size_t)(c - sg.chunk0) * kAdamChunk;
    const size_t hi = lo + kAdamChunk < sg.n ? lo + kAdamChunk : sg.n;
    const unsigned mis = (unsigned)((uintptr_t)sg.p & 15u);
    const bool same = ((uintptr_t)sg.g & 15u) == mis && ((uintptr_t)sg.m & 15u) == mis && ((uintptr_t)sg.v & 15u) == mis && (mis & 3u) == 0;
    if (!same) { adam_scalar_range<kScaled>(sg, lo, hi, k, scale); continue; }
    const size_t head = ((16u - mis) & 15u) >> 2;        // elements in front of the segment's first aligned one
    size_t first = lo <= head ? head : head + (lo - head + 3) / 4 * 4;
    if (first > hi) first = hi;
    const size_t nvec = (hi - first) / 4;
    adam_scalar_range<kScaled>(sg, lo, first, k, scale);
    adam_scalar_range<kScaled>(sg, first + nvec * 4, hi, k, scale);
    gf32x4* const P = (gf32x4*)(sg.p + first);
    gcf32x4* const G = (gcf32x4*)(sg.g + first);
    gf32x4* const M = (gf32x4*)(sg.m + first);
    gf32x4* const V = (gf32x4*)(sg.v + first);
    // a full chunk is four vectors per lane: all sixteen loads are issued before the first update
    if (nvec == kAdamChunk / 4) {
      f32x4 p[4], g[4], m[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t i = (size_t)u * 256 + threadIdx.x;
        p[u] = P[i]; g[u] = __builtin_nontemporal_load(&G[i]); m[u] = M[i]; v[u] = V[i];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t i = (size_t)u * 256 + threadIdx.x;
        adam_vec<kScaled>(p[u], g[u], m[u], v[u], k, scale);
        P[i] = p[u]; M[i] = m[u]; V[i] = v[u];
      }
    } else {
      for (size_t i = threadIdx.x; i < nvec; i += 256) {
        f32x4 p = P[i], m = M[i], v = V[i];
        const f32x4 g = G[i];
        adam_vec<kScaled>(p, g, m, v, k, scale);
        P[i] = p; M[i] = m; V[i] = v;
      }
    }
  }
}

// ---- the global gradient norm (docs/SEMANTICS.md, "Gradient clipping") ----
// The sum of the 256 lanes' doubles in a fixed tree: six butterfly levels inside each wave (every lane of a wave ends with the
// same bits: a + b == b + a), then (w0 + w1) + (w2 + w3) through `red`, four doubles that the caller alternates between calls so
// that one barrier a call suffices.  Valid in thread 0.
__device__ __forceinline__ double block_sum256(double x, double* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[c] = the sum of (double)g * (double)g over chunk c of the table's flat chunk list (adam_multi_kernel's list and its
// segment search), one double per chunk whatever the grid.  Squares of floats are exact in double; a lane adds, in this order,
// its element in front of the chunk's first 16-byte aligned one, its up to four vectors (i = lane, lane + 256, ..: four elements
// each, in order) and its element behind the last whole vector -- at most 18 additions --, then the tree.  A segment whose g is
// not 4-byte aligned goes one float at a time (lane, lane + 256, ..: at most 16).  Only g is read.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamSeg* __restrict__ seg, int nseg, double* __restrict__ partial) {
  __shared__ double red[2][4];
  const unsigned long long total = seg[nseg].chunk0;
  unsigned it = 0;
  for (unsigned long long c = blockIdx.x; c < total; c += gridDim.x, ++it) {
    int lo_s = 0, hi_s = nseg - 1;
    while (lo_s < hi_s) {
      const int mid = (lo_s + hi_s + 1) >> 1;
      if (seg[mid].chunk0 <= c) lo_s = mid; else hi_s = mid - 1;
    }
    const AdamSeg sg = seg[lo_s];
    const size_t lo = (size_t)(c - sg.chunk0) * kAdamChunk;
    const size_t hi = lo + kAdamChunk < sg.n ? lo + kAdamChunk : sg.n;
    gcfloat* const G1 = (gcfloat*)sg.g;
    const unsigned mis = (unsigned)((uintptr_t)sg.g & 15u);
    double acc = 0.0;
    if ((mis & 3u) != 0) {
      for (size_t i = lo + threadIdx.x; i < hi; i += 256) { const double x = (double)G1[i]; acc += x * x; }
    } else {
      const size_t head = ((16u - mis) & 15u) >> 2;
      size_t first = lo <= head ? head : head + (lo - head + 3) / 4 * 4;
      if (first > hi) first = hi;
      const size_t nvec = (hi - first) / 4;
      for (size_t i = lo + threadIdx.x; i < first; i += 256) { const double x = (double)G1[i]; acc += x * x; }
      gcf32x4* const G = (gcf32x4*)(sg.g + first);
      if (nvec == kAdamChunk / 4) {                      // a full chunk: the four loads are issued before the first addition
        f32x4 g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = __builtin_nontemporal_load(&G[(size_t)u * 256 + threadIdx.x]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) { const double x = (double)g[u][e]; acc += x * x; }
      } else {
        for (size_t i = threadIdx.x; i < nvec; i += 256) {
          const f32x4 g = G[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) { const double x = (double)g[e]; acc += x * x; }
        }
      }
      for (size_t i = first + nvec * 4 + threadIdx.x; i < hi; i += 256) { const double x = (double)G1[i]; acc += x * x; }
    }
    const double sum = block_sum256(acc, red[it & 1u]);
    if (threadIdx.x == 0) partial[c] = sum;
  }
}

// One workgroup: lane l adds partial[l], partial[l + 256], .. in that order, then the tree; thread 0 writes the record.
//   norm = sqrt(sumsq); c = max_norm / (norm + 1e-6); scale = c < 1 ? (float)c : 1, all in double (correctly rounded sqrt and /);
//   a sumsq that is not finite, and max_norm = 0 (report only), give scale = 1.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, unsigned long long total,
                                                               double max_norm, GradNormRec* __restrict__ rec) {
  __shared__ double red[4];
  double acc = 0.0;
  for (unsigned long long i = threadIdx.x; i < total; i += 256) acc += partial[i];
  const double sumsq = block_sum256(acc, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(sumsq);
    const double c = max_norm / (norm + 1e-6);
    const bool finite = sumsq - sumsq == 0.0;            // false for inf and NaN
    rec->sumsq = sumsq;
    rec->norm = norm;
    rec->scale = (max_norm > 0.0 && finite && c < 1.0) ? (float)c : 1.f;
    rec->pad_ = 0.f;
  }
}

// One workgroup per row j of the screen's operands (dc_load_weights' host loop, on the device): the bf16 bits of row j of W
// (V1, Hd) -- round to nearest even, a NaN keeps its top bits with the quiet bit set -- zero columns up to Kp and zero rows up to
// V1pad; the row's 2-norm from a sum of squares in double (lane l sums columns l, l + 256, .., then a fixed tree), times 1 + 1e-9,
// square root, rounded UP to fp16 (inf past 65504; NaN stays NaN): an upper bound of the true norm, which DESIGN.md §4.1c needs.
__global__ __launch_bounds__(256) void screen_operands_kernel(const float* __restrict__ W, int V1, int Hd, int Kp,
                                                              uint16_t* __restrict__ wb, uint16_t* __restrict__ wn) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  uint16_t* const row = wb + (size_t)j * Kp;
  if (j >= V1) {
    for (int kk = threadIdx.x; kk < Kp; kk += 256) row[kk] = 0;
    if (threadIdx.x == 0) wn[j] = 0;
    return;
  }
  double ss = 0.0;
  for (int kk = threadIdx.x; kk < Kp; kk += 256) {
    uint16_t b = 0;
    if (kk < Hd) {
      const float x = W[(size_t)j * Hd + kk];
      ss += (double)x * (double)x;
      const uint32_t u = __float_as_uint(x);
      b = (u & 0x7fffffffu) > 0x7f800000u ? (uint16_t)((u >> 16) | 0x40) : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    row[kk] = b;
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double x = sqrt(red[0]) * (1.0 + 1e-9);
    const _Float16 h = (_Float16)(float)x;
    uint16_t u = __builtin_bit_cast(uint16_t, h);
    if ((double)(float)h < x) u += 1;                    // x >= 0: the next pattern up (0x7bff + 1 = inf)
    wn[j] = u;
  }
}

// launch_pack_conv3x3's (Cout, 9 Cin) form, k = tap * Cin + c, back to OIHW (conv3x3_flip_kernel's `packed` indexing)
__global__ __launch_bounds__(256) void unpack_conv3x3_kernel(const float* __restrict__ packed, int Cout, int Cin, float* __restrict__ oihw) {
  const size_t total = (size_t)Cout * Cin * 9;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int tap = (int)(i % 9);
    const size_t oc = i / 9;
    const int c = (int)(oc % Cin);
    const size_t o = oc / Cin;
    oihw[i] = packed[(o * 9 + tap) * Cin + c];
  }
}

}  // namespace

unsigned long long adam_chunks(size_t n) { return (n + kAdamChunk - 1) / kAdamChunk; }

static unsigned adam_grid(unsigned long long chunks, int grid_or_0) {
  if (grid_or_0 > 0) return (unsigned)grid_or_0;
  return (unsigned)(chunks < 2048 ? chunks : 2048);                   // eight workgroups a CU; the rest grid-stride
}

hipError_t launch_adam_multi(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, const AdamScalars& k, int grid_or_0, hipStream_t s) {
  if (nseg < 1 || seg_dev == nullptr) return hipErrorInvalidValue;
  if (chunks == 0) return hipSuccess;
  hipLaunchKernelGGL((adam_multi_kernel<false>), dim3(adam_grid(chunks, grid_or_0)), dim3(256), 0, s, seg_dev, nseg, k);
  return hipGetLastError();
}

hipError_t launch_adam_multi_scaled(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, const AdamScalars& k,
                                    const float* scale_dev, int grid_or_0, hipStream_t s) {
  if (nseg < 1 || seg_dev == nullptr || scale_dev == nullptr) return hipErrorInvalidValue;
  if (chunks == 0) return hipSuccess;
  hipLaunchKernelGGL((adam_multi_kernel<true, const float*>), dim3(adam_grid(chunks, grid_or_0)), dim3(256), 0, s, seg_dev, nseg, k, scale_dev);
  return hipGetLastError();
}

hipError_t launch_grad_sumsq(const AdamSeg* seg_dev, int nseg, unsigned long long chunks, double* partial, int grid_or_0, hipStream_t s) {
  if (nseg < 1 || seg_dev == nullptr || partial == nullptr) return hipErrorInvalidValue;
  if (chunks == 0) return hipSuccess;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(adam_grid(chunks, grid_or_0)), dim3(256), 0, s, seg_dev, nseg, partial);
  return hipGetLastError();
}

hipError_t launch_grad_norm_finish(const double* partial, unsigned long long total, double max_norm, GradNormRec* rec, hipStream_t s) {
  if (partial == nullptr || rec == nullptr || !(max_norm >= 0.0)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, partial, total, max_norm, rec);
  return hipGetLastError();
}

hipError_t launch_screen_operands(const float* W, int V1, int Hd, int V1pad, int Kp, uint16_t* wb, uint16_t* wn, hipStream_t s) {
  if (V1 < 1 || Hd < 1 || V1pad < V1 || Kp < Hd) return hipErrorInvalidValue;
  hipLaunchKernelGGL(screen_operands_kernel, dim3(V1pad), dim3(256), 0, s, W, V1, Hd, Kp, wb, wn);
  return hipGetLastError();
}

hipError_t launch_unpack_conv3x3(const float* packed, float* oihw, int Cout, int Cin, hipStream_t s) {
  if (Cout < 1 || Cin < 1) return hipErrorInvalidValue;
  const size_t total = (size_t)Cout * Cin * 9;
  const size_t g = (total + 255) / 256;
  hipLaunchKernelGGL(unpack_conv3x3_kernel, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, s, packed, Cout, Cin, oihw);
  return hipGetLastError();
}
