// Box pipeline of the LocalizationLayer test path (gfx950): anchors, box transform, clipping,
// fused RPN decode, greedy NMS (rank sort + IoU bit-mask + chunked wavefront scan), gathers.
//
// Bit-exactness: every fp32 expression that feeds an integer decision (valid flags, NMS picks)
// is written with __f*_rn intrinsics in the reference's operation order (no FMA contraction),
// so that, fed the oracle's inputs, the picks are identical to box_utils.nms
// (densecap/box_utils.lua:154-256).
#include <algorithm>
#include <type_traits>

#include "common.h"

// every fp32 op rounds once, in source order (integer decisions depend on it)
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void make_anchors_kernel(float* __restrict__ out, int h, int w, float x0, float y0, float sx, float sy,
                                    const float* __restrict__ anchors, int k) {
  const int total = k * h * w;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  const int a = b / (h * w), rem = b - a * h * w, y = rem / w, x = rem - y * w;
  f32x4 v;
  v[0] = __fadd_rn(__fmul_rn((float)x, sx), x0);   // MakeAnchors.lua:44-47
  v[1] = __fadd_rn(__fmul_rn((float)y, sy), y0);
  v[2] = anchors[a];
  v[3] = anchors[k + a];
  *reinterpret_cast<f32x4*>(out + (size_t)b * 4) = v;
}

__global__ void apply_box_transform_kernel(const float* __restrict__ boxes, const float* __restrict__ trans,
                                           float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
  const f32x4 t = *reinterpret_cast<const f32x4*>(trans + (size_t)i * 4);
  f32x4 o;
  o[0] = __fadd_rn(__fmul_rn(t[0], b[2]), b[0]);   // ApplyBoxTransform.lua:85-88
  o[1] = __fadd_rn(__fmul_rn(t[1], b[3]), b[1]);
  o[2] = __fmul_rn(th_expf(t[2]), b[2]);
  o[3] = __fmul_rn(th_expf(t[3]), b[3]);
  *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = o;
}

__device__ __forceinline__ bool clip_one(const f32x4& b, float x_min, float y_min, float x_max, float y_max,
                                         f32x4& o) {
  float x1, y1, x2, y2;
  corners(b[0], b[1], b[2], b[3], x1, y1, x2, y2);
  x1 = clampf(x1, x_min, x_max - 1.f);               // box_utils.lua:505-508
  y1 = clampf(y1, y_min, y_max - 1.f);
  x2 = clampf(x2, x_min + 1.f, x_max);
  y2 = clampf(y2, y_min + 1.f, y_max);
  o[0] = __fdiv_rn(__fadd_rn(x1, x2), 2.f);          // x1y1x2y2_to_xcycwh (box_utils.lua:400-403)
  o[1] = __fdiv_rn(__fadd_rn(y1, y2), 2.f);
  o[2] = __fsub_rn(x2, x1);
  o[3] = __fsub_rn(y2, y1);
  return (x2 > x1) && (y2 > y1);
}

__global__ void clip_boxes_kernel(const float* __restrict__ boxes, float* __restrict__ clipped,
                                  uint8_t* __restrict__ valid, int n, float x_min, float y_min, float x_max,
                                  float y_max) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
  f32x4 o;
  const bool v = clip_one(b, x_min, y_min, x_max, y_max, o);
  *reinterpret_cast<f32x4*>(clipped + (size_t)i * 4) = o;
  if (valid) valid[i] = v ? 1 : 0;
}

__global__ void xcycwh_to_x1y1x2y2_kernel(const float* __restrict__ boxes, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
  float o0, o1, o2, o3;
  corners(b[0], b[1], b[2], b[3], o0, o1, o2, o3);
  *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = f32x4{o0, o1, o2, o3};
}

// nn.BoxIoU (BoxIoU.lua:40-73).  convention 0 = the module as written ((w-1)/2 corners, area w*h, no +1);
// 1 = box_utils.nms inline form ((w-1)/2 corners, +1 on every extent; box_utils.lua:178-181,219-227);
// 2 = legacy_half_w: the module's original converter (BoxIoU.lua:15-37, commented out there): corners xc -/+ w/2,
//     area w*h, no +1 -- the convention test/BoxIoU_test.lua:13-94 pins.
__device__ __forceinline__ void corners_half_w(float xc, float yc, float w, float h, float& x0, float& y0, float& x1,
                                               float& y1) {
  const float hw = __fdiv_rn(w, 2.f), hh = __fdiv_rn(h, 2.f);
  x0 = __fadd_rn(__fmul_rn(hw, -1.f), xc); x1 = __fadd_rn(hw, xc);
  y0 = __fadd_rn(__fmul_rn(hh, -1.f), yc); y1 = __fadd_rn(hh, yc);
}
__global__ void box_iou_kernel(const float* __restrict__ b1, const float* __restrict__ b2, float* __restrict__ out,
                               int B1, int B2, int convention) {
  const size_t total = (size_t)B1 * B2;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / B2), j = (int)(idx % B2);
    const f32x4 p = *reinterpret_cast<const f32x4*>(b1 + (size_t)i * 4);
    const f32x4 q = *reinterpret_cast<const f32x4*>(b2 + (size_t)j * 4);
    float px1, py1, px2, py2, qx1, qy1, qx2, qy2;
    if (convention == 2) {
      corners_half_w(p[0], p[1], p[2], p[3], px1, py1, px2, py2);
      corners_half_w(q[0], q[1], q[2], q[3], qx1, qy1, qx2, qy2);
    } else {
      corners(p[0], p[1], p[2], p[3], px1, py1, px2, py2);
      corners(q[0], q[1], q[2], q[3], qx1, qy1, qx2, qy2);
    }
    const bool plus1 = convention == 1;
    const float one = plus1 ? 1.f : 0.f;
    const float a1 = plus1 ? __fmul_rn(__fadd_rn(__fsub_rn(px2, px1), 1.f), __fadd_rn(__fsub_rn(py2, py1), 1.f))
                           : __fmul_rn(p[2], p[3]);
    const float a2 = plus1 ? __fmul_rn(__fadd_rn(__fsub_rn(qx2, qx1), 1.f), __fadd_rn(__fsub_rn(qy2, qy1), 1.f))
                           : __fmul_rn(q[2], q[3]);
    const float x0 = fmaxf(px1, qx1), y0 = fmaxf(py1, qy1), x1 = fminf(px2, qx2), y1 = fminf(py2, qy2);
    float w = __fadd_rn(__fsub_rn(x1, x0), one), h = __fadd_rn(__fsub_rn(y1, y0), one);
    w = w > 0.f ? w : 0.f;
    h = h > 0.f ? h : 0.f;
    const float inter = __fmul_rn(w, h);
    out[idx] = __fdiv_rn(inter, __fsub_rn(__fadd_rn(a1, a2), inter));
  }
}

// Fused MakeAnchors + ReshapeBoxFeatures + ApplyBoxTransform + clip_boxes + corners + p(pos)
// (LocalizationLayer.lua:265-308).  heads: (h,w,6k) channels-last, box channels a*4+d, then
// score channels 4k + a*2 + d.  Row b = a*h*w + y*w + x (ReshapeBoxFeatures.lua:24-33).
// blockIdx.y = image of a group: every per-image tensor is `total` rows further on (heads: h*w pixels further on).
__global__ void rpn_decode_kernel(const float* __restrict__ heads, int h, int w, int k,
                                  const float* __restrict__ anchors, float x0, float y0, float sx, float sy,
                                  float img_h, float img_w, float* __restrict__ boxes, float* __restrict__ anc_out,
                                  float* __restrict__ trans_out, float* __restrict__ xyxy, float* __restrict__ p_out,
                                  uint8_t* __restrict__ valid, int clip) {
  const int total = k * h * w;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  {
    const size_t img = blockIdx.y;
    heads += img * (size_t)h * w * 6 * k;
    if (boxes) boxes += img * total * 4;
    if (anc_out) anc_out += img * total * 4;
    if (trans_out) trans_out += img * total * 4;
    if (xyxy) xyxy += img * total * 4;
    if (p_out) p_out += img * total;
    if (valid) valid += img * total;
  }
  const int a = b / (h * w), rem = b - a * h * w, y = rem / w, x = rem - y * w;
  const float* px = heads + (size_t)rem * (6 * k);
  const f32x4 t = *reinterpret_cast<const f32x4*>(px + a * 4);
  const float s1 = px[4 * k + a * 2], s2 = px[4 * k + a * 2 + 1];
  const float xa = __fadd_rn(__fmul_rn((float)x, sx), x0);
  const float ya = __fadd_rn(__fmul_rn((float)y, sy), y0);
  const float wa = anchors[a], ha = anchors[k + a];
  f32x4 bx;
  bx[0] = __fadd_rn(__fmul_rn(t[0], wa), xa);
  bx[1] = __fadd_rn(__fmul_rn(t[1], ha), ya);
  bx[2] = __fmul_rn(th_expf(t[2]), wa);
  bx[3] = __fmul_rn(th_expf(t[3]), ha);
  // "Maybe clip boxes to image boundary" (LocalizationLayer.lua:272-300): with test_clip_boxes = false the boxes stay as
  // transformed and every row is a candidate
  f32x4 cb = bx;
  const bool v = clip ? clip_one(bx, 1.f, 1.f, img_w, img_h, cb) : true;
  if (boxes) *reinterpret_cast<f32x4*>(boxes + (size_t)b * 4) = cb;
  if (anc_out) *reinterpret_cast<f32x4*>(anc_out + (size_t)b * 4) = f32x4{xa, ya, wa, ha};
  if (trans_out) *reinterpret_cast<f32x4*>(trans_out + (size_t)b * 4) = t;
  if (xyxy) {
    float c0, c1, c2, c3;
    corners(cb[0], cb[1], cb[2], cb[3], c0, c1, c2, c3);
    *reinterpret_cast<f32x4*>(xyxy + (size_t)b * 4) = f32x4{c0, c1, c2, c3};
  }
  if (p_out) {
    const float e1 = th_expf(s1), e2 = th_expf(s2);
    p_out[b] = __fmul_rn(__fdiv_rn(1.f, __fadd_rn(e1, e2)), e1);   // pow(-1):cmul (LocalizationLayer.lua:308)
  }
  if (valid) valid[b] = v ? 1 : 0;
}

// ---------------------------------------------------------------------------------------
// NMS (box_utils.nms, box_utils.lua:154-256)
//
// Stage 1 -- sort by (valid desc, score desc, index asc): one MSD bucket pass on the top 16 bits of an
// order-preserving key (histogram -> exclusive scan -> scatter) followed by an exact in-bucket rank
// (compare against the few members of the same bucket).  Deterministic regardless of atomic order, and
// exactly the oracle's tie rule.
// Stage 2/3 -- window by window over the sorted list (4096 boxes, then 32768 at a time): the whole GPU
// computes (a) which window candidates are already suppressed by earlier picks and (b) the window's
// upper-triangular suppression bit-mask; one workgroup then scans the window 64 candidates per step.
// Kernels of later windows exit at once when the pick budget is met (`done` flag), so the common case
// (1000 picks found within the first ~2.3k of 20,520 boxes) touches ~1/25 of the full IoU triangle.
// ---------------------------------------------------------------------------------------
constexpr int NMS_BUCKET_BITS = 16;
constexpr int NMS_BUCKETS = 1 << NMS_BUCKET_BITS;
constexpr int NMS_WIN0 = 4096;

__device__ __forceinline__ uint32_t sort_key(float s, bool valid) {
  if (!valid) return 0xffffffffu;
  if (s != s) return 0u;                 // NaN ranks above every number, as in TH's sort (GT_OR_NAN): picked first
  if (s == 0.f) s = 0.f;                 // -0 == +0 (ties broken by index, as a float compare would)
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // larger float -> larger u
  return ~u;                                          // descending score -> ascending key
}

// Wave-aggregated histogram: RPN scores cluster in a few hundred buckets, so per-lane atomics on the
// same address would serialise (237 us measured); instead each wave walks its distinct bucket values
// (readfirstlane + ballot) and issues ONE atomic per (wave, bucket).
__global__ __launch_bounds__(256) void nms_hist_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ valid,
                                                       int n_cap, const int32_t* __restrict__ n_dev,
                                                       uint32_t* __restrict__ keys, int32_t* __restrict__ hist,
                                                       int32_t* __restrict__ nvalid) {
  const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < n;
  const bool v = in && (valid == nullptr || valid[i] != 0);
  const uint32_t k = in ? sort_key(scores[i], v) : 0u;
  if (in) keys[i] = k;
  const u64 vb = __ballot(v);
  if (lane == 0 && vb) atomicAdd(nvalid, __builtin_popcountll(vb));
  const uint32_t b = k >> (32 - NMS_BUCKET_BITS);
  u64 todo = __ballot(in);
  int my_cnt = 0;                        // > 0 only on the first lane of each distinct bucket value
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const uint32_t b0 = __builtin_amdgcn_readlane((int)b, leader);
    const u64 same = __ballot(in && b == b0) & todo;
    if (lane == leader) my_cnt = __builtin_popcountll(same);
    todo &= ~same;
  }
  if (my_cnt) atomicAdd(&hist[b], my_cnt);
}

// exclusive scan of the histogram by one workgroup of 16 waves: wave w owns the contiguous bins [w*C, (w+1)*C),
// C = NMS_BUCKETS/16, and walks them in coalesced 1 KiB rows (lane l takes bins 4l..4l+3 of a row); a row is scanned with
// wave shuffles, rows chain through a running base; the 16 wave totals meet in LDS.  (One thread per 64 consecutive bins
// made every load touch 64 cache lines: 19 us for 512 KiB of traffic.)
__global__ __launch_bounds__(1024) void nms_bucket_scan_kernel(const int32_t* __restrict__ hist,
                                                                int32_t* __restrict__ off) {
  constexpr int C = NMS_BUCKETS / 16, ROWS = C / 256;
  __shared__ int wtot[16];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const int32_t* src = hist + wid * C;
  i32x4 v[ROWS];
  int excl[ROWS];                                    // exclusive prefix of this lane's 4 bins inside the wave's chunk
  int run = 0;
#pragma unroll
  for (int rw = 0; rw < ROWS; ++rw) {
    v[rw] = *reinterpret_cast<const i32x4*>(src + rw * 256 + lane * 4);
    const int s4 = v[rw][0] + v[rw][1] + v[rw][2] + v[rw][3];
    int incl = s4;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    excl[rw] = run + incl - s4;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) wtot[wid] = run;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wid; ++w) base += wtot[w];
#pragma unroll
  for (int rw = 0; rw < ROWS; ++rw) {
    i32x4 o4;
    int r = base + excl[rw];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o4[e] = r; r += v[rw][e]; }
    *reinterpret_cast<i32x4*>(off + wid * C + rw * 256 + lane * 4) = o4;
  }
}

// bucket scatter with one cursor atomic per (wave, bucket); keeps (key, index) pairs contiguous per bucket
__global__ __launch_bounds__(256) void nms_bucket_scatter_kernel(const uint32_t* __restrict__ keys, int n_cap,
                                                                 const int32_t* __restrict__ n_dev,
                                                                 const int32_t* __restrict__ off,
                                                                 int32_t* __restrict__ cursor,
                                                                 uint32_t* __restrict__ tmp_key,
                                                                 int32_t* __restrict__ tmp_idx) {
  const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < n;
  const uint32_t k = in ? keys[i] : 0u;
  const uint32_t b = k >> (32 - NMS_BUCKET_BITS);
  u64 todo = __ballot(in);
  int my_leader = lane, my_rank = 0, my_cnt = 0;
  while (todo) {                         // scalar walk over the wave's distinct buckets; no memory traffic
    const int leader = __builtin_ctzll(todo);
    const uint32_t b0 = __builtin_amdgcn_readlane((int)b, leader);
    const u64 same = __ballot(in && b == b0) & todo;
    if (in && b == b0 && ((same >> lane) & 1ull)) {
      my_leader = leader;
      my_rank = __builtin_popcountll(same & ((1ull << lane) - 1ull));
      my_cnt = __builtin_popcountll(same);
    }
    todo &= ~same;
  }
  int base = 0;
  if (in && lane == my_leader) base = off[b] + atomicAdd(&cursor[b], my_cnt);   // all leaders at once
  base = __shfl(base, my_leader, 64);
  const int slot = base + my_rank;
  if (in) { tmp_key[slot] = k; tmp_idx[slot] = i; }
}

// exact position inside the bucket (sequential sweep over the bucket's contiguous (key, index) pairs),
// then gather the box into sorted order
__global__ void nms_bucket_rank_kernel(const uint32_t* __restrict__ tmp_key, const int32_t* __restrict__ tmp_idx,
                                       const float* __restrict__ boxes, int n_cap, const int32_t* __restrict__ n_dev,
                                       const int32_t* __restrict__ off, const int32_t* __restrict__ hist,
                                       int32_t* __restrict__ order, float* __restrict__ sboxes,
                                       float* __restrict__ sarea) {
  const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int i = tmp_idx[s];
  const uint32_t k = tmp_key[s];
  const int b = (int)(k >> (32 - NMS_BUCKET_BITS));
  const int lo = off[b], cnt = hist[b];
  // keys only (16-byte loads once aligned); the index is read for equal keys alone (ties -> lower index first)
  int r = 0;
  auto step = [&](uint32_t kj, int q) {
    r += kj < k ? 1 : 0;
    if (kj == k) r += tmp_idx[lo + q] < i ? 1 : 0;
  };
  int q = 0;
  for (; q < cnt && ((lo + q) & 3); ++q) step(tmp_key[lo + q], q);
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  for (; q + 4 <= cnt; q += 4) {
    const u32x4 kk = *reinterpret_cast<const u32x4*>(tmp_key + lo + q);
#pragma unroll
    for (int e = 0; e < 4; ++e) step(kk[e], q + e);
  }
  for (; q < cnt; ++q) step(tmp_key[lo + q], q);
  const int pos = lo + r;
  const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4);
  order[pos] = i;
  *reinterpret_cast<f32x4*>(sboxes + (size_t)pos * 4) = bx;
  // box_utils.lua:178-181: area = (x2-x1+1) * (y2-y1+1)
  sarea[pos] = __fmul_rn(__fadd_rn(__fsub_rn(bx[2], bx[0]), 1.f), __fadd_rn(__fsub_rn(bx[3], bx[1]), 1.f));
}

// IoU test of box_utils.lua:219-227,241 (j = candidate, i = picked box): true <=> candidate is suppressed
__device__ __forceinline__ bool nms_suppresses(const f32x4& bi, float ai, float jx1, float jy1, float jx2, float jy2,
                                               float aj, float thresh) {
  const float xx1 = fmaxf(jx1, bi[0]);
  const float yy1 = fmaxf(jy1, bi[1]);
  const float xx2 = fminf(jx2, bi[2]);
  const float yy2 = fminf(jy2, bi[3]);
  float w = __fadd_rn(__fsub_rn(xx2, xx1), 1.f);
  float h = __fadd_rn(__fsub_rn(yy2, yy1), 1.f);
  w = w > 0.f ? w : 0.f;
  h = h > 0.f ? h : 0.f;
  const float inter = __fmul_rn(w, h);
  const float uni = __fsub_rn(__fadd_rn(aj, ai), inter);
  const float iou = __fdiv_rn(inter, uni);
  return !(iou <= thresh);
}

struct NmsState { int32_t count; int32_t done; };

// (a) candidates of window [r0,r1) vs the picks made in earlier windows.  block = (chunk, split):
// lane = candidate, the 4 waves x gridDim.y splits stride over the picks; one atomicOr per wave.
__global__ __launch_bounds__(256) void nms_cross_kernel(const float* __restrict__ sboxes,
                                                        const float* __restrict__ sarea,
                                                        const int32_t* __restrict__ nvalid,
                                                        const NmsState* __restrict__ st,
                                                        const int32_t* __restrict__ pick_pos, int r0, int r1,
                                                        float thresh, u64* __restrict__ removed0) {
  const int n = *nvalid;
  if (st->done || r0 >= n) return;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int chunk = (r0 >> 6) + blockIdx.x;
  const int j = chunk * 64 + lane;
  if (chunk * 64 >= min(r1, n)) return;
  const int npick = st->count;
  const bool live = j < n;
  f32x4 bj = {0.f, 0.f, 0.f, 0.f};
  float aj = 0.f;
  if (live) { bj = *reinterpret_cast<const f32x4*>(sboxes + (size_t)j * 4); aj = sarea[j]; }
  bool sup = false;
  const int stride = 4 * gridDim.y;
  for (int p = blockIdx.y * 4 + q; p < npick; p += stride) {
    const int pp = pick_pos[p];                       // wave-uniform
    const f32x4 bi = *reinterpret_cast<const f32x4*>(sboxes + (size_t)pp * 4);
    sup = sup || nms_suppresses(bi, sarea[pp], bj[0], bj[1], bj[2], bj[3], aj, thresh);
  }
  const u64 bal = __ballot(sup && live);
  if (lane == 0 && bal) atomicOr(&removed0[chunk], bal);
}

// (b) intra-window upper-triangular bit mask.  wave q of block (cg, rc): rows of chunk rc (window
// relative) against column chunk cg*4+q; bit j set <=> row suppresses column j, j > row.  With `nearband` (windows the band
// scan takes) also the three blocks below the diagonal and the whole diagonal block, packed four words a row.
__global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ sboxes, const float* __restrict__ sarea,
                                                       const int32_t* __restrict__ nvalid,
                                                       const NmsState* __restrict__ st, int r0, int r1, float thresh,
                                                       int wwords, u64* __restrict__ mask, u64* __restrict__ nearband) {
  const int n = min(*nvalid, r1);
  if (st->done || r0 >= n) return;
  const int rc = blockIdx.y, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cc = blockIdx.x * 4 + q;
  if (r0 + rc * 64 >= n) return;
  __shared__ float cb[4][64][5];
  const int cj = r0 + cc * 64 + lane;
  if (cj < n) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(sboxes + (size_t)cj * 4);
    cb[q][lane][0] = b[0]; cb[q][lane][1] = b[1]; cb[q][lane][2] = b[2]; cb[q][lane][3] = b[3];
    cb[q][lane][4] = sarea[cj];
  }
  __syncthreads();
  // blocks on and above the diagonal, and (round 6) the three just below it: nms_scan_band_kernel reads those as "which rows of
  // the previous three chunks suppress this row" (the test is symmetric in its two boxes)
  if (cc < rc - 3 || r0 + cc * 64 >= n) return;
  const int row = r0 + rc * 64 + lane;
  if (row >= n) return;
  const f32x4 bi = *reinterpret_cast<const f32x4*>(sboxes + (size_t)row * 4);
  const float ai = sarea[row];
  const int jn = min(64, n - (r0 + cc * 64));
  // (the diagonal block is computed whole when the band scan will read it: its lower triangle -- "which EARLIER rows of my own
  // chunk suppress me", the transpose of the upper one, the test being symmetric -- lets that kernel resolve a chunk by
  // fixed-point sweeps instead of one scalar step per pick)
  const bool whole_diag = nearband != nullptr && cc == rc;
  u64 word = 0;
  for (int j = (cc == rc && !whole_diag ? lane + 1 : 0); j < jn; ++j)
    if (j != lane || cc != rc)
      if (nms_suppresses(bi, ai, cb[q][j][0], cb[q][j][1], cb[q][j][2], cb[q][j][3], cb[q][j][4], thresh))
        word |= (1ull << j);
  // the words nms_scan_band_kernel keeps in LDS, packed (32 bytes a row: one contiguous 128 KiB read instead of 4096 lines)
  if (nearband != nullptr && cc <= rc) nearband[(size_t)(row - r0) * 4 + (rc - cc)] = word;
  if (whole_diag) word &= ~((2ull << lane) - 1ull);          // the window mask keeps the upper triangle only
  mask[(size_t)(row - r0) * wwords + cc] = word;
}

// (c) greedy scan of one window, 64 candidates (one mask word) per step.  Wave 0 resolves the
// intra-chunk dependencies in the scalar unit (readlane on the diagonal words); all four waves then
// OR the picked rows into the LDS-resident `removed` set of the window's later chunks.
__global__ __launch_bounds__(256) void nms_scan_kernel(const u64* __restrict__ mask, int wwords,
                                                       const int32_t* __restrict__ nvalid,
                                                       const int32_t* __restrict__ order, int r0, int r1,
                                                       int max_boxes, const u64* __restrict__ removed0,
                                                       int32_t* __restrict__ picks, int32_t* __restrict__ pick_pos,
                                                       NmsState* __restrict__ st, int32_t* __restrict__ count_out) {
  __shared__ u64 removed[512];
  __shared__ int s_cnt, s_npick;
  __shared__ int s_rows[64];
  const int ntot = *nvalid;
  if (st->done) return;
  const int tid = threadIdx.x, lane = tid & 63;
  if (r0 >= ntot) {                       // nothing left: close the run
    if (tid == 0) { st->done = 1; *count_out = st->count; }
    return;
  }
  const int n = min(ntot, r1);
  const int nw = (n - r0 + 63) >> 6;      // chunks in this window
  for (int v = tid; v < nw; v += 256) removed[v] = removed0[(r0 >> 6) + v];
  if (tid == 0) { s_cnt = st->count; s_npick = 0; }
  __syncthreads();
  bool full = false;
  // the diagonal word of the NEXT chunk is requested one step ahead (its address does not depend on picks)
  u64 diag_next = (tid < 64 && r0 + lane < n) ? mask[(size_t)lane * wwords] : 0ull;
  for (int w = 0; w < nw; ++w) {
    if (tid < 64) {
      const int row = r0 + w * 64 + lane;
      const u64 diag = diag_next;
      if (w + 1 < nw) {
        const int nrow = row + 64;
        diag_next = nrow < n ? mask[(size_t)(nrow - r0) * wwords + w + 1] : 0ull;
      }
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
      u64 alive = ~removed[w];
      if (n - (r0 + w * 64) < 64) alive &= (1ull << (n - (r0 + w * 64))) - 1ull;
      const unsigned alo = __builtin_amdgcn_readfirstlane((unsigned)alive);
      const unsigned ahi = __builtin_amdgcn_readfirstlane((unsigned)(alive >> 32));
      u64 al = ((u64)ahi << 32) | alo;
      u64 rem = al;
      while (rem) {
        const int b = __builtin_ctzll(rem);
        const u64 dd = ((u64)(unsigned)__builtin_amdgcn_readlane((int)dhi, b) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)dlo, b);
        al &= ~dd;
        rem = al & ~((2ull << b) - 1ull);
      }
      const int cnt = s_cnt;
      if (max_boxes >= 0) {
        const int room = max_boxes - cnt;
        while (__builtin_popcountll(al) > room) al &= ~(1ull << (63 - __builtin_clzll(al)));
      }
      if ((al >> lane) & 1ull) {
        const int pos = __builtin_popcountll(al & ((1ull << lane) - 1ull));
        pick_pos[cnt + pos] = row;           // original indices are written once, after the loop
        s_rows[pos] = row - r0;
      }
      if (lane == 0) {
        s_npick = __builtin_popcountll(al);
        s_cnt = cnt + __builtin_popcountll(al);
      }
    }
    __syncthreads();
    const int npick = s_npick;
    if (max_boxes >= 0 && s_cnt >= max_boxes) { full = true; break; }
    if (npick > 0) {
      // (pick, later word) pairs spread over all 256 threads: independent loads, LDS atomic OR
      const int nlater = nw - (w + 1);
      const int total = npick * nlater;
      // all loads of a batch are issued before the first OR: one L2 round trip per 8 items instead of one per item
      for (int t0 = tid; t0 < total; t0 += 256 * 8) {
        u64 m[8];
        int vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = t0 + u * 256;
          const bool in = t < total;
          const int p = in ? t / nlater : 0;
          vv[u] = w + 1 + (in ? t - p * nlater : 0);
          m[u] = in ? mask[(size_t)s_rows[p] * wwords + vv[u]] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (m[u]) atomicOr(&removed[vv[u]], m[u]);
      }
    }
    __syncthreads();
  }
  // picks of this window: sorted position -> original index, off the per-chunk critical path
  __syncthreads();
  const int c_begin = st->count, c_end = s_cnt;
  for (int i = c_begin + tid; i < c_end; i += 256) picks[i] = order[pick_pos[i]];
  __syncthreads();
  if (tid == 0) {
    st->count = s_cnt;
    if (full || n >= ntot) { st->done = 1; *count_out = s_cnt; }
  }
}

// (c') the same greedy scan for a window of <= NMS_BAND_ROWS rows, without a memory round trip per chunk (round 6).
// nms_scan_kernel above pays, per 64-row chunk, one scalar readlane step per pick (~120 cycles each) and one memory round trip:
// the picks of chunk w fetch their mask rows (written by workgroups on all eight XCDs, so they come from the Infinity Cache)
// before chunk w+1 can be resolved -- 1.4 us x 64 chunks = 90 us for the RPN list.  Here:
//  * everything the NEXT three chunks need is in LDS before the loop starts, at addresses that do not depend on the picks.
//    nms_mask_kernel packs four words per row side by side (`nearband`, 32 bytes a row, one contiguous 128 KiB read): the
//    row's WHOLE diagonal word (plane 0 of `band`) and the words of the three chunks BEFORE the row's own (planes 1..3) -- the
//    blocks just below the diagonal, which that kernel now computes too.  The IoU test is symmetric in its two boxes, so bit p
//    of word c - k of a row of chunk c says "row p of chunk c - k, if picked, suppresses me".
//  * wave 0 resolves chunk after chunk out of LDS.  A row is dead if an earlier window or a pick four or more chunks back
//    removed it (`removed`) or if its three sub-diagonal words meet the pick sets of the last three chunks (three ANDs and a
//    ballot -- no reduction over picks, no atomics).  Inside the chunk the greedy choice is the one solution of a triangular
//    system, found by fixed-point sweeps over the lower triangle of the diagonal block (a ballot per sweep, 3-6 sweeps).
//  * waves 1..3 take the chunks in turn (chunk p: wave 1 + p % 3): as soon as chunk p is published they fetch the FAR words
//    (chunk p+4 onwards; lane = word, so a pick's words are one contiguous run) of ALL its picks in one round trip (16 / 32 /
//    64 loads in flight, addresses past the pick count clamped so that no load hides behind a branch) and OR them into
//    `removed`; wave 0 looks at that helper's progress flag only before chunk p+4.
//  * no barrier inside the loop: the hand-offs are LDS flags (the LDS operations of a wave execute in order, so what was
//    written before a flag is visible to whoever sees the flag).
// RPN list (20,520 boxes, 1000 picks): 90 -> 30 us; final NMS (1000 boxes): 27 -> 14 us (tools/nms_trace.sh).  Same picks as
// nms_scan_kernel, bit for bit (tests/test_gpu_ops.py::test_nms_band_scan_equals_the_chunk_scan).
constexpr int NMS_BAND_ROWS = 4096, NMS_BAND_WORDS = 4;
constexpr size_t NMS_BAND_LDS = (size_t)NMS_BAND_ROWS * NMS_BAND_WORDS * sizeof(u64);
#define NMS_COMPILER_FENCE() asm volatile("" ::: "memory")
__global__ __launch_bounds__(256) void nms_scan_band_kernel(const u64* __restrict__ mask, int wwords,
                                                            const u64* __restrict__ nearband,
                                                            const int32_t* __restrict__ nvalid,
                                                            const int32_t* __restrict__ order, int r0, int r1,
                                                            int max_boxes, const u64* __restrict__ removed0,
                                                            int32_t* __restrict__ picks, int32_t* __restrict__ pick_pos,
                                                            NmsState* __restrict__ st, int32_t* __restrict__ count_out,
                                                            uint32_t* __restrict__ fault) {
  extern __shared__ __attribute__((aligned(16))) u64 band[];       // [NMS_BAND_WORDS][NMS_BAND_ROWS]
  __shared__ u64 removed[NMS_BAND_ROWS / 64];
  __shared__ int s_np[4];
  __shared__ int s_rows[4][64];           // ring of four chunks: picks (window-relative rows) of chunk w in slot w & 3
  __shared__ int s_published;             // chunks resolved by wave 0; kStop once wave 0 is through
  __shared__ int s_applied[3];            // chunks whose far words helper wave h has folded into `removed`
  // (flags are read / written as relaxed workgroup-scope atomics: plain ds_read / ds_write, never cached in a register;
  // `volatile` would turn every access into a flat load behind vmcnt(0) and serialise the helpers' global loads)
  auto flag_load = [](int* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  auto flag_store = [](int* f, int v) { __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  __shared__ int s_result[2];             // {count, full}
  constexpr int kStop = 1 << 30;
  // Every wait on another wave is BOUNDED (as the stream-K owners' waits are): a flag that does not arrive within ~2^20 sleeps
  // (tens of milliseconds; a hand-off normally takes a microsecond) sets the sticky fault word -- the host then fails the call
  // and falls back to the chunk scan instead of delivering a list built on a missing hand-off -- and the wave moves on.
  constexpr unsigned kSpinLimit = 1u << 20;
  auto give_up = [&]() { if (fault != nullptr && (threadIdx.x & 63) == 0) __hip_atomic_store(fault, kFaultNmsBand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const int ntot = *nvalid;
  if (st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (r0 >= ntot) {                       // nothing left: close the run
    if (tid == 0) { st->done = 1; *count_out = st->count; }
    return;
  }
  const int n = min(ntot, r1);
  const int nrows = n - r0;               // <= NMS_BAND_ROWS (launch_nms)
  const int nw = (nrows + 63) >> 6;
  for (int v = tid; v < nw; v += 256) removed[v] = removed0[(r0 >> 6) + v];
  if (tid == 0) { s_published = 0; s_applied[0] = 0; s_applied[1] = 0; s_applied[2] = 0; }
  s_rows[tid >> 6][tid & 63] = 0;
  // the band: nms_mask_kernel packed words c, c-1, c-2, c-3 of every row side by side; 16 loads of 16 bytes in flight per thread
  {
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    const u64x2* nb = reinterpret_cast<const u64x2*>(nearband);
    const int pairs = nw * 64 * 2, last = nrows * 2 - 1;
    for (int j0 = tid; j0 < pairs; j0 += 256 * 16) {
      u64x2 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = nb[min(j0 + i * 256, last)];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = j0 + i * 256, row = j >> 1, k0 = (j & 1) * 2, c = row >> 6;
        if (j < pairs) {
          band[k0 * NMS_BAND_ROWS + row] = (row < nrows && c - k0 >= 0) ? v[i][0] : 0ull;
          band[(k0 + 1) * NMS_BAND_ROWS + row] = (row < nrows && c - k0 - 1 >= 0) ? v[i][1] : 0ull;
        }
      }
    }
  }
  const int count_in = st->count;
  __syncthreads();
  if (wid == 0) {
    u64 al1 = 0, al2 = 0, al3 = 0;        // pick sets of chunks w-1, w-2, w-3
    int cnt = count_in;
    bool full = false;
    for (int w = 0; w < nw; ++w) {
      if (w >= 4) {                       // the far words of the picks of chunk w-4 (and, in order, of all before) are in
        const int p = w - 4;
        unsigned spins = 0;
        while (flag_load(&s_applied[p % 3]) <= p / 3) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > kSpinLimit) { give_up(); break; }
        }
        NMS_COMPILER_FENCE();
      }
      const int row = w * 64 + lane;      // window-relative
      const u64 diag = band[row];
      const u64 t1 = band[NMS_BAND_ROWS + row], t2 = band[2 * NMS_BAND_ROWS + row], t3 = band[3 * NMS_BAND_ROWS + row];
      const bool near = (((t1 & al1) | (t2 & al2)) | (t3 & al3)) != 0ull;
      u64 alive = ~(removed[w] | __ballot(near));
      if (nrows - w * 64 < 64) alive &= (1ull << (nrows - w * 64)) - 1ull;
      const unsigned alo = __builtin_amdgcn_readfirstlane((unsigned)alive);
      const unsigned ahi = __builtin_amdgcn_readfirstlane((unsigned)(alive >> 32));
      const u64 alive_u = ((u64)ahi << 32) | alo;
      // the greedy choice inside the chunk: row j stays iff it is alive and no EARLIER row of the chunk that stays suppresses it --
      // a triangular system with one solution.  Sweeps x_j <- alive_j & !(below_j & X) from X = alive: after k sweeps the first k
      // rows are final, and a sweep that changes nothing has found the solution (usually 3-6 sweeps; the scalar walk it replaces
      // took one readlane step per pick, ~120 cycles each)
      const u64 below = diag & ((1ull << lane) - 1ull);
      const bool alive_j = (alive_u >> lane) & 1ull;
      u64 al = alive_u;
      for (int sweep = 0; sweep < 65; ++sweep) {
        const u64 nx = __ballot(alive_j && (below & al) == 0ull);
        if (nx == al) break;
        al = nx;
      }
      if (max_boxes >= 0) {
        const int room = max_boxes - cnt;
        while (__builtin_popcountll(al) > room) al &= ~(1ull << (63 - __builtin_clzll(al)));
      }
      if ((al >> lane) & 1ull) {
        const int pos = __builtin_popcountll(al & ((1ull << lane) - 1ull));
        pick_pos[cnt + pos] = r0 + row;
        s_rows[w & 3][pos] = row;
      }
      if (lane == 0) s_np[w & 3] = __builtin_popcountll(al);
      cnt += __builtin_popcountll(al);
      NMS_COMPILER_FENCE();
      if (lane == 0) flag_store(&s_published, w + 1);
      al3 = al2; al2 = al1; al1 = al;
      if (max_boxes >= 0 && cnt >= max_boxes) { full = true; break; }
    }
    NMS_COMPILER_FENCE();
    if (lane == 0) { s_result[0] = cnt; s_result[1] = full ? 1 : 0; }
    NMS_COMPILER_FENCE();
    if (lane == 0) flag_store(&s_published, kStop);
  } else {
    const int hw = wid - 1;
    for (int p = hw; p + 4 < nw; p += 3) {               // (chunks whose picks have no far word need no helper)
      int pub;
      unsigned spins = 0;
      while ((pub = flag_load(&s_published)) <= p) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > kSpinLimit) { give_up(); pub = kStop; break; }
      }
      if (pub >= kStop) break;                           // wave 0 is through: nobody reads `removed` any more
      NMS_COMPILER_FENCE();
      const int np = s_np[p & 3];
      const int* rows = s_rows[p & 3];
      const int word = p + 4 + lane, wordc = min(word, wwords - 1);
      // all picks of the chunk in ONE round trip (16, 32 or 64 loads in flight; addresses past the pick count are clamped)
      u64 acc = 0ull;
      auto fetch = [&](auto tag) {
        constexpr int G = decltype(tag)::value;
        u64 g[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int r = __builtin_amdgcn_readfirstlane(rows[u < np ? u : 0]);
          g[u] = mask[(size_t)r * wwords + wordc];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) acc |= (u < np) ? g[u] : 0ull;
      };
      if (np <= 0) {}                                     // a chunk without picks: its slot of s_rows holds nothing to read
      else if (np <= 16) fetch(std::integral_constant<int, 16>());
      else if (np <= 32) fetch(std::integral_constant<int, 32>());
      else fetch(std::integral_constant<int, 64>());
      if (word < nw && acc) atomicOr(&removed[word], acc);
      NMS_COMPILER_FENCE();
      if (lane == 0) flag_store(&s_applied[hw], p / 3 + 1);
    }
  }
  // picks of this window: sorted position -> original index, off the per-chunk critical path
  __syncthreads();
  const int c_end = s_result[0];
  for (int i = count_in + tid; i < c_end; i += 256) picks[i] = order[pick_pos[i]];
  __syncthreads();
  if (tid == 0) {
    st->count = c_end;
    if (s_result[1] || n >= ntot) { st->done = 1; *count_out = c_end; }
  }
}

// ---------------------------------------------------------------------------------------
// Multi-order NMS (dc_op_nms_multi; docs/SEMANTICS.md, "Localising phrases"): the greedy NMS above on ONE box list under Q score
// columns at once.  Which box suppresses which does not depend on the column -- only the order of the walk does -- so the
// suppression bits are computed once, in INDEX space, and the Q walks run side by side, one workgroup each.
//
// (a) nms_multi_mask_kernel: S[i][w], n rows of W = ceil(n_cap / 64) words; bit j of word w set <=> nms_suppresses(box i,
//     box 64w + j) and 64w + j != i (the test is symmetric in its two boxes, so the row of a pick is "what this pick removes").
//     Words past the last box are written as zero: the scan reads whole rows.
// (b) nms_multi_scan_kernel, workgroup = column q:
//     * key = (sort_key(score, candidate) << 32) | index for every row, bitonic-sorted in LDS: decreasing score, the lower index
//       first among equals, -0 == +0; rows that are no candidates (valid == 0, NaN score) carry the key of an invalid box and
//       sort behind all ncand candidates (a NaN is NOT ranked first here, the one departure from the single-order NMS).
//     * wave 0 walks the order 64 positions a chunk, lane = word of the `removed` bit set (n <= 4096 = 64 lanes x 64 bits).
//       Per chunk every lane fetches the removed-bit of its own position (one ds_bpermute pair + a ballot), so positions that
//       are dead already cost nothing; the positions still alive are then taken in order by the scalar unit: re-test the bit
//       (an earlier pick of the same chunk may have removed it), pick, OR the pick's row into `removed`.
//     * the rows of a chunk are at addresses that depend on the ORDER only, never on the picks: while wave 0 walks chunk c out
//       of one LDS buffer, waves 1..3 stage the 64 rows of chunk c + 1 into the other -- no dependent global load per pick.
//       The hand-off is one __syncthreads per chunk; the stop flag alternates between two slots so that a slot is rewritten
//       only after a further barrier (no wave can read the flag of a later chunk in the place of its own).
// A column's walk reads its own column and the shared mask only: its picks do not depend on Q, the other columns or their order.
// ---------------------------------------------------------------------------------------
constexpr int NMS_MULTI_MAX = 4096;

// (mirrors nms_mask_kernel above -- the same LDS staging, area formula and inner loop, in index space and without the
// triangle / near-band cases; a change to the IoU staging there belongs here too)
__global__ __launch_bounds__(256) void nms_multi_mask_kernel(const float* __restrict__ boxes, int n_cap,
                                                             const int32_t* __restrict__ n_dev, float thresh, int W,
                                                             u64* __restrict__ S) {
  const int n = n_dev ? max(0, min(*n_dev, n_cap)) : n_cap;
  const int rc = blockIdx.y, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (rc * 64 >= n) return;                                    // (the whole workgroup)
  const int cc = blockIdx.x * 4 + q;
  __shared__ float cb[4][64][5];
  const int cj = cc * 64 + lane;
  if (cc < W && cj < n) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)cj * 4);
    cb[q][lane][0] = b[0]; cb[q][lane][1] = b[1]; cb[q][lane][2] = b[2]; cb[q][lane][3] = b[3];
    cb[q][lane][4] = __fmul_rn(__fadd_rn(__fsub_rn(b[2], b[0]), 1.f), __fadd_rn(__fsub_rn(b[3], b[1]), 1.f));
  }
  __syncthreads();
  const int row = rc * 64 + lane;
  if (cc >= W || row >= n) return;
  const f32x4 bi = *reinterpret_cast<const f32x4*>(boxes + (size_t)row * 4);
  // box_utils.lua:178-181: area = (x2-x1+1) * (y2-y1+1)
  const float ai = __fmul_rn(__fadd_rn(__fsub_rn(bi[2], bi[0]), 1.f), __fadd_rn(__fsub_rn(bi[3], bi[1]), 1.f));
  const int jn = max(0, min(64, n - cc * 64));
  u64 word = 0;
  for (int j = 0; j < jn; ++j)
    if (cc * 64 + j != row)
      if (nms_suppresses(bi, ai, cb[q][j][0], cb[q][j][1], cb[q][j][2], cb[q][j][3], cb[q][j][4], thresh))
        word |= (1ull << j);
  S[(size_t)row * W + cc] = word;
}

__global__ __launch_bounds__(256) void nms_multi_scan_kernel(const float* __restrict__ scores, int Q,
                                                             const uint8_t* __restrict__ valid, int n_cap,
                                                             const int32_t* __restrict__ n_dev, const u64* __restrict__ S,
                                                             int W, int npad_cap, int M, int32_t* __restrict__ picks,
                                                             int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) u64 nmsm_lds[];     // keys [npad_cap] | rows [2][64 * W]
  u64* keys = nmsm_lds;
  u64* rows = nmsm_lds + npad_cap;
  __shared__ int s_ncand, s_cnt, s_done[2];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n = n_dev ? max(0, min(*n_dev, n_cap)) : n_cap;
  int npad = 64;
  while (npad < n) npad <<= 1;                                  // <= npad_cap (launch_nms_multi pads n_cap the same way)
  if (tid == 0) { s_ncand = 0; s_cnt = 0; s_done[0] = 0; s_done[1] = 0; }
  __syncthreads();
  for (int i = tid; i < npad; i += 256) {                       // (npad is a multiple of 64: whole waves)
    bool cand = false;
    u64 key = ~0ull;
    if (i < n) {
      const float s = scores[(size_t)i * Q + q];
      cand = (valid == nullptr || valid[i] != 0) && !(s != s);
      key = ((u64)sort_key(s, cand) << 32) | (u64)(uint32_t)i;
    }
    keys[i] = key;
    const u64 bal = __ballot(cand);
    if (lane == 0 && bal) atomicAdd(&s_ncand, __builtin_popcountll(bal));
  }
  __syncthreads();
  // bitonic sort, ascending (the keys are distinct but for the padding, which is all ones)
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += 256) {
        const int l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), r = l | j;
        const u64 a = keys[l], b = keys[r];
        if ((a > b) == ((l & k) == 0)) { keys[l] = b; keys[r] = a; }
      }
      __syncthreads();
    }
  const int ncand = s_ncand;
  const int nchunks = (ncand + 63) >> 6;
  const int rowwords = 64 * W;
  // rows of the 64 positions of chunk c -> buffer `buf`, by threads first, first + nthr, ...; 8 loads in flight per thread
  auto stage = [&](int c, int buf, int first, int nthr) {
    u64* dst = rows + (size_t)buf * rowwords;
    for (int t0 = first; t0 < rowwords; t0 += nthr * 8) {
      u64 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u * nthr;
        v[u] = 0ull;
        if (t < rowwords) {
          const int k = t / W, w = t - k * W, p = c * 64 + k;
          if (p < ncand) v[u] = S[(size_t)(uint32_t)keys[p] * W + w];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u * nthr;
        if (t < rowwords) dst[t] = v[u];
      }
    }
  };
  if (nchunks > 0) stage(0, 0, tid, 256);
  __syncthreads();
  u64 removed = 0ull;                                           // wave 0: lane w holds bits 64w .. 64w + 63
  int cnt = 0;
  for (int c = 0; c < nchunks; ++c) {
    if (wid != 0) {
      if (c + 1 < nchunks) stage(c + 1, (c + 1) & 1, tid - 64, 192);
    } else {
      const int p0 = c * 64, np = min(64, ncand - p0);
      const int myi = lane < np ? (int)(uint32_t)keys[p0 + lane] : 0;
      const unsigned rlo = (unsigned)__shfl((int)(unsigned)removed, myi >> 6, 64);
      const unsigned rhi = (unsigned)__shfl((int)(unsigned)(removed >> 32), myi >> 6, 64);
      const u64 mine = ((u64)rhi << 32) | rlo;
      u64 alive = __ballot(lane < np && ((mine >> (myi & 63)) & 1ull) == 0ull);
      const u64* rb = rows + (size_t)(c & 1) * rowwords;
      while (alive != 0ull && cnt < M) {
        const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(alive));
        alive &= alive - 1ull;
        const int i = __builtin_amdgcn_readlane(myi, b);
        const u64 cur = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(removed >> 32), i >> 6) << 32) |
                        (unsigned)__builtin_amdgcn_readlane((int)(unsigned)removed, i >> 6);
        if (((cur >> (i & 63)) & 1ull) == 0ull) {
          if (lane == 0) picks[(size_t)q * M + cnt] = i;
          ++cnt;
          if (lane < W) removed |= rb[b * W + lane];
        }
      }
      if (lane == 0) { s_cnt = cnt; s_done[c & 1] = cnt >= M ? 1 : 0; }
    }
    __syncthreads();
    if (s_done[c & 1]) break;
  }
  const int total = s_cnt;
  for (int j = total + tid; j < M; j += 256) picks[(size_t)q * M + j] = -1;
  if (tid == 0) counts[q] = total;
}

__global__ void gather_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                   const int32_t* __restrict__ count, int cap, int width, float* __restrict__ out) {
  const int total = cap * width;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int i = t / width, c = t - i * width;
  out[t] = i < *count ? src[(size_t)idx[i] * width + c] : 0.f;
}
__global__ void gather_rows_i32_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ idx,
                                       const int32_t* __restrict__ count, int cap, int width,
                                       int32_t* __restrict__ out) {
  const int total = cap * width;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int i = t / width, c = t - i * width;
  out[t] = i < *count ? src[(size_t)idx[i] * width + c] : 0;
}

// Captions after the final NMS, once per GROUP (round 6; DenseCapModel.lua:261-275 keeps K of the P rows -- LSTM rows are
// independent, so only those need a caption): the fc7 rows the final NMS kept, of all `nimg` images of a group, packed
// into ONE row block -- image i's K_i rows at [off_i, off_i + K_i), off_i = sum of min(count_j, P) over j < i, in pick
// order -- so that a single decode of `*total` rows serves the whole group.  Rows past *total are left as they are: the
// decode's launches carry the device-side row count (GemmDesc::m_dev) and never store them.  image = blockIdx.y.
__global__ __launch_bounds__(256) void survivor_compact_kernel(const float* __restrict__ codes,
                                                               const int32_t* __restrict__ picks,
                                                               const int32_t* __restrict__ count, int count_stride,
                                                               int nimg, int P, int D, float* __restrict__ out,
                                                               int32_t* __restrict__ total) {
  const int img = blockIdx.y;
  int off = 0, all = 0;
  for (int j = 0; j < nimg; ++j) {
    const int k = min(count[(size_t)j * count_stride], P);
    if (j < img) off += k;
    all += k;
  }
  if (blockIdx.x == 0 && img == 0 && threadIdx.x == 0) *total = all;
  const int K = min(count[(size_t)img * count_stride], P);
  const int D4 = D >> 2;
  const size_t r0 = (size_t)img * P;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)K * D4; t += (long)gridDim.x * blockDim.x) {
    const int r = (int)(t / D4), c = (int)(t - (long)r * D4);
    const size_t src = r0 + (size_t)picks[r0 + r];
    reinterpret_cast<f32x4*>(out)[((size_t)off + r) * D4 + c] = reinterpret_cast<const f32x4*>(codes)[src * D4 + c];
  }
}

// Caller-supplied boxes in the place of the RPN's (dc_forward_boxes): one workgroup per image of a group (blockIdx.x) reads the
// image's n = min(in_n[img], P) rows of `in` -- n from DEVICE memory, so a captured forward does not depend on it -- and
// writes the rows that stay, in their order, to roi_boxes, the caller's row index of each to box_src and their number to
// count[img * count_stride]: what the RPN NMS + gather leave behind for RoI pooling and everything after it.
// clip: box_utils.clip_boxes(boxes, {1, 1, W, H}, 'xcycwh') in rpn_decode_kernel's arithmetic (clip_one), rows that come out
// invalid are dropped (LocalizationLayer.lua:272-300); without it every row stays as given.
// Order-preserving compaction, 256 rows a step: a ballot per wave, the waves' counts through LDS, rank = rows kept so far +
// kept by the earlier waves + kept by the lower lanes.  Rows [count, P) are zero-filled like the dead rows of the RPN path
// (fc6 .. decode run over all P rows), their box_src is -1.
__global__ __launch_bounds__(256) void boxes_ingest_kernel(const float* __restrict__ in, const int32_t* __restrict__ in_n, int P,
                                                           int clip, float img_h, float img_w, float* __restrict__ roi_boxes,
                                                           int32_t* __restrict__ box_src, int32_t* __restrict__ count,
                                                           int count_stride) {
  __shared__ int s_wave[4];
  const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t r0 = (size_t)img * P;
  const int n = max(0, min(in_n[img], P));
  int kept = 0;                                            // rows kept by the steps so far (the same in every thread)
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    f32x4 b = {0.f, 0.f, 0.f, 0.f}, o = b;
    bool v = false;
    if (i < n) {
      b = *reinterpret_cast<const f32x4*>(in + (r0 + i) * 4);
      o = b;
      v = clip ? clip_one(b, 1.f, 1.f, img_w, img_h, o) : true;
    }
    const u64 bal = __ballot(v);
    if (lane == 0) s_wave[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int before = 0, step = 0;
    for (int w = 0; w < 4; ++w) {
      const int c = s_wave[w];
      if (w < wave) before += c;
      step += c;
    }
    if (v) {
      const int pos = kept + before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));     // < n <= P
      *reinterpret_cast<f32x4*>(roi_boxes + (r0 + pos) * 4) = o;
      box_src[r0 + pos] = i;
    }
    kept += step;
    __syncthreads();                                       // s_wave is rewritten by the next step
  }
  for (int i = kept + (int)threadIdx.x; i < P; i += 256) {
    *reinterpret_cast<f32x4*>(roi_boxes + (r0 + i) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    box_src[r0 + i] = -1;
  }
  if (threadIdx.x == 0) count[(size_t)img * count_stride] = kept;
}

// The results of a group in ONE launch (round 5; three gathers per image before): image = blockIdx.y.  A record is laid out
// exactly as the pinned host staging expects it (kRecK / kRecFault / kRecPayload, common.h) -- so that the whole group leaves in
// one device-to-host copy.
// Row r < K of image i is row picks[i*P + r] of the per-RoI tensors (box_utils.nms order, DenseCapModel.lua:261-275);
// tok_gather = 0: the token rows are already in final order, image by image (captions decoded after the final NMS, rows
// [img*P, img*P + K)); tok_gather = 2: in final order and PACKED over the group (survivor_compact_kernel's row block: image
// img's rows start at the sum of the earlier images' counts).
// kSrc (a forward on caller-supplied boxes): the record carries one more int32 per row after the values, box_src[pick] -- the
// caller's row the region came from (boxes_ingest_kernel's map composed with the final picks).  The instantiation without it
// is the kernel of every other entry point, unchanged.
template <bool kSrc>
__global__ void final_pack_kernel(const float* __restrict__ final_boxes, const float* __restrict__ obj,
                                  const int32_t* __restrict__ tokens, int tok_gather, const float* __restrict__ codes,
                                  const int32_t* __restrict__ picks, const int32_t* __restrict__ count, int count_stride,
                                  const uint32_t* __restrict__ fault, int P, int T, int D, char* __restrict__ pack,
                                  size_t stride, const int32_t* __restrict__ box_src) {
  const int img = blockIdx.y;
  const int W = 5 + (codes != nullptr ? D : T);               // 4-byte words of a row: box, score, tokens | codes
  const int K = min(count[(size_t)img * count_stride], P);
  char* rec = pack + (size_t)img * stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *reinterpret_cast<int32_t*>(rec + kRecK) = K;
    *reinterpret_cast<uint32_t*>(rec + kRecFault) = fault != nullptr ? *fault : 0u;
  }
  float* ob = reinterpret_cast<float*>(rec + kRecPayload);
  float* os = ob + (size_t)P * 4;
  uint32_t* ot = reinterpret_cast<uint32_t*>(os + P);
  const size_t r0 = (size_t)img * P;
  size_t tok0 = r0;
  if (tok_gather == 2) {
    tok0 = 0;
    for (int j = 0; j < img; ++j) tok0 += (size_t)min(count[(size_t)j * count_stride], P);
  }
  if (kSrc) {
    int32_t* osrc = reinterpret_cast<int32_t*>(ot + (size_t)P * (W - 5));
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < K; r += gridDim.x * blockDim.x) osrc[r] = box_src[r0 + (size_t)picks[r0 + r]];
  }
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)K * W; t += (long)gridDim.x * blockDim.x) {
    const int r = (int)(t / W), c = (int)(t - (long)r * W);
    const size_t src = r0 + (size_t)picks[r0 + r];
    if (c < 4) ob[(size_t)r * 4 + c] = final_boxes[src * 4 + c];
    else if (c == 4) os[r] = obj[src];
    else if (codes != nullptr) ot[(size_t)r * D + (c - 5)] = __float_as_uint(codes[src * D + (c - 5)]);
    else ot[(size_t)r * T + (c - 5)] = (uint32_t)tokens[(tok_gather == 1 ? src : tok0 + r) * T + (c - 5)];
  }
}

}  // namespace

#define LAUNCH1D(kern, n, s, ...)                                                        \
  hipLaunchKernelGGL(kern, dim3(((n) + 255) / 256 > 0 ? ((n) + 255) / 256 : 1), dim3(256), 0, s, __VA_ARGS__); \
  return hipGetLastError();

hipError_t launch_make_anchors(float* out, int h, int w, float x0, float y0, float sx, float sy,
                               const float* anchors, int k, hipStream_t s) {
  LAUNCH1D(make_anchors_kernel, k * h * w, s, out, h, w, x0, y0, sx, sy, anchors, k);
}
hipError_t launch_apply_box_transform(const float* boxes, const float* trans, float* out, int n, hipStream_t s) {
  LAUNCH1D(apply_box_transform_kernel, n, s, boxes, trans, out, n);
}
hipError_t launch_clip_boxes(const float* boxes, float* clipped, uint8_t* valid, int n, float x_min, float y_min,
                             float x_max, float y_max, hipStream_t s) {
  LAUNCH1D(clip_boxes_kernel, n, s, boxes, clipped, valid, n, x_min, y_min, x_max, y_max);
}
hipError_t launch_xcycwh_to_x1y1x2y2(const float* boxes, float* out, int n, hipStream_t s) {
  LAUNCH1D(xcycwh_to_x1y1x2y2_kernel, n, s, boxes, out, n);
}
hipError_t launch_box_iou(const float* b1, const float* b2, float* out, int B1, int B2, int convention,
                          hipStream_t s) {
  size_t total = (size_t)B1 * B2;
  int grid = (int)((total + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(box_iou_kernel, dim3(grid), dim3(256), 0, s, b1, b2, out, B1, B2, convention);
  return hipGetLastError();
}
hipError_t launch_rpn_decode(const float* heads, int nimg, int h, int w, int k, const float* anchors, float x0, float y0,
                             float sx, float sy, int img_h, int img_w, float* boxes, float* anchors_out,
                             float* trans, float* x1y1x2y2, float* p, uint8_t* valid, int clip, hipStream_t s) {
  if (nimg <= 0 || nimg > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rpn_decode_kernel, dim3((k * h * w + 255) / 256, nimg), dim3(256), 0, s, heads, h, w, k, anchors, x0, y0,
                     sx, sy, (float)img_h, (float)img_w, boxes, anchors_out, trans, x1y1x2y2, p, valid, clip);
  return hipGetLastError();
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// window k covers sorted rows [win_start(k), win_start(k+1))
// windows: 4096 boxes, then 32768 at a time (the scan kernel's LDS bit set holds 32768).  The pick budget is
// normally met inside the first window; every further window costs three (empty) launches.
// With a large pick budget (> 1024, e.g. 2000 proposals over 36,720 anchors) the picks reach past the first window;
// an intermediate 8192-row window then spares the full 32768-row triangle (graded = true).
static int win_start(int k, bool graded = false) {
  if (k == 0) return 0;
  if (!graded) return NMS_WIN0 + (k - 1) * 32768;
  return k == 1 ? NMS_WIN0 : NMS_WIN0 + 8192 + (k - 2) * 32768;
}
static size_t nms_mask_words(int n) {
  size_t best = 0;
  for (int k = 0; win_start(k) < n; ++k) {
    const int r0 = win_start(k), r1 = std::min(n, win_start(k + 1));
    const size_t rows = (size_t)(r1 - r0), words = (size_t)(r1 - r0 + 63) / 64;
    best = std::max(best, rows * words);
  }
  return best;
}
// one `removed0` bit per sorted box (the reference has no box limit, box_utils.lua:154-256: neither has this)
static size_t nms_removed_words(int n) { return ((size_t)n + 63) / 64; }
size_t nms_workspace_bytes(int n) {
  return align256((size_t)n * 4) * 6 + align256((size_t)n * 16) + align256(NMS_BUCKETS * 4) * 3 + align256(256) * 2 +
         align256(nms_removed_words(n) * 8) + align256(nms_mask_words(n) * 8) + align256(NMS_BAND_LDS);
}
hipError_t nms_workspace_bind(NmsWorkspace& ws, void* base, int n) {
  char* p = static_cast<char*>(base);
  ws.n_cap = n;
  ws.mask_words = nms_mask_words(n);
  ws.keys = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * 4);
  ws.tmp_idx = reinterpret_cast<int32_t*>(p); p += align256((size_t)n * 4);
  ws.tmp_key = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * 4);
  ws.order = reinterpret_cast<int32_t*>(p); p += align256((size_t)n * 4);
  ws.sarea = reinterpret_cast<float*>(p); p += align256((size_t)n * 4);
  ws.pick_pos = reinterpret_cast<int32_t*>(p); p += align256((size_t)n * 4);
  ws.sboxes = reinterpret_cast<float*>(p); p += align256((size_t)n * 16);
  // hist | cursor | state | nvalid | removed0 are contiguous: zeroed by one memset per call
  ws.hist = reinterpret_cast<int32_t*>(p); p += align256(NMS_BUCKETS * 4);
  ws.cursor = reinterpret_cast<int32_t*>(p); p += align256(NMS_BUCKETS * 4);
  ws.state = reinterpret_cast<int32_t*>(p); p += align256(256);
  ws.nvalid = reinterpret_cast<int32_t*>(p); p += align256(256);
  ws.removed0 = reinterpret_cast<unsigned long long*>(p); p += align256(nms_removed_words(n) * 8);
  ws.zero_bytes = (size_t)(p - reinterpret_cast<char*>(ws.hist));
  ws.off = reinterpret_cast<int32_t*>(p); p += align256(NMS_BUCKETS * 4);
  ws.mask = reinterpret_cast<u64*>(p); p += align256(ws.mask_words * 8);
  ws.nearband = reinterpret_cast<u64*>(p);
  return hipSuccess;
}

hipError_t launch_nms(NmsWorkspace& ws, const float* boxes, const float* scores, const uint8_t* valid, int n,
                      const int32_t* n_dev, float thresh, int max_boxes, int32_t* picks, int32_t* count, bool band_scan,
                      hipStream_t s, uint32_t* fault) {
  if (n > ws.n_cap) return hipErrorInvalidValue;
  hipError_t e;
  if (n <= 0) return hipMemsetAsync(count, 0, 4, s);
  if ((e = hipMemsetAsync(ws.hist, 0, ws.zero_bytes, s)) != hipSuccess) return e;
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(nms_hist_kernel, dim3(nb), dim3(256), 0, s, scores, valid, n, n_dev, ws.keys, ws.hist,
                     ws.nvalid);
  hipLaunchKernelGGL(nms_bucket_scan_kernel, dim3(1), dim3(1024), 0, s, ws.hist, ws.off);
  hipLaunchKernelGGL(nms_bucket_scatter_kernel, dim3(nb), dim3(256), 0, s, ws.keys, n, n_dev, ws.off, ws.cursor,
                     ws.tmp_key, ws.tmp_idx);
  hipLaunchKernelGGL(nms_bucket_rank_kernel, dim3(nb), dim3(256), 0, s, ws.tmp_key, ws.tmp_idx, boxes, n, n_dev, ws.off,
                     ws.hist, ws.order, ws.sboxes, ws.sarea);
  NmsState* st = reinterpret_cast<NmsState*>(ws.state);
  const bool graded = max_boxes > 1024 && n > NMS_WIN0 + 8192;
  for (int k = 0;; ++k) {
    const int r0 = win_start(k, graded);
    const int r1 = std::min(n, win_start(k + 1, graded));
    const int rows = std::max(r1 - r0, 0);
    const int wchunks = (rows + 63) / 64;
    const bool band = band_scan && rows > 0 && rows <= NMS_BAND_ROWS;
    if (rows > 0) {
      if (k > 0)
        hipLaunchKernelGGL(nms_cross_kernel, dim3(wchunks, 4), dim3(256), 0, s, ws.sboxes, ws.sarea, ws.nvalid, st,
                           ws.pick_pos, r0, r1, thresh, ws.removed0);
      hipLaunchKernelGGL(nms_mask_kernel, dim3((wchunks + 3) / 4, wchunks), dim3(256), 0, s, ws.sboxes, ws.sarea,
                         ws.nvalid, st, r0, r1, thresh, wchunks, ws.mask, band ? ws.nearband : nullptr);
    }
    if (rows <= 0) break;                // (the last window's scan closes the run: min(*nvalid, r1) >= *nvalid there)
    if (band) {
      const void* fn = reinterpret_cast<const void*>(&nms_scan_band_kernel);
      if ((e = ensure_dyn_lds(fn, NMS_BAND_LDS)) != hipSuccess) return e;
      hipLaunchKernelGGL(nms_scan_band_kernel, dim3(1), dim3(256), NMS_BAND_LDS, s, ws.mask, wchunks, ws.nearband, ws.nvalid, ws.order, r0,
                         r1, max_boxes, ws.removed0, picks, ws.pick_pos, st, count, fault);
    } else {
      hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(256), 0, s, ws.mask, wchunks, ws.nvalid, ws.order, r0, r1, max_boxes,
                         ws.removed0, picks, ws.pick_pos, st, count);
    }
  }
  return hipGetLastError();
}

size_t nms_multi_workspace_bytes(int n) { return align256((size_t)n * (((size_t)n + 63) / 64) * 8); }
hipError_t launch_nms_multi(void* ws, const float* boxes, const float* scores, const uint8_t* valid, int n,
                            const int32_t* n_dev, int Q, float thresh, int max_picks, int32_t* picks, int32_t* counts,
                            hipStream_t s) {
  if (n < 1 || n > NMS_MULTI_MAX || Q < 1 || max_picks < 1 || max_picks > NMS_MULTI_MAX) return hipErrorInvalidValue;
  const int W = (n + 63) / 64;
  int npad = 64;
  while (npad < n) npad <<= 1;
  u64* S = static_cast<u64*>(ws);
  hipLaunchKernelGGL(nms_multi_mask_kernel, dim3((W + 3) / 4, W), dim3(256), 0, s, boxes, n, n_dev, thresh, W, S);
  const size_t lds = ((size_t)npad + 2 * 64 * (size_t)W) * sizeof(u64);         // <= 96 KiB
  const void* fn = reinterpret_cast<const void*>(&nms_multi_scan_kernel);
  hipError_t e = ensure_dyn_lds(fn, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nms_multi_scan_kernel, dim3(Q), dim3(256), lds, s, scores, Q, valid, n, n_dev, S, W, npad, max_picks,
                     picks, counts);
  return hipGetLastError();
}

hipError_t launch_final_pack(const float* final_boxes, const float* obj, const int32_t* tokens, int tok_gather,
                             const float* codes, const int32_t* picks, const int32_t* count, int count_stride,
                             const uint32_t* fault, int nimg, int P, int T, int D, void* pack, size_t stride, hipStream_t s,
                             const int32_t* box_src) {
  if (nimg <= 0 || nimg > 65535 || P <= 0) return hipErrorInvalidValue;
  const long per = (long)P * (5 + (codes != nullptr ? D : T));
  const int gx = (int)std::min<long>((per + 255) / 256, 2048);
  if (box_src != nullptr)
    hipLaunchKernelGGL(final_pack_kernel<true>, dim3(gx, nimg), dim3(256), 0, s, final_boxes, obj, tokens, tok_gather, codes, picks,
                       count, count_stride, fault, P, T, D, static_cast<char*>(pack), stride, box_src);
  else
    hipLaunchKernelGGL(final_pack_kernel<false>, dim3(gx, nimg), dim3(256), 0, s, final_boxes, obj, tokens, tok_gather, codes, picks,
                       count, count_stride, fault, P, T, D, static_cast<char*>(pack), stride, box_src);
  return hipGetLastError();
}

hipError_t launch_boxes_ingest(const float* in, const int32_t* in_n, int nimg, int P, int clip, int img_h, int img_w,
                               float* roi_boxes, int32_t* box_src, int32_t* count, int count_stride, hipStream_t s) {
  if (nimg <= 0 || P <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(boxes_ingest_kernel, dim3(nimg), dim3(256), 0, s, in, in_n, P, clip, (float)img_h, (float)img_w, roi_boxes,
                     box_src, count, count_stride);
  return hipGetLastError();
}

hipError_t launch_survivor_compact(const float* codes, const int32_t* picks, const int32_t* count, int count_stride, int nimg,
                                   int P, int D, float* out, int32_t* total, hipStream_t s) {
  if (nimg <= 0 || nimg > 65535 || P <= 0 || D <= 0 || D % 4) return hipErrorInvalidValue;
  // a final NMS at 0.3 keeps about a quarter of the rows: blocks for P/2 rows, grid-stride beyond
  const long work = (long)std::max(P / 2, 1) * (D / 4);
  const int gx = (int)std::min<long>((work + 255) / 256, 2048);
  hipLaunchKernelGGL(survivor_compact_kernel, dim3(gx, nimg), dim3(256), 0, s, codes, picks, count, count_stride, nimg, P, D, out,
                     total);
  return hipGetLastError();
}

hipError_t launch_gather_rows(const float* src, const int32_t* idx, const int32_t* count, int cap, int width,
                              float* out, hipStream_t s) {
  LAUNCH1D(gather_rows_kernel, cap * width, s, src, idx, count, cap, width, out);
}
hipError_t launch_gather_rows_i32(const int32_t* src, const int32_t* idx, const int32_t* count, int cap, int width,
                                  int32_t* out, hipStream_t s) {
  LAUNCH1D(gather_rows_i32_kernel, cap * width, s, src, idx, count, cap, width, out);
}
