// Vocabulary screen of the greedy decode (densecap.hip::lm_sample_parts, Settings::decode_screen).
//
// scores[m][j] = fp16(bias_j + sum_k bf16(h_mk) * bf16(w_jk)) for every live row m and real vocabulary column j, on
// v_mfma_f32_32x32x16_bf16 (sixteen times the fp32 MFMA rate).  The scores decide nothing by themselves: the row tail
// (elementwise.hip, lstm_rescore_tail_kernel) turns them into a short list of columns that can still hold the fp32 arg-max
// and re-computes those exactly.  Operands are bf16 already: hb is written by the tail that writes h, wb once at weight load.
//
// Tile 128 x 128, K in steps of 64 through a two-stage LDS ring (64 KB: two workgroups per CU); 2 x 2 waves, wave tile
// 64 x 64 = 2 x 2 MFMA blocks; one barrier per K step.  Operands travel global -> registers -> LDS, three K steps ahead of the
// MFMAs (a step's MFMAs take ~0.2 us, a load from beyond the L2 several times that).  LDS rows are 128 bytes (64 bf16);
// 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 7): the sixteen lanes one ds_read_b128 cycle serves then fall into
// sixteen different bank quads.  With eight or more row tiles every XCD (workgroup id mod 8) owns a contiguous eighth of
// them and walks the column tiles with it: its rows of h stay in its L2 and it reads every weight tile once.
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int SBM = 128, SBN = 128, SBK = 64;

__device__ __forceinline__ int lds_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// hb (M rows, Kp bf16 each), wb (V1pad rows, Kp bf16 each), Kp % 64 == 0 (columns past Hd are zero in both);
// scores (M rows, V1pad fp16 each): columns [0, V1) of rows below the live count are written
__global__ __launch_bounds__(256, 2) void decode_screen_kernel(const uint16_t* __restrict__ hb, const uint16_t* __restrict__ wb,
                                                               const float* __restrict__ bias, _Float16* __restrict__ scores,
                                                               int M, const int32_t* __restrict__ m_dev, int V1, int V1pad,
                                                               int Kp, int ntm, int mt_xcd) {
  const int Meff = m_dev ? min(M, *m_dev) : M;
  int tile_m, tile_n;
  if (mt_xcd > 0) {
    const int xcd = blockIdx.x & 7, l = blockIdx.x >> 3;
    tile_m = xcd * mt_xcd + l % mt_xcd;
    tile_n = l / mt_xcd;
    if (tile_m >= ntm) return;
  } else {
    tile_m = blockIdx.x % ntm;                         // m fastest: neighbours share the weight tile
    tile_n = blockIdx.x / ntm;
  }
  const int m0 = tile_m * SBM, n0 = tile_n * SBN;
  if (m0 >= Meff) return;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][SBM * SBK * 2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1, r = lane & 31, hsel = lane >> 5;
  // global -> register -> LDS: thread owns chunk (tid & 7) of rows (tid >> 3) + 32 i of both tiles
  const int lrow = tid >> 3, lchunk = tid & 7;
  const uint16_t* ga[4];
  const uint16_t* gb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ga[i] = hb + (size_t)min(m0 + lrow + 32 * i, M - 1) * Kp + lchunk * 8;       // rows past the buffers are clamped, never stored
    gb[i] = wb + (size_t)min(n0 + lrow + 32 * i, V1pad - 1) * Kp + lchunk * 8;
  }
  u32x4 ra[3][4], rb[3][4];                          // three register sets: K steps kt + 1 .. kt + 3 in flight
  auto gload = [&](int set, int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[set][i] = *reinterpret_cast<const u32x4*>(ga[i] + k0);
      rb[set][i] = *reinterpret_cast<const u32x4*>(gb[i] + k0);
    }
  };
  auto lstore = [&](int st, int set) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(&lds[st][0][lds_off(lrow + 32 * i, lchunk)]) = ra[set][i];
      *reinterpret_cast<u32x4*>(&lds[st][1][lds_off(lrow + 32 * i, lchunk)]) = rb[set][i];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nk = Kp / SBK;
  // K step kt: LDS stage st = kt & 1, register set rs = kt % 3 (compile-time constants at the call sites)
  auto step = [&](int kt, int st, int rs) {
    if (kt + 3 < nk) gload(rs, (kt + 3) * SBK);       // set rs was stored to LDS before the previous barrier
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = 2 * kk + hsel;                   // lane half h supplies k = 16 kk + 8 h .. + 7
      u32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const u32x4*>(&lds[st][0][lds_off(wm * 64 + i * 32 + r, c)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const u32x4*>(&lds[st][1][lds_off(wn * 64 + j * 32 + r, c)]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]), __builtin_bit_cast(bf16x8, b[j]),
                                                              acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) lstore(st ^ 1, (rs + 1) % 3);   // the other stage was last read before the previous barrier
    __syncthreads();
  };
  gload(0, 0);
  if (nk > 1) gload(1, SBK);
  if (nk > 2) gload(2, 2 * SBK);
  lstore(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 6) {
    step(kt, 0, 0);
    if (kt + 1 < nk) step(kt + 1, 1, 1);
    if (kt + 2 < nk) step(kt + 2, 0, 2);
    if (kt + 3 < nk) step(kt + 3, 1, 0);
    if (kt + 4 < nk) step(kt + 4, 0, 1);
    if (kt + 5 < nk) step(kt + 5, 1, 2);
  }
  // register e of block (i, j): row m0 + wm*64 + i*32 + 8*(e>>2) + 4*hsel + (e&3), column n0 + wn*64 + j*32 + r.  Lanes r and
  // r ^ 1 trade one value per register pair (a quad permute): the even lane then holds columns (n, n + 1) of row e, the odd
  // lane columns (n - 1, n) of row e + 1 -- 4-byte stores, a half-wave writes 32 consecutive fp16 of two rows.  The address is a
  // wave-uniform part (scalar unit) plus one lane offset for the whole tile.
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  const bool odd = (r & 1) != 0;
  const int wmu = __builtin_amdgcn_readfirstlane(wm), wnu = __builtin_amdgcn_readfirstlane(wn);
  _Float16* const wtile = scores + (size_t)(m0 + wmu * 64) * V1pad + (n0 + wnu * 64);
  const unsigned lane_off = (unsigned)((4 * hsel + (odd ? 1 : 0)) * V1pad + (r & ~1));
  const bool interior = m0 + SBM <= Meff && n0 + SBN <= V1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + r;
    const float bv = n < V1 ? bias[n] : 0.f;
    const int nl = n & ~1;                             // the pair's first column
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const float v0 = acc[i][j][e] + bv, v1 = acc[i][j][e + 1] + bv;
        const float send = odd ? v0 : v1;
        const float got = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xf, 0xf, false));
        const f16x2 pr = odd ? f16x2{(_Float16)got, (_Float16)v1} : f16x2{(_Float16)v0, (_Float16)got};
        const int ro = i * 32 + 8 * (e >> 2) + (e & 3);              // row of register e inside the wave tile, before the lane's part
        _Float16* dst = wtile + (size_t)ro * V1pad + j * 32 + lane_off;
        if (interior) {
          *reinterpret_cast<f16x2*>(dst) = pr;
        } else {
          const int m = m0 + wm * 64 + ro + 4 * hsel + (odd ? 1 : 0);
          if (m >= Meff) continue;
          if (nl + 1 < V1) *reinterpret_cast<f16x2*>(dst) = pr;
          else if (nl < V1) *dst = pr[0];
        }
      }
  }
}

}  // namespace

hipError_t launch_decode_screen(const uint16_t* hb, const uint16_t* wb, const float* bias, void* scores, int M,
                                const int32_t* m_dev, int V1, int V1pad, int Kp, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  if (Kp <= 0 || Kp % SBK || V1 <= 0 || V1 > V1pad) return hipErrorInvalidValue;
  const int ntm = (M + SBM - 1) / SBM, ntn = (V1 + SBN - 1) / SBN;
  const int mt_xcd = ntm >= 8 ? (ntm + 7) / 8 : 0;     // row tiles per XCD (0: too few to share out)
  const unsigned grid = mt_xcd > 0 ? 8u * mt_xcd * ntn : (unsigned)ntm * ntn;
  hipLaunchKernelGGL(decode_screen_kernel, dim3(grid), dim3(256), 0, s, hb, wb, bias, static_cast<_Float16*>(scores), M, m_dev,
                     V1, V1pad, Kp, ntm, mt_xcd);
  return hipGetLastError();
}
