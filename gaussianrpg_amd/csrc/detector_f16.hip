// The detector's network in FP16 for gfx950: detector.hip's launch list -- the same implicit GEMM, address modes and
// epilogue options, NCHW -- with fp16 activations and weights on v_mfma_f32_32x32x16_f16.  No
// atomics, no split-K: identical calls give identical bits.
//
// conv_f16_kernel<BM, BN, KS>: M = C_out, N = bs * H_out * W_out, K = C_in * k * k, k = (ci * KS + ky) * KS + kx.
//   chain    the accumulator starts at the float32 bias and takes one 32x32x16 instruction per 16 k, k ascending:
//            float32 accumulation of exact fp16 x fp16 products.  The order inside one instruction is the
//            hardware's.  Both tile shapes issue the same instructions per output element: same bits.  One
//            accumulator set (detector.hip's second, `part`, kept the f32 chain short; under a 2^-11 output
//            rounding that buys nothing);
//   epilogue SiLU in float32 (correctly rounded division), then + residual (read as fp16, added in float32), then ONE
//            rounding to fp16 (nearest even, overflow to inf), and that value goes to the plain store and to the
//            2 x 2 upsample store.  out_f32: the float32 value is stored unrounded (Detect's heads).
// Tiles: 128 x 128 (four waves, each 2 x 2 MFMA tiles of 32 x 32) and 64 x 64 (each one tile), both 32 deep: two
// instructions per K tile.
//
// LDS image.  Lane l of the instruction holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31],
// j = 0..7: eight consecutive k of one row / column.  So both tiles are stored k-minor -- As[m][k], Bs[n][k] -- and a
// lane's operand is ONE 16-byte read.  A row is 32 halves (64 bytes) padded by 8 halves, one access width, to
// DET16_LDK = 40 halves = 20 dwords: row r starts at bank 4 * (5 r mod 16), so rows that are distinct modulo 16 sit
// on disjoint 16-byte slots.  A 16-byte LDS read is served in four groups of 16 lanes, each inside one half-wave and
// made of rows distinct modulo 16 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}): no bank conflict.
// LDS per workgroup = (BM + BN) * 40 * 2 bytes: 20480 for 128 x 128, 10240 for 64 x 64.
//
// A (weights) comes from a buffer repacked once (pack_f16_kernel): [bias: M_pad floats][M_pad][K_pad] halves,
// M-major, M_pad a multiple of 128 and K_pad of 32, zeros in the padding, rounded with __float2half_rn.  A row of
// the A tile is then 64 contiguous bytes in memory and in LDS: four unguarded 16-byte loads that land in the image
// without a transpose.  B (the im2col gather) stays lanes-along-pixels, one guarded 2-byte load per element; a
// thread gathers consecutive k of ONE pixel (detector_gather.h: one division per run, then increments), packs them
// and writes them as 16-byte pieces of a row: the transpose is the write address.  Both tiles go global -> registers
// -> LDS, with TWO tiles in flight in registers: tile kt + 2 is requested before the MFMAs of tile kt.
//
// spp_f16_kernel: detector.hip's pool on halves (max is exact, NaN wins, -inf padding).
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>

#include "abi_util.h"
#include "common.h"
#include "detector_gather.h"

namespace grpg {

namespace {

constexpr int DET16_THREADS = 256;
constexpr int DET16_BK = 32;     // two 16-deep instructions
constexpr int DET16_MPAD = 128;  // packed weights: C_out rounded up to this, for either tile
constexpr int DET16_LDK = DET16_BK + 8;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Conv16Args {
  const uint16_t* in;
  void* out;
  const _Float16* res;
  _Float16* up;
  const void* packed;
  int in_c0, in_ct, out_c0, out_ct, res_c0, res_ct, up_c0, up_ct;
  int bs, c_in, c_out, h_in, w_in, h_out, w_out;   // h_in, w_in: the stored tensor's
  int stride, act, focus, out_f32;
  int K, m_pad, k_pad, N;
};

__host__ __device__ inline int round_up(const int v, const int m) { return (v + m - 1) / m * m; }

// rows m of the C/D registers of v_mfma_f32_32x32x16_f16 (the f32 form's map): column lane & 31, row below
__device__ __forceinline__ int cd_row(const int reg, const int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float silu(const float x) { return x * (1.0f / (1.0f + expf(-x))); }

// Registers: the 128 x 128 shape holds 64 accumulator registers and is allocated for two waves per SIMD, the
// 64 x 64 shape 16 for four (tests/test_detector_f16_resources.py).
template <int BM, int BN, int KS>
__global__ void __launch_bounds__(DET16_THREADS, BM == 128 ? 2 : 4) conv_f16_kernel(const Conv16Args a) {
  constexpr int TM = BM / 64, TN = BN / 64;                  // MFMA tiles per wave
  constexpr int A_VEC = BM * (DET16_BK / 8) / DET16_THREADS; // 16-byte loads per thread and tile
  constexpr int B_SEGS = DET16_THREADS / BN;                 // threads per pixel
  constexpr int B_PER = DET16_BK / B_SEGS;                   // consecutive k per thread and tile
  static_assert(A_VEC >= 1 && B_PER >= 8 && B_PER % 8 == 0, "tile too small for the block");
  __shared__ __attribute__((aligned(16))) uint16_t As[BM * DET16_LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[BN * DET16_LDK];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;                    // N < 2^31 - BN (conv_check)

  // ---- this thread's piece of the B tile: one output pixel, B_PER consecutive k (detector_gather.h) ----
  const int bn = t % BN, bk0 = (t / BN) * B_PER;
  const int n = n0 + bn;
  const bool n_ok = n < a.N;
  const uint16_t* in_b = a.in;
  ConvGather<KS> g;
  {
    const int lh = a.focus ? a.h_in >> 1 : a.h_in, lw = a.focus ? a.w_in >> 1 : a.w_in;   // logical input plane
    int iy0 = 0, ix0 = 0;
    if (n_ok) {
      const int hw = a.h_out * a.w_out;
      const int b = n / hw, r = n - b * hw;
      const int oy = r / a.w_out, ox = r - oy * a.w_out;
      iy0 = oy * a.stride - KS / 2;
      ix0 = ox * a.stride - KS / 2;
      in_b += ((size_t)b * a.in_ct + a.in_c0) * ((size_t)a.h_in * a.w_in);
    }
    g.init(n_ok, iy0, ix0, lh, lw, a.h_in, a.w_in, a.focus ? a.c_in >> 2 : a.c_in, a.focus != 0, a.K);
  }
  // B_PER consecutive k from k0, packed in pairs: the fp16's bits, +0 where the tap is padding or beyond K
  auto load_b = [&](const int k0, uint32_t (&rb)[B_PER / 2]) {
    g.start(k0);
#pragma unroll
    for (int v = 0; v < B_PER / 2; v++) {
      const uint32_t lo = g.valid() ? in_b[g.offset()] : 0u;
      g.next();
      const uint32_t hi = g.valid() ? in_b[g.offset()] : 0u;
      g.next();
      rb[v] = lo | (hi << 16);
    }
  };
  const uint16_t* wp = reinterpret_cast<const uint16_t*>(reinterpret_cast<const float*>(a.packed) + a.m_pad);   // behind the bias
  auto load_a = [&](const int k0, const int v) -> u32x4 {
    const int e = v * DET16_THREADS + t, row = e >> 2, seg = e & 3;
    return *reinterpret_cast<const u32x4*>(wp + (size_t)(m0 + row) * a.k_pad + k0 + seg * 8);   // row < m_pad, k < k_pad
  };

  // ---- the accumulator starts at the bias ----
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float bias = reinterpret_cast<const float*>(a.packed)[m0 + wm + i * 32 + cd_row(r, lane)];   // < m_pad: zeros
#pragma unroll
      for (int j = 0; j < TN; j++) acc[i][j][r] = bias;
    }

  // ---- the K loop: two tiles in flight in registers, so that a tile's loads have the whole of the previous
  // tile's iteration to arrive (a layer with few workgroups per compute unit has nothing else to hide them) ----
  const int k_tiles = (a.K + DET16_BK - 1) / DET16_BK;
  u32x4 ra[2][A_VEC];
  uint32_t rb[2][B_PER / 2];
  auto load_tile = [&](const int kt, u32x4 (&qa)[A_VEC], uint32_t (&qb)[B_PER / 2]) {
#pragma unroll
    for (int v = 0; v < A_VEC; v++) qa[v] = load_a(kt * DET16_BK, v);
    load_b(kt * DET16_BK + bk0, qb);
  };
  // stage the tile held in (qa, qb), refill the registers with tile `next` (if any), multiply
  auto step = [&](const int next, u32x4 (&qa)[A_VEC], uint32_t (&qb)[B_PER / 2]) {
#pragma unroll
    for (int v = 0; v < A_VEC; v++) {
      const int e = v * DET16_THREADS + t, row = e >> 2, seg = e & 3;
      *reinterpret_cast<u32x4*>(&As[row * DET16_LDK + seg * 8]) = qa[v];
    }
#pragma unroll
    for (int v = 0; v < B_PER / 8; v++) {
      u32x4 q;
      q[0] = qb[4 * v]; q[1] = qb[4 * v + 1]; q[2] = qb[4 * v + 2]; q[3] = qb[4 * v + 3];
      *reinterpret_cast<u32x4*>(&Bs[bn * DET16_LDK + bk0 + 8 * v]) = q;
    }
    __syncthreads();
    if (next < k_tiles) load_tile(next, qa, qb);
#pragma unroll
    for (int kk = 0; kk < DET16_BK; kk += 16) {
      const int ko = kk + 8 * (lane >> 5), rc = lane & 31;
      f16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) fa[i] = *reinterpret_cast<const f16x8*>(&As[(wm + i * 32 + rc) * DET16_LDK + ko]);
#pragma unroll
      for (int j = 0; j < TN; j++) fb[j] = *reinterpret_cast<const f16x8*>(&Bs[(wn + j * 32 + rc) * DET16_LDK + ko]);
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  };
  load_tile(0, ra[0], rb[0]);
  if (k_tiles > 1) load_tile(1, ra[1], rb[1]);
  for (int kt = 0; kt < k_tiles; kt += 2) {       // k ascending, one instruction per 16 k: the order does not change
    step(kt + 2, ra[0], rb[0]);
    if (kt + 1 < k_tiles) step(kt + 3, ra[1], rb[1]);
  }

  // ---- epilogue: activation, residual, the one rounding, the store(s) ----
  const size_t out_plane = (size_t)a.h_out * a.w_out;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int nn = n0 + wn + j * 32 + (lane & 31);
    if (nn >= a.N) continue;
    const int hw = a.h_out * a.w_out;
    const int b = nn / hw, r = nn - b * hw;
    const int oy = r / a.w_out, ox = r - oy * a.w_out;
    const size_t out_o = ((size_t)b * a.out_ct + a.out_c0) * out_plane + r;
    const _Float16* res_p = a.res ? a.res + ((size_t)b * a.res_ct + a.res_c0) * out_plane + r : nullptr;
    _Float16* up_p = a.up ? a.up + ((size_t)b * a.up_ct + a.up_c0) * (4 * out_plane) + (size_t)(2 * oy) * (2 * a.w_out) + 2 * ox
                          : nullptr;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int rg = 0; rg < 16; rg++) {
        const int m = m0 + wm + i * 32 + cd_row(rg, lane);
        if (m >= a.c_out) continue;
        float v = acc[i][j][rg];
        if (a.act) v = silu(v);
        if (res_p) v = (float)res_p[(size_t)m * out_plane] + v;
        if (a.out_f32) {                                     // Detect's heads: res and up are NULL (conv_check)
          static_cast<float*>(a.out)[out_o + (size_t)m * out_plane] = v;
          continue;
        }
        const _Float16 hv = (_Float16)v;                     // v_cvt_f16_f32: nearest even, overflow to inf
        static_cast<_Float16*>(a.out)[out_o + (size_t)m * out_plane] = hv;
        if (up_p) {
          _Float16* u = up_p + (size_t)m * (4 * out_plane);
          u[0] = hv;
          u[1] = hv;
          u[2 * a.w_out] = hv;
          u[2 * a.w_out + 1] = hv;
        }
      }
  }
}

// OIHW float32 weights + bias -> [bias: m_pad floats][m_pad][k_pad] halves, zeros in the padding; one thread per
// packed element (float or half).
__global__ void __launch_bounds__(DET16_THREADS)
pack_f16_kernel(const float* __restrict__ w, const float* __restrict__ bias, const int c_out, const int K, const int m_pad,
                const int k_pad, void* __restrict__ packed) {
  const size_t i = (size_t)blockIdx.x * DET16_THREADS + threadIdx.x;
  const size_t total = (size_t)m_pad * ((size_t)k_pad + 1);
  if (i >= total) return;
  if (i < (size_t)m_pad) {
    static_cast<float*>(packed)[i] = ((int)i < c_out && bias) ? bias[i] : 0.0f;
    return;
  }
  const size_t e = i - m_pad;
  const int m = (int)(e / k_pad), k = (int)(e - (size_t)m * k_pad);
  const float v = (m < c_out && k < K) ? w[(size_t)m * K + k] : 0.0f;
  reinterpret_cast<__half*>(static_cast<float*>(packed) + m_pad)[e] = __float2half_rn(v);
}

// ---- SPP ----
constexpr int SPP_T = 16, SPP_HALO = 6, SPP_S = SPP_T + 2 * SPP_HALO;   // 28

struct Pool16Args {
  const _Float16* in;
  _Float16* out;
  int in_c0, in_ct, out_c0, out_ct;
  int bs, c, h, w, tiles_x;
};

// max as nn.MaxPool2d takes it: NaN wins
__device__ __forceinline__ _Float16 max_nan(const _Float16 m, const _Float16 v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(DET16_THREADS) spp_f16_kernel(const Pool16Args a) {
  __shared__ _Float16 tile[SPP_S][SPP_S + 1];
  __shared__ _Float16 rows[3][SPP_S][SPP_T + 1];
  const int t = threadIdx.x;
  const int ty0 = (blockIdx.x / a.tiles_x) * SPP_T, tx0 = (blockIdx.x % a.tiles_x) * SPP_T;
  const int c = blockIdx.y, b = blockIdx.z;
  const size_t plane = (size_t)a.h * a.w;
  const _Float16* src = a.in + ((size_t)b * a.in_ct + a.in_c0 + c) * plane;
  for (int e = t; e < SPP_S * SPP_S; e += DET16_THREADS) {
    const int ly = e / SPP_S, lx = e - ly * SPP_S;
    const int y = ty0 + ly - SPP_HALO, x = tx0 + lx - SPP_HALO;
    tile[ly][lx] = (y >= 0 && y < a.h && x >= 0 && x < a.w) ? src[(size_t)y * a.w + x] : (_Float16)(-INFINITY);
  }
  __syncthreads();
  for (int e = t; e < SPP_S * SPP_T; e += DET16_THREADS) {
    const int ly = e / SPP_T, lx = e - ly * SPP_T;   // output column lx: centre at tile column lx + 6
    _Float16 m = tile[ly][lx + SPP_HALO];
#pragma unroll
    for (int d = 1; d <= 6; d++) {
      m = max_nan(max_nan(m, tile[ly][lx + SPP_HALO - d]), tile[ly][lx + SPP_HALO + d]);
      if (d == 2) rows[0][ly][lx] = m;
      if (d == 4) rows[1][ly][lx] = m;
    }
    rows[2][ly][lx] = m;
  }
  __syncthreads();
  const int ly = t / SPP_T, lx = t - ly * SPP_T;
  const int y = ty0 + ly, x = tx0 + lx;
  if (y >= a.h || x >= a.w) return;
#pragma unroll
  for (int p = 0; p < 3; p++) {
    const int rad = 2 + 2 * p;
    _Float16 m = rows[p][ly + SPP_HALO][lx];
    for (int d = 1; d <= rad; d++) m = max_nan(max_nan(m, rows[p][ly + SPP_HALO - d][lx]), rows[p][ly + SPP_HALO + d][lx]);
    a.out[((size_t)b * a.out_ct + a.out_c0 + (size_t)p * a.c + c) * plane + (size_t)y * a.w + x] = m;
  }
}

// ---- checks and launches: detector.hip's, with the element size a parameter and the overlap in bytes ----

bool misaligned(const void* p, const uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// [p, p + n) and [q, q + m) bytes share memory
bool overlap(const void* p, const size_t n, const void* q, const size_t m) {
  return (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}

// [c0, c0 + c) inside [0, ct)
bool slice_ok(const int c0, const int c, const int ct) { return c0 >= 0 && c >= 1 && ct >= 1 && (long long)c0 + c <= ct; }

// bs * ct * h * w elements must stay addressable and the launch's n below 2^31
bool extent_ok(const int bs, const int ct, const int h, const int w) {
  return (long long)bs * ct * h * w < (1ll << 40) && (long long)bs * h * w < (1ll << 31) - 256;
}

int conv_check(const std::string& pre, const grpg_detector_layer_f16& L) {
  if (!L.in || !L.out || !L.packed) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL in / out / packed");
  if (L.out_f32 != 0 && L.out_f32 != 1) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "out_f32 must be 0 or 1");
  if (L.out_f32 && (L.res || L.up))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "a float32 output (out_f32) takes no residual and no upsampled store");
  if (misaligned(L.in, 2) || misaligned(L.out, L.out_f32 ? 4 : 2) || misaligned(L.res, 2) || misaligned(L.up, 2))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "fp16 tensors must be 2-byte aligned, a float32 out 4-byte aligned");
  if ((uintptr_t)L.packed & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "packed must be 16-byte aligned");
  if (L.bs < 1 || L.c_in < 1 || L.c_out < 1 || L.h_in < 1 || L.w_in < 1 || L.h_out < 1 || L.w_out < 1)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "sizes must be positive");
  if (L.k != 1 && L.k != 3) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "k must be 1 or 3");
  if (L.stride != 1 && L.stride != 2) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "stride must be 1 or 2");
  if (L.act != GRPG_DET_ACT_NONE && L.act != GRPG_DET_ACT_SILU)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "unknown activation");
  if (L.in_mode != GRPG_DET_IN_PLAIN && L.in_mode != GRPG_DET_IN_FOCUS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "unknown input mode");
  if (L.tile != GRPG_DET_TILE_128 && L.tile != GRPG_DET_TILE_64)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "unknown tile shape");
  const bool focus = L.in_mode == GRPG_DET_IN_FOCUS;
  if (focus && ((L.c_in & 3) || (L.h_in & 1) || (L.w_in & 1)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "Focus needs c_in a multiple of 4 and an even stored height and width");
  const int cs = focus ? L.c_in / 4 : L.c_in, lh = focus ? L.h_in / 2 : L.h_in, lw = focus ? L.w_in / 2 : L.w_in;
  const int p = L.k / 2;
  if (L.h_out != (lh + 2 * p - L.k) / L.stride + 1 || L.w_out != (lw + 2 * p - L.k) / L.stride + 1)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "h_out / w_out are not what k, stride and padding k / 2 give");
  if (!slice_ok(L.in_c0, cs, L.in_ct) || !slice_ok(L.out_c0, L.c_out, L.out_ct))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the input or output slice leaves its tensor");
  if (L.res && !slice_ok(L.res_c0, L.c_out, L.res_ct))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the residual slice leaves its tensor");
  if (L.up && !slice_ok(L.up_c0, L.c_out, L.up_ct))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the upsampled slice leaves its tensor");
  if ((long long)L.c_in * L.k * L.k >= (1ll << 24)) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "C_in * k * k too large");
  if (!extent_ok(L.bs, L.in_ct, L.h_in, L.w_in) || !extent_ok(L.bs, L.out_ct, L.h_out, L.w_out) ||
      (L.res && !extent_ok(L.bs, L.res_ct, L.h_out, L.w_out)) || (L.up && !extent_ok(L.bs, L.up_ct, 2 * L.h_out, 2 * L.w_out)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "tensor too large for one launch");
  const size_t b_in = 2 * (size_t)L.bs * L.in_ct * L.h_in * L.w_in;
  const size_t b_out = (L.out_f32 ? 4 : 2) * (size_t)L.bs * L.out_ct * L.h_out * L.w_out;
  const size_t b_res = 2 * (size_t)L.bs * L.res_ct * L.h_out * L.w_out, b_up = 8 * (size_t)L.bs * L.up_ct * L.h_out * L.w_out;
  if (overlap(L.out, b_out, L.in, b_in) || (L.res && overlap(L.out, b_out, L.res, b_res)) ||
      (L.up && (overlap(L.up, b_up, L.in, b_in) || overlap(L.up, b_up, L.out, b_out) ||
                (L.res && overlap(L.up, b_up, L.res, b_res)))))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "a convolution cannot write a tensor it reads (or one tensor twice)");
  return GRPG_OK;
}

int pool_check(const std::string& pre, const grpg_detector_layer_f16& L) {
  if (!L.in || !L.out) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL in / out");
  if (L.out_f32) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the pool writes fp16: out_f32 must be 0");
  if (misaligned(L.in, 2) || misaligned(L.out, 2)) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "in and out must be 2-byte aligned");
  if (L.bs < 1 || L.c_in < 1 || L.h_in < 1 || L.w_in < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "sizes must be positive");
  if (L.c_out != 3 * (long long)L.c_in || L.h_out != L.h_in || L.w_out != L.w_in)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the pool writes 3 * c_in channels of the input's size");
  if (L.bs > 65535 || L.c_in > 65535) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "bs and c_in must be below 65536");
  if (!slice_ok(L.in_c0, L.c_in, L.in_ct) || !slice_ok(L.out_c0, L.c_out, L.out_ct))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the input or output slice leaves its tensor");
  if (!extent_ok(L.bs, L.in_ct, L.h_in, L.w_in) || !extent_ok(L.bs, L.out_ct, L.h_in, L.w_in))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "tensor too large for one launch");
  if (L.out == L.in && (L.in_ct != L.out_ct || (L.in_c0 < L.out_c0 + L.c_out && L.out_c0 < L.in_c0 + L.c_in)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "inside one tensor the pool's input and output slices must not overlap");
  return GRPG_OK;
}

template <int BM, int BN>
void conv_launch(const Conv16Args& a, const int k, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + BN - 1) / BN), (unsigned)((a.c_out + BM - 1) / BM));
  if (k == 1) conv_f16_kernel<BM, BN, 1><<<grid, DET16_THREADS, 0, st>>>(a);
  else conv_f16_kernel<BM, BN, 3><<<grid, DET16_THREADS, 0, st>>>(a);
}

void enqueue(const grpg_detector_layer_f16& L, hipStream_t st) {
  if (L.kind == GRPG_DET_CONV) {
    Conv16Args a;
    a.in = static_cast<const uint16_t*>(L.in); a.out = L.out;
    a.res = static_cast<const _Float16*>(L.res); a.up = static_cast<_Float16*>(L.up); a.packed = L.packed;
    a.in_c0 = L.in_c0; a.in_ct = L.in_ct; a.out_c0 = L.out_c0; a.out_ct = L.out_ct;
    a.res_c0 = L.res_c0; a.res_ct = L.res_ct; a.up_c0 = L.up_c0; a.up_ct = L.up_ct;
    a.bs = L.bs; a.c_in = L.c_in; a.c_out = L.c_out; a.h_in = L.h_in; a.w_in = L.w_in; a.h_out = L.h_out; a.w_out = L.w_out;
    a.stride = L.stride; a.act = L.act == GRPG_DET_ACT_SILU; a.focus = L.in_mode == GRPG_DET_IN_FOCUS; a.out_f32 = L.out_f32;
    a.K = L.c_in * L.k * L.k;
    a.m_pad = round_up(L.c_out, DET16_MPAD);
    a.k_pad = round_up(a.K, DET16_BK);
    a.N = L.bs * L.h_out * L.w_out;
    if (L.tile == GRPG_DET_TILE_128) conv_launch<128, 128>(a, L.k, st);
    else conv_launch<64, 64>(a, L.k, st);
  } else {
    Pool16Args a;
    a.in = static_cast<const _Float16*>(L.in); a.out = static_cast<_Float16*>(L.out);
    a.in_c0 = L.in_c0; a.in_ct = L.in_ct; a.out_c0 = L.out_c0; a.out_ct = L.out_ct;
    a.bs = L.bs; a.c = L.c_in; a.h = L.h_in; a.w = L.w_in;
    a.tiles_x = (L.w_in + SPP_T - 1) / SPP_T;
    const dim3 grid((unsigned)(a.tiles_x * ((L.h_in + SPP_T - 1) / SPP_T)), (unsigned)L.c_in, (unsigned)L.bs);
    spp_f16_kernel<<<grid, DET16_THREADS, 0, st>>>(a);
  }
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_conv2d_packed_bytes_f16(int c_out, int c_in, int k) {
  if (c_out < 1 || c_in < 1 || (k != 1 && k != 3) || (long long)c_in * k * k >= (1ll << 24) || c_out > (1 << 24)) return 0;
  const size_t m_pad = (size_t)round_up(c_out, DET16_MPAD);
  return sizeof(float) * m_pad + sizeof(uint16_t) * m_pad * (size_t)round_up(c_in * k * k, DET16_BK);
}

int grpg_conv2d_pack_weights_f16(const float* weight, const float* bias, int c_out, int c_in, int k, void* packed,
                                 void* hip_stream) {
  fail(GRPG_OK, "");
  if (!weight || !packed) return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights_f16: NULL weight / packed");
  if (misaligned(weight, 4) || misaligned(bias, 4) || ((uintptr_t)packed & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights_f16: weight and bias must be 4-byte, packed 16-byte aligned");
  const size_t bytes = grpg_conv2d_packed_bytes_f16(c_out, c_in, k);
  if (!bytes) return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights_f16: c_out, c_in must be positive and k 1 or 3");
  if (int rc = begin_call()) return rc;
  const int K = c_in * k * k, m_pad = round_up(c_out, DET16_MPAD), k_pad = round_up(K, DET16_BK);
  const size_t total = (size_t)m_pad * ((size_t)k_pad + 1);
  pack_f16_kernel<<<(unsigned)((total + DET16_THREADS - 1) / DET16_THREADS), DET16_THREADS, 0, (hipStream_t)hip_stream>>>(
      weight, bias, c_out, K, m_pad, k_pad, packed);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_detector_run_f16(const grpg_detector_layer_f16* layers, int n, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!layers || n < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "detector_run_f16: NULL layers or n < 1");
  for (int i = 0; i < n; i++) {   // every check before the first launch
    const std::string pre = "detector_run_f16: layer " + std::to_string(i) + ": ";
    int rc;
    if (layers[i].kind == GRPG_DET_CONV) rc = conv_check(pre, layers[i]);
    else if (layers[i].kind == GRPG_DET_POOL) rc = pool_check(pre, layers[i]);
    else rc = fail(GRPG_ERR_INVALID_ARGUMENT, pre + "unknown kind");
    if (rc) return rc;
  }
  if (int rc = begin_call()) return rc;
  for (int i = 0; i < n; i++) {
    enqueue(layers[i], (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
  }
  return GRPG_OK;
}

}  // extern "C"
