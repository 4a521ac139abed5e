// The detector's network for gfx950: the inference forward of the reference's YOLOv5 (models/yolo.py:119-159 over
// models/common.py: Focus, Conv, Bottleneck, C3, SPP, nn.Upsample, Concat, and Detect's 1x1 convs), FP32 over NCHW,
// as a list of launches of TWO kernels.  No atomics, no split-K: identical calls give identical bits.
//
// conv_kernel<BM, BN, KS>: an implicit GEMM, M = C_out, N = bs * H_out * W_out, K = C_in * k * k, on
// v_mfma_f32_32x32x2_f32 -- exact f32, a k-ordered fma chain per output element.  Everything the reference does
// around a convolution is an address mode or an epilogue of it:
//   input    a channel slice [c0, c0 + C_in) of a wider tensor; GRPG_DET_IN_FOCUS reads Focus's four strided slices
//            (common.py:175) of the stored image: logical channel blk * C + c is stored channel c at
//            (2 y + (blk & 1), 2 x + (blk >> 1)) -- (even row, even col), (odd, even), (even, odd), (odd, odd);
//   chain    k = (ci * KS + ky) * KS + kx, the weight tensor's own order, in blocks of DET_KBLOCK = 32: a block's
//            partial sum is the fma chain p = 0; p = fma(w_k, x_k, p) for its k ascending, and the output is the
//            chain acc = bias; acc = acc + p for the blocks ascending.  An element's rounding error then grows
//            with 32 + K / 32 roundings instead of K (K = 4608 in the widest 3 x 3 layer): measured on the
//            narrowed model, one plain chain of K lay up to 7 x further from float64 than the reference's
//            blocked CPU convolution, this one 1.4 x.  Padded taps multiply zeros.  Both
//            tile shapes run this order: same bits;
//   epilogue SiLU x * (1 / (1 + expf(-x))) (correctly rounded division), then + residual (Bottleneck's
//            x + cv2(cv1(x)), in that order), then the store into a channel slice of a wider tensor -- Concat and
//            C3's cat are the producers writing into the consumer's buffer -- and, optionally, a second store that
//            replicates every value 2 x 2 into a slice of a tensor of twice the size: nn.Upsample(2, 'nearest').
// Tiles: 128 x 128 (four waves, each 2 x 2 MFMA tiles of 32 x 32) and 64 x 64 (each one tile), both 16 deep; the
// plan picks one per layer.  A (weights) comes from a buffer repacked once (pack_kernel): [bias M_pad][K_pad][M_pad]
// with M_pad a multiple of 128, K_pad of 16 and zeros in the padding, so the A tile is unguarded 16-byte loads.
// B (the im2col gather) is one guarded scalar load per element, lanes along the pixels.  Both tiles go global ->
// registers -> LDS with the next tile's loads issued before the current tile's MFMAs.  LDS rows are k, padded by
// 32 floats: the operand read of lane l, row k0 + (l >> 5), column (l & 31), has its two half-waves on disjoint
// banks.
//
// spp_kernel: SPP's 5 / 9 / 13 max-pools (common.py:160-164; stride 1, -inf padding) of one slice into three
// slices in one launch: a 16 x 16 output tile with its 6-pixel halo in LDS, a row pass and a column pass.  max is
// exact and associative, so the bits are nn.MaxPool2d's; NaN propagates as there.
#include <cmath>
#include <cstdint>

#include "abi_util.h"
#include "common.h"

namespace grpg {

namespace {

constexpr int DET_THREADS = 256;
constexpr int DET_BK = 16;
constexpr int DET_KBLOCK = 32;  // k per partial sum (the rounding order); a multiple of DET_BK
constexpr int DET_MPAD = 128;   // packed weights: C_out rounded up to this, for either tile
constexpr int DET_LDS_PAD = 32;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ConvArgs {
  const float* in;
  float* out;
  const float* res;
  float* up;
  const float* packed;
  int in_c0, in_ct, out_c0, out_ct, res_c0, res_ct, up_c0, up_ct;
  int bs, c_in, c_out, h_in, w_in, h_out, w_out;   // h_in, w_in: the stored tensor's
  int stride, act, focus;
  int K, m_pad, N;
};

__host__ __device__ inline int round_up(const int v, const int m) { return (v + m - 1) / m * m; }

// rows m of the C/D registers of v_mfma_f32_32x32x2_f32: column lane & 31, row below
__device__ __forceinline__ int cd_row(const int reg, const int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float silu(const float x) { return x * (1.0f / (1.0f + expf(-x))); }

// Registers: the 128 x 128 shape holds 2 x 64 accumulator registers (sum and partial sum) and is allocated for two
// waves per SIMD, the 64 x 64 shape 2 x 16 for four (tests/test_detector_resources.py).
template <int BM, int BN, int KS>
__global__ void __launch_bounds__(DET_THREADS, BM == 128 ? 2 : 4) conv_kernel(const ConvArgs a) {
  constexpr int TM = BM / 64, TN = BN / 64;          // MFMA tiles per wave
  constexpr int LDA = BM + DET_LDS_PAD, LDB = BN + DET_LDS_PAD;
  constexpr int A_VEC = DET_BK * BM / 4 / DET_THREADS;   // float4 loads per thread and tile
  constexpr int B_ROWS = DET_THREADS / BN;               // k rows covered per pass
  constexpr int B_PER = DET_BK / B_ROWS;                 // elements per thread and tile
  static_assert(A_VEC >= 1 && B_PER >= 1, "tile too small for the block");
  __shared__ __attribute__((aligned(16))) float As[DET_BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[DET_BK * LDB];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;                    // N < 2^31 - BN (conv_check)

  // ---- this thread's column of the B tile: one output pixel ----
  const int bn = t % BN, bk0 = t / BN;
  const int n = n0 + bn;
  const bool n_ok = n < a.N;
  int iy0 = 0, ix0 = 0;
  const float* in_b = a.in;
  const size_t in_plane = (size_t)a.h_in * a.w_in;
  const int lh = a.focus ? a.h_in >> 1 : a.h_in, lw = a.focus ? a.w_in >> 1 : a.w_in;   // logical input plane
  const int cs = a.focus ? a.c_in >> 2 : a.c_in;                                        // stored channels read
  if (n_ok) {
    const int hw = a.h_out * a.w_out;
    const int b = n / hw, r = n - b * hw;
    const int oy = r / a.w_out, ox = r - oy * a.w_out;
    iy0 = oy * a.stride - KS / 2;
    ix0 = ox * a.stride - KS / 2;
    in_b += ((size_t)b * a.in_ct + a.in_c0) * in_plane;
  }
  auto load_b = [&](const int k) -> float {
    if (!n_ok || k >= a.K) return 0.0f;
    const int ci = k / (KS * KS), rr = k - ci * (KS * KS);
    const int ky = rr / KS, kx = rr - ky * KS;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= lh || ix < 0 || ix >= lw) return 0.0f;
    if (a.focus) {
      const int blk = ci / cs, c = ci - blk * cs;
      return in_b[(size_t)c * in_plane + (size_t)(2 * iy + (blk & 1)) * a.w_in + (2 * ix + (blk >> 1))];
    }
    return in_b[(size_t)ci * in_plane + (size_t)iy * a.w_in + ix];
  };
  const float* wp = a.packed + a.m_pad;              // behind the bias
  auto load_a = [&](const int k0, const int v) -> f32x4 {
    const int e = v * DET_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
    return *reinterpret_cast<const f32x4*>(wp + (size_t)(k0 + kr) * a.m_pad + m0 + mc);   // k0 + kr < K_pad
  };

  // ---- the sum of the blocks starts at the bias, every block's partial sum at zero ----
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  f32x16 acc[TM][TN], part[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float bias = a.packed[m0 + wm + i * 32 + cd_row(r, lane)];   // < m_pad: padded with zeros
#pragma unroll
      for (int j = 0; j < TN; j++) {
        acc[i][j][r] = bias;
        part[i][j][r] = 0.0f;
      }
    }

  const int k_tiles = (a.K + DET_BK - 1) / DET_BK;
  f32x4 ra[A_VEC];
  float rb[B_PER];
#pragma unroll
  for (int v = 0; v < A_VEC; v++) ra[v] = load_a(0, v);
#pragma unroll
  for (int v = 0; v < B_PER; v++) rb[v] = load_b(bk0 + v * B_ROWS);

  for (int kt = 0; kt < k_tiles; kt++) {
#pragma unroll
    for (int v = 0; v < A_VEC; v++) {
      const int e = v * DET_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
      *reinterpret_cast<f32x4*>(&As[kr * LDA + mc]) = ra[v];
    }
#pragma unroll
    for (int v = 0; v < B_PER; v++) Bs[(bk0 + v * B_ROWS) * LDB + bn] = rb[v];
    __syncthreads();
    if (kt + 1 < k_tiles) {
      const int k0 = (kt + 1) * DET_BK;
#pragma unroll
      for (int v = 0; v < A_VEC; v++) ra[v] = load_a(k0, v);
#pragma unroll
      for (int v = 0; v < B_PER; v++) rb[v] = load_b(k0 + bk0 + v * B_ROWS);
    }
#pragma unroll
    for (int kk = 0; kk < DET_BK; kk += 2) {
      const int row = kk + (lane >> 5), col = lane & 31;
      float fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) fa[i] = As[row * LDA + wm + i * 32 + col];
#pragma unroll
      for (int j = 0; j < TN; j++) fb[j] = Bs[row * LDB + wn + j * 32 + col];
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          part[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], part[i][j], 0, 0, 0);
    }
    if ((kt + 1) % (DET_KBLOCK / DET_BK) == 0 || kt + 1 == k_tiles) {   // the block is complete
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
          acc[i][j] += part[i][j];
          part[i][j] = (f32x16)(0.0f);
        }
    }
    __syncthreads();
  }

  // ---- epilogue: activation, residual, the store(s) ----
  const size_t out_plane = (size_t)a.h_out * a.w_out;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int nn = n0 + wn + j * 32 + (lane & 31);
    if (nn >= a.N) continue;
    const int hw = a.h_out * a.w_out;
    const int b = nn / hw, r = nn - b * hw;
    const int oy = r / a.w_out, ox = r - oy * a.w_out;
    float* out_p = a.out + ((size_t)b * a.out_ct + a.out_c0) * out_plane + r;
    const float* res_p = a.res ? a.res + ((size_t)b * a.res_ct + a.res_c0) * out_plane + r : nullptr;
    float* up_p = a.up ? a.up + ((size_t)b * a.up_ct + a.up_c0) * (4 * out_plane) + (size_t)(2 * oy) * (2 * a.w_out) + 2 * ox
                       : nullptr;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int rg = 0; rg < 16; rg++) {
        const int m = m0 + wm + i * 32 + cd_row(rg, lane);
        if (m >= a.c_out) continue;
        float v = acc[i][j][rg];
        if (a.act) v = silu(v);
        if (res_p) v = res_p[(size_t)m * out_plane] + v;
        out_p[(size_t)m * out_plane] = v;
        if (up_p) {
          float* u = up_p + (size_t)m * (4 * out_plane);
          u[0] = v;
          u[1] = v;
          u[2 * a.w_out] = v;
          u[2 * a.w_out + 1] = v;
        }
      }
  }
}

// OIHW weights + bias -> [bias m_pad][k_pad][m_pad], zeros in the padding; one thread per packed float.
__global__ void __launch_bounds__(DET_THREADS)
pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, const int c_out, const int K, const int m_pad,
            const int k_pad, float* __restrict__ packed) {
  const size_t i = (size_t)blockIdx.x * DET_THREADS + threadIdx.x;
  const size_t total = (size_t)m_pad * (k_pad + 1);
  if (i >= total) return;
  const int m = (int)(i % m_pad);
  const long long k = (long long)(i / m_pad) - 1;
  float v = 0.0f;
  if (m < c_out) {
    if (k < 0) v = bias ? bias[m] : 0.0f;
    else if (k < K) v = w[(size_t)m * K + k];
  }
  packed[i] = v;
}

// ---- SPP ----
constexpr int SPP_T = 16, SPP_HALO = 6, SPP_S = SPP_T + 2 * SPP_HALO;   // 28

struct PoolArgs {
  const float* in;
  float* out;
  int in_c0, in_ct, out_c0, out_ct;
  int bs, c, h, w, tiles_x;
};

// max as nn.MaxPool2d takes it: NaN wins
__device__ __forceinline__ float max_nan(const float m, const float v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(DET_THREADS) spp_kernel(const PoolArgs a) {
  __shared__ float tile[SPP_S][SPP_S + 1];
  __shared__ float rows[3][SPP_S][SPP_T + 1];
  const int t = threadIdx.x;
  const int ty0 = (blockIdx.x / a.tiles_x) * SPP_T, tx0 = (blockIdx.x % a.tiles_x) * SPP_T;
  const int c = blockIdx.y, b = blockIdx.z;
  const size_t plane = (size_t)a.h * a.w;
  const float* src = a.in + ((size_t)b * a.in_ct + a.in_c0 + c) * plane;
  for (int e = t; e < SPP_S * SPP_S; e += DET_THREADS) {
    const int ly = e / SPP_S, lx = e - ly * SPP_S;
    const int y = ty0 + ly - SPP_HALO, x = tx0 + lx - SPP_HALO;
    tile[ly][lx] = (y >= 0 && y < a.h && x >= 0 && x < a.w) ? src[(size_t)y * a.w + x] : -INFINITY;
  }
  __syncthreads();
  for (int e = t; e < SPP_S * SPP_T; e += DET_THREADS) {
    const int ly = e / SPP_T, lx = e - ly * SPP_T;   // output column lx: centre at tile column lx + 6
    float m = tile[ly][lx + SPP_HALO];
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
    float m = rows[p][ly + SPP_HALO][lx];
    for (int d = 1; d <= rad; d++) m = max_nan(max_nan(m, rows[p][ly + SPP_HALO - d][lx]), rows[p][ly + SPP_HALO + d][lx]);
    a.out[((size_t)b * a.out_ct + a.out_c0 + (size_t)p * a.c + c) * plane + (size_t)y * a.w + x] = m;
  }
}

// ---- checks and launches ----

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// [p, p + n) and [q, q + m) floats share memory
bool overlap(const float* p, const size_t n, const float* q, const size_t m) {
  return (uintptr_t)p < (uintptr_t)(q + m) && (uintptr_t)q < (uintptr_t)(p + n);
}

// [c0, c0 + c) inside [0, ct)
bool slice_ok(const int c0, const int c, const int ct) { return c0 >= 0 && c >= 1 && ct >= 1 && (long long)c0 + c <= ct; }

// bs * ct * h * w floats must stay addressable and the launch's n below 2^31
bool extent_ok(const int bs, const int ct, const int h, const int w) {
  return (long long)bs * ct * h * w < (1ll << 40) && (long long)bs * h * w < (1ll << 31) - 256;
}

int conv_check(const std::string& pre, const grpg_detector_layer& L) {
  if (!L.in || !L.out || !L.packed) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL in / out / packed");
  if (misaligned(L.in) || misaligned(L.out) || misaligned(L.res) || misaligned(L.up))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "in, out, res and up must be 4-byte aligned");
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
  const size_t n_in = (size_t)L.bs * L.in_ct * L.h_in * L.w_in, n_out = (size_t)L.bs * L.out_ct * L.h_out * L.w_out;
  const size_t n_res = (size_t)L.bs * L.res_ct * L.h_out * L.w_out, n_up = 4 * (size_t)L.bs * L.up_ct * L.h_out * L.w_out;
  if (overlap(L.out, n_out, L.in, n_in) || (L.res && overlap(L.out, n_out, L.res, n_res)) ||
      (L.up && (overlap(L.up, n_up, L.in, n_in) || overlap(L.up, n_up, L.out, n_out) ||
                (L.res && overlap(L.up, n_up, L.res, n_res)))))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "a convolution cannot write a tensor it reads (or one tensor twice)");
  return GRPG_OK;
}

int pool_check(const std::string& pre, const grpg_detector_layer& L) {
  if (!L.in || !L.out) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL in / out");
  if (misaligned(L.in) || misaligned(L.out)) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "in and out must be 4-byte aligned");
  if (L.bs < 1 || L.c_in < 1 || L.h_in < 1 || L.w_in < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "sizes must be positive");
  if (L.c_out != 3 * (long long)L.c_in || L.h_out != L.h_in || L.w_out != L.w_in)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the pool writes 3 * c_in channels of the input's size");
  if (L.bs > 65535 || L.c_in > 65535) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "bs and c_in must be below 65536");
  if (!slice_ok(L.in_c0, L.c_in, L.in_ct) || !slice_ok(L.out_c0, L.c_out, L.out_ct))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "the input or output slice leaves its tensor");
  if (!extent_ok(L.bs, L.in_ct, L.h_in, L.w_in) || !extent_ok(L.bs, L.out_ct, L.h_in, L.w_in))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "tensor too large for one launch");
  if ((const float*)L.out == L.in &&
      (L.in_ct != L.out_ct || (L.in_c0 < L.out_c0 + L.c_out && L.out_c0 < L.in_c0 + L.c_in)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "inside one tensor the pool's input and output slices must not overlap");
  return GRPG_OK;
}

template <int BM, int BN>
void conv_launch(const ConvArgs& a, const int k, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + BN - 1) / BN), (unsigned)((a.c_out + BM - 1) / BM));
  if (k == 1) conv_kernel<BM, BN, 1><<<grid, DET_THREADS, 0, st>>>(a);
  else conv_kernel<BM, BN, 3><<<grid, DET_THREADS, 0, st>>>(a);
}

void enqueue(const grpg_detector_layer& L, hipStream_t st) {
  if (L.kind == GRPG_DET_CONV) {
    ConvArgs a;
    a.in = L.in; a.out = L.out; a.res = L.res; a.up = L.up; a.packed = L.packed;
    a.in_c0 = L.in_c0; a.in_ct = L.in_ct; a.out_c0 = L.out_c0; a.out_ct = L.out_ct;
    a.res_c0 = L.res_c0; a.res_ct = L.res_ct; a.up_c0 = L.up_c0; a.up_ct = L.up_ct;
    a.bs = L.bs; a.c_in = L.c_in; a.c_out = L.c_out; a.h_in = L.h_in; a.w_in = L.w_in; a.h_out = L.h_out; a.w_out = L.w_out;
    a.stride = L.stride; a.act = L.act == GRPG_DET_ACT_SILU; a.focus = L.in_mode == GRPG_DET_IN_FOCUS;
    a.K = L.c_in * L.k * L.k;
    a.m_pad = round_up(L.c_out, DET_MPAD);
    a.N = L.bs * L.h_out * L.w_out;
    if (L.tile == GRPG_DET_TILE_128) conv_launch<128, 128>(a, L.k, st);
    else conv_launch<64, 64>(a, L.k, st);
  } else {
    PoolArgs a;
    a.in = L.in; a.out = L.out;
    a.in_c0 = L.in_c0; a.in_ct = L.in_ct; a.out_c0 = L.out_c0; a.out_ct = L.out_ct;
    a.bs = L.bs; a.c = L.c_in; a.h = L.h_in; a.w = L.w_in;
    a.tiles_x = (L.w_in + SPP_T - 1) / SPP_T;
    const dim3 grid((unsigned)(a.tiles_x * ((L.h_in + SPP_T - 1) / SPP_T)), (unsigned)L.c_in, (unsigned)L.bs);
    spp_kernel<<<grid, DET_THREADS, 0, st>>>(a);
  }
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_conv2d_packed_bytes(int c_out, int c_in, int k) {
  if (c_out < 1 || c_in < 1 || (k != 1 && k != 3) || (long long)c_in * k * k >= (1ll << 24) || c_out > (1 << 24)) return 0;
  return sizeof(float) * (size_t)round_up(c_out, DET_MPAD) * (size_t)(round_up(c_in * k * k, DET_BK) + 1);
}

int grpg_conv2d_pack_weights(const float* weight, const float* bias, int c_out, int c_in, int k, float* packed,
                             void* hip_stream) {
  fail(GRPG_OK, "");
  if (!weight || !packed) return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights: NULL weight / packed");
  if (misaligned(weight) || misaligned(bias) || ((uintptr_t)packed & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights: weight and bias must be 4-byte, packed 16-byte aligned");
  const size_t bytes = grpg_conv2d_packed_bytes(c_out, c_in, k);
  if (!bytes) return fail(GRPG_ERR_INVALID_ARGUMENT, "conv2d_pack_weights: c_out, c_in must be positive and k 1 or 3");
  if (int rc = begin_call()) return rc;
  const int K = c_in * k * k, m_pad = round_up(c_out, DET_MPAD), k_pad = round_up(K, DET_BK);
  const size_t total = bytes / sizeof(float);
  pack_kernel<<<(unsigned)((total + DET_THREADS - 1) / DET_THREADS), DET_THREADS, 0, (hipStream_t)hip_stream>>>(
      weight, bias, c_out, K, m_pad, k_pad, packed);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_detector_run(const grpg_detector_layer* layers, int n, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!layers || n < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "detector_run: NULL layers or n < 1");
  for (int i = 0; i < n; i++) {   // every check before the first launch
    const std::string pre = "detector_run: layer " + std::to_string(i) + ": ";
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
