// The backward of LPIPS (lpips.hip) for gfx950: d sum_p grad_pairs[p] * distances(x, y)[p] / d x, the gradient with
// respect to the rendered images only, FP32 over NCHW, as a list of launches of THREE kinds of kernel behind a forward
// that kept its activations (grpg_lpips_forward_train).  No atomics, no split-K: identical calls give identical bits.
// Only the x images run: y's features enter as constants of the distance.
//
// The chain carries, per convolution, the gradient with respect to its PRE-activation: wherever a kernel stores a
// gradient that lands on a ReLU's output (a kept activation `act`), the store is
//     act > 0 ? acc + tap_gradient : 0
// -- a select, not a product, as torch's threshold_backward: a non-finite value upstream cannot leak through a dead
// activation.  tap_gradient is the distance's own gradient where that activation is a tap.  No stand-alone elementwise
// launch exists.
//
// lpips_bwd_conv_kernel<BM, BN, KS> (stride 1, KS in {3, 5}): convolution backward-data as lpips_conv_kernel's implicit
// GEMM, M = C_in, N = images * H_in * W_in, K = C_out * k * k, on v_mfma_f32_32x32x2_f32.
//   chain    k = (co * KS + ky) * KS + kx ascending in blocks of LB_KBLOCK = 32: a block's partial sum is the fma chain
//            p = 0; p = fma(w[co][ci][ky][kx], g[co][y + pad - ky][x + pad - kx], p), and the sum is acc = 0;
//            acc = acc + p for the blocks ascending.  Taps outside the gradient's plane multiply zeros.  Both tile
//            shapes (128 x 128, 64 x 64) run this order: same bits;
//   epilogue the select above if `act` is given (then `tap` may be), acc / std_c if the produced gradient is the
//            image's (the z-score's derivative: one correctly rounded division), else acc.
// A is a SECOND packed layout of the layer's OIHW weights, made once per model by lpips_bwd_pack_kernel:
// [K_pad][M_pad], M_pad = C_in rounded up to 128, K_pad to 16, zeros in the padding.
//
// lpips_bwd_conv_strided_kernel<11, 4>: AlexNet's first layer (k 11, stride 4, pad 2, 64 -> 3 channels).  Not on the
// matrix pipe: three output channels would fill 3 of a tile's 64 rows, and the taps that reach an input pixel depend on
// its phase (y % 4, x % 4).  One thread per input pixel and all (at most 4) channels; a workgroup's pixels share ONE
// phase (blockIdx.y), so the enumerated taps -- those with (y + pad - ky) % 4 == 0, at most 3 x 3 per output channel of
// the 121 -- and their weights are uniform over the wave: the weights come through the scalar cache, the gradient
// loads are contiguous along x / 4.
//   chain    acc = 0; acc = fma(w, g, acc) over co ascending, then ky ascending, then kx ascending, of the enumerated
//            taps; a tap outside the gradient's plane multiplies zero.  A row or column under no window enumerates only
//            such taps: exactly 0;
//   epilogue as above.  Weights: [C_out * k * k][4] (the channel innermost, zero padded).
//
// lpips_bwd_pool_kernel: MaxPool2d(3, 2) / (2, 2) in gather form.  One thread per pool-INPUT element; it visits the at
// most 2 x 2 windows that cover it, rows then columns ascending, recomputes each window's winner from the kept
// activation -- the FIRST maximum in row-major order, F.max_pool2d's -- and adds the gradients of the windows it won,
// in that order, from 0; then the select above.  An element with act > 0 false is 0 without visiting anything.
//
// lpips_bwd_distance_kernel: one tap, lpips_distance_kernel's layout (a workgroup loads its pixels' C channels of x and
// y once into LDS).  With nx = sqrtf(sum_c x_c^2) and a_c = x_c / (nx + eps) exactly as the forward computes them,
//   q_c = (2 w_c) * (a_c - b_c);   dot = sum_c q_c x_c (an fma chain, c ascending);
//   coef = nx > 0 ? dot / (((nx + eps) * (nx + eps)) * nx) : 0      -- the norm's derivative at 0 is defined as 0;
//   g_c = (grad_pair / (H_l W_l)) * (q_c / (nx + eps) - x_c * coef);   stored: x_c > 0 ? g_c : 0
// -- a tap is a ReLU's output, so its gradient passes the ReLU's select here; for the last tap this IS the last
// convolution's pre-activation gradient.  Written for the x images only.
//
// Launches of grpg_lpips_backward: one per convolution, pool and tap -- 5 + 2 + 5 = 12 for AlexNet, 13 + 4 + 5 = 22 for
// VGG16.  A tap's gradient is enqueued right before the kernel that adds it, into one shared buffer.
#include <cmath>
#include <cstdint>
#include <string>

#include "abi_util.h"
#include "common.h"
#include "lpips_train.h"

namespace grpg {

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_BK = 16;
constexpr int LB_KBLOCK = 32;   // k per partial sum (the rounding order); a multiple of LB_BK
constexpr int LB_MPAD = 128;    // packed weights: C_in rounded up to this, for either tile
constexpr int LB_LDS_PAD = 32;
constexpr int LB_MAX_C = 768;
constexpr float LB_EPS = 1e-10f;
constexpr float LB_STD[3] = {.458f, .448f, .450f};   // BaseNet's buffer (networks.py:44)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// what a store of a produced gradient does besides storing
struct Epilogue {
  const float* act;   // the kept ReLU output the gradient lands on, or NULL
  const float* tap;   // that activation's own gradient from the distance, or NULL (only with act)
  int zs;             // the produced gradient is the image's: divide by std_c
  float std0, std1, std2;
};

__device__ __forceinline__ float finish(const Epilogue& e, const float acc, const size_t idx, const int c) {
  if (e.act) return e.act[idx] > 0.0f ? (e.tap ? acc + e.tap[idx] : acc) : 0.0f;
  if (e.zs) return acc / (c == 0 ? e.std0 : c == 1 ? e.std1 : e.std2);
  return acc;
}

struct BwdConvArgs {
  const float* gout;     // [bs, c_out, h_out, w_out]: the gradient of the convolution's pre-activation
  const float* packed;   // the backward layout
  float* gin;            // [bs, c_in, h_in, w_in]
  Epilogue e;
  int bs, c_in, c_out, h_in, w_in, h_out, w_out, pad;
  int K, m_pad, N;
};

__host__ __device__ inline int round_up(const int v, const int m) { return (v + m - 1) / m * m; }

// rows m of the C/D registers of v_mfma_f32_32x32x2_f32: column lane & 31, row below
__device__ __forceinline__ int cd_row(const int reg, const int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Registers and LDS: lpips_conv_kernel's -- the 128 x 128 shape is allocated for two workgroups per SIMD, the 64 x 64
// shape for four; two 16-deep tiles with rows padded by 32 floats (tests/test_lpips_bwd_resources.py).
template <int BM, int BN, int KS>
__global__ void __launch_bounds__(LB_THREADS, BM == 128 ? 2 : 4) lpips_bwd_conv_kernel(const BwdConvArgs a) {
  constexpr int TM = BM / 64, TN = BN / 64;          // MFMA tiles per wave
  constexpr int LDA = BM + LB_LDS_PAD, LDB = BN + LB_LDS_PAD;
  constexpr int A_VEC = LB_BK * BM / 4 / LB_THREADS;   // float4 loads per thread and tile
  constexpr int B_ROWS = LB_THREADS / BN;              // k rows covered per pass
  constexpr int B_PER = LB_BK / B_ROWS;                // elements per thread and tile
  static_assert(A_VEC >= 1 && B_PER >= 1, "tile too small for the block");
  __shared__ __attribute__((aligned(16))) float As[LB_BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[LB_BK * LDB];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;                    // N < 2^31 - 256 (the entry points check)

  // ---- this thread's column of the B tile: one input pixel ----
  const int bn = t % BN, bk0 = t / BN;
  const int n = n0 + bn;
  const bool n_ok = n < a.N;
  int oy0 = 0, ox0 = 0;
  const float* g_b = a.gout;
  const size_t g_plane = (size_t)a.h_out * a.w_out;
  if (n_ok) {
    const int hw = a.h_in * a.w_in;
    const int b = n / hw, r = n - b * hw;
    const int y = r / a.w_in, x = r - y * a.w_in;
    oy0 = y + a.pad;
    ox0 = x + a.pad;
    g_b = a.gout + (size_t)b * a.c_out * g_plane;
  }
  auto load_b = [&](const int k) -> float {
    if (!n_ok || k >= a.K) return 0.0f;
    const int co = k / (KS * KS), rr = k - co * (KS * KS);
    const int ky = rr / KS, kx = rr - ky * KS;
    const int oy = oy0 - ky, ox = ox0 - kx;
    if (oy < 0 || oy >= a.h_out || ox < 0 || ox >= a.w_out) return 0.0f;
    return g_b[(size_t)co * g_plane + (size_t)oy * a.w_out + ox];
  };
  auto load_a = [&](const int k0, const int v) -> f32x4 {
    const int e = v * LB_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
    return *reinterpret_cast<const f32x4*>(a.packed + (size_t)(k0 + kr) * a.m_pad + m0 + mc);   // k0 + kr < K_pad
  };

  // ---- the sum of the blocks starts at zero, and so does every block's partial sum ----
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  f32x16 acc[TM][TN], part[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      acc[i][j] = (f32x16)(0.0f);
      part[i][j] = (f32x16)(0.0f);
    }

  const int k_tiles = (a.K + LB_BK - 1) / LB_BK;
  f32x4 ra[A_VEC];
  float rb[B_PER];
#pragma unroll
  for (int v = 0; v < A_VEC; v++) ra[v] = load_a(0, v);
#pragma unroll
  for (int v = 0; v < B_PER; v++) rb[v] = load_b(bk0 + v * B_ROWS);

  for (int kt = 0; kt < k_tiles; kt++) {
#pragma unroll
    for (int v = 0; v < A_VEC; v++) {
      const int e = v * LB_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
      *reinterpret_cast<f32x4*>(&As[kr * LDA + mc]) = ra[v];
    }
#pragma unroll
    for (int v = 0; v < B_PER; v++) Bs[(bk0 + v * B_ROWS) * LDB + bn] = rb[v];
    __syncthreads();
    if (kt + 1 < k_tiles) {
      const int k0 = (kt + 1) * LB_BK;
#pragma unroll
      for (int v = 0; v < A_VEC; v++) ra[v] = load_a(k0, v);
#pragma unroll
      for (int v = 0; v < B_PER; v++) rb[v] = load_b(k0 + bk0 + v * B_ROWS);
    }
#pragma unroll
    for (int kk = 0; kk < LB_BK; kk += 2) {
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
    if ((kt + 1) % (LB_KBLOCK / LB_BK) == 0 || kt + 1 == k_tiles) {   // the block is complete
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

  // ---- epilogue: the select (or the z-score's derivative) and the store ----
  const size_t in_plane = (size_t)a.h_in * a.w_in;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int nn = n0 + wn + j * 32 + (lane & 31);
    if (nn >= a.N) continue;
    const int hw = a.h_in * a.w_in;
    const int b = nn / hw, r = nn - b * hw;
    const size_t base = (size_t)b * a.c_in * in_plane + r;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int rg = 0; rg < 16; rg++) {
        const int m = m0 + wm + i * 32 + cd_row(rg, lane);
        if (m >= a.c_in) continue;
        const size_t idx = base + (size_t)m * in_plane;
        a.gin[idx] = finish(a.e, acc[i][j][rg], idx, m);
      }
  }
}

// The strided layer.  grid (ceil(Hq * Wq / 256), S * S phases, bs) with Hq = ceil(h_in / S), Wq = ceil(w_in / S): the
// thread's pixel is (yq * S + py, xq * S + px).  c_in <= 4.
template <int KS, int S>
__global__ void __launch_bounds__(LB_THREADS) lpips_bwd_conv_strided_kernel(const BwdConvArgs a) {
  constexpr int MT = (KS + S - 1) / S;               // taps per axis that can reach one pixel
  const int py = blockIdx.y / S, px = blockIdx.y - py * S, b = blockIdx.z;
  const int wq = (a.w_in + S - 1) / S, hq = (a.h_in + S - 1) / S;
  const int q = blockIdx.x * LB_THREADS + threadIdx.x;   // hq * wq < 2^31 - 256
  if (q >= hq * wq) return;
  const int yq = q / wq, xq = q - yq * wq;
  const int y = yq * S + py, x = xq * S + px;
  if (y >= a.h_in || x >= a.w_in) return;
  // the phase's taps: ky = ky0 + j * S reads row oy = oyb - j (uniform over the workgroup but for yq, xq)
  const int ky0 = (py + a.pad) % S, kx0 = (px + a.pad) % S;
  const int oyb = yq + (py + a.pad - ky0) / S, oxb = xq + (px + a.pad - kx0) / S;
  const size_t g_plane = (size_t)a.h_out * a.w_out;
  const float* g_b = a.gout + (size_t)b * a.c_out * g_plane;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int co = 0; co < a.c_out; co++) {
    const float* g_c = g_b + (size_t)co * g_plane;
#pragma unroll
    for (int jy = 0; jy < MT; jy++) {
      const int ky = ky0 + jy * S, oy = oyb - jy;
      if (ky >= KS) break;
#pragma unroll
      for (int jx = 0; jx < MT; jx++) {
        const int kx = kx0 + jx * S, ox = oxb - jx;
        if (kx >= KS) break;
        const bool in = oy >= 0 && oy < a.h_out && ox >= 0 && ox < a.w_out;
        const float g = in ? g_c[(size_t)oy * a.w_out + ox] : 0.0f;
        const f32x4 w = *reinterpret_cast<const f32x4*>(a.packed + (size_t)((co * KS + ky) * KS + kx) * 4);
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = fmaf(w[c], g, acc[c]);
      }
    }
  }
  const size_t in_plane = (size_t)a.h_in * a.w_in;
  const size_t base = (size_t)b * a.c_in * in_plane + (size_t)y * a.w_in + x;
#pragma unroll
  for (int c = 0; c < 4; c++)
    if (c < a.c_in) {
      const size_t idx = base + (size_t)c * in_plane;
      a.gin[idx] = finish(a.e, acc[c], idx, c);
    }
}

// OIHW weights -> the backward layouts, zeros in the padding; one thread per packed float.
//   strided == 0: [k_pad][m_pad], row k = (co * ks + ky) * ks + kx, column ci
//   strided == 1: [c_out * ks * ks][4], the same rows, ci < 4
__global__ void __launch_bounds__(LB_THREADS)
lpips_bwd_pack_kernel(const float* __restrict__ w, const int c_out, const int c_in, const int ks, const int m_pad,
                      const size_t total, float* __restrict__ packed) {
  const size_t i = (size_t)blockIdx.x * LB_THREADS + threadIdx.x;
  if (i >= total) return;
  const int ci = (int)(i % m_pad);
  const size_t k = i / m_pad;
  float v = 0.0f;
  if (ci < c_in && k < (size_t)c_out * ks * ks) {
    const int co = (int)(k / (ks * ks)), rr = (int)(k - (size_t)co * (ks * ks));
    v = w[((size_t)co * c_in + ci) * (ks * ks) + rr];
  }
  packed[i] = v;
}

struct BwdPoolArgs {
  const float* act;    // [planes, h, w]: the pool's input, a kept ReLU output
  const float* gout;   // [planes, ho, wo]
  const float* tap;    // [planes, h, w] or NULL
  float* gin;          // [planes, h, w]
  size_t total;
  int h, w, ho, wo, k;
};

__global__ void __launch_bounds__(LB_THREADS) lpips_bwd_pool_kernel(const BwdPoolArgs a) {
  const size_t i = (size_t)blockIdx.x * LB_THREADS + threadIdx.x;
  if (i >= a.total) return;
  const float v = a.act[i];
  if (!(v > 0.0f)) {                                 // the select: a dead (or NaN) activation passes nothing
    a.gin[i] = 0.0f;
    return;
  }
  const size_t hw = (size_t)a.h * a.w;
  const size_t plane = i / hw;
  const int r = (int)(i - plane * hw);
  const int y = r / a.w, x = r - y * a.w;
  const float* src = a.act + plane * hw;
  const float* g = a.gout + plane * ((size_t)a.ho * a.wo);
  // windows oy with 2 oy <= y <= 2 oy + k - 1
  const int oy_lo = y - (a.k - 1) <= 0 ? 0 : (y - (a.k - 1) + 1) / 2, oy_hi = min(y / 2, a.ho - 1);
  const int ox_lo = x - (a.k - 1) <= 0 ? 0 : (x - (a.k - 1) + 1) / 2, ox_hi = min(x / 2, a.wo - 1);
  float sum = 0.0f;
  for (int oy = oy_lo; oy <= oy_hi; oy++)
    for (int ox = ox_lo; ox <= ox_hi; ox++) {
      // the window's winner: the first maximum in row-major order (NaN wins, as in lpips_pool_kernel)
      float m = -INFINITY;
      int wy = -1, wx = -1;
      for (int dy = 0; dy < a.k; dy++)
        for (int dx = 0; dx < a.k; dx++) {
          const float c = src[(size_t)(2 * oy + dy) * a.w + 2 * ox + dx];   // 2 oy + k - 1 < h: floor mode
          if (c > m || c != c) { m = c; wy = 2 * oy + dy; wx = 2 * ox + dx; }
        }
      if (wy == y && wx == x) sum = sum + g[(size_t)oy * a.wo + ox];
    }
  a.gin[i] = a.tap ? sum + a.tap[i] : sum;
}

__host__ __device__ inline int distance_px(const int C) { return C <= 192 ? 32 : C <= 384 ? 16 : 8; }

// feat: [2 * pairs, C, hw]; x of pair p is image p, y image pairs + p.  grid (ceil(hw / px), pairs); dynamic LDS:
// 2 * C * px floats, xs[c * px + pixel] then ys likewise (ys is overwritten by q).
__global__ void __launch_bounds__(LB_THREADS)
lpips_bwd_distance_kernel(const float* __restrict__ feat, const float* __restrict__ lin,
                          const float* __restrict__ grad_pairs, const int pairs, const int C, const int hw, const int px,
                          float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) float lb_tile[];
  __shared__ float s_norm[64];
  __shared__ float s_coef[32];
  float* xs = lb_tile;
  float* ys = lb_tile + C * px;
  const int p = blockIdx.y, t = threadIdx.x;
  const int pix = t & (px - 1), row = t / px, rows = LB_THREADS / px;
  const int i = blockIdx.x * px + pix;                   // hw < 2^31 - 256
  const bool ok = i < hw;
  const float* x = feat + (size_t)p * C * hw + i;
  const float* y = feat + (size_t)(pairs + p) * C * hw + i;
  for (int c = row; c < C; c += rows) {
    xs[c * px + pix] = ok ? x[(size_t)c * hw] : 0.0f;
    ys[c * px + pix] = ok ? y[(size_t)c * hw] : 0.0f;
  }
  __syncthreads();
  if (t < 2 * px) {
    const float* src = t < px ? xs : ys;
    float sq = 0.0f;
    for (int c = 0; c < C; c++) {
      const float v = src[c * px + pix];
      sq = fmaf(v, v, sq);
    }
    s_norm[t] = sqrtf(sq);
  }
  __syncthreads();
  const float nx = s_norm[pix];
  const float nxe = nx + LB_EPS, nye = s_norm[px + pix] + LB_EPS;
  for (int c = row; c < C; c += rows) {
    const float d = xs[c * px + pix] / nxe - ys[c * px + pix] / nye;
    ys[c * px + pix] = (2.0f * lin[c]) * d;
  }
  __syncthreads();
  if (t < px) {
    float dot = 0.0f;
    for (int c = 0; c < C; c++) dot = fmaf(ys[c * px + pix], xs[c * px + pix], dot);
    s_coef[pix] = nx > 0.0f ? dot / ((nxe * nxe) * nx) : 0.0f;
  }
  __syncthreads();
  const float sc = grad_pairs[p] / (float)hw;
  const float coef = s_coef[pix];
  float* out = grad + (size_t)p * C * hw + i;
  for (int c = row; c < C; c += rows) {
    const float xv = xs[c * px + pix];
    const float g = sc * (ys[c * px + pix] / nxe - xv * coef);
    if (ok) out[(size_t)c * hw] = xv > 0.0f ? g : 0.0f;
  }
}

// the tile policy of lpips.hip's choose_tile, on the backward's M = c_in; the result does not depend on it
int choose_tile(const int c_in, const long long n) {
  return (c_in >= 96 && (long long)((c_in + 127) / 128) * ((n + 127) / 128) >= 256) ? GRPG_LPIPS_TILE_128 : GRPG_LPIPS_TILE_64;
}

bool strided_layer(const int k, const int stride) { return k == 11 && stride == 4; }
bool mfma_layer(const int k, const int stride) { return (k == 3 || k == 5) && stride == 1; }

template <int BM, int BN>
void conv_launch(const BwdConvArgs& a, const int k, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + BN - 1) / BN), (unsigned)((a.c_in + BM - 1) / BM));
  if (k == 3) lpips_bwd_conv_kernel<BM, BN, 3><<<grid, LB_THREADS, 0, st>>>(a);
  else lpips_bwd_conv_kernel<BM, BN, 5><<<grid, LB_THREADS, 0, st>>>(a);
}

// gout [bs, c_out, h_out, w_out] -> gin [bs, c_in, h_in, w_in]; the caller has checked the geometry
void conv_bwd_enqueue(const float* gout, const float* packed, float* gin, const float* act, const float* tap,
                      const float* sdev, const int bs, const int c_in, const int c_out, const int h_in, const int w_in,
                      const int k, const int stride, const int pad, const int tile, hipStream_t st) {
  BwdConvArgs a;
  a.gout = gout; a.packed = packed; a.gin = gin;
  a.e.act = act; a.e.tap = tap; a.e.zs = sdev != nullptr;
  a.e.std0 = sdev ? sdev[0] : 1.0f; a.e.std1 = sdev ? sdev[1] : 1.0f; a.e.std2 = sdev ? sdev[2] : 1.0f;
  a.bs = bs; a.c_in = c_in; a.c_out = c_out; a.h_in = h_in; a.w_in = w_in;
  a.h_out = (h_in + 2 * pad - k) / stride + 1;
  a.w_out = (w_in + 2 * pad - k) / stride + 1;
  a.pad = pad;
  a.K = c_out * k * k;
  a.m_pad = round_up(c_in, LB_MPAD);
  a.N = bs * h_in * w_in;
  if (strided_layer(k, stride)) {
    const int hq = (h_in + 3) / 4, wq = (w_in + 3) / 4;
    const dim3 grid((unsigned)((hq * wq + LB_THREADS - 1) / LB_THREADS), 16, (unsigned)bs);
    lpips_bwd_conv_strided_kernel<11, 4><<<grid, LB_THREADS, 0, st>>>(a);
  } else if (tile == GRPG_LPIPS_TILE_128) {
    conv_launch<128, 128>(a, k, st);
  } else {
    conv_launch<64, 64>(a, k, st);
  }
}

void pool_bwd_enqueue(const float* act, const float* gout, const float* tap, float* gin, const long long planes,
                      const int h, const int w, const int k, hipStream_t st) {
  BwdPoolArgs a;
  a.act = act; a.gout = gout; a.tap = tap; a.gin = gin;
  a.total = (size_t)planes * h * w;
  a.h = h; a.w = w; a.ho = (h - k) / 2 + 1; a.wo = (w - k) / 2 + 1; a.k = k;
  lpips_bwd_pool_kernel<<<(unsigned)((a.total + LB_THREADS - 1) / LB_THREADS), LB_THREADS, 0, st>>>(a);
}

void distance_bwd_enqueue(const float* feat, const float* lin, const float* grad_pairs, const int pairs, const int c,
                          const int hw, float* grad, hipStream_t st) {
  const int px = distance_px(c);
  const dim3 grid((unsigned)((hw + px - 1) / px), (unsigned)pairs);
  lpips_bwd_distance_kernel<<<grid, LB_THREADS, sizeof(float) * 2 * c * px, st>>>(feat, lin, grad_pairs, pairs, c, hw, px, grad);
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_lpips_conv_bwd_packed_bytes(int c_out, int c_in, int k, int stride) {
  if (c_out < 1 || c_in < 1 || c_out > (1 << 20) || c_in > (1 << 20) || (long long)c_out * k * k >= (1ll << 24)) return 0;
  if (strided_layer(k, stride)) return c_in <= 4 ? sizeof(float) * 4 * (size_t)c_out * k * k : 0;
  if (!mfma_layer(k, stride)) return 0;
  return sizeof(float) * (size_t)round_up(c_in, LB_MPAD) * (size_t)round_up(c_out * k * k, LB_BK);
}

int grpg_lpips_conv_bwd_pack_weights(const float* weight, int c_out, int c_in, int k, int stride, float* packed,
                                     void* hip_stream) {
  fail(GRPG_OK, "");
  if (!weight || !packed) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_bwd_pack_weights: NULL weight / packed");
  if (misaligned(weight) || ((uintptr_t)packed & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_bwd_pack_weights: weight must be 4-byte, packed 16-byte aligned");
  const size_t bytes = grpg_lpips_conv_bwd_packed_bytes(c_out, c_in, k, stride);
  if (!bytes)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_bwd_pack_weights: the backward covers k 3 or 5 at stride 1, and k 11 at "
                                           "stride 4 with at most 4 input channels");
  if (int rc = begin_call()) return rc;
  const size_t total = bytes / sizeof(float);
  const int m_pad = strided_layer(k, stride) ? 4 : round_up(c_in, LB_MPAD);
  lpips_bwd_pack_kernel<<<(unsigned)((total + LB_THREADS - 1) / LB_THREADS), LB_THREADS, 0, (hipStream_t)hip_stream>>>(
      weight, c_out, c_in, k, m_pad, total, packed);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_conv2d_backward_data(const float* grad_out, const float* packed_bwd, const float* act, const float* tap,
                                    float* grad_in, int bs, int c_in, int c_out, int h_in, int w_in, int k, int stride,
                                    int pad, const float* sdev, int tile, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!grad_out || !packed_bwd || !grad_in)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: NULL grad_out / packed_bwd / grad_in");
  if (misaligned(grad_out) || misaligned(grad_in) || misaligned(act) || misaligned(tap) || ((uintptr_t)packed_bwd & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: tensors must be 4-byte, packed_bwd 16-byte aligned");
  if (bs < 1 || c_in < 1 || c_out < 1 || h_in < 1 || w_in < 1)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: sizes must be positive");
  if (!grpg_lpips_conv_bwd_packed_bytes(c_out, c_in, k, stride))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: the backward covers k 3 or 5 at stride 1, and k 11 at "
                                           "stride 4 with at most 4 input channels");
  if (pad < 0 || pad >= k) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: 0 <= pad < k");
  if (tap && !act) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: a tap gradient needs the activation it lands on");
  if (sdev && (act || c_in != 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: std is the z-score's, of a 3-channel image, and excludes act");
  if (tile != GRPG_LPIPS_TILE_128 && tile != GRPG_LPIPS_TILE_64)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: unknown tile shape");
  if ((long long)h_in + 2 * pad < k || (long long)w_in + 2 * pad < k)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: the input is smaller than the window");
  const long long h_out = (h_in + 2 * pad - k) / stride + 1, w_out = (w_in + 2 * pad - k) / stride + 1;
  if ((long long)bs * h_in * w_in >= (1ll << 31) - 256 || bs > 65535 || (long long)bs * c_out * h_out * w_out >= (1ll << 38) ||
      (long long)bs * c_in * h_in * w_in >= (1ll << 38))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d_backward_data: tensor too large for one launch");
  if (int rc = begin_call()) return rc;
  conv_bwd_enqueue(grad_out, packed_bwd, grad_in, act, tap, sdev, bs, c_in, c_out, h_in, w_in, k, stride, pad, tile,
                   (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_max_pool_backward(const float* act, const float* grad_out, const float* tap, float* grad_in,
                                 long long planes, int h, int w, int k, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!act || !grad_out || !grad_in) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool_backward: NULL act / grad_out / grad_in");
  if (misaligned(act) || misaligned(grad_out) || misaligned(tap) || misaligned(grad_in))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool_backward: every pointer must be 4-byte aligned");
  if (k != 2 && k != 3) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool_backward: k must be 2 or 3 (stride 2, no padding, floor mode)");
  if (planes < 1 || h < k || w < k)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool_backward: planes must be positive and the plane at least k x k");
  if (planes >= (1ll << 31) || (long long)h * w >= (1ll << 31) || planes * h * w >= (1ll << 38))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool_backward: tensor too large for one launch");
  if (int rc = begin_call()) return rc;
  pool_bwd_enqueue(act, grad_out, tap, grad_in, planes, h, w, k, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_distance_backward(const float* feat, const float* lin, const float* grad_pairs, int pairs, int c, int hw,
                                 float* grad_x, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!feat || !lin || !grad_pairs || !grad_x)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance_backward: NULL feat / lin / grad_pairs / grad_x");
  if (misaligned(feat) || misaligned(lin) || misaligned(grad_pairs) || misaligned(grad_x))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance_backward: every pointer must be 4-byte aligned");
  if (pairs < 1 || pairs > 65535 || c < 1 || c > LB_MAX_C || hw < 1 || hw >= (1ll << 31) - 256 || 2ll * pairs * c * hw >= (1ll << 40))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance_backward: pairs in 1 .. 65535, c in 1 .. 768, 1 <= hw < 2^31 - 256");
  if (int rc = begin_call()) return rc;
  distance_bwd_enqueue(feat, lin, grad_pairs, pairs, c, hw, grad_x, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_backward(int net, const float* const* packed_bwd, const float* const* lin, void* workspace,
                        const float* grad_pairs, float* grad_x, int pairs, int h, int w, void* hip_stream) {
  fail(GRPG_OK, "");
  if (net != GRPG_LPIPS_ALEX && net != GRPG_LPIPS_VGG16) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: unknown net");
  if (!packed_bwd || !lin || !workspace || !grad_pairs || !grad_x)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: NULL packed_bwd / lin / workspace / grad_pairs / grad_x");
  if (misaligned(grad_pairs) || misaligned(grad_x))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: grad_pairs and grad_x must be 4-byte aligned");
  if ((uintptr_t)workspace & 255) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: workspace must be 256-byte aligned");
  LpipsTrainPlan T;
  if (!lpips_train_plan(net, pairs, h, w, T))
    return fail(GRPG_ERR_INVALID_ARGUMENT, std::string("lpips_backward: pairs must be in 1 .. 65535, the image at least ") +
                (net == GRPG_LPIPS_ALEX ? "31 x 31" : "16 x 16") + " and 2 * pairs * H_out * W_out below 2^31 - 256 in every layer");
  for (int i = 0; i < T.n_convs; i++) {
    if (!packed_bwd[i]) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: NULL packed weights of convolution " + std::to_string(i));
    if ((uintptr_t)packed_bwd[i] & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: packed weights must be 16-byte aligned");
  }
  for (int t = 0; t < LPT_TAPS; t++)
    if (!lin[t] || misaligned(lin[t])) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_backward: NULL or misaligned lin weights of tap " + std::to_string(t));
  if (int rc = begin_call()) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  float* gbuf[2] = {(float*)(ws + T.grad_off[0]), (float*)(ws + T.grad_off[1])};
  float* tapgrad = (float*)(ws + T.tapgrad_off);
  auto out_of = [&](const int i) { return (const float*)(ws + T.L[i].out_off); };   // [2 * pairs, ...]: x's come first
  auto tap_enqueue = [&](const int i, float* dst) {   // the gradient of layer i's output as a tap
    const int t = T.L[i].tap;
    distance_bwd_enqueue(out_of(i), lin[t], grad_pairs, pairs, T.tap_c[t], T.tap_hw[t], dst, st);
  };
  // the last layer is the fifth tap's convolution: its pre-activation gradient is the distance's
  int side = 0, conv = T.n_convs - 1;
  tap_enqueue(T.n_layers - 1, gbuf[side]);
  HIP_TRY(hipGetLastError());
  for (int i = T.n_layers - 1; i >= 0; i--) {
    const LpipsTrainLayer& l = T.L[i];
    const float* cur = gbuf[side];
    float* dst = i == 0 ? grad_x : gbuf[side ^ 1];
    // what the produced gradient lands on: layer i - 1's output -- a kept ReLU output unless that layer is a pool
    const bool on_relu = i > 0 && !T.L[i - 1].pool;
    const float* act = on_relu ? out_of(i - 1) : nullptr;
    const float* tap = nullptr;
    if (on_relu && T.L[i - 1].tap >= 0) {
      tap_enqueue(i - 1, tapgrad);
      HIP_TRY(hipGetLastError());
      tap = tapgrad;
    }
    if (l.pool) {
      pool_bwd_enqueue(act, cur, tap, dst, (long long)pairs * l.c_in, l.h_in, l.w_in, l.k, st);
    } else {
      conv_bwd_enqueue(cur, packed_bwd[conv], dst, act, tap, i == 0 ? LB_STD : nullptr, pairs, l.c_in, l.c_out, l.h_in,
                       l.w_in, l.k, l.stride, l.pad, choose_tile(l.c_in, (long long)pairs * l.h_in * l.w_in), st);
      conv--;
    }
    HIP_TRY(hipGetLastError());
    side ^= 1;
  }
  return GRPG_OK;
}

}  // extern "C"
