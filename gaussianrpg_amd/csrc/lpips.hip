// LPIPS for gfx950: the reference's quality metric (lib/utils/lpipsPyTorch/modules/{lpips,networks,utils}.py, which
// metrics.py:81 calls per test view) with the AlexNet or the VGG16 backbone, FP32 over NCHW, as a list of launches of
// FOUR kernels.  No atomics, no split-K: identical calls give identical bits.  The two images of a pair, and all the
// pairs of a call, run as ONE batch of 2 * pairs images (x's first, then y's): every weight is streamed once.
//
// lpips_conv_kernel<BM, BN, KS>: detector.hip's implicit GEMM (M = C_out, N = bs * H_out * W_out, K = C_in * k * k, on
// v_mfma_f32_32x32x2_f32) with the stride and the padding as arguments, KS in {3, 5, 11}.  The rounding contract is
// that kernel's, word for word:
//   chain    k = (ci * KS + ky) * KS + kx ascending in blocks of LP_KBLOCK = 32: a block's partial sum is the fma
//            chain p = 0; p = fma(w_k, x_k, p), and the output is acc = bias; acc = acc + p for the blocks ascending.
//            Padded taps multiply zeros.  Both tile shapes (128 x 128, 64 x 64) run this order: same bits;
//   z-score  the first layer's gather applies BaseNet.z_score (networks.py:50-51): an in-bounds tap is
//            (x - mean_c) / std_c, one float32 subtraction and one correctly rounded division; an out-of-bounds tap is
//            0 -- the padding comes AFTER the z-score, as Conv2d's does;
//   epilogue ReLU, v < 0 ? 0 : v: NaN propagates as F.relu's does.
// A (weights) is detector.hip's packed layout, [bias M_pad][K_pad][M_pad] with M_pad a multiple of 128, K_pad of 16 and
// zeros in the padding; B (the im2col gather) is one guarded scalar load per element, lanes along the pixels; both go
// global -> registers -> LDS with the next tile's loads issued before the current tile's MFMAs.
//
// lpips_pool_kernel: MaxPool2d(3, 2) and MaxPool2d(2, 2), no padding, floor mode; one thread per output element.  max
// is exact, so the bits are F.max_pool2d's; NaN wins as there.
//
// lpips_distance_kernel: one tap of one call.  A workgroup owns 32, 16 or 8 pixels of one pair (C <= 192, <= 384,
// <= 768) and loads their C channels of x's and y's feature ONCE, into LDS; per pixel
//   1. nx = sqrtf(sum_c x_c^2), ny likewise: fma chains, c ascending;
//   2. a_c = x_c / (nx + 1e-10f), b_c likewise (normalize_activation, utils.py:6-8; the eps outside the root, so an
//      all-zero vector gives 0, not NaN);  s = sum_c w_c * ((a_c - b_c) * (a_c - b_c)), each term rounded three times
//      and added in c ascending order (LinLayers' 1 x 1 convolution on (fx - fy)^2, networks.py:23-30).
// The feature maps are read once and the normalised maps are never written.  s goes to the tap's per-pixel map in
// the workspace and, summed over the workgroup in reduce.h's fixed order, to one slot per workgroup.
// lpips_finish_kernel: one workgroup per pair adds each tap's slots in reduce.h's fixed order, divides by H_l * W_l
// and adds the five terms in tap order.
//
// A tap is the ReLU's output, before any pool: layers [2, 5, 8, 10, 12] of alexnet().features and [4, 9, 16, 23, 30]
// of vgg16().features, counted from 1 (networks.py:57-63, 82, 93); VGG16's fifth pool is never run.  A tap's distance
// is enqueued right behind its convolution, so the workspace is two ping-pong activations, the per-pixel maps and the
// slots.  Launches: 5 convolutions + 2 pools + 5 distances + 1 finish for AlexNet, 13 + 4 + 5 + 1 for VGG16.
//
// grpg_lpips_forward_train is the same launch list on the host with every convolution's output kept in a larger
// workspace (lpips_train.h) for the backward (lpips_bwd.hip): no kernel of its own, the same bits.
#include <cmath>
#include <cstdint>

#include "abi_util.h"
#include "common.h"
#include "lpips_train.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_BK = 16;
constexpr int LP_KBLOCK = 32;   // k per partial sum (the rounding order); a multiple of LP_BK
constexpr int LP_MPAD = 128;    // packed weights: C_out rounded up to this, for either tile
constexpr int LP_LDS_PAD = 32;
constexpr int LP_TAPS = 5;
constexpr int LP_MAX_LAYERS = 17;   // VGG16 up to its fifth tap: 13 convolutions + 4 pools
constexpr float LP_EPS = 1e-10f;
// BaseNet's buffers (networks.py:41-44)
constexpr float LP_MEAN[3] = {-.030f, -.088f, -.188f};
constexpr float LP_STD[3] = {.458f, .448f, .450f};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ConvArgs {
  const float* in_x;    // images [0, split)
  const float* in_y;    // images [split, bs)
  float* out;
  const float* packed;
  int split, bs, c_in, c_out, h_in, w_in, h_out, w_out;
  int stride, pad, zscore;
  float mean0, mean1, mean2, std0, std1, std2;
  int K, m_pad, N;
};

__host__ __device__ inline int round_up(const int v, const int m) { return (v + m - 1) / m * m; }

// rows m of the C/D registers of v_mfma_f32_32x32x2_f32: column lane & 31, row below
__device__ __forceinline__ int cd_row(const int reg, const int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Registers: as detector.hip's conv_kernel -- the 128 x 128 shape holds 2 x 64 accumulator registers and is allocated
// for two waves per SIMD, the 64 x 64 shape 2 x 16 for four (tests/test_lpips_resources.py).
template <int BM, int BN, int KS>
__global__ void __launch_bounds__(LP_THREADS, BM == 128 ? 2 : 4) lpips_conv_kernel(const ConvArgs a) {
  constexpr int TM = BM / 64, TN = BN / 64;          // MFMA tiles per wave
  constexpr int LDA = BM + LP_LDS_PAD, LDB = BN + LP_LDS_PAD;
  constexpr int A_VEC = LP_BK * BM / 4 / LP_THREADS;   // float4 loads per thread and tile
  constexpr int B_ROWS = LP_THREADS / BN;              // k rows covered per pass
  constexpr int B_PER = LP_BK / B_ROWS;                // elements per thread and tile
  static_assert(A_VEC >= 1 && B_PER >= 1, "tile too small for the block");
  __shared__ __attribute__((aligned(16))) float As[LP_BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[LP_BK * LDB];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;                    // N < 2^31 - 256 (plan_of, grpg_lpips_conv2d)

  // ---- this thread's column of the B tile: one output pixel ----
  const int bn = t % BN, bk0 = t / BN;
  const int n = n0 + bn;
  const bool n_ok = n < a.N;
  int iy0 = 0, ix0 = 0;
  const float* in_b = a.in_x;
  const size_t in_plane = (size_t)a.h_in * a.w_in;
  if (n_ok) {
    const int hw = a.h_out * a.w_out;
    const int b = n / hw, r = n - b * hw;
    const int oy = r / a.w_out, ox = r - oy * a.w_out;
    iy0 = oy * a.stride - a.pad;
    ix0 = ox * a.stride - a.pad;
    in_b = b < a.split ? a.in_x + (size_t)b * a.c_in * in_plane : a.in_y + (size_t)(b - a.split) * a.c_in * in_plane;
  }
  auto load_b = [&](const int k) -> float {
    if (!n_ok || k >= a.K) return 0.0f;
    const int ci = k / (KS * KS), rr = k - ci * (KS * KS);
    const int ky = rr / KS, kx = rr - ky * KS;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= a.h_in || ix < 0 || ix >= a.w_in) return 0.0f;
    float v = in_b[(size_t)ci * in_plane + (size_t)iy * a.w_in + ix];
    if (a.zscore) {                                  // c_in == 3 (the first layer; grpg_lpips_conv2d checks)
      const float mean = ci == 0 ? a.mean0 : ci == 1 ? a.mean1 : a.mean2;
      const float sdev = ci == 0 ? a.std0 : ci == 1 ? a.std1 : a.std2;
      v = (v - mean) / sdev;
    }
    return v;
  };
  const float* wp = a.packed + a.m_pad;              // behind the bias
  auto load_a = [&](const int k0, const int v) -> f32x4 {
    const int e = v * LP_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
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

  const int k_tiles = (a.K + LP_BK - 1) / LP_BK;
  f32x4 ra[A_VEC];
  float rb[B_PER];
#pragma unroll
  for (int v = 0; v < A_VEC; v++) ra[v] = load_a(0, v);
#pragma unroll
  for (int v = 0; v < B_PER; v++) rb[v] = load_b(bk0 + v * B_ROWS);

  for (int kt = 0; kt < k_tiles; kt++) {
#pragma unroll
    for (int v = 0; v < A_VEC; v++) {
      const int e = v * LP_THREADS + t, kr = e / (BM / 4), mc = (e - kr * (BM / 4)) * 4;
      *reinterpret_cast<f32x4*>(&As[kr * LDA + mc]) = ra[v];
    }
#pragma unroll
    for (int v = 0; v < B_PER; v++) Bs[(bk0 + v * B_ROWS) * LDB + bn] = rb[v];
    __syncthreads();
    if (kt + 1 < k_tiles) {
      const int k0 = (kt + 1) * LP_BK;
#pragma unroll
      for (int v = 0; v < A_VEC; v++) ra[v] = load_a(k0, v);
#pragma unroll
      for (int v = 0; v < B_PER; v++) rb[v] = load_b(k0 + bk0 + v * B_ROWS);
    }
#pragma unroll
    for (int kk = 0; kk < LP_BK; kk += 2) {
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
    if ((kt + 1) % (LP_KBLOCK / LP_BK) == 0 || kt + 1 == k_tiles) {   // the block is complete
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

  // ---- epilogue: ReLU and the store ----
  const size_t out_plane = (size_t)a.h_out * a.w_out;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int nn = n0 + wn + j * 32 + (lane & 31);
    if (nn >= a.N) continue;
    const int hw = a.h_out * a.w_out;
    const int b = nn / hw, r = nn - b * hw;
    float* out_p = a.out + (size_t)b * a.c_out * out_plane + r;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int rg = 0; rg < 16; rg++) {
        const int m = m0 + wm + i * 32 + cd_row(rg, lane);
        if (m >= a.c_out) continue;
        const float v = acc[i][j][rg];
        out_p[(size_t)m * out_plane] = v < 0.0f ? 0.0f : v;   // NaN stays NaN
      }
  }
}

// OIHW weights + bias -> [bias m_pad][k_pad][m_pad], zeros in the padding; one thread per packed float.
__global__ void __launch_bounds__(LP_THREADS)
lpips_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, const int c_out, const int K,
                  const int m_pad, const int k_pad, float* __restrict__ packed) {
  const size_t i = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
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

// max as F.max_pool2d takes it: NaN wins
__device__ __forceinline__ float max_nan(const float m, const float v) { return (v > m || v != v) ? v : m; }

// planes = bs * c planes of h x w -> ho x wo, window k, stride 2, no padding; one thread per output element.
__global__ void __launch_bounds__(LP_THREADS)
lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, const size_t total, const int h, const int w,
                  const int ho, const int wo, const int k) {
  const size_t i = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= total) return;
  const size_t plane = i / ((size_t)ho * wo);
  const int r = (int)(i - plane * ((size_t)ho * wo));
  const int oy = r / wo, ox = r - oy * wo;
  const float* src = in + plane * ((size_t)h * w) + (size_t)(2 * oy) * w + 2 * ox;   // 2 oy + k - 1 < h: floor mode
  float m = -INFINITY;
  for (int dy = 0; dy < k; dy++)
    for (int dx = 0; dx < k; dx++) m = max_nan(m, src[(size_t)dy * w + dx]);
  out[i] = m;
}

// Pixels per workgroup of the distance kernel: both features of the pixels, 2 * C * px floats, stay in LDS (at most
// 48 KiB) between the two passes, so the feature maps are read from memory once.
__host__ __device__ inline int distance_px(const int C) { return C <= 192 ? 32 : C <= 384 ? 16 : 8; }
constexpr int LP_MAX_C = 768;

// feat: [2 * pairs, C, hw]; x of pair p is image p, y image pairs + p.  grid (ceil(hw / px), pairs), px =
// distance_px(C) pixels per workgroup; dynamic LDS: 2 * C * px floats, xs[c * px + pixel] then ys likewise.
//   load     all 256 threads, rows of px pixels: every row is one contiguous segment of a channel plane;
//   pass 1   thread (side, pixel), 2 px threads: the fma chain over c of that side's squares, then sqrtf(..) + eps;
//   terms    all 256 threads: t_c = w_c * ((x_c / nx - y_c / ny)^2) over xs -- the divisions at full width;
//   pass 2   thread pixel, px threads: s = s + t_c for c ascending; s to the map and, block_sum'ed, to the slot.
__global__ void __launch_bounds__(LP_THREADS)
lpips_distance_kernel(const float* __restrict__ feat, const float* __restrict__ lin, const int pairs, const int C,
                      const int hw, const int px, float* __restrict__ map, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lp_tile[];
  __shared__ float s_norm[64];
  __shared__ float s_red[LP_THREADS / 64];
  float* xs = lp_tile;
  float* ys = lp_tile + C * px;
  const int p = blockIdx.y, t = threadIdx.x;
  const int pix = t & (px - 1), row = t / px, rows = LP_THREADS / px;
  const int i = blockIdx.x * px + pix;                   // hw < 2^31 - 256
  const bool ok = i < hw;
  const float* x = feat + (size_t)p * C * hw + i;
  const float* y = feat + (size_t)(pairs + p) * C * hw + i;
  for (int c = row; c < C; c += rows) {
    xs[c * px + pix] = ok ? x[(size_t)c * hw] : 0.0f;    // a pixel beyond the plane: all zeros, s = 0
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
    s_norm[t] = sqrtf(sq) + LP_EPS;
  }
  __syncthreads();
  const float nx = s_norm[pix], ny = s_norm[px + pix];
  for (int c = row; c < C; c += rows) {
    const float d = xs[c * px + pix] / nx - ys[c * px + pix] / ny;
    xs[c * px + pix] = lin[c] * (d * d);
  }
  __syncthreads();
  float s = 0.0f;
  if (t < px) {
    for (int c = 0; c < C; c++) s = s + xs[c * px + pix];
    if (ok) map[(size_t)p * hw + i] = s;
  }
  const float ts = block_sum(s, s_red);
  if (t == 0) slots[(size_t)p * gridDim.x + blockIdx.x] = ts;
}

struct FinishArgs {
  const float* slots[LP_TAPS];
  int nblk[LP_TAPS], hw[LP_TAPS];
  float* out_pairs;
  float* out_taps;   // or NULL
};

// one workgroup per pair
__global__ void __launch_bounds__(REDUCE_THREADS) lpips_finish_kernel(const FinishArgs a) {
  __shared__ float s_red[REDUCE_THREADS];
  const int p = blockIdx.x;
  float total = 0.0f;
#pragma unroll
  for (int l = 0; l < LP_TAPS; l++) {
    const float sum = slot_sum(a.slots[l] + (size_t)p * a.nblk[l], a.nblk[l], s_red);
    const float term = sum / (float)a.hw[l];
    total = l == 0 ? term : total + term;
    if (threadIdx.x == 0 && a.out_taps) a.out_taps[p * LP_TAPS + l] = term;
  }
  if (threadIdx.x == 0) a.out_pairs[p] = total;
}

// ---- the two networks and the plan of a call ----

struct Layer {
  int pool;                 // 0: convolution + ReLU, 1: max-pool
  int c_in, c_out, k, stride, pad;
  int tap;                  // the tap this layer's output is, or -1
  int h_in, w_in, h_out, w_out;
};

struct Plan {
  int n_layers, n_convs;
  Layer L[LP_MAX_LAYERS];
  int tap_c[LP_TAPS], tap_hw[LP_TAPS], tap_nblk[LP_TAPS];
  size_t act_bytes;                               // ONE of the two ping-pong activations
  size_t map_off[LP_TAPS], slot_off[LP_TAPS];     // bytes from the workspace's start
  size_t total;
};

size_t align256(const size_t v) { return (v + 255) / 256 * 256; }

int net_layers(const int net, Layer* L) {
  int n = 0;
  auto conv = [&](int ci, int co, int k, int s, int p, int tap) { L[n++] = Layer{0, ci, co, k, s, p, tap, 0, 0, 0, 0}; };
  auto pool = [&](int c, int k) { L[n++] = Layer{1, c, c, k, 2, 0, -1, 0, 0, 0, 0}; };
  if (net == GRPG_LPIPS_ALEX) {
    conv(3, 64, 11, 4, 2, 0); pool(64, 3);
    conv(64, 192, 5, 1, 2, 1); pool(192, 3);
    conv(192, 384, 3, 1, 1, 2);
    conv(384, 256, 3, 1, 1, 3);
    conv(256, 256, 3, 1, 1, 4);
  } else if (net == GRPG_LPIPS_VGG16) {
    static const int width[5] = {64, 128, 256, 512, 512}, depth[5] = {2, 2, 3, 3, 3};
    int c = 3;
    for (int st = 0; st < 5; st++) {
      for (int d = 0; d < depth[st]; d++) {
        conv(c, width[st], 3, 1, 1, d == depth[st] - 1 ? st : -1);
        c = width[st];
      }
      if (st < 4) pool(c, 2);
    }
  }
  return n;
}

// false: a size the entry points refuse
bool plan_of(const int net, const int pairs, const int h, const int w, Plan& P) {
  if (net != GRPG_LPIPS_ALEX && net != GRPG_LPIPS_VGG16) return false;
  const int least = net == GRPG_LPIPS_ALEX ? 31 : 16;
  if (pairs < 1 || pairs > 65535 || h < least || w < least || h > (1 << 24) || w > (1 << 24)) return false;
  P.n_layers = net_layers(net, P.L);
  P.n_convs = 0;
  const long long bs = 2ll * pairs;
  long long most = 0;
  int ch = h, cw = w;
  for (int i = 0; i < P.n_layers; i++) {
    Layer& l = P.L[i];
    l.h_in = ch; l.w_in = cw;
    l.h_out = (ch + 2 * l.pad - l.k) / l.stride + 1;
    l.w_out = (cw + 2 * l.pad - l.k) / l.stride + 1;
    if (ch + 2 * l.pad < l.k || cw + 2 * l.pad < l.k || l.h_out < 1 || l.w_out < 1) return false;
    const long long n = bs * l.h_out * l.w_out;
    if (n >= (1ll << 31) - 256) return false;        // a launch's pixel index is an int
    if (n * l.c_out >= (1ll << 38)) return false;
    most = n * l.c_out > most ? n * l.c_out : most;
    if (!l.pool) P.n_convs++;
    if (l.tap >= 0) {
      P.tap_c[l.tap] = l.c_out;
      P.tap_hw[l.tap] = l.h_out * l.w_out;
      P.tap_nblk[l.tap] = (P.tap_hw[l.tap] + distance_px(l.c_out) - 1) / distance_px(l.c_out);
    }
    ch = l.h_out; cw = l.w_out;
  }
  P.act_bytes = align256(sizeof(float) * (size_t)most);
  size_t off = 2 * P.act_bytes;
  for (int t = 0; t < LP_TAPS; t++) {
    P.map_off[t] = off;
    off += align256(sizeof(float) * (size_t)pairs * P.tap_hw[t]);
  }
  for (int t = 0; t < LP_TAPS; t++) {
    P.slot_off[t] = off;
    off += align256(sizeof(float) * (size_t)pairs * P.tap_nblk[t]);
  }
  P.total = off;
  return true;
}

// the tile policy of detector.py's choose_tile: 128 x 128 where the layer has at least 96 output channels and fills
// the 256 compute units with such tiles; the result does not depend on it
int choose_tile(const int c_out, const long long n) {
  return (c_out >= 96 && (long long)((c_out + 127) / 128) * ((n + 127) / 128) >= 256) ? GRPG_LPIPS_TILE_128 : GRPG_LPIPS_TILE_64;
}

template <int BM, int BN>
void conv_launch(const ConvArgs& a, const int k, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + BN - 1) / BN), (unsigned)((a.c_out + BM - 1) / BM));
  if (k == 3) lpips_conv_kernel<BM, BN, 3><<<grid, LP_THREADS, 0, st>>>(a);
  else if (k == 5) lpips_conv_kernel<BM, BN, 5><<<grid, LP_THREADS, 0, st>>>(a);
  else lpips_conv_kernel<BM, BN, 11><<<grid, LP_THREADS, 0, st>>>(a);
}

void conv_enqueue(const float* in_x, const float* in_y, const int split, float* out, const float* packed, const int bs,
                  const int c_in, const int c_out, const int h_in, const int w_in, const int h_out, const int w_out,
                  const int k, const int stride, const int pad, const float* mean, const float* sdev, const int tile,
                  hipStream_t st) {
  ConvArgs a;
  a.in_x = in_x; a.in_y = in_y; a.split = split; a.out = out; a.packed = packed;
  a.bs = bs; a.c_in = c_in; a.c_out = c_out; a.h_in = h_in; a.w_in = w_in; a.h_out = h_out; a.w_out = w_out;
  a.stride = stride; a.pad = pad; a.zscore = mean != nullptr;
  a.mean0 = mean ? mean[0] : 0.0f; a.mean1 = mean ? mean[1] : 0.0f; a.mean2 = mean ? mean[2] : 0.0f;
  a.std0 = sdev ? sdev[0] : 1.0f; a.std1 = sdev ? sdev[1] : 1.0f; a.std2 = sdev ? sdev[2] : 1.0f;
  a.K = c_in * k * k;
  a.m_pad = round_up(c_out, LP_MPAD);
  a.N = bs * h_out * w_out;
  if (tile == GRPG_LPIPS_TILE_128) conv_launch<128, 128>(a, k, st);
  else conv_launch<64, 64>(a, k, st);
}

void pool_enqueue(const float* in, float* out, const long long planes, const int h, const int w, const int k,
                  hipStream_t st) {
  const int ho = (h - k) / 2 + 1, wo = (w - k) / 2 + 1;
  const size_t total = (size_t)planes * ho * wo;
  lpips_pool_kernel<<<(unsigned)((total + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, st>>>(in, out, total, h, w, ho, wo, k);
}

void distance_enqueue(const float* feat, const float* lin, const int pairs, const int c, const int hw, float* map,
                      float* slots, hipStream_t st) {
  const int px = distance_px(c);
  const dim3 grid((unsigned)((hw + px - 1) / px), (unsigned)pairs);
  lpips_distance_kernel<<<grid, LP_THREADS, sizeof(float) * 2 * c * px, st>>>(feat, lin, pairs, c, hw, px, map, slots);
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

bool conv_k_ok(const int k) { return k == 3 || k == 5 || k == 11; }

}  // namespace

// The training workspace (lpips_train.h): the eval plan's maps and slots, then EVERY convolution's output (the
// backward reads the x images' post-ReLU activations and both sides' taps), one buffer for the pools' outputs, and the
// backward's gradients.  The kernels, the tile policy and so the pair values are grpg_lpips_forward's.
bool lpips_train_plan(const int net, const int pairs, const int h, const int w, LpipsTrainPlan& T) {
  Plan P;
  if (!plan_of(net, pairs, h, w, P)) return false;
  T.n_layers = P.n_layers;
  T.n_convs = P.n_convs;
  size_t off = 0;
  for (int t = 0; t < LP_TAPS; t++) {
    T.tap_c[t] = P.tap_c[t]; T.tap_hw[t] = P.tap_hw[t]; T.tap_nblk[t] = P.tap_nblk[t];
    T.map_off[t] = off;
    off += align256(sizeof(float) * (size_t)pairs * P.tap_hw[t]);
  }
  for (int t = 0; t < LP_TAPS; t++) {
    T.slot_off[t] = off;
    off += align256(sizeof(float) * (size_t)pairs * P.tap_nblk[t]);
  }
  size_t most_pool = 0, most_grad = 0, most_tap = 0;
  for (int i = 0; i < P.n_layers; i++) {
    const Layer& l = P.L[i];
    const size_t one = sizeof(float) * (size_t)l.c_out * l.h_out * l.w_out;   // one image
    if (l.pool && 2 * pairs * one > most_pool) most_pool = 2 * pairs * one;
    if (pairs * one > most_grad) most_grad = pairs * one;
    if (l.tap >= 0 && pairs * one > most_tap) most_tap = pairs * one;
  }
  const size_t pool_off = off;
  off += align256(most_pool);
  for (int i = 0; i < P.n_layers; i++) {
    const Layer& l = P.L[i];
    LpipsTrainLayer& o = T.L[i];
    o.pool = l.pool; o.c_in = l.c_in; o.c_out = l.c_out; o.k = l.k; o.stride = l.stride; o.pad = l.pad; o.tap = l.tap;
    o.h_in = l.h_in; o.w_in = l.w_in; o.h_out = l.h_out; o.w_out = l.w_out;
    if (l.pool) {
      o.out_off = pool_off;
    } else {
      o.out_off = off;
      off += align256(sizeof(float) * 2 * (size_t)pairs * l.c_out * l.h_out * l.w_out);
    }
  }
  for (int g = 0; g < 2; g++) {
    T.grad_off[g] = off;
    off += align256(most_grad);
  }
  T.tapgrad_off = off;
  off += align256(most_tap);
  T.total = off;
  return true;
}

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_lpips_conv_packed_bytes(int c_out, int c_in, int k) {
  if (c_out < 1 || c_in < 1 || !conv_k_ok(k) || (long long)c_in * k * k >= (1ll << 24) || c_out > (1 << 24)) return 0;
  return sizeof(float) * (size_t)round_up(c_out, LP_MPAD) * (size_t)(round_up(c_in * k * k, LP_BK) + 1);
}

int grpg_lpips_conv_pack_weights(const float* weight, const float* bias, int c_out, int c_in, int k, float* packed,
                                 void* hip_stream) {
  fail(GRPG_OK, "");
  if (!weight || !packed) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_pack_weights: NULL weight / packed");
  if (misaligned(weight) || misaligned(bias) || ((uintptr_t)packed & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_pack_weights: weight and bias must be 4-byte, packed 16-byte aligned");
  const size_t bytes = grpg_lpips_conv_packed_bytes(c_out, c_in, k);
  if (!bytes) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv_pack_weights: c_out, c_in must be positive and k 3, 5 or 11");
  if (int rc = begin_call()) return rc;
  const int K = c_in * k * k, m_pad = round_up(c_out, LP_MPAD), k_pad = round_up(K, LP_BK);
  const size_t total = bytes / sizeof(float);
  lpips_pack_kernel<<<(unsigned)((total + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, (hipStream_t)hip_stream>>>(
      weight, bias, c_out, K, m_pad, k_pad, packed);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_conv2d(const float* in, const float* packed, float* out, int bs, int c_in, int c_out, int h_in, int w_in,
                      int k, int stride, int pad, const float* mean, const float* sdev, int tile, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!in || !packed || !out) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: NULL in / packed / out");
  if (misaligned(in) || misaligned(out) || ((uintptr_t)packed & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: in and out must be 4-byte, packed 16-byte aligned");
  if (bs < 1 || c_in < 1 || c_out < 1 || h_in < 1 || w_in < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: sizes must be positive");
  if (!grpg_lpips_conv_packed_bytes(c_out, c_in, k)) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: k must be 3, 5 or 11");
  if (stride < 1 || stride > 4 || pad < 0 || pad >= k) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: stride must be 1 .. 4 and 0 <= pad < k");
  if ((mean == nullptr) != (sdev == nullptr) || (mean && c_in != 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: the z-score takes mean AND std, of a 3-channel input");
  if (tile != GRPG_LPIPS_TILE_128 && tile != GRPG_LPIPS_TILE_64) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: unknown tile shape");
  if ((long long)h_in + 2 * pad < k || (long long)w_in + 2 * pad < k) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: the input is smaller than the window");
  const int h_out = (h_in + 2 * pad - k) / stride + 1, w_out = (w_in + 2 * pad - k) / stride + 1;
  if ((long long)bs * h_out * w_out >= (1ll << 31) - 256 || (long long)bs * h_in * w_in >= (1ll << 31) - 256 ||
      (long long)bs * c_out * h_out * w_out >= (1ll << 38) || (long long)bs * c_in * h_in * w_in >= (1ll << 38))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_conv2d: tensor too large for one launch");
  if (int rc = begin_call()) return rc;
  conv_enqueue(in, in, bs, out, packed, bs, c_in, c_out, h_in, w_in, h_out, w_out, k, stride, pad, mean, sdev, tile,
               (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_lpips_max_pool(const float* in, float* out, long long planes, int h, int w, int k, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!in || !out) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool: NULL in / out");
  if (misaligned(in) || misaligned(out)) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool: in and out must be 4-byte aligned");
  if (k != 2 && k != 3) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool: k must be 2 or 3 (stride 2, no padding, floor mode)");
  if (planes < 1 || h < k || w < k) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool: planes must be positive and the plane at least k x k");
  if (planes >= (1ll << 31) || (long long)h * w >= (1ll << 31) || planes * h * w >= (1ll << 38))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_max_pool: tensor too large for one launch");
  if (int rc = begin_call()) return rc;
  pool_enqueue(in, out, planes, h, w, k, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

size_t grpg_lpips_distance_workspace_bytes(int pairs, int c, int hw) {
  if (pairs < 1 || pairs > 65535 || c < 1 || c > LP_MAX_C || hw < 1 || hw >= (1ll << 31) - 256) return 0;
  return align256(sizeof(float) * (size_t)pairs * ((hw + distance_px(c) - 1) / distance_px(c)));
}

int grpg_lpips_distance(const float* feat, const float* lin, int pairs, int c, int hw, void* workspace, float* map,
                        float* out_pairs, void* hip_stream) {
  fail(GRPG_OK, "");
  if (!feat || !lin || !workspace || !map || !out_pairs)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance: NULL feat / lin / workspace / map / out_pairs");
  if (misaligned(feat) || misaligned(lin) || misaligned(workspace) || misaligned(map) || misaligned(out_pairs))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance: every pointer must be 4-byte aligned");
  if (!grpg_lpips_distance_workspace_bytes(pairs, c, hw) || 2ll * pairs * c * hw >= (1ll << 40))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_distance: pairs in 1 .. 65535, c in 1 .. 768, 1 <= hw < 2^31 - 256");
  if (int rc = begin_call()) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  float* slots = (float*)workspace;
  distance_enqueue(feat, lin, pairs, c, hw, map, slots, st);
  FinishArgs f;   // the one tap five times over would count it five times: the other four are empty sums
  for (int l = 0; l < LP_TAPS; l++) { f.slots[l] = slots; f.nblk[l] = l == 0 ? (hw + distance_px(c) - 1) / distance_px(c) : 0; f.hw[l] = hw; }
  f.out_pairs = out_pairs; f.out_taps = nullptr;
  lpips_finish_kernel<<<pairs, REDUCE_THREADS, 0, st>>>(f);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

size_t grpg_lpips_workspace_bytes(int net, int pairs, int h, int w) {
  Plan P;
  return plan_of(net, pairs, h, w, P) ? P.total : 0;
}

size_t grpg_lpips_workspace_map_offset(int net, int pairs, int h, int w, int tap) {
  Plan P;
  if (tap < 0 || tap >= LP_TAPS || !plan_of(net, pairs, h, w, P)) return 0;
  return P.map_off[tap];
}

int grpg_lpips_forward(int net, const float* const* packed, const float* const* lin, const float* x, const float* y,
                       int pairs, int h, int w, void* workspace, float* out_pairs, float* out_taps, void* hip_stream) {
  fail(GRPG_OK, "");
  if (net != GRPG_LPIPS_ALEX && net != GRPG_LPIPS_VGG16) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: unknown net");
  if (!packed || !lin || !x || !y || !workspace || !out_pairs)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: NULL packed / lin / x / y / workspace / out_pairs");
  if (misaligned(x) || misaligned(y) || misaligned(out_pairs) || misaligned(out_taps))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: x, y, out_pairs and out_taps must be 4-byte aligned");
  if ((uintptr_t)workspace & 255) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: workspace must be 256-byte aligned");
  Plan P;
  if (!plan_of(net, pairs, h, w, P))
    return fail(GRPG_ERR_INVALID_ARGUMENT, std::string("lpips_forward: pairs must be in 1 .. 65535, the image at least ") +
                (net == GRPG_LPIPS_ALEX ? "31 x 31" : "16 x 16") + " and 2 * pairs * H_out * W_out below 2^31 - 256 in every layer");
  for (int i = 0; i < P.n_convs; i++) {
    if (!packed[i]) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: NULL packed weights of convolution " + std::to_string(i));
    if ((uintptr_t)packed[i] & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: packed weights must be 16-byte aligned");
  }
  for (int t = 0; t < LP_TAPS; t++)
    if (!lin[t] || misaligned(lin[t])) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward: NULL or misaligned lin weights of tap " + std::to_string(t));
  if (int rc = begin_call()) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  float* act[2] = {(float*)ws, (float*)(ws + P.act_bytes)};
  const int bs = 2 * pairs;
  const float* cur = nullptr;   // NULL: the two input tensors
  int side = 0, conv = 0;
  FinishArgs f;
  for (int i = 0; i < P.n_layers; i++) {
    const Layer& l = P.L[i];
    float* dst = act[side];
    if (l.pool) {
      pool_enqueue(cur, dst, (long long)bs * l.c_in, l.h_in, l.w_in, l.k, st);
    } else {
      const long long n = (long long)bs * l.h_out * l.w_out;
      if (!cur)
        conv_enqueue(x, y, pairs, dst, packed[conv], bs, l.c_in, l.c_out, l.h_in, l.w_in, l.h_out, l.w_out, l.k, l.stride,
                     l.pad, LP_MEAN, LP_STD, choose_tile(l.c_out, n), st);
      else
        conv_enqueue(cur, cur, bs, dst, packed[conv], bs, l.c_in, l.c_out, l.h_in, l.w_in, l.h_out, l.w_out, l.k, l.stride,
                     l.pad, nullptr, nullptr, choose_tile(l.c_out, n), st);
      conv++;
    }
    HIP_TRY(hipGetLastError());
    if (l.tap >= 0) {
      const int t = l.tap;
      float* slots = (float*)(ws + P.slot_off[t]);
      distance_enqueue(dst, lin[t], pairs, P.tap_c[t], P.tap_hw[t], (float*)(ws + P.map_off[t]), slots, st);
      HIP_TRY(hipGetLastError());
      f.slots[t] = slots; f.nblk[t] = P.tap_nblk[t]; f.hw[t] = P.tap_hw[t];
    }
    cur = dst;
    side ^= 1;
  }
  f.out_pairs = out_pairs; f.out_taps = out_taps;
  lpips_finish_kernel<<<pairs, REDUCE_THREADS, 0, st>>>(f);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

size_t grpg_lpips_train_workspace_bytes(int net, int pairs, int h, int w) {
  LpipsTrainPlan T;
  return lpips_train_plan(net, pairs, h, w, T) ? T.total : 0;
}

size_t grpg_lpips_train_activation_offset(int net, int pairs, int h, int w, int conv) {
  LpipsTrainPlan T;
  if (conv < 0 || !lpips_train_plan(net, pairs, h, w, T)) return 0;
  for (int i = 0; i < T.n_layers; i++)
    if (!T.L[i].pool && conv-- == 0) return T.L[i].out_off;
  return 0;
}

int grpg_lpips_forward_train(int net, const float* const* packed, const float* const* lin, const float* x, const float* y,
                             int pairs, int h, int w, void* workspace, float* out_pairs, float* out_taps,
                             void* hip_stream) {
  fail(GRPG_OK, "");
  if (net != GRPG_LPIPS_ALEX && net != GRPG_LPIPS_VGG16) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: unknown net");
  if (!packed || !lin || !x || !y || !workspace || !out_pairs)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: NULL packed / lin / x / y / workspace / out_pairs");
  if (misaligned(x) || misaligned(y) || misaligned(out_pairs) || misaligned(out_taps))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: x, y, out_pairs and out_taps must be 4-byte aligned");
  if ((uintptr_t)workspace & 255) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: workspace must be 256-byte aligned");
  LpipsTrainPlan T;
  if (!lpips_train_plan(net, pairs, h, w, T))
    return fail(GRPG_ERR_INVALID_ARGUMENT, std::string("lpips_forward_train: pairs must be in 1 .. 65535, the image at least ") +
                (net == GRPG_LPIPS_ALEX ? "31 x 31" : "16 x 16") + " and 2 * pairs * H_out * W_out below 2^31 - 256 in every layer");
  for (int i = 0; i < T.n_convs; i++) {
    if (!packed[i]) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: NULL packed weights of convolution " + std::to_string(i));
    if ((uintptr_t)packed[i] & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: packed weights must be 16-byte aligned");
  }
  for (int t = 0; t < LP_TAPS; t++)
    if (!lin[t] || misaligned(lin[t])) return fail(GRPG_ERR_INVALID_ARGUMENT, "lpips_forward_train: NULL or misaligned lin weights of tap " + std::to_string(t));
  if (int rc = begin_call()) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  const int bs = 2 * pairs;
  const float* cur = nullptr;   // NULL: the two input tensors
  int conv = 0;
  FinishArgs f;
  for (int i = 0; i < T.n_layers; i++) {
    const LpipsTrainLayer& l = T.L[i];
    float* dst = (float*)(ws + l.out_off);
    if (l.pool) {
      pool_enqueue(cur, dst, (long long)bs * l.c_in, l.h_in, l.w_in, l.k, st);
    } else {
      const long long n = (long long)bs * l.h_out * l.w_out;
      if (!cur)
        conv_enqueue(x, y, pairs, dst, packed[conv], bs, l.c_in, l.c_out, l.h_in, l.w_in, l.h_out, l.w_out, l.k, l.stride,
                     l.pad, LP_MEAN, LP_STD, choose_tile(l.c_out, n), st);
      else
        conv_enqueue(cur, cur, bs, dst, packed[conv], bs, l.c_in, l.c_out, l.h_in, l.w_in, l.h_out, l.w_out, l.k, l.stride,
                     l.pad, nullptr, nullptr, choose_tile(l.c_out, n), st);
      conv++;
    }
    HIP_TRY(hipGetLastError());
    if (l.tap >= 0) {
      const int t = l.tap;
      float* slots = (float*)(ws + T.slot_off[t]);
      distance_enqueue(dst, lin[t], pairs, T.tap_c[t], T.tap_hw[t], (float*)(ws + T.map_off[t]), slots, st);
      HIP_TRY(hipGetLastError());
      f.slots[t] = slots; f.nblk[t] = T.tap_nblk[t]; f.hw[t] = T.tap_hw[t];
    }
    cur = dst;
  }
  f.out_pairs = out_pairs; f.out_taps = out_taps;
  lpips_finish_kernel<<<pairs, REDUCE_THREADS, 0, st>>>(f);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
