// Fused SSIM + L1 training loss for gfx950: loss_utils.ssim / loss_utils.l1_loss and the
// train.py:118 mix  w_l1 * L1 + w_ssim * (1 - SSIM)  (w_l1 = (1 - lambda_dssim) * lambda_l1,
// w_ssim = lambda_dssim) in one forward and one backward launch chain.
//
// The reference (lib/utils/loss_utils.py) runs five depthwise 11x11 F.conv2d calls and ~15
// elementwise kernels over full-frame planes, and autograd runs the same again in backward.  Here:
//   * ssim_forward_kernel: one workgroup per 32x16 output tile of one (batch, channel) plane.  The
//     tile plus a 5-pixel halo of both images is loaded into LDS with the mask applied (zero outside
//     the image: conv2d's zero padding); the window runs as two 11-tap passes (it is separable) and
//     gives the five moments mu1, mu2, E[x1^2], E[x2^2], E[x1 x2].  From them: the SSIM map, the
//     masked L1 term and the mask count, summed per workgroup into fixed slots (no atomics), and --
//     when a gradient is wanted -- the three per-pixel partials of the map
//         D_mu = dm/dmu1 - 2 mu1 dm/dsigma1^2 - mu2 dm/dsigma12,  D_11 = dm/dsigma1^2,  D_12 = dm/dsigma12
//     (the derivatives with respect to mu1, E[x1^2] and E[x1 x2]).
//   * ssim_reduce_kernel: ONE workgroup combines the per-workgroup slots in a fixed order (float64):
//     identical calls give identical bits.  It writes the stats vector
//         stats[0] loss, [1] L1 mean, [2] SSIM mean, [3] mask count (elements), [4 + b] SSIM of image b.
//   * ssim_backward_kernel (gather form, no atomics): the same tiling over the saved partials,
//         dL/dx1(p) = s_b mask(p) sum_q G(q - p) [D_mu(q) + 2 x1(p) D_11(q) + x2(p) D_12(q)]
//                   + mask(p) sign(x1 - x2) s_l1
//     over in-image q (the partial planes are zero-padded in LDS).  s_b and s_l1 are formed on the
//     device from the upstream gradient of the stats vector and the forward's count: no host sync.
// Semantics of loss_utils kept exactly: the mask selects both images before any moment, as
// torch.where(mask, img, 0) does -- a deselected element counts as 0 whatever it holds (NaN and Inf
// included; it is never multiplied), and its gradient is exactly 0; the SSIM mean runs over all
// B*C*H*W positions, the L1 mean over the selected elements only (all-false mask: NaN, gradient 0);
// C1 = 0.01^2, C2 = 0.03^2; variances as E[x^2] - mu^2.
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int SS_TW = 32, SS_TH = 16;           // output tile
constexpr int SS_R = 5;                         // window radius (window_size 11)
constexpr int SS_IW = SS_TW + 2 * SS_R;         // 42: tile + halo
constexpr int SS_IH = SS_TH + 2 * SS_R;         // 26
constexpr int SS_THREADS = 256;
constexpr int SS_PX = SS_TW * SS_TH / SS_THREADS;   // 2 output pixels per lane

// loss_utils.gaussian(11, 1.5): exp(-(x - 5)^2 / 4.5) normalised by its sum, in float32
constexpr float SS_G[11] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
    0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

constexpr float SS_C1 = 0.01f * 0.01f;
constexpr float SS_C2 = 0.03f * 0.03f;

struct SsimShape {
  int B, C, H, W;
  int tiles_x, tiles_y;
  size_t plane;           // H * W
  size_t mask_bstride;    // elements between the masks of two images (0: one mask for all)
  size_t mask_cstride;    // elements between the masks of two channels (0: one mask per image)
};

__device__ __forceinline__ float mask_at(const unsigned char* __restrict__ mask, const SsimShape& s,
                                         const int b, const int c, const size_t pix) {
  if (!mask) return 1.0f;
  return mask[(size_t)b * s.mask_bstride + (size_t)c * s.mask_cstride + pix] ? 1.0f : 0.0f;
}

__global__ void __launch_bounds__(SS_THREADS)
ssim_forward_kernel(const SsimShape s, const float* __restrict__ x1, const float* __restrict__ x2,
                    const unsigned char* __restrict__ mask, double* __restrict__ part,
                    float* __restrict__ saved) {
  __shared__ float s_a[SS_IH][SS_IW], s_b[SS_IH][SS_IW];
  __shared__ float s_h[5][SS_IH][SS_TW];   // horizontal pass: mu1, mu2, x1^2, x2^2, x1 x2
  __shared__ double s_red[SS_THREADS / 64];
  const int ntiles = s.tiles_x * s.tiles_y;
  const int plane_id = blockIdx.x / ntiles;          // b * C + c
  const int tile = blockIdx.x - plane_id * ntiles;
  const int b = plane_id / s.C, c = plane_id - b * s.C;
  const int ty = tile / s.tiles_x, tx = tile - ty * s.tiles_x;
  const int x0 = tx * SS_TW - SS_R, y0 = ty * SS_TH - SS_R;
  const size_t base = (size_t)plane_id * s.plane;
  const int tid = threadIdx.x;

  for (int i = tid; i < SS_IH * SS_IW; i += SS_THREADS) {
    const int r = i / SS_IW, q = i - r * SS_IW;
    const int gy = y0 + r, gx = x0 + q;
    float a = 0.f, v = 0.f;
    if (gy >= 0 && gy < s.H && gx >= 0 && gx < s.W) {
      const size_t pix = (size_t)gy * s.W + gx;
      // select, as torch.where does: 0 * NaN and 0 * Inf are NaN, and a deselected value must not reach a moment
      if (mask_at(mask, s, b, c, pix) != 0.f) {
        a = x1[base + pix];
        v = x2[base + pix];
      }
    }
    s_a[r][q] = a;
    s_b[r][q] = v;
  }
  __syncthreads();
  for (int i = tid; i < SS_IH * SS_TW; i += SS_THREADS) {
    const int r = i / SS_TW, q = i - r * SS_TW;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float a = s_a[r][q + k], v = s_b[r][q + k], g = SS_G[k];
      m1 += g * a;
      m2 += g * v;
      e11 += g * (a * a);
      e22 += g * (v * v);
      e12 += g * (a * v);
    }
    s_h[0][r][q] = m1; s_h[1][r][q] = m2; s_h[2][r][q] = e11; s_h[3][r][q] = e22; s_h[4][r][q] = e12;
  }
  __syncthreads();

  float sum_ssim = 0.f, sum_l1 = 0.f, sum_cnt = 0.f;
#pragma unroll
  for (int j = 0; j < SS_PX; j++) {
    const int i = tid + j * SS_THREADS;
    const int r = i / SS_TW, q = i - r * SS_TW;
    const int gy = y0 + SS_R + r, gx = x0 + SS_R + q;
    if (gy >= s.H || gx >= s.W) continue;
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float g = SS_G[k];
      mu1 += g * s_h[0][r + k][q];
      mu2 += g * s_h[1][r + k][q];
      e11 += g * s_h[2][r + k][q];
      e22 += g * s_h[3][r + k][q];
      e12 += g * s_h[4][r + k][q];
    }
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float sig1 = e11 - mu1_sq, sig2 = e22 - mu2_sq, sig12 = e12 - mu12;
    const float A1 = 2.f * mu12 + SS_C1, A2 = 2.f * sig12 + SS_C2;
    const float B1 = mu1_sq + mu2_sq + SS_C1, B2 = sig1 + sig2 + SS_C2;
    const float den = B1 * B2;
    const float map = (A1 * A2) / den;
    sum_ssim += map;
    const size_t pix = (size_t)gy * s.W + gx;
    const float m = mask_at(mask, s, b, c, pix);
    sum_l1 += fabsf(s_a[SS_R + r][SS_R + q] - s_b[SS_R + r][SS_R + q]);   // masked values: m |x1 - x2|
    sum_cnt += m;
    if (saved) {
      const float inv = 1.0f / den;
      const float d11 = -map / B2;                                     // dm / dsigma1^2
      const float d12 = 2.f * A1 * inv;                                // dm / dsigma12
      const float dmu = 2.f * mu2 * A2 * inv - map * 2.f * mu1 / B1;   // dm / dmu1 (sigmas held)
      const size_t n = (size_t)s.B * s.C * s.plane;
      saved[base + pix] = dmu - 2.f * mu1 * d11 - mu2 * d12;
      saved[n + base + pix] = d11;
      saved[2 * n + base + pix] = d12;
    }
  }
  const size_t nwg = (size_t)gridDim.x;
  // the butterfly in float32, widened at the wave boundary (reduce.h)
  const double t_ssim = block_sum(sum_ssim, s_red);
  const double t_l1 = block_sum(sum_l1, s_red);
  const double t_cnt = block_sum(sum_cnt, s_red);
  if (tid == 0) {
    part[blockIdx.x] = t_ssim;
    part[nwg + blockIdx.x] = t_l1;
    part[2 * nwg + blockIdx.x] = t_cnt;
  }
}

// one workgroup: the per-workgroup slots in a fixed order -> stats[0..3 + B]
__global__ void __launch_bounds__(REDUCE_THREADS)
ssim_reduce_kernel(const SsimShape s, const double* __restrict__ part, const float w_l1,
                   const float w_ssim, float* __restrict__ stats) {
  __shared__ double s_red[REDUCE_THREADS];
  const size_t per_image = (size_t)s.C * s.tiles_x * s.tiles_y;
  const size_t nwg = per_image * s.B;
  double tot_ssim = 0.0;
  for (int b = 0; b < s.B; b++) {
    const double v = slot_sum(part + b * per_image, per_image, s_red);
    tot_ssim += v;
    if (threadIdx.x == 0) stats[4 + b] = (float)(v / ((double)s.C * (double)s.plane));
  }
  const double l1 = slot_sum(part + nwg, nwg, s_red);
  const double cnt = slot_sum(part + 2 * nwg, nwg, s_red);
  if (threadIdx.x == 0) {
    const double ssim = tot_ssim / ((double)s.B * (double)s.C * (double)s.plane);
    const float l1m = (float)(l1 / cnt);      // 0 / 0 = NaN for an all-false mask, as the reference
    const float ssimf = (float)ssim;
    stats[0] = w_l1 * l1m + w_ssim * (1.0f - ssimf);
    stats[1] = l1m;
    stats[2] = ssimf;
    stats[3] = (float)cnt;
  }
}

__global__ void __launch_bounds__(SS_THREADS)
ssim_backward_kernel(const SsimShape s, const float* __restrict__ x1, const float* __restrict__ x2,
                     const unsigned char* __restrict__ mask, const float* __restrict__ saved,
                     const float* __restrict__ stats, const float* __restrict__ gstats,
                     const float w_l1, const float w_ssim, float* __restrict__ grad) {
  __shared__ float s_d[3][SS_IH][SS_IW];
  __shared__ float s_h[3][SS_IH][SS_TW];
  const int ntiles = s.tiles_x * s.tiles_y;
  const int plane_id = blockIdx.x / ntiles;
  const int tile = blockIdx.x - plane_id * ntiles;
  const int b = plane_id / s.C, c = plane_id - b * s.C;
  const int ty = tile / s.tiles_x, tx = tile - ty * s.tiles_x;
  const int x0 = tx * SS_TW - SS_R, y0 = ty * SS_TH - SS_R;
  const size_t base = (size_t)plane_id * s.plane;
  const size_t n = (size_t)s.B * s.C * s.plane;
  const int tid = threadIdx.x;

  // upstream coefficients: d loss, d L1, d SSIM (mean), d SSIM (image b) -> per-element scales
  const float g_loss = gstats[0], g_l1 = gstats[1], g_ssim = gstats[2], g_img = gstats[4 + b];
  const float cnt = stats[3];
  const float s_ssim = (g_ssim - w_ssim * g_loss) / ((float)s.B * (float)s.C * (float)s.plane) +
                       g_img / ((float)s.C * (float)s.plane);
  const float s_l1 = (g_l1 + w_l1 * g_loss) / cnt;

  for (int i = tid; i < SS_IH * SS_IW; i += SS_THREADS) {
    const int r = i / SS_IW, q = i - r * SS_IW;
    const int gy = y0 + r, gx = x0 + q;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (gy >= 0 && gy < s.H && gx >= 0 && gx < s.W) {
      const size_t k = base + (size_t)gy * s.W + gx;
      d0 = saved[k];
      d1 = saved[n + k];
      d2 = saved[2 * n + k];
    }
    s_d[0][r][q] = d0; s_d[1][r][q] = d1; s_d[2][r][q] = d2;
  }
  __syncthreads();
  for (int i = tid; i < SS_IH * SS_TW; i += SS_THREADS) {
    const int r = i / SS_TW, q = i - r * SS_TW;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float g = SS_G[k];
      h0 += g * s_d[0][r][q + k];
      h1 += g * s_d[1][r][q + k];
      h2 += g * s_d[2][r][q + k];
    }
    s_h[0][r][q] = h0; s_h[1][r][q] = h1; s_h[2][r][q] = h2;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SS_PX; j++) {
    const int i = tid + j * SS_THREADS;
    const int r = i / SS_TW, q = i - r * SS_TW;
    const int gy = y0 + SS_R + r, gx = x0 + SS_R + q;
    if (gy >= s.H || gx >= s.W) continue;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {   // the window is symmetric: G(q - p) = G(p - q)
      const float g = SS_G[k];
      v0 += g * s_h[0][r + k][q];
      v1 += g * s_h[1][r + k][q];
      v2 += g * s_h[2][r + k][q];
    }
    const size_t pix = (size_t)gy * s.W + gx;
    const float m = mask_at(mask, s, b, c, pix);
    const float a = x1[base + pix], v = x2[base + pix];
    float gval = 0.f;
    if (m != 0.f) {
      const float d = a - v;
      const float sgn = (float)((d > 0.f) - (d < 0.f));
      gval = s_ssim * (v0 + 2.f * a * v1 + v * v2) + sgn * s_l1;
    }
    grad[base + pix] = gval;
  }
}

SsimShape make_shape(const int B, const int C, const int H, const int W, const int mask_batch,
                     const int mask_channels) {
  SsimShape s;
  s.B = B; s.C = C; s.H = H; s.W = W;
  s.tiles_x = (W + SS_TW - 1) / SS_TW;
  s.tiles_y = (H + SS_TH - 1) / SS_TH;
  s.plane = (size_t)H * W;
  s.mask_cstride = mask_channels > 1 ? s.plane : 0;
  s.mask_bstride = mask_batch > 1 ? (size_t)mask_channels * s.plane : 0;
  return s;
}

int ssim_check(int B, int C, int height, int width, const float* img1, const float* img2,
               const unsigned char* mask, int mask_batch, int mask_channels) {
  if (B <= 0 || C <= 0 || height <= 0 || width <= 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: B, C, height and width must be positive");
  if ((long long)B * C * height * width > 0x7FFFFFFFll)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: B*C*H*W must be < 2^31");
  if (!img1 || !img2) return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: NULL image pointer");
  if (mask && ((mask_batch != 1 && mask_batch != B) || (mask_channels != 1 && mask_channels != C)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: the mask must have 1 or B images of 1 or C channels");
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_ssim_workspace_bytes(int B, int C, int height, int width) {
  if (B <= 0 || C <= 0 || height <= 0 || width <= 0) return 0;
  const SsimShape s = make_shape(B, C, height, width, 1, 1);
  return align_up(3 * sizeof(double) * (size_t)B * C * s.tiles_x * s.tiles_y, 256);
}

int grpg_ssim_forward(int B, int C, int height, int width, const float* img1, const float* img2,
                      const unsigned char* mask, int mask_batch, int mask_channels, float w_l1,
                      float w_ssim, float* stats, float* saved, void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = ssim_check(B, C, height, width, img1, img2, mask, mask_batch, mask_channels)) return rc;
  if (!stats || !workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: NULL stats / workspace");
  if ((uintptr_t)workspace & 7) return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  const SsimShape s = make_shape(B, C, height, width, mask_batch, mask_channels);
  const int nwg = B * C * s.tiles_x * s.tiles_y;
  double* part = (double*)workspace;
  ssim_forward_kernel<<<nwg, SS_THREADS, 0, st>>>(s, img1, img2, mask, part, saved);
  ssim_reduce_kernel<<<1, REDUCE_THREADS, 0, st>>>(s, part, w_l1, w_ssim, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_ssim_backward(int B, int C, int height, int width, const float* img1, const float* img2,
                       const unsigned char* mask, int mask_batch, int mask_channels, float w_l1,
                       float w_ssim, const float* stats, const float* saved, const float* grad_stats,
                       float* grad_img1, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = ssim_check(B, C, height, width, img1, img2, mask, mask_batch, mask_channels)) return rc;
  if (!stats || !saved || !grad_stats || !grad_img1)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "ssim: NULL stats / saved partials / gradient pointer");
  const SsimShape s = make_shape(B, C, height, width, mask_batch, mask_channels);
  const int nwg = B * C * s.tiles_x * s.tiles_y;
  ssim_backward_kernel<<<nwg, SS_THREADS, 0, (hipStream_t)hip_stream>>>(s, img1, img2, mask, saved, stats,
                                                                         grad_stats, w_l1, w_ssim, grad_img1);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
