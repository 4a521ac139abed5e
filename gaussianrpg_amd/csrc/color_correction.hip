// Colour correction of a frame for gfx950: the per-pixel 3x4 affine map between the sky composite and the evaluation
// clamp of StreetGaussianRenderer.render (lib/models/street_gaussian_renderer.py:105-116), with its backward.
//
// Replaces ColorCorrection.forward (lib/models/color_correction.py:129-132)
//   image = einsum('ij,jhw->ihw', A[:, :3], image) + A[:, 3, None, None]
// and, when the sky inputs are given, the line in front of it and the one behind it:
//   x   = rgb + sky * (1 - acc)            exactly sky_composite_kernel's value (sky_math.h, clamp_out = 0)
//   y_i = A_i0 x_0 + A_i1 x_1 + A_i2 x_2 + A_i3
//   y   = clamp(y, 0, 1)                   evaluation only
//   rgb8[h][w][i] = colour_u8(y_i)         pack_hwc's rule, on the clamped value
// in ONE launch that reads rgb / acc once.  A is read from DEVICE memory (affine_trans[id] is a view of the
// parameter): the address is uniform across the wave, there is no host copy and no host wait.
//
// Arithmetic.  y_i = fma(A_i2, x_2, fma(A_i1, x_1, fma(A_i0, x_0, A_i3))): three roundings; with A = eye(4)[:3] every
// step is exact and y has x's bits.  g_x_j = fma(A_2j, g_2, fma(A_1j, g_1, A_0j * g_0)): three roundings, exact for the
// identity.  Both are written with explicit fmaf in ONE device function each, so the instantiation with the sky
// composite and the one without give the same bits for the same x (tests/test_gpu_color_correction.py compares
// them); everything else in this unit is compiled without contraction.
//
// Backward.  x is recomputed (the forward does not store it).  The twelve sums
//   grad_A[i][j] = sum_pixels g_i * x_j  (j < 3),   grad_A[i][3] = sum_pixels g_i
// take each term as ONE float32 product (g_i itself for j = 3) and add them in a fixed order, without atomics:
//   1. a workgroup is 64 x 4 pixels, one wave per row (the tiling of the sky kernels); a lane outside the image
//      contributes +0.  The 64 lanes of a wave are added by a butterfly (xor 32, 16, ... 1):  6 additions deep;
//   2. thread k < 12 adds the four wave sums of value k in ascending wave order:             3 additions
//      and stores the workgroup's partial into workspace[k][block], block = blockIdx.y * gridDim.x + blockIdx.x;
//   3. one workgroup of REDUCE_THREADS (1024) threads per sum: thread t adds partials t, t + 1024, ... in ascending
//      order:                                                                                  max(0, ceil(nb / 1024) - 1)
//      then the LDS tree of halves 512 ... 1 (reduce.h slot_sum):                            10 additions.
// With nb = ceil(W / 64) * ceil(H / 4) workgroups (about H W / 256), the longest chain of additions a sum passes is
//   d = 19 + max(0, ceil(nb / 1024) - 1)
// (19 up to 1024 workgroups; 28 at 1920 x 1280).  Adding zero is exact, so a one-hot g gives g_i and the rounded
// product g_i * x_j back exactly.  Identical calls give identical bits.  The clamp has no backward (evaluation only);
// with the sky inputs the cube-map and acc gradients come from grpg_sky_backward_ex on g_x (sky.hip, unchanged).
#include "abi_util.h"
#include "color_math.h"
#include "common.h"
#include "reduce.h"
#include "sky_math.h"

namespace grpg {

constexpr int CC_SUMS = 12;

// (row i of the affine map: affine_row, color_math.h -- shared with the frame epilogue of render_fwd.hip)

// column j of A^T g
__device__ __forceinline__ float affine_col(const float* a, const int j, const float (&g)[3]) {
  return fmaf(a[8 + j], g[2], fmaf(a[4 + j], g[1], a[j] * g[0]));
}

// x of pixel (px, py): the composite when SKY, rgb itself otherwise.  SKY: sky_composite_kernel's statements.
template <bool SKY>
__device__ __forceinline__ void corrected_input(const SkyArgs& s, const int px, const int py, const size_t pix,
                                                const size_t HW, const float* rgb, const float* acc, float (&x)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) x[c] = rgb[c * HW + pix];
  if (SKY) {
    const float a = acc[pix];
    const float tr = 1.f - a;
    float sky[3];
    sky_pixel(s, px, py, pix, HW, true, tr, sky);
#pragma unroll
    for (int c = 0; c < 3; c++) x[c] = sky_over(x[c], sky[c], tr, 0);
  }
}

// rgb [3,H,W]; planes [3,H,W] (may be rgb itself) and / or rgb8 [H,W,3]; affine: 12 floats in device memory
template <bool SKY>
__global__ void __launch_bounds__(256)
color_correct_kernel(const SkyArgs s, const int W, const int H, const float* rgb, const float* __restrict__ acc,
                     const float* __restrict__ affine, const int clamp_out, float* planes,
                     unsigned char* __restrict__ rgb8, const float bias) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63);
  const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= W || py >= H) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  float a[CC_SUMS];
#pragma unroll
  for (int k = 0; k < CC_SUMS; k++) a[k] = affine[k];
  float x[3];
  corrected_input<SKY>(s, px, py, pix, HW, rgb, acc, x);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float y = affine_row(a, i, x);
    if (planes) planes[i * HW + pix] = clamp_out ? clamp01(y) : y;
    if (rgb8) rgb8[3 * pix + i] = colour_u8(y, bias);
  }
}

// grad [3,H,W] -> grad_x [3,H,W] (optional) and the workgroup's twelve partial sums (optional) into
// partials[k * nb + block]
template <bool SKY>
__global__ void __launch_bounds__(256)
color_correct_backward_kernel(const SkyArgs s, const int W, const int H, const float* __restrict__ rgb,
                              const float* __restrict__ acc, const float* __restrict__ affine,
                              const float* __restrict__ grad, float* __restrict__ grad_x,
                              float* __restrict__ partials) {
  __shared__ float s_red[CC_SUMS * 4];
  const int px = blockIdx.x * 64 + (threadIdx.x & 63);
  const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
  const bool inside = px < W && py < H;
  float v[CC_SUMS];
#pragma unroll
  for (int k = 0; k < CC_SUMS; k++) v[k] = 0.f;
  if (inside) {
    const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
    const float g[3] = {grad[pix], grad[HW + pix], grad[2 * HW + pix]};
    if (grad_x) {
      float a[CC_SUMS];
#pragma unroll
      for (int k = 0; k < CC_SUMS; k++) a[k] = affine[k];
#pragma unroll
      for (int j = 0; j < 3; j++) grad_x[j * HW + pix] = affine_col(a, j, g);
    }
    if (partials) {
      float x[3];
      corrected_input<SKY>(s, px, py, pix, HW, rgb, acc, x);
#pragma unroll
      for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) v[4 * i + j] = g[i] * x[j];
        v[4 * i + 3] = g[i];
      }
    }
  }
  if (!partials) return;   // uniform across the grid
  const float t = block_sum_each(v, s_red);
  if (threadIdx.x < CC_SUMS) {
    const size_t nb = (size_t)gridDim.x * gridDim.y, block = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[threadIdx.x * nb + block] = t;
  }
}

// one workgroup of REDUCE_THREADS per sum (blockIdx.x = k): grad_affine[k] = the fixed-order sum of
// partials[k * nb .. (k + 1) * nb)
__global__ void __launch_bounds__(REDUCE_THREADS)
color_correct_reduce_kernel(const float* __restrict__ partials, const size_t nb, float* __restrict__ grad_affine) {
  __shared__ float s_red[REDUCE_THREADS];
  const int k = blockIdx.x;
  const float t = slot_sum(partials + k * nb, nb, s_red);
  if (threadIdx.x == 0) grad_affine[k] = t;
}

namespace {

size_t cc_blocks(const int width, const int height) {
  return (size_t)((width + 63) / 64) * (size_t)((height + 3) / 4);
}

// The sky inputs of both entries: all of cube / ray matrix / acc (res > 0), or none of them -- and then no mask or
// jitter either.  Returns 0 (no sky), 1 (sky) or -1 (given in part).
int cc_sky_mode(const float* cube, const int res, const float* ray_matrix, const float* acc,
                const unsigned char* mask, const float* jitter) {
  if (!cube && !ray_matrix && !acc && !mask && !jitter) return 0;
  if (cube && ray_matrix && acc && res > 0) return 1;
  return -1;
}

SkyArgs cc_sky_args(const int sky, const float* cube, const int res, const float* m9, const int m_on_device,
                    const float fill, const unsigned char* mask, const float* jitter) {
  SkyArgs s;
  s.cube = cube; s.res = res; s.fill = fill; s.clamp_out = 0;
  s.mask = mask; s.jitter = jitter;
  s.m_dev = (sky && m_on_device) ? m9 : nullptr;
  for (int i = 0; i < 9; i++) s.m[i] = (sky && !m_on_device) ? m9[i] : 0.f;
  return s;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_color_correct_workspace_bytes(int width, int height) {
  if (width <= 0 || height <= 0) return 0;
  return cc_blocks(width, height) * CC_SUMS * sizeof(float);
}

int grpg_color_correct_forward(int width, int height, const float* rgb, const float* affine, const float* sky_cube,
                               int sky_res, const float* ray_matrix, int ray_matrix_on_device, float sky_fill,
                               const float* acc, const unsigned char* sky_mask, const float* sky_jitter,
                               int clamp_out, float* out_planes, unsigned char* out_rgb8, int truncate,
                               void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (width <= 0 || height <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: sizes must be positive");
  if (!rgb || !affine) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: NULL rgb / affine matrix");
  if (!out_planes && !out_rgb8) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: nothing to write");
  const int sky = cc_sky_mode(sky_cube, sky_res, ray_matrix, acc, sky_mask, sky_jitter);
  if (sky < 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: the sky inputs (cube, res, ray matrix, acc) go together");
  const SkyArgs s = cc_sky_args(sky, sky_cube, sky_res, ray_matrix, ray_matrix_on_device, sky_fill, sky_mask,
                                sky_jitter);
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  const float bias = truncate ? 0.0f : 0.5f;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (sky)
    color_correct_kernel<true><<<grid, 256, 0, stream>>>(s, width, height, rgb, acc, affine, clamp_out, out_planes,
                                                         out_rgb8, bias);
  else
    color_correct_kernel<false><<<grid, 256, 0, stream>>>(s, width, height, rgb, nullptr, affine, clamp_out,
                                                          out_planes, out_rgb8, bias);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_color_correct_backward(int width, int height, const float* rgb, const float* affine, const float* sky_cube,
                                int sky_res, const float* ray_matrix, int ray_matrix_on_device, float sky_fill,
                                const float* acc, const unsigned char* sky_mask, const float* sky_jitter,
                                const float* grad_out, float* grad_x, float* grad_affine, void* workspace,
                                void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (width <= 0 || height <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: sizes must be positive");
  if (!rgb || !affine || !grad_out)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: NULL rgb / affine matrix / gradient");
  if (!grad_x && !grad_affine) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: nothing to write");
  if (grad_affine && (!workspace || ((uintptr_t)workspace & 3)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: grad_affine needs a 4-byte aligned workspace");
  const int sky = cc_sky_mode(sky_cube, sky_res, ray_matrix, acc, sky_mask, sky_jitter);
  if (sky < 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_correct: the sky inputs (cube, res, ray matrix, acc) go together");
  const SkyArgs s = cc_sky_args(sky, sky_cube, sky_res, ray_matrix, ray_matrix_on_device, sky_fill, sky_mask,
                                sky_jitter);
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  float* partials = grad_affine ? (float*)workspace : nullptr;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (sky)
    color_correct_backward_kernel<true><<<grid, 256, 0, stream>>>(s, width, height, rgb, acc, affine, grad_out,
                                                                  grad_x, partials);
  else
    color_correct_backward_kernel<false><<<grid, 256, 0, stream>>>(s, width, height, rgb, nullptr, affine, grad_out,
                                                                   grad_x, partials);
  HIP_TRY(hipGetLastError());
  if (grad_affine) {
    color_correct_reduce_kernel<<<CC_SUMS, REDUCE_THREADS, 0, stream>>>(partials, cc_blocks(width, height), grad_affine);
    HIP_TRY(hipGetLastError());
  }
  return GRPG_OK;
}

}  // extern "C"
