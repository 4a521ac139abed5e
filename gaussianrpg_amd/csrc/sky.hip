// Sky cube map for gfx950: lookup + composite, without nvdiffrast.
//
// Replaces what the reference does per frame in PyTorch + nvdiffrast
// (lib/models/sky_cubemap.py:77-122 SkyCubeMap.forward, lib/models/street_gaussian_renderer.py:
// 106-115, lib/utils/graphics_utils.py:186-207 get_rays_torch):
//   rays_d   = normalize(R^T K^-1 (x + 0.5, y + 0.5, 1))                 (get_rays_torch, no perturbation)
//   mask     = (1 - acc) > 1e-3                                          (sky_cubemap.py:84-85)
//   sky      = mask ? dr.texture(cube[None], rays_d, filter_mode='linear', boundary_mode='cube')
//                   : fill (0, or 1 for a white background)               (:100-120), clamp(0, 1)
//   rgb      = rgb + sky * (1 - acc), then clamp(0, 1) outside train mode (street_gaussian_renderer.py:110,116)
// in ONE launch that reads rgb / acc once and writes rgb once (the reference: ray generation, mask
// compaction, texture fetch, scatter, permute, clamp, multiply, add, clamp -- ten kernels and a
// hard-coded 1080x1920 scratch image, sky_cubemap.py:29-34, that breaks the 1920x1280 Waymo frames).
//
// Cube-map semantics (nvdiffrast `boundary_mode='cube'`, `filter_mode='linear'`; the dependency is
// not vendored, so this restates its documented behaviour -- PARITY UNPINNED beyond the face
// convention, which the reference's own cube_to_dir (sky_cubemap.py:139-146) pins):
//   * the major axis of the direction selects the face: +x 0, -x 1, +y 2, -y 3, +z 4, -z 5; the
//     face coordinates are (u, v) = (0.5 + 0.5 a / |m|, 0.5 + 0.5 b / |m|) with (a, b) per face
//     = (-z,-y) (z,-y) (x,z) (x,-z) (x,-y) (-x,-y), i.e. the inverse of cube_to_dir;
//   * texel centres sit at (i + 0.5) / res; bilinear weights from u * res - 0.5;
//   * a tap that leaves the face across ONE edge continues on the neighbouring face at the same
//     position along the edge (the cube is unfolded about the shared edge); a tap that leaves
//     across a CORNER has no texel: it is dropped and the other three weights are renormalised.
// Backward (training the sky): d rgb / d cube scatters (1 - acc) * weight * dL/drgb into the up to
// four texels, d rgb / d acc = -sky.
#include "abi_util.h"
#include "common.h"
#include "sky_math.h"

namespace grpg {

// rgb [3,H,W] (in place when rgb_out == rgb_in), acc [H,W]; sky_out optional [3,H,W]
__global__ void __launch_bounds__(256)
sky_composite_kernel(const SkyArgs s, const int W, const int H, const float* __restrict__ rgb_in,
                     const float* __restrict__ acc, float* __restrict__ rgb_out,
                     float* __restrict__ sky_out) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63);
  const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= W || py >= H) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  const float a = acc ? acc[pix] : 0.f;
  const float tr = 1.f - a;
  float sky[3];
  sky_pixel(s, px, py, pix, HW, acc != nullptr, tr, sky);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (sky_out) sky_out[c * HW + pix] = sky[c];
    if (rgb_out) rgb_out[c * HW + pix] = sky_over(rgb_in[c * HW + pix], sky[c], tr, s.clamp_out);
  }
}

// dL/dcube += (1 - acc) * w_k * dL/drgb   (only where the texture was fetched and not clamped),
// dL/dacc  = -sum_c sky_c * dL/drgb_c.  grad_rgb is the gradient of the UNclamped composite (train mode).
__global__ void __launch_bounds__(256)
sky_backward_kernel(const SkyArgs s, const int W, const int H, const float* __restrict__ acc,
                    const float* __restrict__ grad_rgb, float* __restrict__ grad_cube,
                    float* __restrict__ grad_acc) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63);
  const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= W || py >= H) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  const float a = acc ? acc[pix] : 0.f;
  const float tr = 1.f - a;
  const float g[3] = {grad_rgb[pix], grad_rgb[HW + pix], grad_rgb[2 * HW + pix]};
  float sky[3] = {s.fill, s.fill, s.fill};
  if (sky_fetches(s, pix, acc != nullptr, tr)) {
    float dx, dy, dz;
    pixel_ray(s, px, py, pix, HW, dx, dy, dz);
    const CubeTaps t = cube_taps(dx, dy, dz, s.res);
    sky[0] = sky[1] = sky[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (t.idx[k] >= 0) {
        const float* c = s.cube + 3 * (size_t)t.idx[k];
        sky[0] += t.w[k] * c[0]; sky[1] += t.w[k] * c[1]; sky[2] += t.w[k] * c[2];
      }
    }
    if (grad_cube) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (sky[c] < 0.f || sky[c] > 1.f) continue;   // clamp(0,1) has zero gradient outside
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (t.idx[k] >= 0) atomicAdd(&grad_cube[3 * (size_t)t.idx[k] + c], tr * t.w[k] * g[c]);
      }
    }
  }
  if (grad_acc) {
    float ga = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) ga -= fminf(fmaxf(sky[c], 0.f), 1.f) * g[c];
    grad_acc[pix] = ga;
  }
}

static SkyArgs make_sky_args(const float* cube, int res, const float* m9, int m_on_device, float fill,
                             int clamp_out, const unsigned char* mask, const float* jitter) {
  SkyArgs s;
  s.cube = cube; s.res = res; s.fill = fill; s.clamp_out = clamp_out;
  s.mask = mask; s.jitter = jitter;
  s.m_dev = m_on_device ? m9 : nullptr;
  for (int i = 0; i < 9; i++) s.m[i] = m_on_device ? 0.f : m9[i];
  return s;
}

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

int grpg_sky_composite_ex(const float* cube, int res, const float* ray_matrix, int ray_matrix_on_device,
                          float fill, int clamp_out, int width, int height, const float* rgb_in,
                          const float* acc, const unsigned char* mask, const float* jitter,
                          float* rgb_out, float* sky_out, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!cube || !ray_matrix || res <= 0 || width <= 0 || height <= 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "bad cube / ray matrix / size");
  if ((rgb_in == nullptr) != (rgb_out == nullptr))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "rgb_in and rgb_out go together");
  if (!rgb_out && !sky_out) return fail(GRPG_ERR_INVALID_ARGUMENT, "nothing to write");
  const SkyArgs s = make_sky_args(cube, res, ray_matrix, ray_matrix_on_device, fill, clamp_out, mask, jitter);
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  sky_composite_kernel<<<grid, 256, 0, (hipStream_t)hip_stream>>>(s, width, height, rgb_in, acc, rgb_out, sky_out);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_sky_composite(const float* cube, int res, const float* ray_matrix, float fill,
                       int clamp_out, int width, int height, const float* rgb_in, const float* acc,
                       float* rgb_out, float* sky_out, void* hip_stream) {
  return grpg_sky_composite_ex(cube, res, ray_matrix, 0, fill, clamp_out, width, height, rgb_in, acc,
                               nullptr, nullptr, rgb_out, sky_out, hip_stream);
}

int grpg_sky_backward_ex(const float* cube, int res, const float* ray_matrix, int ray_matrix_on_device,
                         float fill, int width, int height, const float* acc, const unsigned char* mask,
                         const float* jitter, const float* grad_rgb, float* grad_cube, float* grad_acc,
                         void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!cube || !ray_matrix || !grad_rgb || res <= 0 || width <= 0 || height <= 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "bad cube / ray matrix / gradient / size");
  const SkyArgs s = make_sky_args(cube, res, ray_matrix, ray_matrix_on_device, fill, 0, mask, jitter);
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  sky_backward_kernel<<<grid, 256, 0, (hipStream_t)hip_stream>>>(s, width, height, acc, grad_rgb, grad_cube, grad_acc);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_sky_backward(const float* cube, int res, const float* ray_matrix, float fill, int width,
                      int height, const float* acc, const float* grad_rgb, float* grad_cube,
                      float* grad_acc, void* hip_stream) {
  return grpg_sky_backward_ex(cube, res, ray_matrix, 0, fill, width, height, acc, nullptr, nullptr,
                              grad_rgb, grad_cube, grad_acc, hip_stream);
}

}  // extern "C"
