// Object-alpha plane of a TRAINING frame and its backward, from the blobs the frame's forward left behind.
//
// Replaces the reference's second render of every training iteration with lambda_reg > 0 (train.py:145-158,
// render_object, street_gaussian_renderer.py:42-56): a whole forward and backward of the op over the object models,
// read for acc_obj alone.  The frame already holds the tile ranges, the depth-sorted point list and the projected
// records; the plane needs alpha only -- no colour, depth, SH, sort or preprocess -- and its backward no
// back-to-front recurrence: with acc_obj = 1 - T_obj,
//   d acc_obj / d alpha_i = T_obj,final / (1 - alpha_i)      for every splat that contributed (alpha <= 0.99),
// so ONE front-to-back walk over the object entries serves both directions.
//
// Mapping: one workgroup per 16x16 tile, one pixel per thread.  The four waves of a workgroup are independent (no
// barrier, no hand-over): wave w owns the 16x4 quarter the w-th sub-tile bit of a list entry speaks about, scans the
// tile's list 64 entries at a time (entry + class byte per lane), ballot-compacts the OBJECT entries that can reach
// its quarter and stages only their records in its own LDS rows.  The class comes from a uint8 [P] array: the plain
// training render reads ids through ID_MASK (28 bits), so no bit of the entry is free for it.  Tiles that no object
// Gaussian's rectangle touches are flagged by a small pass over the records; both kernels leave them at once.
// The accept rules and the arithmetic are blend_math.h's, so the plane has the bits the main render's alpha has on
// the object models alone.
#include "blend_math.h"
#include "common.h"

namespace grpg {

constexpr int OA_WAVES = 4;

// ---- class array + tile flags -------------------------------------------------------------------------------------
// cls[idx] = class of Gaussian idx (layer_class, or its model's SegmentDev::pad1 & 1 in a composed frame); every tile
// of a visible object Gaussian's rectangle (the one its list entries were emitted for, auxiliary.h:46-56) is flagged.
// Visibility comes from tiles[idx], the tile count preprocess writes for EVERY index (0 = culled): a culled
// Gaussian's record is never written and holds whatever the blob's memory held before.
// Plain byte stores of the value 1, like the layered frame's preprocess.
__global__ void __launch_bounds__(256)
object_class_kernel(const int P, const unsigned char* __restrict__ layer_class, const SegmentDev* __restrict__ segs,
                    const RecView rec, const uint32_t* __restrict__ tiles, const int gx, const int gy,
                    unsigned char* __restrict__ cls,
                    unsigned char* __restrict__ tile_flags) {
  const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
  if (idx >= P) return;
  bool obj;
  if (layer_class != nullptr) {
    obj = layer_class[idx] != 0;
  } else {
    // the rows' [start, start + count) ascend and end at P: a handful of rows per frame
    int s = 0;
    while (s < MAX_SEGMENTS - 1 && (uint32_t)idx >= segs[s].start + segs[s].count) s++;
    obj = ((uint32_t)(uintptr_t)segs[s].pad1 & 1u) != 0u;
  }
  cls[idx] = obj ? 1 : 0;
  if (!obj || tiles[idx] == 0u) return;   // culled: no list entries, no record
  const float4 r0 = rec.geo0((size_t)idx);
  const int radius = (int)(__float_as_uint(r0.w) & ~REC_CLASS_BIT);
  int minx, miny, maxx, maxy;
  get_rect(r0.x, r0.y, radius, gx, gy, minx, miny, maxx, maxy);
  for (int ty = miny; ty < maxy; ty++)
    for (int tx = minx; tx < maxx; tx++) tile_flags[(size_t)ty * gx + tx] = 1;
}

// ---- forward ----------------------------------------------------------------------------------------------------
// out_alpha = 1 - T_obj (the project's out_alpha = 1 - T), n_contrib_obj = 1-based position, in the wave's sequence
// of staged object entries, of the last splat applied.  A wave ends after at most range.y - range.x entries.
__global__ void __launch_bounds__(256)
object_alpha_forward_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                            const RecView rec, const unsigned char* __restrict__ cls,
                            const unsigned char* __restrict__ tile_flags, const int W, const int H, const int gx,
                            float* __restrict__ out_alpha, uint32_t* __restrict__ n_contrib_obj) {
  __shared__ float4 s_rec[OA_WAVES][WAVE * 2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t tile = blockIdx.x;
  const int ty = (int)(tile / (uint32_t)gx), tx = (int)(tile - (uint32_t)ty * (uint32_t)gx);
  const int px = tx * TILE + (lane & 15), py = ty * TILE + wave * 4 + (lane >> 4);
  const bool inside = px < W && py < H;
  float T = 1.0f;
  uint32_t last = 0;
  if (tile_flags[tile] != 0) {
    const float pxf = (float)px, pyf = (float)py;
    const uint2 range = ranges[tile];
    const uint32_t rb = __builtin_amdgcn_readfirstlane(range.x);
    const uint32_t re = __builtin_amdgcn_readfirstlane(range.y);
    const uint32_t qbit = 1u << (SUBTILE_SHIFT + wave);
    const uint64_t lt = lanemask_lt();
    float4* const my = s_rec[wave];
    bool done = !inside;
    uint32_t seen = 0;   // object entries of this quarter walked so far (wave-uniform)
    for (uint32_t base = rb; base < re; base += WAVE) {
      if (__ballot(!done) == 0ull) break;
      const bool in = base + (uint32_t)lane < re;
      const uint32_t e = in ? point_list[base + lane] : 0u;
      const uint32_t id = e & ID_MASK;
      const bool keep = in && (e & qbit) != 0u && cls[id] != 0;
      const uint64_t m = __ballot(keep);
      const uint32_t n = (uint32_t)__popcll(m);
      if (keep) {
        const int slot = (int)__popcll(m & lt);
        const float4 g0 = rec.geo0(id), g1 = rec.geo1(id);
        const SplatQ q = splat_q(g1.x, g1.y, g1.z);
        my[slot * 2 + 0] = make_float4(g0.x, g0.y, g0.z, 0.f);   // px, py, opacity
        my[slot * 2 + 1] = make_float4(q.A, q.B, q.C, 0.f);
      }
      __builtin_amdgcn_wave_barrier();
      for (uint32_t j = 0; j < n; j++) {
        const float4 a = my[j * 2 + 0];
        const float4 qq = my[j * 2 + 1];
        const SplatTerms st = splat_terms_q(a.x - pxf, SplatQ{qq.x, qq.y, qq.z});
        float G, alpha;
        bool valid = pair_alpha(pair_power(st, a.y - pyf), a.z, G, alpha) && !done;
        const float test_T = T * (1.0f - alpha);
        const bool term = valid && (test_T < 0.0001f);
        done = done || term;
        valid = valid && !term;
        T = valid ? test_T : T;
        last = valid ? seen + j + 1u : last;
      }
      __builtin_amdgcn_wave_barrier();
      seen += n;
    }
  }
  if (inside) {
    const size_t pix = (size_t)py * W + px;
    out_alpha[pix] = 1.0f - T;
    n_contrib_obj[pix] = last;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float oa_dpp_add(const float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// Wave totals of 8 quantities: halving exchanges (v_permlane32_swap, v_permlane16_swap: two quantities per swap +
// add, as in render_bwd.hip) leave quantity k + 2 r in g[k] of row r (lanes 16 r ...); four DPP adds per register
// finish the row sums.  Returns, in lanes 0 and 1 of row r, the totals of v[2 r] and v[2 r + 1].
__device__ __forceinline__ float oa_wave_sum_8(const float (&v)[8], const bool lane_odd) {
  float h[4], g[2];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[k]), __float_as_uint(v[k + 4]), false, false);
    h[k] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(h[k]), __float_as_uint(h[k + 2]), false, false);
    g[k] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  float s0 = g[0], s1 = g[1];
  s0 = oa_dpp_add<0xB1>(s0);  s1 = oa_dpp_add<0xB1>(s1);    // quad_perm [1,0,3,2]
  s0 = oa_dpp_add<0x4E>(s0);  s1 = oa_dpp_add<0x4E>(s1);    // quad_perm [2,3,0,1]
  s0 = oa_dpp_add<0x141>(s0); s1 = oa_dpp_add<0x141>(s1);   // row_half_mirror
  s0 = oa_dpp_add<0x140>(s0); s1 = oa_dpp_add<0x140>(s1);   // row_mirror
  return lane_odd ? s1 : s0;
}

__device__ __forceinline__ uint32_t oa_wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// The same walk and filter as the forward, gated per pixel by n_contrib_obj.  dL/dalpha_i = g T_final / (1 - alpha_i);
// from there the chain of render_bwd.hip: dL/dG = opacity dL/dalpha, dL/dopacity = G dL/dalpha, conic and mean2D
// with the same 0.5 W / 0.5 H factors (backward.cu:501-502, 618-638); no clamp mask on the 0.99, as in the reference.
// One float atomic per (wave, splat, field) into the frame's gradient records: fields 0-2 mean2D (x, y, |x| + |y|),
// 3-5 conic, 9 opacity.
__global__ void __launch_bounds__(256)
object_alpha_backward_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                             const RecView rec, const unsigned char* __restrict__ cls,
                             const unsigned char* __restrict__ tile_flags, const int W, const int H, const int gx,
                             const float* __restrict__ alpha_object, const uint32_t* __restrict__ n_contrib_obj,
                             const float* __restrict__ dL_dalpha_object, float* __restrict__ grad_rec) {
  __shared__ float4 s_rec[OA_WAVES][WAVE * 3];
  const uint32_t tile = blockIdx.x;
  if (tile_flags[tile] == 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ty = (int)(tile / (uint32_t)gx), tx = (int)(tile - (uint32_t)ty * (uint32_t)gx);
  const int px = tx * TILE + (lane & 15), py = ty * TILE + wave * 4 + (lane >> 4);
  const bool inside = px < W && py < H;
  const size_t pix = inside ? (size_t)py * W + px : 0;
  // g T_final: the pixel's factor of every contributor (an exact zero contributes exact zeros: not walked for)
  const float gT = inside ? (1.0f - alpha_object[pix]) * dL_dalpha_object[pix] : 0.f;
  const uint32_t lastc = (inside && gT != 0.f) ? n_contrib_obj[pix] : 0u;
  const uint32_t maxlast = oa_wave_max_u32(lastc);   // nothing behind the quarter's deepest contributor matters
  if (maxlast == 0u) return;
  const float pxf = (float)px, pyf = (float)py;
  const float nddelx = -(float)(0.5 * W), nddely = -(float)(0.5 * H);   // -ddelx_dx, -ddely_dy
  const uint2 range = ranges[tile];
  const uint32_t rb = __builtin_amdgcn_readfirstlane(range.x);
  const uint32_t re = __builtin_amdgcn_readfirstlane(range.y);
  const uint32_t qbit = 1u << (SUBTILE_SHIFT + wave);
  const uint64_t lt = lanemask_lt();
  float4* const my = s_rec[wave];
  // totals of quantity 2 r + k land in lane k (k = 0, 1) of row r: quantities 0-2 mean2D, 3-5 conic moments
  // (accumulated without their -1/2, backward.cu:634-636), 6 opacity, 7 unused
  const int row = lane >> 4, sub = lane & 15;
  const int qi = 2 * row + sub;
  const bool sc_lane = sub < 2 && qi < 7;
  float* const sc_ptr = grad_rec + (qi < 6 ? qi : 9);
  const float sc_scale = (qi >= 3 && qi < 6) ? -0.5f : 1.0f;
  const bool lane_odd = (lane & 1) != 0;
  uint32_t seen = 0;
  for (uint32_t base = rb; base < re && seen < maxlast; base += WAVE) {
    const bool in = base + (uint32_t)lane < re;
    const uint32_t e = in ? point_list[base + lane] : 0u;
    const uint32_t id = e & ID_MASK;
    const bool keep = in && (e & qbit) != 0u && cls[id] != 0;
    const uint64_t m = __ballot(keep);
    const uint32_t n = (uint32_t)__popcll(m);
    if (keep) {
      const int slot = (int)__popcll(m & lt);
      const float4 g0 = rec.geo0(id), g1 = rec.geo1(id);
      const SplatQ q = splat_q(g1.x, g1.y, g1.z);
      my[slot * 3 + 0] = make_float4(g0.x, g0.y, g0.z, __uint_as_float(id));   // px, py, opacity, id
      my[slot * 3 + 1] = make_float4(nddelx * g1.x, nddelx * g1.y, nddely * g1.z, nddely * g1.y);
      my[slot * 3 + 2] = make_float4(q.A, q.B, q.C, 0.f);
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t nn = min(n, maxlast - seen);
    for (uint32_t j = 0; j < nn; j++) {
      const float4 a = my[j * 3 + 0];
      const float4 b = my[j * 3 + 1];
      const float4 qq = my[j * 3 + 2];
      const uint32_t gid = __float_as_uint(a.w);
      const float dx = a.x - pxf, dy = a.y - pyf;
      const SplatTerms st = splat_terms_q(dx, SplatQ{qq.x, qq.y, qq.z});
      const float power2 = pair_power(st, dy);   // identical arithmetic to the forward (blend_math.h)
      float G = __builtin_amdgcn_exp2f(power2);
      float alpha = fminf(ALPHA_MAX, a.z * G);
      const bool valid = !(power2 > 0.0f) && !(alpha < ALPHA_MIN) && (seen + j) < lastc;
      if (__ballot(valid) == 0ull) continue;   // wave-uniform: no pixel of the quarter took this splat
      // a lane that rejected the splat runs the same arithmetic with alpha = G = 0: exact zeros in every sum
      alpha = valid ? alpha : 0.f;
      G = valid ? G : 0.f;
      const float dL_dalpha = __builtin_amdgcn_rcpf(1.f - alpha) * gT;
      const float gd = G * dL_dalpha;                 // dL_dopacity
      const float w = a.z * gd;                       // dL_dG G
      const float tdx = w * dx, tdy = w * dy;
      const float mx = fmaf(b.y, tdy, b.x * tdx);
      const float my_ = fmaf(b.w, tdx, b.z * tdy);
      const float qv[8] = {mx, my_, fabsf(mx) + fabsf(my_), tdx * dx, tdx * dy, tdy * dy, gd, 0.f};
      const float tot = oa_wave_sum_8(qv, lane_odd);
      if (sc_lane) atomicAdd(sc_ptr + (size_t)gid * GRAD_STRIDE, tot * sc_scale);
    }
    __builtin_amdgcn_wave_barrier();
    seen += n;
  }
}

void launch_object_alpha_forward(hipStream_t s, int P, const unsigned char* layer_class, const SegmentDev* segs,
                                 const uint2* ranges, const uint32_t* point_list, const RecView rec,
                                 const uint32_t* tiles, int W, int H, int gx, int gy, unsigned char* cls, float* out_alpha, uint32_t* n_contrib_obj,
                                 unsigned char* tile_flags) {
  const int ntiles = gx * gy;
  if (P <= 0 || ntiles <= 0) return;
  object_class_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, layer_class, segs, rec, tiles, gx, gy, cls, tile_flags);
  object_alpha_forward_kernel<<<ntiles, 256, 0, s>>>(ranges, point_list, rec, cls, tile_flags, W, H, gx, out_alpha,
                                                     n_contrib_obj);
}

void launch_object_alpha_backward(hipStream_t s, const uint2* ranges, const uint32_t* point_list, const RecView rec,
                                  const unsigned char* cls, const unsigned char* tile_flags, int W, int H, int gx,
                                  int gy, const float* alpha_object, const uint32_t* n_contrib_obj,
                                  const float* dL_dalpha_object, float* grad_rec) {
  const int ntiles = gx * gy;
  if (ntiles <= 0) return;
  object_alpha_backward_kernel<<<ntiles, 256, 0, s>>>(ranges, point_list, rec, cls, tile_flags, W, H, gx,
                                                      alpha_object, n_contrib_obj, dL_dalpha_object, grad_rec);
}

}  // namespace grpg
