// Feature planes of a composed frame: the flat [P,F] array the blend forward and backward read by Gaussian id,
// produced on the device from the models' own arrays, and its gradient chained back to them.  F = 3 * normals + S,
// normals first, then the semantic channels: the order in which the reference's renderer concatenates them
// (lib/models/street_gaussian_renderer.py:205-215).
//
// compose_features_kernel: one thread per Gaussian of the frame, all segments in one launch.
//   semantic channels  row j of the segment's semantic[count,S], copied bit for bit (NULL array: zeros) --
//                      StreetGaussianModel.get_semantic (street_gaussian_model.py:420-435)
//   normal channels    GaussianModel.get_normals (lib/models/gaussian_model.py:256-269) on the values compose_one()
//                      forms, i.e. the ones the composed preprocess splats:
//                        k = argmin of the activated scales (ties: the lowest index)
//                        R = quaternion_to_matrix(world rotation) (lib/utils/general_utils.py:125-146: it divides by
//                            the norm once more), n = R[:, k]
//                        n is negated unless sum(-dir / |dir| * n) >= 0, dir = world mean - cam_pos (a NaN compares
//                        false, as in torch.where: a Gaussian at the camera centre gets -R[:, k])
//                      For an actor this is R_obj n_local at unit length with the sign taken in the world frame: what
//                      street_gaussian_model.py:463-484 intends (INTEGRATION.md section 14 names the deviation).
//
// compose_features_backward_kernel: the same thread layout over dL_dfeatures[P,F].  The semantic gradient is WRITTEN
// to the segment's own array.  The normal gradient goes through R[:, k], the normalisations, the quaternion product
// and the flip (rotation_chain_backward of compose_math.h, shared with the composed preprocess backward) and is ADDED
// to the segment's raw-rotation gradient -- one thread per row, no atomics -- and, for an actor, summed into
// dL_dposes[segment][0:4]: per workgroup and segment one slot (block_sum), then feature_pose_sum_kernel adds a
// segment's slots in a fixed order (slot_sum).  No gradient through k, the sign, the means or the scales, like the
// reference.  Given dL_dfeatures, identical calls give identical bits.
//
// Built with -ffp-contract=off: compose_one() must give the bits the composed preprocess sees.
#include "common.h"

#pragma clang fp contract(off)

#include "gaussian_math.h"
#include "compose_math.h"
#include "reduce.h"

namespace grpg {

namespace {

struct Normal {
  float n[3];      // the signed normal
  float4 qu;       // the world quaternion divided by its norm (r, x, y, z)
  float norm;      // that norm
  float sign;      // +1 / -1
  int k;           // the axis of the smallest scale
};

// column k of quaternion_to_matrix's R for a unit quaternion (r, x, y, z) = (q.x, q.y, q.z, q.w)
__device__ __forceinline__ void matrix_column(const float4 q, const int k, float* n) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  if (k == 0) {
    n[0] = 1.f - 2.f * (y * y + z * z); n[1] = 2.f * (x * y + r * z); n[2] = 2.f * (x * z - r * y);
  } else if (k == 1) {
    n[0] = 2.f * (x * y - r * z); n[1] = 1.f - 2.f * (x * x + z * z); n[2] = 2.f * (y * z + r * x);
  } else {
    n[0] = 2.f * (x * z + r * y); n[1] = 2.f * (y * z - r * x); n[2] = 1.f - 2.f * (x * x + y * y);
  }
}

// g = dL/dR[:, k] -> dL/d(unit quaternion)
__device__ __forceinline__ float4 matrix_column_backward(const float4 q, const int k, const float* g) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  if (k == 0)
    return make_float4(2.f * (z * g[1] - y * g[2]), 2.f * (y * g[1] + z * g[2]),
                       -4.f * y * g[0] + 2.f * x * g[1] - 2.f * r * g[2],
                       -4.f * z * g[0] + 2.f * r * g[1] + 2.f * x * g[2]);
  if (k == 1)
    return make_float4(2.f * (x * g[2] - z * g[0]), 2.f * y * g[0] - 4.f * x * g[1] + 2.f * r * g[2],
                       2.f * (x * g[0] + z * g[2]), -2.f * r * g[0] - 4.f * z * g[1] + 2.f * y * g[2]);
  return make_float4(2.f * (y * g[0] - x * g[1]), 2.f * z * g[0] - 2.f * r * g[1] - 4.f * x * g[2],
                     2.f * r * g[0] + 2.f * z * g[1] - 4.f * y * g[2], 2.f * (x * g[0] + y * g[1]));
}

__device__ __forceinline__ Normal normal_one(const Activated& a, const float* __restrict__ campos) {
  Normal o;
  o.k = 0;
  float smin = a.s0;
  if (a.s1 < smin) { o.k = 1; smin = a.s1; }
  if (a.s2 < smin) o.k = 2;
  o.norm = sqrtf(a.q.x * a.q.x + a.q.y * a.q.y + a.q.z * a.q.z + a.q.w * a.q.w);
  o.qu = make_float4(a.q.x / o.norm, a.q.y / o.norm, a.q.z / o.norm, a.q.w / o.norm);
  matrix_column(o.qu, o.k, o.n);
  const float dx = a.mx - campos[0], dy = a.my - campos[1], dz = a.mz - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  const float dot = -(dx / len) * o.n[0] + -(dy / len) * o.n[1] + -(dz / len) * o.n[2];
  o.sign = dot >= 0.f ? 1.f : -1.f;
  if (!(dot >= 0.f)) { o.n[0] = -o.n[0]; o.n[1] = -o.n[1]; o.n[2] = -o.n[2]; }
  return o;
}

__global__ void __launch_bounds__(FEATURE_THREADS)
compose_features_kernel(const int P, const SegmentDev* __restrict__ segs, const FeatureSegDev* __restrict__ fsegs,
                        const int nseg, const int S, const int normals, const float* __restrict__ campos,
                        float* __restrict__ features) {
  const int idx = blockIdx.x * FEATURE_THREADS + threadIdx.x;
  if (idx >= P) return;
  const SegmentDev* sg = find_segment(segs, nseg, (uint32_t)idx);
  const uint32_t j = (uint32_t)idx - sg->start;
  const int F = 3 * normals + S;
  float* out = features + (size_t)idx * F;
  if (normals) {
    const Normal nm = normal_one(compose_one(*sg, j), campos);
    out[0] = nm.n[0]; out[1] = nm.n[1]; out[2] = nm.n[2];
    out += 3;
  }
  const float* sem = fsegs[sg - segs].semantic;
  if (sem != nullptr) {
    sem += (size_t)j * S;
    for (int c = 0; c < S; c++) out[c] = sem[c];
  } else {
    for (int c = 0; c < S; c++) out[c] = 0.f;
  }
}

__global__ void __launch_bounds__(FEATURE_THREADS)
compose_features_backward_kernel(const int P, const SegmentDev* __restrict__ segs,
                                 const FeatureSegDev* __restrict__ fsegs, const int nseg, const int S,
                                 const int normals, const float* __restrict__ campos,
                                 const float* __restrict__ dL_dfeatures, float* __restrict__ partials,
                                 const uint32_t nslots) {
  __shared__ float s_red[FEATURE_THREADS / 64];
  const int idx = blockIdx.x * FEATURE_THREADS + threadIdx.x;
  const int F = 3 * normals + S;
  float pa[4] = {0.f, 0.f, 0.f, 0.f};
  int seg_index = -1;
  if (idx < P) {
    const SegmentDev* sg = find_segment(segs, nseg, (uint32_t)idx);
    seg_index = (int)(sg - segs);
    const uint32_t j = (uint32_t)idx - sg->start;
    const FeatureSegDev fs = fsegs[seg_index];
    const float* g = dL_dfeatures + (size_t)idx * F;
    if (fs.dL_dsemantic != nullptr) {
      float* o = fs.dL_dsemantic + (size_t)j * S;
      for (int c = 0; c < S; c++) o[c] = g[3 * normals + c];
    }
    if (normals && (fs.dL_drotation != nullptr || sg->rigid)) {
      const Activated a = compose_one(*sg, j);
      const Normal nm = normal_one(a, campos);
      const float gn[3] = {nm.sign * g[0], nm.sign * g[1], nm.sign * g[2]};
      const float4 gu = matrix_column_backward(nm.qu, nm.k, gn);
      // through quaternion_to_matrix's own division by the norm
      const float along = nm.qu.x * gu.x + nm.qu.y * gu.y + nm.qu.z * gu.z + nm.qu.w * gu.w;
      const float4 gq = make_float4((gu.x - nm.qu.x * along) / nm.norm, (gu.y - nm.qu.y * along) / nm.norm,
                                    (gu.z - nm.qu.z * along) / nm.norm, (gu.w - nm.qu.w * along) / nm.norm);
      const float4 gr = rotation_chain_backward(*sg, j, a.q, gq, pa);
      if (fs.dL_drotation != nullptr) {
        float4* o = reinterpret_cast<float4*>(fs.dL_drotation) + j;
        const float4 have = *o;
        *o = make_float4(have.x + gr.x, have.y + gr.y, have.z + gr.z, have.w + gr.w);
      }
    }
  }
  if (!normals) return;
  // the actors' sums: one slot per (workgroup, segment) pair, the workgroup's lanes of other segments count as zero
  const int last = min(P, (int)(blockIdx.x + 1) * FEATURE_THREADS) - 1;
  const int s_first = (int)(find_segment(segs, nseg, (uint32_t)(blockIdx.x * FEATURE_THREADS)) - segs);
  const int s_last = (int)(find_segment(segs, nseg, (uint32_t)last) - segs);
  for (int s = s_first; s <= s_last; s++) {
    if (!segs[s].rigid) continue;   // (uniform over the workgroup)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float t = block_sum<float, float>(seg_index == s ? pa[c] : 0.f, s_red);
      if (threadIdx.x == 0) partials[(size_t)c * nslots + blockIdx.x + (uint32_t)s] = t;
    }
  }
}

// one workgroup per segment: dL_dposes[s][0:4] += the segment's slots, added in a fixed order
__global__ void __launch_bounds__(REDUCE_THREADS)
feature_pose_sum_kernel(const SegmentDev* __restrict__ segs, const float* __restrict__ partials,
                        const uint32_t nslots, float* __restrict__ dL_dposes) {
  __shared__ float s_red[REDUCE_THREADS];
  const uint32_t s = blockIdx.x;
  if (!segs[s].rigid) return;
  const uint32_t w0 = segs[s].start / FEATURE_THREADS, w1 = (segs[s].start + segs[s].count - 1u) / FEATURE_THREADS;
  for (int c = 0; c < 4; c++) {
    const float t = slot_sum(partials + (size_t)c * nslots + w0 + s, w1 - w0 + 1u, s_red);
    if (threadIdx.x == 0) dL_dposes[8 * (size_t)s + c] += t;
  }
}

}  // namespace

void launch_compose_features(hipStream_t st, int P, const SegmentDev* segs, const FeatureSegDev* fsegs, int nseg, int S,
                             int normals, const float* campos, float* features) {
  if (P <= 0 || 3 * normals + S <= 0) return;
  const int grid = (P + FEATURE_THREADS - 1) / FEATURE_THREADS;
  hipLaunchKernelGGL(compose_features_kernel, dim3(grid), dim3(FEATURE_THREADS), 0, st, P, segs, fsegs, nseg, S,
                     normals, campos, features);
}

void launch_compose_features_backward(hipStream_t st, int P, const SegmentDev* segs, const FeatureSegDev* fsegs,
                                      int nseg, int S, int normals, const float* campos, const float* dL_dfeatures,
                                      float* partials, uint32_t nslots, float* dL_dposes) {
  if (P <= 0 || 3 * normals + S <= 0) return;
  const int grid = (P + FEATURE_THREADS - 1) / FEATURE_THREADS;
  hipLaunchKernelGGL(compose_features_backward_kernel, dim3(grid), dim3(FEATURE_THREADS), 0, st, P, segs, fsegs, nseg,
                     S, normals, campos, dL_dfeatures, partials, nslots);
  if (normals)
    hipLaunchKernelGGL(feature_pose_sum_kernel, dim3(nseg), dim3(REDUCE_THREADS), 0, st, segs, partials, nslots,
                       dL_dposes);
}

}  // namespace grpg
