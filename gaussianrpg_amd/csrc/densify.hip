// densify_and_prune of every model in one call: the reference's clone -> split -> prune split parents -> prune
// (gaussian_model.py:363-553, gaussian_model_bkgd.py:74-114, gaussian_model_actor.py:206-263) collapsed into one
// classification per row and one gather pass, with the optimizer moments carried along.
//
// densify_classify_kernel: one thread per (model, row), all models in one launch.  A workgroup owns DN_ROWS rows of
//   ONE model (the table carries each model's first workgroup; a binary search over <= log2(models) entries finds
//   it).  Writes one class byte per row -- split, clone and the four survive bits (original, clone, child 0,
//   child 1) -- and per workgroup the counts of the four output streams and the statistics counters, by 64-lane
//   ballots and popcounts.
// densify_scan_kernel: one workgroup per model: exclusive scan of the per-workgroup stream counts (a thread sums a run
//   of consecutive workgroups, the workgroup scans the 256 sums), the model's totals.
// densify_apply_kernel: a workgroup owns the same DN_ROWS source rows.  It rebuilds the four destination rows of
//   each of its rows in LDS from the class bytes and the scanned bases, then walks each tensor's DN_ROWS x w floats
//   flat, parameter and moments in one loop (coalesced, 16 bytes wide where the arrays' alignment allows, several
//   loads per array in flight before the first store), and stores every float to dest_row * w + column of every
//   surviving copy.  Children recompute xyz and scaling by the function the
//   classification used, from the same noise.  Moments move with surviving originals and are zero for new rows.
//
// The output order is the reference's: surviving originals, clones, children 0, children 1, each ascending in the
// source row.  No atomics, no inter-workgroup communication inside a launch: identical calls give identical bits.
// Built with -ffp-contract=off, so that make_child() rounds alike in both kernels that call it.
#include <cmath>
#include <cstring>
#include <vector>

#include "abi_util.h"
#include "common.h"

namespace grpg {

// The device table both phases upload.  Outside the unnamed namespace: the kernels' symbol names carry it.
struct DensifyTensorDev {
  const float* src;
  const float* src_m;                      // exp_avg / exp_avg_sq, NULL when the optimizer has no state yet
  const float* src_v;
  float* dst;
  float* dst_m;
  float* dst_v;
  uint32_t width;                          // floats per row
  uint32_t vec;                            // 16-byte aligned: bit 0 src, 1 dst, 2 src_m, 3 dst_m, 4 src_v, 5 dst_v
};
struct DensifyModelDev {
  DensifyTensorDev t[GRPG_DENSIFY_MAX_TENSORS];
  const float* accum;                      // [P,2]
  const float* denom;                      // [P]
  const float* split_noise;                // [P,2,3]
  const float* box_noise;                  // [P,4,2,3], box rule only
  const float* xyz;                        // the four tensors the rules read
  const float* opacity;
  const float* scaling;
  const float* rotation;
  float* out_accum;                        // apply only
  float* out_denom;
  float* out_max_radii;
  int* out_src_index;
  unsigned char* cls;                      // workspace slices of this model
  uint32_t* wg_counts;                     // [num_wgs, DN_COUNTERS]
  uint32_t* wg_bases;                      // [num_wgs, 4]
  long long* totals;                       // grpg_densify_counts
  long long n_out;                         // apply only: rows of the output arrays
  uint32_t P, first_wg, num_wgs;
  int num_tensors, xyz_t, scaling_t;
  int grad_column, prune_big, has_sphere, has_box;
  float max_grad, dense_thresh, min_opacity, big_thresh;
  float sphere[4];                         // centre, 2 * radius
  float box_min[3], box_max[3];
};
static_assert(sizeof(DensifyModelDev) <= 768, "the header documents 768 bytes per model");
constexpr size_t DN_TABLE_STRIDE = 768;

namespace {

constexpr int DN_ROWS = 256;               // rows per workgroup == threads
constexpr int DN_WAVES = DN_ROWS / WAVE;
// per-workgroup counters: 0-3 the output streams, then clone, split, below_min_opacity, big_ws, pruned
constexpr int DN_COUNTERS = 12;
constexpr int DN_STATS = 9;
constexpr long long DN_MAX_ROWS = 1ll << 29;   // 3 P output rows stay below 2^31

constexpr uint32_t CLS_SPLIT = 1u, CLS_CLONE = 2u, CLS_SURVIVE_SHIFT = 2;

#define GRPG_GLOBAL __attribute__((address_space(1)))
typedef float v4f __attribute__((ext_vector_type(4)));
typedef GRPG_GLOBAL float gfloat;
typedef GRPG_GLOBAL v4f gv4f;

// general_utils.quaternion_to_matrix: q = r / |r|, then the nine entries as written there
__device__ __forceinline__ void quat_matrix(const gfloat* __restrict__ q4, float R[9]) {
  const float a = q4[0], b = q4[1], c = q4[2], d = q4[3];
  const float norm = sqrtf(a * a + b * b + c * c + d * d);
  const float r = a / norm, x = b / norm, y = c / norm, z = d / norm;
  R[0] = 1.f - 2.f * (y * y + z * z);
  R[1] = 2.f * (x * y - r * z);
  R[2] = 2.f * (x * z + r * y);
  R[3] = 2.f * (x * y + r * z);
  R[4] = 1.f - 2.f * (x * x + z * z);
  R[5] = 2.f * (y * z - r * x);
  R[6] = 2.f * (x * z - r * y);
  R[7] = 2.f * (y * z + r * x);
  R[8] = 1.f - 2.f * (x * x + y * y);
}

// R (n * s) + o
__device__ __forceinline__ void place(const float R[9], const float n0, const float n1, const float n2,
                                      const float s[3], const float o[3], float out[3]) {
  const float v0 = n0 * s[0], v1 = n1 * s[1], v2 = n2 * s[2];
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = (R[3 * k] * v0 + R[3 * k + 1] * v1 + R[3 * k + 2] * v2) + o[k];
}

struct RowGeom {
  float R[9];
  float s[3];                              // exp(scaling)
  float o[3];                              // xyz
};

__device__ __forceinline__ void load_geom(const DensifyModelDev& M, const uint32_t i, RowGeom& g) {
  const gfloat* sc = (const gfloat*)M.scaling + 3 * (size_t)i;
  const gfloat* xy = (const gfloat*)M.xyz + 3 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    g.s[k] = expf(sc[k]);
    g.o[k] = xy[k];
  }
  quat_matrix((const gfloat*)M.rotation + 4 * (size_t)i, g.R);
}

// child c of a split row: xyz = R (noise * exp(scaling)) + xyz, scaling = log(exp(scaling) / 1.6); also its scales.
// The classification and the apply pass both call this, so a child's values are the ones its fate was decided on.
__device__ __forceinline__ void make_child(const DensifyModelDev& M, const uint32_t i, const int c, const RowGeom& g,
                                           float xyz_c[3], float scaling_c[3], float s_c[3]) {
  const gfloat* n = (const gfloat*)M.split_noise + 6 * (size_t)i + 3 * c;
  place(g.R, n[0], n[1], n[2], g.s, g.o, xyz_c);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s_c[k] = g.s[k] / 1.6f;
    scaling_c[k] = logf(s_c[k]);
  }
}

__device__ __forceinline__ float max3(const float s[3]) { return fmaxf(fmaxf(s[0], s[1]), s[2]); }

// world-space size rule of one candidate: its own largest scale, exempt far outside the sphere (background model)
__device__ __forceinline__ bool big_ws(const DensifyModelDev& M, const float smax, const float o[3]) {
  bool big = smax > M.big_thresh;
  if (M.has_sphere) {
    const float dx = o[0] - M.sphere[0], dy = o[1] - M.sphere[1], dz = o[2] - M.sphere[2];
    if (sqrtf(dx * dx + dy * dy + dz * dz) > M.sphere[3]) big = false;
  }
  return big;
}

// either of the two samples of noise slot `slot` outside [box_min, box_max] (actor model)
__device__ __forceinline__ bool outside_box(const DensifyModelDev& M, const uint32_t i, const int slot,
                                            const float R[9], const float s[3], const float o[3]) {
  const gfloat* n = (const gfloat*)M.box_noise + 24 * (size_t)i + 6 * slot;
  bool inside = true;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    float p[3];
    place(R, n[3 * j], n[3 * j + 1], n[3 * j + 2], s, o, p);
#pragma unroll
    for (int k = 0; k < 3; k++) inside = inside && p[k] >= M.box_min[k] && p[k] <= M.box_max[k];
  }
  return !inside;
}

// the sum over the wave of a small per-lane count (< 8), by ballots of its bits
__device__ __forceinline__ uint32_t wave_sum3(const uint32_t c) {
  return (uint32_t)__popcll(__ballot(c & 1u)) + 2u * (uint32_t)__popcll(__ballot(c & 2u)) +
         4u * (uint32_t)__popcll(__ballot(c & 4u));
}

// the last model whose first workgroup is <= wg (a model without rows owns none and shares the value of the next)
__device__ __forceinline__ int find_model(const char* __restrict__ table, const int num_models, const uint32_t wg) {
  int lo = 0, hi = num_models - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (((const DensifyModelDev*)(table + DN_TABLE_STRIDE * mid))->first_wg <= wg) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(DN_ROWS)
densify_classify_kernel(const char* __restrict__ table, const int num_models) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_STATS];
  const DensifyModelDev& M = *(const DensifyModelDev*)(table + DN_TABLE_STRIDE * find_model(table, num_models, blockIdx.x));
  const uint32_t lw = blockIdx.x - M.first_wg;
  const uint32_t tid = threadIdx.x;
  const uint32_t i = lw * DN_ROWS + tid;
  uint32_t cnt[DN_STATS];
#pragma unroll
  for (int k = 0; k < DN_STATS; k++) cnt[k] = 0;
  if (i < M.P) {
    float g = ((const gfloat*)M.accum)[2 * (size_t)i + M.grad_column] / ((const gfloat*)M.denom)[i];
    if (g != g) g = 0.f;                                   // grads[grads.isnan()] = 0; inf stays
    RowGeom geom;
    load_geom(M, i, geom);
    const float smax = max3(geom.s);
    const bool sel = g >= M.max_grad;
    const bool clone = sel && smax <= M.dense_thresh;
    const bool split = sel && smax > M.dense_thresh;
    const float op = ((const gfloat*)M.opacity)[i];
    const bool low = 1.f / (1.f + expf(-op)) < M.min_opacity;
    // the original and its clone hold the same values; only their box noise differs
    const bool big_o = M.prune_big && big_ws(M, smax, geom.o);
    bool out_o = false, out_cl = false;
    if (M.has_box && M.prune_big) {
      out_o = outside_box(M, i, 0, geom.R, geom.s, geom.o);
      if (clone) out_cl = outside_box(M, i, 1, geom.R, geom.s, geom.o);
    }
    const bool pruned_o = low || big_o || out_o;
    const bool pruned_cl = low || big_o || out_cl;
    uint32_t cls = (split ? CLS_SPLIT : 0u) | (clone ? CLS_CLONE : 0u);
    const uint32_t orig = split ? 0u : 1u, cl = clone ? 1u : 0u;
    if (!split && !pruned_o) cls |= 1u << CLS_SURVIVE_SHIFT;
    if (clone && !pruned_cl) cls |= 2u << CLS_SURVIVE_SHIFT;
    cnt[4] = cl;
    cnt[5] = split ? 1u : 0u;
    cnt[6] = low ? orig + cl : 0u;
    cnt[7] = big_o ? orig + cl : 0u;
    cnt[8] = (pruned_o ? orig : 0u) + (pruned_cl ? cl : 0u);
    if (split) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        float xyz_c[3], scaling_c[3], s_c[3];
        make_child(M, i, c, geom, xyz_c, scaling_c, s_c);
        const bool big_c = M.prune_big && big_ws(M, max3(s_c), xyz_c);
        const bool out_c = M.has_box && M.prune_big && outside_box(M, i, 2 + c, geom.R, s_c, xyz_c);
        const bool pruned_c = low || big_c || out_c;
        if (!pruned_c) cls |= (4u << c) << CLS_SURVIVE_SHIFT;
        cnt[6] += low ? 1u : 0u;
        cnt[7] += big_c ? 1u : 0u;
        cnt[8] += pruned_c ? 1u : 0u;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) cnt[s] = (cls >> (CLS_SURVIVE_SHIFT + s)) & 1u;
    M.cls[i] = (unsigned char)cls;
  }
  const uint32_t wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
  for (int k = 0; k < DN_STATS; k++) {
    const uint32_t sum = wave_sum3(cnt[k]);
    if (lane == 0) s_cnt[wave][k] = sum;
  }
  __syncthreads();
  if (tid < DN_COUNTERS) {
    uint32_t sum = 0;
    if (tid < DN_STATS)
      for (int w = 0; w < DN_WAVES; w++) sum += s_cnt[w][tid];
    M.wg_counts[(size_t)lw * DN_COUNTERS + tid] = sum;
  }
}

__global__ void __launch_bounds__(DN_ROWS)
densify_scan_kernel(const char* __restrict__ table) {
  __shared__ uint32_t s_wave[DN_WAVES][4];
  __shared__ unsigned long long s_stat[DN_WAVES][5];
  const DensifyModelDev& M = *(const DensifyModelDev*)(table + DN_TABLE_STRIDE * blockIdx.x);
  const uint32_t tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  typedef GRPG_GLOBAL u4 gu4;
  // a thread owns a run of consecutive workgroups: its loads are independent of one another, and the workgroup
  // scans one value per thread and stream instead of looping over the table
  const uint32_t per = (M.num_wgs + DN_ROWS - 1) / DN_ROWS;
  const uint32_t lo = tid * per < M.num_wgs ? tid * per : M.num_wgs;
  const uint32_t hi = lo + per < M.num_wgs ? lo + per : M.num_wgs;
  const gu4* const rows = (const gu4*)M.wg_counts;          // three 16-byte pieces per workgroup
  uint32_t sum[4] = {0, 0, 0, 0};
  unsigned long long stat[5] = {0, 0, 0, 0, 0};
  for (uint32_t w = lo; w < hi; w++) {
    const u4 a = rows[3 * (size_t)w], b = rows[3 * (size_t)w + 1], c = rows[3 * (size_t)w + 2];
    sum[0] += a[0]; sum[1] += a[1]; sum[2] += a[2]; sum[3] += a[3];
    stat[0] += b[0]; stat[1] += b[1]; stat[2] += b[2]; stat[3] += b[3]; stat[4] += c[0];
  }
  uint32_t run[4], total[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    uint32_t x = sum[s];
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, WAVE);
      if ((int)lane >= d) x += y;
    }
    run[s] = x - sum[s];
    if (lane == WAVE - 1) s_wave[wave][s] = x;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    unsigned long long x = stat[k];
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) x += __shfl_down(x, d, WAVE);
    if (lane == 0) s_stat[wave][k] = x;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; s++) {
    total[s] = 0;
    for (int k = 0; k < DN_WAVES; k++) {
      const uint32_t t = s_wave[k][s];
      if (k < (int)wave) run[s] += t;
      total[s] += t;
    }
  }
  for (uint32_t w = lo; w < hi; w++) {
    const u4 a = rows[3 * (size_t)w];
    ((gu4*)M.wg_bases)[w] = u4{run[0], run[1], run[2], run[3]};
    run[0] += a[0]; run[1] += a[1]; run[2] += a[2]; run[3] += a[3];
  }
  if (tid == 0) {
    long long* out = M.totals;
    out[0] = (long long)total[0] + total[1] + total[2] + total[3];
    for (int s = 0; s < 4; s++) out[1 + s] = total[s];
    for (int k = 0; k < 5; k++) {
      unsigned long long all = 0;
      for (int w = 0; w < DN_WAVES; w++) all += s_stat[w][k];
      out[5 + k] = (long long)all;
    }
  }
}

// what the copy of a tensor stores for a source float: the parameter itself or, for xyz and scaling, a child's
// recomputed value
enum CopyKind { COPY_PARAM = 0, COPY_XYZ = 1, COPY_SCALING = 2 };
constexpr int DN_UNROLL = 4;               // loads of this many pieces per thread are in flight before the first store

struct CopyArrays {
  const gfloat* __restrict__ src;          // the workgroup's first source row
  const gfloat* __restrict__ src_m;
  const gfloat* __restrict__ src_v;
  gfloat* __restrict__ dst;
  gfloat* __restrict__ dst_m;
  gfloat* __restrict__ dst_v;
};

// One tensor and, with MOM, its two moments: the workgroup's nrows x w source floats walked flat, every float stored
// to dest_row * w + column of each surviving copy of its row.  The moments of an original move with it; every new
// row's are zero.
template <int KIND, bool MOM>
__device__ __forceinline__ void copy_rows(const CopyArrays A, const uint32_t w, const uint32_t nrows,
                                          const bool vec_src, const bool vec_dst, const int (*dest)[DN_ROWS],
                                          const float (*child)[DN_ROWS][6], const uint32_t tid) {
  const uint32_t n = nrows * w;
  auto emit = [&](const uint32_t r, const uint32_t c, const float p, const float m, const float v) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int d = dest[s][r];
      if (d < 0) continue;
      const size_t o = (size_t)d * w + c;
      float out = p;
      if (KIND == COPY_XYZ && s >= 2) out = child[s - 2][r][c];
      if (KIND == COPY_SCALING && s >= 2) out = child[s - 2][r][3 + c];
      A.dst[o] = out;
      if (MOM) {
        A.dst_m[o] = s == 0 ? m : 0.f;
        A.dst_v[o] = s == 0 ? v : 0.f;
      }
    }
  };
  uint32_t done = 0;
  if (vec_src) {
    const uint32_t nvec = n >> 2;
    const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
    for (uint32_t base = 0; base < nvec; base += DN_ROWS * DN_UNROLL) {
      v4f vp[DN_UNROLL], vm[DN_UNROLL], vv[DN_UNROLL];
#pragma unroll
      for (int u = 0; u < DN_UNROLL; u++) {
        const uint32_t q = base + u * DN_ROWS + tid;
        vp[u] = vm[u] = vv[u] = zero;
        if (q < nvec) {
          vp[u] = ((const gv4f*)A.src)[q];
          if (MOM) {
            vm[u] = ((const gv4f*)A.src_m)[q];
            vv[u] = ((const gv4f*)A.src_v)[q];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < DN_UNROLL; u++) {
        const uint32_t q = base + u * DN_ROWS + tid;
        if (q >= nvec) continue;
        const uint32_t e = q << 2;
        uint32_t r = e / w, c = e - r * w;
        if (KIND == COPY_PARAM && c + 3 < w) {          // the four floats lie in one row
#pragma unroll
          for (int s = 0; s < 4; s++) {
            const int d = dest[s][r];
            if (d < 0) continue;
            const size_t o = (size_t)d * w + c;
            const v4f om = s == 0 ? vm[u] : zero, ov = s == 0 ? vv[u] : zero;
            if (vec_dst && (o & 3) == 0) {
              *(gv4f*)(A.dst + o) = vp[u];
              if (MOM) {
                *(gv4f*)(A.dst_m + o) = om;
                *(gv4f*)(A.dst_v + o) = ov;
              }
            } else {
#pragma unroll
              for (int k = 0; k < 4; k++) {
                A.dst[o + k] = vp[u][k];
                if (MOM) {
                  A.dst_m[o + k] = om[k];
                  A.dst_v[o + k] = ov[k];
                }
              }
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            emit(r, c, vp[u][k], vm[u][k], vv[u][k]);
            if (++c == w) { c = 0; r++; }
          }
        }
      }
    }
    done = nvec << 2;
  }
  // a misaligned source (all of it) or the last n % 4 floats
  for (uint32_t base = done; base < n; base += DN_ROWS * DN_UNROLL) {
    float fp[DN_UNROLL], fm[DN_UNROLL], fv[DN_UNROLL];
#pragma unroll
    for (int u = 0; u < DN_UNROLL; u++) {
      const uint32_t e = base + u * DN_ROWS + tid;
      fp[u] = fm[u] = fv[u] = 0.f;
      if (e < n) {
        fp[u] = A.src[e];
        if (MOM) {
          fm[u] = A.src_m[e];
          fv[u] = A.src_v[e];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < DN_UNROLL; u++) {
      const uint32_t e = base + u * DN_ROWS + tid;
      if (e >= n) continue;
      const uint32_t r = e / w;
      emit(r, e - r * w, fp[u], fm[u], fv[u]);
    }
  }
}

template <int KIND>
__device__ __forceinline__ void copy_tensor(const DensifyTensorDev& T, const uint32_t row0, const uint32_t nrows,
                                            const int (*dest)[DN_ROWS], const float (*child)[DN_ROWS][6],
                                            const uint32_t tid) {
  const uint32_t w = T.width;
  const size_t off = (size_t)row0 * w;
  const CopyArrays A{(const gfloat*)T.src + off, (const gfloat*)T.src_m + off, (const gfloat*)T.src_v + off,
                     (gfloat*)T.dst, (gfloat*)T.dst_m, (gfloat*)T.dst_v};
  if (T.src_m)
    copy_rows<KIND, true>(A, w, nrows, (T.vec & 21u) == 21u, (T.vec & 42u) == 42u, dest, child, tid);
  else
    copy_rows<KIND, false>(A, w, nrows, T.vec & 1u, T.vec & 2u, dest, child, tid);
}

__global__ void __launch_bounds__(DN_ROWS)
densify_apply_kernel(const char* __restrict__ table, const int num_models) {
  __shared__ int s_dest[4][DN_ROWS];
  __shared__ float s_child[2][DN_ROWS][6];
  __shared__ uint32_t s_wave[DN_WAVES][4];
  const DensifyModelDev& M = *(const DensifyModelDev*)(table + DN_TABLE_STRIDE * find_model(table, num_models, blockIdx.x));
  const uint32_t lw = blockIdx.x - M.first_wg;
  const uint32_t tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const uint32_t row0 = lw * DN_ROWS;
  const uint32_t nrows = M.P - row0 < (uint32_t)DN_ROWS ? M.P - row0 : (uint32_t)DN_ROWS;
  const uint32_t i = row0 + tid;
  const uint32_t cls = tid < nrows ? M.cls[i] : 0u;
  uint32_t rank[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const unsigned long long b = __ballot((cls >> (CLS_SURVIVE_SHIFT + s)) & 1u);
    rank[s] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave][s] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  long long stream_off = 0;
  int any_child = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    long long d = -1;
    if ((cls >> (CLS_SURVIVE_SHIFT + s)) & 1u) {
      uint32_t before = 0;
      for (int k = 0; k < (int)wave; k++) before += s_wave[k][s];
      d = stream_off + M.wg_bases[(size_t)lw * 4 + s] + before + rank[s];
      if (d >= M.n_out) d = -1;             // arrays smaller than the plan's counts: never write past them
    }
    stream_off += M.totals[1 + s];
    s_dest[s][tid] = (int)d;
    if (d >= 0) {
      if (s >= 2) any_child = 1;
      ((GRPG_GLOBAL int*)M.out_src_index)[d] = (int)i;
      ((gfloat*)M.out_accum)[2 * (size_t)d] = 0.f;
      ((gfloat*)M.out_accum)[2 * (size_t)d + 1] = 0.f;
      ((gfloat*)M.out_denom)[d] = 0.f;
      ((gfloat*)M.out_max_radii)[d] = 0.f;
    }
  }
  if (any_child) {
    RowGeom geom;
    load_geom(M, i, geom);
#pragma unroll
    for (int c = 0; c < 2; c++) {
      float xyz_c[3], scaling_c[3], s_c[3];
      make_child(M, i, c, geom, xyz_c, scaling_c, s_c);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        s_child[c][tid][k] = xyz_c[k];
        s_child[c][tid][3 + k] = scaling_c[k];
      }
    }
  }
  __syncthreads();
  for (int t = 0; t < M.num_tensors; t++) {
    const DensifyTensorDev T = M.t[t];
    if (T.width == 0) continue;
    if (t == M.xyz_t)
      copy_tensor<COPY_XYZ>(T, row0, nrows, s_dest, s_child, tid);
    else if (t == M.scaling_t)
      copy_tensor<COPY_SCALING>(T, row0, nrows, s_dest, s_child, tid);
    else
      copy_tensor<COPY_PARAM>(T, row0, nrows, s_dest, s_child, tid);
  }
}

struct WsLayout {
  size_t cls = 0, counts = 0, bases = 0, totals = 0, total = 0;
  unsigned long long wgs = 0;
};

inline unsigned long long model_wgs(long long P) { return ((unsigned long long)P + DN_ROWS - 1) / DN_ROWS; }

// class bytes of all models (DN_ROWS per workgroup), the per-workgroup counters and bases, the per-model totals
bool ws_layout(const long long* P, int num_models, WsLayout& L) {
  if (!P || num_models <= 0) return false;
  unsigned long long wgs = 0;
  for (int m = 0; m < num_models; m++) {
    if (P[m] < 0 || P[m] > DN_MAX_ROWS) return false;
    wgs += model_wgs(P[m]);
  }
  if (wgs > 0x7FFFFFFFull) return false;
  L.wgs = wgs;
  L.cls = 0;
  L.counts = align_up(L.cls + (size_t)wgs * DN_ROWS, 256);
  L.bases = align_up(L.counts + (size_t)wgs * DN_COUNTERS * sizeof(uint32_t), 256);
  L.totals = align_up(L.bases + (size_t)wgs * 4 * sizeof(uint32_t), 256);
  L.total = align_up(L.totals + (size_t)num_models * sizeof(grpg_densify_counts), 256);
  return true;
}

bool finite_all(const float* v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// Every argument check of both phases; nothing is queued before it passes.  outputs: NULL for the plan.
int check_models(const char* what, const grpg_densify_model* models, int num_models, const void* workspace,
                 const grpg_densify_output* outputs, grpg_alloc_fn table_alloc) {
  const std::string w(what);
  if (num_models < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": negative model count");
  if (num_models == 0) return GRPG_OK;
  if (!models) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL model table");
  if (!workspace || ((uintptr_t)workspace & 15))
    return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": the workspace must be a 16-byte aligned device array");
  if (!table_alloc) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL table allocator");
  unsigned long long wgs = 0;
  for (int m = 0; m < num_models; m++) {
    const grpg_densify_model& g = models[m];
    if (g.P < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": model with negative P");
    if (g.P > DN_MAX_ROWS) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": more than 2^29 rows in one model");
    wgs += model_wgs(g.P);
    if (g.num_tensors < 0 || g.num_tensors > GRPG_DENSIFY_MAX_TENSORS)
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": num_tensors outside [0, GRPG_DENSIFY_MAX_TENSORS]");
    const int special[4] = {g.xyz_index, g.opacity_index, g.scaling_index, g.rotation_index};
    const int widths[4] = {3, 1, 3, 4};
    for (int k = 0; k < 4; k++) {
      if (special[k] < 0 || special[k] >= g.num_tensors || g.tensors[special[k]].width != widths[k])
        return fail(GRPG_ERR_INVALID_ARGUMENT,
                    w + ": xyz / opacity / scaling / rotation must index tensors of width 3 / 1 / 3 / 4");
    }
    if (g.grad_column != 0 && g.grad_column != 1)
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": grad_column must be 0 or 1");
    if (!std::isfinite(g.max_grad) || !(g.max_grad > 0.f))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": max_grad must be finite and positive");
    if (!std::isfinite(g.percent_dense) || !std::isfinite(g.extent) || !std::isfinite(g.min_opacity) ||
        !std::isfinite(g.percent_big_ws) || (g.has_sphere && !(finite_all(g.sphere_center, 3) &&
        std::isfinite(g.sphere_radius))) || (g.has_box && !(finite_all(g.box_min, 3) && finite_all(g.box_max, 3))))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": non-finite rule value");
    for (int t = 0; t < g.num_tensors; t++) {
      const grpg_densify_tensor& T = g.tensors[t];
      if (T.width < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": tensor with negative width");
      if ((T.exp_avg == nullptr) != (T.exp_avg_sq == nullptr))
        return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": exp_avg and exp_avg_sq must both be given or both be NULL");
      if (g.P > 0 && T.width > 0 && !T.param)
        return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL array with P > 0");
      if (misaligned(T.param) || misaligned(T.exp_avg) || misaligned(T.exp_avg_sq))
        return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": arrays must be 4-byte aligned");
    }
    if (g.P > 0 && (!g.xyz_gradient_accum || !g.denom || !g.split_noise || (g.has_box && g.prune_big && !g.box_noise)))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL array with P > 0");
    if (misaligned(g.xyz_gradient_accum) || misaligned(g.denom) || misaligned(g.split_noise) ||
        misaligned(g.box_noise))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": arrays must be 4-byte aligned");
    if (!outputs) continue;
    const grpg_densify_output& o = outputs[m];
    if (o.n_out < 0 || o.n_out > 3 * g.P)
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": n_out outside [0, 3 P]");
    if (o.n_out > 0 && (!o.xyz_gradient_accum || !o.denom || !o.max_radii2D || !o.src_index))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL output array with n_out > 0");
    if (misaligned(o.xyz_gradient_accum) || misaligned(o.denom) || misaligned(o.max_radii2D) ||
        misaligned(o.src_index))
      return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": arrays must be 4-byte aligned");
    for (int t = 0; t < g.num_tensors; t++) {
      const grpg_densify_tensor& T = g.tensors[t];
      const grpg_densify_out_tensor& O = o.tensors[t];
      if (o.n_out > 0 && T.width > 0 && (!O.param || (T.exp_avg && (!O.exp_avg || !O.exp_avg_sq))))
        return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": NULL output array with n_out > 0");
      if (misaligned(O.param) || misaligned(O.exp_avg) || misaligned(O.exp_avg_sq))
        return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": arrays must be 4-byte aligned");
    }
  }
  if (wgs > 0x7FFFFFFFull) return fail(GRPG_ERR_INVALID_ARGUMENT, w + ": more than 2^31 workgroups of 256 rows");
  return GRPG_OK;
}

uint32_t aligned16(const void* p, uint32_t bit) { return ((uintptr_t)p & 15) == 0 ? bit : 0u; }

// The device table of one phase, written into pinned staging and queued for upload; *dev_out receives its device
// address.  Returns the total number of workgroups through *wgs_out.
int upload_table(const char* what, const grpg_densify_model* models, int num_models, void* workspace,
                 const grpg_densify_output* outputs, grpg_alloc_fn table_alloc, void* table_user, hipStream_t stream,
                 char** dev_out, WsLayout& L) {
  std::vector<long long> P((size_t)num_models);
  for (int m = 0; m < num_models; m++) P[(size_t)m] = models[m].P;
  if (!ws_layout(P.data(), num_models, L)) return fail(GRPG_ERR_INVALID_ARGUMENT, std::string(what) + ": bad sizes");
  const size_t bytes = DN_TABLE_STRIDE * (size_t)num_models;
  OptimStagingSlot* stg = optim_staging_acquire(bytes);
  if (!stg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  char* ws = (char*)workspace;
  unsigned long long first = 0;
  for (int m = 0; m < num_models; m++) {
    const grpg_densify_model& g = models[m];
    DensifyModelDev d{};
    for (int t = 0; t < g.num_tensors; t++) {
      const grpg_densify_tensor& T = g.tensors[t];
      DensifyTensorDev& D = d.t[t];
      D.src = T.param; D.src_m = T.exp_avg; D.src_v = T.exp_avg_sq;
      D.width = (uint32_t)T.width;
      D.vec = aligned16(T.param, 1u) | aligned16(T.exp_avg, 4u) | aligned16(T.exp_avg_sq, 16u);
      if (outputs) {
        const grpg_densify_out_tensor& O = outputs[m].tensors[t];
        D.dst = O.param; D.dst_m = O.exp_avg; D.dst_v = O.exp_avg_sq;
        D.vec |= aligned16(O.param, 2u) | aligned16(O.exp_avg, 8u) | aligned16(O.exp_avg_sq, 32u);
      }
    }
    d.accum = g.xyz_gradient_accum; d.denom = g.denom; d.split_noise = g.split_noise; d.box_noise = g.box_noise;
    d.xyz = g.tensors[g.xyz_index].param; d.opacity = g.tensors[g.opacity_index].param;
    d.scaling = g.tensors[g.scaling_index].param; d.rotation = g.tensors[g.rotation_index].param;
    if (outputs) {
      const grpg_densify_output& o = outputs[m];
      d.out_accum = o.xyz_gradient_accum; d.out_denom = o.denom; d.out_max_radii = o.max_radii2D;
      d.out_src_index = o.src_index;
      d.n_out = o.n_out;
    }
    d.cls = (unsigned char*)ws + L.cls + (size_t)first * DN_ROWS;
    d.wg_counts = (uint32_t*)(ws + L.counts) + (size_t)first * DN_COUNTERS;
    d.wg_bases = (uint32_t*)(ws + L.bases) + (size_t)first * 4;
    d.totals = (long long*)(ws + L.totals + (size_t)m * sizeof(grpg_densify_counts));
    d.P = (uint32_t)g.P; d.first_wg = (uint32_t)first; d.num_wgs = (uint32_t)model_wgs(g.P);
    d.num_tensors = g.num_tensors; d.xyz_t = g.xyz_index; d.scaling_t = g.scaling_index;
    d.grad_column = g.grad_column; d.prune_big = g.prune_big != 0; d.has_sphere = g.has_sphere != 0;
    d.has_box = g.has_box != 0;
    d.max_grad = g.max_grad;
    // the reference multiplies Python floats and compares a float32 tensor with the product
    d.dense_thresh = (float)((double)g.percent_dense * (double)g.extent);
    d.min_opacity = g.min_opacity;
    d.big_thresh = (float)((double)g.extent * (double)g.percent_big_ws);
    for (int k = 0; k < 3; k++) {
      d.sphere[k] = g.sphere_center[k];
      d.box_min[k] = g.box_min[k];
      d.box_max[k] = g.box_max[k];
    }
    d.sphere[3] = (float)(2.0 * (double)g.sphere_radius);
    memcpy(stg->host + DN_TABLE_STRIDE * (size_t)m, &d, sizeof(d));
    first += d.num_wgs;
  }
  char* dev = table_alloc(bytes, table_user);
  if (!dev) return fail(GRPG_ERR_ALLOC, std::string(what) + ": the table allocator returned NULL");
  if ((uintptr_t)dev & 7) return fail(GRPG_ERR_INVALID_ARGUMENT, std::string(what) + ": the table must be 8-byte aligned");
  HIP_TRY(hipMemcpyAsync(dev, stg->host, bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(stg->ev, stream));
  *dev_out = dev;
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_densify_workspace_bytes(const long long* P, int num_models) {
  WsLayout L;
  return ws_layout(P, num_models, L) ? L.total : 0;
}

int grpg_densify_plan(const grpg_densify_model* models, int num_models, void* workspace,
                      grpg_densify_counts* counts_host, grpg_alloc_fn table_alloc, void* table_user,
                      void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = check_models("densify_plan", models, num_models, workspace, nullptr, table_alloc)) return rc;
  if (num_models == 0) return GRPG_OK;
  if (!counts_host) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_plan: NULL counts_host");
  hipStream_t stream = (hipStream_t)hip_stream;
  char* dev = nullptr;
  WsLayout L;
  if (int rc = upload_table("densify_plan", models, num_models, workspace, nullptr, table_alloc, table_user, stream,
                            &dev, L))
    return rc;
  if (L.wgs > 0) {
    hipLaunchKernelGGL(densify_classify_kernel, dim3((uint32_t)L.wgs), dim3(DN_ROWS), 0, stream, (const char*)dev,
                       num_models);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(densify_scan_kernel, dim3((uint32_t)num_models), dim3(DN_ROWS), 0, stream, (const char*)dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(counts_host, (char*)workspace + L.totals, sizeof(grpg_densify_counts) * (size_t)num_models,
                         hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));      // the one host wait of the feature: the caller sizes its arrays
  return GRPG_OK;
}

int grpg_densify_apply(const grpg_densify_model* models, int num_models, void* workspace,
                       const grpg_densify_output* outputs, grpg_alloc_fn table_alloc, void* table_user,
                       void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (num_models > 0 && !outputs) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_apply: NULL output table");
  if (int rc = check_models("densify_apply", models, num_models, workspace, outputs, table_alloc)) return rc;
  if (num_models == 0) return GRPG_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  char* dev = nullptr;
  WsLayout L;
  if (int rc = upload_table("densify_apply", models, num_models, workspace, outputs, table_alloc, table_user, stream,
                            &dev, L))
    return rc;
  if (L.wgs == 0) return GRPG_OK;
  hipLaunchKernelGGL(densify_apply_kernel, dim3((uint32_t)L.wgs), dim3(DN_ROWS), 0, stream, (const char*)dev,
                     num_models);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
