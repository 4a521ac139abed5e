// The tail of the training iteration: optimizer.step() of every model and the densification statistics.
//
// adam_step_kernel: the step of torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False) over EVERY
// tensor of EVERY optimizer in one launch.  One pass over the data: read p, g, m, v; write p, m, v (28 B per
// element), where the foreach path of torch.optim.Adam makes ~10 launches per optimizer, each a pass of its own.
// The tensors are described by a device table of segments; the work is cut into chunks of ADAM_CHUNK_ELEMS elements
// that never straddle a segment, and the table carries for each segment the index of its first chunk, so that
// a workgroup finds the segment of chunk c by a binary search over <= log2(segments) table entries (L2 hits).
// The grid is capped at ADAM_MAX_WGS workgroups which stride over the chunks.
//
// densify_stats_kernel: set_max_radii2D + add_densification_stats of the reference's StreetGaussianModel for all
// models of a composed frame in one launch: one thread per Gaussian, no atomics (the ranges are disjoint).
//
// Built with -ffp-contract=off: every operation below rounds once, in the order written (the tests' 2-ulp bound
// for sqrt(x*x + y*y) is derived for that, and the Adam arithmetic is then the same on every path of the kernel,
// vector or scalar, which the bit-identity tests rely on).  No atomics, no inter-workgroup communication:
// identical calls give identical bits.
#include <cmath>

#include "abi_util.h"
#include "common.h"

namespace grpg {

// The device tables the entries upload.  Outside the unnamed namespace: the kernels' symbol names carry them.
struct AdamSegmentDev {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  unsigned long long n;                    // elements (> 0)
  float step_size, bc2_sqrt, beta2, one_minus_beta1, one_minus_beta2, eps;
  uint32_t first_chunk;                    // chunks of the segments before this one
  uint32_t vec;                            // all four arrays 16-byte aligned: 16-byte loads and stores
};
struct DensifyRangeDev {
  float* accum;                            // [n, 2]
  float* denom;                            // [n]
  float* max_radii;                        // [n]
  int start, end;                          // half-open range of the composed frame, n = end - start > 0
};
static_assert(sizeof(DensifyRangeDev) == 32, "the header documents 32 bytes per range");

namespace {

constexpr int ADAM_THREADS = 256;
#ifndef GRPG_ADAM_UNROLL
#define GRPG_ADAM_UNROLL 4
#endif
#ifndef GRPG_ADAM_MAX_WGS
#define GRPG_ADAM_MAX_WGS 2048   // 256 CUs x 8 resident workgroups
#endif
constexpr int ADAM_UNROLL = GRPG_ADAM_UNROLL;                       // float4 per thread and chunk
// elements per unit of work (4096 = 16 KB per array); a chunk never straddles two segments
constexpr uint32_t ADAM_CHUNK_ELEMS = ADAM_THREADS * 4 * ADAM_UNROLL;
static_assert(ADAM_CHUNK_ELEMS == 4096, "grpg_adam_step's error text names the chunk size");

// The table's pointers are loaded from memory, so the compiler cannot know their address space and would emit
// flat_load / flat_store; they are device global memory by the entry's contract.
#define GRPG_GLOBAL __attribute__((address_space(1)))
typedef float v4f __attribute__((ext_vector_type(4)));
typedef GRPG_GLOBAL float gfloat;
typedef GRPG_GLOBAL v4f gv4f;

struct AdamCoef {
  float step_size, bc2_sqrt, beta2, omb1, omb2, eps;
};

// m = m + (g - m)(1 - b1);  v = v b2 + (g g)(1 - b2);  p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
__device__ __forceinline__ void adam_one(float& p, const float g, float& m, float& v, const AdamCoef& c) {
  m = m + (g - m) * c.omb1;
  v = v * c.beta2 + (g * g) * c.omb2;
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = p - c.step_size * (m / denom);
}

__device__ __forceinline__ void adam_four(v4f& p, const v4f& g, v4f& m, v4f& v, const AdamCoef& c) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    float pe = p[e], me = m[e], ve = v[e];
    adam_one(pe, g[e], me, ve, c);
    p[e] = pe; m[e] = me; v[e] = ve;
  }
}

__global__ void __launch_bounds__(ADAM_THREADS)
adam_step_kernel(const AdamSegmentDev* __restrict__ table, const int num_segments, const uint32_t total_chunks) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    // the last segment whose first chunk is <= c (segments without elements own no chunk and are not in the table)
    int lo = 0, hi = num_segments - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (table[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
    }
    const AdamSegmentDev s = table[lo];
    const AdamCoef k{s.step_size, s.bc2_sqrt, s.beta2, s.one_minus_beta1, s.one_minus_beta2, s.eps};
    const unsigned long long base = (unsigned long long)(c - s.first_chunk) * ADAM_CHUNK_ELEMS;
    const unsigned long long left = s.n - base;
    const uint32_t len = left < ADAM_CHUNK_ELEMS ? (uint32_t)left : ADAM_CHUNK_ELEMS;
    gfloat* const p = (gfloat*)s.param + base;
    const gfloat* const g = (const gfloat*)s.grad + base;
    gfloat* const m = (gfloat*)s.exp_avg + base;
    gfloat* const v = (gfloat*)s.exp_avg_sq + base;
    if (s.vec && len == ADAM_CHUNK_ELEMS) {
      // whole chunk, four 16-byte aligned arrays: every load of the chunk in flight before the first use
      gv4f* const p4 = (gv4f*)p;
      const gv4f* const g4 = (const gv4f*)g;
      gv4f* const m4 = (gv4f*)m;
      gv4f* const v4 = (gv4f*)v;
      v4f rp[ADAM_UNROLL], rg[ADAM_UNROLL], rm[ADAM_UNROLL], rv[ADAM_UNROLL];
#pragma unroll
      for (int u = 0; u < ADAM_UNROLL; u++) {
        const uint32_t i = tid + u * ADAM_THREADS;
        rp[u] = p4[i]; rg[u] = g4[i]; rm[u] = m4[i]; rv[u] = v4[i];
      }
#pragma unroll
      for (int u = 0; u < ADAM_UNROLL; u++) {
        const uint32_t i = tid + u * ADAM_THREADS;
        adam_four(rp[u], rg[u], rm[u], rv[u], k);
        p4[i] = rp[u]; m4[i] = rm[u]; v4[i] = rv[u];
      }
    } else {
      // the last chunk of a segment (vector body + scalar tail) or a misaligned segment (all scalar)
      const uint32_t nvec = s.vec ? (len >> 2) : 0u;
      for (uint32_t i = tid; i < nvec; i += ADAM_THREADS) {
        v4f rp = ((gv4f*)p)[i], rm = ((gv4f*)m)[i], rv = ((gv4f*)v)[i];
        const v4f rg = ((const gv4f*)g)[i];
        adam_four(rp, rg, rm, rv, k);
        ((gv4f*)p)[i] = rp; ((gv4f*)m)[i] = rm; ((gv4f*)v)[i] = rv;
      }
      for (uint32_t i = (nvec << 2) + tid; i < len; i += ADAM_THREADS) {
        float rp = p[i], rm = m[i], rv = v[i];
        adam_one(rp, g[i], rm, rv, k);
        p[i] = rp; m[i] = rm; v[i] = rv;
      }
    }
  }
}

constexpr int DENSIFY_THREADS = 256;

__global__ void __launch_bounds__(DENSIFY_THREADS)
densify_stats_kernel(const int P, const float* __restrict__ grad_xyz, const int* __restrict__ radii,
                     const DensifyRangeDev* __restrict__ ranges, const int num_ranges) {
  const int i = blockIdx.x * DENSIFY_THREADS + threadIdx.x;
  if (i >= P) return;
  const int r = radii[i];
  if (r <= 0) return;                       // the visibility filter: radii > 0
  // the last range that starts at or before i (sorted, disjoint; empty ranges are not in the table)
  int lo = 0, hi = num_ranges - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ranges[mid].start <= i) lo = mid; else hi = mid - 1;
  }
  const DensifyRangeDev R = ranges[lo];
  if (i < R.start || i >= R.end) return;    // a Gaussian of the frame that no listed model owns
  const int j = i - R.start;
  const float gx = grad_xyz[3 * (size_t)i], gy = grad_xyz[3 * (size_t)i + 1], gz = grad_xyz[3 * (size_t)i + 2];
  gfloat* const accum = (gfloat*)R.accum + 2 * (size_t)j;
  gfloat* const denom = (gfloat*)R.denom + j;
  gfloat* const max_radii = (gfloat*)R.max_radii + j;
  accum[0] += sqrtf(gx * gx + gy * gy);
  accum[1] += fabsf(gz);
  *denom += 1.0f;
  *max_radii = fmaxf(*max_radii, (float)r);
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h).  Both entries return without a host wait: their tables go through the
// pinned staging ring of abi_util.h. ----
extern "C" {

size_t grpg_adam_workspace_bytes(int num_segments) {
  if (num_segments <= 0) return 0;
  return sizeof(AdamSegmentDev) * (size_t)num_segments;
}

int grpg_adam_step(const grpg_adam_segment* segments, int num_segments, grpg_alloc_fn table_alloc,
                   void* table_user, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (num_segments < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: negative segment count");
  if (num_segments == 0) return GRPG_OK;
  if (!segments) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: NULL segment table");
  if (!table_alloc) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: NULL table allocator");
  int live = 0;
  unsigned long long chunks = 0;
  for (int i = 0; i < num_segments; i++) {
    const grpg_adam_segment& g = segments[i];
    if (g.n < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: segment with negative n");
    if (g.n == 0) continue;
    if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: segment with a NULL array and n > 0");
    if (((uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq) & 3)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: arrays must be 4-byte aligned");
    if (!std::isfinite(g.bc2_sqrt) || !(g.bc2_sqrt > 0.f))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: bc2_sqrt must be finite and positive");
    if (!std::isfinite(g.step_size) || !std::isfinite(g.beta2) || !std::isfinite(g.one_minus_beta1) ||
        !std::isfinite(g.one_minus_beta2) || !std::isfinite(g.eps))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: non-finite coefficient");
    live++;
    chunks += ((unsigned long long)g.n + ADAM_CHUNK_ELEMS - 1) / ADAM_CHUNK_ELEMS;
  }
  if (live == 0) return GRPG_OK;              // nothing but empty tensors: no launch
  if (chunks > 0xFFFFFFFFull) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: more than 2^32 chunks of 4096 elements");
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t bytes = sizeof(AdamSegmentDev) * (size_t)live;
  OptimStagingSlot* stg = optim_staging_acquire(bytes);
  if (!stg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  AdamSegmentDev* host = (AdamSegmentDev*)stg->host;
  uint32_t first = 0;
  int k = 0;
  for (int i = 0; i < num_segments; i++) {
    const grpg_adam_segment& g = segments[i];
    if (g.n == 0) continue;
    AdamSegmentDev& d = host[k++];
    d.param = g.param; d.grad = g.grad; d.exp_avg = g.exp_avg; d.exp_avg_sq = g.exp_avg_sq;
    d.n = (unsigned long long)g.n;
    d.step_size = g.step_size; d.bc2_sqrt = g.bc2_sqrt; d.beta2 = g.beta2;
    d.one_minus_beta1 = g.one_minus_beta1; d.one_minus_beta2 = g.one_minus_beta2; d.eps = g.eps;
    d.first_chunk = first;
    d.vec = (((uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq) & 15) == 0;
    first += (uint32_t)((d.n + ADAM_CHUNK_ELEMS - 1) / ADAM_CHUNK_ELEMS);
  }
  char* dev = table_alloc(grpg_adam_workspace_bytes(num_segments), table_user);
  if (!dev) return fail(GRPG_ERR_ALLOC, "adam_step: the table allocator returned NULL");
  if ((uintptr_t)dev & 7) return fail(GRPG_ERR_INVALID_ARGUMENT, "adam_step: the table must be 8-byte aligned");
  HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(stg->ev, stream));
  const uint32_t grid = first < (uint32_t)GRPG_ADAM_MAX_WGS ? first : (uint32_t)GRPG_ADAM_MAX_WGS;
  hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(ADAM_THREADS), 0, stream, (const AdamSegmentDev*)dev, live,
                     first);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_densify_stats(int P, const float* grad_xyz, const int* radii, const grpg_range* ranges, int num_ranges,
                       float* const* accum, float* const* denom, float* const* max_radii,
                       grpg_alloc_fn table_alloc, void* table_user, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (P < 0 || num_ranges < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: negative count");
  if (P == 0 || num_ranges == 0) return GRPG_OK;
  if (!grad_xyz || !radii) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: NULL grad_xyz / radii");
  if (!ranges || !accum || !denom || !max_radii)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: NULL range table");
  if (!table_alloc) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: NULL table allocator");
  int live = 0, prev_end = 0;
  for (int i = 0; i < num_ranges; i++) {
    const grpg_range& r = ranges[i];
    if (r.start < prev_end || r.end < r.start || r.end > P)
      return fail(GRPG_ERR_INVALID_ARGUMENT,
                  "densify_stats: ranges must be half-open [start, end), ascending, disjoint and within [0, P)");
    prev_end = r.end;
    if (r.end == r.start) continue;
    if (!accum[i] || !denom[i] || !max_radii[i])
      return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: non-empty range with a NULL array");
    live++;
  }
  if (live == 0) return GRPG_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t bytes = sizeof(DensifyRangeDev) * (size_t)live;
  OptimStagingSlot* stg = optim_staging_acquire(bytes);
  if (!stg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  DensifyRangeDev* host = (DensifyRangeDev*)stg->host;
  int k = 0;
  for (int i = 0; i < num_ranges; i++) {
    if (ranges[i].end == ranges[i].start) continue;
    host[k++] = DensifyRangeDev{accum[i], denom[i], max_radii[i], ranges[i].start, ranges[i].end};
  }
  char* dev = table_alloc(sizeof(DensifyRangeDev) * (size_t)num_ranges, table_user);
  if (!dev) return fail(GRPG_ERR_ALLOC, "densify_stats: the table allocator returned NULL");
  if ((uintptr_t)dev & 7) return fail(GRPG_ERR_INVALID_ARGUMENT, "densify_stats: the table must be 8-byte aligned");
  HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(stg->ev, stream));
  const int grid = (P + DENSIFY_THREADS - 1) / DENSIFY_THREADS;
  hipLaunchKernelGGL(densify_stats_kernel, dim3(grid), dim3(DENSIFY_THREADS), 0, stream, P, grad_xyz, radii,
                     (const DensifyRangeDev*)dev, live);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
