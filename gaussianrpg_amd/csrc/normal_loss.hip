// Fused mono-normal loss for gfx950: the normal term of the reference's train.py:206-225,
//   normal_l1_loss  = |normal_pred[normal_mask] - normal_gt[normal_mask]|.mean()
//   normal_cos_loss = (1 - sum(normal_pred[normal_mask] * normal_gt[normal_mask], -1)).mean()
// with normal_gt = mono_normal @ R.T (R = world_view_transform[:3,:3]) and, in front of it, the renderer's
// F.normalize(normals, dim=0) of street_gaussian_renderer.py:245-246, in one forward and one backward pass with no
// host synchronisation and no boolean gather.
//
// Layout: normals and mono are float32 [3,H,W], channel-major; the masks are uint8 [H,W].  One thread owns one pixel i
// (lanes run along the flat pixel index), so every channel load, p[c * H*W + i], is one contiguous 256-byte row per
// wave whatever the 4-byte alignment of the planes and whatever H*W is.  R is read on the device as 9 floats through
// its two element strides (a transposed or sliced view needs no copy).
//
// Selection of pixel i (row = i / W):
//   sky given:  (mask ? mask[i] : 1) && !sky[i] && row >= top_rows      (train.py:211-213)
//   no sky:     (mask ? mask[i] : 1)                                    (train.py:209, the squeezed mask)
// Per selected pixel, float32 in this operand order, no FMA contraction (the backward recomputes it bit for bit):
//   normalize:  r = sqrt(x0 x0 + x1 x1 + x2 x2), d = max(r, 1e-12), n_c = x_c / d;   else n_c = x_c
//   gt_c = m0 R[c][0] + m1 R[c][1] + m2 R[c][2]
//   l1 = |n0 - gt0| + |n1 - gt1| + |n2 - gt2|,   cos = 1 - (n0 gt0 + n1 gt1 + n2 gt2)
//
// Forward launches: normal_forward_kernel (per-workgroup partials: two float64 sums and a count in fixed slots),
// then normal_reduce_kernel (one workgroup, fixed order: identical calls give identical bits; no atomics).
// Stats (float32 [4]): [0] loss = [1] + [2] (added in float64, rounded once), [1] normal_l1_loss = l1 / (3 n),
// [2] normal_cos_loss = cos / n, [3] n.  n == 0 gives NaN in [0..2] (mean() of an empty gather).  The workspace
// header keeps n as an exact int64 at byte offset 0.
//
// Backward launch: normal_backward_kernel, one pass.  With a = (g0 + g1) / (3 n) and b = (g0 + g2) / n (g the
// upstream gradient of the stats, a device float32 [4]; n from the workspace header):
//   dn_c = a sign(n_c - gt_c) - b gt_c                      sign(0) = 0
//   normalize, r >= 1e-12:  dx_c = (dn_c - n_c (n . dn)) / r
//   normalize, r <  1e-12:  dx_c = dn_c / 1e-12             (clamp_min passes nothing to the norm)
// Unselected pixels, and every pixel when n == 0, get exactly 0.  Every element of d normals is written.
//
// Bytes per pixel: forward 24 + masks (1 each) at a selected pixel, the masks alone otherwise; backward 36 + masks
// at a selected pixel, 12 + masks otherwise.
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int NL_THREADS = 256;
constexpr int NL_MAX_WG = 2048;              // 256 CUs x 8 resident workgroups of 4 waves; grid-strided beyond
constexpr size_t NL_HDR = 256;
constexpr float NL_EPS = 1e-12f;

// Workspace header (offset 0): written by the reduce launch, read by the backward.
struct NlState {
  long long n;
  double l1_sum, cos_sum;
};
static_assert(sizeof(NlState) <= NL_HDR, "NlState");

struct NlWs {
  NlState* st;
  double* part;           // [2][NL_MAX_WG] l1, cos
  unsigned int* cnt;      // [NL_MAX_WG]
};

struct NlArgs {
  int n;                  // H * W
  int W;
  int nwg;
  int normalize;
  int top_rows;           // rows switched off (sky given only)
  int rs, cs;             // element strides of R's rows and columns
  const float* x;         // normals [3,H,W]
  const float* m;         // mono_normal [3,H,W]
  const float* R;
  const unsigned char* mask;
  const unsigned char* sky;
};

__device__ __forceinline__ bool nl_selected(const NlArgs& A, const int i) {
  if (A.mask && !A.mask[i]) return false;
  if (A.sky) {
    if (A.sky[i]) return false;
    if (i / A.W < A.top_rows) return false;
  }
  return true;
}

struct NlRot {
  float r[3][3];
  __device__ __forceinline__ void load(const NlArgs& A) {
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int k = 0; k < 3; k++) r[j][k] = A.R[(long long)j * A.rs + (long long)k * A.cs];
  }
};

// One selected pixel: the prediction n, the target gt, and the norm r of the raw values
struct NlPixel {
  float x[3], n[3], gt[3], r;
  __device__ __forceinline__ void load(const NlArgs& A, const NlRot& Rm, const int i) {
    const size_t np = (size_t)A.n;
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      x[c] = A.x[(size_t)c * np + i];
      m[c] = A.m[(size_t)c * np + i];
    }
    if (A.normalize) {
      r = sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
      const float d = fmaxf(r, NL_EPS);
#pragma unroll
      for (int c = 0; c < 3; c++) n[c] = x[c] / d;
    } else {
      r = 1.0f;
#pragma unroll
      for (int c = 0; c < 3; c++) n[c] = x[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) gt[c] = (m[0] * Rm.r[c][0] + m[1] * Rm.r[c][1]) + m[2] * Rm.r[c][2];
  }
};

__global__ void __launch_bounds__(NL_THREADS) normal_forward_kernel(const NlArgs A, const NlWs ws) {
  __shared__ double s_red_d[NL_THREADS / 64];
  __shared__ unsigned int s_red_u[NL_THREADS / 64];
  NlRot Rm;
  Rm.load(A);
  double l1 = 0.0, cs = 0.0;
  unsigned int cnt = 0;
  // 64-bit loop counter: i + the grid stride may pass 2^31 for the largest planes
  for (long long ii = blockIdx.x * NL_THREADS + threadIdx.x; ii < A.n; ii += A.nwg * NL_THREADS) {
    const int i = (int)ii;
    if (!nl_selected(A, i)) continue;
    NlPixel p;
    p.load(A, Rm, i);
    l1 += (double)((fabsf(p.n[0] - p.gt[0]) + fabsf(p.n[1] - p.gt[1])) + fabsf(p.n[2] - p.gt[2]));
    cs += (double)(1.0f - ((p.n[0] * p.gt[0] + p.n[1] * p.gt[1]) + p.n[2] * p.gt[2]));
    cnt++;
  }
  const double t1 = block_sum(l1, s_red_d);
  const double tc = block_sum(cs, s_red_d);
  const unsigned int tn = block_sum(cnt, s_red_u);
  if (threadIdx.x == 0) {
    ws.part[blockIdx.x] = t1;
    ws.part[NL_MAX_WG + blockIdx.x] = tc;
    ws.cnt[blockIdx.x] = tn;
  }
}

// One workgroup: the slots in a fixed order -> stats[4] and the workspace header
__global__ void __launch_bounds__(REDUCE_THREADS)
normal_reduce_kernel(const int nwg, const NlWs ws, float* __restrict__ stats) {
  __shared__ double s_d[REDUCE_THREADS];
  __shared__ unsigned long long s_u[REDUCE_THREADS];
  const double l1 = slot_sum(ws.part, nwg, s_d);
  const double cs = slot_sum(ws.part + NL_MAX_WG, nwg, s_d);
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < nwg; i += REDUCE_THREADS) c += ws.cnt[i];   // the counts widen while loading
  c = slot_sum(c, s_u);
  if (threadIdx.x != 0) return;
  ws.st->n = (long long)c;
  ws.st->l1_sum = l1;
  ws.st->cos_sum = cs;
  const double ml = l1 / (3.0 * (double)c), mc = cs / (double)c;   // 0 / 0 = NaN for an empty selection
  stats[0] = (float)(ml + mc);
  stats[1] = (float)ml;
  stats[2] = (float)mc;
  stats[3] = (float)c;
}

__global__ void __launch_bounds__(NL_THREADS)
normal_backward_kernel(const NlArgs A, const NlState* __restrict__ st, const float* __restrict__ grad_stats,
                       float* __restrict__ grad) {
  const long long nsel = st->n;
  float a = 0.0f, b = 0.0f;
  if (nsel > 0) {
    a = (grad_stats[0] + grad_stats[1]) / (3.0f * (float)nsel);
    b = (grad_stats[0] + grad_stats[2]) / (float)nsel;
  }
  NlRot Rm;
  Rm.load(A);
  const size_t np = (size_t)A.n;
  for (long long ii = blockIdx.x * NL_THREADS + threadIdx.x; ii < A.n; ii += A.nwg * NL_THREADS) {
    const int i = (int)ii;
    float* g = grad + i;
    if (nsel <= 0 || !nl_selected(A, i)) {
#pragma unroll
      for (int c = 0; c < 3; c++) g[(size_t)c * np] = 0.0f;
      continue;
    }
    NlPixel p;
    p.load(A, Rm, i);
    float dn[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = p.n[c] - p.gt[c];
      const float s = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      dn[c] = a * s - b * p.gt[c];
    }
    if (A.normalize) {
      if (p.r >= NL_EPS) {
        const float dot = (p.n[0] * dn[0] + p.n[1] * dn[1]) + p.n[2] * dn[2];
#pragma unroll
        for (int c = 0; c < 3; c++) dn[c] = (dn[c] - p.n[c] * dot) / p.r;
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++) dn[c] = dn[c] / NL_EPS;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) g[(size_t)c * np] = dn[c];
  }
}

constexpr size_t NL_PART_OFF = NL_HDR;
constexpr size_t NL_CNT_OFF = NL_PART_OFF + 2 * sizeof(double) * NL_MAX_WG;
constexpr size_t NL_END = NL_CNT_OFF + sizeof(unsigned int) * NL_MAX_WG;

NlWs make_ws(char* base) {
  NlWs w;
  w.st = (NlState*)base;
  w.part = (double*)(base + NL_PART_OFF);
  w.cnt = (unsigned int*)(base + NL_CNT_OFF);
  return w;
}

// The entries' planes.  normals / mono [3,H,W] float32; rot: the 3x3 rotation read through its row and column
// element strides; mask / sky uint8 [H,W] or NULL.
struct NormalPlanes {
  const float* normals;
  const float* mono;
  const float* rot;
  int rot_row_stride, rot_col_stride;
  const unsigned char* mask;
  const unsigned char* sky;
};

NlArgs make_args(const int H, const int W, const NormalPlanes& P, const int normalize, const int top_rows) {
  NlArgs A;
  A.n = H * W;
  A.W = W;
  A.nwg = max(1, min(NL_MAX_WG, (A.n + NL_THREADS - 1) / NL_THREADS));
  A.normalize = normalize;
  A.top_rows = top_rows;
  A.rs = P.rot_row_stride;
  A.cs = P.rot_col_stride;
  A.x = P.normals;
  A.m = P.mono;
  A.R = P.rot;
  A.mask = P.mask;
  A.sky = P.sky;
  return A;
}

int normal_loss_check(int height, int width, const float* normals, const float* mono_normal, const float* rotation,
                      int top_rows, const void* workspace) {
  if (int rc = loss_plane_check("normal_loss", height, width)) return rc;
  if (top_rows < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: top_rows must not be negative");
  if (!normals || !mono_normal || !rotation)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: NULL normals / mono_normal / rotation");
  if (((uintptr_t)normals | (uintptr_t)mono_normal | (uintptr_t)rotation) & 3)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: normals, mono_normal and rotation must be 4-byte aligned");
  if (!workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: NULL workspace");
  if ((uintptr_t)workspace & 15)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: workspace must be 16-byte aligned");
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_normal_loss_workspace_bytes(int height, int width) {
  return loss_plane_check(nullptr, height, width) ? 0 : NL_END;
}

int grpg_normal_loss_forward(int height, int width, const float* normals, const float* mono_normal,
                             const float* rotation, int rot_row_stride, int rot_col_stride, const unsigned char* mask,
                             const unsigned char* sky_mask, int normalize, int top_rows, float* stats,
                             void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = normal_loss_check(height, width, normals, mono_normal, rotation, top_rows, workspace)) return rc;
  if (!stats || ((uintptr_t)stats & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: stats must be a 4-byte aligned pointer");
  hipStream_t st = (hipStream_t)hip_stream;
  const NormalPlanes planes{normals, mono_normal, rotation, rot_row_stride, rot_col_stride, mask, sky_mask};
  const NlArgs A = make_args(height, width, planes, normalize ? 1 : 0, top_rows);
  const NlWs ws = make_ws((char*)workspace);
  normal_forward_kernel<<<A.nwg, NL_THREADS, 0, st>>>(A, ws);
  normal_reduce_kernel<<<1, REDUCE_THREADS, 0, st>>>(A.nwg, ws, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_normal_loss_backward(int height, int width, const float* normals, const float* mono_normal,
                              const float* rotation, int rot_row_stride, int rot_col_stride, const unsigned char* mask,
                              const unsigned char* sky_mask, int normalize, int top_rows, const float* grad_stats,
                              const void* workspace, float* grad_normals, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = normal_loss_check(height, width, normals, mono_normal, rotation, top_rows, workspace)) return rc;
  if (!grad_stats || !grad_normals || (((uintptr_t)grad_stats | (uintptr_t)grad_normals) & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "normal_loss: grad_stats and grad_normals must be 4-byte aligned pointers");
  const NormalPlanes planes{normals, mono_normal, rotation, rot_row_stride, rot_col_stride, mask, sky_mask};
  const NlArgs A = make_args(height, width, planes, normalize ? 1 : 0, top_rows);
  const NlWs ws = make_ws((char*)const_cast<void*>(workspace));
  normal_backward_kernel<<<A.nwg, NL_THREADS, 0, (hipStream_t)hip_stream>>>(A, ws.st, grad_stats, grad_normals);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
