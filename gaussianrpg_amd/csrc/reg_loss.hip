// Fused per-Gaussian regularisers for gfx950: the scale-flatten term of the reference's train.py:190-194
// (gaussian_model.py:271-280) and the opacity-sparse term of train.py:196-204, in one forward and one backward pass
// with no host synchronisation, no torch.sort, no get_opacity concatenation and no boolean gather.
//
// Scale flatten.  scaling is float32 [N,3], row-major; one thread owns one Gaussian i (lanes run along the flat
// Gaussian index: the three loads of a wave cover one contiguous 768-byte run, every byte of it used).  float32:
//   v_k = exp(x_k)  (x_k itself when activated)
//   (a, b, c) = v sorted ascending by a stable three-element exchange (0,1) (1,2) (0,1), exchanging on strict >,
//               so equal values keep their index order as torch.sort(stable=True) does
//   s1 = min(max(a, 0), 30), s2 = min(max(b, 1e-5), 30), s3 = min(max(c, 1e-5), 30)
//   r = (s2 - s3)^2 / (s2 s3),   term = |s1| + |r|,   scale_flatten_loss = sum term / N   (NaN for N == 0)
// r is the reference's s2 / s3 + s3 / s2 - 2 without its cancellation: that form loses half an ulp of 2 (1.2e-7
// absolute) of a value that is small exactly where the regulariser has done its work, which float32 PyTorch shows as
// a relative error above 1e-6 for a single Gaussian; the quotient form is good to a few ulp of r itself.
// Opacity sparse.  Every model's raw opacity array (float32 [N_i]) is one segment of the flat index j in [0, P),
// P = sum N_i, in composed order; the segment table (pointers, first flat index, length) is read from device memory,
// each thread keeping the segment it last found.  Visible: radii[j] > 0.  float32:
//   o = 1 / (1 + exp(-x)), u = 1 / (1 + exp(x))   (u = 1 - o without the cancellation; activated: o = x, u = 1 - x)
//   inside = 1e-6 <= o <= 1 - 1e-6;  oc = inside ? o : clamp(o, 1e-6, 1 - 1e-6) (NaN stays NaN, as torch.clamp: the
//   term of a visible Gaussian with a NaN opacity is NaN, its gradient 0),  uc = inside ? u : 1 - oc
//   term = -(oc log oc + uc log uc) (the logs float32, the products and sums float64),
//   opacity_sparse_loss = sum over the visible / n_visible   (NaN for none)
// Accurate expf / logf, no FMA contraction: the backward recomputes the forward bit for bit.
//
// Forward launches: reg_forward_kernel (both terms in one grid-stride loop over max(N, P); per-workgroup partials:
// two float64 sums and the visible count in fixed slots), then reg_reduce_kernel (one workgroup, fixed order:
// identical calls give identical bits; no atomics).
// Stats (float32 [4]): [0] lambda_scale * [1] + lambda_opacity * [2] over the terms that are on, [1]
// scale_flatten_loss, [2] opacity_sparse_loss, [3] n_visible (0 for a term that is off).  The workspace header keeps
// n_visible as an exact int64 at byte offset 0.
//
// Backward launch: reg_backward_kernel, one pass over both terms.  g = the upstream gradient of the stats (device
// float32 [4]).
//   scale:   q = (lambda_scale g0 + g1) / N;  ds1 = q sign(s1) [0 <= a <= 30];  dr = q sign(r);
//            ds2 = dr (s2 - s3)(s2 + s3) / (s2^2 s3) [1e-5 <= b <= 30]     (= dr (1 / s3 - s3 / s2^2))
//            ds3 = dr (s3 - s2)(s3 + s2) / (s3^2 s2) [1e-5 <= c <= 30]     (= dr (1 / s2 - s2 / s3^2))
//            back through the permutation, and dx_k = dv_k v_k through the exp.  sign(0) = 0.
//   opacity: q = (lambda_opacity g0 + g2) / n_visible;  do = -q (log oc - log uc) [inside];  dx = do o u.
//            Invisible Gaussians, and every one when n_visible == 0, get exactly 0.
// Every element of every gradient array that is asked for is written.
//
// Bytes per Gaussian: scale 12 forward, 24 backward; opacity 8 forward (4 when invisible), 12 backward (8).
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_MAX_WG = 2048;              // 256 CUs x 8 resident workgroups of 4 waves; grid-strided beyond
constexpr size_t RG_HDR = 256;
constexpr float RG_SMAX = 30.0f, RG_SMIN = 1e-5f;
constexpr float RG_OMIN = 1e-6f, RG_OMAX = 1.0f - 1e-6f;

// Workspace header (offset 0): written by the reduce launch, read by the backward.
struct RgState {
  long long n_visible;
  double scale_sum, opacity_sum;
};
static_assert(sizeof(RgState) <= RG_HDR, "RgState");

struct RgWs {
  RgState* st;
  double* part;           // [2][RG_MAX_WG] scale, opacity
  unsigned int* cnt;      // [RG_MAX_WG] visible
};

// One row of the device segment table the entries upload into the workspace: slot 0 by the forward, slot 1 (with the
// gradient pointers) by the backward.
struct RegSegDev {
  const float* x;                          // the model's raw opacity [n]
  float* grad;                             // its gradient [n], or NULL (forward; not wanted)
  long long start;                         // first flat index of the composed order
  long long n;                             // > 0
};

struct RgArgs {
  long long N;            // Gaussians of the scale term (0 when off)
  long long P;            // Gaussians of the opacity term (0 when off)
  int nwg;
  int nseg;               // live segments
  int scale_on, opacity_on;
  int scale_activated, opacity_activated;
  float lam_scale, lam_opacity;
  const float* scaling;   // [N,3]
  const int* radii;       // [P]
  const RegSegDev* segs;
};

// The scale term of one Gaussian: the activated values, the permutation and the clamped sorted values
struct RgScale {
  float v[3], a, b, c, s1, s2, s3, r;
  int ia, ib, ic;         // a = v[ia], b = v[ib], c = v[ic]
  __device__ __forceinline__ void load(const RgArgs& A, const long long i) {
    const float* p = A.scaling + 3 * i;
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = A.scale_activated ? p[k] : expf(p[k]);
    a = v[0]; b = v[1]; c = v[2];
    ia = 0; ib = 1; ic = 2;
    auto exch = [](float& x, float& y, int& ix, int& iy) {
      if (x > y) {
        const float t = x; x = y; y = t;
        const int it = ix; ix = iy; iy = it;
      }
    };
    exch(a, b, ia, ib);
    exch(b, c, ib, ic);
    exch(a, b, ia, ib);
    s1 = fminf(fmaxf(a, 0.0f), RG_SMAX);
    s2 = fminf(fmaxf(b, RG_SMIN), RG_SMAX);
    s3 = fminf(fmaxf(c, RG_SMIN), RG_SMAX);
    r = ((s2 - s3) * (s2 - s3)) / (s2 * s3);
  }
};

// The opacity term of one visible Gaussian
struct RgOpacity {
  float o, u, oc, uc, lo, lu;
  bool inside;
  __device__ __forceinline__ void load(const RgArgs& A, const float x) {
    if (A.opacity_activated) {
      o = x;
      u = 1.0f - x;
    } else {
      o = 1.0f / (1.0f + expf(-x));
      u = 1.0f / (1.0f + expf(x));
    }
    inside = o >= RG_OMIN && o <= RG_OMAX;
    // torch.clamp: NaN passes through (fminf / fmaxf would return the bound and hide a NaN opacity of a visible
    // Gaussian, which the reference's mean shows)
    oc = inside ? o : (o < RG_OMIN ? RG_OMIN : (o > RG_OMAX ? RG_OMAX : o));
    uc = inside ? u : 1.0f - oc;
    lo = logf(oc);
    lu = logf(uc);
  }
};

// The segment that holds flat index j: the one last found, else a binary search over the first indices
__device__ __forceinline__ int rg_segment(const RgArgs& A, const long long j, int s) {
  const RegSegDev& h = A.segs[s];
  if (j >= h.start && j - h.start < h.n) return s;
  int lo = 0, hi = A.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.segs[mid].start <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(RG_THREADS) reg_forward_kernel(const RgArgs A, const RgWs ws) {
  __shared__ double s_red_d[RG_THREADS / 64];
  __shared__ unsigned int s_red_u[RG_THREADS / 64];
  double ss = 0.0, so = 0.0;
  unsigned int vis = 0;
  int seg = 0;
  const long long top = A.N > A.P ? A.N : A.P;
  for (long long i = blockIdx.x * RG_THREADS + threadIdx.x; i < top; i += (long long)A.nwg * RG_THREADS) {
    if (i < A.N) {
      RgScale s;
      s.load(A, i);
      ss += (double)fabsf(s.s1) + (double)fabsf(s.r);
    }
    if (i < A.P && A.radii[i] > 0) {
      seg = rg_segment(A, i, seg);
      RgOpacity q;
      q.load(A, A.segs[seg].x[i - A.segs[seg].start]);
      so -= (double)q.oc * (double)q.lo + (double)q.uc * (double)q.lu;   // the products and their sum unrounded
      vis++;
    }
  }
  const double ts = block_sum(ss, s_red_d);
  const double to = block_sum(so, s_red_d);
  const unsigned int tv = block_sum(vis, s_red_u);
  if (threadIdx.x == 0) {
    ws.part[blockIdx.x] = ts;
    ws.part[RG_MAX_WG + blockIdx.x] = to;
    ws.cnt[blockIdx.x] = tv;
  }
}

// One workgroup: the slots in a fixed order -> stats[4] and the workspace header
__global__ void __launch_bounds__(REDUCE_THREADS)
reg_reduce_kernel(const RgArgs A, const RgWs ws, float* __restrict__ stats) {
  __shared__ double s_d[REDUCE_THREADS];
  __shared__ unsigned long long s_u[REDUCE_THREADS];
  const double ss = slot_sum(ws.part, A.nwg, s_d);
  const double so = slot_sum(ws.part + RG_MAX_WG, A.nwg, s_d);
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < A.nwg; i += REDUCE_THREADS) c += ws.cnt[i];   // the counts widen while loading
  c = slot_sum(c, s_u);
  if (threadIdx.x != 0) return;
  ws.st->n_visible = (long long)c;
  ws.st->scale_sum = ss;
  ws.st->opacity_sum = so;
  // 0 / 0 = NaN: mean() of nothing
  const float ms = A.scale_on ? (float)(ss / (double)A.N) : 0.0f;
  const float mo = A.opacity_on ? (float)(so / (double)c) : 0.0f;
  float total = 0.0f;
  if (A.scale_on) total = A.lam_scale * ms;
  if (A.opacity_on) total = total + A.lam_opacity * mo;
  stats[0] = total;
  stats[1] = ms;
  stats[2] = mo;
  stats[3] = (float)c;
}

__global__ void __launch_bounds__(RG_THREADS)
reg_backward_kernel(const RgArgs A, const RgState* __restrict__ st, const float* __restrict__ grad_stats,
                    float* __restrict__ grad_scaling) {
  const long long nvis = st->n_visible;
  const float qs = (grad_scaling && A.N > 0) ? (A.lam_scale * grad_stats[0] + grad_stats[1]) / (float)A.N : 0.0f;
  const float qo = nvis > 0 ? (A.lam_opacity * grad_stats[0] + grad_stats[2]) / (float)nvis : 0.0f;
  int seg = 0;
  const long long top = A.N > A.P ? A.N : A.P;
  for (long long i = blockIdx.x * RG_THREADS + threadIdx.x; i < top; i += (long long)A.nwg * RG_THREADS) {
    if (grad_scaling && i < A.N) {
      RgScale s;
      s.load(A, i);
      const float sg1 = s.s1 > 0.0f ? 1.0f : (s.s1 < 0.0f ? -1.0f : 0.0f);
      const float sgr = s.r > 0.0f ? 1.0f : (s.r < 0.0f ? -1.0f : 0.0f);
      const float dr = qs * sgr;
      const float da = (s.a >= 0.0f && s.a <= RG_SMAX) ? qs * sg1 : 0.0f;
      const float dif = s.s2 - s.s3, sum = s.s2 + s.s3;
      const float db = (s.b >= RG_SMIN && s.b <= RG_SMAX) ? dr * ((dif * sum) / ((s.s2 * s.s2) * s.s3)) : 0.0f;
      const float dc = (s.c >= RG_SMIN && s.c <= RG_SMAX) ? dr * ((-dif * sum) / ((s.s3 * s.s3) * s.s2)) : 0.0f;
      float* g = grad_scaling + 3 * i;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float dv = s.ia == k ? da : (s.ib == k ? db : dc);
        g[k] = A.scale_activated ? dv : dv * s.v[k];
      }
    }
    if (i < A.P) {
      seg = rg_segment(A, i, seg);
      const RegSegDev& h = A.segs[seg];
      if (!h.grad) continue;
      float d = 0.0f;
      if (nvis > 0 && A.radii[i] > 0) {
        RgOpacity q;
        q.load(A, h.x[i - h.start]);
        if (q.inside) {
          d = -qo * (q.lo - q.lu);
          if (!A.opacity_activated) d = d * (q.o * q.u);
        }
      }
      h.grad[i - h.start] = d;
    }
  }
}

constexpr size_t RG_PART_OFF = RG_HDR;
constexpr size_t RG_CNT_OFF = RG_PART_OFF + 2 * sizeof(double) * RG_MAX_WG;
constexpr size_t RG_TABLE_OFF = RG_CNT_OFF + sizeof(unsigned int) * RG_MAX_WG;
static_assert(RG_TABLE_OFF % 256 == 0, "segment table offset");

RgWs make_ws(char* base) {
  RgWs w;
  w.st = (RgState*)base;
  w.part = (double*)(base + RG_PART_OFF);
  w.cnt = (unsigned int*)(base + RG_CNT_OFF);
  return w;
}

// What reg_loss_prepare makes of an entry's arguments
struct RegLossArgs {
  int scale_on, opacity_on;
  int scale_activated, opacity_activated;
  long long n_scaling;                     // N of scaling [N,3]
  long long n_opacity;                     // sum of the segments' n = the length of radii
  int num_live;                            // segments with n > 0 in the device table
  float lam_scale, lam_opacity;
  const float* scaling;
  const int* radii;
};

RgArgs make_args(const RegLossArgs& R, const RegSegDev* segs) {
  RgArgs A;
  A.scale_on = R.scale_on;
  A.opacity_on = R.opacity_on;
  A.N = R.scale_on ? R.n_scaling : 0;
  A.P = R.opacity_on && R.num_live > 0 ? R.n_opacity : 0;
  const long long top = A.N > A.P ? A.N : A.P;
  const long long wg = (top + RG_THREADS - 1) / RG_THREADS;
  A.nwg = (int)(wg < 1 ? 1 : (wg > RG_MAX_WG ? RG_MAX_WG : wg));
  A.nseg = R.num_live;
  A.scale_activated = R.scale_activated;
  A.opacity_activated = R.opacity_activated;
  A.lam_scale = R.lam_scale;
  A.lam_opacity = R.lam_opacity;
  A.scaling = R.scaling;
  A.radii = R.radii;
  A.segs = segs;
  return A;
}

// byte offset of table slot `which` (0 forward, 1 backward; 2: the end of the workspace)
size_t reg_loss_table_offset(const int which, const int num_segments) {
  return RG_TABLE_OFF + (size_t)which * align_up(sizeof(RegSegDev) * (size_t)(num_segments > 0 ? num_segments : 1), 256);
}

// Checks every argument, then uploads the live segments into table slot `which` of the workspace through the pinned
// ring and fills args / table.  Nothing is queued before the last check has passed.
int reg_loss_prepare(const float* scaling, long long n_scaling, int scale_activated, const grpg_reg_segment* segments,
                     int num_segments, int opacity_activated, const int* radii, long long n_radii, float lam_scale,
                     float lam_opacity, void* workspace, const bool backward, const bool want_scale, int which,
                     hipStream_t stream, RegLossArgs& R, const RegSegDev*& table) {
  R = RegLossArgs{};
  R.scale_on = lam_scale > 0.f && (!backward || want_scale);
  R.opacity_on = lam_opacity > 0.f;
  R.scale_activated = scale_activated ? 1 : 0;
  R.opacity_activated = opacity_activated ? 1 : 0;
  R.lam_scale = lam_scale;
  R.lam_opacity = lam_opacity;
  table = nullptr;
  if (!workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: NULL workspace");
  if ((uintptr_t)workspace & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: workspace must be 16-byte aligned");
  if (num_segments < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: negative segment count");
  if (R.scale_on) {
    if (n_scaling < 0 || n_scaling > 0x7FFFFFFFll / 3)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: n_scaling must be in [0, (2^31 - 1) / 3]");
    if (n_scaling > 0 && !scaling) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: NULL scaling with n_scaling > 0");
    if ((uintptr_t)scaling & 3) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: scaling must be 4-byte aligned");
    R.n_scaling = n_scaling;
    R.scaling = scaling;
  }
  if (!R.opacity_on) return GRPG_OK;
  if (num_segments > 0 && !segments) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: NULL segment table");
  long long total = 0;
  int live = 0;
  bool any_grad = false;
  for (int i = 0; i < num_segments; i++) {
    const grpg_reg_segment& g = segments[i];
    if (g.n < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: segment with negative n");
    if (g.n == 0) continue;
    if (!g.opacity) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: segment with a NULL opacity array and n > 0");
    if (((uintptr_t)g.opacity | (uintptr_t)g.grad_opacity) & 3)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: opacity arrays must be 4-byte aligned");
    total += g.n;
    if (total > 0x7FFFFFFFll) return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: more than 2^31 - 1 Gaussians");
    any_grad = any_grad || g.grad_opacity != nullptr;
    live++;
  }
  if (n_radii != total)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: the length of radii must be the sum of the segments' n");
  if (total > 0 && (!radii || ((uintptr_t)radii & 3)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: radii must be a 4-byte aligned pointer");
  R.n_opacity = total;
  R.radii = radii;
  if (backward && !any_grad) {          // no opacity gradient is wanted: the term costs nothing
    R.opacity_on = 0;
    return GRPG_OK;
  }
  if (live == 0) return GRPG_OK;
  const size_t bytes = sizeof(RegSegDev) * (size_t)live;
  OptimStagingSlot* stg = optim_staging_acquire(bytes);
  if (!stg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  RegSegDev* host = (RegSegDev*)stg->host;
  long long start = 0;
  int k = 0;
  for (int i = 0; i < num_segments; i++) {
    const grpg_reg_segment& g = segments[i];
    if (g.n == 0) continue;
    host[k++] = RegSegDev{g.opacity, backward ? g.grad_opacity : nullptr, start, g.n};
    start += g.n;
  }
  char* dev = (char*)workspace + reg_loss_table_offset(which, num_segments);
  HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(stg->ev, stream));
  R.num_live = live;
  table = (const RegSegDev*)dev;
  return GRPG_OK;
}
}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_reg_loss_workspace_bytes(int num_segments) {
  return num_segments < 0 ? 0 : reg_loss_table_offset(2, num_segments);
}

int grpg_reg_loss_forward(const float* scaling, long long n_scaling, int scale_activated,
                          const grpg_reg_segment* segments, int num_segments, int opacity_activated, const int* radii,
                          long long n_radii, float lambda_scale_flatten, float lambda_opacity_sparse, float* stats,
                          void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!stats || ((uintptr_t)stats & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: stats must be a 4-byte aligned pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  RegLossArgs R;
  const RegSegDev* table;
  if (int rc = reg_loss_prepare(scaling, n_scaling, scale_activated, segments, num_segments, opacity_activated, radii,
                                n_radii, lambda_scale_flatten, lambda_opacity_sparse, workspace, false, true, 0,
                                stream, R, table))
    return rc;
  const RgArgs A = make_args(R, table);
  const RgWs ws = make_ws((char*)workspace);
  reg_forward_kernel<<<A.nwg, RG_THREADS, 0, stream>>>(A, ws);
  reg_reduce_kernel<<<1, REDUCE_THREADS, 0, stream>>>(A, ws, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_reg_loss_backward(const float* scaling, long long n_scaling, int scale_activated,
                           const grpg_reg_segment* segments, int num_segments, int opacity_activated, const int* radii,
                           long long n_radii, float lambda_scale_flatten, float lambda_opacity_sparse,
                           const float* grad_stats, void* workspace, float* grad_scaling, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!grad_stats || (((uintptr_t)grad_stats | (uintptr_t)grad_scaling) & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "reg_loss: grad_stats and grad_scaling must be 4-byte aligned pointers");
  hipStream_t stream = (hipStream_t)hip_stream;
  RegLossArgs R;
  const RegSegDev* table;
  if (int rc = reg_loss_prepare(scaling, n_scaling, scale_activated, segments, num_segments, opacity_activated, radii,
                                n_radii, lambda_scale_flatten, lambda_opacity_sparse, workspace, true,
                                grad_scaling != nullptr, 1, stream, R, table))
    return rc;
  if (!R.scale_on && !R.opacity_on) return GRPG_OK;
  const RgArgs A = make_args(R, table);
  const RgWs ws = make_ws((char*)workspace);
  reg_backward_kernel<<<A.nwg, RG_THREADS, 0, stream>>>(A, ws.st, grad_stats, R.scale_on ? grad_scaling : nullptr);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
