// Fused semantic cross-entropy loss for gfx950: the semantic term of the reference's train.py:129-143,
//   F.cross_entropy(semantic[None], gt_semantic, ignore_index=-1, reduction='mean')
// behind its torch.all(gt_semantic == -1) guard, and for semantic_mode 'probabilities' the normalise-and-log step
// of street_gaussian_renderer.py:248-256 in front of it, in one forward and one backward pass with no host
// synchronisation.
//
// Layout: sem is float32 [S,H,W], channel-major; target is [H,W], int64 or int32.  One thread owns one pixel i
// (lanes run along the flat pixel index), so the load of channel c, sem[c * H*W + i], is one contiguous 256-byte
// row per wave whatever the 4-byte alignment of sem and whatever H*W is.  For S <= 32 the pixel's S values are
// read once into registers (register arrays of 4, 8, 16 or 32 floats, indexed only by unrolled loops) and every
// further walk runs over the registers; for S > 32 each walk reads memory again.
//
// The value fed to the softmax, x_c:
//   mode 0 (logits)         x_c = sem_c
//   mode 1 (probabilities)  x_c = log(sem_c / (sum_c sem_c + 1e-8) + 1e-8), float32 in this operand order, the sum
//                           taken in channel order (a first walk)
// One walk with an online softmax (running max m, running sum s of exp(x - m)) yields lse = m + log(s); it also
// captures x at the target and the running argmax of the raw plane values (strict >: ties go to the lowest
// channel; the probabilities transform is monotone, so this is the argmax of x as well without its rounding ties).
// A channel at -inf adds 0 to s, also while m is still -inf: (-inf, -inf, 0) has lse 0, and a pixel whose channels
// are all -inf has lse -inf and the loss NaN, as F.cross_entropy.  The backward needs no such case: it takes lse from
// the forward, and exp(-inf - lse) is 0 for a finite lse.
// Accurate expf / logf, no FMA contraction: the backward recomputes x bit for bit.
//
// Pixels: valid when 0 <= target < S; ignored when target == -1; anything else is bad: counted, treated as
// ignored and never used as an index.
//
// Forward launches: semantic_ce_forward_kernel (lse plane, optional uint8 label plane, per-workgroup partials:
// a float64 loss sum and three integer counts in fixed slots), then semantic_ce_reduce_kernel (one workgroup, fixed
// order: identical calls give identical bits; no atomics anywhere).
// Stats (float32 [4]): [0] loss = sum / n_valid (0 when n_valid == 0: the reference's guard, on the device),
// [1] n_valid, [2] n_bad, [3] n_correct (valid pixels whose argmax is the target).  The workspace header keeps
// n_valid, n_bad, n_correct as exact int64 at byte offsets 0, 8, 16.
//
// Backward launch: semantic_ce_backward_kernel, one pass.  With q = g / n_valid (g a device float32 scalar,
// n_valid from the workspace header):
//   dx_c  = q * (exp(x_c - lse) - [c == target])
//   mode 0: d sem_c = dx_c
//   mode 1: with D = sum_c sem_c + 1e-8, p_c = sem_c / D:  dp_c = dx_c / (p_c + 1e-8),
//           d sem_c = (dp_c - sum_k dp_k p_k) / D
// Ignored and bad pixels, and every pixel when n_valid == 0, get exactly 0.  Every element of d sem is written.
//
// Bytes per pixel (S <= 32): forward 4 S + sizeof(target) + 4 (+ 1 with labels), backward 8 S + sizeof(target) + 4
// (4 S + sizeof(target) for an ignored pixel).
#include <type_traits>

#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int SCE_THREADS = 256;            // (SC_THREADS is the scan's, common.h)
constexpr int SC_MAX_WG = 2048;              // 256 CUs x 8 resident workgroups of 4 waves; grid-strided beyond
constexpr size_t SC_HDR = 256;
constexpr float SC_EPS = 1e-8f;

// Workspace header (offset 0): exact counts, written by the reduce launch, read by the backward.
struct ScState {
  long long n_valid, n_bad, n_correct;
  double loss_sum;
};
static_assert(sizeof(ScState) <= SC_HDR, "ScState");

struct ScArgs {
  int S;
  int n;                  // H * W
  int nwg;
  int t64;                // target is int64 (else int32)
  const float* sem;
  const void* target;
};

struct ScWs {
  ScState* st;
  double* part;           // [SC_MAX_WG] loss sums
  unsigned int* cnt;      // [3][SC_MAX_WG] n_valid, n_bad, n_correct
  float* lse;             // [n]
};

__device__ __forceinline__ long long load_target(const ScArgs& A, const int i) {
  return A.t64 ? reinterpret_cast<const long long*>(A.target)[i]
               : (long long)reinterpret_cast<const int*>(A.target)[i];
}

// The S values of one pixel: registers when CAP > 0 (S <= CAP), memory otherwise.
template <int CAP>
struct Pixel {
  float v[CAP > 0 ? CAP : 1];
  const float* p;         // &sem[i]
  size_t n;
  int S;

  __device__ __forceinline__ void load(const float* sem, const int i, const int n_, const int S_) {
    p = sem + i;
    n = (size_t)n_;
    S = S_;
    if constexpr (CAP > 0) {
#pragma unroll
      for (int c = 0; c < CAP; c++)
        if (c < S) v[c] = p[(size_t)c * n];
    }
  }
  // f(c, value of channel c), in channel order
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
    if constexpr (CAP > 0) {
#pragma unroll
      for (int c = 0; c < CAP; c++)
        if (c < S) f(c, v[c]);
    } else {
      for (int c = 0; c < S; c++) f(c, p[(size_t)c * n]);
    }
  }
  // the denominator of the probabilities transform: sum_c sem_c + 1e-8
  __device__ __forceinline__ float denom() const {
    float t = 0.0f;
    each([&](const int, const float r) { t = t + r; });
    return t + SC_EPS;
  }
};

template <int MODE>
__device__ __forceinline__ float sc_x(const float r, const float D) {
  if constexpr (MODE == 0) return r;
  else return logf(r / D + SC_EPS);
}

template <int CAP, int MODE>
__global__ void __launch_bounds__(SCE_THREADS)
semantic_ce_forward_kernel(const ScArgs A, const ScWs ws, unsigned char* __restrict__ labels) {
  __shared__ double s_red_d[SCE_THREADS / 64];
  __shared__ unsigned int s_red_u[SCE_THREADS / 64];
  double sum = 0.0;
  unsigned int n_valid = 0, n_bad = 0, n_correct = 0;
  // 64-bit loop counter: i + the grid stride may pass 2^31 for the largest planes
  for (long long ii = blockIdx.x * SCE_THREADS + threadIdx.x; ii < A.n; ii += A.nwg * SCE_THREADS) {
    const int i = (int)ii;
    const long long t = load_target(A, i);
    const bool valid = t >= 0 && t < (long long)A.S;
    const int tc = valid ? (int)t : -1;
    Pixel<CAP> px;
    px.load(A.sem, i, A.n, A.S);
    const float D = MODE == 1 ? px.denom() : 1.0f;
    float m = 0.0f, s = 1.0f, xt = 0.0f, best = 0.0f;
    int arg = 0;
    px.each([&](const int c, const float r) {
      const float x = sc_x<MODE>(r, D);
      if (c == 0) {
        m = x;
        best = r;
      } else {
        if (x > m) {
          s = s * expf(m - x) + 1.0f;
          m = x;
        } else {
          // a channel at -inf has probability 0, also while the running max is still -inf (-inf - -inf is NaN)
          s = s + (x == -INFINITY ? 0.0f : expf(x - m));
        }
        if (r > best) {
          best = r;
          arg = c;
        }
      }
      if (c == tc) xt = x;
    });
    const float lse = m + logf(s);
    ws.lse[i] = lse;
    if (labels) labels[i] = (unsigned char)arg;
    if (valid) {
      sum += (double)((m - xt) + logf(s));   // lse - x_target, rounded at the size of the loss, not of lse
      n_valid++;
      n_correct += arg == tc ? 1u : 0u;
    } else if (t != -1) {
      n_bad++;
    }
  }
  const double ts = block_sum(sum, s_red_d);
  const unsigned int tv = block_sum(n_valid, s_red_u);
  const unsigned int tb = block_sum(n_bad, s_red_u);
  const unsigned int tk = block_sum(n_correct, s_red_u);
  if (threadIdx.x == 0) {
    ws.part[blockIdx.x] = ts;
    ws.cnt[blockIdx.x] = tv;
    ws.cnt[SC_MAX_WG + blockIdx.x] = tb;
    ws.cnt[2 * SC_MAX_WG + blockIdx.x] = tk;
  }
}

// One workgroup: the slots in a fixed order -> stats[4] and the workspace header
__global__ void __launch_bounds__(REDUCE_THREADS)
semantic_ce_reduce_kernel(const int nwg, const ScWs ws, float* __restrict__ stats) {
  __shared__ double s_d[REDUCE_THREADS];
  __shared__ unsigned long long s_u[REDUCE_THREADS];
  double sum = 0.0;
  unsigned long long c[3] = {0ull, 0ull, 0ull};
  for (int i = threadIdx.x; i < nwg; i += REDUCE_THREADS) {   // the counts widen while loading
    sum += ws.part[i];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] += ws.cnt[k * SC_MAX_WG + i];
  }
  sum = slot_sum(sum, s_d);
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = slot_sum(c[k], s_u);
  if (threadIdx.x != 0) return;
  ws.st->n_valid = (long long)c[0];
  ws.st->n_bad = (long long)c[1];
  ws.st->n_correct = (long long)c[2];
  ws.st->loss_sum = sum;
  stats[0] = c[0] ? (float)(sum / (double)c[0]) : 0.0f;
  stats[1] = (float)c[0];
  stats[2] = (float)c[1];
  stats[3] = (float)c[2];
}

template <int CAP, int MODE>
__global__ void __launch_bounds__(SCE_THREADS)
semantic_ce_backward_kernel(const ScArgs A, const ScState* __restrict__ st, const float* __restrict__ lse_plane,
                            const float* __restrict__ grad_loss, float* __restrict__ grad_sem) {
  const long long nv = st->n_valid;
  const float q = nv > 0 ? grad_loss[0] / (float)nv : 0.0f;
  const size_t n = (size_t)A.n;
  for (long long ii = blockIdx.x * SCE_THREADS + threadIdx.x; ii < A.n; ii += A.nwg * SCE_THREADS) {
    const int i = (int)ii;
    const long long t = load_target(A, i);
    float* g = grad_sem + i;
    if (!(t >= 0 && t < (long long)A.S) || nv <= 0) {
      for (int c = 0; c < A.S; c++) g[(size_t)c * n] = 0.0f;
      continue;
    }
    const int tc = (int)t;
    const float lse = lse_plane[i];
    Pixel<CAP> px;
    px.load(A.sem, i, A.n, A.S);
    if constexpr (MODE == 0) {
      px.each([&](const int c, const float r) {
        g[(size_t)c * n] = q * (expf(r - lse) - (c == tc ? 1.0f : 0.0f));
      });
    } else {
      const float D = px.denom();
      // dp_c = dx_c / (p_c + 1e-8); its weighted sum over the channels
      auto dp_of = [&](const int c, const float r, float& p) {
        p = r / D;
        const float pe = p + SC_EPS;
        const float dx = q * (expf(logf(pe) - lse) - (c == tc ? 1.0f : 0.0f));
        return dx / pe;
      };
      float acc = 0.0f;
      if constexpr (CAP > 0) {
#pragma unroll
        for (int c = 0; c < CAP; c++)
          if (c < A.S) {
            float p;
            const float dp = dp_of(c, px.v[c], p);
            acc = acc + dp * p;
            px.v[c] = dp;
          }
#pragma unroll
        for (int c = 0; c < CAP; c++)
          if (c < A.S) g[(size_t)c * n] = (px.v[c] - acc) / D;
      } else {
        px.each([&](const int c, const float r) {
          float p;
          const float dp = dp_of(c, r, p);
          acc = acc + dp * p;
        });
        px.each([&](const int c, const float r) {
          float p;
          g[(size_t)c * n] = (dp_of(c, r, p) - acc) / D;
        });
      }
    }
  }
}

int sc_grid(const int n) { return max(1, min(SC_MAX_WG, (n + SCE_THREADS - 1) / SCE_THREADS)); }

constexpr size_t SC_PART_OFF = SC_HDR;
constexpr size_t SC_CNT_OFF = SC_PART_OFF + sizeof(double) * SC_MAX_WG;
constexpr size_t SC_LSE_OFF = SC_CNT_OFF + 3 * sizeof(unsigned int) * SC_MAX_WG;
static_assert(SC_LSE_OFF % 256 == 0, "lse plane offset");

ScWs make_ws(char* base) {
  ScWs w;
  w.st = (ScState*)base;
  w.part = (double*)(base + SC_PART_OFF);
  w.cnt = (unsigned int*)(base + SC_CNT_OFF);
  w.lse = (float*)(base + SC_LSE_OFF);
  return w;
}

ScArgs make_args(const int S, const int H, const int W, const float* sem, const void* target,
                 const int target_bytes) {
  ScArgs A;
  A.S = S;
  A.n = H * W;
  A.nwg = sc_grid(A.n);
  A.t64 = target_bytes == 8;
  A.sem = sem;
  A.target = target;
  return A;
}

// f(CAP, MODE) with both as compile-time constants.  CAP: the smallest register array that holds S values;
// 0 = walk memory
template <class F>
void sc_dispatch(const int S, const int mode, F&& f) {
  auto ladder = [&](auto m) {
    if (S <= 4) f(std::integral_constant<int, 4>{}, m);
    else if (S <= 8) f(std::integral_constant<int, 8>{}, m);
    else if (S <= 16) f(std::integral_constant<int, 16>{}, m);
    else if (S <= 32) f(std::integral_constant<int, 32>{}, m);
    else f(std::integral_constant<int, 0>{}, m);
  };
  if (mode == 0) ladder(std::integral_constant<int, 0>{});
  else ladder(std::integral_constant<int, 1>{});
}

int semantic_ce_check(int S, int height, int width, const float* sem, const void* target, int target_bytes,
                      int mode, const void* workspace) {
  if (S < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: S must be at least 1");
  if (int rc = loss_plane_check("semantic_ce", height, width)) return rc;
  if (!sem || !target) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: NULL sem / target");
  if (mode != 0 && mode != 1)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: mode must be 0 (logits) or 1 (probabilities)");
  if (target_bytes != 4 && target_bytes != 8)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: target_bytes must be 4 (int32) or 8 (int64)");
  if (((uintptr_t)sem & 3) || ((uintptr_t)target & (uintptr_t)(target_bytes - 1)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: sem must be 4-byte aligned, target aligned to its width");
  if (!workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: NULL workspace");
  if ((uintptr_t)workspace & 15)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: workspace must be 16-byte aligned");
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_semantic_ce_workspace_bytes(int height, int width) {
  if (loss_plane_check(nullptr, height, width)) return 0;
  return SC_LSE_OFF + align_up((size_t)height * width * sizeof(float), 256);
}

int grpg_semantic_ce_forward(int S, int height, int width, const float* sem, const void* target, int target_bytes,
                             int mode, float* stats, unsigned char* labels, void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = semantic_ce_check(S, height, width, sem, target, target_bytes, mode, workspace)) return rc;
  if (!stats) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: NULL stats");
  if (((uintptr_t)stats & 3)) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: stats must be 4-byte aligned");
  if (labels && S > 256)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: the uint8 label plane needs S <= 256");
  hipStream_t st = (hipStream_t)hip_stream;
  const ScArgs A = make_args(S, height, width, sem, target, target_bytes);
  const ScWs ws = make_ws((char*)workspace);
  sc_dispatch(S, mode, [&](auto cap, auto m) {
    semantic_ce_forward_kernel<decltype(cap)::value, decltype(m)::value>
        <<<A.nwg, SCE_THREADS, 0, st>>>(A, ws, labels);
  });
  semantic_ce_reduce_kernel<<<1, REDUCE_THREADS, 0, st>>>(A.nwg, ws, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_semantic_ce_backward(int S, int height, int width, const float* sem, const void* target, int target_bytes,
                              int mode, const float* grad_loss, const void* workspace, float* grad_sem,
                              void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = semantic_ce_check(S, height, width, sem, target, target_bytes, mode, workspace)) return rc;
  if (!grad_loss || !grad_sem) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: NULL grad_loss / grad_sem");
  if (((uintptr_t)grad_loss & 3) || ((uintptr_t)grad_sem & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantic_ce: grad_loss and grad_sem must be 4-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  const ScArgs A = make_args(S, height, width, sem, target, target_bytes);
  const ScWs ws = make_ws((char*)const_cast<void*>(workspace));
  sc_dispatch(S, mode, [&](auto cap, auto m) {
    semantic_ce_backward_kernel<decltype(cap)::value, decltype(m)::value>
        <<<A.nwg, SCE_THREADS, 0, st>>>(A, ws.st, ws.lse, grad_loss, grad_sem);
  });
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
