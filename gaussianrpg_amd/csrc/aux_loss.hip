// Fused auxiliary training losses for gfx950: the lidar-depth, sky and object-alpha terms of the
// reference's train.py:121-127,145-158,164-176, in one forward and one backward launch chain with no
// host synchronisation.  All planes are float32 [H,W] (a leading 1 is the same memory); masks are uint8
// (bool) planes of the same H x W.
//
// Terms (a term is evaluated only when its lambda > 0 and its planes are given; otherwise it is 0, not
// part of the total, and gets no gradient):
//   lidar  sel = (lidar > 0) & mask (no mask: all true), N = |sel|,
//          e = |depth / (acc + 1e-10) - lidar| over sel, in float32 in this operand order with no FMA
//          contraction (bit-identical to PyTorch's float32 expression), k = floor(0.95 * (double)N) on the
//          device (Python's int(0.95 * N)), term = mean of the k smallest e.
//          Zero-term rule (the reference's guard torch.nonzero(depth_mask).any() is true only when some
//          selected pixel has a nonzero coordinate): N == 0, or N == 1 with the one selected pixel at flat
//          index 0, give 0 with a zero gradient.  N == 1 elsewhere gives k == 0: the mean of an empty set,
//          NaN, with a zero gradient (as the reference).
//   sky    a = clamp(acc, 1e-6, 1 - 1e-6); term = sky_scale * mean over H*W of
//          where(sky, -log(1 - a), -log(a)).
//   obj    a = clamp(acc_obj, 1e-6, 1 - 1e-6); term = mean over H*W of
//          where(obj_bound, -(a log a + (1 - a) log(1 - a)), -log(1 - a)).
//   total  lambda_depth_lidar * lidar + lambda_sky * sky + lambda_reg * obj  (terms that are on).
// The clamp passes NaN through (NaN propagates) and its gradient is zero outside [lo, hi] (inclusive
// bounds, as clamp backward; zero for NaN).
//
// Selection: e is stored as a uint32 key plane (the bits of |x|, 0xFFFFFFFF for "not selected"; as
// unsigned integers the bits of non-negative floats order like the floats, NaN above +inf, as
// torch.topk(largest=False) orders them).  The k-th smallest key t is found by a radix select over the
// 31 significant bits in digits of 11, 11 and 9 bits: the forward builds the first digit's histogram
// (LDS histogram per workgroup, integer atomics into the global bins), a one-workgroup pick launch finds
// the bin that holds rank k - 1 and carries the prefix and the remaining rank on the device, and each
// further digit costs one histogram and one pick launch.  Ties at t: c_lt keys lie below t, c_eq equal
// it; each tied element gets weight (k - c_lt) / c_eq.  The value is the same for any choice among ties;
// the gradient is a valid subgradient that does not depend on order (torch.topk keeps an unspecified
// subset of the tied elements).
//
// Launches (lidar on): memset of the bins, aux_forward_kernel, pick 0, hist 1, pick 1, hist 2, pick 2,
// aux_lidar_sum_kernel, aux_reduce_kernel; with the lidar term off only aux_forward_kernel and
// aux_reduce_kernel.  Backward: aux_backward_kernel.  Float sums are per-workgroup float64 partials in
// fixed slots, reduced by one workgroup in a fixed order: identical calls give identical bits.  Integer
// atomics only (exact, order-free); no float atomics.
//
// Stats vector (float32 [9]): [0] total, [1] lidar term, [2] sky term (after sky_scale), [3] obj term,
// [4] N, [5] k, [6] t (the k-th smallest error; 0 when k == 0), [7] c_lt, [8] c_eq.  The counts are
// exact in float32 only below 2^24; the workspace header (AuxState) keeps them as exact integers.
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int AX_THREADS = 256;
constexpr int AX_MAX_WG = 1024;              // forward / sum grid (grid-strided over 4-pixel quads)
constexpr int AX_BINS = 2048;                // 11-bit digits
constexpr unsigned AX_NOSEL = 0xFFFFFFFFu;
constexpr int AX_SHIFT[3] = {20, 9, 0};      // digit p covers key bits [AX_SHIFT[p], AX_SHIFT[p] + AX_BITS[p])
constexpr int AX_BITS[3] = {11, 11, 9};

// Workspace header (offset 0).  Exact integers; the picks write it, the backward reads it.
struct AuxState {
  unsigned long long N, k, c_lt, c_eq;
  unsigned int tkey;      // bits of t (valid when k > 0)
  unsigned int prefix;    // digits resolved so far
  unsigned int rank;      // remaining 0-based rank among the keys that match prefix
  unsigned int sel0;      // flat index 0 is selected
  unsigned int zero;      // zero-term rule: N == 0, or N == 1 at flat index 0
  unsigned int valid;     // k > 0: a threshold exists
};
constexpr size_t AX_HDR = 256;
static_assert(sizeof(AuxState) <= AX_HDR, "AuxState");

struct AuxArgs {
  int n;                  // H * W
  int nwg;                // forward / sum grid size
  int vec;                // all planes 16-byte aligned (masks 4-byte): vector loads
  int lidar_on, sky_on, obj_on;
  float sky_scale, lam_lidar, lam_sky, lam_reg;
  const float* depth;
  const float* acc;
  const float* lidar;
  const unsigned char* mask;
  const unsigned char* sky;
  const float* acc_obj;
  const unsigned char* bound;
};

struct AuxWs {
  AuxState* st;
  unsigned int* hist;     // [3][AX_BINS]
  double* part;           // [3][nwg]: sky, obj, lidar sum below t
  unsigned int* keys;     // [n]
};

constexpr float AX_LO = 1e-6f;
constexpr float AX_HI = (float)(1.0 - 1e-6);   // Python's 1. - 1e-6, rounded once to float32
constexpr float AX_EPS = 1e-10f;

__device__ __forceinline__ float clamp_nan(const float x) {   // torch.clamp: NaN passes through
  return x < AX_LO ? AX_LO : (x > AX_HI ? AX_HI : x);
}
__device__ __forceinline__ bool in_clamp(const float x) { return x >= AX_LO && x <= AX_HI; }

__device__ __forceinline__ float sky_val(const float acc, const unsigned char s) {
  const float a = clamp_nan(acc);
  return s ? -logf(1.0f - a) : -logf(a);
}
__device__ __forceinline__ float obj_val(const float acc_obj, const unsigned char b) {
  const float a = clamp_nan(acc_obj);
  return b ? -(a * logf(a) + (1.0f - a) * logf(1.0f - a)) : -logf(1.0f - a);
}

struct Quad {
  float d[4], a[4], l[4], o[4];
  unsigned char m[4], s[4], b[4];
};

// loads the 4 pixels of quad q (count valid pixels) of the planes that are in use
__device__ __forceinline__ int load_quad(const AuxArgs& A, const int q, Quad& v) {
  const int i0 = q * 4;
  const int cnt = min(4, A.n - i0);
  const bool need_acc = A.lidar_on || A.sky_on;
  if (A.vec && cnt == 4) {
    if (A.lidar_on) {
      const float4 d = reinterpret_cast<const float4*>(A.depth)[q];
      const float4 l = reinterpret_cast<const float4*>(A.lidar)[q];
      v.d[0] = d.x; v.d[1] = d.y; v.d[2] = d.z; v.d[3] = d.w;
      v.l[0] = l.x; v.l[1] = l.y; v.l[2] = l.z; v.l[3] = l.w;
      const unsigned m = A.mask ? reinterpret_cast<const unsigned*>(A.mask)[q] : 0x01010101u;
#pragma unroll
      for (int j = 0; j < 4; j++) v.m[j] = (m >> (8 * j)) & 0xFF;
    }
    if (need_acc) {
      const float4 a = reinterpret_cast<const float4*>(A.acc)[q];
      v.a[0] = a.x; v.a[1] = a.y; v.a[2] = a.z; v.a[3] = a.w;
    }
    if (A.sky_on) {
      const unsigned s = reinterpret_cast<const unsigned*>(A.sky)[q];
#pragma unroll
      for (int j = 0; j < 4; j++) v.s[j] = (s >> (8 * j)) & 0xFF;
    }
    if (A.obj_on) {
      const float4 o = reinterpret_cast<const float4*>(A.acc_obj)[q];
      v.o[0] = o.x; v.o[1] = o.y; v.o[2] = o.z; v.o[3] = o.w;
      const unsigned b = reinterpret_cast<const unsigned*>(A.bound)[q];
#pragma unroll
      for (int j = 0; j < 4; j++) v.b[j] = (b >> (8 * j)) & 0xFF;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt) {
      const int i = i0 + j;
      if (A.lidar_on) {
        v.d[j] = A.depth[i];
        v.l[j] = A.lidar[i];
        v.m[j] = A.mask ? A.mask[i] : 1;
      }
      if (need_acc) v.a[j] = A.acc[i];
      if (A.sky_on) v.s[j] = A.sky[i];
      if (A.obj_on) {
        v.o[j] = A.acc_obj[i];
        v.b[j] = A.bound[i];
      }
    }
  }
  return cnt;
}

// the reference's float32 expression: expected = depth / (acc + 1e-10); e = |expected - lidar|
__device__ __forceinline__ float lidar_diff(const float depth, const float acc, const float lidar) {
  const float expected = depth / (acc + AX_EPS);
  return expected - lidar;
}

// the keys of quad q (cnt valid): one 16-byte access when the planes allow it
__device__ __forceinline__ void load_keys(const AuxArgs& A, const unsigned int* keys, const int q,
                                          const int cnt, unsigned (&key)[4]) {
  if (A.vec && cnt == 4) {
    const uint4 k4 = reinterpret_cast<const uint4*>(keys)[q];
    key[0] = k4.x; key[1] = k4.y; key[2] = k4.z; key[3] = k4.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt) key[j] = keys[q * 4 + j];
  }
}
__device__ __forceinline__ void store_keys(const AuxArgs& A, unsigned int* __restrict__ keys, const int q,
                                           const int cnt, const unsigned (&key)[4]) {
  if (A.vec && cnt == 4) {
    reinterpret_cast<uint4*>(keys)[q] = make_uint4(key[0], key[1], key[2], key[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt) keys[q * 4 + j] = key[j];
  }
}

// Forward elementwise pass: key plane, first-digit histogram, sky / obj partial sums.
__global__ void __launch_bounds__(AX_THREADS)
aux_forward_kernel(const AuxArgs A, const AuxWs ws) {
  __shared__ unsigned int h[AX_BINS];
  __shared__ double s_red[AX_THREADS / 64];
  if (A.lidar_on) {
    for (int i = threadIdx.x; i < AX_BINS; i += AX_THREADS) h[i] = 0;
    __syncthreads();
  }
  const int nq = (A.n + 3) / 4;
  double sum_sky = 0.0, sum_obj = 0.0;
  for (int q = blockIdx.x * AX_THREADS + threadIdx.x; q < nq; q += A.nwg * AX_THREADS) {
    Quad v;
    const int cnt = load_quad(A, q, v);
    if (A.lidar_on) {
      unsigned key[4] = {AX_NOSEL, AX_NOSEL, AX_NOSEL, AX_NOSEL};
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < cnt) {
        if (v.l[j] > 0.0f && v.m[j]) {
          key[j] = __float_as_uint(fabsf(lidar_diff(v.d[j], v.a[j], v.l[j])));
          atomicAdd(&h[key[j] >> AX_SHIFT[0]], 1u);
        }
      }
      if (q == 0) ws.st->sel0 = key[0] != AX_NOSEL ? 1u : 0u;
      store_keys(A, ws.keys, q, cnt, key);
    }
    if (A.sky_on)
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < cnt) sum_sky += (double)sky_val(v.a[j], v.s[j]);
    if (A.obj_on)
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < cnt) sum_obj += (double)obj_val(v.o[j], v.b[j]);
  }
  if (A.lidar_on) {
    __syncthreads();
    for (int i = threadIdx.x; i < AX_BINS; i += AX_THREADS)
      if (h[i]) atomicAdd(&ws.hist[i], h[i]);
  }
  const double ts = block_sum(sum_sky, s_red);
  const double to = block_sum(sum_obj, s_red);
  if (threadIdx.x == 0) {
    ws.part[blockIdx.x] = ts;
    ws.part[A.nwg + blockIdx.x] = to;
  }
}

// Histogram of digit p (1 or 2) over the keys whose higher digits equal the resolved prefix.
__global__ void __launch_bounds__(AX_THREADS)
aux_hist_kernel(const AuxArgs A, const AuxWs ws, const int p) {
  __shared__ unsigned int h[AX_BINS];
  if (!ws.st->valid) return;
  const unsigned prefix = ws.st->prefix;
  const int hi_shift = AX_SHIFT[p - 1], shift = AX_SHIFT[p];
  const unsigned dmask = (1u << AX_BITS[p]) - 1u;
  for (int i = threadIdx.x; i < AX_BINS; i += AX_THREADS) h[i] = 0;
  __syncthreads();
  const int nq = (A.n + 3) / 4;
  for (int q = blockIdx.x * AX_THREADS + threadIdx.x; q < nq; q += gridDim.x * AX_THREADS) {
    const int cnt = min(4, A.n - q * 4);
    unsigned key[4];
    load_keys(A, ws.keys, q, cnt, key);
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt)   // AX_NOSEL has bit 31 set and never matches a 31-bit prefix
      if ((key[j] >> hi_shift) == prefix) atomicAdd(&h[(key[j] >> shift) & dmask], 1u);
  }
  __syncthreads();
  unsigned int* gh = ws.hist + (size_t)p * AX_BINS;
  for (int i = threadIdx.x; i <= (int)dmask; i += AX_THREADS)
    if (h[i]) atomicAdd(&gh[i], h[i]);
}

// One workgroup: find the bin of digit p that holds the remaining rank; carry prefix and rank.
// Pass 0 also forms N, k and the zero-term flag; the last pass writes t, c_lt and c_eq.
// Every lane reads the state it needs before the scan; the lane that finds the bin hands it over
// through LDS, and thread 0 alone writes the state back after a barrier.
__global__ void __launch_bounds__(AX_THREADS)
aux_pick_kernel(const AuxWs ws, const int p) {
  __shared__ unsigned long long s_scan[AX_THREADS];
  __shared__ unsigned long long s_rem;
  __shared__ int s_bin;
  AuxState* st = ws.st;
  const unsigned int* hist = ws.hist + (size_t)p * AX_BINS;
  const int nbins = 1 << AX_BITS[p];
  const int per = nbins / AX_THREADS;
  const int tid = threadIdx.x;
  // state of the previous passes (this launch writes it only at the very end)
  const unsigned valid_in = p > 0 ? st->valid : 1u;
  if (!valid_in) return;
  const unsigned prefix_in = p > 0 ? st->prefix : 0u;
  const unsigned long long rank_in = p > 0 ? (unsigned long long)st->rank : 0ull;
  const unsigned long long k_in = p > 0 ? st->k : 0ull;
  const unsigned sel0 = p == 0 ? st->sel0 : 0u;
  unsigned long long s = 0;
  for (int j = 0; j < per; j++) s += hist[tid * per + j];
  s_scan[tid] = s;
  __syncthreads();
  for (int d = 1; d < AX_THREADS; d <<= 1) {   // inclusive scan
    const unsigned long long add = tid >= d ? s_scan[tid - d] : 0ull;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  unsigned long long rank = rank_in, k = k_in;
  if (p == 0) {
    const unsigned long long N = s_scan[AX_THREADS - 1];
    k = (unsigned long long)floor(0.95 * (double)N);
    if (tid == 0) {
      st->N = N;
      st->k = k;
      st->zero = (N == 0ull || (N == 1ull && sel0)) ? 1u : 0u;
      st->valid = k > 0ull ? 1u : 0u;
      st->prefix = 0;
      st->rank = 0;
      st->tkey = 0;
      st->c_lt = 0;
      st->c_eq = 0;
    }
    if (k == 0ull) return;   // uniform: no threshold
    rank = k - 1ull;
  }
  const unsigned long long excl = s_scan[tid] - s;
  if (rank >= excl && rank < s_scan[tid]) {   // exactly one lane
    unsigned long long r = rank - excl;
    int b = tid * per;
    while (r >= hist[b]) r -= hist[b++];
    s_bin = b;
    s_rem = r;
  }
  __syncthreads();
  if (tid == 0) {
    const int b = s_bin;
    const unsigned long long r = s_rem;
    const unsigned prefix = (prefix_in << AX_BITS[p]) | (unsigned)b;
    st->prefix = prefix;
    st->rank = (unsigned)r;
    if (p == 2) {
      st->tkey = prefix;
      st->c_eq = hist[b];
      st->c_lt = k - 1ull - r;
    }
  }
}

// Per workgroup: float64 sum of the selected errors below t (fixed slots).
__global__ void __launch_bounds__(AX_THREADS)
aux_lidar_sum_kernel(const AuxArgs A, const AuxWs ws) {
  __shared__ double s_red[AX_THREADS / 64];
  const bool valid = ws.st->valid != 0u;
  const unsigned tkey = ws.st->tkey;
  double sum = 0.0;
  const int nq = valid ? (A.n + 3) / 4 : 0;
  for (int q = blockIdx.x * AX_THREADS + threadIdx.x; q < nq; q += A.nwg * AX_THREADS) {
    const int cnt = min(4, A.n - q * 4);
    unsigned key[4];
    load_keys(A, ws.keys, q, cnt, key);
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt)
      if (key[j] < tkey) sum += (double)__uint_as_float(key[j]);
  }
  const double t = block_sum(sum, s_red);
  if (threadIdx.x == 0) ws.part[2 * (size_t)A.nwg + blockIdx.x] = t;
}

// One workgroup: the slots in a fixed order -> stats[9]
__global__ void __launch_bounds__(REDUCE_THREADS)
aux_reduce_kernel(const AuxArgs A, const AuxWs ws, float* __restrict__ stats) {
  __shared__ double s_red[REDUCE_THREADS];
  const double sky = A.sky_on ? slot_sum(ws.part, A.nwg, s_red) : 0.0;
  const double obj = A.obj_on ? slot_sum(ws.part + A.nwg, A.nwg, s_red) : 0.0;
  const double lt = A.lidar_on ? slot_sum(ws.part + 2 * (size_t)A.nwg, A.nwg, s_red) : 0.0;
  if (threadIdx.x != 0) return;
  float total = 0.0f, f_lidar = 0.0f, f_sky = 0.0f, f_obj = 0.0f;
  float N = 0.f, k = 0.f, t = 0.f, c_lt = 0.f, c_eq = 0.f;
  if (A.lidar_on) {
    const AuxState* st = ws.st;
    if (st->zero) {
      f_lidar = 0.0f;
    } else if (!st->valid) {
      f_lidar = __builtin_nanf("");          // k == 0: mean of an empty set
    } else {
      const float tv = __uint_as_float(st->tkey);
      f_lidar = (float)((lt + (double)(st->k - st->c_lt) * (double)tv) / (double)st->k);
      t = tv;
    }
    N = (float)st->N; k = (float)st->k; c_lt = (float)st->c_lt; c_eq = (float)st->c_eq;
    total = total + A.lam_lidar * f_lidar;
  }
  if (A.sky_on) {
    f_sky = (float)(sky / (double)A.n) * A.sky_scale;   // sky_loss *= lambda_sky_scale[cam]
    total = total + A.lam_sky * f_sky;
  }
  if (A.obj_on) {
    f_obj = (float)(obj / (double)A.n);
    total = total + A.lam_reg * f_obj;
  }
  stats[0] = total; stats[1] = f_lidar; stats[2] = f_sky; stats[3] = f_obj;
  stats[4] = N; stats[5] = k; stats[6] = t; stats[7] = c_lt; stats[8] = c_eq;
}

// Backward, elementwise: every element of the non-NULL gradient planes.
__global__ void __launch_bounds__(AX_THREADS)
aux_backward_kernel(const AuxArgs A, const AuxState* __restrict__ st, const float* __restrict__ gstats,
                    float* __restrict__ g_depth, float* __restrict__ g_acc, float* __restrict__ g_obj) {
  // upstream scales, formed on the device
  const float g0 = gstats[0];
  float w_lt = 0.f, w_eq = 0.f;
  unsigned tkey = 0u;
  const bool lidar = A.lidar_on && st->valid && !st->zero;
  if (lidar) {
    const float up = A.lam_lidar * g0 + gstats[1];
    w_lt = up / (float)st->k;   // mean backward: one float32 division, as PyTorch's
    // the tied elements' share (k - c_lt) / c_eq, formed in float64; all ties kept: the plain weight
    w_eq = st->k - st->c_lt == st->c_eq
               ? w_lt
               : (float)((double)up * ((double)(st->k - st->c_lt) / (double)st->c_eq) / (double)st->k);
    tkey = st->tkey;
  }
  const float s_sky = A.sky_on ? (A.lam_sky * g0 + gstats[2]) * A.sky_scale / (float)A.n : 0.f;
  const float s_obj = A.obj_on ? (A.lam_reg * g0 + gstats[3]) / (float)A.n : 0.f;
  const int nq = (A.n + 3) / 4;
  for (int q = blockIdx.x * AX_THREADS + threadIdx.x; q < nq; q += gridDim.x * AX_THREADS) {
    Quad v;
    const int cnt = load_quad(A, q, v);
    float gd[4] = {0.f, 0.f, 0.f, 0.f}, ga[4] = {0.f, 0.f, 0.f, 0.f}, go[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < cnt) {
      if (lidar && v.l[j] > 0.0f && v.m[j]) {
        const float diff = lidar_diff(v.d[j], v.a[j], v.l[j]);
        const unsigned key = __float_as_uint(fabsf(diff));
        const float w = key < tkey ? w_lt : (key == tkey ? w_eq : 0.f);
        if (w != 0.f) {
          const float g = (float)((diff > 0.f) - (diff < 0.f)) * w;   // abs backward: sign(0) = 0
          const float b = v.a[j] + AX_EPS;
          gd[j] = g / b;                                              // div backward, PyTorch's order
          ga[j] = -g * ((v.d[j] / b) / b);
        }
      }
      if (A.sky_on && in_clamp(v.a[j])) {
        const float a = v.a[j];
        ga[j] += v.s[j] ? s_sky / (1.0f - a) : -s_sky / a;
      }
      if (A.obj_on && in_clamp(v.o[j])) {
        const float a = v.o[j];
        go[j] = v.b[j] ? s_obj * (logf(1.0f - a) - logf(a)) : s_obj / (1.0f - a);
      }
    }
    if (A.vec && cnt == 4) {
      if (g_depth) reinterpret_cast<float4*>(g_depth)[q] = make_float4(gd[0], gd[1], gd[2], gd[3]);
      if (g_acc) reinterpret_cast<float4*>(g_acc)[q] = make_float4(ga[0], ga[1], ga[2], ga[3]);
      if (g_obj) reinterpret_cast<float4*>(g_obj)[q] = make_float4(go[0], go[1], go[2], go[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < cnt) {
        if (g_depth) g_depth[q * 4 + j] = gd[j];
        if (g_acc) g_acc[q * 4 + j] = ga[j];
        if (g_obj) g_obj[q * 4 + j] = go[j];
      }
    }
  }
}

int aux_grid(const int n) {
  const int nq = (n + 3) / 4;
  return max(1, min(AX_MAX_WG, (nq + AX_THREADS - 1) / AX_THREADS));
}

bool aligned(const void* p, const uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

// The entries' planes, H*W each, NULL when absent.
struct AuxPlanes {
  const float* depth;
  const float* acc;
  const float* lidar;
  const unsigned char* mask;
  const unsigned char* sky;
  const float* acc_obj;
  const unsigned char* bound;
};

AuxArgs make_args(const int H, const int W, const AuxPlanes& P, const float sky_scale,
                  const float lam_lidar, const float lam_sky, const float lam_reg) {
  AuxArgs A;
  A.n = H * W;
  A.nwg = aux_grid(A.n);
  A.lidar_on = lam_lidar > 0.f && P.lidar != nullptr;
  A.sky_on = lam_sky > 0.f && P.sky != nullptr;
  A.obj_on = lam_reg > 0.f && P.bound != nullptr;
  A.sky_scale = sky_scale;
  A.lam_lidar = lam_lidar; A.lam_sky = lam_sky; A.lam_reg = lam_reg;
  A.depth = A.lidar_on ? P.depth : nullptr;
  A.acc = (A.lidar_on || A.sky_on) ? P.acc : nullptr;
  A.lidar = A.lidar_on ? P.lidar : nullptr;
  A.mask = A.lidar_on ? P.mask : nullptr;
  A.sky = A.sky_on ? P.sky : nullptr;
  A.acc_obj = A.obj_on ? P.acc_obj : nullptr;
  A.bound = A.obj_on ? P.bound : nullptr;
  A.vec = aligned(A.depth, 16) && aligned(A.acc, 16) && aligned(A.lidar, 16) && aligned(A.acc_obj, 16) &&
          aligned(A.mask, 4) && aligned(A.sky, 4) && aligned(A.bound, 4);
  return A;
}

// Workspace: header, histograms, partial slots, key plane, each from a 256-byte boundary
struct AuxLayout {
  size_t hist, part, keys, total;
};
AuxLayout aux_layout(const int n) {
  AuxLayout L;
  size_t o = AX_HDR;
  auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
  L.hist = take(3 * AX_BINS * sizeof(unsigned int));
  L.part = take(3 * sizeof(double) * aux_grid(n));
  L.keys = take((size_t)n * sizeof(unsigned int));
  L.total = o;
  return L;
}

AuxWs make_ws(char* base, const int n) {
  const AuxLayout L = aux_layout(n);
  AuxWs w;
  w.st = (AuxState*)base;
  w.hist = (unsigned int*)(base + L.hist);
  w.part = (double*)(base + L.part);
  w.keys = (unsigned int*)(base + L.keys);
  return w;
}

int aux_check(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
              const unsigned char* sky_mask, const float* acc_obj, const unsigned char* obj_bound,
              float lambda_depth_lidar, float lambda_sky, float lambda_reg, const void* workspace) {
  if (int rc = loss_plane_check("aux_loss", height, width)) return rc;
  if (!workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: NULL workspace");
  if ((uintptr_t)workspace & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: workspace must be 16-byte aligned");
  if (lambda_depth_lidar > 0.f && lidar_depth && (!depth || !acc))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: the lidar term needs depth and acc");
  if (lambda_sky > 0.f && sky_mask && !acc) return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: the sky term needs acc");
  if (lambda_reg > 0.f && obj_bound && !acc_obj)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: the object term needs acc_obj");
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_aux_loss_workspace_bytes(int height, int width) {
  return loss_plane_check(nullptr, height, width) ? 0 : aux_layout(height * width).total;
}

int grpg_aux_loss_forward(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                          const unsigned char* mask, const unsigned char* sky_mask, const float* acc_obj,
                          const unsigned char* obj_bound, float sky_scale, float lambda_depth_lidar,
                          float lambda_sky, float lambda_reg, float* stats, void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = aux_check(height, width, depth, acc, lidar_depth, sky_mask, acc_obj, obj_bound, lambda_depth_lidar,
                         lambda_sky, lambda_reg, workspace))
    return rc;
  if (!stats) return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: NULL stats");
  hipStream_t st = (hipStream_t)hip_stream;
  const AuxPlanes planes{depth, acc, lidar_depth, mask, sky_mask, acc_obj, obj_bound};
  const AuxArgs A = make_args(height, width, planes, sky_scale, lambda_depth_lidar, lambda_sky, lambda_reg);
  const AuxWs ws = make_ws((char*)workspace, A.n);
  if (A.lidar_on) (void)hipMemsetAsync(ws.hist, 0, 3 * AX_BINS * sizeof(unsigned int), st);
  aux_forward_kernel<<<A.nwg, AX_THREADS, 0, st>>>(A, ws);
  if (A.lidar_on) {
    aux_pick_kernel<<<1, AX_THREADS, 0, st>>>(ws, 0);
    for (int p = 1; p < 3; p++) {
      aux_hist_kernel<<<A.nwg, AX_THREADS, 0, st>>>(A, ws, p);
      aux_pick_kernel<<<1, AX_THREADS, 0, st>>>(ws, p);
    }
    aux_lidar_sum_kernel<<<A.nwg, AX_THREADS, 0, st>>>(A, ws);
  }
  aux_reduce_kernel<<<1, REDUCE_THREADS, 0, st>>>(A, ws, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_aux_loss_backward(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                           const unsigned char* mask, const unsigned char* sky_mask, const float* acc_obj,
                           const unsigned char* obj_bound, float sky_scale, float lambda_depth_lidar,
                           float lambda_sky, float lambda_reg, const float* grad_stats, const void* workspace,
                           float* grad_depth, float* grad_acc, float* grad_acc_obj, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (int rc = aux_check(height, width, depth, acc, lidar_depth, sky_mask, acc_obj, obj_bound, lambda_depth_lidar,
                         lambda_sky, lambda_reg, workspace))
    return rc;
  if (!grad_stats) return fail(GRPG_ERR_INVALID_ARGUMENT, "aux_loss: NULL grad_stats");
  const AuxPlanes planes{depth, acc, lidar_depth, mask, sky_mask, acc_obj, obj_bound};
  AuxArgs A = make_args(height, width, planes, sky_scale, lambda_depth_lidar, lambda_sky, lambda_reg);
  A.vec = A.vec && aligned(grad_depth, 16) && aligned(grad_acc, 16) && aligned(grad_acc_obj, 16);
  const AuxWs ws = make_ws((char*)const_cast<void*>(workspace), A.n);
  aux_backward_kernel<<<A.nwg, AX_THREADS, 0, (hipStream_t)hip_stream>>>(A, ws.st, grad_stats, grad_depth, grad_acc,
                                                                          grad_acc_obj);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
