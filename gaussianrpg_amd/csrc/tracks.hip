// Tracklets -> actor poses for gfx950: what StreetGaussianModel.parse_camera (lib/models/street_gaussian_model.py:263-283)
// asks of ActorPose.get_tracking_rotation / get_tracking_translation (lib/models/actor_pose.py:83-179) once per visible
// actor and frame, for every actor and every query stamp in ONE launch, and the way back to opt_trans / opt_rots in
// one memset and ONE launch.  No host wait, no atomics, identical bits from identical calls.  tests/tracks_truth.py
// restates the contract in torch (float32 as the reference runs it, float64 as the truth the tests measure against).
//
// Forward, one wave per (query t, actor a):
//  1. selection: the two entries of the actor's list with the smallest |stamps[frame] - t| in float64, ties to the
//     lower list position -- argsort(delta)[:2], NOT a bracketing search.  Lanes stride the list and keep their own two
//     best (delta, position) pairs; a six-step butterfly merges them under the total order (delta, position), after
//     which every lane holds the same two positions.
//  2. translation (x1 * w2 + x2 * w1) / d, x_i = input_trans_i (+ opt_trans_i), the weights float64 differences
//     rounded to float32 (what tensor * np.float64 does);
//  3. rotation: r_i = input_rots_i (x) (cos th_i, 0, 0, sin th_i), both normalised like F.normalize, then the slerp
//     defined in DESIGN.md section 21 at step float((t - t1) / (t2 - t1));
//  4. a validation frame (val_stamps[t, a] finite) evaluates 1-3 at the two camera stamps and combines the results by
//     the same lerp / slerp at t;
//  5. ego pose: q_e = matrix_to_quaternion(ego[:3, :3]) (general_utils.py:159-218), obj_rot = q_e (x) rot,
//     obj_trans = ego[:3, :3] trans + ego[:3, 3].
// After the selection all lanes compute the same pose; lane 0 stores it.
//
// Backward, one wave per actor: it walks the actor's T queries in order, recomputes the forward of each and adds the
// gradients of the at most four touched cells to the zero-filled dense arrays from lane 0.  Cells of different actors
// are disjoint (an entry list is argwhere(track_ids == id)), so no two waves touch one cell.
//
// Built with -ffp-contract=off: every step is the single float32 operation the restatement makes.
#include <climits>
#include <cmath>

#include "abi_util.h"
#include "common.h"

namespace grpg {

namespace {

constexpr int TRK_THREADS = 256;
constexpr int TRK_WAVES = TRK_THREADS / WAVE;
constexpr float TRK_NORM_EPS = 1e-12f;             // F.normalize
constexpr float TRK_SMALL_C = 1.0f - 1e-5f;        // |q0 . q1| above this: the series branch of the slerp

struct TrackDev {
  int F, M, A;
  const double* stamps;
  const float* in_trans;
  const float* in_rots;
  const int* entries;
  const int* offsets;
  const double* start;
  const double* end;
};

struct Quat { float w, x, y, z; };
struct Vec3 { float x, y, z; };

__device__ __forceinline__ Quat qmul(const Quat a, const Quat b) {   // quaternion_raw_multiply, term by term
  Quat o;
  o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  o.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  o.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  return o;
}
__device__ __forceinline__ Quat qconj(const Quat a) { return {a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ float qdot(const Quat a, const Quat b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Quat qscale(const Quat a, const float s) { return {a.w * s, a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ Quat qadd(const Quat a, const Quat b) { return {a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z}; }

// (delta, position) is a total order over an actor's entries: positions are unique
__device__ __forceinline__ bool closer(const double da, const int pa, const double db, const int pb) {
  return da < db || (da == db && pa < pb);
}

struct Entry {
  int cell;     // frame * M + column
  double ts;    // stamps[frame]
};

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// never index past the table, whatever the entry list holds
__device__ __forceinline__ Entry load_entry(const TrackDev& tb, const int off, const int p) {
  const int f = clampi(tb.entries[2 * (off + p)], 0, tb.F - 1);
  const int c = clampi(tb.entries[2 * (off + p) + 1], 0, tb.M - 1);
  return {f * tb.M + c, tb.stamps[f]};
}

// argsort(|stamps[frame] - tq|)[:2] over the list [off, off + L), L >= 2: wave-wide, every lane returns the same pair
__device__ void select2(const TrackDev& tb, const int off, const int L, const double tq, int& r0, int& r1) {
  double d0 = INFINITY, d1 = INFINITY;
  int p0 = INT_MAX, p1 = INT_MAX;
  for (int p = (int)lane_id(); p < L; p += WAVE) {
    const int f = clampi(tb.entries[2 * (off + p)], 0, tb.F - 1);
    const double d = fabs(tb.stamps[f] - tq);
    if (closer(d, p, d0, p0)) { d1 = d0; p1 = p0; d0 = d; p0 = p; }
    else if (closer(d, p, d1, p1)) { d1 = d; p1 = p; }
  }
#pragma unroll
  for (int m = WAVE / 2; m >= 1; m >>= 1) {
    const double e0 = __shfl_xor(d0, m, WAVE), e1 = __shfl_xor(d1, m, WAVE);
    const int q0 = __shfl_xor(p0, m, WAVE), q1 = __shfl_xor(p1, m, WAVE);
    if (closer(e0, q0, d0, p0)) {          // the other lane's best leads: second is my best or its second
      if (closer(e1, q1, d0, p0)) { d1 = e1; p1 = q1; } else { d1 = d0; p1 = p0; }
      d0 = e0; p0 = q0;
    } else if (closer(e0, q0, d1, p1)) {   // mine leads: second is my second or its best
      d1 = e0; p1 = q0;
    }
  }
  // a list of NaN deltas (a NaN query) selects nothing: stay inside the list
  r0 = p0 < L ? p0 : L - 1;
  r1 = p1 < L ? p1 : L - 1;
}

// ---- the slerp and its derivative ----
struct Slerp {
  Quat u0, u1;        // the normalised operands
  float n0, n1;       // max(|q|, eps)
  bool g0, g1;        // |q| > eps: the norm takes part in the gradient
  float sigma, a, b;  // out = a u0 + b sigma u1
  float dadc, dbdc;   // with c = min(|u0 . u1|, 1)
};

__device__ __forceinline__ Quat normalize_q(const Quat q, float& n, bool& g) {
  const float r = sqrtf(qdot(q, q));
  g = r > TRK_NORM_EPS;
  n = g ? r : TRK_NORM_EPS;
  return {q.w / n, q.x / n, q.y / n, q.z / n};
}

__device__ Quat slerp_fwd(const Quat q0, const Quat q1, const float s, Slerp& k) {
  k.u0 = normalize_q(q0, k.n0, k.g0);
  k.u1 = normalize_q(q1, k.n1, k.g1);
  const float dot = qdot(k.u0, k.u1);
  k.sigma = dot < 0.f ? -1.f : 1.f;
  const float cabs = fabsf(dot);
  const float c = cabs > 1.f ? 1.f : cabs;
  const float s1 = 1.f - s;
  if (c > TRK_SMALL_C) {
    // sin(k W) / sin W = k (1 + (1 - k^2) W^2 / 6 + O(W^4)) with W^2 = 2 (1 - c) + O((1 - c)^2)
    const float w3 = (1.f - c) / 3.f;
    k.a = s1 * (1.f + (1.f - s1 * s1) * w3);
    k.b = s * (1.f + (1.f - s * s) * w3);
    const bool open = !(cabs > 1.f);   // the clamp passes no gradient beyond 1
    k.dadc = open ? -(s1 * (1.f - s1 * s1)) / 3.f : 0.f;
    k.dbdc = open ? -(s * (1.f - s * s)) / 3.f : 0.f;
  } else {
    // In float64 from the float32 c, s: d(sin(k W) / sin W) / dW = (k cos(k W) sin W - sin(k W) cos W) / sin^2 W is
    // the difference of two terms of size k W that agree to O(W^3) -- at W = 0.1 float32 keeps three digits of it.
    // One wave per pose makes these few operations free (the launch is what the op costs).
    const double sd = (double)s, s1d = 1.0 - sd;
    const double om = acos((double)c), so = sin(om), co = cos(om);
    const double sa = sin(s1d * om), sb = sin(sd * om);
    k.a = (float)(sa / so);
    k.b = (float)(sb / so);
    const double dadw = (s1d * cos(s1d * om) * so - sa * co) / (so * so);
    const double dbdw = (sd * cos(sd * om) * so - sb * co) / (so * so);
    k.dadc = (float)(-dadw / so);
    k.dbdc = (float)(-dbdw / so);
  }
  return qadd(qscale(k.u0, k.a), qscale(k.u1, k.b * k.sigma));
}

__device__ __forceinline__ Quat normalize_bwd(const Quat u, const float n, const bool g, const Quat du) {
  if (!g) return qscale(du, 1.f / n);
  const float ud = qdot(u, du);
  return {(du.w - u.w * ud) / n, (du.x - u.x * ud) / n, (du.y - u.y * ud) / n, (du.z - u.z * ud) / n};
}

__device__ void slerp_bwd(const Slerp& k, const Quat dout, Quat& dq0, Quat& dq1) {
  const float da = qdot(dout, k.u0), db = k.sigma * qdot(dout, k.u1);
  const float ddot = (da * k.dadc + db * k.dbdc) * k.sigma;
  const Quat du0 = qadd(qscale(dout, k.a), qscale(k.u1, ddot));
  const Quat du1 = qadd(qscale(dout, k.b * k.sigma), qscale(k.u0, ddot));
  dq0 = normalize_bwd(k.u0, k.n0, k.g0, du0);
  dq1 = normalize_bwd(k.u1, k.n1, k.g1, du1);
}

// ---- steps 2 and 3 at one stamp ----
struct Weights { float w1, w2, d, step; };

__device__ __forceinline__ Weights weights_of(const double t1, const double t2, const double tq) {
  Weights w;
  w.w2 = (float)(t2 - tq);
  w.w1 = (float)(tq - t1);
  w.d = (float)(t2 - t1);
  w.step = (float)((tq - t1) / (t2 - t1));
  return w;
}

__device__ __forceinline__ Vec3 lerp3(const Vec3 x1, const Vec3 x2, const Weights w) {
  return {(x1.x * w.w2 + x2.x * w.w1) / w.d, (x1.y * w.w2 + x2.y * w.w1) / w.d, (x1.z * w.w2 + x2.z * w.w1) / w.d};
}

__device__ __forceinline__ Vec3 cell_trans(const TrackDev& tb, const float* __restrict__ opt_trans, const int cell) {
  Vec3 x = {tb.in_trans[3 * cell], tb.in_trans[3 * cell + 1], tb.in_trans[3 * cell + 2]};
  if (opt_trans) { x.x += opt_trans[3 * cell]; x.y += opt_trans[3 * cell + 1]; x.z += opt_trans[3 * cell + 2]; }
  return x;
}

struct Yaw { Quat in; float c, s; };

__device__ __forceinline__ Quat cell_rot(const TrackDev& tb, const float* __restrict__ opt_rots, const int cell, Yaw& y) {
  y.in = {tb.in_rots[4 * cell], tb.in_rots[4 * cell + 1], tb.in_rots[4 * cell + 2], tb.in_rots[4 * cell + 3]};
  if (!opt_rots) return y.in;
  const float th = opt_rots[cell];   // the full angle, as the reference writes it
  y.c = cosf(th);
  y.s = sinf(th);
  return qmul(y.in, {y.c, 0.f, 0.f, y.s});
}

struct Inner { Vec3 tr; Quat rot; };

__device__ Inner inner_fwd(const TrackDev& tb, const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                           const Entry e1, const Entry e2, const double tq) {
  const Weights w = weights_of(e1.ts, e2.ts, tq);
  Inner o;
  o.tr = lerp3(cell_trans(tb, opt_trans, e1.cell), cell_trans(tb, opt_trans, e2.cell), w);
  Yaw y1, y2;
  Slerp k;
  const Quat r1 = cell_rot(tb, opt_rots, e1.cell, y1), r2 = cell_rot(tb, opt_rots, e2.cell, y2);
  o.rot = slerp_fwd(r1, r2, w.step, k);
  return o;
}

// d(out) / d(theta) of out = in (x) (cos th, 0, 0, sin th), given dL/dout
__device__ __forceinline__ float yaw_bwd(const Yaw& y, const Quat dr) {
  const Quat dopt = qmul(qconj(y.in), dr);   // L(in)^T = L(conj(in))
  return dopt.z * y.c - dopt.w * y.s;
}

// the gradients of one evaluation's two cells; `writer` (one lane of the wave) adds them to the dense arrays
__device__ void inner_bwd(const TrackDev& tb, const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                          const Entry e1, const Entry e2, const double tq, const Vec3 dtr, const Quat drot,
                          float* __restrict__ g_trans, float* __restrict__ g_rots, const bool writer) {
  const Weights w = weights_of(e1.ts, e2.ts, tq);
  const Vec3 gd = {dtr.x / w.d, dtr.y / w.d, dtr.z / w.d};
  Yaw y1, y2;
  Slerp k;
  const Quat r1 = cell_rot(tb, opt_rots, e1.cell, y1), r2 = cell_rot(tb, opt_rots, e2.cell, y2);
  slerp_fwd(r1, r2, w.step, k);
  Quat dr1, dr2;
  slerp_bwd(k, drot, dr1, dr2);
  const float dth1 = yaw_bwd(y1, dr1), dth2 = yaw_bwd(y2, dr2);
  if (writer) {
    g_trans[3 * e1.cell] += gd.x * w.w2; g_trans[3 * e1.cell + 1] += gd.y * w.w2; g_trans[3 * e1.cell + 2] += gd.z * w.w2;
    g_trans[3 * e2.cell] += gd.x * w.w1; g_trans[3 * e2.cell + 1] += gd.y * w.w1; g_trans[3 * e2.cell + 2] += gd.z * w.w1;
    g_rots[e1.cell] += dth1;
    g_rots[e2.cell] += dth2;
  }
}

// ---- the ego pose ----
struct Ego { Quat q; float R[9]; Vec3 t; };

__device__ __forceinline__ float sqrt_positive(const float v) { return v > 0.f ? sqrtf(v) : 0.f; }

__device__ Ego load_ego(const float* __restrict__ e) {   // [4,4] row-major
  Ego o;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) o.R[3 * i + j] = e[4 * i + j];
  o.t = {e[3], e[7], e[11]};
  const float m00 = o.R[0], m01 = o.R[1], m02 = o.R[2], m10 = o.R[3], m11 = o.R[4], m12 = o.R[5], m20 = o.R[6],
              m21 = o.R[7], m22 = o.R[8];
  const float qa[4] = {sqrt_positive(1.0f + m00 + m11 + m22), sqrt_positive(1.0f + m00 - m11 - m22),
                       sqrt_positive(1.0f - m00 + m11 - m22), sqrt_positive(1.0f - m00 - m11 + m22)};
  int best = 0;   // argmax: the first maximum
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (qa[i] > qa[best]) best = i;
  Quat c;
  float q;
  if (best == 0) { q = qa[0]; c = {q * q, m21 - m12, m02 - m20, m10 - m01}; }
  else if (best == 1) { q = qa[1]; c = {m21 - m12, q * q, m10 + m01, m02 + m20}; }
  else if (best == 2) { q = qa[2]; c = {m02 - m20, m10 + m01, q * q, m12 + m21}; }
  else { q = qa[3]; c = {m10 - m01, m20 + m02, m21 + m12, q * q}; }
  const float den = 2.0f * (q > 0.1f ? q : 0.1f);
  o.q = {c.w / den, c.x / den, c.y / den, c.z / den};
  return o;
}

// ---- one (query, actor) ----
struct Query {
  bool active, val;
  int off, L;
  double t, c1, c2;
  int pos[4];
  Entry e[4];
};

// wave-uniform: the selections of one (query, actor)
__device__ Query make_query(const TrackDev& tb, const double* __restrict__ stamps_q, const double* __restrict__ val_stamps,
                            const int t, const int a) {
  Query q;
  q.off = tb.offsets[a];
  q.L = tb.offsets[a + 1] - q.off;
  q.t = stamps_q[t];
  q.active = q.L >= 2 && tb.start[a] <= q.t && q.t <= tb.end[a];
  q.val = false;
  q.pos[0] = q.pos[1] = q.pos[2] = q.pos[3] = -1;
  if (!q.active) return q;
  if (val_stamps) {
    q.c1 = val_stamps[2 * ((size_t)t * tb.A + a)];
    q.c2 = val_stamps[2 * ((size_t)t * tb.A + a) + 1];
    q.val = isfinite(q.c1) && isfinite(q.c2);
  }
  if (!q.val) {
    select2(tb, q.off, q.L, q.t, q.pos[0], q.pos[1]);
  } else {
    select2(tb, q.off, q.L, q.c1, q.pos[0], q.pos[1]);
    select2(tb, q.off, q.L, q.c2, q.pos[2], q.pos[3]);
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (q.pos[i] >= 0) q.e[i] = load_entry(tb, q.off, q.pos[i]);
  return q;
}

__global__ void __launch_bounds__(TRK_THREADS)
track_poses_fwd_kernel(const TrackDev tb, const int T, const double* __restrict__ stamps_q, const float* __restrict__ ego,
                       const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                       const double* __restrict__ val_stamps, float* __restrict__ rot, float* __restrict__ trans,
                       unsigned char* __restrict__ active, int* __restrict__ chosen) {
  const int pair = blockIdx.x * TRK_WAVES + (threadIdx.x >> 6);   // wave-uniform; T * A < 2^31 / TRK_WAVES
  if (pair >= T * tb.A) return;
  const int t = pair / tb.A, a = pair - t * tb.A;
  const Query q = make_query(tb, stamps_q, val_stamps, t, a);
  Quat orot = {1.f, 0.f, 0.f, 0.f};
  Vec3 otr = {0.f, 0.f, 0.f};
  if (q.active) {
    Inner r;
    if (!q.val) {
      r = inner_fwd(tb, opt_trans, opt_rots, q.e[0], q.e[1], q.t);
    } else {
      const Inner ra = inner_fwd(tb, opt_trans, opt_rots, q.e[0], q.e[1], q.c1);
      const Inner rb = inner_fwd(tb, opt_trans, opt_rots, q.e[2], q.e[3], q.c2);
      const Weights w = weights_of(q.c1, q.c2, q.t);
      Slerp k;
      r.tr = lerp3(ra.tr, rb.tr, w);
      r.rot = slerp_fwd(ra.rot, rb.rot, w.step, k);
    }
    const Ego e = load_ego(ego + (size_t)t * 16);
    orot = qmul(e.q, r.rot);
    otr.x = (e.R[0] * r.tr.x + e.R[1] * r.tr.y + e.R[2] * r.tr.z) + e.t.x;
    otr.y = (e.R[3] * r.tr.x + e.R[4] * r.tr.y + e.R[5] * r.tr.z) + e.t.y;
    otr.z = (e.R[6] * r.tr.x + e.R[7] * r.tr.y + e.R[8] * r.tr.z) + e.t.z;
  }
  if (lane_id() == 0) {
    float* o = rot + (size_t)pair * 4;
    o[0] = orot.w; o[1] = orot.x; o[2] = orot.y; o[3] = orot.z;
    float* p = trans + (size_t)pair * 3;
    p[0] = otr.x; p[1] = otr.y; p[2] = otr.z;
    active[pair] = q.active ? 1 : 0;
    int* c = chosen + (size_t)pair * 4;
    c[0] = q.pos[0]; c[1] = q.pos[1]; c[2] = q.pos[2]; c[3] = q.pos[3];
  }
}

__global__ void __launch_bounds__(TRK_THREADS)
track_poses_bwd_kernel(const TrackDev tb, const int T, const double* __restrict__ stamps_q, const float* __restrict__ ego,
                       const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                       const double* __restrict__ val_stamps, const float* __restrict__ g_rot,
                       const float* __restrict__ g_trans, float* __restrict__ g_opt_trans, float* __restrict__ g_opt_rots) {
  const int a = blockIdx.x * TRK_WAVES + (threadIdx.x >> 6);   // wave-uniform
  if (a >= tb.A) return;
  const bool writer = lane_id() == 0;
  for (int t = 0; t < T; t++) {   // in order: the same lane adds to a shared cell one query after the other
    const Query q = make_query(tb, stamps_q, val_stamps, t, a);
    if (!q.active) continue;
    const size_t pair = (size_t)t * tb.A + a;
    const Ego e = load_ego(ego + (size_t)t * 16);
    const Quat go = {g_rot[4 * pair], g_rot[4 * pair + 1], g_rot[4 * pair + 2], g_rot[4 * pair + 3]};
    const Vec3 gt = {g_trans[3 * pair], g_trans[3 * pair + 1], g_trans[3 * pair + 2]};
    const Quat drot = qmul(qconj(e.q), go);
    const Vec3 dtr = {e.R[0] * gt.x + e.R[3] * gt.y + e.R[6] * gt.z, e.R[1] * gt.x + e.R[4] * gt.y + e.R[7] * gt.z,
                      e.R[2] * gt.x + e.R[5] * gt.y + e.R[8] * gt.z};
    if (!q.val) {
      inner_bwd(tb, opt_trans, opt_rots, q.e[0], q.e[1], q.t, dtr, drot, g_opt_trans, g_opt_rots, writer);
    } else {
      const Inner ra = inner_fwd(tb, opt_trans, opt_rots, q.e[0], q.e[1], q.c1);
      const Inner rb = inner_fwd(tb, opt_trans, opt_rots, q.e[2], q.e[3], q.c2);
      const Weights w = weights_of(q.c1, q.c2, q.t);
      const Vec3 gd = {dtr.x / w.d, dtr.y / w.d, dtr.z / w.d};
      Slerp k;
      slerp_fwd(ra.rot, rb.rot, w.step, k);
      Quat da, db;
      slerp_bwd(k, drot, da, db);
      inner_bwd(tb, opt_trans, opt_rots, q.e[0], q.e[1], q.c1, {gd.x * w.w2, gd.y * w.w2, gd.z * w.w2}, da, g_opt_trans,
                g_opt_rots, writer);
      inner_bwd(tb, opt_trans, opt_rots, q.e[2], q.e[3], q.c2, {gd.x * w.w1, gd.y * w.w1, gd.z * w.w1}, db, g_opt_trans,
                g_opt_rots, writer);
    }
  }
}

constexpr int TRK_MAX_CELLS = 1 << 27;    // F * M: a cell's float index stays far below 2^31
constexpr int TRK_MAX_ACTORS = 1 << 16;
constexpr int TRK_MAX_PAIRS = 1 << 24;    // T * A

// Everything both entries check, before anything is enqueued.
int track_check(const std::string& pre, const grpg_track_table* tb, const int T, const double* timestamps,
                const float* ego, const float* opt_trans, const float* opt_rots, const double* val_stamps, TrackDev& d) {
  if (!tb) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL table");
  if (tb->F < 1 || tb->M < 1 || (long long)tb->F * tb->M > TRK_MAX_CELLS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "F and M must be positive with F * M <= 2^27");
  if (tb->A < 1 || tb->A > TRK_MAX_ACTORS) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "A must lie in [1, 65536]");
  if (T < 1 || (long long)T * tb->A > TRK_MAX_PAIRS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "T must be positive with T * A <= 2^24");
  if (!tb->stamps || !tb->input_trans || !tb->input_rots || !tb->entries || !tb->entry_offsets || !tb->start ||
      !tb->end || !tb->entry_offsets_host)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL pointer in the table");
  if (!timestamps || !ego) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL timestamps / ego");
  if ((opt_trans == nullptr) != (opt_rots == nullptr))
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "opt_trans and opt_rots come together or not at all");
  if (val_stamps && !opt_trans)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "val_stamps needs opt_trans / opt_rots (validation frames exist with opt_track only)");
  if (((uintptr_t)tb->stamps | (uintptr_t)tb->start | (uintptr_t)tb->end | (uintptr_t)timestamps | (uintptr_t)val_stamps) & 7)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "float64 arrays must be 8-byte aligned");
  if (((uintptr_t)tb->input_trans | (uintptr_t)tb->input_rots | (uintptr_t)tb->entries | (uintptr_t)tb->entry_offsets |
       (uintptr_t)ego | (uintptr_t)opt_trans | (uintptr_t)opt_rots) & 3)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "float32 / int32 arrays must be 4-byte aligned");
  const int* off = tb->entry_offsets_host;
  if (off[0] != 0 || off[tb->A] != tb->E || tb->E > TRK_MAX_CELLS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "entry_offsets must run from 0 to E <= F * M");
  for (int a = 0; a < tb->A; a++)
    if (off[a + 1] - off[a] < 2)
      return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "actor " + std::to_string(a) + " has fewer than two entries");
  d.F = tb->F; d.M = tb->M; d.A = tb->A;
  d.stamps = tb->stamps; d.in_trans = tb->input_trans; d.in_rots = tb->input_rots;
  d.entries = tb->entries; d.offsets = tb->entry_offsets; d.start = tb->start; d.end = tb->end;
  return GRPG_OK;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

int grpg_track_poses_forward(const grpg_track_table* table, int T, const double* timestamps, const float* ego,
                             const float* opt_trans, const float* opt_rots, const double* val_stamps, float* rot,
                             float* trans, unsigned char* active, int* chosen, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  const std::string pre = "track_poses_forward: ";
  TrackDev d;
  if (int rc = track_check(pre, table, T, timestamps, ego, opt_trans, opt_rots, val_stamps, d)) return rc;
  if (!rot || !trans || !active || !chosen) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL rot / trans / active / chosen");
  if (((uintptr_t)rot | (uintptr_t)trans | (uintptr_t)chosen) & 3)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "rot, trans and chosen must be 4-byte aligned");
  const int pairs = T * d.A;
  track_poses_fwd_kernel<<<(pairs + TRK_WAVES - 1) / TRK_WAVES, TRK_THREADS, 0, (hipStream_t)hip_stream>>>(
      d, T, timestamps, ego, opt_trans, opt_rots, val_stamps, rot, trans, active, chosen);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_track_poses_backward(const grpg_track_table* table, int T, const double* timestamps, const float* ego,
                              const float* opt_trans, const float* opt_rots, const double* val_stamps,
                              const float* g_rot, const float* g_trans, float* g_opt_trans, float* g_opt_rots,
                              void* hip_stream) {
  if (int rc = begin_call()) return rc;
  const std::string pre = "track_poses_backward: ";
  TrackDev d;
  if (int rc = track_check(pre, table, T, timestamps, ego, opt_trans, opt_rots, val_stamps, d)) return rc;
  if (!opt_trans) return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "there is nothing to differentiate without opt_trans / opt_rots");
  if (!g_rot || !g_trans || !g_opt_trans || !g_opt_rots)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "NULL g_rot / g_trans / g_opt_trans / g_opt_rots");
  if (((uintptr_t)g_rot | (uintptr_t)g_trans | (uintptr_t)g_opt_trans | (uintptr_t)g_opt_rots) & 3)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "gradient arrays must be 4-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t cells = (size_t)d.F * d.M;
  if (g_opt_rots != g_opt_trans + 3 * cells)
    return fail(GRPG_ERR_INVALID_ARGUMENT, pre + "g_opt_rots must follow g_opt_trans (one allocation of 4 F M floats: one memset)");
  // dense and fully written: a cell no active query touches stays zero
  HIP_TRY(hipMemsetAsync(g_opt_trans, 0, 4 * cells * sizeof(float), st));
  track_poses_bwd_kernel<<<(d.A + TRK_WAVES - 1) / TRK_WAVES, TRK_THREADS, 0, st>>>(
      d, T, timestamps, ego, opt_trans, opt_rots, val_stamps, g_rot, g_trans, g_opt_trans, g_opt_rots);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
