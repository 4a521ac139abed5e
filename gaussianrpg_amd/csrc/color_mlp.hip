// Colour correction, use_mlp variant, for gfx950: camera pose -> the two 3x4 matrices of
// ColorCorrection.get_affine_trans (lib/models/color_correction.py:24-50, 110-116) in ONE launch, and the gradients of
// all sixteen parameter tensors in ONE launch.
//
// Forward, per camera t and network n (0 = affine_trans, 1 = affine_trans_sky):
//   a. c2w = ego_pose[t] @ extrinsic[t]             float32, c_ij = ((e_i0 x_0j + e_i1 x_1j) + e_i2 x_2j) + e_i3 x_3j,
//                                                   every product and every sum rounded (rows 0..2 only)
//   b. quaternion of the rotation block (general_utils.py:159-218):
//        q_abs = sqrt(max(0, .)) of  1 + m00 + m11 + m22 | 1 + m00 - m11 - m22 | 1 - m00 + m11 - m22 | 1 - m00 - m11 + m22
//        (each sum left to right); the candidate row of the FIRST largest q_abs, divided by 2 max(q_abs, 0.1);
//        no sign standardisation: the real part may be negative
//   c. axis-angle (general_utils.py:364-392):
//        n = sqrt((qx qx + qy qy) + qz qz), half = atan2f(n, qw), angle = 2 half,
//        div = 0.5 - angle angle / 48 where |angle| < 1e-6, sinf(half) / angle elsewhere,   r = q_xyz / div
//        x = [r, c2w[:3, 3]]
//      | rotation                     | largest q_abs      | divisor        | result                          |
//      | identity                     | r (q = 1,0,0,0)    | small angle    | exactly zero                    |
//      | angle < 1e-6                 | r                  | small angle    | q_xyz / (0.5 - angle^2 / 48)    |
//      | generic                      | r, i, j or k       | sin(half)/angle| axis * angle                    |
//      | ties (permutations, 180 deg) | first of the equal | sin(half)/angle| that row's signs                |
//      | real part < 0                | i, j or k          | sin(half)/angle| |r| = 2 atan2(n, qw) > pi       |
//   d. h1 = relu(W1 x + b1), h2 = relu(W2 h1 + b2), h3 = relu(W3 h2 + b3), A = view(W4 h3 + b4, 3, 4) + eye(4)[:3]
//      Lane j owns output unit j:  acc = bias[j];  for k ascending: acc = acc + weight[j][k] * h[k]   -- a rounded
//      multiply and a rounded add, never fused (the unit is compiled with -ffp-contract=off).  relu(v) = v > 0 ? v : 0.
//
// One workgroup of two waves per camera: wave n is network n, so the regulariser
//   reg[t] = (sum over i = 0..11 ascending of (|A_i - I_i| + |Asky_i - I_i|)) / 12      (regularization_loss)
// has both matrices in one workgroup and ONE fixed order (thread 0 adds the twelve terms from LDS, starting at +0).
//
// How the weights reach the lane.  The parameters are read in place, as nn.Linear holds them ([out,in] row-major, any
// 4-byte alignment).  A lane that walks its own 256-byte row makes every load instruction touch 64 cache lines; instead
// the wave copies a [64,64] (or [12,64]) matrix row by row -- lane l loads weight[i][l]: one 256-byte line per
// instruction -- into its own LDS region with a row stride of 65 floats, and lane j then reads s[j * 65 + k]: for a
// fixed k the 32 lanes of a half-wave hit banks (j + k) mod 32, all different, and the stores s[i * 65 + l] are
// conflict-free as well.  The 6-column first layer (1.5 KiB in all) is read from global memory directly.  h[k] reaches
// the lanes by v_readlane_b32 with a constant lane index (the loop is fully unrolled): the value arrives in a scalar
// register, which the multiply takes as an operand -- no LDS traffic and no barrier for the activations.  The kernel is
// launch-bound (fewer than 10 k multiply-adds per network); the staging is chosen for not depending on alignment.
//
// The forward stores what the backward needs: x [T,6] and the three post-ReLU vectors hidden [T,2,3,64] (1.5 KiB per
// camera) -- recomputing them would repeat the whole forward inside the backward's serial loop over t.
//
// Backward.  One workgroup of 256 threads per network, grid = 2; it copies the two 64 x 64 matrices into LDS once (the
// transposed products walk their columns for every camera), loops over t ascending and holds its slice of every
// weight gradient in registers (64 x 64 over 256 threads: entry e = thread + 256 i, i < 16, of each of W2 / W3; three of
// W4, at most two of W1; thread j < 64 the three hidden biases, thread o < 12 the last one).
//   d4[o]  = grad_affine[t][n][o] + (grad_reg[t] * sign((A[t][n][o] - I[o]))) / 12      (either part may be absent)
//   gW_l[j][k] = gW_l[j][k] + d_l[j] * h_{l-1}[k],   gb_l[j] = gb_l[j] + d_l[j]         t ascending, from +0
//   dh[k]  = sum over o ascending of weight[o][k] * d[o], from +0;    d_{l-1}[k] = h_{l-1}[k] > 0 ? dh[k] : 0
// The camera pose is not learnable (the reference has no gradient there): nothing flows back through x.  No atomics, no
// host wait, no memset: every output element is written once, identical calls give identical bits.
#include <math.h>
#include <stdint.h>

#include "abi_util.h"

namespace grpg {

constexpr int CM_IN = 6;
constexpr int CM_DIM = 64;
constexpr int CM_OUT = 12;
constexpr int CM_STRIDE = CM_DIM + 1;      // LDS row stride of a staged matrix
constexpr int CM_HIDDEN = 3 * CM_DIM;      // floats of hidden per (t, network)
constexpr int CM_MAX_T = 1 << 20;          // keeps every index inside 31 bits

struct ColorMlpParams {
  const float* w[2][4];
  const float* b[2][4];
};
struct ColorMlpGrads {
  float* w[2][4];
  float* b[2][4];
};

__device__ __forceinline__ float identity_entry(const int o) { return (o == 0 || o == 5 || o == 10) ? 1.f : 0.f; }

// lane k's value in every lane (k a constant after unrolling)
__device__ __forceinline__ float lane_value(const float v, const int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// x[6] of one camera: steps a-c of the header.  e, m: the camera's ego_pose and extrinsic, 16 floats each.
__device__ __forceinline__ void pose_vector(const float* __restrict__ e, const float* __restrict__ m, float (&x)[CM_IN]) {
  float c[3][4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float a = e[4 * i] * m[j];
      a = a + e[4 * i + 1] * m[4 + j];
      a = a + e[4 * i + 2] * m[8 + j];
      a = a + e[4 * i + 3] * m[12 + j];
      c[i][j] = a;
    }
  }
  const float m00 = c[0][0], m01 = c[0][1], m02 = c[0][2];
  const float m10 = c[1][0], m11 = c[1][1], m12 = c[1][2];
  const float m20 = c[2][0], m21 = c[2][1], m22 = c[2][2];
  const float s0 = 1.0f + m00 + m11 + m22, s1 = 1.0f + m00 - m11 - m22;
  const float s2 = 1.0f - m00 + m11 - m22, s3 = 1.0f - m00 - m11 + m22;
  const float a0 = s0 > 0.f ? sqrtf(s0) : 0.f, a1 = s1 > 0.f ? sqrtf(s1) : 0.f;
  const float a2 = s2 > 0.f ? sqrtf(s2) : 0.f, a3 = s3 > 0.f ? sqrtf(s3) : 0.f;
  // the first largest
  int best = 0;
  float ab = a0;
  if (a1 > ab) { best = 1; ab = a1; }
  if (a2 > ab) { best = 2; ab = a2; }
  if (a3 > ab) { best = 3; ab = a3; }
  float qw, qx, qy, qz;
  if (best == 0)      { qw = a0 * a0;  qx = m21 - m12; qy = m02 - m20; qz = m10 - m01; }
  else if (best == 1) { qw = m21 - m12; qx = a1 * a1;  qy = m10 + m01; qz = m02 + m20; }
  else if (best == 2) { qw = m02 - m20; qx = m10 + m01; qy = a2 * a2;  qz = m12 + m21; }
  else                { qw = m10 - m01; qx = m20 + m02; qy = m21 + m12; qz = a3 * a3; }
  const float den = 2.0f * fmaxf(ab, 0.1f);
  qw = qw / den; qx = qx / den; qy = qy / den; qz = qz / den;
  const float n = sqrtf((qx * qx + qy * qy) + qz * qz);
  const float half = atan2f(n, qw);
  const float angle = 2.0f * half;
  const float div = fabsf(angle) < 1e-6f ? 0.5f - (angle * angle) / 48.0f : sinf(half) / angle;
  x[0] = qx / div; x[1] = qy / div; x[2] = qz / div;
  x[3] = c[0][3]; x[4] = c[1][3]; x[5] = c[2][3];
}

// rows [ROWS,64] of a weight into the wave's LDS region, one 256-byte line per load
template <int ROWS>
__device__ __forceinline__ void stage_rows(const float* __restrict__ w, float* s, const int lane) {
#pragma unroll 8
  for (int i = 0; i < ROWS; i++) s[i * CM_STRIDE + lane] = w[i * CM_DIM + lane];
}

// bias + sum over k ascending of s[row][k] * h[k], h held one element per lane
__device__ __forceinline__ float dense64(const float* s, const int row, const float bias, const float h) {
  float acc = bias;
#pragma unroll
  for (int k = 0; k < CM_DIM; k++) acc = acc + s[row * CM_STRIDE + k] * lane_value(h, k);
  return acc;
}

__device__ __forceinline__ float relu(const float v) { return v > 0.f ? v : 0.f; }

// grid = T, block = 128: wave n of workgroup t is network n.  ext_stride: 16, or 0 for one shared extrinsic.
__global__ void __launch_bounds__(128)
color_mlp_forward_kernel(const ColorMlpParams p, const float* __restrict__ ego, const float* __restrict__ ext,
                         const int ext_stride, float* __restrict__ affine, float* __restrict__ xout,
                         float* __restrict__ reg, float* __restrict__ hidden) {
  __shared__ float s_w[2][CM_DIM * CM_STRIDE];
  __shared__ float s_abs[2][CM_OUT];
  const int t = blockIdx.x;
  const int n = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* s = s_w[n];

  float x[CM_IN];
  pose_vector(ego + (size_t)t * 16, ext + (size_t)t * ext_stride, x);
  if (xout && threadIdx.x < CM_IN) {
#pragma unroll
    for (int k = 0; k < CM_IN; k++)
      if (lane == k) xout[(size_t)t * CM_IN + k] = x[k];
  }

  float* hid = hidden ? hidden + ((size_t)t * 2 + n) * CM_HIDDEN : nullptr;
  // layer 1: [64,6], read in place
  float acc = p.b[n][0][lane];
  {
    const float* w = p.w[n][0] + lane * CM_IN;
#pragma unroll
    for (int k = 0; k < CM_IN; k++) acc = acc + w[k] * x[k];
  }
  float h = relu(acc);
  if (hid) hid[lane] = h;

  // layers 2 and 3: [64,64]
#pragma unroll 1
  for (int l = 1; l < 3; l++) {
    __syncthreads();                       // the region's last readers are done
    stage_rows<CM_DIM>(p.w[n][l], s, lane);
    __syncthreads();
    h = relu(dense64(s, lane, p.b[n][l][lane], h));
    if (hid) hid[l * CM_DIM + lane] = h;
  }

  // layer 4: [12,64]; lanes >= 12 repeat row 0 and store nothing
  __syncthreads();
  stage_rows<CM_OUT>(p.w[n][3], s, lane);
  __syncthreads();
  const int o = lane < CM_OUT ? lane : 0;
  const float eye = identity_entry(o);
  const float a = dense64(s, o, p.b[n][3][o], h) + eye;
  if (lane < CM_OUT) {
    if (affine) affine[((size_t)t * 2 + n) * CM_OUT + lane] = a;
    s_abs[n][lane] = fabsf(a - eye);
  }
  if (!reg) return;                        // uniform across the grid
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CM_OUT; i++) sum = sum + (s_abs[0][i] + s_abs[1][i]);
    reg[t] = sum / 12.0f;
  }
}

// grid = 2 (the network), block = 256
__global__ void __launch_bounds__(256)
color_mlp_backward_kernel(const ColorMlpParams p, const ColorMlpGrads g, const int T, const float* __restrict__ x,
                          const float* __restrict__ hidden, const float* __restrict__ affine,
                          const float* __restrict__ grad_affine, const float* __restrict__ grad_reg) {
  __shared__ float s_x[8];
  __shared__ float s_h[3][CM_DIM];
  __shared__ float s_d[3][CM_DIM];
  __shared__ float s_d4[CM_OUT];
  __shared__ float s_w2[CM_DIM * CM_DIM];
  __shared__ float s_w3[CM_DIM * CM_DIM];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* w4 = p.w[n][3];
  // the two 64 x 64 matrices once, for every camera: thread k then walks column k (banks k mod 32: conflict-free)
#pragma unroll
  for (int i = 0; i < 16; i++) {
    s_w2[tid + 256 * i] = p.w[n][1][tid + 256 * i];
    s_w3[tid + 256 * i] = p.w[n][2][tid + 256 * i];
  }

  float gw1[2] = {0.f, 0.f}, gw4[3] = {0.f, 0.f, 0.f}, gw2[16], gw3[16];
#pragma unroll
  for (int i = 0; i < 16; i++) gw2[i] = gw3[i] = 0.f;
  float gb1 = 0.f, gb2 = 0.f, gb3 = 0.f, gb4 = 0.f;

  // a camera's inputs, one register each: loaded one camera ahead, so their latency hides behind the previous one
  float r_x = 0.f, r_h = 0.f, r_ga = 0.f, r_a = 0.f, r_gr = 0.f;
  const auto fetch = [&](const int t) {
    const size_t tn = (size_t)t * 2 + n;
    if (tid < CM_IN) r_x = x[(size_t)t * CM_IN + tid];
    if (tid < CM_HIDDEN) r_h = hidden[tn * CM_HIDDEN + tid];
    if (tid < CM_OUT) {
      if (grad_affine) r_ga = grad_affine[tn * CM_OUT + tid];
      if (grad_reg) {
        r_a = affine[tn * CM_OUT + tid];
        r_gr = grad_reg[t];
      }
    }
  };
  fetch(0);

#pragma unroll 1
  for (int t = 0; t < T; t++) {
    if (tid < CM_IN) s_x[tid] = r_x;
    if (tid < CM_HIDDEN) s_h[tid >> 6][tid & 63] = r_h;
    if (tid < CM_OUT) {
      float d = r_ga;                      // 0 without grad_affine
      if (grad_reg) {
        const float diff = r_a - identity_entry(tid);
        const float sg = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        d = d + (r_gr * sg) / 12.0f;
      }
      s_d4[tid] = d;
    }
    __syncthreads();
    if (t + 1 < T) fetch(t + 1);

    // layer 4
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int e = tid + 256 * i;
      gw4[i] = gw4[i] + s_d4[e >> 6] * s_h[2][e & 63];
    }
    if (tid < CM_OUT) gb4 = gb4 + s_d4[tid];
    if (tid < CM_DIM) {
      float dh = 0.f;
#pragma unroll
      for (int o = 0; o < CM_OUT; o++) dh = dh + w4[o * CM_DIM + tid] * s_d4[o];
      s_d[2][tid] = s_h[2][tid] > 0.f ? dh : 0.f;
    }
    __syncthreads();

    // layer 3
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int e = tid + 256 * i;
      gw3[i] = gw3[i] + s_d[2][e >> 6] * s_h[1][e & 63];
    }
    if (tid < CM_DIM) {
      gb3 = gb3 + s_d[2][tid];
      float dh = 0.f;
#pragma unroll 8
      for (int o = 0; o < CM_DIM; o++) dh = dh + s_w3[o * CM_DIM + tid] * s_d[2][o];
      s_d[1][tid] = s_h[1][tid] > 0.f ? dh : 0.f;
    }
    __syncthreads();

    // layer 2
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int e = tid + 256 * i;
      gw2[i] = gw2[i] + s_d[1][e >> 6] * s_h[0][e & 63];
    }
    if (tid < CM_DIM) {
      gb2 = gb2 + s_d[1][tid];
      float dh = 0.f;
#pragma unroll 8
      for (int o = 0; o < CM_DIM; o++) dh = dh + s_w2[o * CM_DIM + tid] * s_d[1][o];
      s_d[0][tid] = s_h[0][tid] > 0.f ? dh : 0.f;
    }
    __syncthreads();

    // layer 1: 384 entries, e = j * 6 + k
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = tid + 256 * i;
      if (e < CM_DIM * CM_IN) gw1[i] = gw1[i] + s_d[0][e / CM_IN] * s_x[e % CM_IN];
    }
    if (tid < CM_DIM) gb1 = gb1 + s_d[0][tid];
    __syncthreads();                       // before the next camera overwrites the LDS
  }

#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int e = tid + 256 * i;
    if (e < CM_DIM * CM_IN) g.w[n][0][e] = gw1[i];
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    g.w[n][1][tid + 256 * i] = gw2[i];
    g.w[n][2][tid + 256 * i] = gw3[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) g.w[n][3][tid + 256 * i] = gw4[i];
  if (tid < CM_DIM) {
    g.b[n][0][tid] = gb1;
    g.b[n][1][tid] = gb2;
    g.b[n][2][tid] = gb3;
  }
  if (tid < CM_OUT) g.b[n][3][tid] = gb4;
}

namespace {

bool aligned4(const void* q) { return ((uintptr_t)q & 3) == 0; }

// every one of the sixteen tensors present and 4-byte aligned
template <typename S>
bool all_tensors(const S& s) {
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < 4; l++)
      if (!s.weight[n][l] || !s.bias[n][l] || !aligned4(s.weight[n][l]) || !aligned4(s.bias[n][l])) return false;
  return true;
}

ColorMlpParams kernel_params(const grpg_color_mlp_params& s) {
  ColorMlpParams p;
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < 4; l++) {
      p.w[n][l] = s.weight[n][l];
      p.b[n][l] = s.bias[n][l];
    }
  return p;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

int grpg_color_mlp_forward(const grpg_color_mlp_params* params, int T, const float* ego_pose, const float* extrinsic,
                           int extrinsic_shared, float* affine, float* x, float* reg, float* hidden,
                           void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!params || !all_tensors(*params))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: NULL or misaligned parameter tensor");
  if (T <= 0 || T > CM_MAX_T) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: T must be in [1, 2^20]");
  if (!ego_pose || !extrinsic || !aligned4(ego_pose) || !aligned4(extrinsic))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: NULL or misaligned ego_pose / extrinsic");
  if (!affine && !x && !reg) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: nothing to write");
  if (!aligned4(affine) || !aligned4(x) || !aligned4(reg) || !aligned4(hidden))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: misaligned output");
  color_mlp_forward_kernel<<<T, 128, 0, (hipStream_t)hip_stream>>>(kernel_params(*params), ego_pose, extrinsic,
                                                                  extrinsic_shared ? 0 : 16, affine, x, reg, hidden);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_color_mlp_backward(const grpg_color_mlp_params* params, int T, const float* x, const float* hidden,
                            const float* affine, const float* grad_affine, const float* grad_reg,
                            const grpg_color_mlp_grads* grads, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!params || !all_tensors(*params))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: NULL or misaligned parameter tensor");
  if (!grads || !all_tensors(*grads))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: NULL or misaligned gradient tensor");
  if (T <= 0 || T > CM_MAX_T) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: T must be in [1, 2^20]");
  if (!x || !hidden || !aligned4(x) || !aligned4(hidden))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: the backward needs the forward's x and hidden outputs");
  if (!grad_affine && !grad_reg) return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: no upstream gradient");
  if (grad_reg && !affine)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: grad_reg needs the forward's affine output");
  if (!aligned4(affine) || !aligned4(grad_affine) || !aligned4(grad_reg))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "color_mlp: misaligned affine / gradient");
  ColorMlpGrads g;
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < 4; l++) {
      g.w[n][l] = grads->weight[n][l];
      g.b[n][l] = grads->bias[n][l];
    }
  color_mlp_backward_kernel<<<2, 256, 0, (hipStream_t)hip_stream>>>(kernel_params(*params), g, T, x, hidden, affine,
                                                                   grad_affine, grad_reg);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
