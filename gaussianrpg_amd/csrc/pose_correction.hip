// Pose correction of the background for gfx950: the learned rigid transform, one per image or per frame, that
// StreetGaussianModel.get_xyz / get_rotation apply to every background Gaussian (lib/models/camera_pose.py:89-114,
// street_gaussian_model.py:319-320, 345-346), with its backward, and the frame's pose table with the background's
// row in it (grpg_pose_rows_*).
//
// Replaces PoseCorrection.correct_gaussian_xyz / correct_gaussian_rotation
//   q^   = F.normalize(pose_correction_rots[id])              rot / max(|rot|, 1e-12)
//   R    = quaternion_to_matrix(q^)                           divides by |q^| once more (general_utils.py:125-146)
//   xyz' = (cat(xyz, 1) @ cat(R | trans; 0 0 0 1).T)[:, :3]
//   rotation' = quaternion_raw_multiply(q^, rotation)         NOT normalised behind it (camera_pose.py:112)
// in ONE launch for both (either input may be absent).  The row rot [4] / trans [3] is read from DEVICE memory
// (pose_correction_rots[id] is a view of the parameter): the address is uniform across the wave, there is no host copy
// and no host wait.
//
// Arithmetic: one float32 rounding per operation, in the order written (the unit is built without contraction and with
// correctly rounded division and square root):
//   n1 = sqrt(((w w + x x) + y y) + z z),  q^ = rot / max(n1, 1e-12)
//   n2 = sqrt(((q^w q^w + q^x q^x) + q^y q^y) + q^z q^z),  u = q^ / n2
//   R  = quaternion_to_matrix's nine expressions of u (compose_math.h compose_one writes the same ones)
//   xyz'_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i               compose_one's order; it stands in for the reference's
//                                                             [N,4] @ M.T, whose accumulation order PyTorch leaves open
//   rotation' = the sixteen products and twelve additions of quaternion_raw_multiply, left to right, a = q^
// A zero rot gives q^ = 0, n2 = 0, u = NaN: xyz' is NaN and rotation' zero, as in the reference.  No special case.
//
// Backward.  Per row, from the inputs alone (nothing is saved):
//   g_xyz      = R^T g_xyz'                                   ((R_0j g_0 + R_1j g_1) + R_2j g_2)
//   g_rotation = the product's transpose in b (rotation_chain_backward's expressions, a = q^)
// and SIXTEEN numbers that are linear in the upstream gradient and are summed over the N rows:
//   0..8   g_xyz'_i * x_j        (dL/dR_ij; one product each)
//   9..11  g_xyz'_i              (dL/dtrans_i)
//   12..15 the product's transpose in a (dL/dq^ through the product; four products and three additions each)
// The sums are fixed-order, without atomics:
//   1. a workgroup is 256 rows, one per lane; a lane past N contributes +0.  The 64 lanes of a wave are added by a
//      butterfly (xor 32 ... 1): 6 additions deep;
//   2. thread k < 16 adds the four wave sums of value k in ascending wave order: 3 additions (reduce.h block_sum_each),
//      and stores the workgroup's partial into workspace[k * nb + block], nb = ceil(N / 256);
//   3. ONE finishing workgroup of REDUCE_THREADS (1024): for each k, thread t adds partials t, t + 1024, ... in
//      ascending order: max(0, ceil(nb / 1024) - 1) additions, then the LDS tree of halves 512 ... 1 (reduce.h
//      slot_sum): 10 additions.
//   The longest chain of additions a sum passes is d = 19 + max(0, ceil(nb / 1024) - 1)  (19 up to N = 262144; 26 at
//   N = 1.9 M).  Adding zero is exact: a one-hot upstream gradient gives the row's own numbers back exactly.
// Thread 0 of the finishing workgroup then chains ONCE: g_trans is sums 9..11; g_u from sums 0..8 through R(u); g_q^ =
// (g_u - u (u . g_u)) / n2 + sums 12..15; g_rot = (g_q^ - q^ (q^ . g_q^)) / max(n1, 1e-12).  Summing the linear
// numbers and chaining once keeps the per-row work at nine products and the product's transpose, gives every summand
// ONE rounding (four for the product's transpose) where a per-row chain would give it some thirty, and lets the
// chain's own roundings happen once, on the totals.  Identical calls give identical bits.
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

constexpr int PC_THREADS = 256;
constexpr int PC_SUMS = 16;

struct PoseRow {
  float q[4];    // q^ = F.normalize(rot)
  float u[4];    // q^ / |q^|
  float n1, n2;  // max(|rot|, 1e-12), |q^|
  float R[9];    // quaternion_to_matrix(q^), row-major
};

// rot: 4 floats in device memory, raw (w, x, y, z)
__device__ __forceinline__ PoseRow pose_row(const float* __restrict__ rot) {
  PoseRow p;
  const float w = rot[0], x = rot[1], y = rot[2], z = rot[3];
  p.n1 = fmaxf(sqrtf(((w * w + x * x) + y * y) + z * z), 1e-12f);
  p.q[0] = w / p.n1; p.q[1] = x / p.n1; p.q[2] = y / p.n1; p.q[3] = z / p.n1;
  p.n2 = sqrtf(((p.q[0] * p.q[0] + p.q[1] * p.q[1]) + p.q[2] * p.q[2]) + p.q[3] * p.q[3]);
  const float r = p.q[0] / p.n2, qx = p.q[1] / p.n2, qy = p.q[2] / p.n2, qz = p.q[3] / p.n2;
  p.u[0] = r; p.u[1] = qx; p.u[2] = qy; p.u[3] = qz;
  p.R[0] = 1.f - 2.f * (qy * qy + qz * qz); p.R[1] = 2.f * (qx * qy - r * qz); p.R[2] = 2.f * (qx * qz + r * qy);
  p.R[3] = 2.f * (qx * qy + r * qz); p.R[4] = 1.f - 2.f * (qx * qx + qz * qz); p.R[5] = 2.f * (qy * qz - r * qx);
  p.R[6] = 2.f * (qx * qz - r * qy); p.R[7] = 2.f * (qy * qz + r * qx); p.R[8] = 1.f - 2.f * (qx * qx + qy * qy);
  return p;
}

// xyz [N,3] -> out_xyz [N,3] and / or rotation [N,4] -> out_rotation [N,4]; one row per lane
__global__ void __launch_bounds__(PC_THREADS)
pose_correct_kernel(const size_t N, const float* __restrict__ xyz, const float* __restrict__ rotation,
                    const float* __restrict__ rot, const float* __restrict__ trans, float* __restrict__ out_xyz,
                    float* __restrict__ out_rotation) {
  const size_t i = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
  if (i >= N) return;
  const PoseRow p = pose_row(rot);
  if (xyz) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 3; k++)
      out_xyz[3 * i + k] = ((p.R[3 * k] * x + p.R[3 * k + 1] * y) + p.R[3 * k + 2] * z) + trans[k];
  }
  if (rotation) {
    const float aw = p.q[0], ax = p.q[1], ay = p.q[2], az = p.q[3];
    const float bw = rotation[4 * i], bx = rotation[4 * i + 1], by = rotation[4 * i + 2], bz = rotation[4 * i + 3];
    out_rotation[4 * i + 0] = aw * bw - ax * bx - ay * by - az * bz;
    out_rotation[4 * i + 1] = aw * bx + ax * bw + ay * bz - az * by;
    out_rotation[4 * i + 2] = aw * by - ax * bz + ay * bw + az * bx;
    out_rotation[4 * i + 3] = aw * bz + ax * by - ay * bx + az * bw;
  }
}

// g_out_xyz [N,3] / g_out_rotation [N,4] -> g_xyz / g_rotation (optional each) and the workgroup's sixteen partial
// sums (optional) into partials[k * nb + block]
__global__ void __launch_bounds__(PC_THREADS)
pose_correct_backward_kernel(const size_t N, const float* __restrict__ xyz, const float* __restrict__ rotation,
                             const float* __restrict__ rot, const float* __restrict__ g_out_xyz,
                             const float* __restrict__ g_out_rotation, float* __restrict__ g_xyz,
                             float* __restrict__ g_rotation, float* __restrict__ partials) {
  __shared__ float s_red[PC_SUMS * (PC_THREADS / 64)];
  const size_t i = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
  float v[PC_SUMS];
#pragma unroll
  for (int k = 0; k < PC_SUMS; k++) v[k] = 0.f;
  if (i < N) {
    const PoseRow p = pose_row(rot);
    if (g_out_xyz) {
      const float g[3] = {g_out_xyz[3 * i], g_out_xyz[3 * i + 1], g_out_xyz[3 * i + 2]};
      if (g_xyz) {
#pragma unroll
        for (int j = 0; j < 3; j++) g_xyz[3 * i + j] = (p.R[j] * g[0] + p.R[3 + j] * g[1]) + p.R[6 + j] * g[2];
      }
      if (partials) {
        const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
          for (int j = 0; j < 3; j++) v[3 * a + j] = g[a] * x[j];
          v[9 + a] = g[a];
        }
      }
    }
    if (g_out_rotation) {
      const float gw = g_out_rotation[4 * i], gx = g_out_rotation[4 * i + 1], gy = g_out_rotation[4 * i + 2],
                  gz = g_out_rotation[4 * i + 3];
      if (g_rotation) {
        const float aw = p.q[0], ax = p.q[1], ay = p.q[2], az = p.q[3];
        g_rotation[4 * i + 0] = aw * gw + ax * gx + ay * gy + az * gz;
        g_rotation[4 * i + 1] = -ax * gw + aw * gx + az * gy - ay * gz;
        g_rotation[4 * i + 2] = -ay * gw - az * gx + aw * gy + ax * gz;
        g_rotation[4 * i + 3] = -az * gw + ay * gx - ax * gy + aw * gz;
      }
      if (partials) {
        const float bw = rotation[4 * i], bx = rotation[4 * i + 1], by = rotation[4 * i + 2],
                    bz = rotation[4 * i + 3];
        v[12] = bw * gw + bx * gx + by * gy + bz * gz;
        v[13] = -bx * gw + bw * gx - bz * gy + by * gz;
        v[14] = -by * gw + bz * gx + bw * gy - bx * gz;
        v[15] = -bz * gw - by * gx + bx * gy + bw * gz;
      }
    }
  }
  if (!partials) return;   // uniform across the grid
  const float t = block_sum_each(v, s_red);
  if (threadIdx.x < PC_SUMS) partials[threadIdx.x * (size_t)gridDim.x + blockIdx.x] = t;
}

// ONE workgroup of REDUCE_THREADS: the sixteen fixed-order sums of partials[k * nb .. (k + 1) * nb), then the chain
// to g_rot [4] / g_trans [3] (optional each) on thread 0
__global__ void __launch_bounds__(REDUCE_THREADS)
pose_correct_finish_kernel(const float* __restrict__ partials, const size_t nb, const float* __restrict__ rot,
                           float* __restrict__ g_rot, float* __restrict__ g_trans) {
  __shared__ float s_red[REDUCE_THREADS];
  float S[PC_SUMS];
#pragma unroll
  for (int k = 0; k < PC_SUMS; k++) S[k] = slot_sum(partials + k * nb, nb, s_red);
  if (threadIdx.x != 0) return;
  if (g_trans) {
    g_trans[0] = S[9]; g_trans[1] = S[10]; g_trans[2] = S[11];
  }
  if (!g_rot) return;
  const PoseRow p = pose_row(rot);
  const float r = p.u[0], x = p.u[1], y = p.u[2], z = p.u[3];
  // dL/du through the nine expressions of R(u); S[3 i + j] = dL/dR_ij
  const float gu[4] = {
      2.f * (((((x * S[7] - x * S[5]) + y * S[2]) - y * S[6]) + z * S[3]) - z * S[1]),
      2.f * (((((((y * S[1] + y * S[3]) + z * S[2]) + z * S[6]) + r * S[7]) - r * S[5]) - 2.f * (x * S[4])) -
             2.f * (x * S[8])),
      2.f * (((((((x * S[1] + x * S[3]) + z * S[5]) + z * S[7]) + r * S[2]) - r * S[6]) - 2.f * (y * S[0])) -
             2.f * (y * S[8])),
      2.f * (((((((x * S[2] + x * S[6]) + y * S[5]) + y * S[7]) + r * S[3]) - r * S[1]) - 2.f * (z * S[0])) -
             2.f * (z * S[4]))};
  // through u = q^ / n2, plus the product's path into q^
  const float along_u = ((r * gu[0] + x * gu[1]) + y * gu[2]) + z * gu[3];
  float gq[4];
#pragma unroll
  for (int k = 0; k < 4; k++) gq[k] = (gu[k] - p.u[k] * along_u) / p.n2 + S[12 + k];
  // through q^ = rot / max(|rot|, 1e-12)
  const float along_q = ((p.q[0] * gq[0] + p.q[1] * gq[1]) + p.q[2] * gq[2]) + p.q[3] * gq[3];
#pragma unroll
  for (int k = 0; k < 4; k++) g_rot[k] = (gq[k] - p.q[k] * along_q) / p.n1;
}

// rows 0 .. A-1: the actors' rows as they are; row A: the RAW correction row id (compose_one normalises it itself)
__global__ void __launch_bounds__(PC_THREADS)
pose_rows_kernel(const int A, const float* __restrict__ rot, const float* __restrict__ trans,
                 const float* __restrict__ corr_rots, const float* __restrict__ corr_trans, const int id,
                 float* __restrict__ out_rot, float* __restrict__ out_trans) {
  const int i = blockIdx.x * PC_THREADS + threadIdx.x;
  if (i > A) return;
  const float* r = i < A ? rot + 4 * (size_t)i : corr_rots + 4 * (size_t)id;
  const float* t = i < A ? trans + 3 * (size_t)i : corr_trans + 3 * (size_t)id;
#pragma unroll
  for (int k = 0; k < 4; k++) out_rot[4 * (size_t)i + k] = r[k];
#pragma unroll
  for (int k = 0; k < 3; k++) out_trans[3 * (size_t)i + k] = t[k];
}

// dense [n,4] / [n,3] parameter gradients: row id = row A of the table's gradient, every other row zero
__global__ void __launch_bounds__(PC_THREADS)
pose_rows_backward_kernel(const int A, const int n, const int id, const float* __restrict__ g_rot_rows,
                          const float* __restrict__ g_trans_rows, float* __restrict__ g_corr_rots,
                          float* __restrict__ g_corr_trans) {
  const int i = blockIdx.x * PC_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool hit = i == id;
#pragma unroll
  for (int k = 0; k < 4; k++) g_corr_rots[4 * (size_t)i + k] = hit ? g_rot_rows[4 * (size_t)A + k] : 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) g_corr_trans[3 * (size_t)i + k] = hit ? g_trans_rows[3 * (size_t)A + k] : 0.f;
}

namespace {

size_t pc_blocks(const int n) { return n <= 0 ? 0 : ((size_t)n + PC_THREADS - 1) / PC_THREADS; }

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_pose_correct_workspace_bytes(int n) { return pc_blocks(n) * PC_SUMS * sizeof(float); }

int grpg_pose_correct_forward(int n, const float* xyz, const float* rotation, const float* rot, const float* trans,
                              float* out_xyz, float* out_rotation, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (n < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: the number of rows must not be negative");
  if (!xyz && !rotation) return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: neither xyz nor rotation");
  if (!rot || (xyz && !trans)) return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: NULL correction row");
  if ((xyz && !out_xyz) || (rotation && !out_rotation) || (!xyz && out_xyz) || (!rotation && out_rotation))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: one output per input");
  if (misaligned(xyz) || misaligned(rotation) || misaligned(rot) || misaligned(trans) || misaligned(out_xyz) ||
      misaligned(out_rotation))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: pointers must be 4-byte aligned");
  if (n == 0) return GRPG_OK;
  pose_correct_kernel<<<(unsigned)pc_blocks(n), PC_THREADS, 0, (hipStream_t)hip_stream>>>(
      (size_t)n, xyz, rotation, rot, trans, out_xyz, out_rotation);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_pose_correct_backward(int n, const float* xyz, const float* rotation, const float* rot,
                               const float* grad_out_xyz, const float* grad_out_rotation, float* grad_xyz,
                               float* grad_rotation, float* grad_rot, float* grad_trans, void* workspace,
                               void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (n < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: the number of rows must not be negative");
  if (!grad_out_xyz && !grad_out_rotation)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: neither the xyz nor the rotation gradient");
  if (!rot) return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: NULL correction row");
  if ((grad_out_xyz && !xyz) || (grad_out_rotation && !rotation))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: an upstream gradient needs its forward input");
  if ((grad_xyz && !grad_out_xyz) || (grad_rotation && !grad_out_rotation))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: an input gradient needs its upstream gradient");
  if (!grad_xyz && !grad_rotation && !grad_rot && !grad_trans)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: nothing to write");
  const bool sums = grad_rot || grad_trans;
  if (sums && n > 0 && !workspace)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: grad_rot / grad_trans need a workspace");
  if (misaligned(xyz) || misaligned(rotation) || misaligned(rot) || misaligned(grad_out_xyz) ||
      misaligned(grad_out_rotation) || misaligned(grad_xyz) || misaligned(grad_rotation) || misaligned(grad_rot) ||
      misaligned(grad_trans) || misaligned(workspace))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_correct: pointers must be 4-byte aligned");
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t nb = pc_blocks(n);
  float* partials = sums ? (float*)workspace : nullptr;
  if (n > 0) {
    pose_correct_backward_kernel<<<(unsigned)nb, PC_THREADS, 0, stream>>>(
        (size_t)n, xyz, rotation, rot, grad_out_xyz, grad_out_rotation, grad_xyz, grad_rotation, partials);
    HIP_TRY(hipGetLastError());
  }
  if (sums) {
    pose_correct_finish_kernel<<<1, REDUCE_THREADS, 0, stream>>>(partials, nb, rot, grad_rot, grad_trans);
    HIP_TRY(hipGetLastError());
  }
  return GRPG_OK;
}

int grpg_pose_rows_forward(int actors, const float* rot, const float* trans, int n, const float* corr_rots,
                           const float* corr_trans, int id, float* out_rot, float* out_trans, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (actors < 0 || n <= 0 || id < 0 || id >= n)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: actors >= 0, and id one of the n > 0 correction rows");
  if ((actors > 0 && (!rot || !trans)) || !corr_rots || !corr_trans || !out_rot || !out_trans)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: NULL pointer");
  if (misaligned(rot) || misaligned(trans) || misaligned(corr_rots) || misaligned(corr_trans) ||
      misaligned(out_rot) || misaligned(out_trans))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: pointers must be 4-byte aligned");
  pose_rows_kernel<<<(unsigned)pc_blocks(actors + 1), PC_THREADS, 0, (hipStream_t)hip_stream>>>(
      actors, rot, trans, corr_rots, corr_trans, id, out_rot, out_trans);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_pose_rows_backward(int actors, int n, int id, const float* grad_rot_rows, const float* grad_trans_rows,
                            float* grad_corr_rots, float* grad_corr_trans, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (actors < 0 || n <= 0 || id < 0 || id >= n)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: actors >= 0, and id one of the n > 0 correction rows");
  if (!grad_rot_rows || !grad_trans_rows || !grad_corr_rots || !grad_corr_trans)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: NULL pointer");
  if (misaligned(grad_rot_rows) || misaligned(grad_trans_rows) || misaligned(grad_corr_rots) ||
      misaligned(grad_corr_trans))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "pose_rows: pointers must be 4-byte aligned");
  pose_rows_backward_kernel<<<(unsigned)pc_blocks(n), PC_THREADS, 0, (hipStream_t)hip_stream>>>(
      actors, n, id, grad_rot_rows, grad_trans_rows, grad_corr_rots, grad_corr_trans);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
