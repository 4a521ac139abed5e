// Segment tables of a whole pose tape, baked once (grpg_frame_tables_bake).
//
// A closed-loop session replays a tape of T entries, and everything in a frame's SegmentDev rows is fixed by the tape
// entry.  The host builds the static part of ALL frames' rows -- the models' pointers, the running `start`, the class
// bit, the IDFT row -- with the pose fields as the model descriptor holds them and, for a row that takes its pose
// from the tracked batch, pose_row + 1 parked in the bits of the spare word pad0 (segment_pose.hip's convention), and
// uploads them in one copy into the caller's memory.  This kernel, launched once behind that copy, overwrites rot /
// trans of those rows with the indexed rows of pose_rot [R,4] / pose_trans [R,3] and puts pad0 back to 0.f.  Plain
// loads and stores, no arithmetic: a baked row is byte for byte what fill_segments + segment_pose_gather_kernel leave
// in a frame's own table.  It runs at bind time, one thread per row of the tape; nothing to tune.
#include "common.h"

namespace grpg {

static_assert(offsetof(SegmentDev, rot) % 16 == 0 && offsetof(SegmentDev, trans) == offsetof(SegmentDev, rot) + 16 &&
                  offsetof(SegmentDev, pad0) == offsetof(SegmentDev, trans) + 12,
              "rot and (trans, pad0) are stored as two aligned 16-byte pieces");

__global__ void __launch_bounds__(FRAME_TABLE_THREADS)
frame_table_bake_kernel(SegmentDev* __restrict__ rows, const long long nrows, const float* __restrict__ pose_rot,
                        const float* __restrict__ pose_trans) {
  const long long i = (long long)blockIdx.x * FRAME_TABLE_THREADS + threadIdx.x;
  if (i >= nrows) return;
  SegmentDev& d = rows[i];
  const int row = __float_as_int(d.pad0) - 1;
  if (row < 0) return;   // a static model, or a pose the host wrote
  const float* r = pose_rot + 4 * (size_t)row;
  const float* t = pose_trans + 3 * (size_t)row;
  const float4 q = make_float4(r[0], r[1], r[2], r[3]);
  const float4 tp = make_float4(t[0], t[1], t[2], 0.f);   // .w: pad0 as fill_segments writes it without a binding
  *reinterpret_cast<float4*>(d.rot) = q;
  *reinterpret_cast<float4*>(d.trans) = tp;
}

void launch_frame_table_bake(hipStream_t s, SegmentDev* rows, long long nrows, const float* pose_rot,
                             const float* pose_trans) {
  if (nrows <= 0) return;
  const unsigned grid = (unsigned)((nrows + FRAME_TABLE_THREADS - 1) / FRAME_TABLE_THREADS);
  hipLaunchKernelGGL(frame_table_bake_kernel, dim3(grid), dim3(FRAME_TABLE_THREADS), 0, s, rows, nrows, pose_rot,
                     pose_trans);
}

}  // namespace grpg
