// Actor poses from device memory into the device segment table (grpg_bind_device_poses).
//
// A composed entry point uploads its SegmentDev rows from pinned staging; the pose fields of a row are what the host
// wrote into grpg_model_segment.  With a device-pose binding the host never sees the poses: fill_segments leaves the
// pose fields as the caller gave them (zeros, from the Python side) and parks pose_row + 1 in the bits of the row's
// spare word pad0 (0 = keep the host's pose), and this kernel, launched on the call's stream right behind the table's
// copy, overwrites rot / trans of those rows with the indexed rows of pose_rot [R,4] / pose_trans [R,3] and puts pad0
// back to 0.f.  Plain loads and stores, no arithmetic: behind it the table holds byte for byte what the host route
// would have uploaded, so every kernel that reads it computes the same bits.  Launch-sized (at most MAX_SEGMENTS
// threads); nothing to tune.
#include "common.h"

namespace grpg {

constexpr int POSE_GATHER_THREADS = 256;

static_assert(offsetof(SegmentDev, rot) % 16 == 0 && offsetof(SegmentDev, trans) == offsetof(SegmentDev, rot) + 16 &&
                  offsetof(SegmentDev, pad0) == offsetof(SegmentDev, trans) + 12,
              "rot and (trans, pad0) are stored as two aligned 16-byte pieces");

__global__ void __launch_bounds__(POSE_GATHER_THREADS)
segment_pose_gather_kernel(SegmentDev* __restrict__ segs, const int nseg, const float* __restrict__ pose_rot,
                           const float* __restrict__ pose_trans) {
  const int i = blockIdx.x * POSE_GATHER_THREADS + threadIdx.x;
  if (i >= nseg) return;
  SegmentDev& d = segs[i];
  const int row = __float_as_int(d.pad0) - 1;
  if (row < 0) return;   // a static model, or a pose the host wrote
  const float* r = pose_rot + 4 * (size_t)row;
  const float* t = pose_trans + 3 * (size_t)row;
  const float4 q = make_float4(r[0], r[1], r[2], r[3]);
  const float4 tp = make_float4(t[0], t[1], t[2], 0.f);   // .w: pad0 as fill_segments writes it without a binding
  *reinterpret_cast<float4*>(d.rot) = q;
  *reinterpret_cast<float4*>(d.trans) = tp;
}

void launch_segment_pose_gather(hipStream_t s, SegmentDev* segs, int nseg, const float* pose_rot,
                                const float* pose_trans) {
  if (nseg <= 0) return;
  const int grid = (nseg + POSE_GATHER_THREADS - 1) / POSE_GATHER_THREADS;
  hipLaunchKernelGGL(segment_pose_gather_kernel, dim3(grid), dim3(POSE_GATHER_THREADS), 0, s, segs, nseg, pose_rot,
                     pose_trans);
}

}  // namespace grpg
