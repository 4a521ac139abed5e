// Host helpers shared by the C-ABI entry points (include/grpg_rasterizer.h) of libgrpg_rasterizer.so.  The frame's
// entries live in api.hip; every self-contained op keeps its entries next to its kernels (ssim.hip, aux_loss.hip,
// semantic_loss.hip, normal_loss.hip, reg_loss.hip, metrics.hip, optim.hip, knn.hip, sky.hip, color_correction.hip, color_mlp.hip, pose_correction.hip, letterbox.hip, nms.hip, tracks.hip, ego_loop.hip, detector.hip, lpips.hip).  Declarations only:
// each helper is defined once, in api.hip, which also owns the one thread-local string behind grpg_last_error().
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "../../include/grpg_rasterizer.h"

namespace grpg {

// Sets the calling thread's error text and returns code.
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(GRPG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

// GRPG_OK, or GRPG_ERR_NO_DEVICE with its text: there is no CPU fallback.
int ensure_device();
// First statement of an entry: clears the thread's error text, then ensure_device().
int begin_call();

// The H x W plane of the auxiliary, semantic, normal and PSNR entries.  what: the entry's prefix in the error text;
// NULL (the size queries) leaves the error text alone.
int loss_plane_check(const char* what, int height, int width);

// grpg_adam_step, grpg_densify_stats and the reg_loss entries return without a host wait, so the pinned table an
// asynchronous copy reads must outlive the call: ONE ring of growable slots per thread, each guarded by an event the
// caller records behind its copy.  A slot comes round again 32 calls later (16 iterations of a trainer that makes
// both optimizer calls); the host waits for the device only when it has run that far ahead of it.
struct OptimStagingSlot {
  char* host = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};
// The next slot with room for `bytes`, or NULL when its event or pinned memory cannot be had.
OptimStagingSlot* optim_staging_acquire(size_t bytes);

}  // namespace grpg
