// PSNR for gfx950: the reference's loss_utils.psnr (loss_utils.py:61-78), which train.py:258-262 evaluates up to
// three times per iteration through a boolean gather,
//   mse = mean((img1[mask] - img2[mask]) ** 2),   psnr = 20 log10(1 / sqrt(mse))
// in one pass with no host synchronisation.  No gradient is provided: the reference calls it under torch.no_grad().
//
// Layout: img1 and img2 are float32 [C,H,W], channel-major; mask is uint8 [H,W] or NULL.  One thread owns one pixel
// (lanes run along the flat pixel index): every channel load is one contiguous 256-byte row per wave at any 4-byte
// alignment.  The differences are taken and squared in float64 (exact for float32 inputs up to the final rounding
// of the sum), summed per workgroup into fixed slots, and one workgroup adds the slots in a fixed order: identical
// calls give identical bits; no atomics.
// Stats (float32 [2]): [0] psnr, [1] mse.  An empty selection gives NaN in both; identical images give mse 0 and
// psnr +inf.  Bytes per selected pixel: 8 C + 1 with a mask.
#include "abi_util.h"
#include "common.h"
#include "reduce.h"

namespace grpg {

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_MAX_WG = 2048;
constexpr size_t PS_CNT_OFF = sizeof(double) * PS_MAX_WG;

__global__ void __launch_bounds__(PS_THREADS)
psnr_forward_kernel(const int C, const int n, const int nwg, const float* __restrict__ a, const float* __restrict__ b,
                    const unsigned char* __restrict__ mask, double* __restrict__ part, unsigned int* __restrict__ cnt) {
  __shared__ double s_red_d[PS_THREADS / 64];
  __shared__ unsigned int s_red_u[PS_THREADS / 64];
  double sum = 0.0;
  unsigned int sel = 0;
  for (long long ii = blockIdx.x * PS_THREADS + threadIdx.x; ii < n; ii += nwg * PS_THREADS) {
    const int i = (int)ii;
    if (mask && !mask[i]) continue;
    for (int c = 0; c < C; c++) {
      const size_t at = (size_t)c * (size_t)n + i;
      const double d = (double)a[at] - (double)b[at];
      sum += d * d;
    }
    sel++;
  }
  const double ts = block_sum(sum, s_red_d);
  const unsigned int tn = block_sum(sel, s_red_u);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ts;
    cnt[blockIdx.x] = tn;
  }
}

__global__ void __launch_bounds__(REDUCE_THREADS)
psnr_reduce_kernel(const int C, const int nwg, const double* __restrict__ part, const unsigned int* __restrict__ cnt,
                   float* __restrict__ stats) {
  __shared__ double s_d[REDUCE_THREADS];
  __shared__ unsigned long long s_u[REDUCE_THREADS];
  const double sum = slot_sum(part, nwg, s_d);
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < nwg; i += REDUCE_THREADS) c += cnt[i];
  c = slot_sum(c, s_u);
  if (threadIdx.x != 0) return;
  const double mse = sum / ((double)c * (double)C);   // 0 / 0 = NaN for an empty selection
  stats[0] = (float)(20.0 * log10(1.0 / sqrt(mse)));
  stats[1] = (float)mse;
}

}  // namespace

}  // namespace grpg

using namespace grpg;

// ---- C ABI (include/grpg_rasterizer.h) ----
extern "C" {

size_t grpg_psnr_workspace_bytes(void) { return PS_CNT_OFF + sizeof(unsigned int) * PS_MAX_WG; }

int grpg_psnr_forward(int C, int height, int width, const float* img1, const float* img2, const unsigned char* mask,
                      float* stats, void* workspace, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (C < 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "psnr: C must be at least 1");
  if (int rc = loss_plane_check("psnr", height, width)) return rc;
  if (!img1 || !img2 || !stats) return fail(GRPG_ERR_INVALID_ARGUMENT, "psnr: NULL img1 / img2 / stats");
  if (((uintptr_t)img1 | (uintptr_t)img2 | (uintptr_t)stats) & 3)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "psnr: img1, img2 and stats must be 4-byte aligned");
  if (!workspace) return fail(GRPG_ERR_INVALID_ARGUMENT, "psnr: NULL workspace");
  if ((uintptr_t)workspace & 15) return fail(GRPG_ERR_INVALID_ARGUMENT, "psnr: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  const int n = height * width;
  const int nwg = max(1, min(PS_MAX_WG, (n + PS_THREADS - 1) / PS_THREADS));
  double* part = (double*)workspace;
  unsigned int* cnt = (unsigned int*)((char*)workspace + PS_CNT_OFF);
  psnr_forward_kernel<<<nwg, PS_THREADS, 0, st>>>(C, n, nwg, img1, img2, mask, part, cnt);
  psnr_reduce_kernel<<<1, REDUCE_THREADS, 0, st>>>(C, nwg, part, cnt, stats);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
