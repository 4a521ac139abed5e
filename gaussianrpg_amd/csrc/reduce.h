// The fixed-order sums behind "identical calls give identical bits" of the fused losses (ssim.hip, aux_loss.hip,
// semantic_loss.hip, normal_loss.hip, reg_loss.hip, metrics.hip) and of color_correction.hip's matrix gradient; device code only.  A loss kernel sums its lanes with block_sum into one slot per workgroup; a
// launch of one workgroup of REDUCE_THREADS then adds the slots with slot_sum.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace grpg {

constexpr int REDUCE_THREADS = 1024;

// Sum of v over the lanes of the workgroup: a butterfly over the 64 lanes of each wave in T, one LDS slot per wave
// in A, and thread 0 adds the waves in ascending order.  Valid on thread 0.  s_red: blockDim.x / 64 slots.
template <class T, class A>
__device__ __forceinline__ A block_sum(T v, A* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = (A)v;
  __syncthreads();
  A t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += s_red[w];
  __syncthreads();
  return t;
}

// N sums over the lanes of the workgroup at once (color_correction.hip: the twelve sums of the matrix gradient): the
// butterfly of block_sum on each v[k], one LDS slot per value and wave, and thread k adds the waves of value k in
// ascending order.  One pair of barriers for all N.  Valid on threads 0 .. N-1: thread k returns sum k.
// s_red: N * (blockDim.x / 64) slots; blockDim.x >= N.
template <int N>
__device__ __forceinline__ float block_sum_each(float (&v)[N], float* s_red) {
  const int nw = (int)(blockDim.x >> 6);
#pragma unroll
  for (int k = 0; k < N; k++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    if ((threadIdx.x & 63) == 0) s_red[k * nw + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
  float t = 0.f;
  if ((int)threadIdx.x < N)
    for (int w = 0; w < nw; w++) t += s_red[threadIdx.x * nw + w];
  __syncthreads();
  return t;
}

// Sum over the REDUCE_THREADS threads of a value each has already accumulated: an LDS tree of halves, 512 ... 1.
// Valid on every thread.  s_red: REDUCE_THREADS slots.
template <class A>
__device__ A slot_sum(const A v, A* s_red) {
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int w = REDUCE_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
    __syncthreads();
  }
  const A t = s_red[0];
  __syncthreads();
  return t;
}

// Sum of the slots p[0 .. count): thread t adds slots t, t + REDUCE_THREADS, ... in ascending order, then the tree.
template <class A, class N>
__device__ A slot_sum(const A* __restrict__ p, const N count, A* s_red) {
  A v = 0;
  for (N i = threadIdx.x; i < count; i += REDUCE_THREADS) v += p[i];
  return slot_sum(v, s_red);
}

}  // namespace grpg
