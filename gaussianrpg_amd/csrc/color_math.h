// The colour correction's per-pixel arithmetic for gfx950 -- shared by color_correction.hip (the stand-alone launch)
// and render_fwd.hip (the same map inside the render's epilogue, grpg_bind_frame_correction): ONE body of explicit
// fmaf, floating-point contraction switched OFF inside it, so that both launches produce the same bits whatever the
// surrounding code looks like (tests/test_gpu_frame_corrected.py compares bytes and planes).  Semantics:
// color_correction.hip's header comment (lib/models/color_correction.py:129-132).
#pragma once
#include "common.h"

namespace grpg {

// row i of the affine map; a: 12 floats, row-major [3,4]:  fma(A_i2, x_2, fma(A_i1, x_1, fma(A_i0, x_0, A_i3)))
__device__ __forceinline__ float affine_row(const float* a, const int i, const float (&x)[3]) {
#pragma clang fp contract(off)
  return fmaf(a[4 * i + 2], x[2], fmaf(a[4 * i + 1], x[1], fmaf(a[4 * i + 0], x[0], a[4 * i + 3])));
}

// The twelve floats of a matrix in DEVICE memory through a wave-uniform pointer, as loads from the constant address
// space: scalar loads into scalar registers, whatever stores surround them (a plain load behind a store the
// compiler cannot tell apart from the matrix becomes one vector load per lane).  The matrix must not change while
// the launch runs -- the rule of every input array.
__device__ __forceinline__ void load_affine_uniform(const float* affine, float (&a)[12]) {
  typedef const float __attribute__((address_space(4))) const_float;
  const const_float* p = (const const_float*)affine;
#pragma unroll
  for (int k = 0; k < 12; k++) a[k] = p[k];
}

}  // namespace grpg
