// The im2col walk of detector_f16.hip's B tile: one output pixel, consecutive k = (ci * KS + ky) * KS + kx.  Plain
// integer code, host and device, so that it can be checked against the direct formula without a GPU.
//
// A thread asks for runs of consecutive k.  The direct formula costs two constant divisions, four comparisons and two
// 64-bit products per element; here a run starts with one division (start) and every further element is an increment:
// the tap rr = ky * KS + kx counts up and wraps into the next channel, the padding test is one bit of a mask computed
// once per pixel, and the stored offset is  pixel + channel + ky * ystep + rr * xs.
//   plain  stored (iy, ix) = (iy0 + ky, ix0 + kx):                     xs = 1, channel = ci * plane
//   Focus  logical channel blk * cs + c is stored channel c at (2 iy + (blk & 1), 2 ix + (blk >> 1)) (common.py:175):
//          xs = 2, channel = c * plane + (blk & 1) * w + (blk >> 1)
// and with kx = rr - KS * ky:  xs * (ky * w + kx) = ky * xs * (w - KS) + xs * rr, so ystep = xs * (w - KS).
#ifndef GRPG_DETECTOR_GATHER_H_INCLUDED
#define GRPG_DETECTOR_GATHER_H_INCLUDED

#ifndef __host__
#define __host__
#define __device__
#endif

namespace grpg {

template <int KS>
struct ConvGather {
  static_assert(KS == 1 || KS == 3, "the tap's row is (rr * 11) >> 5: rr / 3 for rr < 9");
  // per pixel
  long long pixel;     // xs * (iy0 * w + ix0): may be negative (padding), never dereferenced then
  unsigned mask;       // bit rr: tap rr lies inside the logical plane; 0 for a pixel beyond N
  // per layer
  long long plane;     // h * w of the stored tensor
  int w, xs, ystep, cs, focus, K;
  // the walk
  long long chan;
  int k, rr, c, blk;

  // iy0, ix0: the window's first logical row / column; lh, lw: the logical plane; h_in, w_in: the stored tensor's
  __host__ __device__ void init(const bool pixel_ok, const int iy0, const int ix0, const int lh, const int lw, const int h_in,
                                const int w_in, const int cs_, const bool focus_, const int K_) {
    w = w_in; focus = focus_; xs = focus_ ? 2 : 1; cs = cs_; K = K_;
    plane = (long long)h_in * w_in;
    ystep = xs * (w_in - KS);
    pixel = xs * ((long long)iy0 * w_in + ix0);
    mask = 0;
    if (pixel_ok)
      for (int ky = 0; ky < KS; ky++)
        for (int kx = 0; kx < KS; kx++)
          if (iy0 + ky >= 0 && iy0 + ky < lh && ix0 + kx >= 0 && ix0 + kx < lw) mask |= 1u << (ky * KS + kx);
  }

  __host__ __device__ void channel_offset() {
    chan = focus ? c * plane + (blk & 1) * w + (blk >> 1) : c * plane;
  }

  // the run starts at k0
  __host__ __device__ void start(const int k0) {
    k = k0;
    const int ci = k0 / (KS * KS);
    rr = k0 - ci * (KS * KS);
    if (focus) { blk = ci / cs; c = ci - blk * cs; }
    else { blk = 0; c = ci; }
    channel_offset();
  }

  // whether element k is a real tap, and its offset from the slice's first element
  __host__ __device__ bool valid() const { return k < K && ((mask >> rr) & 1u); }
  __host__ __device__ long long offset() const {
    const int ky = KS == 1 ? 0 : (rr * 11) >> 5;     // rr / 3 for rr < 9
    return pixel + chan + ky * ystep + rr * xs;
  }

  __host__ __device__ void next() {
    k++;
    if (++rr == KS * KS) {
      rr = 0;
      chan += plane;
      if (focus && ++c == cs) { c = 0; blk++; channel_offset(); }
    }
  }
};

}  // namespace grpg
#endif
