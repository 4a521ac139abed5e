// Host check of gaussianrpg_amd/csrc/detector_gather.h (tests/test_detector_f16_host.py compiles and runs it): the
// incremental im2col walk against the direct formula -- validity and offset of every element of runs of 8 and 16 from
// every multiple of 8, beyond K too, for k 1 and 3, stride 1 and 2, plain and Focus, planes down to 1 x 1.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "detector_gather.h"
using namespace grpg;
template <int KS> long check(int c_in, int h_in, int w_in, int stride, bool focus) {
  const int lh = focus ? h_in / 2 : h_in, lw = focus ? w_in / 2 : w_in, cs = focus ? c_in / 4 : c_in, K = c_in * KS * KS;
  const int p = KS / 2, ho = (lh + 2 * p - KS) / stride + 1, wo = (lw + 2 * p - KS) / stride + 1;
  const long long plane = (long long)h_in * w_in;
  long n = 0;
  for (int oy = 0; oy < ho; oy++) for (int ox = 0; ox < wo; ox++) {
    const int iy0 = oy * stride - p, ix0 = ox * stride - p;
    ConvGather<KS> g; g.init(true, iy0, ix0, lh, lw, h_in, w_in, cs, focus, K);
    for (int k0 = 0; k0 < K + 40; k0 += 8) {        // runs of 8 and 16 from every multiple of 8, beyond K too
      for (int len = 8; len <= 16; len += 8) {
        g.start(k0);
        for (int v = 0; v < len; v++, g.next()) {
          const int k = k0 + v;
          bool ok = false; long long off = 0;
          if (k < K) {
            const int ci = k / (KS * KS), rr = k - ci * KS * KS, ky = rr / KS, kx = rr - ky * KS, iy = iy0 + ky, ix = ix0 + kx;
            if (iy >= 0 && iy < lh && ix >= 0 && ix < lw) {
              ok = true;
              if (focus) { const int blk = ci / cs, c = ci - blk * cs; off = c * plane + (long long)(2 * iy + (blk & 1)) * w_in + 2 * ix + (blk >> 1); }
              else off = ci * plane + (long long)iy * w_in + ix;
            }
          }
          if (g.valid() != ok || (ok && g.offset() != off)) { printf("MISMATCH KS%d c%d %dx%d s%d f%d pix %d,%d k %d\n", KS, c_in, h_in, w_in, stride, focus, oy, ox, k); exit(1); }
          if (ok && (off < 0 || off >= cs * plane)) { printf("OOB\n"); exit(1); }
          n++;
        }
      }
    }
    ConvGather<KS> z; z.init(false, iy0, ix0, lh, lw, h_in, w_in, cs, focus, K); z.start(0);
    for (int v = 0; v < 16; v++, z.next()) if (z.valid()) { printf("pixel beyond N valid\n"); exit(1); }
  }
  return n;
}
int main() {
  long n = 0;
  for (int s = 1; s <= 2; s++) for (int c : {1, 3, 4, 12, 33}) for (int h : {1, 2, 5, 8}) for (int w : {1, 3, 7, 10}) {
    n += check<1>(c, h, w, s, false); n += check<3>(c, h, w, s, false);
    if (c % 4 == 0 && h % 2 == 0 && w % 2 == 0) { n += check<1>(c, h, w, s, true); n += check<3>(c, h, w, s, true); }
  }
  printf("ok, %ld elements\n", n);
}
