// The per-sample arithmetic of the raw YUV conversions (yuv.hip), as the kernels and the host entry ta_yuv_convert_samples
// both run it.  Integer work only.
//
// Every output sample is floor(v + 1/2) of an affine map v of three 8-bit inputs (or of three sums of up to four of them)
// with rational coefficients.  v + 1/2 is a multiple of 1/Q, Q the common denominator of the map's coefficients and of 2,
// so floor(v + 1/2) = floor(v + 1/2 + 1/(2Q)).  A row holds the coefficients and that constant rounded to multiples of
// 2^-YUV_SHIFT: the rounding errors add up to less than (sum of the largest inputs + 1) / 2 units, and as long as that
// is below 2^YUV_SHIFT / (2Q) the shifted sum has the floor of the exact one.  Q is at most 9745792000 (the G row of
// bt709 / tv) with inputs up to 255, and at most 2365890 with the quarter sums up to 1020: 2^48 leaves a factor of 37
// and more.  yuv.hip's yuv_make_row checks the inequality for the rows it builds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YUV_HD __host__ __device__
#else
#define YUV_HD
#endif

#define YUV_SHIFT 48

struct yuv_row {
  int64_t k[3], k0;
};
struct yuv_consts {
  yuv_row rgb[3];      // R, G, B over (Y, Cb, Cr)
  yuv_row yuv[3];      // Y, Cb, Cr over (4 R, 4 G, 4 B): the sums of a 2 x 2 block, or of fewer pixels scaled up to four
};

YUV_HD inline uint32_t yuv_apply(const yuv_row& r, uint32_t a, uint32_t b, uint32_t c) {
  const int64_t acc = r.k0 + r.k[0] * (int64_t)a + r.k[1] * (int64_t)b + r.k[2] * (int64_t)c;
  const int64_t v = acc >> YUV_SHIFT;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the chroma sample of a pixel from the two vertical sums (3 near + 1 far, in quarters) the rule names
YUV_HD inline uint32_t yuv_chroma_left_even(uint32_t v) { return (2 * v + 4) >> 3; }
YUV_HD inline uint32_t yuv_chroma_left_odd(uint32_t v0, uint32_t v1) { return (v0 + v1 + 4) >> 3; }
YUV_HD inline uint32_t yuv_chroma_center(uint32_t near, uint32_t far) { return (3 * near + far + 8) >> 4; }
