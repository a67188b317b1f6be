// Device helpers shared by the in-place pixel kernels (tone.hip, filter.hip): a workgroup's strip of rows of a region
// (the host cuts a region into strips with ta_add_strips, frame_regions.h), the walk of a row of RGB pixels in aligned
// dwords, and Image.blend's float32 expression.  The including unit is compiled with -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int WALK_THREADS = 256, WALK_WAVE = 64, WALK_WAVES = WALK_THREADS / WALK_WAVE;
constexpr int STRIP_PIXELS = 16384;        // pixels of one workgroup's strip of rows (at least one row per wave)

struct strip_item {          // one workgroup's strip: rows start .. start + count - 1 of the region recs[rec]
  int32_t rec, start, count;
};

// The lanes of a wave over the `npx` pixels at `p`: one(pixel address) for the head and the tail, four(address of three
// aligned dwords) for the groups.  Pixel k starts at p + 3 k, which is a multiple of 4 when k = p mod 4 (3 * 3 = 1 mod 4).
template <class P, class F1, class F4>
__device__ inline void walk_row(P* p, int npx, int lane, F1 one, F4 four) {
  const int head = min(npx, (int)((uintptr_t)p & 3)), groups = (npx - head) >> 2, rest = head + 4 * groups;
  const int units = head + groups + (npx - rest);
  for (int u = lane; u < units; u += WALK_WAVE) {
    if (u < head)
      one(p + 3 * u);
    else if (u < head + groups)
      four(p + 3 * (head + 4 * (u - head)));
    else
      one(p + 3 * (rest + (u - head - groups)));
  }
}

// The rows of a strip, wave by wave: body(first pixel of the row's span, pixels in it, the row, the span's first x).  Q: a record with frame,
// x0, y0, w and tab, the first row of its ellipse span table (clamped to the box on the host, ta_span_tables) or -1.
template <class P, class Q, class F>
__device__ inline void walk_strip(P* frames, int H, int W, const Q& q, const strip_item& it, const int2* __restrict__ tabs, F body) {
  const int wave = threadIdx.x / WALK_WAVE;
  for (int r = it.start + wave; r < it.start + it.count; r += WALK_WAVES) {
    const int2 span = q.tab >= 0 ? tabs[q.tab + r] : make_int2(0, q.w - 1);
    if (span.x > span.y) continue;
    body(frames + (((size_t)q.frame * H + q.y0 + r) * (size_t)W + q.x0 + span.x) * 3, span.y - span.x + 1, r, span.x);
  }
}

// Image.blend(in1, in2, f) of one sample (libImaging/Blend.c): in1 + f * (in2 - in1), a multiply and an add, never fused;
// `inside`: 0 <= f <= 1, the result is truncated; otherwise clipped to 0 .. 255 first
__device__ inline uint32_t blend(uint32_t in1, uint32_t in2, float f, bool inside) {
  const float t = __fadd_rn((float)(int)in1, __fmul_rn(f, (float)((int)in2 - (int)in1)));
  if (inside) return (uint32_t)(int)t & 255u;
  if (t <= 0.f) return 0;
  if (t >= 255.f) return 255;
  return (uint32_t)(int)t;
}

}  // namespace
