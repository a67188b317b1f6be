// Device helpers shared by the in-place pixel kernels (tone.hip, filter.hip): the walk of a row of RGB pixels in aligned
// dwords, and Image.blend's float32 expression.  The including unit is compiled with -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int WALK_WAVE = 64;

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
