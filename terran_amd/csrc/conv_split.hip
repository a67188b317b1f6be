// The split-role kernels (conv_split_kernels.h) in the half-float split modes f16x3 and f16x2, the only modes with window
// kernels; the entry point of the family, ta_launch_conv_split, which hands the other modes to conv_split_modes.hip; the second
// pass of a K-split launch; the patch bound of the window kernels.
#include "conv_split_kernels.h"

TA_TRACE_READER(ta_debug_trace_read_split)

// Second pass of a K-split conv: out = act(sum_k partial[k] + bias), ranges added in ascending order (deterministic).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const ta_conv_launch p) {
  const int c4 = p.cout >> 2;
  const int total = p.M * c4;
  const int HoWo = p.Ho * p.Wo;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int pix = i / c4, co = (i - pix * c4) * 4;
    const int img = pix / HoWo;
    const int rem = pix - img * HoWo;
    const int y = rem / p.Wo, x = rem - y * p.Wo;
    f32x4 v = *(const f32x4*)(p.bias + co);
    const f32x4 us = *(const f32x4*)((p.bias + p.coutp) + co);
    if (p.bias9) {
      const int cls = ta_border_class(y, x, p.Ho, p.Wo);
      if (cls != TA_INTERIOR) v = *(const f32x4*)(p.bias9 + (size_t)cls * p.coutp + co);
    }
    for (int k = 0; k < p.k_split; ++k) {
      const f32x4 t = *(const f32x4*)(p.partial + ((size_t)k * p.M + pix) * p.coutp + co);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(t[e], us[e], v[e]);      // us == 1: v + t
    }
    if (p.act == TA_ACT_RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ta_relu(v[e]);
    } else if (p.act == TA_ACT_PRELU) {
      const f32x4 sl = *(const f32x4*)(p.prelu + co);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * sl[e];
    }
    if (p.res) {                                     // the same order as the one-pass epilogues: activation, + shortcut, store, second output
      const int ry = p.res_up2 ? (y >> 1) : y, rx = p.res_up2 ? (x >> 1) : x;
      const f32x4 r = ta_ld4(p.res + (size_t)img * p.res_img + (size_t)ry * p.res_row + (size_t)rx * p.res_pix + p.res_off0, p.res_ch + co, p.res_fmt);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += r[e];
    }
    ta_st4(p.out + (size_t)img * p.out_img + (size_t)y * p.out_row + (size_t)x * p.out_pix + p.out_off0, p.out_ch + co,
           p.out_fmt, v);
    unsigned amax = ta_amax4(0u, v);
    if (p.out2) {
      const f32x4 sc = *(const f32x4*)(p.scale2 + co), sh = *(const f32x4*)(p.shift2 + co);
      f32x4 z;
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = v[e] * sc[e] + sh[e];
      ta_st4(p.out2 + (size_t)img * p.o2_img + (size_t)y * p.o2_row + (size_t)x * p.o2_pix + p.o2_off0, p.o2_ch + co, p.o2_fmt, z);
      amax = ta_amax4(amax, z);
    }
    if (p.range_check) ta_range_report(p, amax);
  }
}


// patch rows a BM-pixel tile of this launch can need at most (conv_igemm_win): BM - 1 raster steps, each output row crossed adds
// the two halo columns, each image crossed the halo rows between the images, plus the taps of the last pixel
int ta_win_patch_rows(const ta_conv_launch& p, int BM) {
  if (p.Wo <= 0 || p.Ho <= 0 || p.win_wp <= 0) return 1 << 30;
  const long long n = BM - 1, hp = p.win_img / p.win_wp;
  const long long rows = n + ((n + p.Wo - 1) / p.Wo) * (p.win_wp - p.Wo) + ((n + (long long)p.Ho * p.Wo - 1) / ((long long)p.Ho * p.Wo)) * (hp - p.Ho) * p.win_wp +
                         (long long)(p.k_h - 1) * p.win_wp + p.k_w;
  return rows > (1 << 30) ? (1 << 30) : (int)rows;
}


int ta_launch_conv_split(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  int rc;
  switch (p.prec) {
    case PREC_F16X3: rc = launch_split_variant<PREC_F16X3>(ctx, v, p); break;
    case PREC_F16X2: rc = launch_split_variant<PREC_F16X2>(ctx, v, p); break;
    default: rc = ta_launch_conv_split_modes(ctx, v, p); break;
  }
  if (rc != TA_OK || p.k_split <= 1) return rc;
  const int total = p.M * (p.cout >> 2);            // K ranges: the second pass adds them up and finishes the op
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, p);
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}
