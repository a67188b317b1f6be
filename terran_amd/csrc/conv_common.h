// Device and launcher code shared by the conv kernel units (conv_sym.hip, conv_split.hip + conv_split_modes.hip, conv_dwpw.hip) and their
// dispatcher (conv_igemm.hip, whose file comment explains the scheme): arithmetic modes, MFMA / DMA wrappers, tile
// order, K and pixel walks, the epilogues.  Everything here is inlined into the kernels of the unit that includes it;
// each kernel is instantiated in exactly one unit.
#pragma once
#include <stdio.h>

#include "act_format.h"
#include "ta_internal.h"

#ifdef TA_CONV_TRACE
// Debug build only (TA_EXTRA_FLAGS=-DTA_CONV_TRACE): cycle stamps of ONE workgroup (ta_conv_launch::trace_block: 0 = the first
// one, which starts on an idle chip; a middle block sees the loaded one).  The library is built without relocatable device
// code, so every unit has a buffer of its own; a unit whose stamps a tool reads exports a reader: TA_TRACE_READER(name).
static __device__ __attribute__((unused)) long long ta_trace_buf[64];
#define TA_STAMP(i)                                                              \
  do {                                                                           \
    if (blockIdx.x == (unsigned)p.trace_block && (threadIdx.x & 63) == 0) ta_trace_buf[(i)] = __builtin_readcyclecounter(); \
  } while (0)
#define TA_TRACE_READER(name)                                                                   \
  extern "C" int name(long long* out, int n) {                                                  \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ta_trace_buf), sizeof(long long) * n);      \
  }
#else
#define TA_STAMP(i) do { } while (0)
#define TA_TRACE_READER(name)
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Arithmetic modes of the MFMA inner loop (activation tensors are float32, or pre-split bf16 hi|lo words in the
// bf16 modes: act_format.h):
//   PREC_F32    : v_mfma_f32_32x32x2_f32, exact f32 products.                          157 TF peak
//   PREC_BF16X3 : x = hi + lo (two bf16), products hi*hi + hi*lo + lo*hi on
//                 v_mfma_f32_32x32x16_bf16, f32 accumulate: ~1e-5 relative per product,
//                 i.e. float32-class accuracy at 3/16 of the f32 MFMA cost.              833 TF-equivalent peak
//   PREC_BF16   : hi*hi only (throughput mode, NOT within the 1e-3 parity bar).          2.5 PF peak
//   PREC_F16    : hi*hi only on IEEE half words (11 bits per operand, 2^-11 per product): for networks that take no discrete
//                 decision and whose outputs have a tolerance -- ArcFace: 3e-4 on unit-norm embedding components against a
//                 1e-3 bar (tests/probe_embed_precision.py); same weight scaling and range flag as PREC_F16X3.
//   PREC_F16X3  : the same three-product scheme with IEEE half words on v_mfma_f32_32x32x16_f16: x = hi + lo carries
//                 22 significant bits, every product hi*hi / hi*lo / lo*hi is exact in the float32 accumulator and the
//                 dropped lo*lo term is <= 2^-22 of the product -- below the rounding noise of a float32 dot product.
//                 Same MFMA count and rate as PREC_BF16X3.  Half floats end at 65504: weights are packed times a power of
//                 two per layer (their lo halves stay normal numbers; the epilogue multiplies the sums back, exactly) and
//                 an epilogue that would store |x| > 65504 raises the context's range flag (TA_E_RANGE) instead.
// Weights are split at pack time ([hi x32 | lo x32] 16-bit words per 128-byte row).  Activations either arrive in the
// same image (TA_FMT_SPLIT / TA_FMT_SPLIT16, written by the producer's epilogue) or are float32 and split in registers
// right after the ds_read.
//   PREC_F16X2  : TWO of the three products on the same operands as PREC_F16X3: (w_hi + w_lo) * x_hi -- the weights keep their 22 bits,
//                 every activation enters the contraction rounded to its hi half (11 bits; the `lo` words of the pre-split tensors
//                 are simply not read, so the shortcut trunk of a residual network still carries 22 bits from unit to unit).  A
//                 tolerance mode for networks that take no discrete decision (the embedder: tests/probe_embed_2mfma.py), 2/3 of the
//                 MFMAs of PREC_F16X3; tensors, weight image, scales and range flag are PREC_F16X3's.
enum { PREC_F32 = 0, PREC_BF16X3 = 1, PREC_BF16 = 2, PREC_F16X3 = 3, PREC_F16 = 4, PREC_F16X2 = 5 };
__host__ __device__ constexpr bool prec_x3(int prec) { return prec == PREC_BF16X3 || prec == PREC_F16X3; }
__host__ __device__ constexpr bool prec_x2(int prec) { return prec == PREC_F16X2; }                        // w_lo * x_hi + w_hi * x_hi
__host__ __device__ constexpr bool prec_half(int prec) { return prec == PREC_F16X3 || prec == PREC_F16 || prec == PREC_F16X2; }   // IEEE half words (else bf16)
__host__ __device__ constexpr int prec_nmma(int prec) { return prec_x3(prec) ? 3 : (prec_x2(prec) ? 2 : 1); }   // MFMAs per product term (16-bit modes)

// one 32x32x16 MFMA on 16-bit operand fragments held as raw bits (bf16x8 is the container type for both formats)
template <int PREC>
__device__ __forceinline__ f32x16 ta_mfma16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (prec_half(PREC))
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// float32 -> the mode's 16-bit word (round to nearest even) and back, for operands split in registers
template <int PREC>
__device__ __forceinline__ __bf16 ta_to16(float x) {
  if constexpr (prec_half(PREC)) return __builtin_bit_cast(__bf16, (_Float16)x);
  else return (__bf16)x;
}
template <int PREC>
__device__ __forceinline__ float ta_from16(__bf16 h) {
  if constexpr (prec_half(PREC)) return (float)__builtin_bit_cast(_Float16, h);
  else return (float)h;
}

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// 16 B per lane global -> LDS, address = uniform 64-bit base (SGPR pair) + per-lane 32-bit byte offset (ONE VGPR),
// LDS destination (wave-uniform) through M0.  The two-VGPR address form the builtin emits costs the DMA stream a
// quarter of its rate when MFMAs run on the same SIMD (VGPR read-port contention; tools/probe/dma_mfma_probe.hip:
// 4.8 vs 6.0 B/clk per issuing wave), the saddr form none.
__device__ __forceinline__ void ta_dma16(const char* ubase, unsigned lane_off, const float* lds_dst) {
  const unsigned ldsa = (unsigned)(size_t)LDS_PTR(lds_dst);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(ubase), "s"(ldsa)
               : "memory", "m0");
}

// Block b runs on XCD b % 8 (each XCD has its own L2).  XCD x owns a CONTIGUOUS run of pixel tiles (balanced split
// of n_pt over the 8 XCDs), walked cout-tile fastest: the workgroups of one XCD that are in flight together work on
// neighbouring image rows, so the 3x3 / 7x7 halo rows and the activation tile shared by all cout tiles are fetched
// into ONE L2 once instead of into up to 8 of them.
__device__ __forceinline__ int ta_xcd_tile(int n_pt, int xcd, int local) {
  const int base = n_pt >> 3, rem = n_pt & 7;
  if (local >= base + (xcd < rem ? 1 : 0)) return -1;
  return xcd * base + (xcd < rem ? xcd : rem) + local;
}

// A conv that FOLDS a per-channel affine of its INPUT (ArcFace's BatchNorm in front of a zero-padded 3x3 conv,
// arcface/model.py:12-14) into its weights needs a bias that depends on which filter taps fall into the padding: the
// shift reaches the sum only through in-bounds taps.  Per axis a pixel is first / middle / last -- or the only one (maps of
// one row or column: both outer taps are padding): 4 x 4 classes, bias9[class][coutp] (nine of them occur on maps of two or
// more rows and columns), TA_INTERIOR (middle, middle) == the ordinary bias.  3x3, stride 1, pad 1 only.
#define TA_INTERIOR 5
__device__ __forceinline__ int ta_border_class(int y, int x, int Ho, int Wo) {
  const int cy = Ho == 1 ? 3 : (y == 0 ? 0 : (y == Ho - 1 ? 2 : 1));
  const int cx = Wo == 1 ? 3 : (x == 0 ? 0 : (x == Wo - 1 ? 2 : 1));
  return cy * 4 + cx;
}

// ---- range guard of the half-float programs -----------------------------------------------------------------------------------
// Every epilogue of a program with half-float convs (ta_conv_launch::range_check) tracks the largest |x| it STORES -- whatever
// the op's own arithmetic mode and the tensor's format: a float32 tensor written by an exact-f32 op may be split into half
// floats in registers by its consumer.  The maximum is taken on BIT PATTERNS (sign cleared): for non-negative floats integer
// order is float order, and inf / NaN sort above every finite value -- fmaxf would drop a NaN and let it through.
#define TA_F16_MAX_BITS 0x477FE000u               /* 65504.0f */
__device__ __forceinline__ unsigned ta_absbits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned ta_amax4(unsigned m, const f32x4& v) {
  return max(max(m, max(ta_absbits(v[0]), ta_absbits(v[1]))), max(ta_absbits(v[2]), ta_absbits(v[3])));
}
// end of an epilogue: raise the flag; tools (ta_model_debug_amax) also collect the maximum itself per op
__device__ __forceinline__ void ta_range_report(const ta_conv_launch& p, unsigned amax) {
  if (amax > TA_F16_MAX_BITS) *p.range_flag = 1;
  // tools: the slots live behind the flag word (ta_ctx::range_flag, TA_AMAX_SLOT0).  Every lane reports its own maximum: callers
  // reach this point with part of the wave already returned, so a cross-lane reduction here would read exited lanes
  if (p.amax_index >= 0 && amax) atomicMax((unsigned*)p.range_flag + TA_AMAX_SLOT0 + 2 * p.amax_index, amax);
}
// ReLU that keeps a NaN a NaN (`v > 0 ? v : 0` turns it into 0 and hides it from the range guard)
__device__ __forceinline__ float ta_relu(float v) { return v < 0.f ? 0.f : v; }

// Fused epilogue shared by both kernels.  acc[a][b][r]: pixel = tile col (lane&31);
// cout = 8*(r>>2) + 4*(lane>>5) + (r&3) within the 32x32 tile.
template <int WM_TILES, int WN_TILES>
__device__ __forceinline__ void conv_epilogue(const ta_conv_launch& p, f32x16 (&acc)[WM_TILES][WN_TILES], int co_tile0,
                                              int pix_tile0, int lane, int HoWo) {
  // ---- epilogue ------------------------------------------------------------------------------
  // acc[a][b][r]: pixel = tile col (lane&31); cout = 8*(r>>2) + 4*(lane>>5) + (r&3) within the tile.
  // Loads are grouped ahead of the math and only the stores are predicated, so the compiler can
  // keep them all in flight instead of waiting per access.
  const int co_base = co_tile0 + 4 * (lane >> 5);
  f32x4 bias[WM_TILES][4];
#pragma unroll
  for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) bias[a][j] = *(const f32x4*)(p.bias + co_base + a * 32 + 8 * j);   // padded to coutp
  f32x4 slope[WM_TILES][4];
  if (p.act == TA_ACT_PRELU) {
#pragma unroll
    for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) slope[a][j] = *(const f32x4*)(p.prelu + co_base + a * 32 + 8 * j);
  }
  const int co_max = p.cout - 4;
  // per-channel power of two (weight-row exponent and activation scale of the channel written, ta_op_desc.wus_off): the
  // accumulators are scaled in place, one short-lived vector at a time -- exact, so acc * us + bias rounds once like the fma
  // would, and no [WM_TILES][4] vector array stays live next to the bias through the epilogue (register pressure of the kernel)
#pragma unroll
  for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 u = *(const f32x4*)((p.bias + p.coutp) + co_base + a * 32 + 8 * j);
#pragma unroll
      for (int b = 0; b < WN_TILES; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][4 * j + e] *= u[e];
    }
  unsigned amax = 0;                              // largest |x| stored, as a bit pattern (ta_range_report)
#pragma unroll
  for (int b = 0; b < WN_TILES; ++b) {
    const int pix_raw = pix_tile0 + b * 32 + (lane & 31);
    const int pixc = pix_raw < p.M ? pix_raw : 0;
    const int img = pixc / HoWo;
    const int rem = pixc - img * HoWo;
    const int y = rem / p.Wo;
    const int x = rem - y * p.Wo;
    const bool pix_ok = pix_raw < p.M;
    f32x4 v[WM_TILES][4];
#pragma unroll
    for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[a][j][e] = acc[a][b][4 * j + e] + bias[a][j][e];
    if (p.bias9) {                                      // border pixels: the class's bias instead (see ta_border_class)
      const int cls = ta_border_class(y, x, p.Ho, p.Wo);
      if (cls != TA_INTERIOR) {
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 b9 = *(const f32x4*)(p.bias9 + (size_t)cls * p.coutp + co_base + a * 32 + 8 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[a][j][e] = acc[a][b][4 * j + e] + b9[e];
          }
      }
    }
    if (p.act == TA_ACT_RELU) {
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[a][j][e] = ta_relu(v[a][j][e]);
    } else if (p.act == TA_ACT_PRELU) {
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[a][j][e] = v[a][j][e] > 0.f ? v[a][j][e] : v[a][j][e] * slope[a][j][e];
    }
    if (p.res) {
      const int ry = p.res_up2 ? (y >> 1) : y, rx = p.res_up2 ? (x >> 1) : x;
      const float* rs = p.res + (size_t)img * p.res_img + (size_t)ry * p.res_row + (size_t)rx * p.res_pix + p.res_off0;
      f32x4 r4[WM_TILES][4];
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = co_base + a * 32 + 8 * j;
          r4[a][j] = ta_ld4(rs, p.res_ch + (co < co_max ? co : co_max), p.res_fmt);   // clamped: masked at the store
        }
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[a][j][e] += r4[a][j][e];
    }
    float* o = p.out + (size_t)img * p.out_img + (size_t)y * p.out_row + (size_t)x * p.out_pix + p.out_off0;
    if (pix_ok) {
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = co_base + a * 32 + 8 * j;
          if (co < p.cout) {
            ta_st4(o, p.out_ch + co, p.out_fmt, v[a][j]);
            if (p.range_check) amax = ta_amax4(amax, v[a][j]);
          }
        }
    }
    if (p.out2) {
      float* o2 = p.out2 + (size_t)img * p.o2_img + (size_t)y * p.o2_row + (size_t)x * p.o2_pix + p.o2_off0;
      f32x4 sc[WM_TILES][4], sh[WM_TILES][4];
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sc[a][j] = *(const f32x4*)(p.scale2 + co_base + a * 32 + 8 * j);   // padded to coutp
          sh[a][j] = *(const f32x4*)(p.shift2 + co_base + a * 32 + 8 * j);
        }
      if (pix_ok) {
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = co_base + a * 32 + 8 * j;
            f32x4 z;
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = v[a][j][e] * sc[a][j][e] + sh[a][j][e];
            if (co < p.cout) {
              ta_st4(o2, p.o2_ch + co, p.o2_fmt, z);
              if (p.range_check) amax = ta_amax4(amax, z);
            }
          }
      }
    }
  }
  ta_range_report(p, amax);
}

// K-slab order of the uniform-K kernels (conv_igemm_pipe, conv_igemm_split): channel block OUTERMOST, then ky, then kx.
// A workgroup re-reads its input patch once per filter tap; with the channel block innermost (the packed weight order)
// every slab touches another 128-byte block of every patch pixel, so the bytes a 128 x 256-pixel tile keeps coming back to
// are the whole patch (150 KB at 23 x 40 x 128 ch; 32 co-resident tiles per XCD = 4.8 MB against a 4 MiB L2: measured
// 2.8-4x the fabric reads of the 128 x 128 tiling, tools/fetch_probe.sh).  Walking all kh x kw taps of ONE channel block
// before moving on shrinks that to 1 / cblocks of it.  Every uniform-K kernel uses this one order, so a layer's float
// summation order -- and with it every output bit -- does not depend on which of them the launcher picks for a batch size.
// Slab s' of the walk is packed weight slab (tap * cblocks + cb).  All scalar (wave-uniform) arithmetic.
struct ta_k_walk {
  int cb, kx, ky, b_off, a_slab;
  int cblocks, kw, kh, pix_bytes, row_bytes;
  __device__ __forceinline__ ta_k_walk(const ta_conv_launch& p, int s0) {
    cblocks = p.k_cblocks;
    kw = p.k_w;
    kh = p.k_h;
    pix_bytes = p.in_pix * 4;
    row_bytes = p.in_row * 4;
    if (s0 == 0) {                               // every launch but the K-split ones starts at slab 0: no division
      cb = kx = ky = b_off = a_slab = 0;
      return;
    }
    const int taps = kw * kh;
    cb = s0 / taps;
    const int tap = s0 - cb * taps;
    ky = tap / kw;
    kx = tap - ky * kw;
    b_off = cb * 128 + kx * pix_bytes + ky * row_bytes;
    a_slab = tap * cblocks + cb;
  }
  __device__ __forceinline__ void advance() {
    ++kx;
    b_off += pix_bytes;
    a_slab += cblocks;
    if (kx == kw) {
      kx = 0;
      b_off += row_bytes - kw * pix_bytes;
      if (++ky == kh) {
        ky = 0;
        ++cb;
        b_off += 128 - kh * row_bytes;
        a_slab = cb;
      }
    }
  }
};

// t / d for a launch-uniform divisor whose float32 reciprocal the launcher supplied: one multiply and a +-1 fix-up
// (exact for 0 <= t < 2^24, which the launcher checks: fast_div)
__device__ __forceinline__ int ta_div_r(int t, int d, float rd, int fast) {
  if (!fast) return t / d;
  int q = (int)((float)t * rd);
  const int r = t - q * d;
  if (r < 0) --q;
  else if (r >= d) ++q;
  return q;
}

// (img, y, x) of the pixels pt0 + d of a tile, without a full integer division per lane: the tile's first pixel is
// decomposed once (wave-uniform), every other pixel is d < 65536 further in raster order, so its carries are small
// quotients that an f32 multiply by the reciprocal gets right to +-1 (fixed up exactly).
struct ta_pixel_walk {
  int img0, y0, x0, Wo, Ho;
  float rWo, rHo;
  __device__ __forceinline__ ta_pixel_walk(const ta_conv_launch& p, int pt0, int HoWo) {
    Wo = p.Wo;
    Ho = p.Ho;
    if (p.fast_div) {                            // split-role launches: reciprocals from the launcher
      img0 = ta_div_r(pt0, HoWo, p.r_HoWo, 1);
      const int rem = pt0 - img0 * HoWo;
      y0 = ta_div_r(rem, Wo, p.r_Wo, 1);
      x0 = rem - y0 * Wo;
      rWo = p.r_Wo;
      rHo = p.r_Ho;
      return;
    }
    img0 = pt0 / HoWo;
    const int rem = pt0 - img0 * HoWo;
    y0 = rem / p.Wo;
    x0 = rem - y0 * p.Wo;
    rWo = 1.0f / (float)p.Wo;
    rHo = 1.0f / (float)p.Ho;
  }
  static __device__ __forceinline__ void divmod(int t, int d, float rd, int& q, int& r) {
    q = (int)((float)t * rd);
    r = t - q * d;
    if (r < 0) {
      --q;
      r += d;
    } else if (r >= d) {
      ++q;
      r -= d;
    }
  }
  __device__ __forceinline__ void at(int d, int& img, int& y, int& x) const {
    int qy, qi;
    divmod(x0 + d, Wo, rWo, qy, x);
    divmod(y0 + qy, Ho, rHo, qi, y);
    img = img0 + qi;
  }
};

// Epilogue of the split-role kernel, staged through LDS.  Straight from the accumulators a store instruction
// scatters 8-16 B to 32 different pixels (32 cache lines per instruction, 4-8x write amplification: measured 6.2 us
// per tile, most of a launch's fixed cost).  Here the consumers first park the raw 128 x 128 (64 x 256) tile in LDS
// as [pixel][cout] (16-byte chunks XOR-swizzled with the pixel row so the column-wise writes are conflict-free),
// then every lane takes 8 consecutive channels of one pixel -- a wave instruction covers whole 128-byte lines --
// and applies bias / ReLU / PReLU / residual / second affine output on the way out.
struct ta_f32x8 {
  f32x4 a, b;             // channels ch..ch+3, ch+4..ch+7
};
__device__ __forceinline__ ta_f32x8 ta_ld8(const float* pix, int ch, int fmt) {      // ch % 8 == 0
  ta_f32x8 r;
  if (fmt == TA_FMT_F32) {
    r.a = *(const f32x4*)(pix + ch);
    r.b = *(const f32x4*)(pix + ch + 4);
    return r;
  }
  if (fmt == TA_FMT_F16) {
    const uint4 w = *(const uint4*)((const char*)pix + 2 * ch);
    float v[8];
    ta_unpack2<true>(w.x, v[0], v[1]);
    ta_unpack2<true>(w.y, v[2], v[3]);
    ta_unpack2<true>(w.z, v[4], v[5]);
    ta_unpack2<true>(w.w, v[6], v[7]);
    r.a = f32x4{v[0], v[1], v[2], v[3]};
    r.b = f32x4{v[4], v[5], v[6], v[7]};
    return r;
  }
  const char* q = (const char*)pix + ta_split_chan(ch);
  const uint4 h = *(const uint4*)q, l = *(const uint4*)(q + 64);
  const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
  float v[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float h0, h1, l0, l1;
    if (fmt == TA_FMT_SPLIT16) {
      ta_unpack2<true>(hw[i], h0, h1);
      ta_unpack2<true>(lw[i], l0, l1);
    } else {
      ta_unpack2<false>(hw[i], h0, h1);
      ta_unpack2<false>(lw[i], l0, l1);
    }
    v[2 * i] = h0 + l0;
    v[2 * i + 1] = h1 + l1;
  }
  r.a = f32x4{v[0], v[1], v[2], v[3]};
  r.b = f32x4{v[4], v[5], v[6], v[7]};
  return r;
}
__device__ __forceinline__ void ta_st8(float* pix, int ch, int fmt, const ta_f32x8& v) {   // ch % 8 == 0
  if (fmt == TA_FMT_F32) {
    *(f32x4*)(pix + ch) = v.a;
    *(f32x4*)(pix + ch + 4) = v.b;
    return;
  }
  if (fmt == TA_FMT_F16) {
    *(uint4*)((char*)pix + 2 * ch) = make_uint4(ta_pack_half2(v.a[0], v.a[1]), ta_pack_half2(v.a[2], v.a[3]),
                                                 ta_pack_half2(v.b[0], v.b[1]), ta_pack_half2(v.b[2], v.b[3]));
    return;
  }
  const float x[8] = {v.a[0], v.a[1], v.a[2], v.a[3], v.b[0], v.b[1], v.b[2], v.b[3]};
  unsigned hw[4], lw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (fmt == TA_FMT_SPLIT16) ta_pack2<true>(x[2 * i], x[2 * i + 1], hw[i], lw[i]);
    else ta_pack2<false>(x[2 * i], x[2 * i + 1], hw[i], lw[i]);
  }
  char* q = (char*)pix + ta_split_chan(ch);
  *(uint4*)q = make_uint4(hw[0], hw[1], hw[2], hw[3]);
  *(uint4*)(q + 64) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
}

// largest |x| (bit pattern) among the n4 (1 or 2) stored 4-channel halves of v
__device__ __forceinline__ unsigned ta_absmax8(unsigned m, const ta_f32x8& v, int n4) {
  m = ta_amax4(m, v.a);
  if (n4 == 2) m = ta_amax4(m, v.b);
  return m;
}

template <int BN>
__device__ __forceinline__ void conv_epilogue_park(f32x16 (&acc)[2][2], float* lds, int cm, int cn, int lane) {
  constexpr int NCH = BN / 4;                      // 16-byte chunks per pixel row of the staged tile
  // ---- phase 1: accumulators -> LDS [pixel][cout]; acc[a][b][r]: pixel = lane & 31, cout = 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row = cn * 64 + b * 32 + (lane & 31);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (cm * 64 + a * 32 + 8 * j + 4 * (lane >> 5)) >> 2;
        *(f32x4*)(lds + (row * NCH + (c ^ (row & (NCH - 1)))) * 4) =
            f32x4{acc[a][b][4 * j], acc[a][b][4 * j + 1], acc[a][b][4 * j + 2], acc[a][b][4 * j + 3]};
      }
  }
}

// ---- phase 2 (all NT threads of the workgroup, producers included): lane = (pixel row, 8 consecutive channels)
template <int BN, int BM, int NT>
__device__ __forceinline__ void conv_epilogue_drain(const ta_conv_launch& p, const float* lds, int ct0, int pt0, int tid,
                                                    int HoWo, int ks) {
  constexpr int NCH = BN / 4;
  constexpr int G = BN / 8;                        // 8-channel groups per pixel
  constexpr int RPI = NT / G;                      // pixel rows per pass of the workgroup
  const int k8 = tid % G, r0 = tid / G;
  const int co = ct0 + 8 * k8;
  unsigned amax = 0;                               // largest |x| stored, as a bit pattern (ta_range_report)
  const bool chk = p.range_check, chk2 = chk && p.out2;
  if (p.k_split > 1) {                             // K-split: raw sums of this K range -> partial[ks][pixel][coutp]
    float* dst = p.partial + (size_t)ks * p.M * p.coutp + co;
    for (int row = r0; row < BM && pt0 + row < p.M; row += RPI) {
      const int sw = row & (NCH - 1);
      float* o = dst + (size_t)(pt0 + row) * p.coutp;
      *(f32x4*)o = *(const f32x4*)(lds + (row * NCH + ((2 * k8) ^ sw)) * 4);
      *(f32x4*)(o + 4) = *(const f32x4*)(lds + (row * NCH + ((2 * k8 + 1) ^ sw)) * 4);
    }
    return;
  }
  const int n4 = p.cout - co >= 8 ? 2 : (p.cout - co >= 4 ? 1 : 0);    // valid 4-channel halves (cout % 4 == 0)
  if (n4 == 0) return;
  const f32x4 bias0 = *(const f32x4*)(p.bias + co), bias1 = *(const f32x4*)(p.bias + co + 4);   // padded to coutp
  const f32x4 us0 = *(const f32x4*)(p.bias + p.coutp + co), us1 = *(const f32x4*)(p.bias + p.coutp + co + 4);   // per-channel power of two (ta_op_desc.wus_off)
  f32x4 sl0 = {0, 0, 0, 0}, sl1 = {0, 0, 0, 0}, sc0 = sl0, sc1 = sl0, sh0 = sl0, sh1 = sl0;
  if (p.act == TA_ACT_PRELU) {
    sl0 = *(const f32x4*)(p.prelu + co);
    sl1 = *(const f32x4*)(p.prelu + co + 4);
  }
  if (p.out2) {
    sc0 = *(const f32x4*)(p.scale2 + co);
    sc1 = *(const f32x4*)(p.scale2 + co + 4);
    sh0 = *(const f32x4*)(p.shift2 + co);
    sh1 = *(const f32x4*)(p.shift2 + co + 4);
  }
  if (p.pool) {
    // 2x2 max-pool in the epilogue: rows 4 w .. 4 w + 3 of the staged tile are the four pixels of window w and sit in lanes
    // G and 2 G apart (same 8 channels): two shuffle-max steps, then the window's first lane stores the pooled pixel.
    // (bias and ReLU are applied first -- the values the separate pool kernel would have read.)
    static_assert(4 * G <= 64 && (RPI & 3) == 0, "a window's four rows live in one wave");
    const ta_pixel_walk walk(p, pt0 >> 2, HoWo);
    for (int row = r0; row < BM; row += RPI) {
      if (pt0 + row >= p.M) break;                   // M is a multiple of 4: whole windows drop out together
      const int sw = row & (NCH - 1);
      ta_f32x8 v;
      v.a = *(const f32x4*)(lds + (row * NCH + ((2 * k8) ^ sw)) * 4);
      v.b = *(const f32x4*)(lds + (row * NCH + ((2 * k8 + 1) ^ sw)) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v.a[e] = __builtin_fmaf(v.a[e], us0[e], bias0[e]);     // us == 1 outside the half-float programs: v + bias
        v.b[e] = __builtin_fmaf(v.b[e], us1[e], bias1[e]);
        if (p.act == TA_ACT_RELU) {
          v.a[e] = ta_relu(v.a[e]);
          v.b[e] = ta_relu(v.b[e]);
        }
      }
#pragma unroll
      for (int m = G; m <= 2 * G; m <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v.a[e] = fmaxf(v.a[e], __shfl_xor(v.a[e], m));
          v.b[e] = fmaxf(v.b[e], __shfl_xor(v.b[e], m));
        }
      if ((row & 3) == 0) {
        int img, qy, qx;
        walk.at(row >> 2, img, qy, qx);
        float* o = p.out + (size_t)img * p.out_img + (size_t)qy * p.out_row + (size_t)qx * p.out_pix + p.out_off0;
        if (n4 == 2) ta_st8(o, p.out_ch + co, p.out_fmt, v);
        else ta_st4(o, p.out_ch + co, p.out_fmt, v.a);
        if (chk) amax = ta_absmax8(amax, v, n4);
      }
    }
    ta_range_report(p, amax);
    return;
  }
  int pix = pt0 + r0;
  int img, y, x;
  ta_pixel_walk(p, pt0, HoWo).at(r0, img, y, x);
#pragma unroll 2
  for (int row = r0; row < BM; row += RPI, pix += RPI) {
    if (pix >= p.M) break;
    const int sw = row & (NCH - 1);
    ta_f32x8 v;
    v.a = *(const f32x4*)(lds + (row * NCH + ((2 * k8) ^ sw)) * 4);
    v.b = *(const f32x4*)(lds + (row * NCH + ((2 * k8 + 1) ^ sw)) * 4);
    f32x4 bb0 = bias0, bb1 = bias1;
    if (p.bias9) {
      const int cls = ta_border_class(y, x, p.Ho, p.Wo);
      if (cls != TA_INTERIOR) {
        bb0 = *(const f32x4*)(p.bias9 + (size_t)cls * p.coutp + co);
        bb1 = *(const f32x4*)(p.bias9 + (size_t)cls * p.coutp + co + 4);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v.a[e] = __builtin_fmaf(v.a[e], us0[e], bb0[e]);
      v.b[e] = __builtin_fmaf(v.b[e], us1[e], bb1[e]);
    }
    if (p.act == TA_ACT_RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v.a[e] = ta_relu(v.a[e]);
        v.b[e] = ta_relu(v.b[e]);
      }
    } else if (p.act == TA_ACT_PRELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v.a[e] = v.a[e] > 0.f ? v.a[e] : v.a[e] * sl0[e];
        v.b[e] = v.b[e] > 0.f ? v.b[e] : v.b[e] * sl1[e];
      }
    }
    if (p.res) {
      const int ry = p.res_up2 ? (y >> 1) : y, rx = p.res_up2 ? (x >> 1) : x;
      const float* rs = p.res + (size_t)img * p.res_img + (size_t)ry * p.res_row + (size_t)rx * p.res_pix + p.res_off0;
      if (n4 == 2) {
        const ta_f32x8 r = ta_ld8(rs, p.res_ch + co, p.res_fmt);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v.a[e] += r.a[e];          // (a shortcut carries the exponents of the sum it joins: pack.Program.tensor_scales)
          v.b[e] += r.b[e];
        }
      } else {
        const f32x4 r = ta_ld4(rs, p.res_ch + co, p.res_fmt);
#pragma unroll
        for (int e = 0; e < 4; ++e) v.a[e] += r[e];
      }
    }
    float* o = p.out + (size_t)img * p.out_img + (size_t)y * p.out_row + (size_t)x * p.out_pix + p.out_off0;
    if (n4 == 2) ta_st8(o, p.out_ch + co, p.out_fmt, v);
    else ta_st4(o, p.out_ch + co, p.out_fmt, v.a);
    if (chk) amax = ta_absmax8(amax, v, n4);
    if (p.out2) {
      float* o2 = p.out2 + (size_t)img * p.o2_img + (size_t)y * p.o2_row + (size_t)x * p.o2_pix + p.o2_off0;
      ta_f32x8 z;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z.a[e] = v.a[e] * sc0[e] + sh0[e];
        z.b[e] = v.b[e] * sc1[e] + sh1[e];
      }
      if (n4 == 2) ta_st8(o2, p.o2_ch + co, p.o2_fmt, z);
      else ta_st4(o2, p.o2_ch + co, p.o2_fmt, z.a);
      if (chk2) amax = ta_absmax8(amax, z, n4);
    }
    x += RPI;                                        // next pass: RPI pixels further in raster order
    while (x >= p.Wo) {
      x -= p.Wo;
      if (++y == p.Ho) {
        y = 0;
        ++img;
      }
    }
  }
  ta_range_report(p, amax);
}

// ---- the same phase 2, specialised at compile time for the three epilogues that carry the bf16 workloads (launcher
// flag fast_drain: split-format tensors addressed with 32-bit byte offsets, every lane's 8 channels inside cout, no
// pool, no K-split).  The generic drain above spends ~19 lane-instructions per output element on run-time flags and
// 64-bit addressing and is VALU-issue-bound (tools/conv_trace.py); this one is ~2x leaner.  Same arithmetic, same
// order, same bits.
// F16 (the format kind): 0 = TA_FMT_SPLIT (bf16 words), 1 = TA_FMT_SPLIT16 (half words), 2 = TA_FMT_F16 (plain half floats, one
// 16-byte chunk per 8 channels); for 1 and 2 `amax` collects the largest |x| stored (range flag)
template <int F16>
__device__ __forceinline__ void ta_split_store8(char* q, const float (&x)[8], unsigned& amax) {
  if constexpr (F16 == 2) {
    *(uint4*)q = make_uint4(ta_pack_half2(x[0], x[1]), ta_pack_half2(x[2], x[3]), ta_pack_half2(x[4], x[5]), ta_pack_half2(x[6], x[7]));
  } else {
    unsigned hw[4], lw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ta_pack2<F16 == 1>(x[2 * i], x[2 * i + 1], hw[i], lw[i]);
    *(uint4*)q = make_uint4(hw[0], hw[1], hw[2], hw[3]);
    *(uint4*)(q + 64) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
  }
  if constexpr (F16 != 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = max(amax, max(ta_absbits(x[2 * i]), ta_absbits(x[2 * i + 1])));   // bit patterns: a NaN cannot hide
  }
}
template <int BN, int BM, int NT, int ACT, bool RES, int F16, bool POOL = false, bool OUT2 = RES, bool B9 = false>
// RES: + shortcut; OUT2: the second (affine) output; POOL: fused 2x2 max-pool; B9: border-class bias (ta_border_class)
__device__ __forceinline__ void conv_drain_fast(const ta_conv_launch& p, const float* lds, int ct0, int pt0, int tid, int HoWo) {
  constexpr int NCH = BN / 4;
  constexpr int G = BN / 8;
  constexpr int RPI = NT / G;
  const int k8 = tid % G, r0 = tid / G;
  const int co = ct0 + 8 * k8;
  if (co >= p.cout) return;                        // cout % 8 == 0: a lane is inside or outside with all 8 channels
  float bias[8], sl[8], sc[8], sh[8], us[8];
  *(f32x4*)bias = *(const f32x4*)(p.bias + co);
  *(f32x4*)(bias + 4) = *(const f32x4*)(p.bias + co + 4);
  *(f32x4*)us = *(const f32x4*)(p.bias + p.coutp + co);             // per-channel power of two, stored behind the bias (ta_op_desc.wus_off)
  *(f32x4*)(us + 4) = *(const f32x4*)(p.bias + p.coutp + co + 4);
  if (ACT == TA_ACT_PRELU) {
    *(f32x4*)sl = *(const f32x4*)(p.prelu + co);
    *(f32x4*)(sl + 4) = *(const f32x4*)(p.prelu + co + 4);
  }
  if (OUT2) {
    *(f32x4*)sc = *(const f32x4*)(p.scale2 + co);
    *(f32x4*)(sc + 4) = *(const f32x4*)(p.scale2 + co + 4);
    *(f32x4*)sh = *(const f32x4*)(p.shift2 + co);
    *(f32x4*)(sh + 4) = *(const f32x4*)(p.shift2 + co + 4);
  }
  auto chan = [](int ch) { return F16 == 2 ? (unsigned)(2 * ch) : ta_split_chan(ch); };
  unsigned amax = 0;
  char* const ob = (char*)p.out + chan(p.out_ch + co);
  const char* const rb = RES ? (const char*)p.res + chan(p.res_ch + co) : nullptr;
  char* const o2b = OUT2 ? (char*)p.out2 + chan(p.o2_ch + co) : nullptr;
  // POOL: rows 4 w .. 4 w + 3 of the staged tile are the pixels of window w (lanes G and 2 G apart hold the same 8
  // channels of a window's other rows); coordinates below are those of the POOLED map and a pass advances STEP of its pixels
  static_assert(!POOL || (4 * G <= 64 && (RPI & 3) == 0), "a window's four rows live in one wave");
  constexpr int STEP = POOL ? RPI / 4 : RPI;
  int img, y, x;
  ta_pixel_walk(p, POOL ? pt0 >> 2 : pt0, HoWo).at(POOL ? r0 >> 2 : r0, img, y, x);
  int pix = pt0 + r0;
  // a pass is STEP pixels further in raster order: (dy rows, dx columns) with at most one carry each when dy < Ho
  const int dy = ta_div_r(STEP, p.Wo, p.r_Wo, 1), dx = STEP - dy * p.Wo;
  const bool one_carry = dy < p.Ho;
#pragma unroll 2
  for (int row = r0; row < BM; row += RPI, pix += RPI) {
    if (pix >= p.M) break;
    const int sw = row & (NCH - 1);
    float v[8];
    *(f32x4*)v = *(const f32x4*)(lds + (row * NCH + ((2 * k8) ^ sw)) * 4);
    *(f32x4*)(v + 4) = *(const f32x4*)(lds + (row * NCH + ((2 * k8 + 1) ^ sw)) * 4);
    unsigned rh[4], rl[4];
    if (RES) {
      const int ry = p.res_up2 ? (y >> 1) : y, rx = p.res_up2 ? (x >> 1) : x;
      const char* rs = rb + 4u * (unsigned)(img * p.res_img + ry * p.res_row + rx * p.res_pix + p.res_off0);
      *(uint4*)rh = *(const uint4*)rs;
      if (F16 != 2) *(uint4*)rl = *(const uint4*)(rs + 64);
    }
    float bb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bb[e] = bias[e];
    if (B9) {
      const int cls = ta_border_class(y, x, p.Ho, p.Wo);
      if (cls != TA_INTERIOR) {
        *(f32x4*)bb = *(const f32x4*)(p.bias9 + cls * p.coutp + co);
        *(f32x4*)(bb + 4) = *(const f32x4*)(p.bias9 + cls * p.coutp + co + 4);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = __builtin_fmaf(v[e], us[e], bb[e]);       // us = 2^(a_out[co] - s[co]); all ones in the bf16 programs: v + bb
      if (ACT == TA_ACT_RELU) v[e] = ta_relu(v[e]);
      if (ACT == TA_ACT_PRELU) v[e] = v[e] > 0.f ? v[e] : v[e] * sl[e];
    }
    if (RES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float h0, h1, l0 = 0.f, l1 = 0.f;
        ta_unpack2<F16 != 0>(rh[i], h0, h1);
        if (F16 != 2) ta_unpack2<F16 != 0>(rl[i], l0, l1);
        v[2 * i] += h0 + l0;
        v[2 * i + 1] += h1 + l1;
      }
    }
    if (POOL) {
#pragma unroll
      for (int m = G; m <= 2 * G; m <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], __shfl_xor(v[e], m));
    }
    if (!POOL || (row & 3) == 0)
      ta_split_store8<F16>(ob + 4u * (unsigned)(img * p.out_img + y * p.out_row + x * p.out_pix + p.out_off0), v, amax);
    if (OUT2) {
      float z[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = v[e] * sc[e] + sh[e];
      ta_split_store8<F16>(o2b + 4u * (unsigned)(img * p.o2_img + y * p.o2_row + x * p.o2_pix + p.o2_off0), z, amax);
    }
    if (one_carry) {                                 // branch-free
      x += dx;
      const int cx = x >= p.Wo ? 1 : 0;
      x -= cx ? p.Wo : 0;
      y += dy + cx;
      const int cy = y >= p.Ho ? 1 : 0;
      y -= cy ? p.Ho : 0;
      img += cy;
    } else {
      x += STEP;
      while (x >= p.Wo) {
        x -= p.Wo;
        if (++y == p.Ho) {
          y = 0;
          ++img;
        }
      }
    }
  }
  if constexpr (F16 != 0) ta_range_report(p, amax);
}
// picks the lean drain when the launch qualifies; false = run the generic one
template <int BN, int BM, int NT, int F16>
__device__ __forceinline__ bool conv_drain_dispatch(const ta_conv_launch& p, const float* lds, int ct0, int pt0, int tid, int HoWo) {
  if (!p.fast_drain) return false;
  if (p.pool) {
    if constexpr (4 * (BN / 8) <= 64 && ((NT / (BN / 8)) & 3) == 0) {
      if (p.act == TA_ACT_RELU && !p.res && !p.out2) {
        conv_drain_fast<BN, BM, NT, TA_ACT_RELU, false, F16, true>(p, lds, ct0, pt0, tid, HoWo);
        return true;
      }
    }
    return false;
  }
  if (p.bias9) {                                      // ArcFace unit-opening convs: folded input BatchNorm, PReLU
    if (p.act == TA_ACT_PRELU && !p.res && !p.out2) {
      conv_drain_fast<BN, BM, NT, TA_ACT_PRELU, false, F16, false, false, true>(p, lds, ct0, pt0, tid, HoWo);
      return true;
    }
    return false;
  }
  if (!p.res && !p.out2) {
    if (p.act == TA_ACT_RELU) conv_drain_fast<BN, BM, NT, TA_ACT_RELU, false, F16>(p, lds, ct0, pt0, tid, HoWo);
    else if (p.act == TA_ACT_PRELU) conv_drain_fast<BN, BM, NT, TA_ACT_PRELU, false, F16>(p, lds, ct0, pt0, tid, HoWo);
    else conv_drain_fast<BN, BM, NT, TA_ACT_NONE, false, F16>(p, lds, ct0, pt0, tid, HoWo);
    return true;
  }
  if (p.res && p.act == TA_ACT_NONE) {                // unit-closing convs: + shortcut, with or without the second output
    if (p.out2) conv_drain_fast<BN, BM, NT, TA_ACT_NONE, true, F16, false, true>(p, lds, ct0, pt0, tid, HoWo);
    else conv_drain_fast<BN, BM, NT, TA_ACT_NONE, true, F16, false, false>(p, lds, ct0, pt0, tid, HoWo);
    return true;
  }
  return false;
}

// ---- LDS-staged epilogue of the symmetric-wave kernels (conv_igemm, conv_igemm_pipe, conv_dwpw) ---------------------
// The direct epilogue above stores straight from the accumulators: a store instruction scatters 16 B to 32 different
// pixels (32 cache lines per instruction).  Like the split-role kernel, these kernels now park the raw tile in the LDS ring
// they are done with -- [pixel][cout], 16-byte chunks XOR-swizzled with the pixel row -- and drain it with one lane per
// (pixel, 8 consecutive channels), whole 128-byte lines per instruction, through the same conv_epilogue_drain.  Same
// arithmetic in the same order (fma(acc, unscale, bias), activation, shortcut, second output): same bits.
// DIRECT_OK: the kernel also carries the direct epilogue (stores straight from the accumulators) for channel slices that are
// not on 8-channel boundaries.  Only the generic kernel does: the fallback sets the register budget of whatever kernel it is
// compiled into (its bias / slope / value arrays are live next to all accumulators), and no layer of the three networks takes it.
template <int WAVES_M, int WAVES_N, int WM_TILES, int WN_TILES, bool DIRECT_OK = false>
__device__ __forceinline__ void conv_finish_sym(const ta_conv_launch& p, f32x16 (&acc)[WM_TILES][WN_TILES], float* lds, int ct0,
                                                int pt0, int wm, int wn, int tid, int lane, int HoWo) {
  constexpr int BN = WAVES_M * WM_TILES * 32, BM = WAVES_N * WN_TILES * 32, NCH = BN / 4;
  if constexpr (DIRECT_OK) {
    const bool staged = ((p.out_ch | p.res_ch | p.o2_ch) & 7) == 0 && (p.cout & 3) == 0;
    if (!staged) {
      conv_epilogue<WM_TILES, WN_TILES>(p, acc, ct0 + wm * WM_TILES * 32, pt0 + wn * WN_TILES * 32, lane, HoWo);
      return;
    }
  }
  __syncthreads();                                  // every wave is done reading operand fragments: the ring is free
  if (tid == 0) TA_STAMP(21);
#pragma unroll
  for (int b = 0; b < WN_TILES; ++b) {
    const int row = (wn * WN_TILES + b) * 32 + (lane & 31);
#pragma unroll
    for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ((wm * WM_TILES + a) * 32 + 8 * j + 4 * (lane >> 5)) >> 2;
        *(f32x4*)(lds + (row * NCH + (c ^ (row & (NCH - 1)))) * 4) =
            f32x4{acc[a][b][4 * j], acc[a][b][4 * j + 1], acc[a][b][4 * j + 2], acc[a][b][4 * j + 3]};
      }
  }
  __syncthreads();
  if (tid == 0) TA_STAMP(22);                       // tile parked
  conv_epilogue_drain<BN, BM, 256>(p, lds, ct0, pt0, tid, HoWo, 0);
}

// One K slab (32) of a symmetric-wave tile: A fragments from the packed weight rows, B fragments from float32 pixel rows
// (split into 16-bit hi / lo words in registers in the split modes).  Shared by conv_igemm and conv_dwpw.
template <int WM_TILES, int WN_TILES, int PREC>
__device__ __forceinline__ void conv_slab_mma(const float* st, f32x16 (&acc)[WM_TILES][WN_TILES], int a_row0, int b_row0, int fsw,
                                              int fcb, int lane) {
  if constexpr (PREC == PREC_F32) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int pc = ((fcb + g) ^ fsw) * 4;
      f32x4 av[WM_TILES], bv[WN_TILES];
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a) av[a] = *(const f32x4*)(st + (a_row0 + a * 32) * 32 + pc);
#pragma unroll
      for (int b = 0; b < WN_TILES; ++b) bv[b] = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + pc);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int b = 0; b < WN_TILES; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][e], bv[b][e], acc[a][b], 0, 0, 0);
    }
  } else {
    // K-step t covers k = 16*kgrp + 8t + (0..7): weight chunk 2*kgrp+t (hi) / 4+2*kgrp+t (lo),
    // activation float chunks kgrp*4 + 2t and kgrp*4 + 2t + 1.
    const int kg = lane >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bf16x8 ah[WM_TILES], al[WM_TILES], bh[WN_TILES], bl[WN_TILES];
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a) {
        ah[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
        if constexpr (prec_x3(PREC) || prec_x2(PREC)) al[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
      }
#pragma unroll
      for (int b = 0; b < WN_TILES; ++b) {
        const f32x4 x0 = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + ((fcb + 2 * t) ^ fsw) * 4);
        const f32x4 x1 = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + ((fcb + 2 * t + 1) ^ fsw) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const __bf16 h0 = ta_to16<PREC>(x0[e]), h1 = ta_to16<PREC>(x1[e]);
          bh[b][e] = h0;
          bh[b][4 + e] = h1;
          if constexpr (prec_x3(PREC)) {
            bl[b][e] = ta_to16<PREC>(x0[e] - ta_from16<PREC>(h0));
            bl[b][4 + e] = ta_to16<PREC>(x1[e] - ta_from16<PREC>(h1));
          }
        }
      }
      if constexpr (prec_x3(PREC) || prec_x2(PREC)) {
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int b = 0; b < WN_TILES; ++b)
            acc[a][b] = ta_mfma16<PREC>(al[a], bh[b], acc[a][b]);
      }
      if constexpr (prec_x3(PREC)) {
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int b = 0; b < WN_TILES; ++b)
            acc[a][b] = ta_mfma16<PREC>(ah[a], bl[b], acc[a][b]);
      }
#pragma unroll
      for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
        for (int b = 0; b < WN_TILES; ++b)
          acc[a][b] = ta_mfma16<PREC>(ah[a], bh[b], acc[a][b]);
    }
  }
}

// ---- launcher side ------------------------------------------------------------------------------------------------------------
// Grid of a BN x BM tiling: n_ct cout tiles x n_pt pixel tiles, the pixel tiles dealt over the 8 XCDs (ta_xcd_tile), so
// groups * 8 workgroups of which the last few of an XCD may find no tile.
struct ta_tile_grid {
  int n_ct, n_pt, groups;
  ta_tile_grid(const ta_conv_launch& p, int BN, int BM) : n_ct(p.coutp / BN), n_pt((p.M + BM - 1) / BM), groups(((n_pt + 7) / 8) * n_ct) {}
};

// ctx->note_kernel with the kernel instance's name, formatted once per call site (one call site per template instance)
#define TA_NOTE_KERNEL(ctx, ...)                                    \
  do {                                                              \
    static char _name[80];                                          \
    if (!_name[0]) snprintf(_name, sizeof(_name), __VA_ARGS__);     \
    (ctx)->note_kernel(_name);                                      \
  } while (0)
