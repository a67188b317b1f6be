// Implicit-GEMM convolution for gfx950 (CDNA4): float32 accumulate on the exact-f32 matrix pipe
// (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain, 157 TF peak) or on the bf16 pipe with split operands
// (x = hi + lo, three v_mfma_f32_32x32x16_bf16 per product term: float32-class accuracy; modes below).
//
// One kernel serves every dense conv of the three networks (RetinaFace 1x1/3x3,
// ArcFace 3x3 s1/s2 + 1x1 s2 shortcut + FC, OpenPose 3x3/7x7/1x1):
//
//   D[cout][pixel] = sum_k  W[cout][k] * X[k][pixel],     k = (ky, kx, cin)
//
// * Activations are NHWC, 4 bytes per element, with a physical zero halo, so a filter tap is a constant
//   byte offset from a pixel's base address: no bounds checks in the K loop, and padding
//   costs nothing (reference convs are all "same"/zero padded, e.g. openpose/model.py:6-24).
// * K is cut in slabs of 32 floats = 8 chunks of 16 B; `ktab[slab*8+chunk]` is the byte offset
//   (tap + channel) of that chunk from the pixel base.  One table covers 1x1, 3x3, 7x7, strided,
//   channel-sliced and tiny-Cin (several taps per slab) convs alike.
// * Both operands are DMA'd straight into LDS with global_load_lds (16 B per lane, no VGPR
//   round trip), 2 or 3 LDS stages: later slabs stream in under the MFMAs of slab s.
//   The LDS image of a tile row is 128 B; the chunk a lane fetches is XOR-swizzled with
//   (row>>1)&7 on the SOURCE address (the DMA destination is lane-linear), which makes the
//   ds_read_b128 fragment reads bank-conflict free.
// * MFMA rows are output channels, columns are pixels: each lane ends up with 4 consecutive
//   channels of one pixel per accumulator quad -> 16-byte NHWC stores, fused bias / ReLU /
//   PReLU / residual (optionally nearest-x2 upsampled) / second affine output.
//
// This unit is the dispatcher: which kernel variants can run a launch, the automatic choice, the checks of ta_launch_conv.
// The kernels live one family per translation unit -- conv_sym.hip (conv_igemm, conv_igemm_pipe), conv_split.hip
// (conv_igemm_split, conv_igemm_win), conv_dwpw.hip (the fused depthwise + 1x1 blocks) -- on top of conv_common.h.
#include <string.h>

#include "conv_common.h"

// ---- kernel selection ---------------------------------------------------------------------------------------------
static bool is_split_variant(int v) {                // the streamed split-role kernels: the ones that know K ranges and the fused pool
  return v == TA_CV_SPLIT_2x2 || v == TA_CV_SPLIT_2x2_P8 || v == TA_CV_SPLIT_2x4 || v == TA_CV_SPLIT_1x4 || v == TA_CV_SPLIT_1x4_W2 || v == TA_CV_SPLIT_2x2_W2;
}

// Which variants can run this conv at all (a forced variant that cannot is an error, never a silent substitution).
static bool variant_eligible(int v, const ta_conv_launch& p) {
  const bool split_in = p.in_fmt == ta_split_fmt_of(p.prec);   // what the split-role kernel reads: float32 in f32 mode, else the mode's pre-split format
  const bool deep = p.uniform_k && (p.n_slabs >= 2 || p.prec == PREC_F16);   // f16 mode: a 1x1 conv over 64 channels is ONE slab of 64
  // the split-role kernel has the LDS-staged epilogue only: every channel slice on an 8-channel boundary
  const bool staged = ((p.out_ch | p.res_ch | p.o2_ch) & 7) == 0 && (p.cout & 3) == 0;
  switch (v) {
    case TA_CV_GENERIC: return p.in_fmt == TA_FMT_F32 && !p.group_cout;
    case TA_CV_PIPE64: return deep && staged && p.coutp % 64 == 0 && !p.group_cout && (p.in_fmt == TA_FMT_F32 || (split_in && p.prec != PREC_F16));
    case TA_CV_PIPE128: return deep && staged && p.coutp % 128 == 0 && !p.group_cout && p.in_fmt == TA_FMT_F32;
    case TA_CV_SPLIT_2x2:
    case TA_CV_SPLIT_2x2_P8:
    case TA_CV_SPLIT_2x4: return deep && split_in && staged && p.coutp % 128 == 0;
    case TA_CV_SPLIT_1x4: return deep && split_in && staged && p.coutp % 64 == 0 && (!p.group_cout || p.group_cout % 64 == 0);
    case TA_CV_SPLIT_2x2_W2: return deep && split_in && staged && p.coutp % 128 == 0 && p.k_split <= 1;
    case TA_CV_SPLIT_1x4_W2: return deep && split_in && staged && p.coutp % 64 == 0 && (!p.group_cout || p.group_cout % 64 == 0) && p.k_split <= 1;
    case TA_CV_WIN_2x2:
    case TA_CV_WIN_2x4:
    case TA_CV_WIN_1x4: {
      // window-resident pixel operand: stride-1 convs with >= 4 taps on pre-split half-float tensors (f16x3 / f16x2), no fused
      // pool, no K ranges, and a patch that fits the instantiated capacity
      const bool base = deep && split_in && staged && (p.prec == PREC_F16X3 || p.prec == PREC_F16X2) && p.stride == 1 && !p.pool && p.k_split <= 1 &&
                        p.k_w * p.k_h >= 4 && p.n_slabs == p.k_w * p.k_h * p.k_cblocks;
      if (!base) return false;
      if (v == TA_CV_WIN_1x4) return p.coutp % 64 == 0 && (!p.group_cout || p.group_cout % 64 == 0) && ta_win_patch_rows(p, 256) <= TA_WIN_PR_1x4;
      if (p.coutp % 128) return false;
      return v == TA_CV_WIN_2x2 ? ta_win_patch_rows(p, 128) <= TA_WIN_PR_2x2 : ta_win_patch_rows(p, 256) <= TA_WIN_PR_2x4;
    }
  }
  return false;
}

// The automatic choice.
static int choose_variant_streamed(const ta_conv_launch& p);
static int choose_variant(const ta_conv_launch& p) {
  const int v = choose_variant_streamed(p);
  // the same tile with the pixel operand window-resident, wherever the layer qualifies (stride-1 3x3 / 7x7 on pre-split half-float
  // tensors whose patch fits): same bits, fewer L2 -> LDS bytes
  const int w = v == TA_CV_SPLIT_2x2 ? TA_CV_WIN_2x2 : (v == TA_CV_SPLIT_2x4 ? TA_CV_WIN_2x4 : (v == TA_CV_SPLIT_1x4 ? TA_CV_WIN_1x4 : 0));
  return (w && variant_eligible(w, p)) ? w : v;
}
static int choose_variant_streamed(const ta_conv_launch& p) {
  if (p.uniform_k && (p.n_slabs >= 2 || p.prec == PREC_F16)) {
    if (variant_eligible(TA_CV_SPLIT_2x2, p)) {
      if (p.prec != PREC_F32 && p.k_split == 1) {
        // 128 x 256 tiles (8 consumer waves) stream 25 % fewer DMA bytes per FLOP and measure ~8 % faster per tile
        // pair, but a CU holds one workgroup either way: take them when they do not cost a round of the 256 CUs
        const int n_ct = p.coutp / 128;
        const int t1 = ((p.M + 127) / 128) * n_ct, t2 = ((p.M + 255) / 256) * n_ct;
        const int r1 = (t1 + 255) / 256, r2 = (t2 + 255) / 256;
        if (r2 * 184 < r1 * 100) return TA_CV_SPLIT_2x4;
      }
      return TA_CV_SPLIT_2x2;
    }
    if (variant_eligible(TA_CV_SPLIT_1x4, p)) {
      // 64-channel layers with a short K (18 slabs: conv1_2 of the pose network, 544 us per step) and many tiles: two workgroups
      // per CU on a 2-stage ring hide one tile's fixed cost under the other's loop (+6 ... 10 % on those shapes, tools/conv_bench.py).
      // It pays where the K loop is as short as a tile's fixed cost (10 - 12 k cycles against the 14 k of an 18-slab loop) and
      // there are tiles for several rounds of the 256 CUs; on 36-slab shapes it measured level with or below the 3-stage and
      // window kernels (profiles/r05_w2_conv_bench.txt), and the energy A/B of the choice is closed (profiles/r06_energy_ab.txt).
      constexpr int W2_SLABS = 18, W2_TILES = 1024;
      if (p.prec != PREC_F32 && p.n_slabs <= W2_SLABS && (p.M + 255) / 256 * (p.coutp / 64) >= W2_TILES && variant_eligible(TA_CV_SPLIT_1x4_W2, p))
        return TA_CV_SPLIT_1x4_W2;
      return TA_CV_SPLIT_1x4;
    }
    if (variant_eligible(TA_CV_PIPE64, p)) return TA_CV_PIPE64;
  }
  return TA_CV_GENERIC;
}

static int launch_variant(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  switch (v) {
    case TA_CV_GENERIC:
    case TA_CV_PIPE64:
    case TA_CV_PIPE128: return ta_launch_conv_sym(ctx, v, p);
    case TA_CV_SPLIT_2x2:
    case TA_CV_SPLIT_2x2_P8:
    case TA_CV_SPLIT_2x4:
    case TA_CV_SPLIT_1x4:
    case TA_CV_SPLIT_1x4_W2:
    case TA_CV_SPLIT_2x2_W2:
    case TA_CV_WIN_2x2:
    case TA_CV_WIN_2x4:
    case TA_CV_WIN_1x4: return ta_launch_conv_split(ctx, v, p);
  }
  return ta_fail(ctx, TA_E_INVALID, "conv: unknown kernel variant %d", v);
}

int ta_launch_conv(ta_ctx* ctx, const ta_conv_launch& p_in, double flops) {
  if (p_in.M <= 0) return TA_OK;
  ta_conv_launch p = p_in;
#ifdef TA_CONV_TRACE
  p.trace_block = ctx->conv_trace_block;
#endif
  if (p.k_split < 1 || !p.partial) p.k_split = 1;
  if (p.coutp % 32 != 0 || p.cout % 4 != 0) return ta_fail(ctx, TA_E_INVALID, "conv: bad cout padding");
  if (p.prec != PREC_F32 && p.prec != PREC_BF16X3 && p.prec != PREC_BF16 && p.prec != PREC_F16X3 && p.prec != PREC_F16 && p.prec != PREC_F16X2)
    return ta_fail(ctx, TA_E_INVALID, "conv: unknown precision mode %d", p.prec);
  if (p.in_fmt != TA_FMT_F32 && p.in_fmt != ta_split_fmt_of(p.prec))
    return ta_fail(ctx, TA_E_INVALID, "conv: input tensor format %d does not belong to precision mode %d", p.in_fmt, p.prec);
  p.range_flag = ctx->range_flag;
  int v = p.variant;
  if (v != TA_CV_AUTO) {
    if (!variant_eligible(v, p))
      return ta_fail(ctx, TA_E_INVALID, "conv: forced kernel variant %d cannot run this layer (cin-uniform %d, slabs %d, coutp %d, "
                     "input format %d, groups %d)", v, p.uniform_k, p.n_slabs, p.coutp, p.in_fmt, p.group_cout ? 1 : 0);
  } else {
    const bool prefer = ctx->conv_force && variant_eligible(ctx->conv_force, p) && (!p.pool || is_split_variant(ctx->conv_force));   // (the window kernels have no fused pool)
    v = prefer ? ctx->conv_force : choose_variant(p);
    if (!variant_eligible(v, p)) return ta_fail(ctx, TA_E_INVALID, "conv: pre-split input reached a kernel that cannot read it");
  }
  const bool is_split = is_split_variant(v);
  if (!is_split || v == TA_CV_SPLIT_1x4_W2 || v == TA_CV_SPLIT_2x2_W2) p.k_split = 1;              // only the 3-stage split-role kernel knows K ranges
  if (p.pool) {                                      // only the split-role kernel's LDS-staged epilogue knows 2x2 windows
    if (!is_split || p.res || p.out2 || (p.out_ch & 7) || (p.M & 3) || (p.act != TA_ACT_RELU && p.act != TA_ACT_NONE))
      return ta_fail(ctx, TA_E_INVALID, "conv: the fused max-pool needs the split-role kernel and a plain epilogue (variant %d)", v);
    p.k_split = 1;
  }
  ctx->conv_counts[v] += 1;
  ctx->cur_flops = flops;
  ta_prof_scope scope(ctx, 0, flops);
  return launch_variant(ctx, v, p);
}

extern "C" {

int ta_debug_conv_variant(ta_ctx* ctx, int variant) {
  if (!ctx || variant < 0 || variant >= TA_CV_COUNT) return TA_E_INVALID;
  ctx->conv_force = variant;
  return TA_OK;
}

int ta_debug_kernel_work(ta_ctx* ctx, char* csv, size_t capacity, int reset) {
  if (!ctx || (!csv && capacity)) return TA_E_INVALID;
  std::string out;
  for (const auto& kv : ctx->kernel_work) {
    char line[200];
    const auto t = ctx->kernel_ms.find(kv.first);
    snprintf(line, sizeof(line), "%s;%lld;%.6e;%.6f\n", kv.first.c_str(), (long long)kv.second.first, kv.second.second,
             t == ctx->kernel_ms.end() ? 0.0 : t->second);
    out += line;
  }
  if (reset) {
    ta_drain_profile(ctx);                           // pending events point at the keys: read them out first
    ctx->kernel_work.clear();
    ctx->kernel_ms.clear();
  }
  if (out.size() + 1 > capacity) return ta_fail(ctx, TA_E_CAPACITY, "kernel_work: %zu bytes needed", out.size() + 1);
  memcpy(csv, out.c_str(), out.size() + 1);
  return TA_OK;
}

int ta_debug_conv_counts(ta_ctx* ctx, int64_t* counts16, int reset) {
  if (!ctx) return TA_E_INVALID;
  for (int i = 0; i < TA_CV_COUNT; ++i) {
    if (counts16) counts16[i] = ctx->conv_counts[i];
    if (reset) ctx->conv_counts[i] = 0;
  }
  return TA_OK;
}

}  // extern "C"
