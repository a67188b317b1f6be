// The symmetric-wave dense conv kernels (every wave issues its own DMA and MFMAs): conv_igemm, the generic K-offset-table
// kernel, and conv_igemm_pipe, its deep-pipelined form for uniform-K layers.  conv_igemm.hip explains the scheme and
// chooses the kernel; conv_common.h holds what these kernels share with the other families.
#include "conv_common.h"

template <int WAVES_M, int WAVES_N, int WM_TILES, int WN_TILES, int PREC, bool DIRECT = false>
__global__ __launch_bounds__(256, 2) void conv_igemm(const ta_conv_launch p) {
  constexpr int BN = WAVES_M * WM_TILES * 32;   // output channels per workgroup
  constexpr int BM = WAVES_N * WN_TILES * 32;   // pixels per workgroup
  constexpr int QA = BN / 32;                   // A-tile DMA instructions per wave per slab
  constexpr int QB = BM / 32;                   // B-tile DMA instructions per wave per slab
  constexpr int STAGE = (BN + BM) * 32;         // floats per pipeline stage
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");

  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;

  // XCD-aware tile order: all cout-tiles of one pixel-tile run back to back on one XCD
  // (block b lands on XCD b%8), so the activation tile is fetched into one L2 only.
  const int n_ct = p.coutp / BN;
  const int bid = blockIdx.x;
  const int grp = bid >> 3, xcd = bid & 7;
  const int ct = grp % n_ct;
  const int n_pt = (p.M + BM - 1) / BM;
  const int pt = ta_xcd_tile(n_pt, xcd, grp / n_ct);
  if (pt < 0) return;
  const int ct0 = ct * BN;
  const int pt0 = pt * BM;

  // ---- per-lane DMA source bases -------------------------------------------------------
  // DMA instruction t (0..(BN+BM)/8) copies 8 tile rows x 128 B; lane -> (row = t*8 + lane/8,
  // physical chunk = lane%8).  Instruction t = q*4 + wave.
  const int pchunk = lane & 7;
  const int lchunk = pchunk ^ ((4 * (wave & 1) + (lane >> 4)) & 7);   // logical chunk fetched
  const int HoWo = p.Ho * p.Wo;

  const char* a_src[QA];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    const int row = (q * 4 + wave) * 8 + (lane >> 3);
    a_src[q] = (const char*)(p.w + ((size_t)(ct0 + row)) * 32 + lchunk * 4);
  }
  const char* b_src[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    const int row = (q * 4 + wave) * 8 + (lane >> 3);
    int pix = pt0 + row;
    if (pix >= p.M) pix = 0;                       // clamp: value unused (store is masked)
    const int img = pix / HoWo;
    const int rem = pix - img * HoWo;
    const int y = rem / p.Wo;
    const int x = rem - y * p.Wo;
    const size_t off = (size_t)img * p.in_img + (size_t)(y * p.stride) * p.in_row +
                       (size_t)(x * p.stride) * p.in_pix + p.in_off0;
    b_src[q] = (const char*)(p.in + off);
  }
  const size_t a_slab_bytes = (size_t)p.coutp * 128;

  auto issue = [&](int s, int stage, int koff) {
    float* base = lds + stage * STAGE;
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int t = q * 4 + wave;
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src[q] + (size_t)s * a_slab_bytes),
                                       LDS_PTR(base + t * 256), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int t = q * 4 + wave;
      __builtin_amdgcn_global_load_lds(GLB_PTR(b_src[q] + koff), LDS_PTR(base + BN * 32 + t * 256),
                                       16, 0, 0);
    }
  };

  f32x16 acc[WM_TILES][WN_TILES];
#pragma unroll
  for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
    for (int b = 0; b < WN_TILES; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // fragment read addresses: row = tile row (lane&31), logical chunk = (lane>>5)*4 + g,
  // physical chunk = logical ^ ((row>>1)&7); tile bases are multiples of 32 rows.
  const int frow = lane & 31;
  const int fsw = (frow >> 1) & 7;
  const int fcb = (lane >> 5) * 4;
  const int a_row0 = wm * WM_TILES * 32 + frow;
  const int b_row0 = BN + wn * WN_TILES * 32 + frow;

  const int S = p.n_slabs;
  int kt = p.ktab[lchunk];
  issue(0, 0, kt);
  int kt_next = (S > 1) ? p.ktab[8 + lchunk] : 0;

  for (int s = 0; s < S; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // slab s landed for every wave; everyone is done reading the other stage
    if (s + 1 < S) {
      issue(s + 1, (s + 1) & 1, kt_next);
      if (s + 2 < S) kt_next = p.ktab[(s + 2) * 8 + lchunk];
    }
    const float* st = lds + (s & 1) * STAGE;
    conv_slab_mma<WM_TILES, WN_TILES, PREC>(st, acc, a_row0, b_row0, fsw, fcb, lane);
  }

  conv_finish_sym<WAVES_M, WAVES_N, WM_TILES, WN_TILES, DIRECT>(p, acc, lds, ct0, pt0, wm, wn, tid, lane, HoWo);
}

// ---------------------------------------------------------------------------------------------------
// Deep-pipelined variant for convs whose K slabs never straddle a filter tap (cin % 32 == 0: every heavy
// layer).  Differences from conv_igemm above:
//  * the per-slab source offset is walked with scalar counters (channel block -> kx -> ky), so the K loop
//    contains no ordinary global load at all (hipcc would otherwise drain the DMA queue with vmcnt(0) at
//    the load's first use);
//  * STAGES LDS buffers, raw s_barrier and a COUNTED s_waitcnt vmcnt(N): STAGES-1 slabs stay in flight
//    across the barrier, which is what hides the L2/HBM latency once the MFMA work per slab shrinks
//    (bf16x3 / bf16: 768 / 256 MFMA cycles per slab instead of 4096).
template <int WAVES_M, int WAVES_N, int WM_TILES, int WN_TILES, int PREC, int STAGES, bool BSPLIT>
__global__ __launch_bounds__(256, (STAGES * (WAVES_M * WM_TILES + WAVES_N * WN_TILES) * 32 * 128 <= 80 * 1024) ? 2 : 1) void conv_igemm_pipe(const ta_conv_launch p) {
  constexpr int BN = WAVES_M * WM_TILES * 32;
  constexpr int BM = WAVES_N * WN_TILES * 32;
  constexpr int QA = BN / 32;
  constexpr int QB = BM / 32;
  constexpr int NI = QA + QB;                    // DMA instructions per wave per slab
  constexpr int STAGE = (BN + BM) * 32;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  static_assert(STAGES >= 2 && STAGES <= 4, "2..4 stages");

  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;

  const int n_ct = p.coutp / BN;
  const int bid = blockIdx.x;
  const int grp = bid >> 3, xcd = bid & 7;
  const int ct = grp % n_ct;
  const int n_pt = (p.M + BM - 1) / BM;
  const int pt = ta_xcd_tile(n_pt, xcd, grp / n_ct);
  if (pt < 0) return;
  const int ct0 = ct * BN;
  const int pt0 = pt * BM;

  const int pchunk = lane & 7;
  const int lchunk = pchunk ^ ((4 * (wave & 1) + (lane >> 4)) & 7);
  const int HoWo = p.Ho * p.Wo;

  const char* a_src[QA];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    const int row = (q * 4 + wave) * 8 + (lane >> 3);
    a_src[q] = (const char*)(p.w + ((size_t)(ct0 + row)) * 32 + lchunk * 4);
  }
  const char* b_src[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    const int row = (q * 4 + wave) * 8 + (lane >> 3);
    int pix = pt0 + row;
    if (pix >= p.M) pix = 0;
    const int img = pix / HoWo;
    const int rem = pix - img * HoWo;
    const int y = rem / p.Wo;
    const int x = rem - y * p.Wo;
    const size_t off = (size_t)img * p.in_img + (size_t)(y * p.stride) * p.in_row +
                       (size_t)(x * p.stride) * p.in_pix + p.in_off0 + p.in_ch_off;
    b_src[q] = (const char*)(p.in + off) + lchunk * 16;
  }
  const size_t a_slab_bytes = (size_t)p.coutp * 128;

  ta_k_walk kw_(p, 0);                            // the next slab to issue (ta_k_walk: channel block outermost)
  auto issue = [&](int, int stage) {
    float* base = lds + stage * STAGE;
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int t = q * 4 + wave;
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src[q] + (size_t)kw_.a_slab * a_slab_bytes), LDS_PTR(base + t * 256), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int t = q * 4 + wave;
      __builtin_amdgcn_global_load_lds(GLB_PTR(b_src[q] + kw_.b_off), LDS_PTR(base + BN * 32 + t * 256), 16, 0, 0);
    }
    kw_.advance();
  };

  f32x16 acc[WM_TILES][WN_TILES];
#pragma unroll
  for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
    for (int b = 0; b < WN_TILES; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int frow = lane & 31;
  const int fsw = (frow >> 1) & 7;
  const int fcb = (lane >> 5) * 4;
  const int a_row0 = wm * WM_TILES * 32 + frow;
  const int b_row0 = BN + wn * WN_TILES * 32 + frow;
  const int kg = lane >> 5;

  // Register-level software pipeline on top of the LDS ring: while the MFMAs of slab s run from one
  // fragment set, the other set is filled from LDS (ds_read_b128) and split into bf16 hi/lo for slab s+1,
  // so matrix pipe, LDS and VALU of ONE wave overlap instead of serialising (measured additive before:
  // MFMA 37 % + conversion 25 % + DMA 23 % + reads/barrier 36 % of a 7x7 layer).
  struct Frag {
    f32x4 a32[WM_TILES][4], b32[WN_TILES][4];                      // raw 16-byte chunks (f32 mode uses them directly)
    bf16x8 ah[WM_TILES][2], al[WM_TILES][2], bh[WN_TILES][2], bl[WN_TILES][2];
  };
  auto load_raw = [&](Frag& f, const float* st) {
    if constexpr (PREC == PREC_F32) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int pc = ((fcb + g) ^ fsw) * 4;
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a) f.a32[a][g] = *(const f32x4*)(st + (a_row0 + a * 32) * 32 + pc);
#pragma unroll
        for (int b = 0; b < WN_TILES; ++b) f.b32[b][g] = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + pc);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a) {
          f.ah[a][t] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
          if constexpr (prec_x3(PREC) || prec_x2(PREC)) f.al[a][t] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
        }
#pragma unroll
        for (int b = 0; b < WN_TILES; ++b) {
          if constexpr (BSPLIT) {      // pre-split activations: same [hi | lo] row image as the weights
            f.bh[b][t] = *(const bf16x8*)(st + (b_row0 + b * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
            if constexpr (prec_x3(PREC)) f.bl[b][t] = *(const bf16x8*)(st + (b_row0 + b * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
          } else {
            f.b32[b][2 * t] = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + ((fcb + 2 * t) ^ fsw) * 4);
            f.b32[b][2 * t + 1] = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + ((fcb + 2 * t + 1) ^ fsw) * 4);
          }
        }
      }
    }
  };
  auto convert = [&](Frag& f) {
    if constexpr (PREC != PREC_F32 && !BSPLIT) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < WN_TILES; ++b)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x0 = f.b32[b][2 * t][e], x1 = f.b32[b][2 * t + 1][e];
            const __bf16 h0 = ta_to16<PREC>(x0), h1 = ta_to16<PREC>(x1);
            f.bh[b][t][e] = h0;
            f.bh[b][t][4 + e] = h1;
            if constexpr (prec_x3(PREC)) {
              f.bl[b][t][e] = ta_to16<PREC>(x0 - ta_from16<PREC>(h0));
              f.bl[b][t][4 + e] = ta_to16<PREC>(x1 - ta_from16<PREC>(h1));
            }
          }
    }
  };
  auto mma = [&](const Frag& f) {
    if constexpr (PREC == PREC_F32) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
            for (int b = 0; b < WN_TILES; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a32[a][g][e], f.b32[b][g][e], acc[a][b], 0, 0, 0);
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if constexpr (prec_x3(PREC) || prec_x2(PREC)) {
#pragma unroll
          for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
            for (int b = 0; b < WN_TILES; ++b)
              acc[a][b] = ta_mfma16<PREC>(f.al[a][t], f.bh[b][t], acc[a][b]);
        }
        if constexpr (prec_x3(PREC)) {
#pragma unroll
          for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
            for (int b = 0; b < WN_TILES; ++b)
              acc[a][b] = ta_mfma16<PREC>(f.ah[a][t], f.bl[b][t], acc[a][b]);
        }
#pragma unroll
        for (int a = 0; a < WM_TILES; ++a)
#pragma unroll
          for (int b = 0; b < WN_TILES; ++b)
            acc[a][b] = ta_mfma16<PREC>(f.ah[a][t], f.bh[b][t], acc[a][b]);
      }
    }
  };

  const int S = p.n_slabs;
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i)
    if (i < S) issue(i, i);
  // slab 0 -> fragment set X
  {
    const int ahead = (S - 1) < (STAGES - 2) ? (S - 1) : (STAGES - 2);
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NI) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (STAGES - 1 < S) issue(STAGES - 1, STAGES - 1);
  }
  Frag X, Y;
  load_raw(X, lds);
  convert(X);
  int nxt_stage = 1;              // LDS stage of slab s+1
  int free_stage = 0;             // stage of slab s: free once every wave has loaded its fragments
  // one step (s + 1 < S): fragments of slab s are in `cur`; bring slab s+1 into `nxt` under the MFMAs of slab s.
  // Everything after the issue is one straight-line block so the scheduler can interleave it.
  auto step = [&](Frag& cur, Frag& nxt, int s) {
    const int rem = S - 2 - s;                         // slabs younger than s+1 that exist
    const int ahead = rem < (STAGES - 2) ? rem : (STAGES - 2);
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NI) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the fragment reads of slab s (issued in the previous step) must have RETURNED before the barrier hands its stage to the
    // next DMA: with pre-split or float32 operands nothing consumes them before the barrier (convert() is empty), so the
    // compiler's own wait sits in front of their first MFMA -- behind the barrier.  (A read that lost the race returned the
    // next slab's bytes: one run in a few hundred, found when the kernel's register allocation changed.)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // slab s+1 visible; all waves are done reading slab s from LDS
    asm volatile("" ::: "memory");
    if (s + STAGES < S) issue(s + STAGES, free_stage);
    __builtin_amdgcn_sched_barrier(0);
    load_raw(nxt, lds + nxt_stage * STAGE);
    mma(cur);
    convert(nxt);
    if constexpr (PREC != PREC_F32 && !BSPLIT) {
      // hipcc otherwise emits the MFMAs back to back and the hi/lo split after them: pin an interleave
      // (all fragment reads first, then 1 MFMA : VPM VALU) so the split runs in the MFMA shadows.
      constexpr int NREAD = 2 * (WM_TILES * ((prec_x3(PREC) || prec_x2(PREC)) ? 2 : 1) + 2 * WN_TILES);
      constexpr int NMFMA = 2 * WM_TILES * WN_TILES * prec_nmma(PREC);
      constexpr int VPM = (prec_x3(PREC) ? 58 : 30) * WN_TILES / NMFMA + 1;
      __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
#pragma unroll
      for (int i = 0; i < NMFMA; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);
      }
    }
    free_stage = nxt_stage;
    nxt_stage = nxt_stage + 1 == STAGES ? 0 : nxt_stage + 1;
  };
  int s = 0;
  for (; s + 2 < S; s += 2) {
    step(X, Y, s);
    step(Y, X, s + 1);
  }
  if (s + 1 < S) {          // S - s == 2
    step(X, Y, s);
    mma(Y);
  } else {                  // S - s == 1
    mma(X);
  }

  conv_finish_sym<WAVES_M, WAVES_N, WM_TILES, WN_TILES>(p, acc, lds, ct0, pt0, wm, wn, tid, lane, HoWo);
}

template <int WAVES_M, int WAVES_N, int WM_TILES, int WN_TILES, int PREC>
static int launch_cfg(ta_ctx* ctx, const ta_conv_launch& p) {
  constexpr int BN = WAVES_M * WM_TILES * 32;
  constexpr int BM = WAVES_N * WN_TILES * 32;
  const int groups = ta_tile_grid(p, BN, BM).groups;
  const size_t lds_bytes = 2 * (size_t)(BN + BM) * 32 * sizeof(float);
  // two instances: the usual one drains through LDS only; channel slices off the 8-channel boundaries take the one that
  // also carries the direct epilogue -- and pays for it in registers
  const bool staged = ((p.out_ch | p.res_ch | p.o2_ch) & 7) == 0 && (p.cout & 3) == 0;
  if (staged) {
    TA_NOTE_KERNEL(ctx, "conv_igemm<%d,%d,%d,%d,%d,false>", WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC);
    auto kern = conv_igemm<WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC, false>;
    TA_SET_LDS_ATTR(ctx, kern, lds_bytes);
    hipLaunchKernelGGL(kern, dim3(groups * 8), dim3(256), lds_bytes, ctx->stream, p);
  } else {
    TA_NOTE_KERNEL(ctx, "conv_igemm<%d,%d,%d,%d,%d,true>", WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC);
    auto kern = conv_igemm<WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC, true>;
    TA_SET_LDS_ATTR(ctx, kern, lds_bytes);
    hipLaunchKernelGGL(kern, dim3(groups * 8), dim3(256), lds_bytes, ctx->stream, p);
  }
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}

template <int WAVES_M, int WAVES_N, int WM_TILES, int WN_TILES, int PREC, int STAGES, bool BSPLIT>
static int launch_pipe(ta_ctx* ctx, const ta_conv_launch& p) {
  constexpr int BN = WAVES_M * WM_TILES * 32;
  constexpr int BM = WAVES_N * WN_TILES * 32;
  const int groups = ta_tile_grid(p, BN, BM).groups;
  const size_t lds_bytes = (size_t)STAGES * (BN + BM) * 32 * sizeof(float);
  auto kern = conv_igemm_pipe<WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC, STAGES, BSPLIT>;
  TA_NOTE_KERNEL(ctx, "conv_igemm_pipe<%d,%d,%d,%d,%d,%d,%s>", WAVES_M, WAVES_N, WM_TILES, WN_TILES, PREC, STAGES, BSPLIT ? "true" : "false");
  TA_SET_LDS_ATTR(ctx, kern, lds_bytes);
  hipLaunchKernelGGL(kern, dim3(groups * 8), dim3(256), lds_bytes, ctx->stream, p);
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}

template <int PREC>
static int launch_sym(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  switch (v) {
    case TA_CV_GENERIC:
      if (p.coutp % 128 == 0) return launch_cfg<2, 2, 2, 2, PREC>(ctx, p);
      if (p.coutp % 64 == 0) return launch_cfg<1, 4, 2, 1, PREC>(ctx, p);
      return launch_cfg<1, 4, 1, 1, PREC>(ctx, p);
    case TA_CV_PIPE64:
      if constexpr (PREC != PREC_F32) {
        if (p.in_fmt != TA_FMT_F32) return launch_pipe<1, 4, 2, 1, PREC, 3, true>(ctx, p);
      }
      return launch_pipe<1, 4, 2, 1, PREC, 3, false>(ctx, p);
    case TA_CV_PIPE128: return launch_pipe<2, 2, 2, 2, PREC, 3, false>(ctx, p);
  }
  return ta_fail(ctx, TA_E_INVALID, "conv: unknown kernel variant %d", v);
}

int ta_launch_conv_sym(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  switch (p.prec) {
    case PREC_F32: return launch_sym<PREC_F32>(ctx, v, p);
    case PREC_BF16X3: return launch_sym<PREC_BF16X3>(ctx, v, p);
    case PREC_F16X3: return launch_sym<PREC_F16X3>(ctx, v, p);
    case PREC_F16: return launch_sym<PREC_F16>(ctx, v, p);
    case PREC_F16X2: return launch_sym<PREC_F16X2>(ctx, v, p);
    default: return launch_sym<PREC_BF16>(ctx, v, p);
  }
}
