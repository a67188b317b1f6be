// The split-role dense conv kernels (consumer waves that only read fragments and issue MFMAs, producer waves that only issue
// the LDS DMA): conv_igemm_split, which streams both operands, and conv_igemm_win, which keeps the pixel operand of a channel
// block resident in LDS; their launchers and the switch from a TA_CV_* variant to the template instance.  conv_igemm.hip
// explains the scheme and chooses the kernel; conv_common.h holds what these kernels share with the other families.
// Two units include this file and instantiate one group of arithmetic modes each -- conv_split.hip (f16x3, f16x2: the modes
// with window kernels) and conv_split_modes.hip (f32, bf16x3, bf16, f16) -- so that neither is the whole build.
#pragma once
#include "conv_common.h"

// ---- what conv_igemm_split and conv_igemm_win have in common -----------------------------------------------------------------
// Both give every consumer wave a 64 x 64 register tile (2 x 2 MFMA tiles) and step through K sixteen at a time.
__device__ __forceinline__ void split_acc_clear(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// one k-step (16) of a consumer in the 16-bit modes, on pre-split operand fragments: al * bh, ah * bl, [al * bl], ah * bh
template <int PREC>
__device__ __forceinline__ void split_mma16(f32x16 (&acc)[2][2], const bf16x8 (&ah)[2], const bf16x8 (&al)[2], const bf16x8 (&bh)[2],
                                            const bf16x8 (&bl)[2]) {
  if constexpr (prec_x3(PREC) || prec_x2(PREC)) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = ta_mfma16<PREC>(al[a], bh[b], acc[a][b]);
  }
  if constexpr (prec_x3(PREC)) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = ta_mfma16<PREC>(ah[a], bl[b], acc[a][b]);
  }
  if constexpr (PREC == PREC_F16) {                 // a row is 64 channels of plain halfs: its second 64 bytes are 32 more of K
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = ta_mfma16<PREC>(al[a], bl[b], acc[a][b]);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ta_mfma16<PREC>(ah[a], bh[b], acc[a][b]);
}

// pin "reads first, one per MFMA slot, then the remaining MFMAs" (NREAD ds_read_b128 and NMMA MFMAs per k-step): hipcc
// otherwise sinks the reads next to their use to save registers and exposes the LDS latency in front of every group of MFMAs
template <int NREAD, int NMMA>
__device__ __forceinline__ void split_pin() {
#pragma unroll
  for (int i = 0; i < NREAD; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, NMMA - NREAD, 0);
}

// The end of a workgroup (E0, park, E1, lean-or-generic drain) is NOT shared: it stays written out in the producer and the
// consumer branch of both kernels.  One function for it, taking `bool is_consumer`, changed the instruction order of the
// 2-stage K loop of conv_igemm_split<2,2,4,.,2> (a wait and an MFMA swapped) although nothing in that loop calls it.

// ---- split-role kernel (f32 mode, or bf16 modes on pre-split activations; 128 x 128 or 64 x 256 tiles) --
// Measured with tools/probe/*: the global -> LDS DMA path sustains at most ~34 B/clk/CU however many slabs are in
// flight (24 with only 4 issuing waves), and MFMA issue is NOT slowed by DMA waves on the same SIMD -- but a wave
// that has to issue its own DMA stalls in front of the saturated texture addresser with its MFMAs queued behind.
// So the roles are split: waves 0..3 (one per SIMD) are CONSUMERS, each owning a 64 x 64 register tile (4 MFMA
// tiles, 24 MFMAs per slab in bf16x3) and doing nothing but ds_read + MFMA; waves 4..4+NP-1 are PRODUCERS that walk
// K and issue the LDS-DMA for the whole 128 x 128 workgroup tile (32 KiB per slab -> 1.5x the FLOPs per DMA byte of
// the 64 x 128 kernel conv_igemm_pipe of conv_sym.hip).  One s_barrier per slab hands a landed slab to the consumers and a drained stage back
// to the producers.  The consumer loop is software-pipelined at k-step (16) granularity with the barrier in the
// middle, so both fragment reads of a slab hide under 12 MFMAs each and only two 8-fragment sets are live.
// STAGES == 2 (4 consumer waves only): the "two tiles per CU" variant for SHORT-K layers.  A 2-stage ring of a 128 x 128 or 64 x 256 tile
// is <= 80 KiB, so two workgroups share a CU: one's fixed cost (kernel entry, address set-up, first DMA latency, park, drain: 10 - 12 k
// cycles against the 14 - 28 k of an 18 / 36-slab loop) runs under the other's K loop.  Four waves per SIMD leave 128 VGPRs per lane: the
// consumer keeps ONE fragment set (reads of a k-step, then its MFMAs) -- the LDS latency that the three-stage kernel hides inside a wave
// is hidden by the other workgroup's consumer on the same SIMD.  Same tiles, K order and MFMA order: same bits.
template <int CM, int CN, int NP, int PREC, int STAGES>
__global__ __launch_bounds__(64 * (CM * CN + NP), STAGES == 2 ? 4 : (CM * CN + NP) / 4) void conv_igemm_split(const ta_conv_launch p) {
  static_assert(NP == 4 || NP == 8, "4 or 8 producer waves");
  static_assert(STAGES == 3 || (STAGES == 2 && CM * CN == 4 && NP == 4), "3-stage ring, or the 2-stage two-workgroups-per-CU variant of the 8-wave tiles");
  static_assert(CM * CN == 4 || CM * CN == 8, "consumer grid: 1x4 (64 cout x 256 px), 2x2 (128 x 128) or 2x4 (128 x 256)");
  constexpr int NC = CM * CN;                    // consumer waves (the first NC waves of the workgroup)
  constexpr int BN = CM * 64, BM = CN * 64;
  constexpr int NI = (BN + BM) / 8 / NP;         // DMA instructions per producer wave per slab
  constexpr int QA = BN / 8 / NP;                // ... of which weight rows
  constexpr int STAGE = (BN + BM) * 32;          // floats per stage
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave == 0) TA_STAMP(0);                       // kernel entry (consumer 0)
  if (wave == NC) TA_STAMP(8);                      // kernel entry (producer 0)

  // set-up without integer divisions (launch-uniform divisors come with their reciprocals; K ranges only when K-split)
  const int n_ct = p.coutp / BN;                                 // BN, BM: powers of two
  const int n_pt = (p.M + BM - 1) / BM;
  const int tile_blocks = (((n_pt + 7) >> 3) * n_ct) << 3;      // blocks per K range
  const int ks = p.k_split > 1 ? ta_div_r(blockIdx.x, tile_blocks, p.r_tile_blocks, p.fast_div) : 0;   // K range of this workgroup
  const int bid = blockIdx.x - ks * tile_blocks;
  const int grp = bid >> 3, xcd = bid & 7;
  const int gq = ta_div_r(grp, n_ct, p.r_nct, p.fast_div);
  const int pt = ta_xcd_tile(n_pt, xcd, gq);
  if (pt < 0) return;
  const int ct0 = (grp - gq * n_ct) * BN;
  const int pt0 = pt * BM;
  const int HoWo = p.Ho * p.Wo;
  int s_begin = 0, S = p.n_slabs;
  if (p.k_split > 1) {
    s_begin = (int)(((long long)ks * p.n_slabs) / p.k_split);
    S = (int)(((long long)(ks + 1) * p.n_slabs) / p.k_split) - s_begin;
  }
  // The epilogue is ALWAYS the LDS-staged, line-coalesced one: the launcher gives this kernel only layers whose channel
  // slices are 8-aligned (variant_eligible).  The direct epilogue (stores straight from the accumulators) used to be
  // compiled in as a fallback no layer of the three networks ever took -- and set the register budget of the whole kernel:
  // 168 VGPRs + 121 spilled in the 12-wave variants, 241 in the 8-wave ones, against 143 and no spill without it.

  if (wave >= NC) {
    // ================= producer =================
    const int pw = wave - NC;
    const int pchunk = lane & 7;
    const int lchunk = pchunk ^ ((4 * (pw & 1) + (lane >> 4)) & 7);
    // uniform 64-bit base (SGPRs) + per-lane 32-bit byte offset (one VGPR): the saddr form of global_load_lds
    const char* a_base = (const char*)p.w;
    const size_t a_slab_bytes = (size_t)p.coutp * 128;
    unsigned a_off[QA];
    unsigned b_off[NI - QA];
#pragma unroll
    for (int q = 0; q < QA; ++q) a_off[q] = (unsigned)(((ct0 + (q * NP + pw) * 8 + (lane >> 3)) * 32 + lchunk * 4) * 4);
    ta_k_walk wa(p, s_begin);                       // weight rows and pixel rows are issued in the same slab order, the
    auto issue_a = [&](int, int stage) {            // weight rows two slabs ahead at the start: two walkers
#pragma unroll
      for (int q = 0; q < QA; ++q) ta_dma16(a_base + (size_t)wa.a_slab * a_slab_bytes, a_off[q], lds + stage * STAGE + (q * NP + pw) * 256);
      wa.advance();
    };
    // the weight rows of the first two slabs need no pixel arithmetic: get them moving first
    issue_a(0, 0);
    if (S > 1) issue_a(1, 1);
    // pixel rows: offsets relative to the tile's first pixel (pixels of a tile ascend in raster order)
    // fused max-pool: the walk runs over 2x2 windows (pooled map), pixel d of the tile is position (d >> 1 & 1, d & 1) of window d >> 2
    const int pl = p.pool;
    const ta_pixel_walk walk(p, pl ? pt0 >> 2 : pt0, HoWo);
    const int in_ch = p.in_ch_off + (p.group_cout ? (ct0 / p.group_cout) * p.group_cin : 0);   // grouped conv: this tile's group
    const size_t off0 = (size_t)walk.img0 * p.in_img + (size_t)((walk.y0 << pl) * p.stride) * p.in_row +
                        (size_t)((walk.x0 << pl) * p.stride) * p.in_pix + p.in_off0 + in_ch;
    const char* b_base = (const char*)(p.in + off0);
    ta_k_walk wb(p, s_begin);
    // every pixel row's DMA of slab 0 goes out as soon as its address is known: the index arithmetic of the later rows
    // (two reciprocal divisions each) then runs under the flight time of the earlier ones instead of in front of them all
#pragma unroll
    for (int q = QA; q < NI; ++q) {
      const int d = (q * NP + pw) * 8 + (lane >> 3) - BN;   // pixel row of the stage image
      int img, y, x;
      const int dd = pt0 + d < p.M ? d : 0;
      walk.at(pl ? dd >> 2 : dd, img, y, x);
      if (pl) {
        y = 2 * y + ((dd >> 1) & 1);
        x = 2 * x + (dd & 1);
      }
      const size_t off = (size_t)img * p.in_img + (size_t)(y * p.stride) * p.in_row + (size_t)(x * p.stride) * p.in_pix +
                         p.in_off0 + in_ch;
      b_off[q - QA] = (unsigned)((off - off0) * 4 + lchunk * 16);
      ta_dma16(b_base + wb.b_off, b_off[q - QA], lds + (q * NP + pw) * 256);      // slab 0 -> stage 0
    }
    wb.advance();
    auto issue_b = [&](int stage) {                 // pixel rows of the next slab in K order
#pragma unroll
      for (int q = QA; q < NI; ++q) ta_dma16(b_base + wb.b_off, b_off[q - QA], lds + stage * STAGE + (q * NP + pw) * 256);
      wb.advance();
    };
    if (wave == NC) TA_STAMP(9);                    // producer: addresses ready, slab 0 issued
    if (S > 1) issue_b(1);
    if (wave == NC) TA_STAMP(10);                    // producer: first slabs issued
    int stage = STAGES == 2 ? 0 : 2;                // stage the next issued slab goes to
    if constexpr (STAGES == 2) {
      // two stages: slabs 0 and 1 are in flight; slab s + 1 (s >= 1) goes out once B_s has handed back the stage of slab s - 1
      for (int s = 0; s < S; ++s) {
        if (s == 0 && S > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI - QA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();               // B_s
        asm volatile("" ::: "memory");
        if (s >= 1 && s + 1 < S) {
          issue_a(s + 1, stage);
          issue_b(stage);
          stage ^= 1;
        }
      }
    } else
    for (int s = 0; s < S; ++s) {
      // slab s must have landed; issue order was [A0 A1 B0 B1] then [A B] per slab, and vmcnt counts in issue order
      if (s == 0 && S > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI - QA) : "memory");
      else if (s + 1 < S) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                 // B_s: slab s landed (all producers); consumers have drained slab s-1
      asm volatile("" ::: "memory");
      if (s + 2 < S) {
        issue_a(s + 2, stage);
        issue_b(stage);
        stage = stage == 2 ? 0 : stage + 1;
      }
    }
    {                                               // help drain the parked tile: twice the lanes for the epilogue math
      __builtin_amdgcn_s_barrier();                 // E0
      __builtin_amdgcn_s_barrier();                 // E1
      asm volatile("" ::: "memory");
      bool done = false;
      if constexpr (PREC != PREC_F32) done = conv_drain_dispatch<BN, BM, 64 * (NC + NP), (PREC == PREC_F16 ? 2 : (prec_half(PREC) ? 1 : 0))>(p, lds, ct0, pt0, tid, HoWo);
      if (!done) conv_epilogue_drain<BN, BM, 64 * (NC + NP)>(p, lds, ct0, pt0, tid, HoWo, ks);
    }
    return;
  }

  // ================= consumer =================
  const int cm = wave / CN, cn = wave % CN;
  int stage = 0;                                    // stage of the slab being consumed
  f32x16 acc[2][2];
  split_acc_clear(acc);
  const int frow = lane & 31;
  const int fsw = (frow >> 1) & 7;
  const int kg = lane >> 5;
  const int a_row0 = cm * 64 + frow;
  const int b_row0 = BN + cn * 64 + frow;
  struct Frag {                                     // one k-step (16) of a slab
    bf16x8 ah[2], al[2], bh[2], bl[2];              // bf16 modes: operands pre-split in LDS
    f32x4 a32[2][2], b32[2][2];                     // f32 mode: lane (row, kg) holds k = 16 kg + 8 t + 0..7
  };
  const int fcb = kg * 4;
  auto load = [&](Frag& f, const float* st, int t) {
    if constexpr (PREC == PREC_F32) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int pc = ((fcb + 2 * t + g) ^ fsw) * 4;
#pragma unroll
        for (int a = 0; a < 2; ++a) f.a32[a][g] = *(const f32x4*)(st + (a_row0 + a * 32) * 32 + pc);
#pragma unroll
        for (int b = 0; b < 2; ++b) f.b32[b][g] = *(const f32x4*)(st + (b_row0 + b * 32) * 32 + pc);
      }
      return;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f.ah[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
      if constexpr (prec_x3(PREC) || prec_x2(PREC) || PREC == PREC_F16) f.al[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      f.bh[b] = *(const bf16x8*)(st + (b_row0 + b * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
      if constexpr (prec_x3(PREC) || PREC == PREC_F16) f.bl[b] = *(const bf16x8*)(st + (b_row0 + b * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
    }
  };
  auto mma = [&](const Frag& f) {
    if constexpr (PREC == PREC_F32) {
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a32[a][g][e], f.b32[b][g][e], acc[a][b], 0, 0, 0);
      return;
    }
    split_mma16<PREC>(acc, f.ah, f.al, f.bh, f.bl);
  };
  constexpr int NREAD = PREC == PREC_BF16 ? 4 : (prec_x2(PREC) ? 6 : 8);          // ds_read_b128 per k-step
  constexpr int NMMA = PREC == PREC_F32 ? 32 : (prec_x3(PREC) ? 12 : ((PREC == PREC_F16 || prec_x2(PREC)) ? 8 : 4));         // MFMAs per k-step
  Frag F0, F1;
  if (wave == 0) TA_STAMP(1);                       // consumer: set up, waiting for slab 0
  __builtin_amdgcn_s_barrier();                     // B_0: slab 0 visible
  asm volatile("" ::: "memory");
  if (wave == 0) TA_STAMP(2);                       // consumer: slab 0 landed
  if constexpr (STAGES == 2) {
    // one fragment set: the other workgroup's consumer on this SIMD covers the read latency
    for (int s = 0; s < S; ++s) {
      const float* st = lds + (s & 1) * STAGE;
      load(F0, st, 0);
      mma(F0);
      load(F0, st, 1);
      mma(F0);
      if (s + 1 < S) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();               // B_{s+1}
        asm volatile("" ::: "memory");
      }
    }
  } else {
  load(F0, lds + stage * STAGE, 0);
  for (int s = 0; s + 1 < S; ++s) {                 // branch-free body; the last slab is peeled below
    const float* st = lds + stage * STAGE;
    stage = stage + 1 == STAGES ? 0 : stage + 1;
    __builtin_amdgcn_sched_barrier(0);
    load(F1, st, 1);                                // second k-step of slab s under the MFMAs of the first
    mma(F0);
    split_pin<NREAD, NMMA>();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every fragment of slab s is in registers
    __builtin_amdgcn_s_barrier();                          // B_{s+1}: slab s+1 visible, stage of slab s handed back
    asm volatile("" ::: "memory");
    load(F0, lds + stage * STAGE, 0);               // first k-step of slab s+1 under the MFMAs of the second
    mma(F1);
    split_pin<NREAD, NMMA>();
    __builtin_amdgcn_sched_barrier(0);
  }
  load(F1, lds + stage * STAGE, 1);
  stage = stage + 1 == STAGES ? 0 : stage + 1;
  mma(F0);
  mma(F1);
  }
  if (wave == 0) TA_STAMP(3);                       // consumer: main loop done (last MFMAs issued)
  {
    __builtin_amdgcn_s_barrier();                   // E0: every consumer has its last fragments: the ring can be reused
    asm volatile("" ::: "memory");
    if (wave == 0) TA_STAMP(5);                     // consumer: past E0
    conv_epilogue_park<BN>(acc, lds, cm, cn, lane);
    if (wave == 0) TA_STAMP(6);                     // consumer: accumulators parked (LDS writes issued)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // ... and executed: a raw s_barrier does not wait for them
    __builtin_amdgcn_s_barrier();                   // E1: tile parked
    asm volatile("" ::: "memory");
    if (wave == 0) TA_STAMP(7);                     // consumer: past E1
    bool done = false;
    if constexpr (PREC != PREC_F32) done = conv_drain_dispatch<BN, BM, 64 * (NC + NP), (PREC == PREC_F16 ? 2 : (prec_half(PREC) ? 1 : 0))>(p, lds, ct0, pt0, tid, HoWo);
    if (!done) conv_epilogue_drain<BN, BM, 64 * (NC + NP)>(p, lds, ct0, pt0, tid, HoWo, ks);
  }
  if (wave == 0) TA_STAMP(4);                       // consumer: epilogue stores issued
}

// ---- split-role kernel with a WINDOW-RESIDENT pixel operand (3x3 / 7x7 stride-1 convs on pre-split half-float tensors) --------
// conv_igemm_split streams both operands per K slab: over the kh x kw taps of one channel block the same input pixels are
// fetched kh x kw times from L2 into LDS (each time shifted by one tap).  Here the pixel operand of a channel block is loaded
// ONCE: the tile's BM pixels are consecutive interior pixels in raster order, so every tap of every one of them lies inside
// one contiguous run of the padded tensor -- from the first pixel's tap (0, 0) to the last pixel's tap (kh-1, kw-1), halo
// rows and, where a tile crosses into the next image, the halo rows between the images included.  That run (<= PR pixel rows
// of 128 bytes: one 32-channel block, [hi x32 | lo x32]) is the PATCH.  Producers DMA patch cb + 1 into the second patch
// buffer while the kh x kw slabs of block cb are consumed; per slab only the weight rows stream (BN x 128 bytes instead of
// (BN + BM) x 128).  A consumer lane keeps the patch row of its two pixels and reads tap (ky, kx) at row + ky * Wp + kx -- the
// same XOR swizzle on the row index, so the fragment reads stay conflict-free (16 consecutive rows per quarter wave).
// K order, MFMA order and epilogue are conv_igemm_split's: a layer's bits do not depend on which of the two kernels runs it.
// L2 -> LDS bytes per tile and channel block: kh kw BN 128 + ~1.5 BM 128 instead of kh kw (BN + BM) 128 (3x3, 128 x 128:
// 172 KiB instead of 288; the embedder's two-product mode is bound by exactly this stream).
template <int CM, int CN, int PREC, int PR>
__global__ __launch_bounds__(64 * (CM * CN + 4), (CM * CN + 4) / 4) void conv_igemm_win(const ta_conv_launch p) {
  static_assert(prec_half(PREC) && PREC != PREC_F16, "pre-split half-float tensors (f16x3 / f16x2)");
  static_assert(CM * CN == 4 || CM * CN == 8, "consumer grid: 1x4 (64 cout x 256 px), 2x2 (128 x 128) or 2x4 (128 x 256)");
  static_assert(PR % 32 == 0, "whole DMA instructions per producer wave");
  constexpr int NC = CM * CN, NP = 4;
  constexpr int BN = CM * 64, BM = CN * 64;
  constexpr int QA = BN / 8 / NP;                // weight-row DMA instructions per producer wave per slab
  constexpr int NPW = PR / 8 / NP;               // patch DMA instructions per producer wave per channel block
  constexpr int A_STAGE = BN * 32;               // floats per weight stage (3 stages)
  constexpr int PATCH = PR * 32;                 // floats per patch buffer (2 buffers)
  static_assert(QA + NPW < 64, "s_waitcnt vmcnt is a 6-bit count");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const patch0 = lds + 3 * A_STAGE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_ct = p.coutp / BN;
  const int n_pt = (p.M + BM - 1) / BM;
  const int bid = blockIdx.x;
  const int grp = bid >> 3, xcd = bid & 7;
  const int gq = ta_div_r(grp, n_ct, p.r_nct, p.fast_div);
  const int pt = ta_xcd_tile(n_pt, xcd, gq);
  if (pt < 0) return;
  const int ct0 = (grp - gq * n_ct) * BN;
  const int pt0 = pt * BM;
  const int HoWo = p.Ho * p.Wo;
  const int S = p.n_slabs;
  const int T = p.k_w * p.k_h;                   // slabs per channel block
  if (wave == 0) TA_STAMP(0);                       // consumer entry (tile decoded)
  if (wave == NC) TA_STAMP(8);                      // producer entry
  // padded-raster index of a pixel's tap (0, 0) relative to the tile's first pixel: the patch row it reads at that tap
  const ta_pixel_walk walk(p, pt0, HoWo);
  const int wp = p.win_wp, wimg = p.win_img;    // pixels per padded row / per padded image (launcher)

  if (wave >= NC) {
    // ================= producer =================
    const int pw = wave - NC;
    const int pchunk = lane & 7;
    const int lchunk = pchunk ^ ((4 * (pw & 1) + (lane >> 4)) & 7);
    const char* a_base = (const char*)p.w;
    const size_t a_slab_bytes = (size_t)p.coutp * 128;
    unsigned a_off[QA];
#pragma unroll
    for (int q = 0; q < QA; ++q) a_off[q] = (unsigned)(((ct0 + (q * NP + pw) * 8 + (lane >> 3)) * 32 + lchunk * 4) * 4);
    ta_k_walk wa(p, 0);
    auto issue_a = [&](int stage) {
#pragma unroll
      for (int q = 0; q < QA; ++q) ta_dma16(a_base + (size_t)wa.a_slab * a_slab_bytes, a_off[q], lds + stage * A_STAGE + (q * NP + pw) * 256);
      wa.advance();
    };
    issue_a(0);                                     // needs no pixel arithmetic: moving first
    // the patch: rows 0 .. n_patch - 1 of the padded tensor from the first pixel's tap (0, 0) on
    const int last = (p.M - pt0 < BM ? p.M - pt0 : BM) - 1;
    int img1, y1, x1;
    walk.at(last, img1, y1, x1);
    const int n_patch = (img1 - walk.img0) * wimg + (y1 - walk.y0) * wp + (x1 - walk.x0) + (p.k_h - 1) * wp + p.k_w;
    const int in_ch = p.in_ch_off + (p.group_cout ? (ct0 / p.group_cout) * p.group_cin : 0);
    const size_t off0 = (size_t)walk.img0 * p.in_img + (size_t)walk.y0 * p.in_row + (size_t)walk.x0 * p.in_pix + p.in_off0 + in_ch;
    const char* b_base = (const char*)(p.in + off0);
    unsigned p_off[NPW];
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int r = (i * NP + pw) * 8 + (lane >> 3);                      // LDS row; rows past the patch re-read its last row
      const int rr = r < n_patch ? r : n_patch - 1;
      p_off[i] = (unsigned)rr * (unsigned)(p.in_pix * 4) + (unsigned)(lchunk * 16);
    }
    auto issue_patch = [&](int cb) {
      float* dst = patch0 + (cb & 1) * PATCH;
#pragma unroll
      for (int i = 0; i < NPW; ++i) ta_dma16(b_base + (size_t)cb * 128, p_off[i], dst + (i * NP + pw) * 256);
    };
    if (wave == NC) TA_STAMP(9);                    // producer: addresses ready, first weight rows issued
    issue_patch(0);
    if (S > 1) issue_a(1);
    if (wave == NC) TA_STAMP(10);                   // producer: patch 0 + second weight slab issued
    int stage = 2, t = 0, cb = 0;
    bool patch_behind = false;                      // a patch was issued right after the previous barrier
    for (int g = 0; g < S; ++g) {
      // vmcnt counts in issue order: [A0 P0 A1], then per barrier [P(cb+1) if tap 0] A(g+2).  Slab g's weight rows must have
      // landed; what may stay in flight is the next slab's rows and a patch issued behind slab g's rows
      const bool more = g + 1 < S;
      if (patch_behind) {
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA + NPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory");
      } else {
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();                 // B_g: slab g (and, at tap 0, its patch) landed; consumers drained slab g-1
      asm volatile("" ::: "memory");
      patch_behind = false;
      if (t == 0 && cb + 1 < p.k_cblocks) {         // the other patch buffer was last read by block cb-1: free since this barrier
        issue_patch(cb + 1);
        patch_behind = true;
      }
      if (g + 2 < S) {
        issue_a(stage);
        stage = stage == 2 ? 0 : stage + 1;
      }
      if (++t == T) {
        t = 0;
        ++cb;
      }
    }
    // (a patch is never left in flight here: the last block issues none)
    {                                               // help drain the parked tile: twice the lanes for the epilogue math
      __builtin_amdgcn_s_barrier();                 // E0
      __builtin_amdgcn_s_barrier();                 // E1
      asm volatile("" ::: "memory");
      if (!conv_drain_dispatch<BN, BM, 64 * (NC + NP), 1>(p, lds, ct0, pt0, tid, HoWo))
        conv_epilogue_drain<BN, BM, 64 * (NC + NP)>(p, lds, ct0, pt0, tid, HoWo, 0);
    }
    return;
  }

  // ================= consumer =================
  const int cm = wave / CN, cn = wave % CN;
  f32x16 acc[2][2];
  split_acc_clear(acc);
  const int frow = lane & 31;
  const int fsw = (frow >> 1) & 7;
  const int kg = lane >> 5;
  const int a_row0 = cm * 64 + frow;
  int rB[2];                                        // patch row of this lane's two pixels at tap (0, 0)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int d = cn * 64 + b * 32 + frow;
    int img, y, x;
    walk.at(pt0 + d < p.M ? d : 0, img, y, x);     // pixels past M: the tile's first pixel (their stores are masked)
    rB[b] = (img - walk.img0) * wimg + (y - walk.y0) * wp + (x - walk.x0);
  }
  struct Frag {
    bf16x8 ah[2], al[2], bh[2], bl[2];
  };
  unsigned pb[2];                                   // byte offset (inside the patch buffers) of this slab's B rows, k-step 0, hi words
  auto baddr = [&](int tap_off, int buf) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const unsigned row = (unsigned)(rB[b] + tap_off);
      pb[b] = (unsigned)buf * (unsigned)(PATCH * 4) + row * 128u + ((((unsigned)(2 * kg)) ^ ((row >> 1) & 7u)) << 4);
    }
  };
  auto load = [&](Frag& f, const float* st, int t) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f.ah[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((2 * kg + t) ^ fsw) * 4);
      f.al[a] = *(const bf16x8*)(st + (a_row0 + a * 32) * 32 + ((4 + 2 * kg + t) ^ fsw) * 4);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const char* q = (const char*)patch0 + (pb[b] ^ (unsigned)(t << 4));      // chunk 2 kg + t: bit 0 of the chunk index
      f.bh[b] = *(const bf16x8*)q;
      if constexpr (prec_x3(PREC)) f.bl[b] = *(const bf16x8*)((const char*)patch0 + ((pb[b] ^ (unsigned)(t << 4)) ^ 64u));   // + 4 chunks: the lo words
    }
  };
  auto mma = [&](const Frag& f) { split_mma16<PREC>(acc, f.ah, f.al, f.bh, f.bl); };
  constexpr int NREAD = prec_x3(PREC) ? 8 : 6;
  constexpr int NMMA = prec_x3(PREC) ? 12 : 8;
  // K walk of the consumer side (scalar): tap offset inside the patch and the patch buffer of the slab being read
  int kx = 0, ky = 0, cb = 0, tap_off = 0, stage = 0;
  Frag F0, F1;
  baddr(0, 0);
  if (wave == 0) TA_STAMP(1);                       // consumer: set up, waiting for slab 0
  __builtin_amdgcn_s_barrier();                     // B_0
  asm volatile("" ::: "memory");
  if (wave == 0) TA_STAMP(2);                       // consumer: slab 0 + patch 0 landed
  load(F0, lds, 0);
  for (int g = 0; g + 1 < S; ++g) {
    const float* st = lds + stage * A_STAGE;
    stage = stage == 2 ? 0 : stage + 1;
    __builtin_amdgcn_sched_barrier(0);
    load(F1, st, 1);
    mma(F0);
    split_pin<NREAD, NMMA>();
    __builtin_amdgcn_sched_barrier(0);
    // the next slab's tap (scalar walk) and its B addresses, while the reads of this slab return
    if (++kx == p.k_w) {
      kx = 0;
      tap_off += wp - p.k_w;
      if (++ky == p.k_h) {
        ky = 0;
        ++cb;
        tap_off = -1;
      }
    }
    ++tap_off;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every fragment of slab g is in registers
    baddr(tap_off, cb & 1);
    __builtin_amdgcn_s_barrier();                          // B_{g+1}
    asm volatile("" ::: "memory");
    load(F0, lds + stage * A_STAGE, 0);
    mma(F1);
    split_pin<NREAD, NMMA>();
    __builtin_amdgcn_sched_barrier(0);
  }
  load(F1, lds + stage * A_STAGE, 1);
  mma(F0);
  mma(F1);
  if (wave == 0) TA_STAMP(3);                       // consumer: main loop done (last MFMAs issued)
  {
    __builtin_amdgcn_s_barrier();                   // E0: every consumer has its last fragments: the ring can be reused
    asm volatile("" ::: "memory");
    if (wave == 0) TA_STAMP(5);                     // consumer: past E0
    conv_epilogue_park<BN>(acc, lds, cm, cn, lane);
    if (wave == 0) TA_STAMP(6);                     // consumer: accumulators parked (LDS writes issued)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // ... and executed: a raw s_barrier does not wait for them
    __builtin_amdgcn_s_barrier();                   // E1: tile parked
    asm volatile("" ::: "memory");
    if (wave == 0) TA_STAMP(7);                     // consumer: past E1
    if (!conv_drain_dispatch<BN, BM, 64 * (NC + NP), 1>(p, lds, ct0, pt0, tid, HoWo))
      conv_epilogue_drain<BN, BM, 64 * (NC + NP)>(p, lds, ct0, pt0, tid, HoWo, 0);
  }
  if (wave == 0) TA_STAMP(4);                       // consumer: epilogue stores issued
}

// Fills what the launcher of a split-role kernel owes the kernel: the reciprocals of the launch-uniform divisors, fast_div and
// fast_drain.  `lean_ok`: the mode and the launch have a lean drain at all (not the f32 mode, no K ranges); `split_fmt`: the
// mode's pre-split tensor format.  q.k_split is final here.
static void split_launch_facts(ta_ctx* ctx, ta_conv_launch& q, const ta_tile_grid& g, int BM, int split_fmt, bool lean_ok) {
  q.r_nct = 1.0f / (float)g.n_ct;
  q.r_tile_blocks = 1.0f / (float)(g.groups * 8);
  q.r_Wo = 1.0f / (float)q.Wo;
  q.r_Ho = 1.0f / (float)q.Ho;
  q.r_HoWo = 1.0f / (float)(q.Ho * q.Wo);
  // division-free set-up: every dividend (block index, pixel index) below 2^24, where the float32 reciprocal is exact to +-1
  const long long grid = (long long)g.groups * 8 * q.k_split;
  q.fast_div = (grid < (1 << 24) && (long long)q.M + BM < (1 << 24)) ? 1 : 0;
  // lean epilogue: split-format tensors whose byte offsets fit 32 bits, channel slices on 8-channel boundaries
  const long long n_img = q.Ho * q.Wo > 0 ? ((long long)q.M + q.Ho * q.Wo - 1) / (q.Ho * q.Wo) : 0;
  auto fits = [&](long long img_stride, int off0) { return ((n_img + 1) * img_stride + off0) * 4 < (1LL << 32); };
  bool ok = lean_ok && q.out_fmt == split_fmt && (q.cout & 7) == 0 && ((q.out_ch | q.res_ch | q.o2_ch) & 7) == 0 && fits(q.out_img, q.out_off0);
  if (q.res) ok = ok && q.res_fmt == split_fmt && fits(q.res_img, q.res_off0);
  if (q.out2) ok = ok && q.o2_fmt == split_fmt && fits(q.o2_img, q.o2_off0);
  // ... and one of the shapes conv_drain_dispatch is compiled for: every other launch takes the generic drain and is not counted
  const bool plain = !q.res && !q.out2;
  ok = ok && (q.pool ? (plain && q.act == TA_ACT_RELU) : (q.bias9 ? (plain && q.act == TA_ACT_PRELU) : (plain || (q.res && q.act == TA_ACT_NONE))));
  q.fast_drain = ok ? 1 : 0;
  if (ok) ctx->conv_counts[TA_CV_COUNT - 1] += 1;     // slot 15: launches whose epilogue ran the specialised drain
}

template <int CM, int CN, int NP, int PREC, int STAGES>
static int launch_split(ta_ctx* ctx, const ta_conv_launch& p) {
  constexpr int BN = CM * 64, BM = CN * 64;
  const ta_tile_grid g(p, BN, BM);
  const size_t lds_bytes = (size_t)STAGES * (BN + BM) * 32 * sizeof(float);
  auto kern = conv_igemm_split<CM, CN, NP, PREC, STAGES>;
  TA_SET_LDS_ATTR(ctx, kern, lds_bytes);
  ta_conv_launch q = p;
  constexpr int SPLIT_FMT = PREC == PREC_F16 ? TA_FMT_F16 : (prec_half(PREC) ? TA_FMT_SPLIT16 : TA_FMT_SPLIT);
  split_launch_facts(ctx, q, g, BM, SPLIT_FMT, PREC != PREC_F32 && p.k_split == 1);
  TA_NOTE_KERNEL(ctx, "conv_igemm_split<%d,%d,%d,%d,%d>", CM, CN, NP, PREC, STAGES);
  hipLaunchKernelGGL(kern, dim3(g.groups * 8 * p.k_split), dim3(64 * (CM * CN + NP)), lds_bytes, ctx->stream, q);
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}

template <int CM, int CN, int PREC, int PR>
static int launch_win(ta_ctx* ctx, const ta_conv_launch& p) {
  constexpr int BN = CM * 64, BM = CN * 64;
  const ta_tile_grid g(p, BN, BM);
  constexpr size_t ring = (size_t)(3 * BN + 2 * PR) * 128, park = (size_t)BM * BN * 4;
  constexpr size_t lds_bytes = ring > park ? ring : park;
  static_assert(lds_bytes <= 160 * 1024, "one workgroup's LDS");
  auto kern = conv_igemm_win<CM, CN, PREC, PR>;
  TA_SET_LDS_ATTR(ctx, kern, lds_bytes);
  ta_conv_launch q = p;
  q.k_split = 1;
  split_launch_facts(ctx, q, g, BM, TA_FMT_SPLIT16, true);
  TA_NOTE_KERNEL(ctx, "conv_igemm_win<%d,%d,%d,%d>", CM, CN, PREC, PR);
  hipLaunchKernelGGL(kern, dim3(g.groups * 8), dim3(64 * (CM * CN + 4)), lds_bytes, ctx->stream, q);
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}

template <int PREC>
static int launch_split_variant(ta_ctx* ctx, int v, const ta_conv_launch& p) {
  switch (v) {
    case TA_CV_SPLIT_2x2: return launch_split<2, 2, 4, PREC, 3>(ctx, p);
    case TA_CV_SPLIT_2x2_P8: return launch_split<2, 2, 8, PREC, 3>(ctx, p);
    case TA_CV_SPLIT_2x4: return launch_split<2, 4, 4, PREC, 3>(ctx, p);
    case TA_CV_SPLIT_1x4: return launch_split<1, 4, 4, PREC, 3>(ctx, p);
    case TA_CV_SPLIT_1x4_W2: return launch_split<1, 4, 4, PREC, 2>(ctx, p);
    case TA_CV_SPLIT_2x2_W2: return launch_split<2, 2, 4, PREC, 2>(ctx, p);
    case TA_CV_WIN_2x2:
    case TA_CV_WIN_2x4:
    case TA_CV_WIN_1x4:
      if constexpr (PREC == PREC_F16X3 || PREC == PREC_F16X2) {
        if (v == TA_CV_WIN_2x2) return launch_win<2, 2, PREC, TA_WIN_PR_2x2>(ctx, p);
        if (v == TA_CV_WIN_2x4) return launch_win<2, 4, PREC, TA_WIN_PR_2x4>(ctx, p);
        return launch_win<1, 4, PREC, TA_WIN_PR_1x4>(ctx, p);
      }
      break;
  }
  return ta_fail(ctx, TA_E_INVALID, "conv: unknown kernel variant %d", v);
}
