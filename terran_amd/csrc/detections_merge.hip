// Detections of many tiles -> detections of their frames (ta_detections_merge): the tail of tiled detection.
//
//  map     every coordinate v of a candidate's box and landmarks becomes v / zoom + origin of its group (one correctly
//          rounded division, one addition, float32)
//  edge    a candidate whose mapped box comes within `edge` pixels of an interior side of its group's rectangle is dropped
//  order   per frame: descending score, equal scores by ascending candidate row
//  NMS     greedy over that order, suppress iff ovr > nms_thr; ovr = inter / (area_a + area_b - inter), or
//          inter / fminf(area_a, area_b) -- the operation order of rf_select_kernel and oracle.retinaface_post.nms
//
// A crowd frame cut in 30-odd tiles brings thousands of candidates: nothing here is one workgroup's job but the last walk.
//  1. dm_map_kernel     a thread per candidate: map, edge rule, and the survivors' 64-bit keys (score descending | row)
//                       appended to their frame's list (atomic counter, one addition per wave and frame: the order of the list is arbitrary, the keys are
//                       distinct, so the ranks below are not)
//  2. dm_rank_kernel    the sort, by counting: rank of key i = number of keys of its frame below it; 256 keys per workgroup
//                       against the frame's list staged through LDS 256 at a time.  The same n^2 / 256 workgroups of work
//                       as the matrix, and no power-of-two padding or LDS limit.  Leaves the frame's rows and mapped boxes
//                       in order.
//  3. dm_matrix_kernel  the suppression bit matrix, as rf_select_kernel's fast path builds it, but in the context's scratch
//                       block and by a workgroup per 64 x 64 block of pairs (i, j >= i's block): lane = candidate j, a
//                       wave walks 16 rows i, the ballot is the row's word.  Only words at or behind a row's own block
//                       are ever written -- or read.
//  4. dm_scan_kernel    one wave per frame walks the order a block of 64 at a time: the block's own column decides its 64
//                       candidates on scalars (readlane), then the rows of the kept ones are ORed into the removed set,
//                       lane l holding words l, l + 64, ...; sixteen rows' loads are in flight together.
//  5. dm_gather_kernel  kept candidates -> packed outputs.
// Frames are independent; the matrix of a call is cut in batches of frames that fit DM_MATRIX_BYTES of scratch.
//
// Compiled with -ffp-contract=off (build.py): every float step is single-rounded, the decisions are bit-exact with the
// numpy model in tests/tiles_model.py.  Scores and coordinates must be finite (NaN keys have no defined place).
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <vector>

#include "frame_regions.h"

#define DM_MAX_PER_FRAME 16384                    // candidates of one frame: 256 words per matrix row, 4 per lane of the scan
#define DM_SCAN_K (DM_MAX_PER_FRAME / 64 / 64)
#define DM_MATRIX_BYTES ((size_t)256 << 20)       // scratch the matrices of one batch of frames may take (one frame at the limit: 32 MiB)
#define DM_SCAN_UNROLL 16

namespace {

struct dm_frame {
  int32_t off;          // first slot of the frame in the per-frame arrays (keys, rows, boxes in order, kept rows)
  int32_t cap;          // candidates of its groups: what the slots hold at most
  int32_t wstride;      // 64-bit words per matrix row
  int32_t out_base;     // first output slot (filled in behind the scan)
  uint64_t moff;        // first word of its matrix within its batch's block
};

typedef unsigned long long dm_u64;

__device__ __forceinline__ dm_u64 dm_readlane64(dm_u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((dm_u64)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void dm_map_kernel(const ta_merge_group* __restrict__ groups, const int32_t* __restrict__ gidx, const float4* __restrict__ boxes,
                                                     const float2* __restrict__ lmks, const float* __restrict__ scores, int C, float edge,
                                                     const dm_frame* __restrict__ frames, float4* __restrict__ mboxes, float2* __restrict__ mlmks,
                                                     dm_u64* __restrict__ ukeys, int* cnt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int g = gidx[c];
  if (g < 0) return;
  const ta_merge_group G = groups[g];
  const float4 b = boxes[c];
  float4 m;
  m.x = __fadd_rn(__fdiv_rn(b.x, G.zoom), G.ox);
  m.y = __fadd_rn(__fdiv_rn(b.y, G.zoom), G.oy);
  m.z = __fadd_rn(__fdiv_rn(b.z, G.zoom), G.ox);
  m.w = __fadd_rn(__fdiv_rn(b.w, G.zoom), G.oy);
  mboxes[c] = m;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float2 l = lmks[(size_t)c * 5 + k];
    mlmks[(size_t)c * 5 + k] = make_float2(__fadd_rn(__fdiv_rn(l.x, G.zoom), G.ox), __fadd_rn(__fdiv_rn(l.y, G.zoom), G.oy));
  }
  if (edge > 0.f) {
    bool cut = false;
    cut |= (G.interior & 1) && m.x < __fadd_rn(G.x0, edge);
    cut |= (G.interior & 2) && m.y < __fadd_rn(G.y0, edge);
    cut |= (G.interior & 4) && m.z > __fsub_rn(G.x1, edge);
    cut |= (G.interior & 8) && m.w > __fsub_rn(G.y1, edge);
    if (cut) return;
  }
  // ascending key == descending score, then ascending row; -0 counts as +0
  const unsigned u = __float_as_uint(__fadd_rn(scores[c], 0.0f));
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const dm_frame F = frames[G.frame];
  // one atomic per frame and wave, not per candidate (thousands on one address otherwise): the lanes that append to the frame
  // of the first lane still waiting take consecutive slots behind one addition, then leave the loop
  const int lane = threadIdx.x & 63;
  int pos = 0;
  for (;;) {
    const int lead_frame = __builtin_amdgcn_readfirstlane(G.frame);
    const dm_u64 peers = __ballot(G.frame == lead_frame);
    if (G.frame == lead_frame) {
      const int lead = __ffsll((long long)peers) - 1;
      int base = 0;
      if (lane == lead) base = atomicAdd(&cnt[lead_frame], __popcll(peers));
      base = __shfl(base, lead);
      pos = base + __popcll(peers & ((1ull << lane) - 1ull));   // < F.cap: the frame's groups hold F.cap candidates in all
      break;
    }
  }
  ukeys[(size_t)F.off + pos] = ((dm_u64)(~ord) << 32) | (unsigned)c;
}

// grid (blocks of 256 keys, frames of the batch)
__global__ __launch_bounds__(256) void dm_rank_kernel(const dm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const dm_u64* __restrict__ ukeys,
                                                      const float4* __restrict__ mboxes, int32_t* __restrict__ srow, float4* __restrict__ sbox) {
  __shared__ dm_u64 tile[256];
  const int f = f0 + blockIdx.y;
  const int n = cnt[f];
  if ((int)blockIdx.x * 256 >= n) return;            // uniform
  const dm_u64* keys = ukeys + frames[f].off;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const dm_u64 key = i < n ? keys[i] : ~0ull;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    tile[threadIdx.x] = j0 + (int)threadIdx.x < n ? keys[j0 + threadIdx.x] : ~0ull;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) rank += tile[k] < key;
    __syncthreads();
  }
  if (i < n) {
    const int row = (int)(unsigned)key;
    srow[(size_t)frames[f].off + rank] = row;
    sbox[(size_t)frames[f].off + rank] = mboxes[row];
  }
}

// grid (blocks of 64 x 64 pairs of the largest frame, frames of the batch)
__global__ __launch_bounds__(256) void dm_matrix_kernel(const dm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const float4* __restrict__ sbox,
                                                        float nms_thr, int metric, dm_u64* __restrict__ mat) {
  const int f = f0 + blockIdx.y;
  const int n = cnt[f];
  const int nb = (n + 63) >> 6;
  int p = blockIdx.x, I = 0;
  if ((long long)p >= (long long)nb * (nb + 1) / 2) return;
  while (p >= nb - I) {                               // pairs (0,0) (0,1) .. (0,nb-1) (1,1) ..
    p -= nb - I;
    ++I;
  }
  const int J = I + p;
  const dm_frame F = frames[f];
  const float4* box = sbox + F.off;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = J * 64 + lane;
  const float4 b = j < n ? box[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float area_b = (b.z - b.x) * (b.w - b.y);
  dm_u64 mine = 0;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int i = I * 64 + wv * 16 + k;               // uniform in the wave
    bool sup = false;
    if (i < n) {
      const float4 a = box[i];
      if (j > i && j < n) {
        const float area = (a.z - a.x) * (a.w - a.y);
        const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
        const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
        const float iw = fmaxf(0.0f, xx2 - xx1), ih = fmaxf(0.0f, yy2 - yy1);
        const float inter = iw * ih;
        const float ovr = metric ? __fdiv_rn(inter, fminf(area, area_b)) : __fdiv_rn(inter, area + area_b - inter);
        sup = ovr > nms_thr;
      }
    }
    const dm_u64 m = __ballot(sup);
    if (lane == k) mine = m;
  }
  const int i = I * 64 + wv * 16 + lane;
  if (lane < 16 && i < n) mat[F.moff + (size_t)i * F.wstride + J] = mine;
}

// one wave per frame of the batch
__global__ __launch_bounds__(64) void dm_scan_kernel(const dm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const int32_t* __restrict__ srow,
                                                     const dm_u64* __restrict__ mat, int32_t* __restrict__ krow, int* __restrict__ kcnt) {
  const int f = f0 + blockIdx.x;
  const int n = cnt[f];
  const dm_frame F = frames[f];
  const int lane = threadIdx.x;
  const int W = (n + 63) >> 6, K = (W + 63) >> 6;
  const dm_u64* M = mat + F.moff;
  const size_t ws = (size_t)F.wstride;
  dm_u64 removed[DM_SCAN_K];                          // lane l: words l + 64 k of the removed set
#pragma unroll
  for (int k = 0; k < DM_SCAN_K; ++k) removed[k] = 0;
  int kept = 0;
  for (int w = 0; w < W; ++w) {
    const int i0 = w * 64, nn = n - i0 < 64 ? n - i0 : 64;
    const int row = i0 + lane;
    const dm_u64 own = lane < nn ? M[(size_t)row * ws + w] : 0ull;   // the block's own column: the first word a row has
    dm_u64 sel = removed[0];
#pragma unroll
    for (int k = 1; k < DM_SCAN_K; ++k) sel = (w >> 6) == k ? removed[k] : sel;
    dm_u64 cur = dm_readlane64(sel, w & 63);
    dm_u64 keptbits = 0;
    for (int i = 0; i < nn; ++i) {
      if ((cur >> i) & 1ull) continue;
      keptbits |= 1ull << i;
      cur |= dm_readlane64(own, i);
    }
    if ((keptbits >> lane) & 1ull) krow[(size_t)F.off + kept + __popcll(keptbits & ((1ull << lane) - 1ull))] = srow[(size_t)F.off + row];
    kept += __popcll(keptbits);
    if (w + 1 == W) break;
    // the kept rows' words behind this block, DM_SCAN_UNROLL rows at a time
    dm_u64 kb = keptbits;
    while (kb) {
      int r[DM_SCAN_UNROLL];
#pragma unroll
      for (int u = 0; u < DM_SCAN_UNROLL; ++u) {
        r[u] = kb ? i0 + __builtin_ctzll(kb) : -1;
        kb &= kb - 1;                                 // 0 stays 0
      }
#pragma unroll
      for (int k = 0; k < DM_SCAN_K; ++k) {
        if (k >= K) break;                            // uniform
        const int wd = lane + 64 * k;
        const bool live = wd > w && wd < W;
        dm_u64 v[DM_SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < DM_SCAN_UNROLL; ++u) v[u] = (live && r[u] >= 0) ? M[(size_t)r[u] * ws + wd] : 0ull;
#pragma unroll
        for (int u = 0; u < DM_SCAN_UNROLL; ++u) removed[k] |= v[u];
      }
    }
  }
  if (lane == 0) kcnt[f] = kept;
}

// one workgroup per frame
__global__ __launch_bounds__(256) void dm_gather_kernel(const dm_frame* __restrict__ frames, const int* __restrict__ kcnt, const int32_t* __restrict__ krow,
                                                        const float4* __restrict__ mboxes, const float2* __restrict__ mlmks, const float* __restrict__ scores,
                                                        float4* __restrict__ o_boxes, float2* __restrict__ o_lmks, float* __restrict__ o_scores,
                                                        int32_t* __restrict__ o_source) {
  const dm_frame F = frames[blockIdx.x];
  const int K = kcnt[blockIdx.x];
  for (int k = threadIdx.x; k < K; k += 256) {
    const int row = krow[(size_t)F.off + k];
    const size_t o = (size_t)F.out_base + k;
    o_boxes[o] = mboxes[row];
#pragma unroll
    for (int e = 0; e < 5; ++e) o_lmks[o * 5 + e] = mlmks[(size_t)row * 5 + e];
    o_scores[o] = scores[row];
    o_source[o] = row;
  }
}

}  // namespace

extern "C" int ta_detections_merge(ta_ctx* ctx, const ta_merge_group* groups, int n_groups, int n_frames, const float* boxes, const float* landmarks,
                                   const float* scores, int n_candidates, float nms_thr, int metric, float edge, int capacity, int32_t* counts,
                                   float* out_boxes, float* out_landmarks, float* out_scores, int32_t* out_source, int32_t* required) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (required) *required = 0;
  if (n_groups < 0 || n_frames < 0 || n_candidates < 0 || (n_groups > 0 && !groups) || (n_frames > 0 && !counts))
    return ta_fail(ctx, TA_E_INVALID, "detections_merge: bad args");
  if (n_candidates > 0 && (!boxes || !landmarks || !scores)) return ta_fail(ctx, TA_E_INVALID, "detections_merge: null candidate arrays");
  if (metric != 0 && metric != 1) return ta_fail(ctx, TA_E_INVALID, "detections_merge: metric %d is neither 0 (IoU) nor 1 (IoS)", metric);
  if (!(edge >= 0.f) || !std::isfinite(edge) || !std::isfinite(nms_thr)) return ta_fail(ctx, TA_E_INVALID, "detections_merge: edge %g, nms_thr %g", (double)edge, (double)nms_thr);
  if (capacity > 0 && (!out_boxes || !out_landmarks || !out_scores || !out_source)) return ta_fail(ctx, TA_E_INVALID, "detections_merge: null outputs");
  for (int f = 0; f < n_frames; ++f) counts[f] = 0;

  // the groups: sorted by frame, rows inside the candidate arrays, no row in two groups
  std::vector<int32_t> gidx((size_t)n_candidates, -1);
  std::vector<dm_frame> fr((size_t)n_frames);
  for (dm_frame& F : fr) memset(&F, 0, sizeof(F));
  for (int g = 0; g < n_groups; ++g) {
    const ta_merge_group& G = groups[g];
    if (G.frame < 0 || G.frame >= n_frames) return ta_fail(ctx, TA_E_INVALID, "detections_merge: group %d: frame %d out of range [0, %d)", g, G.frame, n_frames);
    if (g > 0 && G.frame < groups[g - 1].frame) return ta_fail(ctx, TA_E_INVALID, "detections_merge: group %d: the groups are not sorted by frame", g);
    if (G.first < 0 || G.count < 0 || (long long)G.first + G.count > n_candidates)
      return ta_fail(ctx, TA_E_INVALID, "detections_merge: group %d: rows %d .. %lld are not inside the %d candidates", g, G.first, (long long)G.first + G.count - 1, n_candidates);
    if (!(G.zoom > 0.f) || !std::isfinite(G.zoom) || !std::isfinite(G.ox) || !std::isfinite(G.oy))
      return ta_fail(ctx, TA_E_INVALID, "detections_merge: group %d: zoom %g, origin (%g, %g)", g, (double)G.zoom, (double)G.ox, (double)G.oy);
    for (int c = G.first; c < G.first + G.count; ++c) {
      if (gidx[c] >= 0) return ta_fail(ctx, TA_E_INVALID, "detections_merge: candidate row %d belongs to groups %d and %d", c, gidx[c], g);
      gidx[c] = g;
    }
    if ((long long)fr[G.frame].cap + G.count > DM_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "detections_merge: frame %d has more than %d candidates, the limit per frame", G.frame, DM_MAX_PER_FRAME);
    fr[G.frame].cap += G.count;
  }
  long long slots = 0;
  int max_cap = 0;
  for (dm_frame& F : fr) {
    F.off = (int32_t)slots;
    F.wstride = (F.cap + 63) / 64;
    slots += F.cap;                                   // <= n_candidates
    max_cap = std::max(max_cap, F.cap);
  }
  if (slots == 0) return TA_OK;

  // batches of frames: matrices within DM_MATRIX_BYTES, at most 65535 frames (grid.y)
  size_t budget = DM_MATRIX_BYTES / 8;
  if (const char* e = getenv("TA_DM_MATRIX_BYTES")) budget = (size_t)strtoull(e, nullptr, 10) / 8;   // tests: many batches at small sizes
  std::vector<int> batch_end;
  size_t mat_words = 0, batch_words = 0;
  for (int f = 0, b0 = 0; f < n_frames; ++f) {
    const size_t w = (size_t)fr[f].cap * fr[f].wstride;
    if (f > b0 && (batch_words + w > budget || f - b0 == 65535)) {
      batch_end.push_back(f);
      b0 = f;
      batch_words = 0;
    }
    fr[f].moff = batch_words;
    batch_words += w;
    mat_words = std::max(mat_words, batch_words);
  }
  batch_end.push_back(n_frames);

  const size_t C = (size_t)n_candidates, cap = capacity > 0 ? (size_t)capacity : 0;
  ta_staging st;
  const size_t o_groups = st.put(groups, (size_t)n_groups * sizeof(ta_merge_group));
  const size_t o_gidx = st.put(gidx);
  const size_t o_boxes = st.put(boxes, C * 16), o_lmks = st.put(landmarks, C * 40), o_scores = st.put(scores, C * 4);
  const size_t o_fr = st.put(fr);
  const size_t o_cnt = st.device_only((size_t)n_frames * 8);      // candidates left by the edge rule | kept, per frame
  const size_t o_mboxes = st.device_only(C * 16), o_mlmks = st.device_only(C * 40);
  const size_t o_ukeys = st.device_only((size_t)slots * 8), o_srow = st.device_only((size_t)slots * 4), o_sbox = st.device_only((size_t)slots * 16);
  const size_t o_krow = st.device_only((size_t)slots * 4);
  const size_t o_mat = st.device_only(mat_words * 8);
  const size_t o_ob = st.device_only(cap * 16), o_ol = st.device_only(cap * 40), o_os = st.device_only(cap * 4), o_src = st.device_only(cap * 4);
  const size_t h_fr = st.host_only((size_t)n_frames * sizeof(dm_frame));
  TA_TRY(st.commit(ctx));
  int* cnt = st.dev<int>(o_cnt);
  int* kcnt = cnt + n_frames;
  const dm_frame* dfr = st.dev<const dm_frame>(o_fr);
  TA_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)n_frames * 8, ctx->stream));
  {
    ta_prof_scope scope(ctx, 3, (double)C * 14);
    ctx->cur_flops = 0;
    ctx->note_kernel("dm_map_kernel");
    hipLaunchKernelGGL(dm_map_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, st.dev<const ta_merge_group>(o_groups), st.dev<const int32_t>(o_gidx),
                       st.dev<const float4>(o_boxes), st.dev<const float2>(o_lmks), st.dev<const float>(o_scores), n_candidates, edge, dfr, st.dev<float4>(o_mboxes),
                       st.dev<float2>(o_mlmks), st.dev<dm_u64>(o_ukeys), cnt);
    TA_HIP(ctx, hipGetLastError());
  }
  for (size_t b = 0, f0 = 0; b < batch_end.size(); f0 = batch_end[b++]) {
    const int nf = batch_end[b] - (int)f0;
    int cap_b = 0;
    for (int f = (int)f0; f < batch_end[b]; ++f) cap_b = std::max(cap_b, fr[f].cap);
    if (nf == 0 || cap_b == 0) continue;              // (kcnt stays 0)
    const unsigned nb = (unsigned)((cap_b + 63) / 64);
    const double pairs = (double)cap_b * cap_b * nf;
    {
      ta_prof_scope scope(ctx, 3, pairs);
      ctx->note_kernel("dm_rank_kernel");
      hipLaunchKernelGGL(dm_rank_kernel, dim3((unsigned)((cap_b + 255) / 256), (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (const int*)cnt,
                         st.dev<const dm_u64>(o_ukeys), st.dev<const float4>(o_mboxes), st.dev<int32_t>(o_srow), st.dev<float4>(o_sbox));
      TA_HIP(ctx, hipGetLastError());
    }
    {
      ta_prof_scope scope(ctx, 3, pairs / 2);
      ctx->note_kernel("dm_matrix_kernel");
      hipLaunchKernelGGL(dm_matrix_kernel, dim3(nb * (nb + 1) / 2, (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (const int*)cnt, st.dev<const float4>(o_sbox), nms_thr,
                         metric, st.dev<dm_u64>(o_mat));
      TA_HIP(ctx, hipGetLastError());
    }
    ta_prof_scope scope(ctx, 3, (double)cap_b * nf);
    ctx->note_kernel("dm_scan_kernel");
    hipLaunchKernelGGL(dm_scan_kernel, dim3((unsigned)nf), dim3(64), 0, ctx->stream, dfr, (int)f0, (const int*)cnt, st.dev<const int32_t>(o_srow), st.dev<const dm_u64>(o_mat),
                       st.dev<int32_t>(o_krow), kcnt);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipMemcpyAsync(counts, kcnt, (size_t)n_frames * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  long long total = 0;
  for (int f = 0; f < n_frames; ++f) {
    fr[f].out_base = (int32_t)total;
    total += counts[f];
  }
  if (required) *required = (int32_t)total;
  if (total > capacity) return ta_fail(ctx, TA_E_CAPACITY, "detections_merge: %lld detections, capacity %d", total, capacity);
  if (total == 0) return TA_OK;
  dm_frame* hfr = st.host<dm_frame>(h_fr);            // the frames once more, with their output slots
  memcpy(hfr, fr.data(), (size_t)n_frames * sizeof(dm_frame));
  TA_HIP(ctx, hipMemcpyAsync((void*)dfr, hfr, (size_t)n_frames * sizeof(dm_frame), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(dm_gather_kernel, dim3((unsigned)n_frames), dim3(256), 0, ctx->stream, dfr, (const int*)kcnt, st.dev<const int32_t>(o_krow), st.dev<const float4>(o_mboxes),
                     st.dev<const float2>(o_mlmks), st.dev<const float>(o_scores), st.dev<float4>(o_ob), st.dev<float2>(o_ol), st.dev<float>(o_os), st.dev<int32_t>(o_src));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipMemcpyAsync(out_boxes, st.dev<char>(o_ob), (size_t)total * 16, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_landmarks, st.dev<char>(o_ol), (size_t)total * 40, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_scores, st.dev<char>(o_os), (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_source, st.dev<char>(o_src), (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}
