// Poses of many tiles -> poses of their frames (ta_poses_merge): the tail of tiled pose estimation.
//
//  map     a present joint (kp[j][2] != 0) becomes (x + ox, y + oy, kp[j][2]) of its group, an absent one (0, 0, 0); a candidate
//          with no present joint is dropped
//  extent  bx0, bx1, by0, by1 over the mapped present joints; s2 = (bx1 - bx0 + 1) * (by1 - by0 + 1) (int64); np = present joints
//  edge    a candidate whose extent comes within `edge` pixels of an interior side of its group's rectangle is dropped
//  order   per frame: descending np, then descending score (-0 == +0), then ascending candidate row
//  pair    a, b of DIFFERENT groups are duplicates iff shared = popcount(present_a & present_b) >= min_shared and
//          (double)matched >= agree * (double)shared, matched = shared joints with (double)(dx * dx + dy * dy) <= r2 * (double)max(s2_a, s2_b),
//          r2 = radius * radius once in double
//  greedy  over the order: kept iff no earlier kept candidate is its duplicate
//
// The shape is that of detections_merge.hip: nothing is one workgroup's job but the last walk.
//  1. pm_map_kernel     a thread per candidate: coordinate bound, presence, extent, edge rule, and the survivors' two-word keys
//                       (18 - np | score descending | row) appended to their frame's list (one atomic per wave and frame)
//  2. pm_rank_kernel    the sort, by counting: rank of key i = number of keys of its frame below it, 256 keys per workgroup against
//                       the frame's list staged through LDS 256 at a time.  Leaves the frame's rows in order and its candidates
//                       WORD-MAJOR (PM_WORDS planes of one int32 per slot: 18 x, 18 y, presence mask, group, s2 low / high, extent),
//                       so that 64 consecutive candidates of one word are one 256-byte line.
//  3. pm_matrix_kernel  a workgroup per 64 x 64 block of pairs (i, j >= i's block).  Its 64 + 64 candidates are staged in LDS
//                       joint-major (word w of candidate c at [w][c]: the staging writes and lane c's own reads walk consecutive
//                       banks).  lane = candidate j keeps its own 18 joints in registers; a wave walks 16 rows i, every read of
//                       candidate i is one address for the whole wave (a broadcast); the ballot is the row's word.  A row whose
//                       extent, grown by the pair's radius, meets no lane's extent skips its joint loop.
//  4. pm_scan_kernel    one wave per frame walks the order a block of 64 at a time (readlane on the block's own column, then the
//                       kept rows ORed into the removed set, lane l holding words l, l + 64, ...).
//  5. pm_gather_kernel  kept candidates -> packed outputs.
// Frames are independent; the matrices of a call are cut in batches of frames that fit PM_MATRIX_BYTES of scratch.
//
// Exactness.  |x|, |y|, |ox|, |oy| < 2^22 is checked, so a mapped coordinate is below 2^23, dx below 2^24, dx * dx + dy * dy below
// 2^49 and s2 below 2^48: every one of them is the same number in int64 and in double, and the kernel forms d2 as
// (double)dx * (double)dx + (double)dy * (double)dy -- three exact operations, whatever the contraction -- where the definition
// says int64.  The only roundings are r2, r2 * S and agree * shared, one IEEE double multiply each; compiled with
// -ffp-contract=off (build.py).  tests/pose_tiles_model.py says the same with Python ints and floats.
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <vector>

#include "frame_regions.h"

#define PM_MAX_PER_FRAME 16384                    // candidates of one frame: 256 words per matrix row, 4 per lane of the scan
#define PM_SCAN_K (PM_MAX_PER_FRAME / 64 / 64)
#define PM_MATRIX_BYTES ((size_t)256 << 20)       // scratch the matrices of one batch of frames may take (one frame at the limit: 32 MiB)
#define PM_SCAN_UNROLL 16
#define PM_COORD_LIMIT (1 << 22)
#define PM_J 18
// planes of a sorted candidate
#define PM_X 0
#define PM_Y 18
#define PM_MASK 36
#define PM_GROUP 37
#define PM_S2LO 38
#define PM_S2HI 39
#define PM_BX0 40
#define PM_BX1 41
#define PM_BY0 42
#define PM_BY1 43
#define PM_WORDS 44

namespace {

struct pm_frame {
  int32_t off;          // first slot of the frame in the per-frame arrays (keys, rows, planes in order, kept rows)
  int32_t cap;          // candidates of its groups: what the slots hold at most
  int32_t wstride;      // 64-bit words per matrix row
  int32_t out_base;     // first output slot (filled in behind the scan)
  uint64_t moff;        // first word of its matrix within its batch's block
};

struct pm_params {
  double r2, agree;
  int32_t min_shared;
};

typedef unsigned long long pm_u64;

__device__ __forceinline__ pm_u64 pm_readlane64(pm_u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((pm_u64)hi << 32) | lo;
}

struct pm_extent {
  int32_t mask, np, bx0, bx1, by0, by1;
};

// the mapped joints of one candidate (mkp: (18, 3) int32) -> presence and extent
__device__ __forceinline__ pm_extent pm_measure(const int32_t* __restrict__ m) {
  pm_extent e = {0, 0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
#pragma unroll
  for (int j = 0; j < PM_J; ++j) {
    if (m[j * 3 + 2] == 0) continue;
    e.mask |= 1 << j;
    ++e.np;
    e.bx0 = min(e.bx0, m[j * 3]), e.bx1 = max(e.bx1, m[j * 3]);
    e.by0 = min(e.by0, m[j * 3 + 1]), e.by1 = max(e.by1, m[j * 3 + 1]);
  }
  return e;
}

__global__ __launch_bounds__(256) void pm_map_kernel(const ta_pose_group* __restrict__ groups, const int32_t* __restrict__ gidx, const int32_t* __restrict__ kp,
                                                     const double* __restrict__ scores, int C, int edge, const pm_frame* __restrict__ frames,
                                                     int32_t* __restrict__ mkp, pm_u64* __restrict__ ukeys, int* cnt, int* bad) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int g = gidx[c];
  if (g < 0) return;
  const ta_pose_group G = groups[g];
  int32_t m[PM_J * 3];
  bool wild = false;
#pragma unroll
  for (int j = 0; j < PM_J; ++j) {
    const int32_t x = kp[(size_t)c * 54 + j * 3], y = kp[(size_t)c * 54 + j * 3 + 1], p = kp[(size_t)c * 54 + j * 3 + 2];
    wild |= x <= -PM_COORD_LIMIT || x >= PM_COORD_LIMIT || y <= -PM_COORD_LIMIT || y >= PM_COORD_LIMIT;
    m[j * 3] = p ? x + G.ox : 0;                      // |ox|, |oy| < 2^22: checked on the host
    m[j * 3 + 1] = p ? y + G.oy : 0;
    m[j * 3 + 2] = p;
  }
  if (wild) {                                         // the call fails; the lowest such row goes into its message
    atomicMin(bad, c);
    return;
  }
#pragma unroll
  for (int k = 0; k < PM_J * 3; ++k) mkp[(size_t)c * 54 + k] = m[k];
  const pm_extent e = pm_measure(m);
  if (e.np == 0) return;
  if (edge > 0) {
    bool cut = false;
    cut |= (G.interior & 1) && (long long)e.bx0 < (long long)G.x0 + edge;
    cut |= (G.interior & 2) && (long long)e.by0 < (long long)G.y0 + edge;
    cut |= (G.interior & 4) && (long long)e.bx1 >= (long long)G.x1 - edge;
    cut |= (G.interior & 8) && (long long)e.by1 >= (long long)G.y1 - edge;
    if (cut) return;
  }
  // ascending key == descending np, then descending score, then ascending row; -0 counts as +0
  const pm_u64 u = (pm_u64)__double_as_longlong(__dadd_rn(scores[c], 0.0));
  const pm_u64 ord = (u >> 63) ? ~u : (u | (1ull << 63));
  const pm_u64 desc = ~ord;
  const pm_frame F = frames[G.frame];
  // one atomic per frame and wave: the lanes that append to the frame of the first lane still waiting take consecutive slots
  // behind one addition, then leave the loop
  const int lane = threadIdx.x & 63;
  int pos = 0;
  for (;;) {
    const int lead_frame = __builtin_amdgcn_readfirstlane(G.frame);
    const pm_u64 peers = __ballot(G.frame == lead_frame);
    if (G.frame == lead_frame) {
      const int lead = __ffsll((long long)peers) - 1;
      int base = 0;
      if (lane == lead) base = atomicAdd(&cnt[lead_frame], __popcll(peers));
      base = __shfl(base, lead);
      pos = base + __popcll(peers & ((1ull << lane) - 1ull));   // < F.cap: the frame's groups hold F.cap candidates in all
      break;
    }
  }
  // (18 - np, desc, row) compared word by word
  ukeys[((size_t)F.off + pos) * 2] = ((pm_u64)(unsigned)(PM_J - e.np) << 32) | (desc >> 32);
  ukeys[((size_t)F.off + pos) * 2 + 1] = (desc << 32) | (unsigned)c;
}

// grid (blocks of 256 keys, frames of the batch); planes: PM_WORDS x slots int32
__global__ __launch_bounds__(256) void pm_rank_kernel(const pm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const pm_u64* __restrict__ ukeys,
                                                      const int32_t* __restrict__ mkp, const int32_t* __restrict__ gidx, int32_t* __restrict__ srow,
                                                      int32_t* __restrict__ planes, size_t slots) {
  __shared__ pm_u64 t0[256], t1[256];
  const int f = f0 + blockIdx.y;
  const int n = cnt[f];
  if ((int)blockIdx.x * 256 >= n) return;            // uniform
  const pm_u64* keys = ukeys + (size_t)frames[f].off * 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const pm_u64 k0 = i < n ? keys[(size_t)i * 2] : ~0ull, k1 = i < n ? keys[(size_t)i * 2 + 1] : ~0ull;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + (int)threadIdx.x;
    t0[threadIdx.x] = j < n ? keys[(size_t)j * 2] : ~0ull;     // a real key's first word is below 2^37
    t1[threadIdx.x] = j < n ? keys[(size_t)j * 2 + 1] : ~0ull;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) rank += t0[k] < k0 || (t0[k] == k0 && t1[k] < k1);
    __syncthreads();
  }
  if (i < n) {
    const int row = (int)(unsigned)k1;
    const size_t s = (size_t)frames[f].off + rank;
    srow[s] = row;
    const int32_t* m = mkp + (size_t)row * 54;
    const pm_extent e = pm_measure(m);
#pragma unroll
    for (int j = 0; j < PM_J; ++j) {
      planes[(PM_X + j) * slots + s] = m[j * 3];
      planes[(PM_Y + j) * slots + s] = m[j * 3 + 1];
    }
    const long long s2 = (long long)(e.bx1 - e.bx0 + 1) * (long long)(e.by1 - e.by0 + 1);
    planes[PM_MASK * slots + s] = e.mask;
    planes[PM_GROUP * slots + s] = gidx[row];
    planes[PM_S2LO * slots + s] = (int32_t)(unsigned)(pm_u64)s2;
    planes[PM_S2HI * slots + s] = (int32_t)(s2 >> 32);
    planes[PM_BX0 * slots + s] = e.bx0;
    planes[PM_BX1 * slots + s] = e.bx1;
    planes[PM_BY0 * slots + s] = e.by0;
    planes[PM_BY1 * slots + s] = e.by1;
  }
}

// grid (blocks of 64 x 64 pairs of the largest frame, frames of the batch)
__global__ __launch_bounds__(256) void pm_matrix_kernel(const pm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const int32_t* __restrict__ planes,
                                                        size_t slots, pm_params P, pm_u64* __restrict__ mat) {
  __shared__ int32_t lds[2][PM_WORDS][64];            // [0]: the rows i of block I, [1]: the columns j of block J; 22 KiB
  const int f = f0 + blockIdx.y;
  const int n = cnt[f];
  const int nb = (n + 63) >> 6;
  int p = blockIdx.x, I = 0;
  if ((long long)p >= (long long)nb * (nb + 1) / 2) return;   // uniform
  while (p >= nb - I) {                               // pairs (0,0) (0,1) .. (0,nb-1) (1,1) ..
    p -= nb - I;
    ++I;
  }
  const int J = I + p;
  const pm_frame F = frames[f];
  // staging: 64 consecutive threads read one 256-byte line of a plane and write 64 consecutive banks; a slot at or behind n is
  // all zero (mask 0: it shares no joint with anybody)
  for (int t = threadIdx.x; t < 2 * PM_WORDS * 64; t += 256) {
    const int side = t / (PM_WORDS * 64), w = (t >> 6) % PM_WORDS, c = t & 63;
    const int idx = (side ? J : I) * 64 + c;
    lds[side][w][c] = idx < n ? planes[(size_t)w * slots + F.off + idx] : 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = J * 64 + lane;
  int32_t xb[PM_J], yb[PM_J];
#pragma unroll
  for (int q = 0; q < PM_J; ++q) xb[q] = lds[1][PM_X + q][lane], yb[q] = lds[1][PM_Y + q][lane];
  const int mask_b = lds[1][PM_MASK][lane], group_b = lds[1][PM_GROUP][lane];
  const long long s2_b = (long long)(((pm_u64)(unsigned)lds[1][PM_S2HI][lane] << 32) | (unsigned)lds[1][PM_S2LO][lane]);
  const double bx0 = (double)lds[1][PM_BX0][lane], bx1 = (double)lds[1][PM_BX1][lane];
  const double by0 = (double)lds[1][PM_BY0][lane], by1 = (double)lds[1][PM_BY1][lane];
  pm_u64 mine = 0;
  for (int k = 0; k < 16; ++k) {
    const int a = wv * 16 + k;                        // uniform in the wave, and so is every lds[0][..][a]
    const int i = I * 64 + a;
    const int both = lds[0][PM_MASK][a] & mask_b;
    const int shared = __popc(both);
    const bool live = i < n && j > i && j < n && lds[0][PM_GROUP][a] != group_b && shared >= P.min_shared;
    const long long s2_a = (long long)(((pm_u64)(unsigned)lds[0][PM_S2HI][a] << 32) | (unsigned)lds[0][PM_S2LO][a]);
    const double limit = P.r2 * (double)(s2_a > s2_b ? s2_a : s2_b);
    // a matched joint has |dx|, |dy| <= sqrt(limit) <= reach, and each end lies in its candidate's extent: extents further apart
    // than reach match nothing, and matched = 0 is no duplicate (shared >= 1, agree > 0).  A NaN or infinite reach skips nothing.
    const double reach = ceil(sqrt(limit)) + 1.0;
    const bool apart = (double)lds[0][PM_BX0][a] - reach > bx1 || bx0 - reach > (double)lds[0][PM_BX1][a] ||
                       (double)lds[0][PM_BY0][a] - reach > by1 || by0 - reach > (double)lds[0][PM_BY1][a];
    bool dup = false;
    if (__ballot(live && !apart)) {                   // uniform
      int matched = 0;
#pragma unroll
      for (int q = 0; q < PM_J; ++q) {
        const double dx = (double)(lds[0][PM_X + q][a] - xb[q]), dy = (double)(lds[0][PM_Y + q][a] - yb[q]);
        const double d2 = dx * dx + dy * dy;          // exact: see the head of the file
        matched += ((both >> q) & 1) && d2 <= limit;
      }
      dup = live && (double)matched >= P.agree * (double)shared;
    }
    const pm_u64 m = __ballot(dup);
    if (lane == k) mine = m;
  }
  const int i = I * 64 + wv * 16 + lane;
  if (lane < 16 && i < n) mat[F.moff + (size_t)i * F.wstride + J] = mine;
}

// one wave per frame of the batch
__global__ __launch_bounds__(64) void pm_scan_kernel(const pm_frame* __restrict__ frames, int f0, const int* __restrict__ cnt, const int32_t* __restrict__ srow,
                                                     const pm_u64* __restrict__ mat, int32_t* __restrict__ krow, int* __restrict__ kcnt) {
  const int f = f0 + blockIdx.x;
  const int n = cnt[f];
  const pm_frame F = frames[f];
  const int lane = threadIdx.x;
  const int W = (n + 63) >> 6, K = (W + 63) >> 6;
  const pm_u64* M = mat + F.moff;
  const size_t ws = (size_t)F.wstride;
  pm_u64 removed[PM_SCAN_K];                          // lane l: words l + 64 k of the removed set
#pragma unroll
  for (int k = 0; k < PM_SCAN_K; ++k) removed[k] = 0;
  int kept = 0;
  for (int w = 0; w < W; ++w) {
    const int i0 = w * 64, nn = n - i0 < 64 ? n - i0 : 64;
    const int row = i0 + lane;
    const pm_u64 own = lane < nn ? M[(size_t)row * ws + w] : 0ull;   // the block's own column: the first word a row has
    pm_u64 sel = removed[0];
#pragma unroll
    for (int k = 1; k < PM_SCAN_K; ++k) sel = (w >> 6) == k ? removed[k] : sel;
    pm_u64 cur = pm_readlane64(sel, w & 63);
    pm_u64 keptbits = 0;
    for (int i = 0; i < nn; ++i) {
      if ((cur >> i) & 1ull) continue;
      keptbits |= 1ull << i;
      cur |= pm_readlane64(own, i);
    }
    if ((keptbits >> lane) & 1ull) krow[(size_t)F.off + kept + __popcll(keptbits & ((1ull << lane) - 1ull))] = srow[(size_t)F.off + row];
    kept += __popcll(keptbits);
    if (w + 1 == W) break;
    // the kept rows' words behind this block, PM_SCAN_UNROLL rows at a time
    pm_u64 kb = keptbits;
    while (kb) {
      int r[PM_SCAN_UNROLL];
#pragma unroll
      for (int u = 0; u < PM_SCAN_UNROLL; ++u) {
        r[u] = kb ? i0 + __builtin_ctzll(kb) : -1;
        kb &= kb - 1;                                 // 0 stays 0
      }
#pragma unroll
      for (int k = 0; k < PM_SCAN_K; ++k) {
        if (k >= K) break;                            // uniform
        const int wd = lane + 64 * k;
        const bool live = wd > w && wd < W;
        pm_u64 v[PM_SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < PM_SCAN_UNROLL; ++u) v[u] = (live && r[u] >= 0) ? M[(size_t)r[u] * ws + wd] : 0ull;
#pragma unroll
        for (int u = 0; u < PM_SCAN_UNROLL; ++u) removed[k] |= v[u];
      }
    }
  }
  if (lane == 0) kcnt[f] = kept;
}

// one workgroup per frame
__global__ __launch_bounds__(256) void pm_gather_kernel(const pm_frame* __restrict__ frames, const int* __restrict__ kcnt, const int32_t* __restrict__ krow,
                                                        const int32_t* __restrict__ mkp, const double* __restrict__ scores, int32_t* __restrict__ o_kp,
                                                        double* __restrict__ o_scores, int32_t* __restrict__ o_source) {
  const pm_frame F = frames[blockIdx.x];
  const int K = kcnt[blockIdx.x];
  for (int t = threadIdx.x; t < K * 54; t += 256) {
    const int k = t / 54, e = t - k * 54;
    o_kp[((size_t)F.out_base + k) * 54 + e] = mkp[(size_t)krow[(size_t)F.off + k] * 54 + e];
  }
  for (int k = threadIdx.x; k < K; k += 256) {
    const int row = krow[(size_t)F.off + k];
    o_scores[(size_t)F.out_base + k] = scores[row];
    o_source[(size_t)F.out_base + k] = row;
  }
}

}  // namespace

extern "C" int ta_poses_merge(ta_ctx* ctx, const ta_pose_group* groups, int n_groups, int n_frames, const int32_t* keypoints, const double* scores,
                              int n_candidates, double radius, double agree, int min_shared, int edge, int capacity, int32_t* counts,
                              int32_t* out_keypoints, double* out_scores, int32_t* out_source, int32_t* required) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (required) *required = 0;
  if (n_groups < 0 || n_frames < 0 || n_candidates < 0 || (n_groups > 0 && !groups) || (n_frames > 0 && !counts))
    return ta_fail(ctx, TA_E_INVALID, "poses_merge: bad args");
  if (n_candidates > 0 && (!keypoints || !scores)) return ta_fail(ctx, TA_E_INVALID, "poses_merge: null candidate arrays");
  if (!std::isfinite(radius) || !(radius >= 0.0)) return ta_fail(ctx, TA_E_INVALID, "poses_merge: radius %g is not a finite number >= 0", radius);
  if (!(agree > 0.0 && agree <= 1.0)) return ta_fail(ctx, TA_E_INVALID, "poses_merge: agree %g is outside (0, 1]", agree);
  if (min_shared < 1 || min_shared > PM_J) return ta_fail(ctx, TA_E_INVALID, "poses_merge: min_shared %d is outside 1 .. %d", min_shared, PM_J);
  if (edge < 0) return ta_fail(ctx, TA_E_INVALID, "poses_merge: edge %d is negative", edge);
  if (capacity > 0 && (!out_keypoints || !out_scores || !out_source)) return ta_fail(ctx, TA_E_INVALID, "poses_merge: null outputs");
  for (int f = 0; f < n_frames; ++f) counts[f] = 0;

  // the groups: sorted by frame, rows inside the candidate arrays, no row in two groups
  std::vector<int32_t> gidx((size_t)n_candidates, -1);
  std::vector<pm_frame> fr((size_t)n_frames);
  for (pm_frame& F : fr) memset(&F, 0, sizeof(F));
  for (int g = 0; g < n_groups; ++g) {
    const ta_pose_group& G = groups[g];
    if (G.frame < 0 || G.frame >= n_frames) return ta_fail(ctx, TA_E_INVALID, "poses_merge: group %d: frame %d out of range [0, %d)", g, G.frame, n_frames);
    if (g > 0 && G.frame < groups[g - 1].frame) return ta_fail(ctx, TA_E_INVALID, "poses_merge: group %d: the groups are not sorted by frame", g);
    if (G.first < 0 || G.count < 0 || (long long)G.first + G.count > n_candidates)
      return ta_fail(ctx, TA_E_INVALID, "poses_merge: group %d: rows %d .. %lld are not inside the %d candidates", g, G.first, (long long)G.first + G.count - 1, n_candidates);
    if (G.ox <= -PM_COORD_LIMIT || G.ox >= PM_COORD_LIMIT || G.oy <= -PM_COORD_LIMIT || G.oy >= PM_COORD_LIMIT)
      return ta_fail(ctx, TA_E_INVALID, "poses_merge: group %d: origin (%d, %d) is not below 2^22 in size", g, G.ox, G.oy);
    for (int c = G.first; c < G.first + G.count; ++c) {
      if (gidx[c] >= 0) return ta_fail(ctx, TA_E_INVALID, "poses_merge: candidate row %d belongs to groups %d and %d", c, gidx[c], g);
      gidx[c] = g;
    }
    if ((long long)fr[G.frame].cap + G.count > PM_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "poses_merge: frame %d has more than %d candidates, the limit per frame", G.frame, PM_MAX_PER_FRAME);
    fr[G.frame].cap += G.count;
  }
  long long slots = 0;
  for (pm_frame& F : fr) {
    F.off = (int32_t)slots;
    F.wstride = (F.cap + 63) / 64;
    slots += F.cap;                                   // <= n_candidates
  }
  if (slots == 0) return TA_OK;

  // batches of frames: matrices within PM_MATRIX_BYTES, at most 65535 frames (grid.y)
  size_t budget = PM_MATRIX_BYTES / 8;
  if (const char* e = getenv("TA_PM_MATRIX_BYTES")) budget = (size_t)strtoull(e, nullptr, 10) / 8;   // tests: many batches at small sizes
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

  const size_t C = (size_t)n_candidates, cap = capacity > 0 ? (size_t)capacity : 0, S = (size_t)slots;
  ta_staging st;
  const size_t o_groups = st.put(groups, (size_t)n_groups * sizeof(ta_pose_group));
  const size_t o_gidx = st.put(gidx);
  const size_t o_kp = st.put(keypoints, C * 216), o_scores = st.put(scores, C * 8);
  const size_t o_fr = st.put(fr);
  const size_t o_cnt = st.device_only((size_t)n_frames * 8 + 4);  // candidates left by the map | kept, per frame | the lowest row out of bounds
  const size_t o_mkp = st.device_only(C * 216);
  const size_t o_ukeys = st.device_only(S * 16), o_srow = st.device_only(S * 4), o_planes = st.device_only(S * PM_WORDS * 4);
  const size_t o_krow = st.device_only(S * 4);
  const size_t o_mat = st.device_only(mat_words * 8);
  const size_t o_okp = st.device_only(cap * 216), o_os = st.device_only(cap * 8), o_src = st.device_only(cap * 4);
  const size_t h_fr = st.host_only((size_t)n_frames * sizeof(pm_frame) + 4);
  TA_TRY(st.commit(ctx));
  int* cnt = st.dev<int>(o_cnt);
  int* kcnt = cnt + n_frames;
  int* bad = cnt + 2 * (size_t)n_frames;
  const pm_frame* dfr = st.dev<const pm_frame>(o_fr);
  pm_frame* hfr = st.host<pm_frame>(h_fr);
  int* hbad = (int*)(hfr + n_frames);
  pm_params P;
  P.r2 = radius * radius;
  P.agree = agree;
  P.min_shared = min_shared;
  TA_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)n_frames * 8, ctx->stream));
  TA_HIP(ctx, hipMemsetAsync(bad, 0x7f, 4, ctx->stream));
  {
    ta_prof_scope scope(ctx, 3, (double)C * 54);
    ctx->cur_flops = 0;
    ctx->note_kernel("pm_map_kernel");
    hipLaunchKernelGGL(pm_map_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, st.dev<const ta_pose_group>(o_groups), st.dev<const int32_t>(o_gidx),
                       st.dev<const int32_t>(o_kp), st.dev<const double>(o_scores), n_candidates, edge, dfr, st.dev<int32_t>(o_mkp), st.dev<pm_u64>(o_ukeys), cnt, bad);
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
      ctx->note_kernel("pm_rank_kernel");
      hipLaunchKernelGGL(pm_rank_kernel, dim3((unsigned)((cap_b + 255) / 256), (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (const int*)cnt,
                         st.dev<const pm_u64>(o_ukeys), st.dev<const int32_t>(o_mkp), st.dev<const int32_t>(o_gidx), st.dev<int32_t>(o_srow), st.dev<int32_t>(o_planes), S);
      TA_HIP(ctx, hipGetLastError());
    }
    {
      ta_prof_scope scope(ctx, 3, pairs / 2);
      ctx->note_kernel("pm_matrix_kernel");
      hipLaunchKernelGGL(pm_matrix_kernel, dim3(nb * (nb + 1) / 2, (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (const int*)cnt, st.dev<const int32_t>(o_planes), S, P,
                         st.dev<pm_u64>(o_mat));
      TA_HIP(ctx, hipGetLastError());
    }
    ta_prof_scope scope(ctx, 3, (double)cap_b * nf);
    ctx->note_kernel("pm_scan_kernel");
    hipLaunchKernelGGL(pm_scan_kernel, dim3((unsigned)nf), dim3(64), 0, ctx->stream, dfr, (int)f0, (const int*)cnt, st.dev<const int32_t>(o_srow), st.dev<const pm_u64>(o_mat),
                       st.dev<int32_t>(o_krow), kcnt);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipMemcpyAsync(counts, kcnt, (size_t)n_frames * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(hbad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (*hbad < n_candidates) {
    const int row = *hbad;
    for (int f = 0; f < n_frames; ++f) counts[f] = 0;
    return ta_fail(ctx, TA_E_INVALID, "poses_merge: candidate row %d has a coordinate that is not below 2^22 in size", row);
  }
  long long total = 0;
  for (int f = 0; f < n_frames; ++f) {
    fr[f].out_base = (int32_t)total;
    total += counts[f];
  }
  if (required) *required = (int32_t)total;
  if (total > (long long)cap) return ta_fail(ctx, TA_E_CAPACITY, "poses_merge: %lld poses, capacity %d", total, capacity);   // a negative capacity counts as 0
  if (total == 0) return TA_OK;
  memcpy(hfr, fr.data(), (size_t)n_frames * sizeof(pm_frame));   // the frames once more, with their output slots
  TA_HIP(ctx, hipMemcpyAsync((void*)dfr, hfr, (size_t)n_frames * sizeof(pm_frame), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(pm_gather_kernel, dim3((unsigned)n_frames), dim3(256), 0, ctx->stream, dfr, (const int*)kcnt, st.dev<const int32_t>(o_krow), st.dev<const int32_t>(o_mkp),
                     st.dev<const double>(o_scores), st.dev<int32_t>(o_okp), st.dev<double>(o_os), st.dev<int32_t>(o_src));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipMemcpyAsync(out_keypoints, st.dev<char>(o_okp), (size_t)total * 216, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_scores, st.dev<char>(o_os), (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_source, st.dev<char>(o_src), (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}
