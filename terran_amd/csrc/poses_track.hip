// Skeletons of consecutive frames -> which skeleton of an earlier frame each one continues (ta_poses_track).
//
//  pairs    a in frame ta, b in frame tb of the same sequence, tb no history frame, g = tb - ta, 1 <= g <= max_gap + 1
//  shared   the joints present in both, s of them; size = max(max x - min x, max y - min y) over a skeleton's present joints,
//           M = the larger size of the two; D = sum over the shared joints of dx^2 + dy^2
//  pair     qualifies iff s >= min_shared and D * 1 000 000 <= radius_permille^2 * g * M^2 * s
//  cost     D * (12 252 240 / s), 12 252 240 = lcm(1 .. 18)
//  match    frames ascending; at frame t the qualifying pairs with b in t and a open (not closed on input, no successor so far) in
//           the order (cost, g, a, b); a pair links iff a has no successor and b no predecessor yet
//
// As in faces_poses_link.hip, the greedy walk over a strict total order equals committing every mutually best pair again and
// again: within a frame the open predecessors and the free rows only get fewer, so a pair that is the cheapest of its b by (cost,
// g, a) and of its a by (cost, b) -- an a lies in one frame, its g is fixed -- is cheaper than every pair it conflicts with, and
// the sorted walk takes it first.  Whether a pair qualifies never changes, so the O(n^2 * 18) scan runs once for every (frame, gap)
// of a batch, in parallel, and leaves a bit matrix; only availability is sequential, and it walks set bits.
//  1. pt_pack_kernel     a thread per skeleton: word-major planes (18 x, 18 y, presence mask, size, the extent of the present
//                        joints), 64 consecutive skeletons of one word one 256-byte line.  An absent joint gets x = y = 0, whatever
//                        the row held; a skeleton with no joint has the empty mask and qualifies with nobody.
//  2. pt_scan_kernel     a workgroup per 64 a x 256 b of one (frame, gap), many per pair of frames.  The 64 a rows sit in LDS
//                        word-major (42 words a row, 10.5 KiB), every read one address for the wave: a broadcast.  lane = b keeps
//                        its 36 coordinates, mask, size and extent in registers.  popcount(mask_a & mask_b) comes first; then the
//                        extents: every shared joint moved at least the gap between the two extents, so
//                        (gx^2 + gy^2) * 10^6 > r^2 g M^2 refuses the pair with two 64-bit products; only a wave with a lane left
//                        runs the 18-joint sum.  The ballot is a's row word, each lane collects its own bit per a into b's row word:
//                        both sides get rows, word-major as in the link, and nothing is combined across waves.
//  3. pt_resolve_kernel  ONE workgroup of 1024 threads per sequence, persistent over the frames of the batch and the rounds of a
//                        frame, with barriers between the halves of a round: no launch per round.  Half one: a thread per free b
//                        walks its row words over the gaps ascending and keeps the cheapest open a (strict compare on the whole
//                        int64 cost; g and a ascend, so of equal costs the first stays); a thread per open a of the max_gap + 1
//                        frames before walks its row word over t's rows and keeps the cheapest free b.  Half two: a thread per b
//                        commits a mutual choice (only it writes prev[b] and succ[a]); a b with no open partner left is retired,
//                        an a with no free partner left is marked idle for this frame.  __syncthreads_or says whether anything
//                        was linked; a silent round ends the frame.  No atomics at all.
//  4. pt_root_kernel     root by pointer jumping, double-buffered, ceil(log2(frames of the longest sequence)) launches.
// Frames are cut in batches whose matrices fit PT_MATRIX_BYTES of scratch; a frame's pairs all lie in its batch, batches run in
// frame order, and succ / prev stay on the device between them.
//
// What the resolution costs.  A frame at the 4 096 limit with max_gap = 30 has 4 096 b rows (4 a thread) and up to 126 976 a rows
// (124 a thread), each row 64 words a gap: a round reads at most 2 * 31 * 2 MiB of matrix words through one CU, and the rounds
// of a moving crowd are few (most rows commit in the first).  Rows that already have a successor cost one load.  The sequences
// run side by side, one CU each; a call with one sequence uses one CU for this step and says so in DESIGN 7q.
//
// Exactness.  Everything is integer.  |x|, |y| < 2^14 (checked, every joint of every row), so |dx| < 2^15, dx^2 + dy^2 < 2^31
// (one uint32), D < 18 * 2^31 < 2^36 and D * 10^6 < 2^56.  size < 2^15, M^2 < 2^30, r^2 <= 10^6 < 2^20, g <= 31 < 2^5, s <= 18 <
// 2^5: the right side is below 2^60.  12 252 240 < 2^24, so cost < 2^60.  The extent test: gx, gy < 2^15, gx^2 + gy^2 < 2^31,
// times 10^6 below 2^51; r^2 g M^2 < 2^55.  int64 (uint64) holds every one; no float appears anywhere.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "frame_regions.h"

#define PT_MAX_PER_FRAME 4096
#define PT_MATRIX_BYTES ((size_t)256 << 20)       // scratch the matrices of one batch of frames may take
#define PT_COORD_LIMIT (1 << 14)
#define PT_LCM 12252240ll
#define PT_B_CHUNK 256                            // b rows of one workgroup of the scan: 64 per wave
#define PT_RESOLVE_THREADS 1024
// planes of a packed skeleton
#define PT_X 0
#define PT_Y 18
#define PT_MASK 36
#define PT_SIZE 37
#define PT_BX0 38
#define PT_BX1 39
#define PT_BY0 40
#define PT_BY1 41
#define PT_WORDS 42
// states of prev[] / succ[] while the call runs
#define PT_FREE (-1)
#define PT_RETIRED (-2)                           // prev: no open partner left; succ: closed on input

namespace {

typedef unsigned long long pt_u64;

// one (frame t, gap g) with rows on both sides
struct pt_pair {
  int32_t boff, nb;     // the rows of t: global rows boff .. boff + nb - 1
  int32_t aoff, na;     // the rows of t - g
  int32_t g, pad;
  uint64_t moff;        // first word of b's rows (nb x ceil(na / 64) words, word-major) within the batch's block
  uint64_t toff;        // ... of a's rows (na x ceil(nb / 64) words)
};

struct pt_frame {
  int32_t poff, np;     // its rows
  int32_t pair0, npairs;   // its pairs in the pair list, gaps ascending (none for a history frame)
};

struct pt_span {
  int32_t f0, f1;       // frames of one sequence inside one batch
};

__global__ __launch_bounds__(256) void pt_pack_kernel(const int32_t* __restrict__ kp, const uint8_t* __restrict__ closed, int P,
                                                      int32_t* __restrict__ planes, int32_t* __restrict__ prev, int32_t* __restrict__ succ,
                                                      int32_t* __restrict__ idle) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int mask = 0, bx0 = INT32_MAX, bx1 = INT32_MIN, by0 = INT32_MAX, by1 = INT32_MIN;
  for (int j = 0; j < 18; ++j) {
    const int32_t* q = kp + (size_t)p * 54 + j * 3;
    const bool here = q[2] != 0;
    const int x = here ? q[0] : 0, y = here ? q[1] : 0;
    if (here) {
      mask |= 1 << j;
      bx0 = min(bx0, x), bx1 = max(bx1, x), by0 = min(by0, y), by1 = max(by1, y);
    }
    planes[(size_t)(PT_X + j) * P + p] = x;
    planes[(size_t)(PT_Y + j) * P + p] = y;
  }
  if (!mask) bx0 = bx1 = by0 = by1 = 0;
  planes[(size_t)PT_MASK * P + p] = mask;
  planes[(size_t)PT_SIZE * P + p] = max(bx1 - bx0, by1 - by0);
  planes[(size_t)PT_BX0 * P + p] = bx0;
  planes[(size_t)PT_BX1 * P + p] = bx1;
  planes[(size_t)PT_BY0 * P + p] = by0;
  planes[(size_t)PT_BY1 * P + p] = by1;
  prev[p] = PT_FREE;
  succ[p] = closed && closed[p] ? PT_RETIRED : PT_FREE;
  idle[p] = -1;
}

// grid (a blocks x b chunks of the batch's largest pair, pairs of the batch)
__global__ __launch_bounds__(256) void pt_scan_kernel(const pt_pair* __restrict__ pairs, int q0, int bchunks, const int32_t* __restrict__ planes, int P,
                                                      int r2, int min_shared, pt_u64* __restrict__ mat) {
  __shared__ int32_t sa[PT_WORDS][64];
  const pt_pair Q = pairs[q0 + blockIdx.y];
  const int I = blockIdx.x / bchunks, chunk = blockIdx.x - I * bchunks;
  if (I * 64 >= Q.na || chunk * PT_B_CHUNK >= Q.nb) return;        // uniform
  for (int k = threadIdx.x; k < PT_WORDS * 64; k += 256) {
    const int w = k >> 6, r = k & 63, a = I * 64 + r;
    sa[w][r] = a < Q.na ? planes[(size_t)w * P + Q.aoff + a] : 0;   // a row behind the frame: the empty mask
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, J = chunk * (PT_B_CHUNK / 64) + (threadIdx.x >> 6);
  if (J * 64 >= Q.nb) return;                           // uniform in the wave, and behind the only barrier
  const int b = J * 64 + lane;
  const bool live = b < Q.nb;
  const size_t gb = (size_t)Q.boff + (live ? b : 0);
  int x[18], y[18];
#pragma unroll
  for (int j = 0; j < 18; ++j) x[j] = planes[(size_t)(PT_X + j) * P + gb], y[j] = planes[(size_t)(PT_Y + j) * P + gb];
  const int mb = live ? planes[(size_t)PT_MASK * P + gb] : 0;       // a lane behind the frame's rows shares no joint
  const int zb = planes[(size_t)PT_SIZE * P + gb];
  const int bx0 = planes[(size_t)PT_BX0 * P + gb], bx1 = planes[(size_t)PT_BX1 * P + gb];
  const int by0 = planes[(size_t)PT_BY0 * P + gb], by1 = planes[(size_t)PT_BY1 * P + gb];
  const pt_u64 K = (pt_u64)r2 * (pt_u64)Q.g;            // < 2^25
  pt_u64 mine = 0, col = 0;                             // lane k: the row word of a = I * 64 + k; lane b: its own bits over the 64 a
  for (int k = 0; k < 64; ++k) {
    const int m = sa[PT_MASK][k] & mb;                  // one address for the wave
    const int s = __popc(m);
    bool q = false;
    if (__ballot(s >= min_shared)) {                    // uniform
      const int M = max(sa[PT_SIZE][k], zb);
      const pt_u64 KM = K * (pt_u64)((unsigned)M * (unsigned)M);    // r^2 g M^2 < 2^55
      const int gx = max(0, max(bx0 - sa[PT_BX1][k], sa[PT_BX0][k] - bx1)), gy = max(0, max(by0 - sa[PT_BY1][k], sa[PT_BY0][k] - by1));
      // every shared joint moved at least (gx, gy): D / s >= gx^2 + gy^2
      const bool near = s >= min_shared && (pt_u64)((unsigned)(gx * gx) + (unsigned)(gy * gy)) * 1000000ull <= KM;
      if (__ballot(near)) {                             // uniform
        pt_u64 D = 0;
#pragma unroll
        for (int j = 0; j < 18; ++j) {
          const int dx = x[j] - sa[PT_X + j][k], dy = y[j] - sa[PT_Y + j][k];
          const unsigned d = (unsigned)(dx * dx) + (unsigned)(dy * dy);     // < 2^31
          D += ((m >> j) & 1) ? d : 0u;
        }
        q = near && D * 1000000ull <= KM * (pt_u64)s;
      }
    }
    const pt_u64 w = __ballot(q);
    if (lane == k) mine = w;
    col |= (pt_u64)q << k;
  }
  const int a = I * 64 + lane;
  if (a < Q.na) mat[Q.toff + (size_t)J * Q.na + a] = mine;
  if (live) mat[Q.moff + (size_t)I * Q.nb + b] = col;
}

// D * (lcm / s) of two packed rows (s >= 1: the pair qualifies)
__device__ __forceinline__ long long pt_cost(const int32_t* planes, int P, size_t ga, const int* x, const int* y, int mb) {
  const int m = planes[(size_t)PT_MASK * P + ga] & mb;
  pt_u64 D = 0;
#pragma unroll
  for (int j = 0; j < 18; ++j) {
    const int dx = x[j] - planes[(size_t)(PT_X + j) * P + ga], dy = y[j] - planes[(size_t)(PT_Y + j) * P + ga];
    const unsigned d = (unsigned)(dx * dx) + (unsigned)(dy * dy);
    D += ((m >> j) & 1) ? d : 0u;
  }
  return (long long)D * (PT_LCM / __popc(m));
}

// grid: the sequences that have frames in this batch; prev, succ, idle and the choices are read and written by the same
// workgroup across barriers, so none of them is __restrict__ or const
__global__ __launch_bounds__(PT_RESOLVE_THREADS) void pt_resolve_kernel(const pt_span* __restrict__ spans, const pt_frame* __restrict__ frames,
                                                                        const pt_pair* __restrict__ pairs, const int32_t* __restrict__ planes, int P,
                                                                        const pt_u64* __restrict__ mat, int32_t* prev, int32_t* succ, int32_t* idle,
                                                                        int32_t* best_a, int32_t* best_b) {
  const pt_span S = spans[blockIdx.x];
  for (int t = S.f0; t < S.f1; ++t) {                   // uniform
    const pt_frame F = frames[t];
    if (F.npairs == 0 || F.np == 0) continue;
    for (;;) {
      // half one: every free b of t, every open a of the frames before, chooses
      for (int b = threadIdx.x; b < F.np; b += PT_RESOLVE_THREADS) {
        const size_t gb = (size_t)F.poff + b;
        if (prev[gb] != PT_FREE) continue;
        int x[18], y[18];
#pragma unroll
        for (int j = 0; j < 18; ++j) x[j] = planes[(size_t)(PT_X + j) * P + gb], y[j] = planes[(size_t)(PT_Y + j) * P + gb];
        const int mb = planes[(size_t)PT_MASK * P + gb];
        long long best = INT64_MAX;
        int who = -1;
        for (int q = 0; q < F.npairs; ++q) {            // gaps ascending
          const pt_pair Q = pairs[F.pair0 + q];
          const int W = (Q.na + 63) >> 6;
          for (int w = 0; w < W; ++w) {
            pt_u64 bits = mat[Q.moff + (size_t)w * Q.nb + b];
            while (bits) {
              const int a = Q.aoff + w * 64 + __builtin_ctzll(bits);      // the scan sets no bit behind the frame's rows
              bits &= bits - 1;
              if (succ[a] != PT_FREE) continue;
              const long long c = pt_cost(planes, P, (size_t)a, x, y, mb);
              if (c < best) best = c, who = a;          // g, then a, ascend: of equal costs the first stays
            }
          }
        }
        best_a[gb] = who;
      }
      for (int q = 0; q < F.npairs; ++q) {
        const pt_pair Q = pairs[F.pair0 + q];
        const int W = (Q.nb + 63) >> 6;
        for (int a = threadIdx.x; a < Q.na; a += PT_RESOLVE_THREADS) {
          const size_t ga = (size_t)Q.aoff + a;
          if (succ[ga] != PT_FREE || idle[ga] == t) continue;
          int x[18], y[18];
#pragma unroll
          for (int j = 0; j < 18; ++j) x[j] = planes[(size_t)(PT_X + j) * P + ga], y[j] = planes[(size_t)(PT_Y + j) * P + ga];
          const int ma = planes[(size_t)PT_MASK * P + ga];
          long long best = INT64_MAX;
          int who = -1;
          for (int w = 0; w < W; ++w) {
            pt_u64 bits = mat[Q.toff + (size_t)w * Q.na + a];
            while (bits) {
              const int b = Q.boff + w * 64 + __builtin_ctzll(bits);
              bits &= bits - 1;
              if (prev[b] != PT_FREE) continue;
              const long long c = pt_cost(planes, P, (size_t)b, x, y, ma);
              if (c < best) best = c, who = b;
            }
          }
          best_b[ga] = who;
          if (who < 0) idle[ga] = t;                    // the free rows of t only get fewer
        }
      }
      __syncthreads();
      // half two: mutual choices link.  A b that was free has a fresh choice; so has the a it chose, which was open with b free
      bool linked = false;
      for (int b = threadIdx.x; b < F.np; b += PT_RESOLVE_THREADS) {
        const size_t gb = (size_t)F.poff + b;
        if (prev[gb] != PT_FREE) continue;
        const int a = best_a[gb];
        if (a < 0) {
          prev[gb] = PT_RETIRED;
        } else if (best_b[a] == (int)gb) {              // only this thread writes these two words in this half
          prev[gb] = a;
          succ[a] = (int)gb;
          linked = true;
        }
      }
      if (!__syncthreads_or(linked)) break;             // uniform: a silent round ends the frame
    }
  }
}

__global__ __launch_bounds__(256) void pt_root_init_kernel(const int32_t* __restrict__ prev, int P, int32_t* __restrict__ root) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < P) root[p] = prev[p] >= 0 ? prev[p] : p;
}

__global__ __launch_bounds__(256) void pt_root_kernel(const int32_t* __restrict__ in, int P, int32_t* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < P) out[p] = in[in[p]];
}

}  // namespace

extern "C" int ta_poses_track(ta_ctx* ctx, int n_sequences, const int32_t* frames_per_sequence, const int32_t* history_frames, int n_frames,
                              const int32_t* pose_counts, const int32_t* keypoints, const uint8_t* closed, int n_poses, int radius_permille,
                              int min_shared, int max_gap, int32_t* prev_out, int32_t* root_out, int32_t* links) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_sequences < 0 || n_frames < 0 || n_poses < 0) return ta_fail(ctx, TA_E_INVALID, "poses_track: bad args");
  if ((n_sequences > 0 && (!frames_per_sequence || !history_frames)) || (n_frames > 0 && !pose_counts) ||
      (n_poses > 0 && (!keypoints || !prev_out || !root_out)))
    return ta_fail(ctx, TA_E_INVALID, "poses_track: a null array that has rows");
  if (radius_permille < 1 || radius_permille > 1000)
    return ta_fail(ctx, TA_E_INVALID, "poses_track: radius_permille %d is outside 1 .. 1000", radius_permille);
  if (min_shared < 1 || min_shared > 18) return ta_fail(ctx, TA_E_INVALID, "poses_track: min_shared %d is outside 1 .. 18", min_shared);
  if (max_gap < 0 || max_gap > 30) return ta_fail(ctx, TA_E_INVALID, "poses_track: max_gap %d is outside 0 .. 30", max_gap);
  long long T = 0, P = 0;
  for (int s = 0; s < n_sequences; ++s) {
    if (frames_per_sequence[s] < 0) return ta_fail(ctx, TA_E_INVALID, "poses_track: sequence %d: negative count (%d frames)", s, frames_per_sequence[s]);
    if (history_frames[s] < 0 || history_frames[s] > frames_per_sequence[s])
      return ta_fail(ctx, TA_E_INVALID, "poses_track: sequence %d: history_frames %d is outside 0 .. %d", s, history_frames[s], frames_per_sequence[s]);
    T += frames_per_sequence[s];
  }
  if (T != n_frames) return ta_fail(ctx, TA_E_INVALID, "poses_track: the sequences sum to %lld frames, the arrays have %d", T, n_frames);
  for (int f = 0; f < n_frames; ++f) {
    if (pose_counts[f] < 0) return ta_fail(ctx, TA_E_INVALID, "poses_track: frame %d: negative count (%d poses)", f, pose_counts[f]);
    P += pose_counts[f];
  }
  if (P != n_poses) return ta_fail(ctx, TA_E_INVALID, "poses_track: the counts sum to %lld poses, the arrays have %d rows", P, n_poses);
  for (int f = 0; f < n_frames; ++f)
    if (pose_counts[f] > PT_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "poses_track: frame %d has %d poses, the limit per frame is %d", f, pose_counts[f], PT_MAX_PER_FRAME);
  for (long long r = 0; r < P; ++r) {
    const int32_t* q = keypoints + r * 54;
    unsigned wild = 0;                                  // |v| < 2^14  <=>  (unsigned)(v + 2^14 - 1) < 2^15 - 1
    for (int j = 0; j < 18; ++j)
      wild |= (unsigned)((unsigned)q[j * 3] + (PT_COORD_LIMIT - 1) >= 2u * PT_COORD_LIMIT - 1u) | (unsigned)((unsigned)q[j * 3 + 1] + (PT_COORD_LIMIT - 1) >= 2u * PT_COORD_LIMIT - 1u);
    if (wild) return ta_fail(ctx, TA_E_INVALID, "poses_track: pose row %lld has a coordinate that is not below 2^14 in size", r);
  }

  for (long long k = 0; k < P; ++k) prev_out[k] = -1, root_out[k] = (int32_t)k;
  if (links)
    for (int f = 0; f < n_frames; ++f) links[f] = 0;

  // frames, and the (frame, gap) pairs that have rows on both sides
  const int G = max_gap + 1;
  std::vector<pt_frame> fr((size_t)n_frames);
  std::vector<int32_t> seq_of((size_t)n_frames);
  std::vector<pt_pair> pairs;
  int longest = 0;
  {
    long long off = 0;
    int f = 0;
    for (int s = 0; s < n_sequences; ++s) {
      longest = std::max(longest, frames_per_sequence[s]);
      for (int k = 0; k < frames_per_sequence[s]; ++k, ++f) {
        memset(&fr[f], 0, sizeof(pt_frame));
        fr[f].poff = (int32_t)off, fr[f].np = pose_counts[f];
        fr[f].pair0 = (int32_t)pairs.size();
        seq_of[f] = s;
        if (k >= history_frames[s] && fr[f].np > 0)
          for (int g = 1; g <= G && g <= k; ++g) {
            if (fr[f - g].np == 0) continue;
            pt_pair q;
            memset(&q, 0, sizeof q);
            q.boff = fr[f].poff, q.nb = fr[f].np, q.aoff = fr[f - g].poff, q.na = fr[f - g].np, q.g = g;
            pairs.push_back(q);
          }
        fr[f].npairs = (int32_t)pairs.size() - fr[f].pair0;
        off += pose_counts[f];
      }
    }
  }
  if (pairs.empty()) return TA_OK;

  // batches of frames: matrices within PT_MATRIX_BYTES, at most 65535 pairs (grid.y); a frame's pairs stay together
  size_t budget = PT_MATRIX_BYTES / 8;
  if (const char* e = getenv("TA_PT_MATRIX_BYTES")) budget = (size_t)strtoull(e, nullptr, 10) / 8;     // tests: many batches at small sizes
  std::vector<int> batch_end;
  size_t mat_words = 0, batch_words = 0;
  for (int f = 0, b0 = 0; f < n_frames; ++f) {
    size_t wf = 0;
    for (int q = 0; q < fr[f].npairs; ++q) {
      const pt_pair& Q = pairs[fr[f].pair0 + q];
      wf += (size_t)Q.nb * ((Q.na + 63) / 64) + (size_t)Q.na * ((Q.nb + 63) / 64);
    }
    if (f > b0 && (batch_words + wf > budget || fr[f].pair0 + fr[f].npairs - fr[b0].pair0 > 65535)) {
      batch_end.push_back(f);
      b0 = f;
      batch_words = 0;
    }
    for (int q = 0; q < fr[f].npairs; ++q) {
      pt_pair& Q = pairs[fr[f].pair0 + q];
      Q.moff = batch_words;
      Q.toff = batch_words + (size_t)Q.nb * ((Q.na + 63) / 64);
      batch_words = Q.toff + (size_t)Q.na * ((Q.nb + 63) / 64);
    }
    mat_words = std::max(mat_words, batch_words);
  }
  batch_end.push_back(n_frames);
  // per batch, the runs of frames of one sequence
  std::vector<pt_span> spans;
  std::vector<int> span_end;
  for (size_t b = 0, f0 = 0; b < batch_end.size(); f0 = batch_end[b++]) {
    for (int f = (int)f0; f < batch_end[b];) {
      int e = f + 1;
      while (e < batch_end[b] && seq_of[e] == seq_of[f]) ++e;
      bool work = false;
      for (int k = f; k < e; ++k) work |= fr[k].npairs > 0;
      if (work) spans.push_back({f, e});
      f = e;
    }
    span_end.push_back((int)spans.size());
  }

  const size_t nP = (size_t)P;
  ta_staging st;
  const size_t o_fr = st.put(fr), o_pairs = st.put(pairs), o_spans = st.put(spans);
  const size_t o_kp = st.put(keypoints, nP * 216);
  const size_t o_closed = closed ? st.put(closed, nP) : 0;
  const size_t o_planes = st.device_only(nP * PT_WORDS * 4);
  const size_t o_state = st.device_only(nP * 4 * 5);    // prev | succ | idle | each b's choice | each a's
  const size_t o_root = st.device_only(nP * 4 * 2);
  const size_t o_mat = st.device_only(mat_words * 8);
  const size_t h_out = st.host_only(nP * 4 * 2);
  TA_TRY(st.commit(ctx));
  const pt_frame* dfr = st.dev<const pt_frame>(o_fr);
  const pt_pair* dpairs = st.dev<const pt_pair>(o_pairs);
  const pt_span* dspans = st.dev<const pt_span>(o_spans);
  const int32_t* dplanes = st.dev<const int32_t>(o_planes);
  int32_t* prev = st.dev<int32_t>(o_state);
  int32_t *succ = prev + nP, *idle = succ + nP, *best_a = idle + nP, *best_b = best_a + nP;
  int32_t* root[2] = {st.dev<int32_t>(o_root), st.dev<int32_t>(o_root) + nP};
  pt_u64* dmat = st.dev<pt_u64>(o_mat);
  const unsigned pblocks = (unsigned)((nP + 255) / 256);
  {
    ta_prof_scope scope(ctx, 3, (double)nP * 54);
    ctx->cur_flops = 0;
    ctx->note_kernel("pt_pack_kernel");
    hipLaunchKernelGGL(pt_pack_kernel, dim3(pblocks), dim3(256), 0, ctx->stream, st.dev<const int32_t>(o_kp),
                       closed ? st.dev<const uint8_t>(o_closed) : (const uint8_t*)nullptr, (int)P, st.dev<int32_t>(o_planes), prev, succ, idle);
    TA_HIP(ctx, hipGetLastError());
  }
  for (size_t b = 0, f0 = 0, s0 = 0; b < batch_end.size(); f0 = batch_end[b], s0 = span_end[b], ++b) {
    const int q0 = fr[f0].pair0, q1 = batch_end[b] < n_frames ? fr[batch_end[b]].pair0 : (int)pairs.size();
    if (q1 == q0) continue;
    int max_a = 0, max_b = 0;
    double work = 0;
    for (int q = q0; q < q1; ++q) {
      max_a = std::max(max_a, pairs[q].na), max_b = std::max(max_b, pairs[q].nb);
      work += (double)pairs[q].na * pairs[q].nb;
    }
    const unsigned ablocks = (unsigned)((max_a + 63) / 64), bchunks = (unsigned)((max_b + PT_B_CHUNK - 1) / PT_B_CHUNK);
    {
      ta_prof_scope scope(ctx, 3, work * 18);
      ctx->note_kernel("pt_scan_kernel");
      hipLaunchKernelGGL(pt_scan_kernel, dim3(ablocks * bchunks, (unsigned)(q1 - q0)), dim3(256), 0, ctx->stream, dpairs, q0, (int)bchunks, dplanes,
                         (int)P, radius_permille * radius_permille, min_shared, dmat);
      TA_HIP(ctx, hipGetLastError());
    }
    const int ns = span_end[b] - (int)s0;
    ta_prof_scope scope(ctx, 3, work);
    ctx->note_kernel("pt_resolve_kernel");
    hipLaunchKernelGGL(pt_resolve_kernel, dim3((unsigned)ns), dim3(PT_RESOLVE_THREADS), 0, ctx->stream, dspans + s0, dfr, dpairs, dplanes, (int)P,
                       (const pt_u64*)dmat, prev, succ, idle, best_a, best_b);
    TA_HIP(ctx, hipGetLastError());
  }
  int cur = 0;
  {
    ta_prof_scope scope(ctx, 3, (double)nP);
    ctx->note_kernel("pt_root_kernel");
    hipLaunchKernelGGL(pt_root_init_kernel, dim3(pblocks), dim3(256), 0, ctx->stream, (const int32_t*)prev, (int)P, root[0]);
    TA_HIP(ctx, hipGetLastError());
    // a chain has at most `longest` rows: after k jumps a row points 2^k links back, or at its root
    for (int reach = 1; reach < longest - 1; reach *= 2, cur ^= 1) {
      hipLaunchKernelGGL(pt_root_kernel, dim3(pblocks), dim3(256), 0, ctx->stream, (const int32_t*)root[cur], (int)P, root[cur ^ 1]);
      TA_HIP(ctx, hipGetLastError());
    }
  }
  int32_t* hout = st.host<int32_t>(h_out);
  TA_HIP(ctx, hipMemcpyAsync(hout, prev, nP * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(hout + nP, root[cur], nP * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < nP; ++k) prev_out[k] = hout[k] >= 0 ? hout[k] : -1;
  memcpy(root_out, hout + nP, nP * 4);
  if (links)
    for (int f = 0; f < n_frames; ++f)
      for (int k = 0; k < fr[f].np; ++k) links[f] += prev_out[fr[f].poff + k] >= 0;
  return TA_OK;
}
