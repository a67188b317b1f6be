// Skeletons -> the pixels of the people they describe, blended into resident frames in place (ta_poses_paint).
//
//  size     M = max(max x - min x, max y - min y) over a pose's present joints; r_c = max(min_radius, M * permille[c] / 1000) for
//           the classes HEAD 0, TORSO 1, LIMB 2
//  shapes   a disc of its class's radius at every present joint, a capsule of its class's radius along each of the 18 segments
//           whose two ends are present; a pose covers a pixel iff one of its shapes does (all tests inclusive, int64)
//  paint    the poses of a frame in list order, a pixel blended ONCE per pose that covers it: ((v >> 8) + v) >> 8 of
//           v = in * (255 - a) + ink * a + 128, draw.hip's blend
//
// Host: the checks, then one record per pose in the staging copy -- joints (absent ones at 0, 0), presence mask, the three radii,
// ink, and the set of shapes worth testing: a disc is left out when a present segment of at least its radius ends at its joint (the
// capsule's cap is that disc or a larger one), which for a whole skeleton leaves the 18 capsules -- and beside it the pose's box:
// the extent of its present joints widened by its largest radius and clipped to the frame (empty for alpha 0 and for no joint).
//  1. pp_bin_kernel     a wave per (tile, 64 poses): lane = pose, its box against the tile, the ballot is the word.  The tile x pose
//                       bit matrix lives in the context's scratch block; nothing is a list, so nothing truncates.
//  2. pp_paint_kernel   a workgroup per tile of 16 rows x 16 groups of 4 pixels, a thread per group.  A row's groups are cut where
//                       its bytes are dword aligned: group G of a row whose address is phi mod 4 holds the pixels phi + 4 (G - 1) ..
//                       + 3, so every whole group is three aligned dwords (pixel_walk.h's cut; group 0 is the row's head, the last
//                       may be a tail: those go bytewise).  The workgroup walks its tile's row of the matrix: words and records are
//                       uniform, so the compiler keeps them in scalar registers.  Per pose and shape: the shape's box against the
//                       tile (uniform), against the thread's row and pixels, then the int64 test; a covered pixel takes no further
//                       test of that pose and a wave whose pixels are all covered leaves the pose's shapes.  Pixels are loaded at
//                       the first pose that covers one of the thread's four and stored only then: with clear == 0 a tile no pose
//                       touches issues no load and no store.  With clear the pixels start as 0, are never loaded and always stored.
// Frames are taken in batches whose matrices fit PP_MATRIX_BYTES; a frame whose own matrix does not is cut into runs of poses that
// go in consecutive launches (the order of a pixel's blends is the list's either way), only the first of which clears.
//
// Exactness.  |x|, |y| < 2^14 (checked), frames at most 16384 a side: |p|, |d| < 2^15, t, L2, p.p, cross < 2^31, cross^2 < 2^62,
// r < 2^15, r^2 L2 < 2^61.  int64 throughout; no float appears anywhere.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "frame_regions.h"

#define PP_MAX_PER_FRAME 16384
#define PP_MATRIX_BYTES ((size_t)256 << 20)       // scratch the matrices of one batch of frames may take
#define PP_COORD_LIMIT (1 << 14)
#define PP_SIDE_LIMIT 16384
#define PP_MIN_RADIUS_LIMIT 4096
#define PP_TILE_ROWS 16
#define PP_TILE_GROUPS 16                         // groups of 4 pixels in a tile's row
#define PP_SHAPES 36                              // 18 segments, then 18 discs

namespace {

typedef unsigned long long pp_u64;

struct pp_rec {
  int32_t x[18], y[18];
  uint32_t shapes_lo, shapes_hi;    // bit s: shape s is tested (s < 18: segment s; s >= 18: the disc of joint s - 18)
  int32_t r[3];
  uint32_t rgba;
  int32_t pad[6];
};
static_assert(sizeof(pp_rec) == 192, "pp_rec is 48 words");

// a frame's poses, or a run of them, against the frame's tiles
struct pp_job {
  int32_t frame;
  int32_t p0, np;       // global rows p0 .. p0 + np - 1
  int32_t words;        // ceil(np / 64)
  int32_t clear, pad;
  uint64_t moff;        // first word of its matrix (tiles x words, tile-major) within the batch's block
};

// the 17 connections of vis.POSE_CONNECTIONS and (8, 11); the class of each segment, then of each joint
constexpr int PP_A[18] = {0, 0, 14, 0, 15, 1, 2, 3, 1, 8, 9, 1, 5, 6, 1, 11, 12, 8};
constexpr int PP_B[18] = {1, 14, 16, 15, 17, 2, 3, 4, 8, 9, 10, 5, 6, 7, 11, 12, 13, 11};
constexpr int PP_SEG_CLASS[18] = {0, 0, 0, 0, 0, 1, 2, 2, 1, 2, 2, 1, 2, 2, 1, 2, 2, 1};
constexpr int PP_JOINT_CLASS[18] = {0, 1, 1, 2, 2, 1, 2, 2, 1, 2, 2, 1, 2, 2, 0, 0, 0, 0};

// grid (waves of the batch's largest job / 4, jobs of the batch)
__global__ __launch_bounds__(256) void pp_bin_kernel(const pp_job* __restrict__ jobs, int j0, const int4* __restrict__ boxes, int tiles_x, int tiles,
                                                     pp_u64* __restrict__ mat) {
  const pp_job J = jobs[j0 + blockIdx.y];
  const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave >= (size_t)tiles * J.words) return;          // uniform in the wave
  const int tile = (int)(wave / J.words), w = (int)(wave - (size_t)tile * J.words), lane = threadIdx.x & 63;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  // the pixels a tile's groups can hold, whatever the rows' phases: 64 tx - 4 .. 64 tx + 62
  const int x0 = tx * (PP_TILE_GROUPS * 4) - 4, x1 = x0 + PP_TILE_GROUPS * 4 + 2, y0 = ty * PP_TILE_ROWS, y1 = y0 + PP_TILE_ROWS - 1;
  const int p = w * 64 + lane;
  bool hit = false;
  if (p < J.np) {
    const int4 b = boxes[(size_t)J.p0 + p];             // x0, y0, x1, y1 inclusive; empty: x0 > x1
    hit = b.x <= b.z && b.x <= x1 && b.z >= x0 && b.y <= y1 && b.w >= y0;
  }
  const pp_u64 bits = __ballot(hit);
  if (lane == 0) mat[J.moff + wave] = bits;
}

__device__ __forceinline__ bool pp_covers(int px, int py, int ax, int ay, int dx, int dy, long long L2, long long r2, pp_u64 r2L2) {
  const int qx = px - ax, qy = py - ay;
  const long long t = (long long)qx * dx + (long long)qy * dy;
  if (t <= 0) return (long long)qx * qx + (long long)qy * qy <= r2;
  if (t >= L2) {
    const int ex = qx - dx, ey = qy - dy;
    return (long long)ex * ex + (long long)ey * ey <= r2;
  }
  const long long c = (long long)qx * dy - (long long)qy * dx;
  return (pp_u64)(c * c) <= r2L2;
}

__device__ __forceinline__ uint32_t pp_blend(uint32_t in, uint32_t add, uint32_t ib) {      // add = ink * a + 128, ib = 255 - a
  const uint32_t v = in * ib + add;
  return ((v >> 8) + v) >> 8;
}

// grid (tiles of a frame, jobs of the batch)
__global__ __launch_bounds__(256) void pp_paint_kernel(uint8_t* __restrict__ frames, int H, int W, int tiles_x, const pp_job* __restrict__ jobs, int j0,
                                                       const pp_rec* __restrict__ recs, const pp_u64* __restrict__ mat) {
  const pp_job J = jobs[j0 + blockIdx.y];
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int tx0 = tx * (PP_TILE_GROUPS * 4) - 4, tx1 = tx0 + PP_TILE_GROUPS * 4 + 2, ty0 = ty * PP_TILE_ROWS, ty1 = ty0 + PP_TILE_ROWS - 1;
  const int py = ty0 + (int)(threadIdx.x >> 4);
  if (py >= H) return;                                  // no barrier below
  uint8_t* row = frames + ((size_t)J.frame * H + py) * (size_t)W * 3;
  const int phi = (int)((uintptr_t)row & 3);
  const int xs = phi + 4 * (tx * PP_TILE_GROUPS + (int)(threadIdx.x & 15) - 1);
  unsigned valid = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) valid |= (unsigned)(xs + i >= 0 && xs + i < W) << i;
  if (!valid) return;
  const bool whole = valid == 15u;                      // three aligned dwords
  uint8_t* at = row + (ptrdiff_t)xs * 3;
  uint32_t px[3] = {0, 0, 0};
  bool have = J.clear != 0;

  const pp_u64* words = mat + J.moff + (size_t)tile * J.words;
  for (int w = 0; w < J.words; ++w) {                   // uniform
    pp_u64 bits = words[w];
    while (bits) {
      const pp_rec& R = recs[(size_t)J.p0 + w * 64 + __builtin_ctzll(bits)];
      bits &= bits - 1;
      const pp_u64 shapes = (pp_u64)R.shapes_lo | (pp_u64)R.shapes_hi << 32;
      unsigned cov = 0;
#pragma unroll
      for (int s = 0; s < PP_SHAPES; ++s) {
        if (!((shapes >> s) & 1)) continue;             // uniform
        const int ja = s < 18 ? PP_A[s] : s - 18, jb = s < 18 ? PP_B[s] : s - 18;
        const int r = R.r[s < 18 ? PP_SEG_CLASS[s] : PP_JOINT_CLASS[s - 18]];
        const int ax = R.x[ja], ay = R.y[ja], bx = R.x[jb], by = R.y[jb];
        const int sx0 = min(ax, bx) - r, sx1 = max(ax, bx) + r, sy0 = min(ay, by) - r, sy1 = max(ay, by) + r;
        if (sx1 < tx0 || sx0 > tx1 || sy1 < ty0 || sy0 > ty1) continue;      // uniform
        if (py >= sy0 && py <= sy1) {
          const int dx = bx - ax, dy = by - ay;
          const long long L2 = (long long)dx * dx + (long long)dy * dy, r2 = (long long)r * r;
          const pp_u64 r2L2 = (pp_u64)r2 * (pp_u64)L2;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int x = xs + i;
            if (!((cov >> i) & 1) && x >= sx0 && x <= sx1 && pp_covers(x, py, ax, ay, dx, dy, L2, r2, r2L2)) cov |= 1u << i;
          }
        }
        if (__all((cov & valid) == valid)) break;       // the wave's pixels are all covered: no further shape of this pose
      }
      cov &= valid;
      if (!cov) continue;
      if (!have) {
        have = true;
        if (whole) {
          const uint32_t* q = (const uint32_t*)at;
          px[0] = q[0], px[1] = q[1], px[2] = q[2];
        } else {
#pragma unroll
          for (int b = 0; b < 12; ++b)
            if ((valid >> (b / 3)) & 1) px[b >> 2] |= (uint32_t)at[b] << (8 * (b & 3));
        }
      }
      const uint32_t a = R.rgba >> 24, ib = 255u - a;
      const uint32_t add[3] = {(R.rgba & 255u) * a + 128u, ((R.rgba >> 8) & 255u) * a + 128u, ((R.rgba >> 16) & 255u) * a + 128u};
#pragma unroll
      for (int b = 0; b < 12; ++b) {
        if (!((cov >> (b / 3)) & 1)) continue;
        const int sh = 8 * (b & 3);
        const uint32_t out = pp_blend((px[b >> 2] >> sh) & 255u, add[b % 3], ib);
        px[b >> 2] = (px[b >> 2] & ~(255u << sh)) | out << sh;
      }
    }
  }
  if (!have) return;
  if (whole) {
    uint32_t* q = (uint32_t*)at;
    q[0] = px[0], q[1] = px[1], q[2] = px[2];
  } else {
#pragma unroll
    for (int b = 0; b < 12; ++b)
      if ((valid >> (b / 3)) & 1) at[b] = (uint8_t)(px[b >> 2] >> (8 * (b & 3)));
  }
}

}  // namespace

extern "C" int ta_poses_paint(ta_ctx* ctx, ta_frames* frames, int n_frames, const int32_t* pose_counts, const int32_t* keypoints, const uint8_t* rgba,
                              int n_poses, const int32_t radius_permille[3], int min_radius, int clear) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_TRY(ta_check_batch(ctx, "poses_paint", frames, pose_counts, n_frames));
  if (n_poses < 0 || !radius_permille) return ta_fail(ctx, TA_E_INVALID, "poses_paint: bad args");
  if (n_poses > 0 && (!keypoints || !rgba)) return ta_fail(ctx, TA_E_INVALID, "poses_paint: a null array that has rows");
  const int H = frames->h, W = frames->w;
  if (n_frames > frames->n) return ta_fail(ctx, TA_E_INVALID, "poses_paint: %d frames listed, the batch has %d", n_frames, frames->n);
  if (H > PP_SIDE_LIMIT || W > PP_SIDE_LIMIT) return ta_fail(ctx, TA_E_INVALID, "poses_paint: frames of %d x %d, the limit is %d a side", W, H, PP_SIDE_LIMIT);
  for (int c = 0; c < 3; ++c)
    if (radius_permille[c] < 0 || radius_permille[c] > 1000)
      return ta_fail(ctx, TA_E_INVALID, "poses_paint: radius_permille[%d] = %d is outside 0 .. 1000", c, radius_permille[c]);
  if (min_radius < 0 || min_radius > PP_MIN_RADIUS_LIMIT)
    return ta_fail(ctx, TA_E_INVALID, "poses_paint: min_radius %d is outside 0 .. %d", min_radius, PP_MIN_RADIUS_LIMIT);
  long long P = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (pose_counts[f] < 0) return ta_fail(ctx, TA_E_INVALID, "poses_paint: frame %d: negative count (%d poses)", f, pose_counts[f]);
    P += pose_counts[f];
  }
  if (P != n_poses) return ta_fail(ctx, TA_E_INVALID, "poses_paint: the counts sum to %lld poses, the arrays have %d rows", P, n_poses);
  for (int f = 0; f < n_frames; ++f)
    if (pose_counts[f] > PP_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "poses_paint: frame %d has %d poses, the limit per frame is %d", f, pose_counts[f], PP_MAX_PER_FRAME);
  for (long long r = 0; r < P; ++r) {
    const int32_t* q = keypoints + r * 54;
    unsigned wild = 0;                                  // |v| < 2^14  <=>  (unsigned)(v + 2^14 - 1) < 2^15 - 1
    for (int j = 0; j < 18; ++j)
      wild |= (unsigned)((unsigned)q[j * 3] + (PP_COORD_LIMIT - 1) >= 2u * PP_COORD_LIMIT - 1u) | (unsigned)((unsigned)q[j * 3 + 1] + (PP_COORD_LIMIT - 1) >= 2u * PP_COORD_LIMIT - 1u);
    if (wild) return ta_fail(ctx, TA_E_INVALID, "poses_paint: pose row %lld has a coordinate that is not below 2^14 in size", r);
  }
  if (n_frames == 0 || (P == 0 && !clear)) return TA_OK;

  // a record and a box per pose
  std::vector<pp_rec> recs((size_t)P);
  std::vector<int4> boxes((size_t)P);
  for (long long k = 0; k < P; ++k) {
    const int32_t* q = keypoints + k * 54;
    pp_rec& R = recs[(size_t)k];
    memset(&R, 0, sizeof R);
    unsigned mask = 0;
    int bx0 = INT32_MAX, bx1 = INT32_MIN, by0 = INT32_MAX, by1 = INT32_MIN;
    for (int j = 0; j < 18; ++j) {
      if (q[j * 3 + 2] == 0) continue;
      mask |= 1u << j;
      R.x[j] = q[j * 3], R.y[j] = q[j * 3 + 1];
      bx0 = std::min(bx0, R.x[j]), bx1 = std::max(bx1, R.x[j]), by0 = std::min(by0, R.y[j]), by1 = std::max(by1, R.y[j]);
    }
    const uint8_t* ink = rgba + k * 4;
    R.rgba = (uint32_t)ink[0] | (uint32_t)ink[1] << 8 | (uint32_t)ink[2] << 16 | (uint32_t)ink[3] << 24;
    boxes[(size_t)k] = make_int4(1, 1, 0, 0);
    if (!mask) continue;
    const long long M = std::max(bx1 - bx0, by1 - by0);
    int rmax = 0;
    for (int c = 0; c < 3; ++c) {
      R.r[c] = (int32_t)std::max<long long>(min_radius, M * radius_permille[c] / 1000);
      rmax = std::max(rmax, R.r[c]);
    }
    pp_u64 shapes = 0;
    int cap[18];                                        // the largest radius of a present segment that ends at the joint
    for (int j = 0; j < 18; ++j) cap[j] = -1;
    for (int s = 0; s < 18; ++s)
      if ((mask >> PP_A[s]) & (mask >> PP_B[s]) & 1u) {
        shapes |= (pp_u64)1 << s;
        cap[PP_A[s]] = std::max(cap[PP_A[s]], R.r[PP_SEG_CLASS[s]]);
        cap[PP_B[s]] = std::max(cap[PP_B[s]], R.r[PP_SEG_CLASS[s]]);
      }
    for (int j = 0; j < 18; ++j)
      if (((mask >> j) & 1u) && cap[j] < R.r[PP_JOINT_CLASS[j]]) shapes |= (pp_u64)1 << (18 + j);
    R.shapes_lo = (uint32_t)shapes, R.shapes_hi = (uint32_t)(shapes >> 32);
    if (ink[3] == 0) continue;                          // changes nothing: touches no tile
    const int x0 = std::max(bx0 - rmax, 0), y0 = std::max(by0 - rmax, 0), x1 = std::min(bx1 + rmax, W - 1), y1 = std::min(by1 + rmax, H - 1);
    if (x0 <= x1 && y0 <= y1) boxes[(size_t)k] = make_int4(x0, y0, x1, y1);
  }

  // jobs, and the batches of them whose matrices fit the budget: at most 65535 a batch (grid.y), a frame once a batch
  const int groups = (W + 3) / 4 + 1;                   // a head, then the aligned groups, the last maybe a tail
  const int tiles_x = (groups + PP_TILE_GROUPS - 1) / PP_TILE_GROUPS, tiles_y = (H + PP_TILE_ROWS - 1) / PP_TILE_ROWS;
  const size_t tiles = (size_t)tiles_x * tiles_y;
  size_t budget = PP_MATRIX_BYTES / 8;
  if (const char* e = getenv("TA_PP_MATRIX_BYTES")) budget = (size_t)strtoull(e, nullptr, 10) / 8;     // tests: many batches at small sizes
  std::vector<pp_job> jobs;
  std::vector<int> batch_end;
  size_t mat_words = 0, batch_words = 0;
  {
    long long off = 0;
    int b0 = 0;
    for (int f = 0; f < n_frames; off += pose_counts[f], ++f) {
      const int nf = pose_counts[f];
      if (nf == 0 && !clear) continue;
      const int words_f = (nf + 63) / 64;
      const int run = tiles * words_f > budget ? (int)std::max<size_t>(1, budget / tiles) : std::max(words_f, 1);    // words of a run of poses
      for (int w0 = 0; w0 == 0 || w0 < words_f; w0 += run) {
        pp_job J;
        memset(&J, 0, sizeof J);
        J.frame = f, J.p0 = (int32_t)(off + (long long)w0 * 64), J.np = std::min(nf - w0 * 64, run * 64), J.words = (J.np + 63) / 64;
        J.clear = clear && w0 == 0;
        const size_t need = tiles * J.words;
        if ((int)jobs.size() > b0 && (batch_words + need > budget || w0 > 0 || (int)jobs.size() - b0 >= 65535)) {
          batch_end.push_back((int)jobs.size());
          b0 = (int)jobs.size();
          batch_words = 0;
        }
        J.moff = batch_words;
        batch_words += need;
        mat_words = std::max(mat_words, batch_words);
        jobs.push_back(J);
      }
    }
  }
  if (jobs.empty()) return TA_OK;
  batch_end.push_back((int)jobs.size());

  ta_staging st;
  const size_t o_jobs = st.put(jobs), o_boxes = st.put(boxes), o_recs = st.put(recs, 64);
  const size_t o_mat = st.device_only(mat_words * 8);
  TA_TRY(st.commit(ctx));
  const pp_job* djobs = st.dev<const pp_job>(o_jobs);
  pp_u64* dmat = st.dev<pp_u64>(o_mat);
  for (size_t b = 0, j0 = 0; b < batch_end.size(); j0 = batch_end[b++]) {
    const int nj = batch_end[b] - (int)j0;
    int max_words = 0;
    for (int j = (int)j0; j < batch_end[b]; ++j) max_words = std::max(max_words, jobs[j].words);
    if (max_words > 0) {
      const size_t waves = tiles * max_words;
      hipLaunchKernelGGL(pp_bin_kernel, dim3((unsigned)((waves + 3) / 4), (unsigned)nj), dim3(256), 0, ctx->stream, djobs, (int)j0,
                         st.dev<const int4>(o_boxes), tiles_x, (int)tiles, dmat);
      TA_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(pp_paint_kernel, dim3((unsigned)tiles, (unsigned)nj), dim3(256), 0, ctx->stream, frames->dev, H, W, tiles_x, djobs, (int)j0,
                       st.dev<const pp_rec>(o_recs), (const pp_u64*)dmat);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));       // pinned / scratch staging is reused by the next call
  return TA_OK;
}
