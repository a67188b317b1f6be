// Faces and skeletons of many frames -> which face belongs to which skeleton (ta_faces_poses_link).
//
//  head     joints 0, 14, 15, 16, 17 (nose, eyes, ears); present iff kp[j][2] != 0; n = present head joints
//  box      w = x1 - x0, h = y1 - y0 (a negative one holds nothing); mx = w * margin_permille / 1000, my likewise; a joint is inside
//           iff x0 - mx <= x <= x1 + mx and y0 - my <= y <= y1 + my
//  pair     qualifies iff inside >= min_inside and 2 * inside >= n
//  cost     S = sum over ALL present head joints of (2x - cx)^2 + (2y - cy)^2, cx = x0 + x1, cy = y0 + y1; cost = S * (60 / n)
//  match    the qualifying pairs of a frame in the order (cost, f, p); a pair links iff both its ends are still free
//
// Greedy matching over a strict total order equals committing every mutually best pair again and again: a pair that is the
// cheapest free pair of its face and of its pose is cheaper than every pair it conflicts with, so the sorted walk takes it first.
// Whether a pair qualifies does not change from round to round, so the O(F * P * 5) scan runs ONCE and leaves a bit matrix; the
// rounds walk its few set bits.
//  1. fl_pack_kernel    a thread per face and per pose: the widened box (lo / hi per axis, an empty interval for a negative
//                       box); the five head joints WORD-MAJOR (planes of one int32 per pose: 5 x, 5 y, presence mask, the head's
//                       extent), so that 64 consecutive poses of one word are one 256-byte line.  An absent joint gets
//                       x = INT32_MIN, which lies in no box: the scan needs no mask.
//  2. fl_matrix_kernel  a workgroup per 64 faces x 256 poses, many per frame.  The 64 widened boxes sit in LDS (1 KiB, every read
//                       one address for the whole wave: a broadcast); lane = pose keeps its joints and extent in registers (they
//                       come straight from the planes, coalesced, and are used 64 times).  A face whose box meets no lane's head
//                       extent skips the joint test.  The ballot is the face's row word; each lane collects its own bit per face
//                       into the pose's row word of the TRANSPOSED matrix, so both sides get rows and nothing is combined across
//                       waves.  Words are stored word-major (word w of row r at [w][r]): a wave's 64 rows write, and later read,
//                       consecutive addresses.
//  3. fl_best_kernel    a thread per free face and per free pose walks its row and keeps the cheapest free partner by (cost,
//                       index): ascending index and a strict compare on the whole int64 cost, nothing packed or shortened.  No
//                       atomics, no reduction across lanes: the answer cannot depend on an order of arrival.
//  4. fl_commit_kernel  a thread per face links mutual choices; a free row with no free partner left is retired for the rest of
//                       the call (partners only ever get fewer).  One counter per round says whether anything was linked.
// Steps 3 and 4 are launched FL_FIRST_ROUNDS, then FL_MORE_ROUNDS rounds at a time with one read of their counters behind them:
// the rounds behind the first silent one find every row linked or retired and do nothing.  A round thus costs two small
// launches and a fraction of a synchronisation.  Frames are independent; the matrices of a call are cut in batches of frames
// that fit FL_MATRIX_BYTES of scratch, as ta_poses_merge does.
//
// Exactness.  Everything is integer.  |x|, |y| and every box coordinate are below 2^22 (checked), so w, h < 2^23, mx, my <= 4 w
// < 2^25 and the widened box within +-2^26: int32.  |2x - cx| < 2^23 + 2^23 = 2^24, a square below 2^48, a joint's two below 2^49,
// S < n * 2^49 and cost = S * (60 / n) < 60 * 2^49 < 2^55: int64 holds it.  (Costs pass 2^53; they happen to be multiples of 4,
// so a double would hold them too -- nothing here relies on that.)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "frame_regions.h"

#define FL_MAX_PER_FRAME 16384                    // faces, and poses, of one frame: the limit of the two merge calls that feed it
#define FL_MATRIX_BYTES ((size_t)256 << 20)       // scratch the matrices of one batch of frames may take (one frame at the limit: 64 MiB)
#define FL_COORD_LIMIT (1 << 22)
#define FL_FIRST_ROUNDS 4
#define FL_MORE_ROUNDS 16
#define FL_POSE_CHUNK 256                         // poses of one workgroup of the scan: 64 per wave
// planes of a packed pose
#define FL_X 0
#define FL_Y 5
#define FL_MASK 10
#define FL_BX0 11
#define FL_BX1 12
#define FL_BY0 13
#define FL_BY1 14
#define FL_WORDS 15
// states of a row in pose_of_face / face_of_pose while the call runs
#define FL_FREE (-1)
#define FL_RETIRED (-2)

namespace {

struct fl_frame {
  int32_t foff, nf;     // its faces: rows foff .. foff + nf - 1 of the face arrays
  int32_t poff, np;     // its poses
  uint64_t moff;        // first word of its face rows (nf x ceil(np / 64) words) within its batch's block
  uint64_t toff;        // ... of its pose rows (np x ceil(nf / 64) words)
};

typedef unsigned long long fl_u64;

// grid: blocks of 256 over the F faces, then over the P poses
__global__ __launch_bounds__(256) void fl_pack_kernel(const int32_t* __restrict__ boxes, int F, const int32_t* __restrict__ kp, int P, int margin,
                                                      int4* __restrict__ wbox, int32_t* __restrict__ planes, int fblocks) {
  if ((int)blockIdx.x < fblocks) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int4 b = ((const int4*)boxes)[f];             // x0, y0, x1, y1
    const int w = b.z - b.x, h = b.w - b.y;
    int4 o = make_int4(INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN);   // x lo, x hi, y lo, y hi: nothing is inside
    if (w >= 0 && h >= 0) {
      const int mx = (int)(((long long)w * margin) / 1000), my = (int)(((long long)h * margin) / 1000);
      o = make_int4(b.x - mx, b.z + mx, b.y - my, b.w + my);
    }
    wbox[f] = o;
    return;
  }
  const int p = ((int)blockIdx.x - fblocks) * 256 + threadIdx.x;
  if (p >= P) return;
  const int head[5] = {0, 14, 15, 16, 17};            // nose, eyes, ears
  int mask = 0, bx0 = INT32_MAX, bx1 = INT32_MIN, by0 = INT32_MAX, by1 = INT32_MIN;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int32_t* q = kp + (size_t)p * 54 + head[j] * 3;
    const bool here = q[2] != 0;
    const int x = here ? q[0] : INT32_MIN, y = here ? q[1] : 0;
    if (here) {
      mask |= 1 << j;
      bx0 = min(bx0, x), bx1 = max(bx1, x), by0 = min(by0, y), by1 = max(by1, y);
    }
    planes[(size_t)(FL_X + j) * P + p] = x;
    planes[(size_t)(FL_Y + j) * P + p] = y;
  }
  planes[(size_t)FL_MASK * P + p] = mask;
  planes[(size_t)FL_BX0 * P + p] = bx0;
  planes[(size_t)FL_BX1 * P + p] = bx1;
  planes[(size_t)FL_BY0 * P + p] = by0;
  planes[(size_t)FL_BY1 * P + p] = by1;
}

// grid (face blocks x pose chunks of the batch's largest frame, frames of the batch)
__global__ __launch_bounds__(256) void fl_matrix_kernel(const fl_frame* __restrict__ frames, int f0, int pchunks, const int4* __restrict__ wbox,
                                                        const int32_t* __restrict__ planes, int P, int min_inside, fl_u64* __restrict__ mat) {
  __shared__ int4 sbox[64];
  const fl_frame F = frames[f0 + blockIdx.y];
  const int I = blockIdx.x / pchunks, chunk = blockIdx.x - I * pchunks;
  if (I * 64 >= F.nf || chunk * FL_POSE_CHUNK >= F.np) return;      // uniform
  if (threadIdx.x < 64) {
    const int f = I * 64 + threadIdx.x;
    sbox[threadIdx.x] = f < F.nf ? wbox[F.foff + f] : make_int4(INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, J = chunk * (FL_POSE_CHUNK / 64) + (threadIdx.x >> 6);
  if (J * 64 >= F.np) return;                           // uniform in the wave, and behind the only barrier
  const int p = J * 64 + lane;
  const bool live = p < F.np;
  const size_t gp = (size_t)F.poff + (live ? p : 0);
  int x[5], y[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) x[j] = planes[(size_t)(FL_X + j) * P + gp], y[j] = planes[(size_t)(FL_Y + j) * P + gp];
  const int n = __popc(planes[(size_t)FL_MASK * P + gp]);
  // a lane behind the frame's poses has an empty extent and meets no box
  const int bx0 = live ? planes[(size_t)FL_BX0 * P + gp] : INT32_MAX, bx1 = live ? planes[(size_t)FL_BX1 * P + gp] : INT32_MIN;
  const int by0 = planes[(size_t)FL_BY0 * P + gp], by1 = planes[(size_t)FL_BY1 * P + gp];
  fl_u64 mine = 0, col = 0;                             // lane k: the row word of face I * 64 + k; lane p: its own bits over the 64 faces
  for (int k = 0; k < 64; ++k) {
    const int4 b = sbox[k];                             // one address for the wave
    // a joint inside the box lies inside the head's extent too: extents that miss the box have inside == 0 < min_inside
    const bool near = bx1 >= b.x && bx0 <= b.y && by1 >= b.z && by0 <= b.w;
    bool q = false;
    if (__ballot(near)) {                               // uniform
      int inside = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) inside += x[j] >= b.x && x[j] <= b.y && y[j] >= b.z && y[j] <= b.w;
      q = near && inside >= min_inside && 2 * inside >= n;
    }
    const fl_u64 m = __ballot(q);
    if (lane == k) mine = m;
    col |= (fl_u64)q << k;
  }
  const int f = I * 64 + lane;
  if (f < F.nf) mat[F.moff + (size_t)J * F.nf + f] = mine;
  if (live) mat[F.toff + (size_t)I * F.np + p] = col;
}

// S * (60 / n) of one box against one pose's present head joints (n >= 1: the pair qualifies)
__device__ __forceinline__ long long fl_cost(int4 box, const int* x, const int* y, int mask) {
  const long long cx = (long long)box.x + box.z, cy = (long long)box.y + box.w;
  long long S = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const long long dx = 2ll * x[j] - cx, dy = 2ll * y[j] - cy;
    S += ((mask >> j) & 1) ? dx * dx + dy * dy : 0ll;
  }
  return S * (60 / __popc(mask));
}

// grid (blocks of 256 rows: the faces, then the poses, of the batch's largest frame; frames of the batch)
__global__ __launch_bounds__(256) void fl_best_kernel(const fl_frame* __restrict__ frames, int f0, int fblocks, const int32_t* __restrict__ boxes,
                                                      const int32_t* __restrict__ planes, int P, const fl_u64* __restrict__ mat,
                                                      const int32_t* __restrict__ pof, const int32_t* __restrict__ fop, int32_t* __restrict__ best_p,
                                                      int32_t* __restrict__ best_f) {
  const fl_frame F = frames[f0 + blockIdx.y];
  long long best = INT64_MAX;
  int who = -1;
  if ((int)blockIdx.x < fblocks) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F.nf || pof[F.foff + f] != FL_FREE) return;
    const int4 box = ((const int4*)boxes)[F.foff + f];
    const int W = (F.np + 63) >> 6;
    for (int w = 0; w < W; ++w) {
      fl_u64 bits = mat[F.moff + (size_t)w * F.nf + f];
      while (bits) {
        const int p = w * 64 + __builtin_ctzll(bits);   // < F.np: the scan sets no bit behind the frame's poses
        bits &= bits - 1;
        if (fop[F.poff + p] >= 0) continue;             // linked (a retired pose has no free partner: it is not met here)
        const size_t gp = (size_t)F.poff + p;
        int x[5], y[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) x[j] = planes[(size_t)(FL_X + j) * P + gp], y[j] = planes[(size_t)(FL_Y + j) * P + gp];
        const long long c = fl_cost(box, x, y, planes[(size_t)FL_MASK * P + gp]);
        if (c < best) best = c, who = p;                // p ascends: of equal costs the lowest stays
      }
    }
    best_p[F.foff + f] = who;
    return;
  }
  const int p = ((int)blockIdx.x - fblocks) * 256 + threadIdx.x;
  if (p >= F.np || fop[F.poff + p] != FL_FREE) return;
  const size_t gp = (size_t)F.poff + p;
  int x[5], y[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) x[j] = planes[(size_t)(FL_X + j) * P + gp], y[j] = planes[(size_t)(FL_Y + j) * P + gp];
  const int mask = planes[(size_t)FL_MASK * P + gp];
  const int W = (F.nf + 63) >> 6;
  for (int w = 0; w < W; ++w) {
    fl_u64 bits = mat[F.toff + (size_t)w * F.np + p];
    while (bits) {
      const int f = w * 64 + __builtin_ctzll(bits);
      bits &= bits - 1;
      if (pof[F.foff + f] >= 0) continue;
      const long long c = fl_cost(((const int4*)boxes)[F.foff + f], x, y, mask);
      if (c < best) best = c, who = f;
    }
  }
  best_f[F.poff + p] = who;
}

// the same grid.  Every row that was free in fl_best_kernel has a fresh choice; so has the partner it chose, which was free too.
__global__ __launch_bounds__(256) void fl_commit_kernel(const fl_frame* __restrict__ frames, int f0, int fblocks, const int32_t* __restrict__ best_p,
                                                        const int32_t* __restrict__ best_f, int32_t* __restrict__ pof, int32_t* __restrict__ fop,
                                                        int* __restrict__ committed) {
  const fl_frame F = frames[f0 + blockIdx.y];
  if ((int)blockIdx.x < fblocks) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool linked = false;
    if (f < F.nf && pof[F.foff + f] == FL_FREE) {
      const int p = best_p[F.foff + f];
      if (p < 0) {
        pof[F.foff + f] = FL_RETIRED;
      } else if (best_f[F.poff + p] == f) {             // only this thread writes these two words in this launch
        pof[F.foff + f] = p;
        fop[F.poff + p] = f;
        linked = true;
      }
    }
    const fl_u64 any = __ballot(linked);
    if (any && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)any) - 1)) atomicAdd(committed, __popcll(any));
    return;
  }
  // a pose that chose nobody: no face chose it either (a face chooses free qualifying partners, and then this pose had one)
  const int p = ((int)blockIdx.x - fblocks) * 256 + threadIdx.x;
  if (p < F.np && best_f[F.poff + p] < 0 && fop[F.poff + p] == FL_FREE) fop[F.poff + p] = FL_RETIRED;
}

}  // namespace

extern "C" int ta_faces_poses_link(ta_ctx* ctx, int n_frames, const int32_t* face_counts, const int32_t* boxes, int n_faces, const int32_t* pose_counts,
                                   const int32_t* keypoints, int n_poses, int margin_permille, int min_inside, int32_t* pose_of_face,
                                   int32_t* face_of_pose, int32_t* links, int32_t* rounds) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_frames < 0 || n_faces < 0 || n_poses < 0 || (n_frames > 0 && (!face_counts || !pose_counts)))
    return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: bad args");
  if ((n_faces > 0 && (!boxes || !pose_of_face)) || (n_poses > 0 && (!keypoints || !face_of_pose)))
    return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: a null array that has rows");
  if (margin_permille < 0 || margin_permille > 4000)
    return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: margin_permille %d is outside 0 .. 4000", margin_permille);
  if (min_inside < 1 || min_inside > 5) return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: min_inside %d is outside 1 .. 5", min_inside);
  long long F = 0, P = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (face_counts[f] < 0 || pose_counts[f] < 0)
      return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: frame %d: negative count (%d faces, %d poses)", f, face_counts[f], pose_counts[f]);
    F += face_counts[f];
    P += pose_counts[f];
  }
  if (F != n_faces || P != n_poses)
    return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: the counts sum to %lld faces and %lld poses, the arrays have %d and %d rows", F, P, n_faces, n_poses);
  std::vector<fl_frame> fr((size_t)n_frames);
  F = P = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (face_counts[f] > FL_MAX_PER_FRAME || pose_counts[f] > FL_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "faces_poses_link: frame %d has %d faces and %d poses, the limit per frame is %d of each", f, face_counts[f],
                     pose_counts[f], FL_MAX_PER_FRAME);
    memset(&fr[f], 0, sizeof(fl_frame));
    fr[f].foff = (int32_t)F, fr[f].nf = face_counts[f];
    fr[f].poff = (int32_t)P, fr[f].np = pose_counts[f];
    F += face_counts[f];
    P += pose_counts[f];
  }
  for (long long k = 0; k < F * 4; ++k)
    if (boxes[k] <= -FL_COORD_LIMIT || boxes[k] >= FL_COORD_LIMIT)
      return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: face row %lld has a coordinate that is not below 2^22 in size", k / 4);
  for (long long r = 0; r < P; ++r) {
    const int32_t* q = keypoints + r * 54;
    unsigned wild = 0;                                  // |v| < 2^22  <=>  (unsigned)(v + 2^22 - 1) < 2^23 - 1
    for (int j = 0; j < 18; ++j)
      wild |= (unsigned)((unsigned)q[j * 3] + (FL_COORD_LIMIT - 1) >= 2u * FL_COORD_LIMIT - 1u) | (unsigned)((unsigned)q[j * 3 + 1] + (FL_COORD_LIMIT - 1) >= 2u * FL_COORD_LIMIT - 1u);
    if (wild) return ta_fail(ctx, TA_E_INVALID, "faces_poses_link: pose row %lld has a coordinate that is not below 2^22 in size", r);
  }

  for (long long k = 0; k < F; ++k) pose_of_face[k] = -1;
  for (long long k = 0; k < P; ++k) face_of_pose[k] = -1;
  if (links)
    for (int f = 0; f < n_frames; ++f) links[f] = 0;
  if (rounds) *rounds = n_frames > 0 ? 1 : 0;           // a frame with nothing to link runs its one silent round in no time
  bool work = false;
  for (const fl_frame& f : fr) work |= f.nf > 0 && f.np > 0;
  if (!work) return TA_OK;

  // batches of frames: matrices within FL_MATRIX_BYTES, at most 65535 frames (grid.y)
  size_t budget = FL_MATRIX_BYTES / 8;
  if (const char* e = getenv("TA_FL_MATRIX_BYTES")) budget = (size_t)strtoull(e, nullptr, 10) / 8;   // tests: many batches at small sizes
  std::vector<int> batch_end;
  size_t mat_words = 0, batch_words = 0;
  for (int f = 0, b0 = 0; f < n_frames; ++f) {
    const size_t wf = (size_t)fr[f].nf * ((fr[f].np + 63) / 64), wp = (size_t)fr[f].np * ((fr[f].nf + 63) / 64);
    if (f > b0 && (batch_words + wf + wp > budget || f - b0 == 65535)) {
      batch_end.push_back(f);
      b0 = f;
      batch_words = 0;
    }
    fr[f].moff = batch_words;
    fr[f].toff = batch_words + wf;
    batch_words += wf + wp;
    mat_words = std::max(mat_words, batch_words);
  }
  batch_end.push_back(n_frames);

  const size_t nF = (size_t)F, nP = (size_t)P;
  ta_staging st;
  const size_t o_fr = st.put(fr);
  const size_t o_boxes = st.put(boxes, nF * 16), o_kp = st.put(keypoints, nP * 216);
  const size_t o_wbox = st.device_only(nF * 16), o_planes = st.device_only(nP * FL_WORDS * 4);
  const size_t o_link = st.device_only((nF + nP) * 4);  // pose_of_face | face_of_pose
  const size_t o_best = st.device_only((nF + nP) * 4);  // each face's choice | each pose's
  const size_t o_cnt = st.device_only(FL_MORE_ROUNDS * 4);
  const size_t o_mat = st.device_only(mat_words * 8);
  const size_t h_cnt = st.host_only(FL_MORE_ROUNDS * 4 + (nF + nP) * 4);
  TA_TRY(st.commit(ctx));
  const fl_frame* dfr = st.dev<const fl_frame>(o_fr);
  const int32_t* dboxes = st.dev<const int32_t>(o_boxes);
  const int32_t* dplanes = st.dev<const int32_t>(o_planes);
  int32_t* pof = st.dev<int32_t>(o_link);
  int32_t* fop = pof + nF;
  int32_t* best_p = st.dev<int32_t>(o_best);
  int32_t* best_f = best_p + nF;
  int* cnt = st.dev<int>(o_cnt);
  int* hcnt = st.host<int>(h_cnt);
  int32_t* hlink = (int32_t*)(hcnt + FL_MORE_ROUNDS);
  TA_HIP(ctx, hipMemsetAsync(pof, 0xff, (nF + nP) * 4, ctx->stream));   // FL_FREE
  {
    const unsigned fb = (unsigned)((nF + 255) / 256), pb = (unsigned)((nP + 255) / 256);
    ta_prof_scope scope(ctx, 3, (double)(nF * 4 + nP * 54));
    ctx->cur_flops = 0;
    ctx->note_kernel("fl_pack_kernel");
    hipLaunchKernelGGL(fl_pack_kernel, dim3(fb + pb), dim3(256), 0, ctx->stream, dboxes, (int)F, st.dev<const int32_t>(o_kp), (int)P, margin_permille,
                       st.dev<int4>(o_wbox), st.dev<int32_t>(o_planes), (int)fb);
    TA_HIP(ctx, hipGetLastError());
  }
  int total_rounds = 1;
  for (size_t b = 0, f0 = 0; b < batch_end.size(); f0 = batch_end[b++]) {
    const int nf = batch_end[b] - (int)f0;
    int max_f = 0, max_p = 0;
    double pairs = 0;
    for (int f = (int)f0; f < batch_end[b]; ++f) {
      max_f = std::max(max_f, fr[f].nf), max_p = std::max(max_p, fr[f].np);
      pairs += (double)fr[f].nf * fr[f].np;
    }
    if (nf == 0 || pairs == 0) continue;
    const unsigned fblocks64 = (unsigned)((max_f + 63) / 64), pchunks = (unsigned)((max_p + FL_POSE_CHUNK - 1) / FL_POSE_CHUNK);
    {
      ta_prof_scope scope(ctx, 3, pairs * 5);
      ctx->note_kernel("fl_matrix_kernel");
      hipLaunchKernelGGL(fl_matrix_kernel, dim3(fblocks64 * pchunks, (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (int)pchunks, st.dev<const int4>(o_wbox),
                         dplanes, (int)P, min_inside, st.dev<fl_u64>(o_mat));
      TA_HIP(ctx, hipGetLastError());
    }
    const unsigned fb = (unsigned)((max_f + 255) / 256), pb = (unsigned)((max_p + 255) / 256);
    // a frame links at most min(nf, np) pairs, one a round at the least, and then runs its silent round
    const int bound = std::min(max_f, max_p) + 1;
    int ran = 0;
    bool silent = false;
    while (!silent) {
      if (ran >= bound) return ta_fail(ctx, TA_E_DEVICE, "faces_poses_link: the links did not settle within %d rounds", bound);
      const int group = ran == 0 ? FL_FIRST_ROUNDS : FL_MORE_ROUNDS;
      TA_HIP(ctx, hipMemsetAsync(cnt, 0, FL_MORE_ROUNDS * 4, ctx->stream));
      for (int r = 0; r < group; ++r) {
        {
          ta_prof_scope scope(ctx, 3, (double)(max_f + max_p) * nf);
          ctx->note_kernel("fl_best_kernel");
          hipLaunchKernelGGL(fl_best_kernel, dim3(fb + pb, (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (int)fb, dboxes, dplanes, (int)P,
                             st.dev<const fl_u64>(o_mat), (const int32_t*)pof, (const int32_t*)fop, best_p, best_f);
          TA_HIP(ctx, hipGetLastError());
        }
        ta_prof_scope scope(ctx, 3, (double)(max_f + max_p) * nf);
        ctx->note_kernel("fl_commit_kernel");
        hipLaunchKernelGGL(fl_commit_kernel, dim3(fb + pb, (unsigned)nf), dim3(256), 0, ctx->stream, dfr, (int)f0, (int)fb, (const int32_t*)best_p,
                           (const int32_t*)best_f, pof, fop, cnt + r);
        TA_HIP(ctx, hipGetLastError());
      }
      TA_HIP(ctx, hipMemcpyAsync(hcnt, cnt, FL_MORE_ROUNDS * 4, hipMemcpyDeviceToHost, ctx->stream));
      TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (int r = 0; r < group && !silent; ++r) {
        ++ran;                                          // rounds up to and including the first that linked nothing
        silent = hcnt[r] == 0;
      }
    }
    total_rounds = std::max(total_rounds, ran);
  }
  TA_HIP(ctx, hipMemcpyAsync(hlink, pof, (nF + nP) * 4, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < nF; ++k) pose_of_face[k] = hlink[k] >= 0 ? hlink[k] : -1;
  for (size_t k = 0; k < nP; ++k) face_of_pose[k] = hlink[nF + k] >= 0 ? hlink[nF + k] : -1;
  if (links)
    for (int f = 0; f < n_frames; ++f)
      for (int k = 0; k < fr[f].nf; ++k) links[f] += pose_of_face[fr[f].foff + k] >= 0;
  if (rounds) *rounds = total_rounds;
  return TA_OK;
}
