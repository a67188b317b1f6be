// Tracked rows of consecutive frames -> the same rows with the frames and points a track missed filled in (ta_tracks_fill).
//
//  link     a = prev[b], d = frame(b) - frame(a) >= 1; G = max_gap + 1; no two rows share a predecessor: a chain is a line
//  rows     the real rows of a frame first, in input order; a link with 2 <= d <= G adds a synthesized row to every frame
//           strictly between its ends, a frame's synthesized rows ordered by their link's b
//  points   a present point of a real row is copied; every other point of an output row at frame t looks for the nearest row of
//           its chain before t and the nearest after t that have the point, and if they are at most G frames apart it is
//           v0 + floor((2 (v1 - v0)(t - t0) + (t1 - t0)) / (2 (t1 - t0))) with the third value `mark`; else (0, 0, 0)
//
// Everything the answer's SHAPE depends on (the rows a frame gains, the offsets of the frames in the output) is a sum over
// frames that the host's validation pass has to make anyway: it walks prev once to check it.  The device gets the two
// exclusive scans (input rows, output rows) and does what grows with rows x points:
//  1. tf_link_kernel    a thread per row: frame(row) by bisection of the input scan, next[prev[row]] = row.  next is set to -1
//                       by a memset in front; a row has one successor at most (checked), so every word has one writer.
//  2. tf_rank_kernel    a workgroup per frame t.  It writes (r, r) for t's real rows, then walks the global rows of the frames
//                       t + 1 .. t + G - 1 -- a link that spans t and adds rows ends there -- in order, 256 at a time: a row
//                       spans t iff frame(prev) < t and d <= G; its rank is the running base + the waves before it (four
//                       counts through LDS) + the lanes before it in its wave's ballot.  Global rows ascend along the walk, so
//                       the rank is the order by b; no atomics, and nothing another workgroup does is waited for.
//  3. tf_points_kernel  a thread per (output row, point), 256 consecutive ones a workgroup: reads and writes run along the
//                       arrays.  A thread that has to fill walks prev, then next, and stops at the first row outside the
//                       window: frames strictly descend along prev (checked), so each walk takes G steps at most.  The point
//                       leaves as three consecutive words.
// The three are separate launches on the context's stream; the order between them is the stream's.
//
// Exactness.  |x|, |y| < 2^22 (checked, every point of every row), |v1 - v0| < 2^23, t - t0 <= 30, t1 - t0 <= 31: the numerator
// is below 2^23 * 31 * 2 + 31 < 2^29 in size, int32 holds it; no float appears anywhere.
#include <string.h>

#include <vector>

#include "frame_regions.h"

#define TF_MAX_PER_FRAME 16384
#define TF_COORD_LIMIT (1 << 22)
#define TF_THREADS 256

namespace {

typedef unsigned long long tf_u64;

__global__ __launch_bounds__(TF_THREADS) void tf_link_kernel(const int32_t* __restrict__ roff, int n_frames, const int32_t* __restrict__ prev, int P,
                                                             int32_t* __restrict__ next, int32_t* __restrict__ frame) {
  const int r = blockIdx.x * TF_THREADS + threadIdx.x;
  if (r >= P) return;
  int lo = 0, hi = n_frames;                            // the largest f with roff[f] <= r: empty frames in front of it are passed
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (roff[mid] <= r) lo = mid; else hi = mid;
  }
  frame[r] = lo;
  const int a = prev[r];
  if (a >= 0) next[a] = r;
}

// grid: the frames
__global__ __launch_bounds__(TF_THREADS) void tf_rank_kernel(const int32_t* __restrict__ roff, const int32_t* __restrict__ ooff, int n_frames,
                                                             const int32_t* __restrict__ prev, const int32_t* __restrict__ frame, int G,
                                                             int32_t* __restrict__ src, int32_t* __restrict__ oframe) {
  __shared__ int wave_sum[TF_THREADS / 64];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = roff[t], n = roff[t + 1] - r0;
  const size_t o0 = (size_t)ooff[t];
  for (int k = tid; k < n; k += TF_THREADS) {
    src[(o0 + k) * 2] = r0 + k, src[(o0 + k) * 2 + 1] = r0 + k;
    oframe[o0 + k] = t;
  }
  const int b0 = roff[t + 1], b1 = roff[min(t + G, n_frames)];
  int base = 0;
  for (int c = b0; c < b1; c += TF_THREADS) {           // uniform
    const int b = c + tid;
    int a = -1;
    bool spans = false;
    if (b < b1) {
      a = prev[b];
      if (a >= 0) {
        const int fa = frame[a];
        spans = fa < t && frame[b] - fa <= G;
      }
    }
    const tf_u64 m = __ballot(spans);
    if (lane == 0) wave_sum[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < TF_THREADS / 64; ++k) {
      const int s = wave_sum[k];
      before += k < w ? s : 0, all += s;
    }
    if (spans) {                                        // the host counted the same rows: o stays below ooff[t + 1]
      const size_t o = o0 + n + base + before + __popcll(m & (((tf_u64)1 << lane) - 1));
      src[o * 2] = a, src[o * 2 + 1] = b;
      oframe[o] = t;
    }
    base += all;
    __syncthreads();                                    // wave_sum is written again
  }
}

struct tf_point {
  int32_t x, y, p;
};

// floor((2 dv k + dt) / (2 dt)), dt > 0
__device__ __forceinline__ int tf_step(int dv, int k, int dt) {
  const int num = 2 * dv * k + dt, den = 2 * dt;
  const int q = num / den;
  return q - (num % den < 0 ? 1 : 0);
}

__global__ __launch_bounds__(TF_THREADS) void tf_points_kernel(const tf_point* __restrict__ points, const int32_t* __restrict__ prev,
                                                               const int32_t* __restrict__ next, const int32_t* __restrict__ frame,
                                                               const int32_t* __restrict__ src, const int32_t* __restrict__ oframe, size_t total,
                                                               int np, int G, int mark, tf_point* __restrict__ out) {
  const size_t first = (size_t)blockIdx.x * TF_THREADS;             // uniform: one 64-bit division a workgroup
  const size_t R0 = first / (unsigned)np;
  const unsigned l = threadIdx.x + (unsigned)(first - R0 * (unsigned)np);
  const size_t R = R0 + l / (unsigned)np;
  const int j = (int)(l % (unsigned)np);
  const size_t i = first + threadIdx.x;
  if (i >= total) return;
  const int a = src[R * 2], b = src[R * 2 + 1], t = oframe[R];
  int back = a, fwd = b;
  if (a == b) {
    const tf_point q = points[(size_t)a * np + j];
    if (q.p != 0) {
      out[i] = q;
      return;
    }
    back = prev[a], fwd = next[a];
  }
  tf_point v = {0, 0, 0};
  int t0 = 0, x0 = 0, y0 = 0;
  bool have = false;
  while (back >= 0) {
    const int f = frame[back];
    if (t - f >= G) break;                              // t1 >= t + 1: nothing this far back can close within G
    const tf_point q = points[(size_t)back * np + j];
    if (q.p != 0) {
      have = true, t0 = f, x0 = q.x, y0 = q.y;
      break;
    }
    back = prev[back];
  }
  while (have && fwd >= 0) {
    const int f = frame[fwd];
    if (f - t0 > G) break;
    const tf_point q = points[(size_t)fwd * np + j];
    if (q.p != 0) {
      v.x = x0 + tf_step(q.x - x0, t - t0, f - t0);
      v.y = y0 + tf_step(q.y - y0, t - t0, f - t0);
      v.p = mark;
      break;
    }
    fwd = next[fwd];
  }
  out[i] = v;
}

}  // namespace

extern "C" int ta_tracks_fill(ta_ctx* ctx, int n_frames, const int32_t* counts, const int32_t* points, int n_points, const int32_t* prev, int n_rows,
                              int max_gap, int mark, int32_t* out_counts, int32_t* out_points, int32_t* out_source, int out_capacity, int32_t* n_out) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_frames < 0 || n_rows < 0 || out_capacity < 0) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: bad args");
  if (n_points < 1 || n_points > 18) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: n_points %d is outside 1 .. 18", n_points);
  if (max_gap < 0 || max_gap > 30) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: max_gap %d is outside 0 .. 30", max_gap);
  if (mark < 1 || mark > 255) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: mark %d is outside 1 .. 255", mark);
  if ((n_frames > 0 && !counts) || (n_rows > 0 && (!points || !prev))) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: a null array that has rows");
  const int G = max_gap + 1;
  std::vector<int32_t> roff((size_t)n_frames + 1, 0);
  {
    long long P = 0;
    for (int f = 0; f < n_frames; ++f) {
      if (counts[f] < 0) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: frame %d: negative count (%d rows)", f, counts[f]);
      P += counts[f];
      roff[f + 1] = (int32_t)std::min<long long>(P, INT32_MAX);
    }
    if (P != n_rows) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: the counts sum to %lld rows, the arrays have %d", P, n_rows);
  }
  for (int f = 0; f < n_frames; ++f)
    if (counts[f] > TF_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "tracks_fill: frame %d has %d rows, the limit per frame is %d", f, counts[f], TF_MAX_PER_FRAME);
  const size_t nP = (size_t)n_rows, W = (size_t)n_points * 3;
  for (size_t r = 0; r < nP; ++r) {
    const int32_t* q = points + r * W;
    unsigned wild = 0;                                  // |v| < 2^22  <=>  (unsigned)(v + 2^22 - 1) < 2^23 - 1
    for (int j = 0; j < n_points; ++j)
      wild |= (unsigned)((unsigned)q[j * 3] + (TF_COORD_LIMIT - 1) >= 2u * TF_COORD_LIMIT - 1u) | (unsigned)((unsigned)q[j * 3 + 1] + (TF_COORD_LIMIT - 1) >= 2u * TF_COORD_LIMIT - 1u);
    if (wild) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: row %zu has a coordinate that is not below 2^22 in size", r);
  }
  // prev: a row of an earlier frame, nobody's predecessor twice; the rows every frame gains (a difference array over the frames)
  std::vector<int32_t> frame_of(nP), gain((size_t)n_frames + 1, 0);
  std::vector<uint8_t> taken(nP, 0);
  for (int f = 0; f < n_frames; ++f)
    for (int32_t r = roff[f]; r < roff[f + 1]; ++r) frame_of[r] = f;
  for (size_t b = 0; b < nP; ++b) {
    const int32_t a = prev[b];
    if (a == -1) continue;
    if (a < 0 || a >= roff[frame_of[b]])
      return ta_fail(ctx, TA_E_INVALID, "tracks_fill: prev[%zu] = %d is neither -1 nor a row of an earlier frame", b, a);
    if (taken[a]) return ta_fail(ctx, TA_E_INVALID, "tracks_fill: row %d is the prev of two rows (the second is %zu)", a, b);
    taken[a] = 1;
    const int fa = frame_of[a], fb = frame_of[b];
    if (fb - fa >= 2 && fb - fa <= G) ++gain[fa + 1], --gain[fb];
  }
  std::vector<int32_t> ooff((size_t)n_frames + 1, 0), oc((size_t)n_frames, 0);
  long long need = 0;
  for (int f = 0, g = 0; f < n_frames; ++f) {
    g += gain[f];
    oc[f] = counts[f] + g;
    if (oc[f] > TF_MAX_PER_FRAME)
      return ta_fail(ctx, TA_E_OVERFLOW, "tracks_fill: frame %d would have %d rows, the limit per frame is %d", f, oc[f], TF_MAX_PER_FRAME);
    need += oc[f];
    ooff[f + 1] = (int32_t)std::min<long long>(need, INT32_MAX);
  }
  if (need > INT32_MAX) {
    if (n_out) *n_out = INT32_MAX;
    return ta_fail(ctx, TA_E_OVERFLOW, "tracks_fill: %lld output rows, the limit of a call is 2^31 - 1", need);
  }
  if (n_out) *n_out = (int32_t)need;
  if (need > out_capacity) return ta_fail(ctx, TA_E_OVERFLOW, "tracks_fill: %lld output rows, out_capacity is %d", need, out_capacity);
  if ((n_frames > 0 && !out_counts) || (need > 0 && (!out_points || !out_source)))
    return ta_fail(ctx, TA_E_INVALID, "tracks_fill: a null output array that has rows");
  if (need == 0) {
    for (int f = 0; f < n_frames; ++f) out_counts[f] = 0;
    return TA_OK;
  }

  const size_t nO = (size_t)need, total = nO * (size_t)n_points;      // need > 0 has n_rows > 0: a synthesized row has a link
  ta_staging st;
  const size_t o_roff = st.put(roff), o_ooff = st.put(ooff);
  const size_t o_prev = st.put(prev, nP * 4), o_points = st.put(points, nP * W * 4);
  const size_t o_rows = st.device_only(nP * 4 * 2);     // next | frame
  const size_t o_src = st.device_only(nO * 4 * 3);      // out_source | the frame of every output row
  const size_t o_out = st.device_only(total * 12);
  const size_t h_src = st.host_only(nO * 8), h_out = st.host_only(total * 12);
  TA_TRY(st.commit(ctx));
  const int32_t *droff = st.dev<const int32_t>(o_roff), *dooff = st.dev<const int32_t>(o_ooff), *dprev = st.dev<const int32_t>(o_prev);
  int32_t* next = st.dev<int32_t>(o_rows);
  int32_t* frame = next + nP;
  int32_t* src = st.dev<int32_t>(o_src);
  int32_t* oframe = src + nO * 2;
  tf_point* out = st.dev<tf_point>(o_out);
  ctx->cur_flops = 0;
  TA_HIP(ctx, hipMemsetAsync(next, 0xff, nP * 4, ctx->stream));       // -1: no successor
  {
    ta_prof_scope scope(ctx, 3, (double)nP);
    ctx->note_kernel("tf_link_kernel");
    hipLaunchKernelGGL(tf_link_kernel, dim3((unsigned)((nP + TF_THREADS - 1) / TF_THREADS)), dim3(TF_THREADS), 0, ctx->stream, droff, n_frames, dprev,
                       (int)n_rows, next, frame);
    TA_HIP(ctx, hipGetLastError());
  }
  {
    ta_prof_scope scope(ctx, 3, (double)nP * G);
    ctx->note_kernel("tf_rank_kernel");
    hipLaunchKernelGGL(tf_rank_kernel, dim3((unsigned)n_frames), dim3(TF_THREADS), 0, ctx->stream, droff, dooff, n_frames, dprev,
                       (const int32_t*)frame, G, src, oframe);
    TA_HIP(ctx, hipGetLastError());
  }
  {
    ta_prof_scope scope(ctx, 3, (double)total);
    ctx->note_kernel("tf_points_kernel");
    hipLaunchKernelGGL(tf_points_kernel, dim3((unsigned)((total + TF_THREADS - 1) / TF_THREADS)), dim3(TF_THREADS), 0, ctx->stream,
                       st.dev<const tf_point>(o_points), dprev, (const int32_t*)next, (const int32_t*)frame, (const int32_t*)src,
                       (const int32_t*)oframe, total, n_points, G, mark, out);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipMemcpyAsync(st.host<void>(h_src), src, nO * 8, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(st.host<void>(h_out), out, total * 12, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out_counts, oc.data(), (size_t)n_frames * 4);
  memcpy(out_source, st.host<void>(h_src), nO * 8);
  memcpy(out_points, st.host<void>(h_out), total * 12);
  return TA_OK;
}
