// Pillow's Gaussian blur of regions of a resident frame batch, shared by ta_frames_blur (blur.hip) and the unsharp mask of
// ta_frames_filter (filter.hip): the device passes, the host set-up of their weights and the planning of one round.
//
// Pillow's Gaussian blur is three box-blur passes along the rows, then three along the columns, every pass rounded to
// uint8 (libImaging/BoxBlur.c).  A pass over a line p[0..n-1], indices clamped to the line (the region's own border, not
// the frame's):
//   out[x] = (uint8)((sum_{d=-r..r} p[x+d] * ww + (p[x-r-1] + p[x+r+1]) * fw + 2^23) >> 24)     in uint32 arithmetic
// with r, ww, fw derived from the radius by a float set-up that the HOST does here exactly as the C code does it
// (box_params; the including unit is compiled with -ffp-contract=off, build.py): the device sees integers only.
//
// Device side: two launches per round of regions that are pairwise disjoint within their frame.
//   blur_rows: a workgroup takes a strip of rows of one region, runs the three horizontal passes in LDS (bytes, two
//              buffers, ping-pong) and writes the strip to the region's packed image in scratch memory;
//   blur_cols: a workgroup takes a strip of columns (24 pixels = 72 bytes per row unless the region is taller than 1137
//              rows), runs the three vertical passes and writes the frame where the shape's mask covers the pixel:
//              the blurred value, or under UNSHARP libImaging's UnsharpMask of the frame's own value and the blurred one.
// A thread owns a chunk of consecutive outputs of one line and slides the window sum along it: two LDS reads per output
// after the first.  Every output of a pass depends only on the pass's input buffer, so the result does not depend on
// the launch geometry.  The ellipse mask is TA_DRAW_DISC's span table (ta_span_tables, frame_regions.h).
#pragma once
#include "frame_regions.h"

#include <math.h>

namespace {
namespace gauss {

constexpr int LDS_BUDGET = 160 * 1024;     // one workgroup's LDS: both buffers of a strip
constexpr int MAX_SIDE = 16384;            // of a region: one line, twice, within LDS_BUDGET
constexpr int ROW_STRIP = 16;              // rows of a row-stage strip (fewer where 2 x 16 lines outgrow the LDS)
constexpr int COL_STRIP = 24;              // pixels of a column-stage strip: 72 contiguous bytes per row
constexpr int THREADS = 256;
constexpr float MAX_RADIUS = 1024.f;

struct blur_rec {            // 56 bytes
  int32_t frame, x0, y0, w, h;
  int32_t r;                 // box radius, whole part
  uint32_t ww, fw;           // weight of a window pixel and of the two pixels next to the window, 2^24 = 1
  int32_t tab;               // ellipse: first row of the span table; box: -1
  int32_t percent, threshold;   // UNSHARP
  int32_t pad;
  uint64_t scratch;          // byte offset of the region's packed h x 3w image in the pixel scratch
};
static_assert(sizeof(blur_rec) == 56, "blur_rec");

struct blur_item {           // one workgroup's strip
  int32_t rec, start, count; // rows (blur_rows) or pixel columns (blur_cols) start .. start + count - 1 of the region
};

// One box pass src -> dst over the strip's lines.  ALONG_ROWS: line l is channel l % 3 of row l / 3, samples 3 bytes apart;
// otherwise line l is byte column l, samples `pitch` bytes apart.  n samples per line, nl lines.
template <bool ALONG_ROWS>
__device__ inline void box_pass(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int nl, int n, int pitch, int r,
                                uint32_t ww, uint32_t fw) {
  const int k = max(1, min(THREADS / nl, (n + 7) / 8));   // chunks per line: all threads busy, chunks of 8 outputs or more
  const int ch = (n + k - 1) / k;
  const int step = ALONG_ROWS ? 3 : pitch;
  for (int t = threadIdx.x; t < nl * k; t += THREADS) {
    const int l = t % nl, xa = (t / nl) * ch, xb = min(n, xa + ch);
    if (xa >= xb) continue;
    const int base = ALONG_ROWS ? (l / 3) * pitch + l % 3 : l;
    auto at = [&](int i) { return (uint32_t)src[base + min(max(i, 0), n - 1) * step]; };
    const int lo = xa - r, hi = xa + r;
    uint32_t s = 0;                                       // the window sum at xa: 255 (2 r + 1) < 2^32
    for (int i = max(lo, 0); i <= min(hi, n - 1); ++i) s += src[base + i * step];
    if (lo < 0) s += (uint32_t)(-lo) * at(0);
    if (hi > n - 1) s += (uint32_t)(hi - (n - 1)) * at(n - 1);
    uint32_t le = at(xa - r - 1), re = at(xa + r + 1);
    for (int x = xa; x < xb; ++x) {
      dst[base + x * step] = (uint8_t)((s * ww + (le + re) * fw + (1u << 23)) >> 24);
      const uint32_t sub = at(x - r);
      s += re - sub;
      le = sub;
      re = at(x + r + 2);
    }
  }
}

template <bool ALONG_ROWS>
__device__ inline uint8_t* three_passes(uint8_t* a, uint8_t* b, int nl, int n, int pitch, const blur_rec& q) {
  __syncthreads();
  box_pass<ALONG_ROWS>(a, b, nl, n, pitch, q.r, q.ww, q.fw);
  __syncthreads();
  box_pass<ALONG_ROWS>(b, a, nl, n, pitch, q.r, q.ww, q.fw);
  __syncthreads();
  box_pass<ALONG_ROWS>(a, b, nl, n, pitch, q.r, q.ww, q.fw);
  __syncthreads();
  return b;
}

__global__ __launch_bounds__(THREADS) void blur_rows(const uint8_t* __restrict__ frames, int H, int W,
                                                     const blur_rec* __restrict__ recs, const blur_item* __restrict__ items,
                                                     uint8_t* __restrict__ scratch) {
  extern __shared__ uint8_t lds[];
  const blur_item it = items[blockIdx.x];
  const blur_rec q = recs[it.rec];
  const int pitch = 3 * q.w, bytes = it.count * pitch;
  uint8_t *a = lds, *b = lds + bytes;
  const uint8_t* src = frames + (((size_t)q.frame * H + q.y0 + it.start) * (size_t)W + q.x0) * 3;
  for (int i = threadIdx.x; i < bytes; i += THREADS) a[i] = src[(size_t)(i / pitch) * W * 3 + i % pitch];
  const uint8_t* out = three_passes<true>(a, b, 3 * it.count, q.w, pitch, q);
  uint8_t* dst = scratch + q.scratch + (size_t)it.start * pitch;   // the strip's rows are contiguous there
  for (int i = threadIdx.x; i < bytes; i += THREADS) dst[i] = out[i];
}

// libImaging/UnsharpMask.c on one sample: `in` stays where it is within `threshold` of its blur, otherwise it moves away
// from the blur by percent / 100 of the difference (integer division towards zero), clipped.  The product is taken in
// 64 bits: Pillow's int overflows for percents beyond 2^31 / 255.
__device__ inline uint8_t unsharp(int in, int blurred, int percent, int threshold) {
  const int diff = in - blurred;
  if (abs(diff) <= threshold) return (uint8_t)in;
  const long long v = in + (long long)diff * percent / 100;
  return (uint8_t)(v <= 0 ? 0 : v >= 255 ? 255 : v);
}

template <bool UNSHARP>
__global__ __launch_bounds__(THREADS) void blur_cols(uint8_t* __restrict__ frames, int H, int W,
                                                     const blur_rec* __restrict__ recs, const blur_item* __restrict__ items,
                                                     const int2* __restrict__ tabs, const uint8_t* __restrict__ scratch) {
  extern __shared__ uint8_t lds[];
  const blur_item it = items[blockIdx.x];
  const blur_rec q = recs[it.rec];
  const int pitch = 3 * it.count, bytes = q.h * pitch;
  uint8_t *a = lds, *b = lds + bytes;
  const uint8_t* src = scratch + q.scratch + (size_t)3 * it.start;
  for (int i = threadIdx.x; i < bytes; i += THREADS) a[i] = src[(size_t)(i / pitch) * (3 * q.w) + i % pitch];
  const uint8_t* out = three_passes<false>(a, b, pitch, q.h, pitch, q);
  uint8_t* dst = frames + (((size_t)q.frame * H + q.y0) * (size_t)W + q.x0 + it.start) * 3;
  for (int i = threadIdx.x; i < bytes; i += THREADS) {
    const int row = i / pitch, c = i % pitch, px = it.start + c / 3;
    // the span is clamped to the box on the host (ta_span_tables); px is in 0 .. w - 1 anyway, so that changes nothing here
    const int2 span = q.tab >= 0 ? tabs[q.tab + row] : make_int2(0, q.w - 1);
    if (px < span.x || px > span.y) continue;
    uint8_t* d = dst + (size_t)row * W * 3 + c;
    *d = UNSHARP ? unsharp(*d, out[i], q.percent, q.threshold) : out[i];   // the sample's own value: no other thread writes it
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// libImaging/BoxBlur.c: _gaussian_blur_radius(radius, passes = 3), then the weights of ImagingLineBoxBlur8's caller.  The
// variables are floats, the literals doubles, as there; the division for ww is a float32 division.
inline void box_params(float radius, float* box_radius, int32_t* r, uint32_t* ww, uint32_t* fw) {
  float sigma2, L, l, a;
  sigma2 = radius * radius / 3;
  L = sqrt(12.0 * sigma2 + 1.0);
  l = floor((L - 1.0) / 2.0);
  a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
  a /= 6 * (sigma2 - (l + 1) * (l + 1));
  const float fr = l + a;
  const int ri = (int)fr;
  const uint32_t w = (uint32_t)((uint32_t)(1 << 24) / (fr * 2 + 1));
  *box_radius = fr;
  *r = ri;
  *ww = w;
  *fw = ((uint32_t)(1 << 24) - (uint32_t)(ri * 2 + 1) * w) / 2;
}

inline bool radius_ok(float radius) { return radius >= 0.f && radius <= MAX_RADIUS; }   // false for a NaN

struct blur_job {            // one region of a round
  int32_t frame, x0, y0, x1, y1, shape;
  float radius;              // not 0
  int32_t percent, threshold;
};

// What one call launches: the records of the regions that change something, round by round, the strips of both stages
// of every round (one workgroup each), the ellipse span tables and the size of the pixel scratch (the largest round's).
struct blur_launch {
  int row0 = 0, rows = 0, col0 = 0, cols = 0;   // the round's strips in `items`
  size_t row_lds = 0, col_lds = 0;              // dynamic LDS of its two launches
};
struct blur_work {
  std::vector<blur_rec> recs;
  std::vector<blur_item> items;
  ta_span_tables spans;
  std::vector<blur_launch> launches;
  size_t pixels = 0;

  // records, strips and the pixel scratch of one round: `jobs` are pairwise disjoint within their frame
  void add_round(const std::vector<blur_job>& jobs) {
    const size_t first = recs.size();
    size_t at = 0;
    for (const blur_job& q : jobs) {
      blur_rec r;
      memset(&r, 0, sizeof(r));
      r.frame = q.frame;
      r.x0 = q.x0;
      r.y0 = q.y0;
      r.w = q.x1 - q.x0;
      r.h = q.y1 - q.y0;
      float fr;
      box_params(q.radius, &fr, &r.r, &r.ww, &r.fw);
      r.percent = q.percent;
      r.threshold = q.threshold;
      r.tab = q.shape == TA_BLUR_ELLIPSE ? spans.of(r.w, r.h) : -1;
      r.scratch = at;
      at += ((size_t)r.w * r.h * 3 + 15) & ~(size_t)15;
      recs.push_back(r);
    }
    pixels = std::max(pixels, at);
    blur_launch L;
    L.row0 = (int)items.size();
    for (size_t j = first; j < recs.size(); ++j) {
      const int pitch = 3 * recs[j].w;
      const int strip = std::max(1, std::min(ROW_STRIP, LDS_BUDGET / (2 * pitch)));
      for (int y = 0; y < recs[j].h; y += strip) items.push_back({(int32_t)j, y, std::min(strip, recs[j].h - y)});
      L.row_lds = std::max(L.row_lds, (size_t)2 * std::min(strip, recs[j].h) * pitch);
    }
    L.rows = (int)items.size() - L.row0;
    L.col0 = (int)items.size();
    for (size_t j = first; j < recs.size(); ++j) {
      const int h = recs[j].h;
      const int strip = std::max(1, std::min(COL_STRIP, LDS_BUDGET / (2 * 3 * h)));
      for (int x = 0; x < recs[j].w; x += strip) items.push_back({(int32_t)j, x, std::min(strip, recs[j].w - x)});
      L.col_lds = std::max(L.col_lds, (size_t)2 * 3 * std::min(strip, recs[j].w) * h);
    }
    L.cols = (int)items.size() - L.col0;
    launches.push_back(L);
  }

  // records, strips and span tables into the call's staging (frame_regions.h)
  size_t o_rec = 0, o_item = 0, o_tab = 0;
  void put(ta_staging& st) { o_rec = st.put(recs), o_item = st.put(items), o_tab = st.put(spans.table()); }

  // the two launches of round k, after the staging's commit; `pixels`: the pixel scratch on the device
  template <bool UNSHARP>
  void launch_round(hipStream_t stream, uint8_t* frames, int H, int W, size_t k, const ta_staging& st, uint8_t* pixels) const {
    const blur_launch& L = launches[k];
    if (!L.rows) return;
    const blur_rec* d_recs = st.dev<const blur_rec>(o_rec);
    const blur_item* d_items = st.dev<const blur_item>(o_item);
    hipLaunchKernelGGL(blur_rows, dim3(L.rows), dim3(THREADS), L.row_lds, stream, (const uint8_t*)frames, H, W, d_recs, d_items + L.row0, pixels);
    hipLaunchKernelGGL(blur_cols<UNSHARP>, dim3(L.cols), dim3(THREADS), L.col_lds, stream, frames, H, W, d_recs, d_items + L.col0,
                       st.dev<const int2>(o_tab), (const uint8_t*)pixels);
  }
};

}  // namespace gauss
}  // namespace
