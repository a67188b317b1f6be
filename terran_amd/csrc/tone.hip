// Pixel-value operations on regions of a resident frame batch, bit for bit with Pillow:
//   ta_frames_histogram  im.crop(box).histogram(mask), or the histogram of its convert('L')
//   ta_frames_point      im.paste(im.crop(box).point(lut), box)
//   ta_frames_saturate   im.paste(ImageEnhance.Color(im.crop(box)).enhance(factor), box)
// Pillow's luma is integer, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  Image.blend is the float32 expression
// in1 + alpha * (in2 - in1), a multiply and an add, truncated to uint8 for 0 <= alpha <= 1 and clipped to 0 .. 255 first
// otherwise (libImaging/Blend.c); a fused multiply-add changes some results, so this unit is compiled with
// -ffp-contract=off (build.py) and the two operations are spelled __fmul_rn / __fadd_rn besides.
//
// Device side, the same walk in all three kernels: a workgroup takes a strip of rows of one region (about 16384 pixels),
// each of its four waves takes every fourth row of the strip, and the lanes of a wave walk the row's pixels -- under the
// ellipse shape the row's span of TA_DRAW_DISC's table (ta_disc_rows, draw.hip) -- as a head of single pixels up to the
// first pixel that starts on a 4-byte boundary, groups of four pixels = three aligned dwords, and a tail of single
// pixels: 3 W is generally no multiple of 4 and 3 x0 is arbitrary, so the head differs from row to row.  A dword holds
// only bytes of the walked pixels, so the in-place kernels never touch a byte outside their region.
//
// Histogram: every wave counts into bins of its own in LDS (ds integer adds; four equal values of one lane are added as
// one 4), the workgroup sums its four copies and adds every non-zero bin to the region's bins in device memory with one
// global integer atomic.  Integer sums do not depend on their order: the result is deterministic.  A flat frame sends
// every lane of a wave to one LDS address, which the LDS serialises; the global atomics stay one per bin and workgroup.
// The in-place kernels run in rounds of regions that are pairwise disjoint within their frame (frame_regions.h), one
// launch per round.
#include "ta_internal.h"
#include "pixel_walk.h"
#include "frame_regions.h"

#include <math.h>
#include <string.h>

#include <utility>
#include <vector>

namespace {

constexpr int THREADS = WALK_THREADS, WAVE = WALK_WAVE, WAVES = WALK_WAVES;
constexpr int MAX_SIDE = 16384;            // of a region: 2^28 pixels at most, so a count fits uint32

struct tone_rec {            // 32 bytes
  int32_t frame, x0, y0, w, h;
  int32_t tab;               // ellipse: first row of the span table; box: -1
  int32_t arg;               // histogram: the region's index in `hist`; point: its table
  float factor;              // saturate
};
static_assert(sizeof(tone_rec) == 32, "tone_rec");

__device__ inline uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// the twelve bytes of a group: d[0] = R0 G0 B0 R1, d[1] = G1 B1 R2 G2, d[2] = B2 R3 G3 B3 (lowest byte first)
struct quad {
  uint32_t r[4], g[4], b[4];
};
__device__ inline quad unpack(const uint32_t d0, const uint32_t d1, const uint32_t d2) {
  quad v;
  v.r[0] = d0 & 255, v.g[0] = d0 >> 8 & 255, v.b[0] = d0 >> 16 & 255, v.r[1] = d0 >> 24;
  v.g[1] = d1 & 255, v.b[1] = d1 >> 8 & 255, v.r[2] = d1 >> 16 & 255, v.g[2] = d1 >> 24;
  v.b[2] = d2 & 255, v.r[3] = d2 >> 8 & 255, v.g[3] = d2 >> 16 & 255, v.b[3] = d2 >> 24;
  return v;
}
__device__ inline void pack(const quad& v, uint32_t* d) {
  d[0] = v.r[0] | v.g[0] << 8 | v.b[0] << 16 | v.r[1] << 24;
  d[1] = v.g[1] | v.b[1] << 8 | v.r[2] << 16 | v.g[2] << 24;
  d[2] = v.b[2] | v.r[3] << 8 | v.g[3] << 16 | v.b[3] << 24;
}

__device__ inline void count4(uint32_t* bins, const uint32_t v[4]) {
  if (v[0] == v[1] && v[2] == v[3] && v[0] == v[2]) {
    atomicAdd(bins + v[0], 4u);
  } else {
    for (int k = 0; k < 4; ++k) atomicAdd(bins + v[k], 1u);
  }
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void hist_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                       const tone_rec* __restrict__ recs, const strip_item* __restrict__ items,
                                                       const int2* __restrict__ tabs, uint32_t* __restrict__ bins) {
  constexpr int NB = MODE == TA_HIST_RGB ? 768 : 256;
  __shared__ uint32_t lds[WAVES * NB];
  for (int i = threadIdx.x; i < WAVES * NB; i += THREADS) lds[i] = 0;
  __syncthreads();
  const strip_item it = items[blockIdx.x];
  const tone_rec q = recs[it.rec];
  uint32_t* mine = lds + (threadIdx.x / WAVE) * NB;
  const int lane = threadIdx.x % WAVE;
  walk_strip(frames, H, W, q, it, tabs, [&](const uint8_t* p, int npx, int, int) {
    walk_row(
        p, npx, lane,
        [&](const uint8_t* px) {
          if (MODE == TA_HIST_RGB) {
            atomicAdd(mine + px[0], 1u);
            atomicAdd(mine + 256 + px[1], 1u);
            atomicAdd(mine + 512 + px[2], 1u);
          } else {
            atomicAdd(mine + luma(px[0], px[1], px[2]), 1u);
          }
        },
        [&](const uint8_t* px) {
          const uint32_t* d = (const uint32_t*)px;
          const quad v = unpack(d[0], d[1], d[2]);
          if (MODE == TA_HIST_RGB) {
            count4(mine, v.r);
            count4(mine + 256, v.g);
            count4(mine + 512, v.b);
          } else {
            uint32_t l[4];
            for (int k = 0; k < 4; ++k) l[k] = luma(v.r[k], v.g[k], v.b[k]);
            count4(mine, l);
          }
        });
  });
  __syncthreads();
  uint32_t* out = bins + (size_t)q.arg * NB;
  for (int b = threadIdx.x; b < NB; b += THREADS) {
    uint32_t c = 0;
    for (int k = 0; k < WAVES; ++k) c += lds[k * NB + b];
    if (c) atomicAdd(out + b, c);
  }
}

__global__ __launch_bounds__(THREADS) void point_kernel(uint8_t* __restrict__ frames, int H, int W, const tone_rec* __restrict__ recs,
                                                        const strip_item* __restrict__ items, const int2* __restrict__ tabs,
                                                        const uint8_t* __restrict__ luts) {
  __shared__ uint32_t words[192];
  const strip_item it = items[blockIdx.x];
  const tone_rec q = recs[it.rec];
  const uint32_t* src = (const uint32_t*)(luts + (size_t)q.arg * 768);     // tables start on a 16-byte boundary, 768 apart
  if (threadIdx.x < 192) words[threadIdx.x] = src[threadIdx.x];
  __syncthreads();
  const uint8_t *tr = (const uint8_t*)words, *tg = tr + 256, *tb = tr + 512;
  walk_strip(frames, H, W, q, it, tabs, [&](uint8_t* p, int npx, int, int) {
    walk_row(
        p, npx, threadIdx.x % WAVE,
        [&](uint8_t* px) {
          px[0] = tr[px[0]];
          px[1] = tg[px[1]];
          px[2] = tb[px[2]];
        },
        [&](uint8_t* px) {
          uint32_t* d = (uint32_t*)px;
          quad v = unpack(d[0], d[1], d[2]);
          for (int k = 0; k < 4; ++k) v.r[k] = tr[v.r[k]], v.g[k] = tg[v.g[k]], v.b[k] = tb[v.b[k]];
          pack(v, d);
        });
  });
}

__global__ __launch_bounds__(THREADS) void saturate_kernel(uint8_t* __restrict__ frames, int H, int W, const tone_rec* __restrict__ recs,
                                                           const strip_item* __restrict__ items, const int2* __restrict__ tabs) {
  const strip_item it = items[blockIdx.x];
  const tone_rec q = recs[it.rec];
  const float f = q.factor;
  const bool inside = f >= 0.f && f <= 1.f;
  walk_strip(frames, H, W, q, it, tabs, [&](uint8_t* p, int npx, int, int) {
    walk_row(
        p, npx, threadIdx.x % WAVE,
        [&](uint8_t* px) {
          const uint32_t r = px[0], g = px[1], b = px[2], l = luma(r, g, b);
          px[0] = (uint8_t)blend(l, r, f, inside);
          px[1] = (uint8_t)blend(l, g, f, inside);
          px[2] = (uint8_t)blend(l, b, f, inside);
        },
        [&](uint8_t* px) {
          uint32_t* d = (uint32_t*)px;
          quad v = unpack(d[0], d[1], d[2]);
          for (int k = 0; k < 4; ++k) {
            const uint32_t l = luma(v.r[k], v.g[k], v.b[k]);
            v.r[k] = blend(l, v.r[k], f, inside);
            v.g[k] = blend(l, v.g[k], f, inside);
            v.b[k] = blend(l, v.b[k], f, inside);
          }
          pack(v, d);
        });
  });
}

// ---- host ------------------------------------------------------------------------------------------------------------
// What one call launches: a record per region that does something, round by round, the strips of every round (one
// workgroup each) and the ellipse span tables; checks, rounds, span tables and staging are frame_regions.h's.
struct tone_work {
  std::vector<tone_rec> recs;
  std::vector<strip_item> items;
  ta_span_tables spans;
  std::vector<std::pair<int, int>> launches;   // first strip and strips of every round
  size_t closed = 0;                           // records of the rounds closed so far

  template <class R>
  tone_rec& add(const R& q) {
    tone_rec r;
    memset(&r, 0, sizeof(r));
    r.frame = q.frame, r.x0 = q.x0, r.y0 = q.y0, r.w = q.x1 - q.x0, r.h = q.y1 - q.y0;
    r.tab = q.shape == TA_BLUR_ELLIPSE ? spans.of(r.w, r.h) : -1;
    recs.push_back(r);
    return recs.back();
  }
  // closes a round: the strips of the records added since the last one
  void close() {
    const int at = (int)items.size();
    launches.push_back({at, ta_add_strips(items, recs, closed, WALK_WAVES, STRIP_PIXELS)});
    closed = recs.size();
  }
  // records, strips and span tables into the call's staging; after its commit, where they are on the device
  size_t o_rec = 0, o_item = 0, o_tab = 0;
  void put(ta_staging& st) { o_rec = st.put(recs), o_item = st.put(items), o_tab = st.put(spans.table()); }
  const tone_rec* d_recs(const ta_staging& st) const { return st.dev<const tone_rec>(o_rec); }
  const strip_item* d_items(const ta_staging& st) const { return st.dev<const strip_item>(o_item); }
  const int2* d_tab(const ta_staging& st) const { return st.dev<const int2>(o_tab); }
};

// the records of an in-place call, round by round; skip(region): the region changes nothing
template <class R, class S, class F>
void plan_rounds(const R* regions, int n, tone_work& w, S skip, F fill) {
  ta_each_round(
      regions, n,
      [&](const R& q) {
        if (!skip(q)) fill(w.add(q), q);
      },
      [&] { w.close(); });
}

}  // namespace

extern "C" int ta_frames_histogram(ta_ctx* ctx, const ta_frames* frames, const ta_hist_region* regions, int n, int mode, uint32_t* hist) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_TRY(ta_check_regions(ctx, "frames_histogram", frames, regions, n, MAX_SIDE, [](const ta_hist_region&) { return (const char*)nullptr; }));
  if (mode != TA_HIST_RGB && mode != TA_HIST_L) return ta_fail(ctx, TA_E_INVALID, "frames_histogram: unknown mode %d", mode);
  if (n == 0) return TA_OK;
  if (!hist) return ta_fail(ctx, TA_E_INVALID, "frames_histogram: hist is NULL");

  tone_work w;
  for (int i = 0; i < n; ++i) w.add(regions[i]).arg = i;
  w.close();
  const size_t b_bins = (size_t)n * (mode == TA_HIST_RGB ? 768 : 256) * sizeof(uint32_t);
  ta_staging st;                                    // one H2D copy; the bins behind it on the device, and pinned for the read-back
  w.put(st);
  const size_t o_bins = st.device_only(b_bins), o_host = st.host_only(b_bins);
  TA_TRY(st.commit(ctx));
  uint32_t* bins = st.dev<uint32_t>(o_bins);
  TA_HIP(ctx, hipMemsetAsync(bins, 0, b_bins, ctx->stream));
  const int strips = w.launches[0].second;
  if (mode == TA_HIST_RGB)
    hipLaunchKernelGGL(hist_kernel<TA_HIST_RGB>, dim3(strips), dim3(THREADS), 0, ctx->stream, (const uint8_t*)frames->dev, frames->h,
                       frames->w, w.d_recs(st), w.d_items(st), w.d_tab(st), bins);
  else
    hipLaunchKernelGGL(hist_kernel<TA_HIST_L>, dim3(strips), dim3(THREADS), 0, ctx->stream, (const uint8_t*)frames->dev, frames->h,
                       frames->w, w.d_recs(st), w.d_items(st), w.d_tab(st), bins);
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipMemcpyAsync(st.host<uint32_t>(o_host), bins, b_bins, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  memcpy(hist, st.host<uint32_t>(o_host), b_bins);
  return TA_OK;
}

extern "C" int ta_frames_point(ta_ctx* ctx, ta_frames* frames, const ta_point_region* regions, int n, const uint8_t* luts, int n_luts) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_luts < 0 || (n > 0 && !luts)) return ta_fail(ctx, TA_E_INVALID, "frames_point: bad args");
  TA_TRY(ta_check_regions(ctx, "frames_point", frames, regions, n, MAX_SIDE,
                          [&](const ta_point_region& q) { return q.lut < 0 || q.lut >= n_luts ? "lut index out of range" : (const char*)nullptr; }));
  if (n == 0) return TA_OK;

  tone_work w;
  plan_rounds(regions, n, w, [](const ta_point_region&) { return false; }, [](tone_rec& r, const ta_point_region& q) { r.arg = q.lut; });
  ta_staging st;                                    // one H2D copy
  w.put(st);
  const size_t o_luts = st.put(luts, (size_t)n_luts * 768, 16);   // point_kernel reads the tables as dwords: a 16-byte boundary
  TA_TRY(st.commit(ctx));
  for (const auto& L : w.launches)
    if (L.second)
      hipLaunchKernelGGL(point_kernel, dim3(L.second), dim3(THREADS), 0, ctx->stream, frames->dev, frames->h, frames->w, w.d_recs(st),
                         w.d_items(st) + L.first, w.d_tab(st), st.dev<const uint8_t>(o_luts));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}

extern "C" int ta_frames_saturate(ta_ctx* ctx, ta_frames* frames, const ta_saturate_region* regions, int n) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  TA_TRY(ta_check_regions(ctx, "frames_saturate", frames, regions, n, MAX_SIDE,
                          [](const ta_saturate_region& q) { return isfinite(q.factor) ? (const char*)nullptr : "factor not finite"; }));
  if (n == 0) return TA_OK;

  tone_work w;
  plan_rounds(regions, n, w, [](const ta_saturate_region& q) { return q.factor == 1.f; },    // Image.blend copies the image
              [](tone_rec& r, const ta_saturate_region& q) { r.factor = q.factor; });
  if (w.recs.empty()) return TA_OK;
  ta_staging st;                                    // one H2D copy
  w.put(st);
  TA_TRY(st.commit(ctx));
  for (const auto& L : w.launches)
    if (L.second)
      hipLaunchKernelGGL(saturate_kernel, dim3(L.second), dim3(THREADS), 0, ctx->stream, frames->dev, frames->h, frames->w, w.d_recs(st),
                         w.d_items(st) + L.first, w.d_tab(st));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
