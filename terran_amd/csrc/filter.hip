// ta_frames_filter: Pillow's `im.paste(im.crop(box).filter(F), box[, ellipse mask])` on regions of a resident frame batch,
// in place, bit for bit, for F a convolution kernel (ImageFilter.Kernel and the ten built-in filters, optionally blended
// with the original as ImageEnhance.Sharpness does), a rank filter (RankFilter, MinFilter, MedianFilter, MaxFilter) or
// UnsharpMask.  The arithmetic is libImaging's (Filter.c, RankFilter.c, UnsharpMask.c) and is spelled out in
// include/terran_amd.h; the float32 steps are never fused: this unit is compiled with -ffp-contract=off (build.py) and
// the multiplies and adds are spelled __fmul_rn / __fadd_rn besides.  The host divides the kernel by its scale and adds
// 0.5 to the offset (normalise): the device sees those float32 values only.
//
// A filter reads neighbours that the same call overwrites, so every round of regions that are pairwise disjoint within
// their frame (frame_regions.h) runs in two launches:
//   filter_tiles: a workgroup takes a TILE_W x TILE_H = 128 x 32 pixel tile of one region, loads it with a halo of
//                 size / 2 pixels, clipped to the region, into LDS as bytes -- whole aligned dwords of the frame, so a row
//                 sits in LDS at the byte phase (0 .. 3) it has in memory -- and every thread computes groups of four
//                 pixels = three dwords of the region's packed result image in scratch (rows of 12 bytes per group, so the
//                 stores are aligned whatever the region's place in the frame);
//   filter_paste: a workgroup takes a strip of rows of one region and copies the packed result into the frame under the
//                 shape's mask, each row walked as tone.hip walks it (a head of single pixels, groups of four pixels =
//                 three aligned dwords, a tail); the source of a group is four aligned dwords, shifted by its byte phase.
// A kernel's window never leaves the region (the outer size / 2 pixels keep their values); a rank filter's coordinates are
// clamped to the region.  Rank: the window's size^2 bytes go from LDS into registers (every loop is unrolled: no
// per-thread array in memory) and an 8-step bitwise search on the value counts the bytes below the candidate: exact for
// any size and rank, no sort.  Every output depends only on the frame as the round found it.
// UnsharpMask runs blur_passes.h's two launches, the last with its unsharp write.
#include "blur_passes.h"
#include "pixel_walk.h"
#include "frame_regions.h"

namespace {

constexpr int THREADS = WALK_THREADS;
constexpr int MAX_SIDE = gauss::MAX_SIDE;
constexpr int TILE_W = 128, TILE_H = 32, MAX_R = 3;       // pixels of a tile; the widest halo (rank size 7)
constexpr int GROUPS = TILE_W / 4;                        // groups of four pixels in a tile row
constexpr int TILE_ROWS = TILE_H + 2 * MAX_R;
constexpr int PITCH = (3 + 3 * (TILE_W + 2 * MAX_R) + 3) & ~3;   // bytes of a tile row in LDS: phase, pixels, rounded up
constexpr int PITCH_DW = PITCH / 4;
enum { BLEND_NONE = 0, BLEND_TRUNCATE = 1, BLEND_CLIP = 2 };

struct filter_rec {          // 40 bytes
  int32_t frame, x0, y0, w, h;
  int32_t tab;               // ellipse: first row of the span table; box: -1
  int32_t spec;
  int32_t pitch;             // bytes of a row of the packed result: 12 per group of four pixels
  uint64_t scratch;          // byte offset of the packed result in the pixel scratch, a multiple of 16
};
static_assert(sizeof(filter_rec) == 40, "filter_rec");

struct filter_dspec {        // 128 bytes: a spec as the device sees it
  int32_t kind, size, rank, blend;
  float k[25];               // kernel[i] / scale
  float offset;              // offset + 0.5f
  float factor;
  int32_t pad;
};
static_assert(sizeof(filter_dspec) == 128, "filter_dspec");

struct filter_item {         // filter_tiles: the tile's first pixel (x, y) in the region
  int32_t rec, x, y;
};

// the tile in LDS: rows ry0 .. of the region from pixel cx0 on, row r at byte phase (ph0 + r * phs) & 3
struct tile_view {
  const uint8_t* bytes;
  int cx0, ry0, ph0, phs;
  __device__ const uint8_t* at(int y, int x) const {
    const int r = y - ry0;
    return bytes + r * PITCH + ((ph0 + r * phs) & 3) + 3 * (x - cx0);
  }
};

// libImaging/Filter.c, one channel of one pixel
template <int S>
__device__ inline uint32_t conv(const tile_view& t, const filter_dspec& sp, int w, int h, int x, int y, int c) {
  constexpr int R = S / 2;
  const uint32_t o = t.at(y, x)[c];
  if (x < R || y < R || x >= w - R || y >= h - R) return o;
  float ss = sp.offset;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const uint8_t* p = t.at(y + R - j, x - R) + c;
    float row = __fmul_rn((float)p[0], sp.k[j * S]);
#pragma unroll
    for (int i = 1; i < S; ++i) row = __fadd_rn(row, __fmul_rn((float)p[3 * i], sp.k[j * S + i]));
    ss = __fadd_rn(ss, row);
  }
  const uint32_t f = ss <= 0.f ? 0u : ss >= 255.f ? 255u : (uint32_t)(int)ss;
  return sp.blend == BLEND_NONE ? f : blend(f, o, sp.factor, sp.blend == BLEND_TRUNCATE);
}

// libImaging/RankFilter.c on ImagingExpand's edge replication, one channel of one pixel: the largest v with fewer than
// rank + 1 window values below it
template <int S>
__device__ inline uint32_t rank_of(const tile_view& t, const filter_dspec& sp, int w, int h, int x, int y, int c) {
  constexpr int R = S / 2;
  uint32_t win[S * S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const uint8_t* row = t.at(min(max(y + j - R, 0), h - 1), t.cx0) + c;
#pragma unroll
    for (int i = 0; i < S; ++i) win[j * S + i] = row[3 * (min(max(x + i - R, 0), w - 1) - t.cx0)];
  }
  uint32_t v = 0;
#pragma unroll
  for (uint32_t bit = 128; bit; bit >>= 1) {
    const uint32_t cand = v | bit;
    int below = 0;
#pragma unroll
    for (int i = 0; i < S * S; ++i) below += win[i] < cand;
    if (below <= sp.rank) v = cand;
  }
  return v;
}

// every group of four pixels of the tile: sample(x, y, c) of its twelve bytes, three aligned dwords of the packed result
template <class F>
__device__ inline void run_tile(const filter_item& it, const filter_rec& q, uint8_t* __restrict__ scratch, F sample) {
  for (int u = threadIdx.x; u < TILE_H * GROUPS; u += THREADS) {
    const int y = it.y + u / GROUPS, x = it.x + 4 * (u % GROUPS);
    if (y >= q.h || x >= q.w) continue;
    uint32_t* dst = (uint32_t*)(scratch + q.scratch + (size_t)y * q.pitch + 3 * x);
#pragma unroll 1
    for (int d = 0; d < 3; ++d) {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = 4 * d + b, px = x + k / 3;
        if (px < q.w) v |= sample(px, y, k % 3) << (8 * b);
      }
      dst[d] = v;
    }
  }
}

__global__ __launch_bounds__(THREADS) void filter_tiles(const uint8_t* __restrict__ frames, size_t total, int H, int W,
                                                        const filter_rec* __restrict__ recs, const filter_dspec* __restrict__ specs,
                                                        const filter_item* __restrict__ items, uint8_t* __restrict__ scratch) {
  __shared__ uint32_t lds[TILE_ROWS * PITCH_DW];
  const filter_item it = items[blockIdx.x];
  const filter_rec q = recs[it.rec];
  const filter_dspec sp = specs[q.spec];
  const int R = sp.size >> 1;
  const int cx0 = max(it.x - R, 0), cx1 = min(it.x + TILE_W + R, q.w), ry0 = max(it.y - R, 0), ry1 = min(it.y + TILE_H + R, q.h);
  const size_t row_bytes = (size_t)W * 3;
  const size_t off0 = (((size_t)q.frame * H + q.y0 + ry0) * (size_t)W + q.x0 + cx0) * 3;
  const int nbytes = 3 * (cx1 - cx0);
  for (int i = threadIdx.x; i < (ry1 - ry0) * PITCH_DW; i += THREADS) {
    const int r = i / PITCH_DW, j = i % PITCH_DW;
    const size_t off = off0 + (size_t)r * row_bytes;
    if (j >= (int)(((off & 3) + nbytes + 3) >> 2)) continue;
    const size_t at = (off & ~(size_t)3) + 4 * (size_t)j;       // an aligned dword that holds a byte of the row
    uint32_t v = 0;
    if (at + 4 <= total) {
      v = *(const uint32_t*)(frames + at);
    } else {                                                    // the batch's last bytes: never read past them
      for (size_t b = at; b < total; ++b) v |= (uint32_t)frames[b] << (8 * (b - at));
    }
    lds[i] = v;
  }
  __syncthreads();
  const tile_view t = {(const uint8_t*)lds, cx0, ry0, (int)(off0 & 3), (int)(row_bytes & 3)};
  const int w = q.w, h = q.h;
  if (sp.kind == TA_FILTER_KERNEL) {
    if (sp.size == 3)
      run_tile(it, q, scratch, [&](int x, int y, int c) { return conv<3>(t, sp, w, h, x, y, c); });
    else
      run_tile(it, q, scratch, [&](int x, int y, int c) { return conv<5>(t, sp, w, h, x, y, c); });
  } else if (sp.size == 3) {
    run_tile(it, q, scratch, [&](int x, int y, int c) { return rank_of<3>(t, sp, w, h, x, y, c); });
  } else if (sp.size == 5) {
    run_tile(it, q, scratch, [&](int x, int y, int c) { return rank_of<5>(t, sp, w, h, x, y, c); });
  } else {
    run_tile(it, q, scratch, [&](int x, int y, int c) { return rank_of<7>(t, sp, w, h, x, y, c); });
  }
}

__global__ __launch_bounds__(THREADS) void filter_paste(uint8_t* __restrict__ frames, int H, int W, const filter_rec* __restrict__ recs,
                                                        const strip_item* __restrict__ items, const int2* __restrict__ tabs,
                                                        const uint8_t* __restrict__ scratch) {
  const strip_item it = items[blockIdx.x];
  const filter_rec q = recs[it.rec];
  walk_strip(frames, H, W, q, it, tabs, [&](uint8_t* p, int npx, int r, int x) {
    const uint8_t* s = scratch + q.scratch + (size_t)r * q.pitch + 3 * x;
    walk_row(
        p, npx, threadIdx.x % WALK_WAVE,
        [&](uint8_t* px) {
          const uint8_t* from = s + (px - p);
          px[0] = from[0], px[1] = from[1], px[2] = from[2];
        },
        [&](uint8_t* px) {
          const uint8_t* from = s + (px - p);
          const uint32_t m = (uint32_t)((uintptr_t)from & 3);
          const uint32_t* a = (const uint32_t*)(from - m);          // the row is dword aligned in scratch
          const uint32_t d0 = a[0], d1 = a[1], d2 = a[2], d3 = m ? a[3] : 0u;   // a[3] holds a byte of the group only when m != 0
          uint32_t* d = (uint32_t*)px;
          d[0] = __builtin_amdgcn_alignbyte(d1, d0, m);
          d[1] = __builtin_amdgcn_alignbyte(d2, d1, m);
          d[2] = __builtin_amdgcn_alignbyte(d3, d2, m);
        });
  });
}

// ---- host ------------------------------------------------------------------------------------------------------------
const char* check_spec(const ta_filter_spec& s) {
  switch (s.kind) {
    case TA_FILTER_KERNEL:
      if (s.size != 3 && s.size != 5) return "a kernel size other than 3 or 5";
      for (int i = 0; i < s.size * s.size; ++i)
        if (!isfinite(s.kernel[i])) return "a kernel entry that is not finite";
      if (!isfinite(s.scale) || s.scale == 0.f) return "a scale that is 0 or not finite";
      if (!isfinite(s.offset)) return "an offset that is not finite";
      if (s.has_factor && !isfinite(s.factor)) return "a factor that is not finite";
      return nullptr;
    case TA_FILTER_RANK:
      if (s.size < 1 || s.size > 7 || s.size % 2 == 0) return "a rank size that is even or outside 1 .. 7";
      if (s.rank < 0 || s.rank >= s.size * s.size) return "a rank outside 0 .. size^2 - 1";
      return nullptr;
    case TA_FILTER_UNSHARP:
      if (!gauss::radius_ok(s.radius)) return "radius negative, not finite or above 1024";
      if (s.percent < 0 || s.threshold < 0) return "a negative percent or threshold";
      return nullptr;
  }
  return "unknown kind";
}

// a spec as the device sees it: libImaging divides the float32 kernel by the float32 divisor and adds 0.5 to the offset
void normalise(const ta_filter_spec& s, filter_dspec& d) {
  memset(&d, 0, sizeof(d));
  d.kind = s.kind, d.size = s.size, d.rank = s.rank;
  if (s.kind != TA_FILTER_KERNEL) return;
  for (int i = 0; i < s.size * s.size; ++i) d.k[i] = s.kernel[i] / s.scale;
  d.offset = s.offset + 0.5f;
  if (s.has_factor) d.factor = s.factor, d.blend = s.factor >= 0.f && s.factor <= 1.f ? BLEND_TRUNCATE : BLEND_CLIP;
}

// does the region change nothing?  A kernel larger than the region (Pillow copies the image), a blend that returns the
// original, a window of one pixel, a blur of radius 0 (the difference to it is 0, within every threshold).
bool idle(const ta_filter_region& q, const ta_filter_spec& s) {
  if (s.kind == TA_FILTER_KERNEL) return q.x1 - q.x0 < s.size || q.y1 - q.y0 < s.size || (s.has_factor && s.factor == 1.f);
  if (s.kind == TA_FILTER_RANK) return s.size == 1;
  return s.radius == 0.f;
}

struct filter_round {
  int tile0 = 0, tiles = 0, strip0 = 0, strips = 0;   // the round's workgroups in `tiles` and `strips`
};
struct filter_work {
  std::vector<filter_rec> recs;
  std::vector<filter_item> tiles;
  std::vector<strip_item> strips;
  ta_span_tables spans;
  std::vector<filter_round> rounds;
  size_t pixels = 0;                                  // the largest round's packed results
  size_t closed = 0, at = 0;                          // records of the rounds closed so far; bytes of the open round

  void add(const ta_filter_region& q) {
    filter_rec r;
    memset(&r, 0, sizeof(r));
    r.frame = q.frame, r.x0 = q.x0, r.y0 = q.y0, r.w = q.x1 - q.x0, r.h = q.y1 - q.y0;
    r.spec = q.spec;
    r.tab = q.shape == TA_BLUR_ELLIPSE ? spans.of(r.w, r.h) : -1;
    r.pitch = 12 * ((r.w + 3) / 4);
    r.scratch = at;
    at += ((size_t)r.pitch * r.h + 15) & ~(size_t)15;
    recs.push_back(r);
  }
  // closes a round: the tiles and the strips of the records added since the last one
  void close() {
    filter_round L;
    L.tile0 = (int)tiles.size();
    for (size_t j = closed; j < recs.size(); ++j)
      for (int y = 0; y < recs[j].h; y += TILE_H)
        for (int x = 0; x < recs[j].w; x += TILE_W) tiles.push_back({(int32_t)j, x, y});
    L.tiles = (int)tiles.size() - L.tile0;
    L.strip0 = (int)strips.size();
    L.strips = ta_add_strips(strips, recs, closed, WALK_WAVES, STRIP_PIXELS);
    rounds.push_back(L);
    pixels = std::max(pixels, at);
    closed = recs.size(), at = 0;
  }
};

// a region's own defect: its spec
auto spec_in(int n_specs) {
  return [n_specs](const ta_filter_region& q) { return q.spec < 0 || q.spec >= n_specs ? "spec index out of range" : (const char*)nullptr; };
}

}  // namespace

extern "C" int ta_filter_plan(const ta_filter_region* regions, int n, const ta_filter_spec* specs, int n_specs, int32_t* rounds,
                              float* kernels, float* offsets) {
  if (n < 0 || n_specs < 0 || (n > 0 && !regions) || (n_specs > 0 && !specs)) return TA_E_INVALID;
  for (int s = 0; s < n_specs; ++s)
    if (check_spec(specs[s])) return TA_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (ta_region_defect(regions[i], spec_in(n_specs))) return TA_E_INVALID;
  std::vector<int32_t> round;
  ta_plan_rounds(regions, n, round);
  for (int i = 0; i < n && rounds; ++i) rounds[i] = round[i];
  for (int s = 0; s < n_specs; ++s) {
    filter_dspec d;
    normalise(specs[s], d);
    if (kernels) memcpy(kernels + 25 * (size_t)s, d.k, sizeof(d.k));
    if (offsets) offsets[s] = d.offset;
  }
  return TA_OK;
}

extern "C" int ta_frames_filter(ta_ctx* ctx, ta_frames* frames, const ta_filter_region* regions, int n, const ta_filter_spec* specs,
                                int n_specs) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_specs < 0 || (n_specs > 0 && !specs)) return ta_fail(ctx, TA_E_INVALID, "frames_filter: bad args");
  TA_TRY(ta_check_batch(ctx, "frames_filter", frames, regions, n));
  for (int s = 0; s < n_specs; ++s)
    if (const char* why = check_spec(specs[s])) return ta_fail(ctx, TA_E_INVALID, "frames_filter: spec %d: %s", s, why);
  TA_TRY(ta_check_boxes(ctx, "frames_filter", frames, regions, n, MAX_SIDE, spec_in(n_specs)));
  if (n == 0) return TA_OK;

  // round by round: the kernel and rank regions of a round go through filter_tiles / filter_paste, its unsharp regions
  // through the blur passes; they are disjoint, so the order of the two within a round does not matter
  filter_work fw;
  gauss::blur_work bw;
  std::vector<gauss::blur_job> jobs;
  ta_each_round(
      regions, n,
      [&](const ta_filter_region& q) {
        const ta_filter_spec& s = specs[q.spec];
        if (idle(q, s)) return;
        if (s.kind == TA_FILTER_UNSHARP)
          jobs.push_back({q.frame, q.x0, q.y0, q.x1, q.y1, q.shape, s.radius, s.percent, s.threshold});
        else
          fw.add(q);
      },
      [&] {
        fw.close();
        bw.add_round(jobs);
        jobs.clear();
      });
  if (fw.recs.empty() && bw.recs.empty()) return TA_OK;
  std::vector<filter_dspec> dspecs(n_specs);
  for (int s = 0; s < n_specs; ++s) normalise(specs[s], dspecs[s]);

  // one H2D copy: the filter's records, specs, workgroups and spans, then the blur's; behind them the two pixel areas
  ta_staging st;
  const size_t o_frec = st.put(fw.recs), o_spec = st.put(dspecs), o_tile = st.put(fw.tiles), o_strip = st.put(fw.strips);
  const size_t o_ftab = st.put(fw.spans.table());
  bw.put(st);
  const size_t o_fpix = st.device_only(fw.pixels), o_bpix = st.device_only(bw.pixels);
  TA_TRY(st.commit(ctx));
  const filter_rec* d_frec = st.dev<const filter_rec>(o_frec);
  const int H = frames->h, W = frames->w;
  const size_t total = (size_t)frames->n * H * W * 3;
  TA_SET_LDS_ATTR(ctx, gauss::blur_rows, gauss::LDS_BUDGET);
  TA_SET_LDS_ATTR(ctx, gauss::blur_cols<true>, gauss::LDS_BUDGET);
  for (size_t k = 0; k < fw.rounds.size(); ++k) {
    const filter_round& L = fw.rounds[k];
    if (L.tiles) {
      hipLaunchKernelGGL(filter_tiles, dim3(L.tiles), dim3(THREADS), 0, ctx->stream, (const uint8_t*)frames->dev, total, H, W, d_frec,
                         st.dev<const filter_dspec>(o_spec), st.dev<const filter_item>(o_tile) + L.tile0, st.dev<uint8_t>(o_fpix));
      hipLaunchKernelGGL(filter_paste, dim3(L.strips), dim3(THREADS), 0, ctx->stream, frames->dev, H, W, d_frec,
                         st.dev<const strip_item>(o_strip) + L.strip0, st.dev<const int2>(o_ftab), st.dev<const uint8_t>(o_fpix));
    }
    bw.launch_round<true>(ctx->stream, frames->dev, H, W, k, st, st.dev<uint8_t>(o_bpix));
  }
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
