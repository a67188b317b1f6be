// Operations of two images on regions of a resident frame batch, in place and bit for bit with Pillow:
//   ta_frames_combine   dst.paste(R, box), R = a with b pasted under a mask | Image.blend(a, b, alpha) | ImageChops.<op>(a, b)
// for a = dst.crop(box) and b = the equally sized box of a frame of a second batch (include/terran_amd.h has the formulas
// of libImaging/Paste.c, Blend.c and Chops.c).  ImageChops.add / subtract divide in float32: the division is __fdiv_rn, a
// correctly rounded one, never a multiplication by the reciprocal, and Image.blend's multiply and add are not fused, so
// this unit is compiled with -ffp-contract=off (build.py).
//
// Device side, one kernel: a workgroup takes a strip of rows of one region and walks the DESTINATION row as tone.hip does
// (pixel_walk.h): a head of single pixels up to the first one on a 4-byte boundary, groups of four pixels = three aligned
// dwords, a tail of single pixels.  The source row, and the mask row of a bitmap or a mask batch, sit at any byte offset
// relative to the destination: 3 W, the boxes' x and the batches' sizes are arbitrary.  A group therefore loads the
// aligned dwords that COVER the source's twelve bytes (three when the source is aligned too, four otherwise) and the
// bitmap's four (one or two) and shifts them into place in registers (v_alignbyte_b32); the offset within a dword is the
// same for every group of a row, so the choice is uniform in a wave.  A covering dword holds a byte of the batch, and a
// batch is allocated in multiples of 16 bytes at an aligned address (frames_alloc, runtime.hip), the staged bitmaps
// likewise: no load leaves an allocation.  Consecutive lanes read consecutive 12-byte groups, so a wave's loads and
// stores cover contiguous bytes.  The op and the mask kind are uniform in a region: the workgroup branches on them once.
// Regions run in rounds of pairwise disjoint ones within their frame (frame_regions.h), one launch per round.
#include "ta_internal.h"
#include "pixel_walk.h"
#include "frame_regions.h"

#include <math.h>
#include <string.h>

#include <set>
#include <utility>
#include <vector>

namespace {

constexpr int THREADS = WALK_THREADS;
constexpr int MAX_SIDE = 16384;            // of a region, as in tone.hip

struct combine_rec {         // 72 bytes
  int32_t frame, x0, y0, w, h;
  int32_t tab;               // ellipse: first row of the span table; box: -1
  int32_t op, mask_kind;
  uint64_t src_off;          // byte offset in `src` of the source box's first pixel
  uint64_t mask_off;         // BITMAP: byte offset of the bitmap in the staged masks; FRAMES: of the mask box's first pixel in `mask_frames`
  int32_t src_pitch, mask_pitch;   // bytes from a row to the next
  int32_t mask_value;        // CONSTANT
  int32_t mask_band;         // FRAMES
  float alpha;               // BLEND: alpha; ADD, SUBTRACT: scale
  int32_t offset;            // ADD, SUBTRACT
};
static_assert(sizeof(combine_rec) == 72, "combine_rec");

struct quad {                // the twelve bytes of a group, as in tone.hip
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

// the twelve bytes at `s`, of any alignment, out of the aligned dwords that cover them
__device__ inline void fetch12(const uint8_t* s, uint32_t d[3]) {
  const uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
  const uint32_t* w = (const uint32_t*)(s - sh);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = sh ? w[3] : 0u;      // byte s + 11 lies in w[3] exactly when sh != 0
  d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  d[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
}
// the four bytes at `m` likewise
__device__ inline uint32_t fetch4(const uint8_t* m) {
  const uint32_t sh = (uint32_t)(uintptr_t)m & 3u;
  const uint32_t* w = (const uint32_t*)(m - sh);
  const uint32_t w0 = w[0], w1 = sh ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(w1, w0, sh);
}

struct sample_args {
  float alpha, offset;       // offset as C's `float + int` converts it
  bool inside;               // BLEND: 0 <= alpha <= 1
};

__device__ inline uint32_t clip_float(float t) {          // libImaging's CHOP clip of a float result
  if (t <= 0.f) return 0;
  if (t >= 255.f) return 255;
  return (uint32_t)(int)t;
}

// one sample of R; m: the mask's value (PASTE under a mask)
template <int OP, int MK>
__device__ inline uint32_t sample(uint32_t a, uint32_t b, uint32_t m, const sample_args& k) {
  switch (OP) {
    case TA_COMBINE_PASTE: {
      if (MK == TA_MASK_NONE) return b;
      const uint32_t t = a * (255u - m) + b * m + 128u;
      return ((t >> 8) + t) >> 8;
    }
    case TA_COMBINE_BLEND: return blend(a, b, k.alpha, k.inside);
    case TA_COMBINE_LIGHTER: return max(a, b);
    case TA_COMBINE_DARKER: return min(a, b);
    case TA_COMBINE_DIFFERENCE: return a > b ? a - b : b - a;
    case TA_COMBINE_MULTIPLY: return a * b / 255u;
    case TA_COMBINE_SCREEN: return 255u - (255u - a) * (255u - b) / 255u;
    case TA_COMBINE_ADD: return clip_float(__fadd_rn(__fdiv_rn((float)(int)(a + b), k.alpha), k.offset));
    case TA_COMBINE_SUBTRACT: return clip_float(__fadd_rn(__fdiv_rn((float)((int)a - (int)b), k.alpha), k.offset));
    case TA_COMBINE_ADD_MODULO: return (a + b) & 255u;
    case TA_COMBINE_SUBTRACT_MODULO: return (a - b) & 255u;
    case TA_COMBINE_SOFT_LIGHT:
      return (((255u - a) * (a * b)) / 65536u + (a * (255u - ((255u - a) * (255u - b) / 255u))) / 255u) & 255u;
    case TA_COMBINE_HARD_LIGHT: return (b < 128u ? a * b / 127u : 255u - (255u - b) * (255u - a) / 127u) & 255u;
    default: return (a < 128u ? a * b / 127u : 255u - (255u - a) * (255u - b) / 127u) & 255u;      // OVERLAY
  }
}

template <int OP, int MK>
__device__ inline void run(uint8_t* dst, int H, int W, const uint8_t* src, const uint8_t* mask_base, const combine_rec& q,
                           const strip_item& it, const int2* __restrict__ tabs) {
  sample_args k;
  k.alpha = q.alpha, k.offset = (float)q.offset, k.inside = q.alpha >= 0.f && q.alpha <= 1.f;
  const uint32_t mconst = (uint32_t)q.mask_value, band = (uint32_t)q.mask_band;
  walk_strip(dst, H, W, q, it, tabs, [&](uint8_t* p, int npx, int r, int sx) {
    const uint8_t* s = src + q.src_off + (size_t)r * (size_t)q.src_pitch + 3 * sx;
    const uint8_t* mrow = nullptr;                                         // the mask row's entry for pixel sx
    if (MK == TA_MASK_BITMAP) mrow = mask_base + q.mask_off + (size_t)r * (size_t)q.mask_pitch + sx;
    if (MK == TA_MASK_FRAMES) mrow = mask_base + q.mask_off + (size_t)r * (size_t)q.mask_pitch + 3 * sx;
    walk_row(
        p, npx, threadIdx.x % WALK_WAVE,
        [&](uint8_t* px) {
          const int at = (int)(px - p);                                    // 3 x the pixel's index in the span
          const uint8_t* sp = s + at;
          uint32_t m = mconst;
          if (MK == TA_MASK_BITMAP) m = mrow[at / 3];
          if (MK == TA_MASK_FRAMES) m = mrow[at + band];
          px[0] = (uint8_t)sample<OP, MK>(px[0], sp[0], m, k);
          px[1] = (uint8_t)sample<OP, MK>(px[1], sp[1], m, k);
          px[2] = (uint8_t)sample<OP, MK>(px[2], sp[2], m, k);
        },
        [&](uint8_t* px) {
          const int at = (int)(px - p);
          uint32_t* d = (uint32_t*)px;
          uint32_t sd[3];
          fetch12(s + at, sd);
          if (OP == TA_COMBINE_PASTE && MK == TA_MASK_NONE) {
            d[0] = sd[0], d[1] = sd[1], d[2] = sd[2];
            return;
          }
          uint32_t m[4] = {mconst, mconst, mconst, mconst};
          if (MK == TA_MASK_BITMAP) {
            const uint32_t md = fetch4(mrow + at / 3);
            m[0] = md & 255u, m[1] = md >> 8 & 255u, m[2] = md >> 16 & 255u, m[3] = md >> 24;
          }
          if (MK == TA_MASK_FRAMES) {
            uint32_t md[3];
            fetch12(mrow + at, md);
            const quad mq = unpack(md[0], md[1], md[2]);
            for (int j = 0; j < 4; ++j) m[j] = band == 0 ? mq.r[j] : band == 1 ? mq.g[j] : mq.b[j];
          }
          quad a = unpack(d[0], d[1], d[2]);
          const quad b = unpack(sd[0], sd[1], sd[2]);
          for (int j = 0; j < 4; ++j) {
            a.r[j] = sample<OP, MK>(a.r[j], b.r[j], m[j], k);
            a.g[j] = sample<OP, MK>(a.g[j], b.g[j], m[j], k);
            a.b[j] = sample<OP, MK>(a.b[j], b.b[j], m[j], k);
          }
          pack(a, d);
        });
  });
}

// dst and src carry no __restrict__: they may be one batch (the host lets no frame be both written and read)
__global__ __launch_bounds__(THREADS) void combine_kernel(uint8_t* dst, int H, int W, const uint8_t* src, const uint8_t* mask_frames,
                                                          const uint8_t* bitmaps, const combine_rec* __restrict__ recs,
                                                          const strip_item* __restrict__ items, const int2* __restrict__ tabs) {
  const strip_item it = items[blockIdx.x];
  const combine_rec q = recs[it.rec];
#define TA_RUN(OP, MK, BASE)                              \
  run<OP, MK>(dst, H, W, src, BASE, q, it, tabs); \
  break
  switch (q.op) {
    case TA_COMBINE_PASTE:
      switch (q.mask_kind) {
        case TA_MASK_NONE: TA_RUN(TA_COMBINE_PASTE, TA_MASK_NONE, nullptr);
        case TA_MASK_CONSTANT: TA_RUN(TA_COMBINE_PASTE, TA_MASK_CONSTANT, nullptr);
        case TA_MASK_BITMAP: TA_RUN(TA_COMBINE_PASTE, TA_MASK_BITMAP, bitmaps);
        default: TA_RUN(TA_COMBINE_PASTE, TA_MASK_FRAMES, mask_frames);
      }
      break;
    case TA_COMBINE_BLEND: TA_RUN(TA_COMBINE_BLEND, TA_MASK_NONE, nullptr);
    case TA_COMBINE_LIGHTER: TA_RUN(TA_COMBINE_LIGHTER, TA_MASK_NONE, nullptr);
    case TA_COMBINE_DARKER: TA_RUN(TA_COMBINE_DARKER, TA_MASK_NONE, nullptr);
    case TA_COMBINE_DIFFERENCE: TA_RUN(TA_COMBINE_DIFFERENCE, TA_MASK_NONE, nullptr);
    case TA_COMBINE_MULTIPLY: TA_RUN(TA_COMBINE_MULTIPLY, TA_MASK_NONE, nullptr);
    case TA_COMBINE_SCREEN: TA_RUN(TA_COMBINE_SCREEN, TA_MASK_NONE, nullptr);
    case TA_COMBINE_ADD: TA_RUN(TA_COMBINE_ADD, TA_MASK_NONE, nullptr);
    case TA_COMBINE_SUBTRACT: TA_RUN(TA_COMBINE_SUBTRACT, TA_MASK_NONE, nullptr);
    case TA_COMBINE_ADD_MODULO: TA_RUN(TA_COMBINE_ADD_MODULO, TA_MASK_NONE, nullptr);
    case TA_COMBINE_SUBTRACT_MODULO: TA_RUN(TA_COMBINE_SUBTRACT_MODULO, TA_MASK_NONE, nullptr);
    case TA_COMBINE_SOFT_LIGHT: TA_RUN(TA_COMBINE_SOFT_LIGHT, TA_MASK_NONE, nullptr);
    case TA_COMBINE_HARD_LIGHT: TA_RUN(TA_COMBINE_HARD_LIGHT, TA_MASK_NONE, nullptr);
    default: TA_RUN(TA_COMBINE_OVERLAY, TA_MASK_NONE, nullptr);
  }
#undef TA_RUN
}

// what is wrong with a region before any frame is looked at, or nullptr
const char* own_defect(const ta_combine_region& q, const ta_frames* mask_frames, const uint8_t* masks, size_t mask_bytes) {
  if (q.op < TA_COMBINE_PASTE || q.op > TA_COMBINE_OVERLAY) return "unknown op";
  if (q.mask_kind < TA_MASK_NONE || q.mask_kind > TA_MASK_FRAMES) return "unknown mask kind";
  if (q.mask_kind != TA_MASK_NONE && q.op != TA_COMBINE_PASTE) return "a mask on an op other than PASTE";
  if (!isfinite(q.alpha)) return "alpha / scale not finite";
  if ((q.op == TA_COMBINE_ADD || q.op == TA_COMBINE_SUBTRACT) && q.alpha == 0.f) return "scale is 0";
  if (q.mask_kind == TA_MASK_CONSTANT && (q.mask_value < 0 || q.mask_value > 255)) return "mask value outside 0 .. 255";
  if (q.mask_kind == TA_MASK_BITMAP) {
    if (!masks) return "a bitmap mask, but masks is NULL";
    const uint64_t need = (uint64_t)(q.x1 - q.x0) * (uint64_t)(q.y1 - q.y0);       // the box is neither empty nor inverted here
    if (q.mask_value < 0 || (uint64_t)q.mask_value + need > (uint64_t)mask_bytes) return "the bitmap reaches past mask_bytes";
  }
  if (q.mask_kind == TA_MASK_FRAMES) {
    if (!mask_frames) return "a frames mask, but mask_frames is NULL";
    if (q.mask_band < 0 || q.mask_band > 2) return "mask band outside 0 .. 2";
  }
  return nullptr;
}

// the equally sized box at (x, y) of frame `f` of `b` lies inside it
int check_read_box(ta_ctx* ctx, int i, const char* what, const ta_frames* b, int f, int x, int y, int w, int h) {
  if (f < 0 || f >= b->n) return ta_fail(ctx, TA_E_INVALID, "frames_combine: region %d: %s frame %d out of range [0, %d)", i, what, f, b->n);
  if (x < 0 || y < 0 || x > b->w - w || y > b->h - h)
    return ta_fail(ctx, TA_E_INVALID, "frames_combine: region %d: the %s box [%d, %d) x [%d, %d) is not inside the %d x %d frame", i, what,
                   x, x + w, y, y + h, b->w, b->h);
  return TA_OK;
}

}  // namespace

extern "C" int ta_frames_combine(ta_ctx* ctx, ta_frames* dst, const ta_frames* src, const ta_frames* mask_frames,
                                 const ta_combine_region* regions, int n, const uint8_t* masks, size_t mask_bytes) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  const char* who = "frames_combine";
  if (!src) return ta_fail(ctx, TA_E_INVALID, "%s: bad args", who);
  TA_TRY(ta_check_batch(ctx, who, dst, regions, n));
  if (src->ctx->device != ctx->device || (mask_frames && mask_frames->ctx->device != ctx->device))
    return ta_fail(ctx, TA_E_INVALID, "%s: a batch lives on another device", who);
  TA_TRY(ta_check_boxes(ctx, who, dst, regions, n, MAX_SIDE,
                        [&](const ta_combine_region& q) { return own_defect(q, mask_frames, masks, mask_bytes); }));
  bool bitmaps = false;
  for (int i = 0; i < n; ++i) {
    const ta_combine_region& q = regions[i];
    const int w = q.x1 - q.x0, h = q.y1 - q.y0;
    TA_TRY(check_read_box(ctx, i, "source", src, q.src_frame, q.src_x, q.src_y, w, h));
    if (q.mask_kind == TA_MASK_FRAMES) TA_TRY(check_read_box(ctx, i, "mask", mask_frames, q.mask_frame, q.mask_x, q.mask_y, w, h));
    bitmaps |= q.mask_kind == TA_MASK_BITMAP;
  }
  // a batch that is both written and read: no frame may be both
  const bool src_is_dst = src->dev == dst->dev, mask_is_dst = mask_frames && mask_frames->dev == dst->dev;
  if (src_is_dst || mask_is_dst) {
    std::set<int32_t> written;
    for (int i = 0; i < n; ++i) written.insert(regions[i].frame);
    for (int i = 0; i < n; ++i) {
      const ta_combine_region& q = regions[i];
      if (src_is_dst && written.count(q.src_frame))
        return ta_fail(ctx, TA_E_INVALID, "%s: region %d: its source frame %d is a frame the call writes", who, i, q.src_frame);
      if (mask_is_dst && q.mask_kind == TA_MASK_FRAMES && written.count(q.mask_frame))
        return ta_fail(ctx, TA_E_INVALID, "%s: region %d: its mask frame %d is a frame the call writes", who, i, q.mask_frame);
    }
  }
  if (n == 0) return TA_OK;

  // a record per region, round by round, the strips of every round (one workgroup each), the ellipse span tables
  std::vector<combine_rec> recs;
  std::vector<strip_item> items;
  ta_span_tables spans;
  std::vector<std::pair<int, int>> launches;       // first strip and strips of every round
  size_t closed = 0;
  ta_each_round(
      regions, n,
      [&](const ta_combine_region& q) {
        combine_rec r;
        memset(&r, 0, sizeof(r));
        r.frame = q.frame, r.x0 = q.x0, r.y0 = q.y0, r.w = q.x1 - q.x0, r.h = q.y1 - q.y0;
        r.tab = q.shape == TA_BLUR_ELLIPSE ? spans.of(r.w, r.h) : -1;
        r.op = q.op, r.mask_kind = q.mask_kind, r.alpha = q.alpha, r.offset = q.offset;
        r.src_pitch = src->w * 3;
        r.src_off = (((uint64_t)q.src_frame * src->h + q.src_y) * (uint64_t)src->w + q.src_x) * 3;
        if (q.mask_kind == TA_MASK_CONSTANT) r.mask_value = q.mask_value;
        if (q.mask_kind == TA_MASK_BITMAP) r.mask_off = (uint64_t)q.mask_value, r.mask_pitch = r.w;
        if (q.mask_kind == TA_MASK_FRAMES) {
          r.mask_pitch = mask_frames->w * 3, r.mask_band = q.mask_band;
          r.mask_off = (((uint64_t)q.mask_frame * mask_frames->h + q.mask_y) * (uint64_t)mask_frames->w + q.mask_x) * 3;
        }
        recs.push_back(r);
      },
      [&] {
        const int at = (int)items.size();
        launches.push_back({at, ta_add_strips(items, recs, closed, WALK_WAVES, STRIP_PIXELS)});
        closed = recs.size();
      });
  ta_staging st;                                    // one H2D copy; 16 bytes behind it, for the dword that covers a bitmap's last byte
  st.slack = 16;
  const size_t o_rec = st.put(recs), o_item = st.put(items), o_tab = st.put(spans.table());
  const size_t o_masks = bitmaps ? st.put(masks, mask_bytes, 16) : 0;
  TA_TRY(st.commit(ctx));
  for (const auto& L : launches)
    if (L.second)
      hipLaunchKernelGGL(combine_kernel, dim3(L.second), dim3(THREADS), 0, ctx->stream, dst->dev, dst->h, dst->w, (const uint8_t*)src->dev,
                         mask_frames ? (const uint8_t*)mask_frames->dev : nullptr, bitmaps ? st.dev<const uint8_t>(o_masks) : nullptr,
                         st.dev<const combine_rec>(o_rec), st.dev<const strip_item>(o_item) + L.first, st.dev<const int2>(o_tab));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
