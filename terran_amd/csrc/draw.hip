// ta_frames_draw / ta_frames_draw_masks: Pillow's ImageDraw.Draw(img, 'RGBA') primitives (terran/vis/pillow.py: rectangle
// outlines and fills, wide and thin lines, filled ellipses, draw.text's coverage bitmaps) rasterised into a resident frame
// batch in place, bit for bit.
//
// Host side (this file, C++): validation, a stable sort of the primitives by frame, the quadrilateral of every wide line
// (Pillow's ImagingDrawWideLine: libm hypot and double rounding, done here so the device never re-derives a vertex) and
// one span table per distinct ellipse box (Pillow's integer ellipse walk; a handful of shapes per call).  The coverage
// bitmaps of mask primitives (rasterised by the caller: FreeType is host code) ride in the same staging copy.
// Device side: one wave per frame row.  Every wave walks its frame's primitives in list order; for a primitive that covers
// its row it computes the row's spans (uniform over the wave) and lane l blends the pixels x with x % 64 == l.  A pixel is
// only ever read and written by one lane, in primitive order: the result does not depend on the launch geometry, and no
// pixel outside a primitive's spans is touched.  Compiled with -ffp-contract=off (build.py): the polygon scan's float
// arithmetic must round as Pillow's C does.
#include "frame_regions.h"

#include <math.h>

namespace {

enum { K_BAR = 0, K_THIN = 1, K_QUAD = 2, K_DISC = 3, K_MASK = 4 };

struct draw_rec {          // 64 bytes
  int32_t kind;
  uint32_t rgba;           // r | g << 8 | b << 16 | a << 24
  int32_t v[8];            // BAR: x0, x1 | THIN: x0, y0, x1, y1 | QUAD: vertices (x, y) x 4 | DISC: x0, y0, table offset
                           // MASK: x0, x1, y0, byte offset of the bitmap (its pitch is x1 - x0 + 1)
  float dx[4];             // QUAD: edge i runs v[i] -> v[i + 1]; slope (x1 - x0) / (y1 - y0) as Pillow's add_edge computes it
  int32_t pymax;           // QUAD: the scan's last row as Pillow clamps it (min(H, max(0, ymax)))
  int32_t pad[1];
};
static_assert(sizeof(draw_rec) == 64, "draw_rec");

// ---- the polygon scan of one row (Pillow's polygon_generic with hasAlpha: every pixel once) --------------------------
struct edge_t {
  int x0, y0, xmin, xmax, ymin, ymax;
  float dx;
};

__device__ inline float edge_x(const edge_t& e, int y) { return (float)(y - e.y0) * e.dx + (float)e.x0; }
__device__ inline int round_up(float f) { return f >= 0.f ? (int)floorf(f + 0.5f) : -(int)floorf(fabsf(f) + 0.5f); }
__device__ inline int round_down(float f) { return f >= 0.f ? (int)ceilf(f - 0.5f) : -(int)ceilf(fabsf(f) - 0.5f); }

// Every array below is indexed with compile-time constants only (unrolled loops, selects): the row scan lives in registers.

// horizontal edges of the row that start at or before xpos (Pillow's draw_horizontal_lines)
template <class F>
__device__ inline void quad_hlines(const edge_t (&e)[4], int y, int& xpos, F&& emit) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (e[i].ymin != y || e[i].ymax != y) continue;
    int xmin = e[i].xmin;
    if (xpos != -1 && xpos < xmin) continue;
    const int xmax = e[i].xmax;
    if (xpos > xmin) {
      xmin = xpos;
      if (xmax < xmin) continue;
    }
    emit(xmin, xmax);
    xpos = xmax + 1;
  }
}

__device__ inline void xx_set(float (&xx)[8], int j, float v) {
#pragma unroll
  for (int s = 0; s < 8; ++s)
    if (s == j) xx[s] = v;
}

__device__ inline void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// the spans of row y of a wide line's quadrilateral, handed to emit(x_lo, x_hi) left to right, disjoint
template <class F>
__device__ void quad_row(const draw_rec& r, int y, F&& emit) {
  edge_t e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ax = r.v[2 * i], ay = r.v[2 * i + 1], bx = r.v[(2 * i + 2) & 7], by = r.v[(2 * i + 3) & 7];
    e[i].x0 = ax;
    e[i].y0 = ay;
    e[i].xmin = min(ax, bx);
    e[i].xmax = max(ax, bx);
    e[i].ymin = min(ay, by);
    e[i].ymax = max(ay, by);
    e[i].dx = r.dx[i];
  }
  const int pymax = r.pymax;
  float xx[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) xx[s] = INFINITY;      // unused slots sort to the end
  int j = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const edge_t& c = e[i];
    if (c.ymin == c.ymax || y < c.ymin || y > c.ymax) continue;
    float v = edge_x(c, y);
    xx_set(xx, j++, v);
    if (y == c.ymax && y < pymax) {
      xx_set(xx, j++, v);                              // "needed to draw consistent polygons"
    } else if (c.dx != 0.f && (j & 1) && roundf(v) == v) {
      bool done = false;                               // "connect discontiguous corners"
#pragma unroll
      for (int k = 0; k < i; ++k) {
        const edge_t& o = e[k];
        if (done || o.ymin == o.ymax) continue;
        if ((c.dx > 0.f && o.dx <= 0.f) || (c.dx < 0.f && o.dx >= 0.f)) continue;
        if (v == edge_x(o, y)) {
          const int off = y == pymax ? -1 : 1;
          const float a1 = edge_x(c, y + off);
          if (y + off >= o.ymin && y + off <= o.ymax) {
            const float a2 = edge_x(o, y + off);
            if (v > a1 + 1.f && v > a2 + 1.f)
              v = roundf(fmaxf(a1, a2)) + 1.f;
            else if (v < a1 - 1.f && v < a2 - 1.f)
              v = roundf(fminf(a1, a2)) - 1.f;
            xx_set(xx, j - 1, v);
            done = true;
          }
        }
      }
    }
  }
  // ascending: an 8-input sorting network (19 compare-exchanges)
  cswap(xx[0], xx[2]); cswap(xx[1], xx[3]); cswap(xx[4], xx[6]); cswap(xx[5], xx[7]);
  cswap(xx[0], xx[4]); cswap(xx[1], xx[5]); cswap(xx[2], xx[6]); cswap(xx[3], xx[7]);
  cswap(xx[0], xx[1]); cswap(xx[2], xx[3]); cswap(xx[4], xx[5]); cswap(xx[6], xx[7]);
  cswap(xx[2], xx[4]); cswap(xx[3], xx[5]);
  cswap(xx[1], xx[4]); cswap(xx[3], xx[6]);
  cswap(xx[1], xx[2]); cswap(xx[3], xx[4]); cswap(xx[5], xx[6]);
  int xpos = j == 0 ? -1 : 0;
#pragma unroll
  for (int i = 1; i < 8; i += 2) {
    if (i >= j) continue;
    const int xe = round_down(xx[i]);
    if (xe < xpos) continue;
    quad_hlines(e, y, xpos, emit);
    if (xe < xpos) continue;
    int xs = round_up(xx[i - 1]);
    if (xpos > xs) {
      xs = xpos;
      if (xe < xs) continue;
    }
    emit(xs, xe);
    xpos = xe + 1;
  }
  quad_hlines(e, y, xpos, emit);
}

__device__ inline int64_t ceil_div(int64_t a, int64_t b) {   // b > 0
  return a >= 0 ? (a + b - 1) / b : -((-a) / b);
}

// Pillow's thin line: Bresenham without its end point, then the end point.  Point i of the major axis lies at
// minor = floor((2 d_minor i + d_major) / (2 d_major)) (the error term's closed form, ties step).  -> false: row not hit
__device__ inline bool thin_row(const draw_rec& r, int y, int& lo_x, int& hi_x) {
  const int x0 = r.v[0], y0 = r.v[1], x1 = r.v[2], y1 = r.v[3];
  const int64_t dx = x1 >= x0 ? (int64_t)x1 - x0 : (int64_t)x0 - x1, dy = y1 >= y0 ? (int64_t)y1 - y0 : (int64_t)y0 - y1;
  const int xs = x1 >= x0 ? 1 : -1, ys = y1 >= y0 ? 1 : -1;
  const int64_t m = ys > 0 ? (int64_t)y - y0 : (int64_t)y0 - y;
  if (m < 0 || m > dy) return false;
  if (dx > dy) {
    int64_t lo = 0, hi = dx;
    if (dy) {
      lo = max((int64_t)0, ceil_div(2 * dx * m - dx, 2 * dy));
      hi = min(dx, ceil_div(2 * dx * m + dx, 2 * dy) - 1);
    }
    if (lo > hi) return false;
    lo_x = (int)(xs > 0 ? x0 + lo : x0 - hi);
    hi_x = (int)(xs > 0 ? x0 + hi : x0 - lo);
    return true;
  }
  if (dy == 0) {                                       // coincident end points
    lo_x = hi_x = x0;
    return true;
  }
  lo_x = hi_x = (int)(x0 + xs * ((2 * dx * m + dy) / (2 * dy)));
  return true;
}

__global__ __launch_bounds__(256) void draw_kernel(uint8_t* __restrict__ frames, int H, int W,
                                                   const int32_t* __restrict__ fstart, const int2* __restrict__ ybound,
                                                   const draw_rec* __restrict__ recs, const int2* __restrict__ disc_tab,
                                                   const uint8_t* __restrict__ masks) {
  const int f = blockIdx.y;
  const int y = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (y >= H) return;
  uint8_t* row = frames + ((size_t)f * H + y) * (size_t)W * 3;
  const int p1 = fstart[f + 1];
  for (int p = fstart[f]; p < p1; ++p) {
    const int2 yb = ybound[p];
    if (y < yb.x || y > yb.y) continue;
    const draw_rec& r = recs[p];
    const int ia = (int)(r.rgba >> 24), ib = 255 - ia;
    const int cr = (int)(r.rgba & 255) * ia + 128, cg = (int)((r.rgba >> 8) & 255) * ia + 128,
              cb = (int)((r.rgba >> 16) & 255) * ia + 128;
    auto blend = [&](int lo, int hi) {
      lo = max(lo, 0);
      hi = min(hi, W - 1);
      for (int x = (lo & ~63) + lane; x <= hi; x += 64) {   // pixel x belongs to lane x % 64, whatever the span
        if (x < lo) continue;
        uint8_t* px = row + (size_t)x * 3;
        const int vr = px[0] * ib + cr, vg = px[1] * ib + cg, vb = px[2] * ib + cb;
        px[0] = (uint8_t)(((vr >> 8) + vr) >> 8);
        px[1] = (uint8_t)(((vg >> 8) + vg) >> 8);
        px[2] = (uint8_t)(((vb >> 8) + vb) >> 8);
      }
    };
    if (r.kind == K_BAR) {
      blend(r.v[0], r.v[1]);
    } else if (r.kind == K_THIN) {
      int lo, hi;
      if (thin_row(r, y, lo, hi)) blend(lo, hi);
    } else if (r.kind == K_QUAD) {
      quad_row(r, y, blend);
    } else if (r.kind == K_MASK) {
      // the bitmap's row is contiguous: the 64 lanes read 64 consecutive bytes; coverage m plays the alpha
      const int x0 = r.v[0], lo = max(x0, 0), hi = min(r.v[1], W - 1);
      const uint8_t* mrow = masks + (size_t)r.v[3] + (size_t)(y - r.v[2]) * (size_t)(r.v[1] - x0 + 1);
      const int ir = (int)(r.rgba & 255), ig = (int)((r.rgba >> 8) & 255), ibl = (int)((r.rgba >> 16) & 255);
      for (int x = (lo & ~63) + lane; x <= hi; x += 64) {
        if (x < lo) continue;
        const int m = mrow[x - x0];
        if (m == 0) continue;
        uint8_t* px = row + (size_t)x * 3;
        const int vr = px[0] * (255 - m) + ir * m + 128, vg = px[1] * (255 - m) + ig * m + 128,
                  vb = px[2] * (255 - m) + ibl * m + 128;
        px[0] = (uint8_t)(((vr >> 8) + vr) >> 8);
        px[1] = (uint8_t)(((vg >> 8) + vg) >> 8);
        px[2] = (uint8_t)(((vb >> 8) + vb) >> 8);
      }
    } else {
      const int2 t = disc_tab[r.v[2] + (y - r.v[1])];
      blend(r.v[0] + t.x, r.v[0] + t.y);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
inline int round_up_d(double f) { return (int)(f >= 0.0 ? floor(f + 0.5F) : -floor(fabs(f) + 0.5F)); }
inline int round_down_d(double f) { return (int)(f >= 0.0 ? ceil(f - 0.5F) : -ceil(fabs(f) - 0.5F)); }

// Pillow's ellipse walk (ellipse_init / ellipse_next with width = a + b, i.e. filled): per row of the box the span
// [x0 + lo, x0 + hi] (lo > hi: nothing), rows 0..b.
struct quarter {
  int32_t cx, cy, ex, ey;
  int64_t a2, b2, a2b2;
  bool finished;
  quarter(int32_t a, int32_t b) {
    finished = a < 0 || b < 0;
    if (finished) return;
    cx = a;
    cy = b % 2;
    ex = a % 2;
    ey = b;
    a2 = (int64_t)a * a;
    b2 = (int64_t)b * b;
    a2b2 = a2 * b2;
  }
  int64_t delta(int64_t x, int64_t y) const {
    const int64_t d = a2 * y * y + b2 * x * x - a2b2;
    return d < 0 ? -d : d;
  }
  bool next(int32_t* rx, int32_t* ry) {
    if (finished) return false;
    *rx = cx;
    *ry = cy;
    if (cx == ex && cy == ey) {
      finished = true;
    } else {
      int32_t nx = cx, ny = cy + 2;
      int64_t nd = delta(nx, ny);
      if (nx > 1) {
        int64_t d = delta(cx - 2, cy + 2);
        if (nd > d) {
          nx = cx - 2;
          ny = cy + 2;
          nd = d;
        }
        d = delta(cx - 2, cy);
        if (nd > d) {
          nx = cx - 2;
          ny = cy;
        }
      }
      cx = nx;
      cy = ny;
    }
    return true;
  }
};

void disc_rows(int a, int b, std::vector<int2>& tab) {
  const size_t base = tab.size();
  tab.resize(base + b + 1, make_int2(1, 0));
  auto put = [&](int X0, int Y, int X1) {
    const int row = (Y + b) / 2, lo = (X0 + a) / 2, hi = (X1 + a) / 2;
    int2& t = tab[base + row];
    if (t.x > t.y) t = make_int2(lo, hi);
    else t = make_int2(std::min(t.x, lo), std::max(t.y, hi));   // the walk's left and right halves of one row
  };
  quarter o(a, b);
  int32_t pr, py;
  if (a + b < 1 || !o.next(&pr, &py)) return;
  const int l = a % 2;                                // a filled ellipse has no inner rim: the left end stays `leftmost`
  bool finished = false;
  while (!finished) {
    const int32_t y = py, r = pr;
    int32_t cx = 0, cy = 0;
    bool more;
    while ((more = o.next(&cx, &cy)) && cy <= y) {
    }
    if (!more) finished = true;
    else {
      pr = cx;
      py = cy;
    }
    if ((l > 0 || r > 0) && y > 0) put(l == 0 ? 2 : l, y, r);
    if (y > 0) put(-r, y, -l);
    if (l > 0 || r > 0) put(l == 0 ? 2 : l, -y, r);
    put(-r, -y, -l);
  }
}

// both entry points; `with_masks`: TA_DRAW_MASK is a known kind and `masks` (mask_bytes bytes, may be NULL) holds the bitmaps
int draw(ta_ctx* ctx, ta_frames* frames, const ta_draw_prim* prims, int n, bool with_masks, const uint8_t* masks,
         size_t mask_bytes) {
  TA_TRY(ta_check_batch(ctx, "frames_draw", frames, prims, n));
  const int N = frames->n, H = frames->h, W = frames->w;
  const int LIM = 1 << 24;
  for (int i = 0; i < n; ++i) {
    const ta_draw_prim& q = prims[i];
    if (q.frame < 0 || q.frame >= N) return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: frame %d out of range [0, %d)", i, q.frame, N);
    if (q.kind != TA_DRAW_BAR && q.kind != TA_DRAW_LINE && q.kind != TA_DRAW_DISC && !(with_masks && q.kind == TA_DRAW_MASK))
      return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: unknown kind %d", i, q.kind);
    if (std::abs((int64_t)q.x0) > LIM || std::abs((int64_t)q.y0) > LIM || std::abs((int64_t)q.x1) > LIM || std::abs((int64_t)q.y1) > LIM)
      return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: coordinate beyond +-2^24", i);
    if (q.kind != TA_DRAW_LINE && (q.x1 < q.x0 || q.y1 < q.y0))
      return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: x1 < x0 or y1 < y0", i);
    if (q.kind == TA_DRAW_DISC && (q.x1 - q.x0 > 32768 || q.y1 - q.y0 > 32768))
      return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: ellipse box larger than 32768", i);
    if (q.kind == TA_DRAW_LINE && q.width < 0) return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: negative width", i);
    if (q.kind == TA_DRAW_MASK) {
      if (q.rgba[3] != 255) return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: a mask's alpha must be 255", i);
      if (!masks) return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: a mask primitive, but no masks", i);
      if (q.width < 0) return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: negative mask offset", i);
      const uint64_t end = (uint64_t)q.width + (uint64_t)(q.x1 - q.x0 + 1) * (uint64_t)(q.y1 - q.y0 + 1);   // < 2^52
      if (end > (uint64_t)mask_bytes)
        return ta_fail(ctx, TA_E_INVALID, "frames_draw: primitive %d: mask reaches byte %llu of %llu", i, (unsigned long long)end,
                       (unsigned long long)mask_bytes);
    }
  }
  if (n == 0 || N == 0 || H == 0 || W == 0) return TA_OK;

  // stable order by frame
  std::vector<int32_t> fstart(N + 1, 0);
  for (int i = 0; i < n; ++i) fstart[prims[i].frame + 1]++;
  for (int f = 0; f < N; ++f) fstart[f + 1] += fstart[f];
  std::vector<int32_t> order(n), fill(fstart.begin(), fstart.end() - 1);
  for (int i = 0; i < n; ++i) order[fill[prims[i].frame]++] = i;

  std::vector<draw_rec> recs(n);
  std::vector<int2> yb(n);
  ta_span_tables spans(false);                          // relative to the primitive's corner, not clamped: the kernel clips
  for (int k = 0; k < n; ++k) {
    const ta_draw_prim& q = prims[order[k]];
    draw_rec& r = recs[k];
    memset(&r, 0, sizeof(r));
    r.rgba = (uint32_t)q.rgba[0] | (uint32_t)q.rgba[1] << 8 | (uint32_t)q.rgba[2] << 16 | (uint32_t)q.rgba[3] << 24;
    int ylo, yhi;
    if (q.kind == TA_DRAW_BAR) {
      r.kind = K_BAR;
      r.v[0] = q.x0;
      r.v[1] = q.x1;
      ylo = q.y0;
      yhi = q.y1;
      if (q.x1 < 0 || q.x0 >= W) ylo = 1, yhi = 0;
    } else if (q.kind == TA_DRAW_MASK) {
      r.kind = K_MASK;
      r.v[0] = q.x0;
      r.v[1] = q.x1;
      r.v[2] = q.y0;
      r.v[3] = q.width;
      ylo = q.y0;
      yhi = q.y1;
      if (q.x1 < 0 || q.x0 >= W) ylo = 1, yhi = 0;
    } else if (q.kind == TA_DRAW_DISC) {
      const int a = q.x1 - q.x0, b = q.y1 - q.y0;
      r.kind = K_DISC;
      r.v[0] = q.x0;
      r.v[1] = q.y0;
      r.v[2] = spans.of(a + 1, b + 1);                  // ellipse([0, 0, a, b])
      ylo = q.y0;
      yhi = q.y1;
      if (a + b < 1) ylo = 1, yhi = 0;                 // Pillow draws nothing for a one-pixel box
    } else if (q.width <= 1 || (q.x0 == q.x1 && q.y0 == q.y1)) {
      r.kind = K_THIN;                                  // coincident end points: the single point either way
      r.v[0] = q.x0;
      r.v[1] = q.y0;
      r.v[2] = q.x1;
      r.v[3] = q.y1;
      ylo = std::min(q.y0, q.y1);
      yhi = std::max(q.y0, q.y1);
    } else {
      // ImagingDrawWideLine: the quadrilateral around the segment
      const int dx = q.x1 - q.x0, dy = q.y1 - q.y0;
      const double big = hypot((double)dx, (double)dy);
      const double small = (q.width - 1) / 2.0;
      const double ratio_max = round_up_d(small) / big, ratio_min = round_down_d(small) / big;
      const int dxmin = round_down_d(ratio_min * dy), dxmax = round_down_d(ratio_max * dy);
      const int dymin = round_down_d(ratio_min * dx), dymax = round_down_d(ratio_max * dx);
      const int v[8] = {q.x0 - dxmin, q.y0 + dymax, q.x1 - dxmin, q.y1 + dymax,
                        q.x1 + dxmax, q.y1 - dymin, q.x0 + dxmax, q.y0 - dymin};
      r.kind = K_QUAD;
      int emin = H - 1, emax = 0;
      for (int i = 0; i < 4; ++i) {
        const int ax = v[2 * i], ay = v[2 * i + 1], bx = v[(2 * i + 2) & 7], by = v[(2 * i + 3) & 7];
        r.v[2 * i] = ax;
        r.v[2 * i + 1] = ay;
        r.dx[i] = ay == by ? 0.f : (float)(bx - ax) / (by - ay);
        emin = std::min(emin, std::min(ay, by));
        emax = std::max(emax, std::max(ay, by));
      }
      r.pymax = std::min(H, std::max(0, emax));
      ylo = std::max(0, emin);
      yhi = r.pymax;
    }
    yb[k] = make_int2(std::max(ylo, 0), std::min(yhi, H - 1));
  }

  ta_staging st;                                        // one H2D copy; draw_kernel loads whole records: a 64-byte boundary
  const size_t o_fs = st.put(fstart), o_yb = st.put(yb), o_rec = st.put(recs, 64), o_tab = st.put(spans.table(), 8);
  const size_t o_mask = st.put(masks, masks ? mask_bytes : 0, 1);
  TA_TRY(st.commit(ctx));
  hipLaunchKernelGGL(draw_kernel, dim3((H + 3) / 4, N), dim3(256), 0, ctx->stream, frames->dev, H, W, st.dev<const int32_t>(o_fs),
                     st.dev<const int2>(o_yb), st.dev<const draw_rec>(o_rec), st.dev<const int2>(o_tab), st.dev<const uint8_t>(o_mask));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}

}  // namespace

void ta_disc_rows(int a, int b, std::vector<int2>& tab) { disc_rows(a, b, tab); }   // ta_frames_blur's ellipse shape

extern "C" int ta_frames_draw(ta_ctx* ctx, ta_frames* frames, const ta_draw_prim* prims, int n) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  return draw(ctx, frames, prims, n, false, nullptr, 0);
}

extern "C" int ta_frames_draw_masks(ta_ctx* ctx, ta_frames* frames, const ta_draw_prim* prims, int n, const uint8_t* masks,
                                    size_t mask_bytes) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  return draw(ctx, frames, prims, n, true, masks, mask_bytes);
}
