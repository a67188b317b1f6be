// Colour conversions on regions of a resident frame batch, in place and bit for bit with Pillow (ta_frames_color):
//   TA_COLOR_MATRIX      im.convert('RGB', m)                  libImaging/Matrix.c
//   TA_COLOR_RGB2YCBCR   im.convert('YCbCr'), and _YCBCR2RGB   libImaging/ConvertYCbCr.c
//   TA_COLOR_RGB2HSV     im.convert('HSV'), and _HSV2RGB       libImaging/Convert.c
//   TA_COLOR_LUT3D       im.filter(ImageFilter.Color3DLUT)     libImaging/ColorLUT.c, _imaging.c's table preparation
// each pasted back into its box under the region's shape.  The float steps are C's as written there: float32 products and
// sums rounded one by one (matrix), double expressions over float32 operands that are rounded back to float32 (HSV); this
// unit is compiled with -ffp-contract=off (build.py) and the operations whose order matters are spelled with the _rn
// intrinsics besides.  YCbCr and the 3-D table are integer work on int16 tables that the host builds and stages.
//
// Device side: tone.hip's walk (pixel_walk.h): a workgroup takes a strip of rows of one region, its waves every fourth row,
// the lanes a head of single pixels, groups of four pixels = three aligned dwords and a tail, so no byte outside a region
// is touched.  A workgroup serves one region and so one op: the switch on its kind is uniform.  The YCbCr tables (6.5 KB)
// always sit in LDS.  A 3-D table is eight node reads per pixel, a node four int16 = one 8-byte read; a table of at most
// LDS_TABLE_BYTES (64 KiB of nodes, up to 20^3, so the usual 17^3) is copied into LDS by every workgroup -- 39 KB from
// L2 per strip of 16384 pixels, against 1 MB of node reads -- and a larger one (33^3: 287 KB, 65^3: 2.2 MB) is read
// where it lies: it fits the 4 MiB L2 of every XCD.  LDS is dynamic and sized per launch by what the round's ops need.
#include "ta_internal.h"
#include "pixel_walk.h"
#include "frame_regions.h"

#include <math.h>
#include <string.h>

#include <utility>
#include <vector>

namespace {

constexpr int THREADS = WALK_THREADS, WAVE = WALK_WAVE;
constexpr int MAX_SIDE = 16384;
constexpr int LUT_MIN = 2, LUT_MAX = 65;           // Color3DLUT's axis sizes
constexpr size_t LDS_TABLE_BYTES = 65536;          // a 3-D table up to this many bytes of nodes is held in LDS
constexpr int YCC_TABLES = 13, YCC_BYTES = YCC_TABLES * 256 * 2;
constexpr int SCALE_BITS = 18, SHIFT_BITS = 15, PRECISION_BITS = 6;       // ColorLUT.c

struct color_rec {           // 32 bytes
  int32_t frame, x0, y0, w, h;
  int32_t tab;               // ellipse: first row of the span table; box: -1
  int32_t op;
  int32_t pad;
};
static_assert(sizeof(color_rec) == 32, "color_rec");

struct color_dop {           // an op as the device reads it
  int32_t kind;
  int32_t s0, s01, count;    // LUT3D: nodes along R, nodes of an R-G plane, all nodes
  int32_t scale[3];          // LUT3D: (int)((s - 1) / 255.0 * 2^18) per axis
  uint32_t node0;            // LUT3D: its first node in the call's nodes
  int32_t in_lds;            // LUT3D: the table is copied into LDS
  float m[12];               // MATRIX
};
static_assert(sizeof(color_dop) == 84, "color_dop");

// the twelve bytes of a group, as in tone.hip
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

__device__ inline uint32_t clip8(int v) { return (uint32_t)min(max(v, 0), 255); }

// Matrix.c's CLIPF of m0 r + m1 g + m2 b + m3 + 0.5.  C adds the 0.5 in double and rounds to float32, which is the
// float32 addition (tests/color_model.py has the argument).
__device__ inline uint32_t matrix_band(const float* m, float r, float g, float b) {
  float v = __fmul_rn(m[0], r);
  v = __fadd_rn(v, __fmul_rn(m[1], g));
  v = __fadd_rn(v, __fmul_rn(m[2], b));
  v = __fadd_rn(__fadd_rn(v, m[3]), 0.5f);
  if (v <= 0.f) return 0;
  if (v >= 255.f) return 255;
  return (uint32_t)(int)v;
}

// t: the 13 tables of ycbcr_tables() below
__device__ inline void rgb2ycbcr(const int16_t* t, uint32_t& r, uint32_t& g, uint32_t& b) {
  const int y = (t[r] + t[256 + g] + t[512 + b]) >> 6;
  const int cb = ((t[768 + r] + t[1024 + g] + t[1280 + b]) >> 6) + 128;
  const int cr = ((t[1536 + r] + t[1792 + g] + t[2048 + b]) >> 6) + 128;
  r = (uint32_t)y & 255u, g = (uint32_t)cb & 255u, b = (uint32_t)cr & 255u;
}
__device__ inline void ycbcr2rgb(const int16_t* t, uint32_t& y, uint32_t& cb, uint32_t& cr) {
  const int r = (int)y + (t[2304 + cr] >> 6);
  const int g = (int)y + ((t[2560 + cb] + t[2816 + cr]) >> 6);
  const int b = (int)y + (t[3072 + cb] >> 6);
  y = clip8(r), cb = clip8(g), cr = clip8(b);
}

// Convert.c's rgb2hsv_row: the float32 quotients, the hue's 2.0 + rc - bc evaluated in double and rounded to float32
__device__ inline void rgb2hsv(uint32_t& r, uint32_t& g, uint32_t& b) {
  const int mx = (int)max(r, max(g, b)), mn = (int)min(r, min(g, b));
  if (mx == mn) {
    r = 0, g = 0, b = (uint32_t)mx;
    return;
  }
  const float cr = (float)(mx - mn);
  const float s = __fdiv_rn(cr, (float)mx);
  const float rc = __fdiv_rn((float)(mx - (int)r), cr), gc = __fdiv_rn((float)(mx - (int)g), cr), bc = __fdiv_rn((float)(mx - (int)b), cr);
  float h;
  if ((int)r == mx)
    h = __fsub_rn(bc, gc);
  else if ((int)g == mx)
    h = (float)__dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
  else
    h = (float)__dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
  const double x = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);      // 5/6 .. 11/6: fmod(x, 1.0) is x - floor(x), exact
  h = (float)(x - floor(x));
  r = clip8((int)__dmul_rn((double)h, 255.0));
  g = clip8((int)__dmul_rn((double)s, 255.0));
  b = (uint32_t)mx;
}

// Convert.c's hsv2rgb_row
__device__ inline uint32_t hsv_level(double v, double x) {
  const double y = (double)(float)__dmul_rn(v, x);                  // never negative: round() is floor(y + 0.5)
  return clip8((int)(y + 0.5));
}
__device__ inline void hsv2rgb(uint32_t& h, uint32_t& s, uint32_t& v) {
  if (s == 0) {
    h = v, s = v;
    return;
  }
  const double h6 = __ddiv_rn(__dmul_rn((double)(float)h, 6.0), 255.0);
  const double fl = floor(h6);
  const double f = (double)(float)__dsub_rn(h6, fl);
  const double fs = (double)(float)__ddiv_rn((double)s, 255.0);
  const double vd = (double)v;
  const uint32_t p = hsv_level(vd, __dsub_rn(1.0, fs));
  const uint32_t q = hsv_level(vd, __dsub_rn(1.0, __dmul_rn(fs, f)));
  const uint32_t t = hsv_level(vd, __dsub_rn(1.0, __dmul_rn(fs, __dsub_rn(1.0, f))));
  const uint32_t val = v;
  switch ((int)fl % 6) {
    case 0: h = val, s = t, v = p; break;
    case 1: h = q, s = val, v = p; break;
    case 2: h = p, s = val, v = t; break;
    case 3: h = p, s = q, v = val; break;
    case 4: h = t, s = p, v = val; break;
    default: h = val, s = p, v = q; break;
  }
}

// ColorLUT.c: the node and the 15-bit weight per axis, interpolation along R, then G, then B, every step
// (a (2^15 - w) + b w) >> 15 on signed values, then clip8((x + 32) >> 6).  255 never divides (s - 1) 2^18, so the node
// of 255 is s - 2 at most: node + 1 stays inside the table.
struct node3 {
  int c[3];
};
// clip8((x + 32) >> 6), clamped BEFORE the shift: hipcc turns two clamps of a shifted value into one v_ashr_pk_u8_i32
// and then ORs further bytes onto its result as if the upper half were zero, which it was not on gfx950 (bytes 2 and 3 of
// the packed dwords came out wrong); clamping first gives the same value and no such instruction
__device__ inline uint32_t round8(int x) {
  constexpr int HALF = 1 << (PRECISION_BITS - 1), TOP = (256 << PRECISION_BITS) - 1;
  return (uint32_t)min(max(x + HALF, 0), TOP) >> PRECISION_BITS;
}
__device__ inline node3 load_node(const uint2* nodes, uint32_t i) {
  const uint2 v = nodes[i];
  node3 n;
  n.c[0] = (int)(int16_t)(v.x & 0xffffu), n.c[1] = (int)v.x >> 16, n.c[2] = (int)(int16_t)(v.y & 0xffffu);
  return n;
}
__device__ inline node3 lerp(const node3& a, const node3& b, int w) {
  node3 o;
  for (int k = 0; k < 3; ++k) o.c[k] = (a.c[k] * ((1 << SHIFT_BITS) - w) + b.c[k] * w) >> SHIFT_BITS;
  return o;
}
__device__ inline void lut3d(const uint2* nodes, const color_dop& op, uint32_t& r, uint32_t& g, uint32_t& b) {
  constexpr int MASK = (1 << SCALE_BITS) - 1, DOWN = SCALE_BITS - SHIFT_BITS;
  const int i0 = (int)r * op.scale[0], i1 = (int)g * op.scale[1], i2 = (int)b * op.scale[2];
  const int w0 = (i0 & MASK) >> DOWN, w1 = (i1 & MASK) >> DOWN, w2 = (i2 & MASK) >> DOWN;
  const uint32_t s0 = (uint32_t)op.s0, s01 = (uint32_t)op.s01;
  const uint32_t at = (uint32_t)(i0 >> SCALE_BITS) + s0 * (uint32_t)(i1 >> SCALE_BITS) + s01 * (uint32_t)(i2 >> SCALE_BITS);
  const node3 ll = lerp(load_node(nodes, at), load_node(nodes, at + 1), w0);
  const node3 lr = lerp(load_node(nodes, at + s0), load_node(nodes, at + s0 + 1), w0);
  const node3 rl = lerp(load_node(nodes, at + s01), load_node(nodes, at + s01 + 1), w0);
  const node3 rr = lerp(load_node(nodes, at + s01 + s0), load_node(nodes, at + s01 + s0 + 1), w0);
  const node3 x = lerp(lerp(ll, lr, w1), lerp(rl, rr, w1), w2);
  r = round8(x.c[0]), g = round8(x.c[1]), b = round8(x.c[2]);
}

// every pixel of the workgroup's strip through f(r, g, b), in place
template <class F>
__device__ inline void each_pixel(uint8_t* frames, int H, int W, const color_rec& q, const strip_item& it, const int2* __restrict__ tabs, F f) {
  walk_strip(frames, H, W, q, it, tabs, [&](uint8_t* p, int npx, int, int) {
    walk_row(
        p, npx, threadIdx.x % WAVE,
        [&](uint8_t* px) {
          uint32_t r = px[0], g = px[1], b = px[2];
          f(r, g, b);
          px[0] = (uint8_t)r, px[1] = (uint8_t)g, px[2] = (uint8_t)b;
        },
        [&](uint8_t* px) {
          uint32_t* d = (uint32_t*)px;
          quad v = unpack(d[0], d[1], d[2]);
          for (int k = 0; k < 4; ++k) f(v.r[k], v.g[k], v.b[k]);
          pack(v, d);
        });
  });
}

extern __shared__ uint2 color_lds[];       // the YCbCr tables or the op's 3-D table; sized by the launch

__global__ __launch_bounds__(THREADS) void color_kernel(uint8_t* __restrict__ frames, int H, int W, const color_rec* __restrict__ recs,
                                                        const strip_item* __restrict__ items, const int2* __restrict__ tabs,
                                                        const color_dop* __restrict__ ops, const uint2* __restrict__ ycc,
                                                        const uint2* __restrict__ nodes) {
  const strip_item it = items[blockIdx.x];
  const color_rec q = recs[it.rec];
  const color_dop op = ops[q.op];
  switch (op.kind) {
    case TA_COLOR_MATRIX:
      each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) {
        const float fr = (float)(int)r, fg = (float)(int)g, fb = (float)(int)b;
        r = matrix_band(op.m, fr, fg, fb), g = matrix_band(op.m + 4, fr, fg, fb), b = matrix_band(op.m + 8, fr, fg, fb);
      });
      break;
    case TA_COLOR_RGB2YCBCR:
    case TA_COLOR_YCBCR2RGB: {
      for (int i = threadIdx.x; i < YCC_BYTES / 8; i += THREADS) color_lds[i] = ycc[i];
      __syncthreads();
      const int16_t* t = (const int16_t*)color_lds;
      if (op.kind == TA_COLOR_RGB2YCBCR)
        each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { rgb2ycbcr(t, r, g, b); });
      else
        each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { ycbcr2rgb(t, r, g, b); });
      break;
    }
    case TA_COLOR_RGB2HSV:
      each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { rgb2hsv(r, g, b); });
      break;
    case TA_COLOR_HSV2RGB:
      each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { hsv2rgb(r, g, b); });
      break;
    default: {                                       // TA_COLOR_LUT3D: the host lets no other kind through
      const uint2* mine = nodes + op.node0;
      if (op.in_lds) {
        for (int i = threadIdx.x; i < op.count; i += THREADS) color_lds[i] = mine[i];
        __syncthreads();
        each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { lut3d(color_lds, op, r, g, b); });
      } else {
        each_pixel(frames, H, W, q, it, tabs, [&](uint32_t& r, uint32_t& g, uint32_t& b) { lut3d(mine, op, r, g, b); });
      }
      break;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// ConvertYCbCr.c's tables: Y_R Y_G Y_B Cb_R Cb_G Cb_B Cr_R Cr_G Cr_B over i, then R_Cr G_Cb G_Cr B_Cb over i - 128; every
// entry (int)(c 64 i + 0.5), C's truncating cast, so a negative entry is rounded up
const std::vector<int16_t>& ycbcr_tables() {
  static const std::vector<int16_t> t = [] {
    const double c[YCC_TABLES] = {0.299, 0.587, 0.114, -0.16874, -0.33126, 0.5, 0.5, -0.41869, -0.08131, 1.402, -0.34414, -0.71414, 1.772};
    std::vector<int16_t> v(YCC_TABLES * 256);
    for (int k = 0; k < YCC_TABLES; ++k)
      for (int i = 0; i < 256; ++i) v[k * 256 + i] = (int16_t)(int)(c[k] * 64 * (k < 9 ? i : i - 128) + 0.5);
    return v;
  }();
  return t;
}

size_t lut_nodes(const ta_color_op& o) { return (size_t)o.size[0] * o.size[1] * o.size[2]; }

// what is wrong with an op, or nullptr
const char* check_op(const ta_color_op& o, const float* tables, size_t n_tables) {
  size_t need = 0;
  switch (o.kind) {
    case TA_COLOR_MATRIX: need = 12; break;
    case TA_COLOR_RGB2YCBCR:
    case TA_COLOR_YCBCR2RGB:
    case TA_COLOR_RGB2HSV:
    case TA_COLOR_HSV2RGB: return nullptr;
    case TA_COLOR_LUT3D:
      for (int k = 0; k < 3; ++k)
        if (o.size[k] < LUT_MIN || o.size[k] > LUT_MAX) return "an axis outside 2 .. 65";
      need = 3 * lut_nodes(o);
      break;
    default: return "unknown kind";
  }
  if (!tables || o.table < 0) return "its table is missing";
  if ((size_t)o.table > n_tables || need > n_tables - (size_t)o.table) return "its table reaches past n_tables";
  for (size_t i = 0; i < need; ++i)
    if (!isfinite(tables[(size_t)o.table + i])) return "a table entry that is not finite";
  return nullptr;
}

// _imaging.c's _prepare_lut_table: the float32 product t (255 << 6), +-0x7fff at the ends, else rounded half away from zero
int16_t quantise(float t) {
  const float item = t * (float)(255 << PRECISION_BITS);
  if (item >= 0x7fff - 0.5) return 0x7fff;
  if (item <= -0x7fff + 0.5) return -0x7fff;
  return (int16_t)(item < 0 ? item - 0.5 : item + 0.5);
}

// appends the op's nodes, four int16 each
void add_nodes(const ta_color_op& o, const float* tables, std::vector<int16_t>& nodes) {
  const float* t = tables + o.table;
  for (size_t i = 0, n = lut_nodes(o); i < n; ++i) {
    for (int c = 0; c < 3; ++c) nodes.push_back(quantise(t[3 * i + c]));
    nodes.push_back(0);
  }
}

// a region's own defect: its op
auto op_in(int n_ops) {
  return [n_ops](const ta_color_region& q) { return q.op < 0 || q.op >= n_ops ? "op index out of range" : (const char*)nullptr; };
}

// the dynamic LDS a workgroup of this op needs
size_t lds_of(const color_dop& d) {
  if (d.kind == TA_COLOR_RGB2YCBCR || d.kind == TA_COLOR_YCBCR2RGB) return YCC_BYTES;
  return d.kind == TA_COLOR_LUT3D && d.in_lds ? (size_t)d.count * 8 : 0;
}

struct color_launch {
  int first, strips;
  size_t lds;
};

}  // namespace

extern "C" int ta_color_plan(const ta_color_region* regions, int n, const ta_color_op* ops, int n_ops, const float* tables, size_t n_tables,
                             int32_t* rounds, int16_t* nodes) {
  if (n < 0 || n_ops < 0 || (n > 0 && !regions) || (n_ops > 0 && !ops)) return TA_E_INVALID;
  for (int s = 0; s < n_ops; ++s)
    if (check_op(ops[s], tables, n_tables)) return TA_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (ta_region_defect(regions[i], op_in(n_ops))) return TA_E_INVALID;
  std::vector<int32_t> round;
  ta_plan_rounds(regions, n, round);
  for (int i = 0; i < n && rounds; ++i) rounds[i] = round[i];
  if (nodes) {
    std::vector<int16_t> v;
    for (int s = 0; s < n_ops; ++s)
      if (ops[s].kind == TA_COLOR_LUT3D) add_nodes(ops[s], tables, v);
    if (!v.empty()) memcpy(nodes, v.data(), v.size() * sizeof(int16_t));
  }
  return TA_OK;
}

extern "C" int ta_frames_color(ta_ctx* ctx, ta_frames* frames, const ta_color_region* regions, int n, const ta_color_op* ops, int n_ops,
                               const float* tables, size_t n_tables) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (n_ops < 0 || (n_ops > 0 && !ops)) return ta_fail(ctx, TA_E_INVALID, "frames_color: bad args");
  TA_TRY(ta_check_batch(ctx, "frames_color", frames, regions, n));
  for (int s = 0; s < n_ops; ++s)
    if (const char* why = check_op(ops[s], tables, n_tables)) return ta_fail(ctx, TA_E_INVALID, "frames_color: op %d: %s", s, why);
  TA_TRY(ta_check_boxes(ctx, "frames_color", frames, regions, n, MAX_SIDE, op_in(n_ops)));
  if (n == 0) return TA_OK;

  // the ops as the device reads them; the nodes of the 3-D tables that a region uses
  std::vector<char> used(n_ops, 0);
  for (int i = 0; i < n; ++i) used[regions[i].op] = 1;
  std::vector<color_dop> dops(n_ops);
  std::vector<int16_t> nodes;
  bool ycc = false;
  for (int s = 0; s < n_ops; ++s) {
    const ta_color_op& o = ops[s];
    color_dop& d = dops[s];
    memset(&d, 0, sizeof(d));
    d.kind = o.kind;
    if (!used[s]) continue;
    ycc |= o.kind == TA_COLOR_RGB2YCBCR || o.kind == TA_COLOR_YCBCR2RGB;
    if (o.kind == TA_COLOR_MATRIX) memcpy(d.m, tables + o.table, sizeof(d.m));
    if (o.kind == TA_COLOR_LUT3D) {
      d.s0 = o.size[0], d.s01 = o.size[0] * o.size[1], d.count = (int32_t)lut_nodes(o);
      for (int k = 0; k < 3; ++k) d.scale[k] = (int)((o.size[k] - 1) / 255.0 * (1 << SCALE_BITS));
      d.node0 = (uint32_t)(nodes.size() / 4);
      d.in_lds = (size_t)d.count * 8 <= LDS_TABLE_BYTES;
      add_nodes(o, tables, nodes);
    }
  }

  // round by round: records, strips and the LDS of the round's launch
  std::vector<color_rec> recs;
  std::vector<strip_item> items;
  std::vector<color_launch> launches;
  ta_span_tables spans;
  size_t closed = 0, lds = 0;
  ta_each_round(
      regions, n,
      [&](const ta_color_region& q) {
        color_rec r;
        memset(&r, 0, sizeof(r));
        r.frame = q.frame, r.x0 = q.x0, r.y0 = q.y0, r.w = q.x1 - q.x0, r.h = q.y1 - q.y0, r.op = q.op;
        r.tab = q.shape == TA_BLUR_ELLIPSE ? spans.of(r.w, r.h) : -1;
        recs.push_back(r);
        lds = std::max(lds, lds_of(dops[q.op]));
      },
      [&] {
        const int at = (int)items.size();
        launches.push_back({at, ta_add_strips(items, recs, closed, WALK_WAVES, STRIP_PIXELS), lds});
        closed = recs.size(), lds = 0;
      });

  ta_staging st;                                    // one H2D copy
  const size_t o_rec = st.put(recs), o_item = st.put(items), o_tab = st.put(spans.table()), o_op = st.put(dops);
  const size_t o_ycc = ycc ? st.put(ycbcr_tables()) : 0, o_node = st.put(nodes);
  TA_TRY(st.commit(ctx));
  for (const color_launch& L : launches)
    if (L.strips)
      hipLaunchKernelGGL(color_kernel, dim3(L.strips), dim3(THREADS), L.lds, ctx->stream, frames->dev, frames->h, frames->w,
                         st.dev<const color_rec>(o_rec), st.dev<const strip_item>(o_item) + L.first, st.dev<const int2>(o_tab),
                         st.dev<const color_dop>(o_op), st.dev<const uint2>(o_ycc), st.dev<const uint2>(o_node));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
