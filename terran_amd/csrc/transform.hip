// ta_frames_transform / ta_frames_transform_mesh / ta_frames_transpose: Pillow's `Image.transform(size, AFFINE | PERSPECTIVE |
// MESH, data, resample, fillcolor=)` and `Image.transpose(op)` on uint8 RGB, bit for bit, over a resident frame batch.
//
// Image.transform (libImaging/Geometry.c) maps every OUTPUT pixel centre to a source point in double,
//   xin = x + 0.5, yin = y + 0.5;  xs = a0 xin + a1 yin + a2, ys = a3 xin + a4 yin + a5;  perspective: both / (a6 xin + a7 yin + 1)
// and a pixel whose point fails 0 <= xs < W && 0 <= ys < H keeps the fill colour (zeros for fillcolor=None).  BILINEAR and
// BICUBIC subtract 0.5, floor, clip their 2 x 2 / 4 x 4 taps to the image and interpolate in double, rows first:
// bilinear a + (b - a) d truncated; bicubic p1 + d (p2 + d (p3 + d p4)) clamped to 0 .. 255, then truncated.
// NEAREST takes the route Pillow takes (rec::route):
//   SCALE    affine with a1 == a3 == 0 (ImagingScaleAffine): per axis, the coordinate starts at a2 + a0 / 2 and is advanced
//            by ADDING a0; the HOST accumulates it into one table of source indices per axis (-1: outside)
//   FIXED    other affine maps whose four output corners stay below 32768 (affine_fixed): 16.16 fixed point, int32
//   ACCUM    the remaining affine maps: the double coordinate accumulated by adding a0, a3 along a row and a1, a4 down the
//            rows.  Serial by nature and, in Pillow's words, of no reasonable use: one thread per output row
//   GENERIC  perspective: (int) of the double point
// Pillow converts out-of-range and non-finite doubles to int (undefined in C); here every point is range-tested in double
// first and a point that is not inside, NaN included, gives the fill colour: no address is ever formed from it.
// Compiled with -ffp-contract=off (build.py): a fused multiply-add rounds differently from Pillow's C.
//
// transform_kernel<filter>: one launch serves all regions.  A workgroup belongs to ONE region (its record is read through
// uniform loads); a lane owns 4 consecutive pixels of the region's output image in raster order, 12 bytes, and stores them
// as three dwords when the image starts on a dword (always when out_h * out_w is a multiple of 4, else for every fourth
// image), byte by byte otherwise and for the ragged tail at the image's end.  The source is gathered with byte loads.
// ta_frames_transform_mesh: Image.transform(size, MESH | QUAD, ...) (ImageOps.deform).  An output image is assembled from
// cells, each a box of the output with a bilinear map of its own (quad_transform: xs = a0 + a1 xin + a2 yin + a3 xin yin
// with xin, yin relative to the box's CLAMPED origin), applied in list order; they may overlap, leave gaps and reach
// outside.  No rounds: the host bins a mesh's cells into the 64 x 16 tiles of the output they touch (CSR, list order),
// once per call however many images share the mesh, and mesh_kernel -- one launch, one workgroup per tile and image, the
// same 4 pixels and packed store per lane -- lets every pixel pick the LAST cell that Pillow would have let write it.
// transpose_kernel: a 32 x 32 pixel tile goes through LDS (one dword per pixel, rows padded to 33) so that, for the four
// ops that swap the axes, consecutive lanes read consecutive source pixels AND write consecutive output pixels.
#include "frame_regions.h"

#include <math.h>

#include <tuple>

namespace {

constexpr int MAX_OUT = 16384;
constexpr int THREADS = 256;
constexpr int PIXELS_PER_LANE = 4;
constexpr int TILE = 32;                   // transpose: a tile's side; 256 threads = 32 columns x 8 rows, 4 rows each
enum { ROUTE_GENERIC = 0, ROUTE_SCALE = 1, ROUTE_FIXED = 2, ROUTE_ACCUM = 3 };

struct tf_rec {                // 112 bytes
  int32_t frame, route, perspective, pad;
  double a[8];
  int32_t f[6];                // FIXED: a0 .. a5 in 16.16, the half-pixel offsets folded into f[2], f[5]
  uint32_t xtab, ytab;         // SCALE: offsets of the two index tables
};
static_assert(sizeof(tf_rec) == 112, "tf_rec");

struct source {
  const uint8_t* img;
  int H, W;
  __device__ uint32_t at(int y, int x) const {
    const uint8_t* p = img + ((size_t)y * W + x) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
};

__device__ inline int clipi(int v, int hi) { return v < 0 ? 0 : (v < hi ? v : hi - 1); }

__device__ inline bool source_point(const tf_rec& q, int x, int y, const source& s, double* xs, double* ys) {
  const double xin = (double)x + 0.5, yin = (double)y + 0.5;
  double u = q.a[0] * xin + q.a[1] * yin + q.a[2];
  double v = q.a[3] * xin + q.a[4] * yin + q.a[5];
  if (q.perspective) {
    const double d = q.a[6] * xin + q.a[7] * yin + 1;
    u = u / d;
    v = v / d;
  }
  *xs = u, *ys = v;
  return u >= 0.0 && u < (double)s.W && v >= 0.0 && v < (double)s.H;        // false for NaN
}

__device__ inline double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// the filter's sample (packed R | G << 8 | B << 16) at a source point that passed the inside test
template <int FILTER>
__device__ inline uint32_t sample_at(const source& s, double xs, double ys) {
  if (FILTER == TA_RESAMPLE_NEAREST) return s.at((int)ys, (int)xs);
  xs -= 0.5, ys -= 0.5;
  const double fx = floor(xs), fy = floor(ys);
  const double dx = xs - fx, dy = ys - fy;
  const int ix = (int)fx, iy = (int)fy;                 // -1 .. W - 1, -1 .. H - 1
  uint32_t out = 0;
  if (FILTER == TA_RESAMPLE_BILINEAR) {
    const int x0 = clipi(ix, s.W), x1 = clipi(ix + 1, s.W);
    const uint32_t p00 = s.at(clipi(iy, s.H), x0), p01 = s.at(clipi(iy, s.H), x1);
    const uint32_t p10 = s.at(clipi(iy + 1, s.H), x0), p11 = s.at(clipi(iy + 1, s.H), x1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = (p00 >> (8 * c)) & 255, b = (p01 >> (8 * c)) & 255, e = (p10 >> (8 * c)) & 255, f = (p11 >> (8 * c)) & 255;
      const double v1 = a + (b - a) * dx, v2 = e + (f - e) * dx;
      out |= (uint32_t)(uint8_t)(v1 + (v2 - v1) * dy) << (8 * c);
    }
    return out;
  }
  int xc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) xc[k] = clipi(ix - 1 + k, s.W);
  double r[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yy = clipi(iy - 1 + j, s.H);
    const uint32_t p0 = s.at(yy, xc[0]), p1 = s.at(yy, xc[1]), p2 = s.at(yy, xc[2]), p3 = s.at(yy, xc[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      r[j][c] = cubic((double)((p0 >> (8 * c)) & 255), (double)((p1 >> (8 * c)) & 255), (double)((p2 >> (8 * c)) & 255),
                      (double)((p3 >> (8 * c)) & 255), dx);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = cubic(r[0][c], r[1][c], r[2][c], r[3][c], dy);
    out |= (uint32_t)(v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (uint8_t)v)) << (8 * c);
  }
  return out;
}

// the pixel (packed R | G << 8 | B << 16) of output position (x, y)
template <int FILTER>
__device__ inline uint32_t sample(const tf_rec& q, const int32_t* __restrict__ tab, const source& s, int x, int y, uint32_t fill) {
  if (FILTER == TA_RESAMPLE_NEAREST) {
    if (q.route == ROUTE_SCALE) {
      const int sx = tab[q.xtab + x], sy = tab[q.ytab + y];
      return sx >= 0 && sy >= 0 ? s.at(sy, sx) : fill;
    }
    if (q.route == ROUTE_FIXED) {                       // int32 arithmetic that wraps as Pillow's repeated additions do
      const int sx = (int32_t)((uint32_t)q.f[2] + (uint32_t)y * (uint32_t)q.f[1] + (uint32_t)x * (uint32_t)q.f[0]) >> 16;
      const int sy = (int32_t)((uint32_t)q.f[5] + (uint32_t)y * (uint32_t)q.f[4] + (uint32_t)x * (uint32_t)q.f[3]) >> 16;
      return sx >= 0 && sx < s.W && sy >= 0 && sy < s.H ? s.at(sy, sx) : fill;
    }
  }
  double xs, ys;
  return source_point(q, x, y, s, &xs, &ys) ? sample_at<FILTER>(s, xs, ys) : fill;
}

// a lane's `count` <= 4 consecutive pixels to d: three dwords when all four are there and d is on a dword, bytes otherwise
__device__ inline void store_pixels(uint8_t* d, const uint32_t* px, int count, bool on_dword) {
  if (count == PIXELS_PER_LANE && on_dword) {
    uint32_t* d4 = (uint32_t*)d;
    d4[0] = px[0] | (px[1] << 24);
    d4[1] = (px[1] >> 8) | (px[2] << 16);
    d4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    for (int j = 0; j < count; ++j) d[3 * j] = (uint8_t)px[j], d[3 * j + 1] = (uint8_t)(px[j] >> 8), d[3 * j + 2] = (uint8_t)(px[j] >> 16);
  }
}

// grid.x = regions x groups; region r's image is out + r * oh * ow * 3
template <int FILTER>
__global__ __launch_bounds__(THREADS) void transform_kernel(const uint8_t* __restrict__ frames, int H, int W, const tf_rec* __restrict__ recs,
                                                            const int32_t* __restrict__ tab, uint8_t* __restrict__ out, int oh, int ow,
                                                            int groups, uint32_t fill) {
  const int r = blockIdx.x / groups;
  const tf_rec& q = recs[r];                            // the same for the whole workgroup
  if (FILTER == TA_RESAMPLE_NEAREST && q.route == ROUTE_ACCUM) return;       // transform_accum_rows writes this image
  const int npix = oh * ow;                             // <= 2^28
  const int p0 = ((blockIdx.x - r * groups) * THREADS + threadIdx.x) * PIXELS_PER_LANE;
  if (p0 >= npix) return;
  const source s = {frames + (size_t)q.frame * H * W * 3, H, W};
  int y = p0 / ow, x = p0 - y * ow;
  const int count = min(PIXELS_PER_LANE, npix - p0);
  uint32_t px[PIXELS_PER_LANE] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < PIXELS_PER_LANE; ++j) {
    if (j < count) {
      px[j] = sample<FILTER>(q, tab, s, x, y, fill);
      if (++x == ow) x = 0, ++y;
    }
  }
  const size_t image = (size_t)r * npix * 3;
  store_pixels(out + image + (size_t)p0 * 3, px, count, (image & 3) == 0);      // p0 * 3 is a multiple of 12
}

// ---- mesh ------------------------------------------------------------------------------------------------------------
// A cell as the device reads it: the box clamped to the output (empty: the cell is in no tile's list) and a0 .. a7.
struct mesh_rec {              // 80 bytes
  int32_t x0, y0, x1, y1;
  double a[8];
};
static_assert(sizeof(mesh_rec) == 80, "mesh_rec");
constexpr int MESH_TW = TA_MESH_TILE_W, MESH_TH = TA_MESH_TILE_H, MESH_LANES_X = MESH_TW / PIXELS_PER_LANE;
static_assert(MESH_TW * MESH_TH == THREADS * PIXELS_PER_LANE && MESH_TW % PIXELS_PER_LANE == 0, "one lane per 4 pixels of a tile");

// grid.x = images x tiles.  A workgroup owns one tile of one image; its cell list first[mesh * tiles + tile] .. is the same
// for all its lanes, so the list and the records come through uniform loads.  A lane owns 4 consecutive pixels of a row and
// walks the list from the LAST cell to the first: a pixel is settled by the first cell whose clamped box holds it and --
// under a fill colour (keep), where Pillow leaves a pixel whose point is outside as it is -- whose point is inside the
// source.  What no cell settles, and what a cell settles with a point outside, is the fill.  Every pixel is written once.
template <int FILTER>
__global__ __launch_bounds__(THREADS) void mesh_kernel(const uint8_t* __restrict__ frames, int H, int W, const mesh_rec* __restrict__ recs,
                                                       const int32_t* __restrict__ first, const int32_t* __restrict__ list,
                                                       const ta_mesh_image* __restrict__ images, uint8_t* __restrict__ out, int oh, int ow,
                                                       int tiles_x, int tiles, uint32_t fill, int keep) {
  const int i = blockIdx.x / tiles, t = blockIdx.x - i * tiles;
  const ta_mesh_image im = images[i];
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y = ty * MESH_TH + threadIdx.x / MESH_LANES_X, x = tx * MESH_TW + (threadIdx.x % MESH_LANES_X) * PIXELS_PER_LANE;
  if (y >= oh || x >= ow) return;
  const int count = min(PIXELS_PER_LANE, ow - x);
  const size_t at = (size_t)im.mesh * tiles + t;
  const int begin = first[at], end = first[at + 1];
  const source s = {frames + (size_t)im.frame * H * W * 3, H, W};
  double xs[PIXELS_PER_LANE], ys[PIXELS_PER_LANE];
  unsigned pending = (1u << count) - 1, inside = 0;
  for (int e = end - 1; e >= begin && pending; --e) {
    const mesh_rec& c = recs[list[e]];
    if (y < c.y0 || y >= c.y1) continue;
    const double yin = (double)(y - c.y0) + 0.5;
#pragma unroll
    for (int j = 0; j < PIXELS_PER_LANE; ++j) {
      if (!((pending >> j) & 1) || x + j < c.x0 || x + j >= c.x1) continue;
      const double xin = (double)(x + j - c.x0) + 0.5;
      const double u = c.a[0] + c.a[1] * xin + c.a[2] * yin + c.a[3] * xin * yin;
      const double v = c.a[4] + c.a[5] * xin + c.a[6] * yin + c.a[7] * xin * yin;
      const bool in = u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H;      // false for NaN
      if (in) xs[j] = u, ys[j] = v, inside |= 1u << j;
      if (in || !keep) pending &= ~(1u << j);
    }
  }
  uint32_t px[PIXELS_PER_LANE];
#pragma unroll
  for (int j = 0; j < PIXELS_PER_LANE; ++j) px[j] = (inside >> j) & 1 ? sample_at<FILTER>(s, xs[j], ys[j]) : fill;
  uint8_t* d = out + ((size_t)i * oh * ow + (size_t)y * ow + x) * 3;
  store_pixels(d, px, count, ((size_t)d & 3) == 0);
}

// NEAREST, ROUTE_ACCUM: one thread per output row of such a region
__global__ __launch_bounds__(THREADS) void transform_accum_rows(const uint8_t* __restrict__ frames, int H, int W, const tf_rec* __restrict__ recs,
                                                                int n, uint8_t* __restrict__ out, int oh, int ow, uint32_t fill) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= (int64_t)n * oh) return;
  const int r = (int)(t / oh), y = (int)(t - (int64_t)r * oh);
  const tf_rec& q = recs[r];
  if (q.route != ROUTE_ACCUM) return;
  const source s = {frames + (size_t)q.frame * H * W * 3, H, W};
  double xx = q.a[2] + q.a[1] * 0.5 + q.a[0] * 0.5, yy = q.a[5] + q.a[4] * 0.5 + q.a[3] * 0.5;
  for (int i = 0; i < y; ++i) xx += q.a[1], yy += q.a[4];
  uint8_t* d = out + ((size_t)r * oh + y) * (size_t)ow * 3;
  for (int x = 0; x < ow; ++x, d += 3) {
    const bool inside = xx >= 0.0 && xx < (double)W && yy >= 0.0 && yy < (double)H;
    const uint32_t p = inside ? s.at((int)yy, (int)xx) : fill;
    d[0] = (uint8_t)p, d[1] = (uint8_t)(p >> 8), d[2] = (uint8_t)(p >> 16);
    xx += q.a[0], yy += q.a[3];
  }
}

// out[i][j] = in[sy][sx] with (sy, sx) = swap ? (j, i) : (i, j), then sy = H - 1 - sy under flip_y, sx = W - 1 - sx under flip_x.
// grid.x = images x tiles_x, grid.y = tiles_y over the OUTPUT (oh x ow).
__global__ __launch_bounds__(THREADS) void transpose_kernel(const uint8_t* __restrict__ in, int H, int W, uint8_t* __restrict__ out, int oh, int ow,
                                                            int tiles_x, int swap, int flip_x, int flip_y) {
  __shared__ uint32_t tile[TILE][TILE + 1];
  const int img = blockIdx.x / tiles_x;
  const int i0 = blockIdx.y * TILE, j0 = (blockIdx.x - img * tiles_x) * TILE;
  const int c = threadIdx.x % TILE, r0 = threadIdx.x / TILE;
  const uint8_t* src = in + (size_t)img * H * W * 3;
  for (int r = r0; r < TILE; r += THREADS / TILE) {
    const int i = swap ? i0 + c : i0 + r, j = swap ? j0 + r : j0 + c;       // lanes walk the source's x
    if (i < oh && j < ow) {
      int sy = swap ? j : i, sx = swap ? i : j;
      if (flip_y) sy = H - 1 - sy;
      if (flip_x) sx = W - 1 - sx;
      const uint8_t* p = src + ((size_t)sy * W + sx) * 3;
      tile[r][c] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
  }
  __syncthreads();
  uint8_t* dst = out + (size_t)img * oh * ow * 3;
  for (int r = r0; r < TILE; r += THREADS / TILE) {
    const int i = i0 + r, j = j0 + c;                   // lanes walk the output's x
    if (i < oh && j < ow) {
      const uint32_t p = swap ? tile[c][r] : tile[r][c];
      uint8_t* d = dst + ((size_t)i * ow + j) * 3;
      d[0] = (uint8_t)p, d[1] = (uint8_t)(p >> 8), d[2] = (uint8_t)(p >> 16);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// Geometry.c: #define FLOOR(v) ((v) < 0.0 ? ((int)floor(v)) : ((int)(v))), FIX(v) FLOOR((v) * 65536.0 + 0.5)
int32_t fix16(double v) {
  v = v * 65536.0 + 0.5;
  return v < 0.0 ? (int32_t)floor(v) : (int32_t)v;
}
bool check_fixed(const double* a, int x, int y) {
  return fabs(x * a[0] + y * a[1] + a[2]) < 32768.0 && fabs(x * a[3] + y * a[4] + a[5]) < 32768.0;
}

// ImagingScaleAffine's source index per output sample along one axis, appended to `tab`; equal axes share one table
struct scale_tabs {
  std::vector<int32_t> tab;
  std::map<std::tuple<double, double, int, int>, uint32_t> seen;
  uint32_t axis(double start, double step, int out_size, int in_size) {
    const auto key = std::make_tuple(start, step, out_size, in_size);
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    const uint32_t at = (uint32_t)tab.size();
    double v = start;
    for (int i = 0; i < out_size; ++i) {
      tab.push_back(v >= 0.0 && v < (double)in_size ? (int32_t)v : -1);
      v += step;
    }
    seen.emplace(key, at);
    return at;
  }
};

// ---- mesh: the host plan -------------------------------------------------------------------------------------------------
constexpr int MESH_COORD_LIMIT = 1 << 24;

const char* mesh_cell_defect(const ta_mesh_cell& c) {
  if (c.x1 <= c.x0 || c.y1 <= c.y0) return "empty or inverted box";
  for (int32_t v : {c.x0, c.y0, c.x1, c.y1})
    if (v < -MESH_COORD_LIMIT || v > MESH_COORD_LIMIT) return "a box coordinate beyond +-2^24";
  for (double v : c.quad)
    if (!isfinite(v)) return "a corner that is not finite";
  return nullptr;
}

// What is wrong with a call's cells and output size whatever its frames, or nullptr; *cell: the cell it is about, or -1.
const char* mesh_defect(const ta_mesh_cell* cells, int n_cells, int out_h, int out_w, int* cell) {
  *cell = -1;
  if (n_cells < 0 || (n_cells > 0 && !cells)) return "bad args";
  if (out_h <= 0 || out_w <= 0 || out_h > MAX_OUT || out_w > MAX_OUT) return "output sides must be 1 .. 16384";
  if (n_cells > TA_MESH_MAX_CELLS) return "more than TA_MESH_MAX_CELLS cells";
  for (int i = 0; i < n_cells; ++i)
    if (const char* why = mesh_cell_defect(cells[i])) {
      *cell = i;
      return why;
    }
  return nullptr;
}

// Pillow's QUAD coefficients (Image.__transformer) and the box clamped as ImagingGenericTransform clamps it
mesh_rec mesh_record(const ta_mesh_cell& c, int out_h, int out_w) {
  mesh_rec r;
  const double* q = c.quad;                           // nw 0, 1; sw 2, 3; se 4, 5; ne 6, 7
  const double As = 1.0 / (c.x1 - c.x0), At = 1.0 / (c.y1 - c.y0);
  r.a[0] = q[0], r.a[1] = (q[6] - q[0]) * As, r.a[2] = (q[2] - q[0]) * At, r.a[3] = (q[4] - q[2] - q[6] + q[0]) * As * At;
  r.a[4] = q[1], r.a[5] = (q[7] - q[1]) * As, r.a[6] = (q[3] - q[1]) * At, r.a[7] = (q[5] - q[3] - q[7] + q[1]) * As * At;
  r.x0 = std::max(c.x0, 0), r.y0 = std::max(c.y0, 0), r.x1 = std::min(c.x1, out_w), r.y1 = std::min(c.y1, out_h);
  return r;
}

// The meshes of a call over one output size: a record per cell and, in CSR form, the cells of every (mesh, tile) in list
// order.  first[m * tiles + t] .. first[m * tiles + t + 1] - 1 index `list`, whose entries index `recs`.
struct mesh_plan {
  int tiles_x = 0, tiles = 0;
  std::vector<mesh_rec> recs;
  std::vector<int32_t> first, list;

  // false: more than TA_MESH_MAX_ENTRIES (cell, tile) pairs or first indices.  The cells are valid (mesh_defect).
  bool build(const ta_mesh_cell* cells, const int32_t* mesh_first, int n_meshes, int out_h, int out_w) {
    tiles_x = (out_w + MESH_TW - 1) / MESH_TW;
    tiles = tiles_x * ((out_h + MESH_TH - 1) / MESH_TH);
    const int n_cells = n_meshes ? mesh_first[n_meshes] : 0;
    if ((int64_t)n_meshes * tiles + 1 > TA_MESH_MAX_ENTRIES) return false;
    recs.resize(n_cells);
    int64_t entries = 0;
    for (int i = 0; i < n_cells; ++i) {
      const mesh_rec& r = recs[i] = mesh_record(cells[i], out_h, out_w);
      if (r.x1 > r.x0 && r.y1 > r.y0) entries += (int64_t)span(r.x0, r.x1, MESH_TW) * span(r.y0, r.y1, MESH_TH);
    }
    if (entries > TA_MESH_MAX_ENTRIES) return false;
    first.assign((size_t)n_meshes * tiles + 1, 0);
    list.resize((size_t)entries);
    for (int pass = 0; pass < 2; ++pass) {              // count into first[.. + 1], sum, then fill in list order
      for (int m = 0; m < n_meshes; ++m) {
        int32_t* f = first.data() + (size_t)m * tiles;
        for (int i = mesh_first[m]; i < mesh_first[m + 1]; ++i) {
          const mesh_rec& r = recs[i];
          if (r.x1 <= r.x0 || r.y1 <= r.y0) continue;
          for (int ty = r.y0 / MESH_TH; ty <= (r.y1 - 1) / MESH_TH; ++ty)
            for (int tx = r.x0 / MESH_TW; tx <= (r.x1 - 1) / MESH_TW; ++tx) {
              if (pass == 0) ++f[ty * tiles_x + tx + 1];
              else list[(size_t)f[ty * tiles_x + tx]++] = i;
            }
        }
      }
      if (pass == 0) {
        for (size_t k = 1; k < first.size(); ++k) first[k] += first[k - 1];
      } else {                                          // every first[k] now holds its tile's end: shift back
        for (size_t k = first.size() - 1; k > 0; --k) first[k] = first[k - 1];
        first[0] = 0;
      }
    }
    return true;
  }

 private:
  static int span(int lo, int hi, int tile) { return (hi - 1) / tile - lo / tile + 1; }
};

}  // namespace

extern "C" int ta_frames_transform(ta_ctx* ctx, const ta_frames* src, const ta_transform_region* regions, int n, int out_h, int out_w,
                                   int filter, const uint8_t* fill_rgb, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (out) *out = nullptr;
  if (!out) return ta_fail(ctx, TA_E_INVALID, "frames_transform: bad args");
  TA_TRY(ta_check_batch(ctx, "frames_transform", src, regions, n));
  if (filter != TA_RESAMPLE_NEAREST && filter != TA_RESAMPLE_BILINEAR && filter != TA_RESAMPLE_BICUBIC)
    return ta_fail(ctx, TA_E_INVALID, "frames_transform: filter %d, must be NEAREST, BILINEAR or BICUBIC", filter);
  if (out_h <= 0 || out_w <= 0 || out_h > MAX_OUT || out_w > MAX_OUT)
    return ta_fail(ctx, TA_E_INVALID, "frames_transform: output %d x %d, sides must be 1 .. %d", out_w, out_h, MAX_OUT);
  const int N = src->n, H = src->h, W = src->w;
  for (int i = 0; i < n; ++i) {
    const ta_transform_region& q = regions[i];
    TA_TRY(ta_check_frame(ctx, "frames_transform", i, q.frame, N));
    if (q.method != TA_TRANSFORM_AFFINE && q.method != TA_TRANSFORM_PERSPECTIVE)
      return ta_fail(ctx, TA_E_INVALID, "frames_transform: region %d: unknown method %d", i, q.method);
    for (int k = 0; k < (q.method == TA_TRANSFORM_AFFINE ? 6 : 8); ++k)
      if (!isfinite(q.a[k])) return ta_fail(ctx, TA_E_INVALID, "frames_transform: region %d: coefficient %d is not finite", i, k);
  }
  if (n == 0) return TA_OK;
  const int npix = out_h * out_w;
  const int groups = (npix + THREADS * PIXELS_PER_LANE - 1) / (THREADS * PIXELS_PER_LANE);
  if ((int64_t)n * groups > 0x7fffffffLL || (int64_t)n * out_h > 0x7fffffffLL * THREADS)
    return ta_fail(ctx, TA_E_INVALID, "frames_transform: %d regions of %d x %d are more than one launch holds", n, out_w, out_h);

  std::vector<tf_rec> recs(n);
  scale_tabs st_tabs;
  bool accum = false;
  for (int i = 0; i < n; ++i) {
    const ta_transform_region& q = regions[i];
    tf_rec& r = recs[i];
    memset(&r, 0, sizeof(r));
    r.frame = q.frame;
    r.perspective = q.method == TA_TRANSFORM_PERSPECTIVE;
    memcpy(r.a, q.a, sizeof(double) * (r.perspective ? 8 : 6));
    const double* a = r.a;
    if (filter != TA_RESAMPLE_NEAREST || r.perspective) {
      r.route = ROUTE_GENERIC;
    } else if (a[1] == 0 && a[3] == 0) {
      r.route = ROUTE_SCALE;
      r.xtab = st_tabs.axis(a[2] + a[0] * 0.5, a[0], out_w, W);
      r.ytab = st_tabs.axis(a[5] + a[4] * 0.5, a[4], out_h, H);
    } else if (check_fixed(a, 0, 0) && check_fixed(a, out_w, out_h) && check_fixed(a, 0, out_h) && check_fixed(a, out_w, 0)) {
      r.route = ROUTE_FIXED;
      r.f[0] = fix16(a[0]), r.f[1] = fix16(a[1]), r.f[3] = fix16(a[3]), r.f[4] = fix16(a[4]);
      r.f[2] = fix16(a[2] + a[0] * 0.5 + a[1] * 0.5), r.f[5] = fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
    } else {
      r.route = ROUTE_ACCUM;
      accum = true;
    }
  }
  const uint32_t fill = fill_rgb ? (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16) : 0u;

  ta_frames* dst = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, n, out_h, out_w, &dst));
  ta_staging st;                                    // one H2D copy: records, then the scale tables
  st.slack = 16;                                    // kept: not shown from the kernels that nothing reads past the tables
  const size_t o_rec = st.put(recs), o_tab = st.put(st_tabs.tab);
  int rc = st.commit(ctx);                          // a code, no return: dst is freed below on every failure
  if (rc == TA_OK) {
    const tf_rec* drec = st.dev<const tf_rec>(o_rec);
    const int32_t* dtab = st.dev<const int32_t>(o_tab);
    const dim3 grid((unsigned)(n * groups)), block(THREADS);
    const uint8_t* in = src->dev;
    if (filter == TA_RESAMPLE_NEAREST)
      hipLaunchKernelGGL(transform_kernel<TA_RESAMPLE_NEAREST>, grid, block, 0, ctx->stream, in, H, W, drec, dtab, dst->dev, out_h, out_w, groups, fill);
    else if (filter == TA_RESAMPLE_BILINEAR)
      hipLaunchKernelGGL(transform_kernel<TA_RESAMPLE_BILINEAR>, grid, block, 0, ctx->stream, in, H, W, drec, dtab, dst->dev, out_h, out_w, groups, fill);
    else
      hipLaunchKernelGGL(transform_kernel<TA_RESAMPLE_BICUBIC>, grid, block, 0, ctx->stream, in, H, W, drec, dtab, dst->dev, out_h, out_w, groups, fill);
    if (accum)
      hipLaunchKernelGGL(transform_accum_rows, dim3((unsigned)(((int64_t)n * out_h + THREADS - 1) / THREADS)), block, 0, ctx->stream, in, H, W, drec,
                         n, dst->dev, out_h, out_w, fill);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);             // pinned / scratch staging is reused by the next call
    if (e != hipSuccess) rc = ta_fail(ctx, TA_E_DEVICE, "frames_transform: %s", hipGetErrorString(e));
  }
  if (rc != TA_OK) {
    ta_frames_free(dst);
    return rc;
  }
  *out = dst;
  return TA_OK;
}

extern "C" int ta_frames_transform_mesh(ta_ctx* ctx, const ta_frames* src, const ta_mesh_cell* cells, int n_cells, const int32_t* mesh_first,
                                        int n_meshes, const ta_mesh_image* images, int n_images, int out_h, int out_w, int filter,
                                        const uint8_t* fill_rgb, ta_frames** out) {
  const char* who = "frames_transform_mesh";
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (out) *out = nullptr;
  if (!out) return ta_fail(ctx, TA_E_INVALID, "%s: bad args", who);
  TA_TRY(ta_check_batch(ctx, who, src, images, n_images));
  if (filter != TA_RESAMPLE_NEAREST && filter != TA_RESAMPLE_BILINEAR && filter != TA_RESAMPLE_BICUBIC)
    return ta_fail(ctx, TA_E_INVALID, "%s: filter %d, must be NEAREST, BILINEAR or BICUBIC", who, filter);
  if (n_meshes < 0 || (n_meshes > 0 && !mesh_first)) return ta_fail(ctx, TA_E_INVALID, "%s: bad args", who);
  int cell;
  if (const char* why = mesh_defect(cells, n_cells, out_h, out_w, &cell))
    return cell < 0 ? ta_fail(ctx, TA_E_INVALID, "%s: %s (%d cells, output %d x %d)", who, why, n_cells, out_w, out_h)
                    : ta_fail(ctx, TA_E_INVALID, "%s: cell %d: %s", who, cell, why);
  for (int m = 0; m < n_meshes; ++m)
    if (mesh_first[m] < 0 || mesh_first[m + 1] < mesh_first[m] || mesh_first[m + 1] > n_cells)
      return ta_fail(ctx, TA_E_INVALID, "%s: mesh %d: cells %d .. %d, the offsets must ascend within 0 .. %d", who, m, mesh_first[m],
                     mesh_first[m + 1], n_cells);
  const int N = src->n, H = src->h, W = src->w;
  for (int i = 0; i < n_images; ++i) {
    TA_TRY(ta_check_frame(ctx, who, i, images[i].frame, N));
    if (images[i].mesh < 0 || images[i].mesh >= n_meshes)
      return ta_fail(ctx, TA_E_INVALID, "%s: image %d: mesh %d out of range [0, %d)", who, i, images[i].mesh, n_meshes);
  }
  mesh_plan plan;
  if (!plan.build(cells, mesh_first, n_meshes, out_h, out_w))
    return ta_fail(ctx, TA_E_INVALID, "%s: more than %d tile entries", who, TA_MESH_MAX_ENTRIES);
  if (n_images == 0) return TA_OK;
  if ((int64_t)n_images * plan.tiles > 0x7fffffffLL)
    return ta_fail(ctx, TA_E_INVALID, "%s: %d images of %d x %d are more than one launch holds", who, n_images, out_w, out_h);
  const uint32_t fill = fill_rgb ? (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16) : 0u;

  ta_frames* dst = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, n_images, out_h, out_w, &dst));
  ta_staging st;                                    // one H2D copy: cell records, the tile lists, the image records
  const size_t o_rec = st.put(plan.recs), o_first = st.put(plan.first), o_list = st.put(plan.list);
  const size_t o_img = st.put(images, (size_t)n_images * sizeof(ta_mesh_image));
  int rc = st.commit(ctx);                          // a code, no return: dst is freed below on every failure
  if (rc == TA_OK) {
    const mesh_rec* drec = st.dev<const mesh_rec>(o_rec);
    const int32_t *dfirst = st.dev<const int32_t>(o_first), *dlist = st.dev<const int32_t>(o_list);
    const ta_mesh_image* dimg = st.dev<const ta_mesh_image>(o_img);
    const dim3 grid((unsigned)(n_images * plan.tiles)), block(THREADS);
    const uint8_t* in = src->dev;
    const int keep = fill_rgb != nullptr;
    if (filter == TA_RESAMPLE_NEAREST)
      hipLaunchKernelGGL(mesh_kernel<TA_RESAMPLE_NEAREST>, grid, block, 0, ctx->stream, in, H, W, drec, dfirst, dlist, dimg, dst->dev, out_h, out_w,
                         plan.tiles_x, plan.tiles, fill, keep);
    else if (filter == TA_RESAMPLE_BILINEAR)
      hipLaunchKernelGGL(mesh_kernel<TA_RESAMPLE_BILINEAR>, grid, block, 0, ctx->stream, in, H, W, drec, dfirst, dlist, dimg, dst->dev, out_h, out_w,
                         plan.tiles_x, plan.tiles, fill, keep);
    else
      hipLaunchKernelGGL(mesh_kernel<TA_RESAMPLE_BICUBIC>, grid, block, 0, ctx->stream, in, H, W, drec, dfirst, dlist, dimg, dst->dev, out_h, out_w,
                         plan.tiles_x, plan.tiles, fill, keep);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);             // pinned / scratch staging is reused by the next call
    if (e != hipSuccess) rc = ta_fail(ctx, TA_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
  }
  if (rc != TA_OK) {
    ta_frames_free(dst);
    return rc;
  }
  *out = dst;
  return TA_OK;
}

extern "C" int ta_mesh_plan(const ta_mesh_cell* cells, int n_cells, int out_h, int out_w, double* coefs, int32_t* boxes, int32_t* tile_first,
                            int32_t* tile_cells, int capacity, int* n_entries) {
  int cell;
  if (!n_entries || mesh_defect(cells, n_cells, out_h, out_w, &cell)) return TA_E_INVALID;
  const int32_t mesh_first[2] = {0, n_cells};
  mesh_plan plan;
  if (!plan.build(cells, mesh_first, 1, out_h, out_w)) return TA_E_INVALID;
  *n_entries = (int)plan.list.size();
  if (*n_entries > capacity) return TA_E_CAPACITY;
  for (int i = 0; i < n_cells; ++i) {
    const mesh_rec& r = plan.recs[i];
    if (coefs) memcpy(coefs + 8 * (size_t)i, r.a, sizeof(r.a));
    if (boxes) boxes[4 * i] = r.x0, boxes[4 * i + 1] = r.y0, boxes[4 * i + 2] = r.x1, boxes[4 * i + 3] = r.y1;
  }
  if (tile_first) memcpy(tile_first, plan.first.data(), plan.first.size() * sizeof(int32_t));
  if (tile_cells && *n_entries) memcpy(tile_cells, plan.list.data(), plan.list.size() * sizeof(int32_t));
  return TA_OK;
}

extern "C" int ta_frames_transpose(ta_ctx* ctx, const ta_frames* src, int op, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (out) *out = nullptr;
  if (!src || !out) return ta_fail(ctx, TA_E_INVALID, "frames_transpose: bad args");
  if (src->ctx->device != ctx->device) return ta_fail(ctx, TA_E_INVALID, "frames_transpose: the batch lives on another device");
  if (op < TA_FLIP_LEFT_RIGHT || op > TA_TRANSVERSE) return ta_fail(ctx, TA_E_INVALID, "frames_transpose: unknown op %d", op);
  const int N = src->n, H = src->h, W = src->w;
  const bool swap = op == TA_ROTATE_90 || op == TA_ROTATE_270 || op == TA_TRANSPOSE || op == TA_TRANSVERSE;
  const bool flip_x = op == TA_FLIP_LEFT_RIGHT || op == TA_ROTATE_90 || op == TA_ROTATE_180 || op == TA_TRANSVERSE;
  const bool flip_y = op == TA_FLIP_TOP_BOTTOM || op == TA_ROTATE_180 || op == TA_ROTATE_270 || op == TA_TRANSVERSE;
  const int oh = swap ? W : H, ow = swap ? H : W;
  ta_frames* dst = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, N, oh, ow, &dst));
  if (N > 0 && H > 0 && W > 0) {
    const int tiles_x = (ow + TILE - 1) / TILE, tiles_y = (oh + TILE - 1) / TILE;
    int rc = TA_OK;
    if ((int64_t)N * tiles_x > 0x7fffffffLL || tiles_y > 65535) {
      rc = ta_fail(ctx, TA_E_INVALID, "frames_transpose: %d images of %d x %d are more than one launch holds", N, W, H);
    } else {
      hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(N * tiles_x), tiles_y), dim3(THREADS), 0, ctx->stream, (const uint8_t*)src->dev, H, W,
                         dst->dev, oh, ow, tiles_x, (int)swap, (int)flip_x, (int)flip_y);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = ta_fail(ctx, TA_E_DEVICE, "frames_transpose: %s", hipGetErrorString(e));
    }
    if (rc != TA_OK) {
      ta_frames_free(dst);
      return rc;
    }
  }
  *out = dst;
  return TA_OK;
}
