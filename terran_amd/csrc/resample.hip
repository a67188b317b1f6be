// ta_frames_resample / ta_frames_pixelate: Pillow's `Image.resize(size, filter, box=)` on uint8 RGB, bit for bit, over many
// regions of a resident frame batch in one set of launches.
//
// Pillow's ImagingResample is two passes of fixed-point convolution, horizontal first, the horizontal result rounded to
// uint8.  Per axis and output sample i it derives, in double (libImaging/Resample.c precompute_coeffs; the box arrives
// as float32, and b1 - b0 is a float32 subtraction):
//   scale = (b1 - b0) / out, filterscale = max(scale, 1), support = filter_support * filterscale,
//   ksize = (int)ceil(support) * 2 + 1, center = b0 + (i + 0.5) * scale,
//   first = max(0, (int)(center - support + 0.5)), count = min(in, (int)(center + support + 0.5)) - first,
//   w[t] = filter((t + first - center + 0.5) * (1 / filterscale)), normalised to sum 1, then (int)(w * 2^22 +- 0.5)
// and a pixel is clip8((2^21 + sum src * coef) >> 22).  NEAREST is not a convolution there but the affine scaler
// (Geometry.c): source index (int) of a double coordinate that starts at b0 + 0.5 * step and is advanced by ADDING
// step = (b1 - b0) / out.  Here it is the same two passes with one tap of weight 2^22 per output sample.
// The HOST builds the tables (plan_axis; compiled with -ffp-contract=off, build.py); the device sees integers only.
//
// Device side: resample_rows (horizontal) writes, for every region, the source rows its vertical table references into
// the context's scratch; resample_cols (vertical) reads them and writes the result.  A thread owns one output pixel (its
// three bytes), consecutive lanes consecutive pixels of a row: a wave stores 192 contiguous bytes.  A workgroup is a tile
// 64 pixels wide; the coefficient rows it needs (those of its 64 columns, or of its 4 rows) are staged in LDS when they
// fit in 32 KiB (transposed for the horizontal pass: lane-consecutive dwords, no bank conflict), else read from global
// memory, so the tap count has no limit.  A pass Pillow skips (same size, box over the whole axis) is skipped: the other
// pass then reads the frame or writes the result directly; when both are skipped the horizontal pass copies.
// ta_frames_pixelate runs the same two kernels (BOX filter, the box as the cropped image) into small images in scratch
// and pixelate_paste writes them back enlarged by NEAREST under the region's shape.
#include "frame_regions.h"

#include <math.h>
#include <stdio.h>

#include <tuple>

namespace {

constexpr int MAX_OUT = 16384;             // an output side, a pixelate region's side, a block
constexpr int TX = 64, TY = 4;             // a workgroup's threads: 64 pixels of a row x 4 rows
constexpr int THREADS = TX * TY;
constexpr int ROWS_PER_GROUP = 16;         // rows a horizontal workgroup walks: its staged coefficients serve all of them
constexpr int LDS_INTS = 8192;             // 32 KiB of coefficients per workgroup
constexpr int PRECISION_BITS = 22;
constexpr int SKIP_ROWS = 1, SKIP_COLS = 2;   // rs_rec::flags: the horizontal / the vertical pass is skipped

struct rs_rec {                // 96 bytes
  int32_t frame;
  int32_t sx0, sy0;            // origin of the image the tables index, in the frame (pixelate: the box's corner)
  int32_t ry0, rows;           // the rows of that image the horizontal pass produces: ry0 .. ry0 + rows - 1
  int32_t ow, oh;              // size of the result
  int32_t kx, ky;              // taps per coefficient row
  int32_t flags;
  uint32_t xb, xc, yb, yc;     // bounds (first, count per sample) and coefficients of both axes, int32 offsets in the tables
  int32_t w, h;                // pixelate: the box's size,
  uint32_t xu, yu;             //           the NEAREST tables (bounds only) that enlarge the small image to it,
  int32_t span, pad;           //           the first row of its ellipse span table or -1
  uint64_t mid, out;           // byte offsets: the horizontal result in the scratch, the result in the output
};
static_assert(sizeof(rs_rec) == 96, "rs_rec");

__device__ inline uint8_t clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(THREADS) void resample_rows(const uint8_t* __restrict__ frames, int H, int W,
                                                         const rs_rec* __restrict__ recs, const int32_t* __restrict__ tab,
                                                         uint8_t* __restrict__ mid, uint8_t* __restrict__ out, int tiles_x) {
  __shared__ int32_t lc[LDS_INTS];
  const rs_rec q = recs[blockIdx.x / tiles_x];
  const int x0 = (blockIdx.x % tiles_x) * TX, y0 = blockIdx.y * ROWS_PER_GROUP;
  if ((q.flags & SKIP_ROWS) || x0 >= q.ow || y0 >= q.rows) return;          // the same for the whole workgroup
  const int k = q.kx, nx = min(TX, q.ow - x0);
  const bool in_lds = TX * k <= LDS_INTS;
  const int32_t* coef = tab + q.xc + (size_t)x0 * k;
  if (in_lds) {
    for (int i = threadIdx.x; i < nx * k; i += THREADS) lc[(i % k) * TX + i / k] = coef[i];
    __syncthreads();
  }
  const int xl = threadIdx.x % TX, yl = threadIdx.x / TX;
  if (xl >= nx) return;
  const int x = x0 + xl;
  const int lo = tab[q.xb + 2 * x], cnt = tab[q.xb + 2 * x + 1];
  const int32_t* kg = coef + (size_t)xl * k;
  uint8_t* dst = (q.flags & SKIP_COLS) ? out + q.out : mid + q.mid;
  const int y_end = min(q.rows, y0 + ROWS_PER_GROUP);
  for (int y = y0 + yl; y < y_end; y += TY) {
    const uint8_t* s = frames + (((size_t)q.frame * H + q.sy0 + q.ry0 + y) * (size_t)W + q.sx0 + lo) * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    if (in_lds) {
      for (int t = 0; t < cnt; ++t) {
        const int c = lc[t * TX + xl];
        a0 += s[3 * t] * c, a1 += s[3 * t + 1] * c, a2 += s[3 * t + 2] * c;
      }
    } else {
      for (int t = 0; t < cnt; ++t) {
        const int c = kg[t];
        a0 += s[3 * t] * c, a1 += s[3 * t + 1] * c, a2 += s[3 * t + 2] * c;
      }
    }
    uint8_t* d = dst + ((size_t)y * q.ow + x) * 3;
    d[0] = clip8(a0), d[1] = clip8(a1), d[2] = clip8(a2);
  }
}

__global__ __launch_bounds__(THREADS) void resample_cols(const uint8_t* __restrict__ frames, int H, int W,
                                                         const rs_rec* __restrict__ recs, const int32_t* __restrict__ tab,
                                                         const uint8_t* __restrict__ mid, uint8_t* __restrict__ out, int tiles_x) {
  __shared__ int32_t lc[LDS_INTS];
  const rs_rec q = recs[blockIdx.x / tiles_x];
  const int x0 = (blockIdx.x % tiles_x) * TX, y0 = blockIdx.y * TY;
  if ((q.flags & SKIP_COLS) || x0 >= q.ow || y0 >= q.oh) return;            // the same for the whole workgroup
  const int k = q.ky, ny = min(TY, q.oh - y0);
  const bool in_lds = TY * k <= LDS_INTS;
  const int32_t* coef = tab + q.yc + (size_t)y0 * k;
  if (in_lds) {
    for (int i = threadIdx.x; i < ny * k; i += THREADS) lc[i] = coef[i];
    __syncthreads();
  }
  const int xl = threadIdx.x % TX, yl = threadIdx.x / TX;
  if (xl >= min(TX, q.ow - x0) || yl >= ny) return;
  const int x = x0 + xl, y = y0 + yl;
  const int lo = tab[q.yb + 2 * y], cnt = tab[q.yb + 2 * y + 1];
  const uint8_t* s;
  size_t pitch;
  if (q.flags & SKIP_ROWS) {                                                // no horizontal pass: the image itself, ow wide
    s = frames + (((size_t)q.frame * H + q.sy0 + lo) * (size_t)W + q.sx0 + x) * 3;
    pitch = (size_t)W * 3;
  } else {
    s = mid + q.mid + ((size_t)(lo - q.ry0) * q.ow + x) * 3;
    pitch = (size_t)q.ow * 3;
  }
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  if (in_lds) {
    const int32_t* kl = lc + yl * k;
    for (int t = 0; t < cnt; ++t, s += pitch) {
      const int c = kl[t];
      a0 += s[0] * c, a1 += s[1] * c, a2 += s[2] * c;
    }
  } else {
    const int32_t* kg = coef + (size_t)yl * k;
    for (int t = 0; t < cnt; ++t, s += pitch) {
      const int c = kg[t];
      a0 += s[0] * c, a1 += s[1] * c, a2 += s[2] * c;
    }
  }
  uint8_t* d = out + q.out + ((size_t)y * q.ow + x) * 3;
  d[0] = clip8(a0), d[1] = clip8(a1), d[2] = clip8(a2);
}

// The small image of every region, enlarged to the box by NEAREST, into the frame where the region's shape covers it.
__global__ __launch_bounds__(THREADS) void pixelate_paste(uint8_t* __restrict__ frames, int H, int W, const rs_rec* __restrict__ recs,
                                                          const int32_t* __restrict__ tab, const int2* __restrict__ spans,
                                                          const uint8_t* __restrict__ small, int tiles_x) {
  const rs_rec q = recs[blockIdx.x / tiles_x];
  const int x = (blockIdx.x % tiles_x) * TX + threadIdx.x % TX, y = blockIdx.y * TY + threadIdx.x / TX;
  if (x >= q.w || y >= q.h) return;
  if (q.span >= 0) {
    const int2 sp = spans[q.span + y];                  // clamped to the box (ta_span_tables); x is in 0 .. w - 1 anyway
    if (x < sp.x || x > sp.y) return;
  }
  const int sx = tab[q.xu + 2 * x], sy = tab[q.yu + 2 * y];
  const uint8_t* s = small + q.out + ((size_t)sy * q.ow + sx) * 3;
  uint8_t* d = frames + (((size_t)q.frame * H + q.sy0 + y) * (size_t)W + q.sx0 + x) * 3;
  d[0] = s[0], d[1] = s[1], d[2] = s[2];
}

// ---- host ------------------------------------------------------------------------------------------------------------
// libImaging/Resample.c's filters
double box_filter(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double hamming_filter(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * M_PI;
  return sin(x) / x * (0.54f + 0.46f * cos(x));         // float literals, as there
}
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) { return -3.0 <= x && x < 3.0 ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

bool filter_of(int code, double (**f)(double), double* support) {
  switch (code) {
    case TA_RESAMPLE_NEAREST: *f = nullptr, *support = 0.0; return true;
    case TA_RESAMPLE_LANCZOS: *f = lanczos_filter, *support = 3.0; return true;
    case TA_RESAMPLE_BILINEAR: *f = bilinear_filter, *support = 1.0; return true;
    case TA_RESAMPLE_BICUBIC: *f = bicubic_filter, *support = 2.0; return true;
    case TA_RESAMPLE_BOX: *f = box_filter, *support = 0.5; return true;
    case TA_RESAMPLE_HAMMING: *f = hamming_filter, *support = 1.0; return true;
  }
  return false;
}

// Pillow's own check of box= along one axis
bool box_ok(float b0, float b1, int in_size) { return b0 >= 0.f && b0 < b1 && b1 <= (float)in_size; }

int axis_ksize(float b0, float b1, int out_size, int filter) {
  double (*f)(double);
  double support;
  filter_of(filter, &f, &support);
  if (!f) return 1;
  const double scale = (double)(b1 - b0) / out_size;
  return (int)ceil(support * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// One axis' tables, appended: bounds (first, count) per output sample and out_size rows of ksize coefficients.
void plan_axis(int in_size, float b0, float b1, int out_size, int filter, int32_t* bounds, int32_t* coef) {
  double (*f)(double);
  double support;
  filter_of(filter, &f, &support);
  if (!f) {                                             // ImagingScaleAffine: the coordinate is accumulated
    const double step = (double)(b1 - b0) / out_size;
    double at = b0 + step * 0.5;
    for (int i = 0; i < out_size; ++i) {
      const int s = at < 0.0 ? 0 : (int)at;
      bounds[2 * i] = std::min(s, in_size - 1);
      bounds[2 * i + 1] = 1;
      coef[i] = 1 << PRECISION_BITS;
      at += step;
    }
    return;
  }
  double filterscale, scale;
  filterscale = scale = (double)(b1 - b0) / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  support = support * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = b0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      k[x] = f((x + xmin - center + 0.5) * ss);
      ww += k[x];
    }
    int32_t* row = coef + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      if (x >= xmax) {
        row[x] = 0;
        continue;
      }
      const double v = ww != 0.0 ? k[x] / ww : k[x];
      row[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (double)(1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
}

// The tables of one call: equal axes (a whole-frame resize of a batch; faces of one size) share one copy.
struct axis_tab {
  uint32_t b, c;
  int32_t k, first, last;      // the source samples referenced: first .. last - 1
};
struct table_set {
  std::vector<int32_t> tab;
  std::map<std::tuple<int, float, float, int, int>, axis_tab> seen;

  const axis_tab& axis(int in_size, float b0, float b1, int out_size, int filter) {
    const auto key = std::make_tuple(in_size, b0, b1, out_size, filter);
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    axis_tab a;
    a.k = axis_ksize(b0, b1, out_size, filter);
    a.b = (uint32_t)tab.size();
    a.c = a.b + 2 * (uint32_t)out_size;
    tab.resize(tab.size() + (size_t)out_size * (2 + (size_t)a.k));
    plan_axis(in_size, b0, b1, out_size, filter, tab.data() + a.b, tab.data() + a.c);
    const int32_t* bd = tab.data() + a.b;
    a.first = bd[0];
    a.last = bd[2 * out_size - 2] + bd[2 * out_size - 1];
    for (int i = 0; i < out_size; ++i) a.first = std::min(a.first, bd[2 * i]), a.last = std::max(a.last, bd[2 * i] + bd[2 * i + 1]);
    return seen.emplace(key, a).first->second;
  }
  // one sample per output sample, itself: the copy of a pass-less resize
  const axis_tab& identity(int size) { return axis(size, 0.f, (float)size, size, TA_RESAMPLE_NEAREST); }
};

// The record of `image.resize((ow, oh), filter, box)` where the image is the w x h rectangle at (sx0, sy0) of a frame.
// `mid_at` is advanced by the scratch the horizontal result takes.
rs_rec make_rec(table_set& ts, int frame, int sx0, int sy0, int w, int h, float bx0, float by0, float bx1, float by1, int ow,
                int oh, int filter, size_t* mid_at) {
  rs_rec r;
  memset(&r, 0, sizeof(r));
  r.frame = frame, r.sx0 = sx0, r.sy0 = sy0, r.ow = ow, r.oh = oh, r.span = -1;
  const bool need_x = ow != w || bx0 != 0.f || bx1 != (float)w;
  const bool need_y = oh != h || by0 != 0.f || by1 != (float)h;
  if (need_y) {
    const axis_tab& y = ts.axis(h, by0, by1, oh, filter);
    r.yb = y.b, r.yc = y.c, r.ky = y.k, r.ry0 = y.first, r.rows = std::max(0, y.last - y.first);
  } else {
    r.flags |= SKIP_COLS, r.ry0 = 0, r.rows = h;
  }
  if (need_x || !need_y) {
    const axis_tab& x = need_x ? ts.axis(w, bx0, bx1, ow, filter) : ts.identity(w);
    r.xb = x.b, r.xc = x.c, r.kx = x.k;
  } else {
    r.flags |= SKIP_ROWS;
  }
  if (!(r.flags & (SKIP_ROWS | SKIP_COLS))) {
    r.mid = *mid_at;
    *mid_at += ((size_t)r.rows * ow * 3 + 15) & ~(size_t)15;
  }
  return r;
}

// Records, tables and span tables of a call in the context's scratch, the pixels behind them: one H2D copy.  Both blocks
// keep the 16 slack bytes they always had: it was not shown from the kernels that nothing reads past the staged tables.
struct staged {
  const rs_rec* recs;
  const int32_t* tab;
  const int2* spans;
  uint8_t* pixels;
};

int stage(ta_ctx* ctx, const std::vector<rs_rec>& recs, const std::vector<int32_t>& tab, const std::vector<int2>& spans,
          size_t pixel_bytes, staged* s) {
  ta_staging st;
  st.slack = 16;
  const size_t o_rec = st.put(recs), o_tab = st.put(tab), o_span = st.put(spans), o_pix = st.device_only(pixel_bytes);
  TA_TRY(st.commit(ctx));
  *s = {st.dev<const rs_rec>(o_rec), st.dev<const int32_t>(o_tab), st.dev<const int2>(o_span), st.dev<uint8_t>(o_pix)};
  return TA_OK;
}

// The workgroups both passes take over recs[first .. first + count - 1]: x for both, y of each (0: the pass is not launched).
struct pass_grid {
  int tiles_x;
  size_t x, rows_y, cols_y;
};
pass_grid grid_of(const std::vector<rs_rec>& recs, size_t first, size_t count) {
  int max_ow = 0, max_rows = 0, max_oh = 0;
  for (size_t j = first; j < first + count; ++j) {
    const rs_rec& r = recs[j];
    if (!(r.flags & SKIP_ROWS)) max_rows = std::max(max_rows, r.rows);
    if (!(r.flags & SKIP_COLS)) max_oh = std::max(max_oh, r.oh);
    max_ow = std::max(max_ow, r.ow);
  }
  const int tiles_x = (max_ow + TX - 1) / TX;
  return {tiles_x, count * tiles_x, ((size_t)max_rows + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP, ((size_t)max_oh + TY - 1) / TY};
}

// Both passes over recs[first .. first + count - 1]; `mid` and `out` are what the records' offsets count from.
void launch_passes(ta_ctx* ctx, const ta_frames* src, const staged& s, const std::vector<rs_rec>& recs, size_t first, size_t count,
                   uint8_t* mid, uint8_t* out) {
  const pass_grid g = grid_of(recs, first, count);
  if (g.rows_y > 0)
    hipLaunchKernelGGL(resample_rows, dim3((unsigned)g.x, (unsigned)g.rows_y), dim3(THREADS), 0, ctx->stream, (const uint8_t*)src->dev,
                       src->h, src->w, s.recs + first, s.tab, mid, out, g.tiles_x);
  if (g.cols_y > 0)
    hipLaunchKernelGGL(resample_cols, dim3((unsigned)g.x, (unsigned)g.cols_y), dim3(THREADS), 0, ctx->stream, (const uint8_t*)src->dev,
                       src->h, src->w, s.recs + first, s.tab, (const uint8_t*)mid, out, g.tiles_x);
}

// `regions` of `src`, checked by the caller and n > 0 of them, resized to out_w x out_h each into a new batch.  An output
// the launches cannot cover is refused here, before anything is allocated: a launch has at most 65535 workgroups along
// y and 2^32 - 1 threads along x, and the tables are addressed in 32 bits.
int resample_regions(ta_ctx* ctx, const char* who, const ta_frames* src, const ta_resample_region* regions, int n, int out_h, int out_w,
                     int filter, ta_frames** out) {
  table_set ts;
  std::vector<rs_rec> recs;
  size_t mid_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const ta_resample_region& q = regions[i];
    rs_rec r = make_rec(ts, q.frame, 0, 0, src->w, src->h, q.x0, q.y0, q.x1, q.y1, out_w, out_h, filter, &mid_bytes);
    r.out = (size_t)i * out_h * out_w * 3;
    recs.push_back(r);
  }
  const pass_grid g = grid_of(recs, 0, recs.size());
  if (g.rows_y > 65535 || g.cols_y > 65535 || g.x * THREADS > UINT32_MAX || ts.tab.size() > UINT32_MAX)
    return ta_fail(ctx, TA_E_INVALID, "%s: %d images of %d x %d from %d x %d are more than one set of launches covers", who, n, out_w, out_h,
                   src->w, src->h);
  ta_frames* dst = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, n, out_h, out_w, &dst));
  staged s;
  int rc = stage(ctx, recs, ts.tab, std::vector<int2>(), mid_bytes, &s);
  if (rc == TA_OK) {
    launch_passes(ctx, src, s, recs, 0, recs.size(), s.pixels, dst->dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);           // pinned / scratch staging is reused by the next call
    if (e != hipSuccess) rc = ta_fail(ctx, TA_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
  }
  if (rc != TA_OK) {
    ta_frames_free(dst);
    return rc;
  }
  *out = dst;
  return TA_OK;
}

}  // namespace

extern "C" int ta_resample_plan(int in_size, double b0, double b1, int out_size, int filter, int32_t* bounds, int32_t* coefs,
                                int capacity, int* ksize) {
  double (*f)(double);
  double support;
  if (in_size <= 0 || out_size <= 0 || out_size > MAX_OUT || !filter_of(filter, &f, &support) || !ksize) return TA_E_INVALID;
  const float f0 = (float)b0, f1 = (float)b1;           // the box is float32 in Pillow and in ta_resample_region
  if (!box_ok(f0, f1, in_size)) return TA_E_INVALID;
  const int k = axis_ksize(f0, f1, out_size, filter);
  *ksize = k;
  if (capacity < 0 || (int64_t)out_size * k > (int64_t)capacity) return TA_E_CAPACITY;
  if (!bounds || !coefs) return TA_E_INVALID;
  plan_axis(in_size, f0, f1, out_size, filter, bounds, coefs);
  return TA_OK;
}

extern "C" int ta_frames_resample(ta_ctx* ctx, const ta_frames* src, const ta_resample_region* regions, int n, int out_h, int out_w,
                                  int filter, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (out) *out = nullptr;
  if (!out) return ta_fail(ctx, TA_E_INVALID, "frames_resample: bad args");
  TA_TRY(ta_check_batch(ctx, "frames_resample", src, regions, n));
  double (*f)(double);
  double support;
  if (!filter_of(filter, &f, &support)) return ta_fail(ctx, TA_E_INVALID, "frames_resample: unknown filter %d", filter);
  if (out_h <= 0 || out_w <= 0 || out_h > MAX_OUT || out_w > MAX_OUT)
    return ta_fail(ctx, TA_E_INVALID, "frames_resample: output %d x %d, sides must be 1 .. %d", out_w, out_h, MAX_OUT);
  const int N = src->n, H = src->h, W = src->w;
  for (int i = 0; i < n; ++i) {
    const ta_resample_region& q = regions[i];
    TA_TRY(ta_check_frame(ctx, "frames_resample", i, q.frame, N));
    if (!box_ok(q.x0, q.x1, W) || !box_ok(q.y0, q.y1, H))
      return ta_fail(ctx, TA_E_INVALID, "frames_resample: region %d: box (%g, %g, %g, %g) must satisfy 0 <= x0 < x1 <= %d, 0 <= y0 < y1 <= %d", i,
                     q.x0, q.y0, q.x1, q.y1, W, H);
  }
  if (n == 0) return TA_OK;
  return resample_regions(ctx, "frames_resample", src, regions, n, out_h, out_w, filter, out);
}

// The whole of every image of the batch with the BICUBIC filter: one region per image, one axis table for all of them.
// No 16384 cap on a side, and an empty batch gives an empty batch.
extern "C" int ta_frames_resize_bicubic(ta_ctx* ctx, const ta_frames* src, int dst_h, int dst_w, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx || !src || !out || dst_h <= 0 || dst_w <= 0) return ta_fail(ctx, TA_E_INVALID, "frames_resize_bicubic: bad args");
  std::vector<ta_resample_region> whole(src->n);
  for (int i = 0; i < src->n; ++i) whole[i] = {i, 0.f, 0.f, (float)src->w, (float)src->h};
  TA_TRY(ta_check_batch(ctx, "frames_resize_bicubic", src, whole.data(), src->n));
  if (src->n == 0) return ta_frames_alloc_uninit(ctx, 0, dst_h, dst_w, out);
  return resample_regions(ctx, "frames_resize_bicubic", src, whole.data(), src->n, dst_h, dst_w, TA_RESAMPLE_BICUBIC, out);
}

extern "C" int ta_frames_pixelate(ta_ctx* ctx, ta_frames* frames, const ta_pixelate_region* regions, int n) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  char why[64];
  TA_TRY(ta_check_regions(ctx, "frames_pixelate", frames, regions, n, MAX_OUT, [&](const ta_pixelate_region& q) {
    if (q.block >= 1 && q.block <= MAX_OUT) return (const char*)nullptr;
    snprintf(why, sizeof(why), "block %d, must be 1 .. %d", q.block, MAX_OUT);
    return (const char*)why;
  }));
  if (n == 0) return TA_OK;

  const int H = frames->h, W = frames->w;
  table_set ts;
  std::vector<rs_rec> recs;
  ta_span_tables spans;
  std::vector<size_t> first(1, 0);                      // the first record of every round, and the end
  size_t pixel_bytes = 0, small_at = 0, mid_at = 0;
  const int rounds = ta_each_round(
      regions, n,
      [&](const ta_pixelate_region& q) {
        if (q.block == 1) return;                       // block 1: the region as it is
        const int w = q.x1 - q.x0, h = q.y1 - q.y0, sw = std::max(1, w / q.block), sh = std::max(1, h / q.block);
        rs_rec r = make_rec(ts, q.frame, q.x0, q.y0, w, h, 0.f, 0.f, (float)w, (float)h, sw, sh, TA_RESAMPLE_BOX, &mid_at);
        r.w = w, r.h = h;
        r.xu = ts.axis(sw, 0.f, (float)sw, w, TA_RESAMPLE_NEAREST).b;
        r.yu = ts.axis(sh, 0.f, (float)sh, h, TA_RESAMPLE_NEAREST).b;
        if (q.shape == TA_BLUR_ELLIPSE) r.span = spans.of(w, h);
        r.out = small_at;
        small_at += ((size_t)sw * sh * 3 + 15) & ~(size_t)15;
        recs.push_back(r);
      },
      [&] {
        for (size_t j = first.back(); j < recs.size(); ++j) recs[j].mid += small_at;   // the round's small images, then its horizontal results
        pixel_bytes = std::max(pixel_bytes, small_at + mid_at);
        first.push_back(recs.size());
        small_at = mid_at = 0;
      });
  if (recs.empty()) return TA_OK;

  staged s;
  TA_TRY(stage(ctx, recs, ts.tab, spans.table(), pixel_bytes, &s));
  for (int k = 0; k < rounds; ++k) {
    const size_t count = first[k + 1] - first[k];
    if (!count) continue;
    launch_passes(ctx, frames, s, recs, first[k], count, s.pixels, s.pixels);
    int max_w = 0, max_h = 0;
    for (size_t j = first[k]; j < first[k + 1]; ++j) max_w = std::max(max_w, recs[j].w), max_h = std::max(max_h, recs[j].h);
    const int tiles_x = (max_w + TX - 1) / TX;
    hipLaunchKernelGGL(pixelate_paste, dim3((unsigned)(count * tiles_x), (max_h + TY - 1) / TY), dim3(THREADS), 0, ctx->stream, frames->dev, H, W,
                       s.recs + first[k], s.tab, s.spans, (const uint8_t*)s.pixels, tiles_x);
  }
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));       // pinned / scratch staging is reused by the next call
  return TA_OK;
}
