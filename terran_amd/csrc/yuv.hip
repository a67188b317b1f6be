// Raw YUV video frames in and out (ta_frames_from_yuv, ta_frames_to_yuv): yuv420p, nv12 and yuv444p as ffmpeg's rawvideo
// lays them out, converted with the standards' affine maps, exact rationals rounded once (include/terran_amd.h states the
// definition, tests/yuv_model.py restates it in numpy).  No swscale parity is claimed.
//
// Arithmetic: yuv_math.h -- 64-bit fixed point at a scale that is shown to give the exact floor.  Integer work only, so this
// unit needs no -ffp-contract=off.  The host builds the rows from the rationals (yuv_make_consts) and the kernels take them
// as arguments.
//
// Device side, both kernels: a thread owns a unit of four pixels of BOTH luma rows of a chroma row -- x = 4 u .. 4 u + 3,
// y = 2 j and 2 j + 1 -- so a unit starts on the chroma grid, the chroma row j is fetched (from_yuv) or produced (to_yuv)
// once for the pair of rows (a bilinear luma row adds the chroma row beyond it, j - 1 or j + 1, which only it uses), and
// consecutive lanes take consecutive units of a row: 12 bytes of RGB and 4 of luma per lane and
// row.  Frames of 4:2:0 video may have an odd size and rows an odd width, so every row starts at an arbitrary address.
// Reads of a unit's bytes are ALIGNED dwords around them, shifted into place (load_span: only dwords that hold a byte of
// the unit are read, so nothing outside the buffer is); stores are aligned dwords with single bytes in front and behind
// (store_span: no byte outside the unit is written, the neighbouring lanes own those).  With w a multiple of four every
// RGB store is three dwords, as in pixel_walk.h's walk_row.  The few chroma samples that a bilinear unit needs around its
// own (clamped to the plane) are byte loads.  Every byte offset is a size_t: n frames may pass 2^31 bytes.
#include "ta_internal.h"
#include "yuv_math.h"

#include <string.h>

#include <algorithm>

namespace {

constexpr int THREADS = 256;
constexpr int MAX_SIDE = 65535;
constexpr size_t SLACK = 16;                 // behind the staged frames

enum { MODE_NEAREST = 0, MODE_LEFT = 1, MODE_CENTER = 2 };

struct yuv_geom {
  int n, h, w, cw, ch;
  int format, mode;                          // TA_YUV_420P .. ; MODE_*
  size_t frame_bytes;
};

// ---- device ----------------------------------------------------------------------------------------------------------
// `need` (1 .. 4 NDW) bytes at p as NDW dwords, byte 0 of p in the low byte of d[0]; bytes past `need` are unspecified
template <int NDW>
__device__ inline void load_span(const uint8_t* p, int need, uint32_t* d) {
  const uintptr_t at = (uintptr_t)p;
  const uint32_t* a = (const uint32_t*)(at & ~(uintptr_t)3);
  const int lead = (int)(at & 3), sh = lead * 8;
  uint32_t w[NDW + 1];
#pragma unroll
  for (int i = 0; i <= NDW; ++i) w[i] = 4 * i < lead + need ? a[i] : 0u;       // dword i holds bytes 4 i - lead .. of the span
#pragma unroll
  for (int i = 0; i < NDW; ++i) d[i] = lead ? (w[i] >> sh) | (w[i + 1] << (32 - sh)) : w[i];
}

// the first `nbytes` (0 .. 4 NDW) bytes of d to q: single bytes up to the first aligned address, dwords, single bytes
template <int NDW>
__device__ inline void store_span(uint8_t* q, const uint32_t* d, int nbytes) {
  const int head = min(nbytes, (int)((4 - ((uintptr_t)q & 3)) & 3)), dwords = (nbytes - head) >> 2, tail = head + 4 * dwords;
#pragma unroll
  for (int b = 0; b < 4 * NDW; ++b)
    if ((b < head || b >= tail) && b < nbytes) q[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
  const int sh = head * 8;
#pragma unroll
  for (int i = 0; i < NDW; ++i)
    if (i < dwords) {
      const uint32_t hi = i + 1 < NDW ? d[i + 1] : 0u;
      *(uint32_t*)(q + head + 4 * i) = head ? (d[i] >> sh) | (hi << (32 - sh)) : d[i];
    }
}

__device__ inline uint32_t byte_of(uint32_t v, int k) { return v >> (8 * k) & 255u; }

// A unit: frame, chroma row, unit of the row.  The grid's x runs over the units of a row, its y strides over the row pairs
// of the batch, so frame and row come from one division that is uniform in the workgroup.
struct unit_at {
  size_t f;
  int j, u;
};

// where the chroma samples of a 4:2:0 frame lie: sample (r, c) of U at u + r * row + c * step, of V likewise
struct chroma_planes {
  size_t u, v, row;
  int step;
};
__device__ inline chroma_planes planes_of(const yuv_geom& g) {
  const size_t luma = (size_t)g.h * g.w;
  if (g.format == TA_YUV_NV12) return {luma, luma + 1, (size_t)g.cw * 2, 2};
  return {luma, luma + (size_t)g.cw * g.ch, (size_t)g.cw, 1};
}

__global__ __launch_bounds__(THREADS) void from_yuv_kernel(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, const yuv_geom g,
                                                           const yuv_consts k) {
  const int u = (int)(blockIdx.x * THREADS + threadIdx.x);
  if (u >= (g.w + 3) >> 2) return;
  const size_t pairs_of_rows = (size_t)g.n * g.ch;
  const chroma_planes cp = planes_of(g);
  for (size_t rp = blockIdx.y; rp < pairs_of_rows; rp += gridDim.y) {
    const size_t frame = rp / (size_t)g.ch;
    const unit_at t = {frame, (int)(rp - frame * (size_t)g.ch), u};
    const uint8_t* fb = yuv + t.f * g.frame_bytes;
    const int x0 = 4 * t.u, cnt = min(4, g.w - x0);
    // 4:2:0: the unit's own chroma row at the columns 2 u - 1 .. 2 u + 2, clamped, read once for both luma rows (nearest
    // needs the middle two only)
    size_t col[4];
    uint32_t nu[4] = {0, 0, 0, 0}, nv[4] = {0, 0, 0, 0};
    if (g.format != TA_YUV_444P) {
      const size_t near = (size_t)t.j * cp.row;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        col[c] = (size_t)min(max(2 * t.u - 1 + c, 0), g.cw - 1) * cp.step;
        if (g.mode != MODE_NEAREST || c == 1 || c == 2) nu[c] = fb[cp.u + near + col[c]], nv[c] = fb[cp.v + near + col[c]];
      }
    }
    for (int half = 0; half < 2; ++half) {
      const int y = 2 * t.j + half;
      if (y >= g.h) break;
      const size_t row = (size_t)y * g.w + x0;
      uint32_t yy, cb[4], cr[4];
      load_span<1>(fb + row, cnt, &yy);
      if (g.format == TA_YUV_444P) {
        uint32_t uu, vv;
        load_span<1>(fb + (size_t)g.h * g.w + row, cnt, &uu);
        load_span<1>(fb + 2 * (size_t)g.h * g.w + row, cnt, &vv);
#pragma unroll
        for (int p = 0; p < 4; ++p) cb[p] = byte_of(uu, p), cr[p] = byte_of(vv, p);
      } else if (g.mode == MODE_NEAREST) {
        cb[0] = cb[1] = nu[1], cb[2] = cb[3] = nu[2];
        cr[0] = cr[1] = nv[1], cr[2] = cr[3] = nv[2];
      } else {
        // vertical sums of the four columns: 3 of the unit's own chroma row, 1 of the one beyond this luma row
        const size_t far = (size_t)(half ? min(t.j + 1, g.ch - 1) : max(t.j - 1, 0)) * cp.row;
        uint32_t su[4], sv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          su[c] = 3u * nu[c] + fb[cp.u + far + col[c]];
          sv[c] = 3u * nv[c] + fb[cp.v + far + col[c]];
        }
        if (g.mode == MODE_LEFT) {
          cb[0] = yuv_chroma_left_even(su[1]), cb[1] = yuv_chroma_left_odd(su[1], su[2]);
          cb[2] = yuv_chroma_left_even(su[2]), cb[3] = yuv_chroma_left_odd(su[2], su[3]);
          cr[0] = yuv_chroma_left_even(sv[1]), cr[1] = yuv_chroma_left_odd(sv[1], sv[2]);
          cr[2] = yuv_chroma_left_even(sv[2]), cr[3] = yuv_chroma_left_odd(sv[2], sv[3]);
        } else {
          cb[0] = yuv_chroma_center(su[1], su[0]), cb[1] = yuv_chroma_center(su[1], su[2]);
          cb[2] = yuv_chroma_center(su[2], su[1]), cb[3] = yuv_chroma_center(su[2], su[3]);
          cr[0] = yuv_chroma_center(sv[1], sv[0]), cr[1] = yuv_chroma_center(sv[1], sv[2]);
          cr[2] = yuv_chroma_center(sv[2], sv[1]), cr[3] = yuv_chroma_center(sv[2], sv[3]);
        }
      }
      uint32_t r[4], gg[4], b[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t l = byte_of(yy, p);
        r[p] = yuv_apply(k.rgb[0], l, cb[p], cr[p]);
        gg[p] = yuv_apply(k.rgb[1], l, cb[p], cr[p]);
        b[p] = yuv_apply(k.rgb[2], l, cb[p], cr[p]);
      }
      uint32_t d[3];
      d[0] = r[0] | gg[0] << 8 | b[0] << 16 | r[1] << 24;
      d[1] = gg[1] | b[1] << 8 | r[2] << 16 | gg[2] << 24;
      d[2] = b[2] | r[3] << 8 | gg[3] << 16 | b[3] << 24;
      store_span<3>(rgb + (t.f * g.h * g.w + row) * 3, d, 3 * cnt);
    }
  }
}

__global__ __launch_bounds__(THREADS) void to_yuv_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yuv, const yuv_geom g,
                                                         const yuv_consts k) {
  const int u = (int)(blockIdx.x * THREADS + threadIdx.x);
  if (u >= (g.w + 3) >> 2) return;
  const size_t pairs_of_rows = (size_t)g.n * g.ch;
  const chroma_planes cp = planes_of(g);
  for (size_t rp = blockIdx.y; rp < pairs_of_rows; rp += gridDim.y) {
    const size_t frame = rp / (size_t)g.ch;
    const unit_at t = {frame, (int)(rp - frame * (size_t)g.ch), u};
    uint8_t* fb = yuv + t.f * g.frame_bytes;
    const int x0 = 4 * t.u, cnt = min(4, g.w - x0);
    uint32_t sr[2] = {0, 0}, sg[2] = {0, 0}, sb[2] = {0, 0};       // the unit's two blocks: sums over the pixels inside the frame
    const int rows = min(2, g.h - 2 * t.j);
    for (int half = 0; half < rows; ++half) {
      const size_t row = (size_t)(2 * t.j + half) * g.w + x0;
      uint32_t d[3];
      load_span<3>(rgb + (t.f * g.h * g.w + row) * 3, 3 * cnt, d);
      uint32_t r[4], gg[4], b[4];
      r[0] = d[0] & 255, gg[0] = d[0] >> 8 & 255, b[0] = d[0] >> 16 & 255, r[1] = d[0] >> 24;
      gg[1] = d[1] & 255, b[1] = d[1] >> 8 & 255, r[2] = d[1] >> 16 & 255, gg[2] = d[1] >> 24;
      b[2] = d[2] & 255, r[3] = d[2] >> 8 & 255, gg[3] = d[2] >> 16 & 255, b[3] = d[2] >> 24;
      uint32_t yy = 0, uu = 0, vv = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        yy |= yuv_apply(k.yuv[0], 4 * r[p], 4 * gg[p], 4 * b[p]) << (8 * p);
        if (g.format == TA_YUV_444P) {
          uu |= yuv_apply(k.yuv[1], 4 * r[p], 4 * gg[p], 4 * b[p]) << (8 * p);
          vv |= yuv_apply(k.yuv[2], 4 * r[p], 4 * gg[p], 4 * b[p]) << (8 * p);
        } else if (p < cnt) {
          sr[p >> 1] += r[p], sg[p >> 1] += gg[p], sb[p >> 1] += b[p];
        }
      }
      store_span<1>(fb + row, &yy, cnt);
      if (g.format == TA_YUV_444P) {
        store_span<1>(fb + (size_t)g.h * g.w + row, &uu, cnt);
        store_span<1>(fb + 2 * (size_t)g.h * g.w + row, &vv, cnt);
      }
    }
    if (g.format == TA_YUV_444P) continue;
    uint32_t cu[2] = {0, 0}, cv[2] = {0, 0};
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int cols = min(2, cnt - 2 * blk);
      if (cols <= 0) continue;
      const uint32_t up = 4u / (uint32_t)(cols * rows);            // 1, 2 or 4 pixels: the sums in quarters of the mean
      cu[blk] = yuv_apply(k.yuv[1], up * sr[blk], up * sg[blk], up * sb[blk]);
      cv[blk] = yuv_apply(k.yuv[2], up * sr[blk], up * sg[blk], up * sb[blk]);
    }
    const int samples = (cnt + 1) >> 1;
    const size_t at = (size_t)t.j * cp.row + (size_t)(2 * t.u) * cp.step;
    if (g.format == TA_YUV_NV12) {
      const uint32_t uv = cu[0] | cv[0] << 8 | cu[1] << 16 | cv[1] << 24;
      store_span<1>(fb + cp.u + at, &uv, 2 * samples);
    } else {
      const uint32_t us = cu[0] | cu[1] << 8, vs = cv[0] | cv[1] << 8;
      store_span<1>(fb + cp.u + at, &us, samples);
      store_span<1>(fb + cp.v + at, &vs, samples);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// exact rationals over 128-bit integers: the coefficients are products of a few small numbers
typedef __int128 wide;
struct rat {
  wide n, d;                                 // d > 0, reduced
};
wide gcd_of(wide a, wide b) {
  if (a < 0) a = -a;
  while (b) {
    const wide t = a % b;
    a = b, b = t;
  }
  return a;
}
rat make(wide n, wide d) {
  if (d < 0) n = -n, d = -d;
  const wide c = gcd_of(n, d);
  return c > 1 ? rat{n / c, d / c} : rat{n, d};
}
rat operator*(const rat& a, const rat& b) { return make(a.n * b.n, a.d * b.d); }
rat operator+(const rat& a, const rat& b) { return make(a.n * b.d + b.n * a.d, a.d * b.d); }
rat operator-(const rat& a) { return rat{-a.n, a.d}; }
rat operator/(const rat& a, const rat& b) { return make(a.n * b.d, a.d * b.n); }
wide floor_div(wide a, wide b) {             // b > 0
  const wide q = a / b;
  return a % b < 0 ? q - 1 : q;
}
int64_t fixed(const rat& r) { return (int64_t)floor_div(2 * r.n * ((wide)1 << YUV_SHIFT) + r.d, 2 * r.d); }   // nearest

// The row of v = c[0] a + c[1] b + c[2] c + c0 for inputs 0 .. top, c0 with the rounding half in it (yuv_math.h): false when
// the scale does not carry the common denominator.
bool yuv_make_row(const rat* c, const rat& c0, int top, yuv_row* out) {
  wide q = 2;
  for (int i = 0; i < 4; ++i) {
    const wide d = i < 3 ? c[i].d : c0.d;
    q = q / gcd_of(q, d) * d;
  }
  if (q * 2 * (3 * (wide)top + 1) >= ((wide)1 << (YUV_SHIFT + 1))) return false;      // errors (3 top + 1) / 2 < 2^S / (2 q)
  for (int i = 0; i < 3; ++i) out->k[i] = fixed(c[i]);
  out->k0 = fixed(c0 + make(1, 2 * q));
  return true;
}

bool yuv_make_consts(int matrix, int range, yuv_consts* k) {
  const wide D = matrix == TA_YUV_BT601 ? 1000 : 10000;
  const rat kr = make(matrix == TA_YUV_BT601 ? 299 : 2126, D), kb = make(matrix == TA_YUV_BT601 ? 114 : 722, D);
  const rat one = make(1, 1), two = make(2, 1), half = make(1, 2), zero = make(0, 1);
  const rat kg = one + -kr + -kb;
  const bool tv = range == TA_YUV_TV;
  const rat y0 = make(tv ? 16 : 0, 1), ys = make(tv ? 219 : 255, 1), cs = make(tv ? 224 : 255, 1), full = make(255, 1), mid = make(128, 1);
  // 255 X' + 1/2 over (Y, Cb, Cr)
  const rat ay = full / ys, rv = full * two * (one + -kr) / cs, bu = full * two * (one + -kb) / cs;
  const rat gv = -(full * two * kr * (one + -kr) / kg / cs), gu = -(full * two * kb * (one + -kb) / kg / cs);
  const rat rows_rgb[3][3] = {{ay, zero, rv}, {ay, gu, gv}, {ay, bu, zero}};
  for (int c = 0; c < 3; ++c) {
    const rat c0 = -(ay * y0) + -(mid * (rows_rgb[c][1] + rows_rgb[c][2])) + half;
    if (!yuv_make_row(rows_rgb[c], c0, 255, &k->rgb[c])) return false;
  }
  // Y, Cb, Cr over the quarters (4 R, 4 G, 4 B)
  const rat q = make(1, 4), sy = ys / full * q, sb = cs / full / (two * (one + -kb)) * q, sr = cs / full / (two * (one + -kr)) * q;
  const rat rows_yuv[3][3] = {{sy * kr, sy * kg, sy * kb}, {-(sb * kr), -(sb * kg), sb * (one + -kb)}, {sr * (one + -kr), -(sr * kg), -(sr * kb)}};
  for (int c = 0; c < 3; ++c)
    if (!yuv_make_row(rows_yuv[c], (c == 0 ? y0 : mid) + half, 1020, &k->yuv[c])) return false;
  return true;
}

const char* spec_defect(const ta_yuv_spec* s) {
  if (!s) return "null spec";
  if (s->format != TA_YUV_420P && s->format != TA_YUV_NV12 && s->format != TA_YUV_444P) return "unknown format";
  if (s->matrix != TA_YUV_BT601 && s->matrix != TA_YUV_BT709) return "unknown matrix";
  if (s->range != TA_YUV_TV && s->range != TA_YUV_PC) return "unknown range";
  if (s->chroma != TA_YUV_NEAREST && s->chroma != TA_YUV_BILINEAR) return "unknown chroma";
  if (s->siting != TA_YUV_LEFT && s->siting != TA_YUV_CENTER) return "unknown siting";
  return nullptr;
}

yuv_geom geom_of(const ta_yuv_spec& s, int n, int h, int w) {
  yuv_geom g;
  g.n = n, g.h = h, g.w = w, g.cw = (w + 1) >> 1, g.ch = (h + 1) >> 1;
  g.format = s.format;
  g.mode = s.chroma == TA_YUV_NEAREST ? MODE_NEAREST : (s.siting == TA_YUV_LEFT ? MODE_LEFT : MODE_CENTER);
  g.frame_bytes = ta_yuv_frame_bytes(s.format, h, w);
  return g;
}

dim3 grid_of(const yuv_geom& g) {
  const int ux = (g.w + 3) >> 2;
  return dim3((unsigned)((ux + THREADS - 1) / THREADS), (unsigned)std::min<size_t>((size_t)g.n * g.ch, 65535));
}

// launch() between an event pair of profiling class `klass` while the context profiles (tools/yuv_bench.py: the kernel's
// own time); otherwise launch() alone, which leaves the context's profiling state untouched
template <class F>
void timed_launch(ta_ctx* ctx, int klass, double bytes, F launch) {
  if (!ctx->profiling) return launch();
  ta_prof_scope scope(ctx, klass, bytes);
  launch();
}

// ta_frames_from_yuv's own staging block (ta_ctx::yuv_in): idle between calls, every call ends with a synchronisation
int staging_in(ta_ctx* ctx, size_t bytes, void** out) {
  if (bytes > ctx->yuv_in_bytes) {
    if (ctx->yuv_in) (void)hipFree(ctx->yuv_in);
    ctx->yuv_in = nullptr, ctx->yuv_in_bytes = 0;
    const size_t want = bytes + bytes / 4 + (1 << 16);
    TA_HIP(ctx, hipMalloc(&ctx->yuv_in, want));
    ctx->yuv_in_bytes = want;
  }
  *out = ctx->yuv_in;
  return TA_OK;
}

}  // namespace

extern "C" size_t ta_yuv_frame_bytes(int format, int h, int w) {
  if (h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE) return 0;
  const size_t luma = (size_t)h * w, chroma = (size_t)((h + 1) >> 1) * ((w + 1) >> 1);
  if (format == TA_YUV_420P || format == TA_YUV_NV12) return luma + 2 * chroma;
  return format == TA_YUV_444P ? 3 * luma : 0;
}

extern "C" int ta_yuv_convert_samples(const ta_yuv_spec* spec, int to_yuv, const uint8_t* in3, size_t n, uint8_t* out3) {
  if (spec_defect(spec) || (to_yuv != 0 && to_yuv != 1) || (n > 0 && (!in3 || !out3))) return TA_E_INVALID;
  yuv_consts k;
  if (!yuv_make_consts(spec->matrix, spec->range, &k)) return TA_E_INVALID;
  const yuv_row* rows = to_yuv ? k.yuv : k.rgb;
  const uint32_t up = to_yuv ? 4 : 1;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t a = up * in3[3 * i], b = up * in3[3 * i + 1], c = up * in3[3 * i + 2];
    for (int ch = 0; ch < 3; ++ch) out3[3 * i + ch] = (uint8_t)yuv_apply(rows[ch], a, b, c);
  }
  return TA_OK;
}

extern "C" int ta_frames_from_yuv(ta_ctx* ctx, const uint8_t* host_yuv, int n, int h, int w, const ta_yuv_spec* spec, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (!host_yuv || !out || n < 1) return ta_fail(ctx, TA_E_INVALID, "frames_from_yuv: bad args");
  if (const char* why = spec_defect(spec)) return ta_fail(ctx, TA_E_INVALID, "frames_from_yuv: %s", why);
  const yuv_geom g = geom_of(*spec, n, h, w);
  if (!g.frame_bytes) return ta_fail(ctx, TA_E_INVALID, "frames_from_yuv: %d x %d: a side outside 1 .. %d", w, h, MAX_SIDE);
  yuv_consts k;
  if (!yuv_make_consts(spec->matrix, spec->range, &k)) return ta_fail(ctx, TA_E_INVALID, "frames_from_yuv: the fixed-point scale is too small");
  const size_t bytes = (size_t)n * g.frame_bytes;
  void* staged = nullptr;
  TA_TRY(staging_in(ctx, bytes + SLACK, &staged));
  ta_frames* f = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, n, h, w, &f));
  hipError_t e = hipMemcpyAsync(staged, host_yuv, bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    timed_launch(ctx, 2, (double)bytes + (double)n * h * w * 3, [&] {
      hipLaunchKernelGGL(from_yuv_kernel, grid_of(g), dim3(THREADS), 0, ctx->stream, (const uint8_t*)staged, f->dev, g, k);
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging block is reused by the next call
  if (e != hipSuccess) {
    ta_frames_free(f);
    return ta_fail(ctx, TA_E_DEVICE, "frames_from_yuv: %s", hipGetErrorString(e));
  }
  *out = f;
  return TA_OK;
}

extern "C" int ta_frames_to_yuv(ta_ctx* ctx, const ta_frames* frames, const ta_yuv_spec* spec, uint8_t* host_yuv) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (!frames || !host_yuv || frames->n < 1) return ta_fail(ctx, TA_E_INVALID, "frames_to_yuv: bad args");
  if (frames->ctx->device != ctx->device) return ta_fail(ctx, TA_E_INVALID, "frames_to_yuv: the batch lives on another device");
  if (const char* why = spec_defect(spec)) return ta_fail(ctx, TA_E_INVALID, "frames_to_yuv: %s", why);
  const yuv_geom g = geom_of(*spec, frames->n, frames->h, frames->w);
  if (!g.frame_bytes) return ta_fail(ctx, TA_E_INVALID, "frames_to_yuv: %d x %d: a side outside 1 .. %d", frames->w, frames->h, MAX_SIDE);
  yuv_consts k;
  if (!yuv_make_consts(spec->matrix, spec->range, &k)) return ta_fail(ctx, TA_E_INVALID, "frames_to_yuv: the fixed-point scale is too small");
  const size_t bytes = (size_t)g.n * g.frame_bytes;
  void* staged = nullptr;
  TA_TRY(ta_scratch(ctx, bytes + SLACK, &staged));
  timed_launch(ctx, 3, (double)bytes + (double)g.n * g.h * g.w * 3, [&] {
    hipLaunchKernelGGL(to_yuv_kernel, grid_of(g), dim3(THREADS), 0, ctx->stream, (const uint8_t*)frames->dev, (uint8_t*)staged, g, k);
  });
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipMemcpyAsync(host_yuv, staged, bytes, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}
