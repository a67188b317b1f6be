// Device-resident uint8 frame batches: allocation (with the context's cache of parked buffers), upload, download, the
// cv2-style bilinear resize and the zero-pad paste.  The Pillow resize of a batch is resample.hip's.
#include <cmath>

#include "frame_regions.h"

// cv2.resize INTER_LINEAR for uint8 (OpenCV's classic two-pass fixed-point bilinear: 11-bit
// coefficients; horizontal pass into int, vertical pass ((b0*(r0>>4))>>16 + (b1*(r1>>4))>>16 + 2)>>2).
// Coefficient tables are built on the host exactly as oracle/facade.py does and uploaded.
__global__ __launch_bounds__(256) void resize_linear_kernel(const uint8_t* src, int N, int H, int W, uint8_t* dst,
                                                             int dh, int dw, const int32_t* xtab, const int32_t* ytab) {
  // xtab: [dw][4] = sx0, sx1, a0, a1 ; ytab: [dh][4] = y0, y1, b0, b1
  const size_t total = (size_t)N * dh * dw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    size_t pix = i;
    const int x = (int)(pix % dw);
    pix /= dw;
    const int y = (int)(pix % dh);
    const int img = (int)(pix / dh);
    const int4 xt = *(const int4*)(xtab + 4 * x);
    const int4 yt = *(const int4*)(ytab + 4 * y);
    const uint8_t* r0 = src + ((size_t)img * H + yt.x) * W * 3;
    const uint8_t* r1 = src + ((size_t)img * H + yt.y) * W * 3;
    uint8_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = r0[xt.x * 3 + c] * xt.z + r0[xt.y * 3 + c] * xt.w;
      const int h1 = r1[xt.x * 3 + c] * xt.z + r1[xt.y * 3 + c] * xt.w;
      int v = (((yt.z * (h0 >> 4)) >> 16) + ((yt.w * (h1 >> 4)) >> 16) + 2) >> 2;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      o[c] = (uint8_t)v;
    }
    uint8_t* d = dst + i * 3;
    d[0] = o[0];
    d[1] = o[1];
    d[2] = o[2];
  }
}

__global__ __launch_bounds__(256) void paste_kernel(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw,
                                                     int top, int left) {
  const size_t total = (size_t)sh * sw * 3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    size_t pix = i / 3;
    const int x = (int)(pix % sw);
    const int y = (int)(pix / sw);
    dst[((size_t)(y + top) * dw + x + left) * 3 + c] = src[i];
  }
}

static void axis_table(int src, int dst, bool clamp_frac, std::vector<int32_t>& tab) {
  // mirrors oracle/facade.py:_axis_coeffs/_to_short (OpenCV resize.cpp semantics)
  tab.resize((size_t)dst * 4);
  const double scale = 1.0 / ((double)dst / (double)src);
  for (int d = 0; d < dst; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    int s0, s1;
    if (clamp_frac) {
      if (s < 0) { f = 0.f; s = 0; }
      if (s >= src - 1) { f = 0.f; s = src - 1; }
      s0 = s;
      s1 = s + 1 < src ? s + 1 : src - 1;
    } else {
      s0 = s < 0 ? 0 : (s > src - 1 ? src - 1 : s);
      s1 = s + 1 < 0 ? 0 : (s + 1 > src - 1 ? src - 1 : s + 1);
    }
    auto to_short = [](float c) {
      float v = nearbyintf(c * 2048.0f);   // round half to even (default rounding mode)
      if (v > 32767.f) v = 32767.f;
      if (v < -32768.f) v = -32768.f;
      return (int32_t)v;
    };
    tab[4 * d + 0] = s0;
    tab[4 * d + 1] = s1;
    tab[4 * d + 2] = to_short(1.0f - f);
    tab[4 * d + 3] = to_short(f);
  }
}

extern "C" {

int ta_host_alloc(ta_ctx* ctx, size_t bytes, void** out) {
  ta_enter(ctx);
  if (!ctx || !out || bytes == 0) return ta_fail(ctx, TA_E_INVALID, "host_alloc: bad args");
  *out = nullptr;
  TA_HIP(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return TA_OK;
}

void ta_host_free(ta_ctx* ctx, void* ptr) {
  ta_enter(ctx);
  if (ptr) (void)hipHostFree(ptr);
}

// parked frame buffers per context: a handful of recent sizes, bounded in bytes
#define TA_FRAME_CACHE_SLOTS 8
#define TA_FRAME_CACHE_BYTES ((size_t)2 << 30)
static int frames_alloc(ta_ctx* ctx, int n, int h, int w, bool zero, ta_frames** out);

int ta_frames_alloc(ta_ctx* ctx, int n, int h, int w, ta_frames** out) {
  ta_enter(ctx);
  return frames_alloc(ctx, n, h, w, true, out);
}

static int frames_alloc(ta_ctx* ctx, int n, int h, int w, bool zero, ta_frames** out) {
  if (!ctx || !out || n < 0 || h <= 0 || w <= 0) return ta_fail(ctx, TA_E_INVALID, "frames_alloc: bad shape");
  ta_frames* f = new ta_frames{ctx, n, h, w, nullptr};
  size_t bytes = ((size_t)n * h * w * 3 + 15) & ~(size_t)15;      // kernels read the frames in aligned dwords (rf_stem_kernel)
  if (bytes == 0) bytes = 16;
  {
    std::lock_guard<std::mutex> lock(ctx->frame_cache_mu);
    for (size_t i = 0; i < ctx->frame_cache.size(); ++i)
      if (ctx->frame_cache[i].first == bytes) {
        f->dev = (uint8_t*)ctx->frame_cache[i].second;
        ctx->frame_cache_bytes -= bytes;
        ctx->frame_cache.erase(ctx->frame_cache.begin() + i);
        break;
      }
  }
  if (!f->dev) {
    hipError_t e = hipMalloc((void**)&f->dev, bytes);
    if (e != hipSuccess) {
      delete f;
      return ta_fail(ctx, TA_E_DEVICE, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
  }
  f->cap = bytes;
  if (zero) TA_HIP(ctx, hipMemsetAsync(f->dev, 0, bytes, ctx->stream));   // only pad-merge canvases need zeros
  *out = f;
  return TA_OK;
}

int ta_frames_upload(ta_ctx* ctx, const uint8_t* nhwc_rgb, int n, int h, int w, ta_frames** out) {
  if (!ctx || !out) return TA_E_INVALID;
  ta_enter(ctx);            // hipMalloc below must land on the context's GPU, whatever the calling thread used last
  if (!nhwc_rgb && n > 0) return ta_fail(ctx, TA_E_INVALID, "frames_upload: null data");
  TA_TRY(frames_alloc(ctx, n, h, w, false, out));
  const size_t bytes = (size_t)n * h * w * 3;
  if (bytes) {
    TA_HIP(ctx, hipMemcpyAsync((*out)->dev, nhwc_rgb, bytes, hipMemcpyHostToDevice, ctx->stream));
    TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // caller's buffer may be reused immediately
  }
  return TA_OK;
}

int ta_frames_shape(const ta_frames* f, int* n, int* h, int* w) {
  if (!f) return TA_E_INVALID;
  if (n) *n = f->n;
  if (h) *h = f->h;
  if (w) *w = f->w;
  return TA_OK;
}

int ta_frames_download(const ta_frames* f, uint8_t* nhwc_rgb) {
  ta_enter(f ? f->ctx : nullptr);
  if (!f || !nhwc_rgb) return TA_E_INVALID;
  ta_ctx* ctx = f->ctx;
  const size_t bytes = (size_t)f->n * f->h * f->w * 3;
  if (bytes) {
    TA_HIP(ctx, hipMemcpyAsync(nhwc_rgb, f->dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return TA_OK;
}

void ta_frames_free(ta_frames* f) {
  ta_enter(f ? f->ctx : nullptr);
  if (!f) return;
  ta_ctx* ctx = f->ctx;
  (void)hipStreamSynchronize(ctx->stream);
  if (f->dev) {
    // every entry point is synchronous at its end, so the buffer is idle here: park it for the next batch
    std::vector<void*> evict;
    {
      std::lock_guard<std::mutex> lock(ctx->frame_cache_mu);
      ctx->frame_cache.emplace_back(f->cap, f->dev);
      ctx->frame_cache_bytes += f->cap;
      while (ctx->frame_cache.size() > TA_FRAME_CACHE_SLOTS || ctx->frame_cache_bytes > TA_FRAME_CACHE_BYTES) {
        ctx->frame_cache_bytes -= ctx->frame_cache.front().first;
        evict.push_back(ctx->frame_cache.front().second);
        ctx->frame_cache.erase(ctx->frame_cache.begin());
      }
    }
    for (void* p : evict) (void)hipFree(p);
  }
  delete f;
}

int ta_frames_resize(ta_ctx* ctx, const ta_frames* src, int dst_h, int dst_w, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx || !src || !out || dst_h <= 0 || dst_w <= 0) return ta_fail(ctx, TA_E_INVALID, "frames_resize: bad args");
  TA_TRY(frames_alloc(ctx, src->n, dst_h, dst_w, false, out));
  std::vector<int32_t> xt, yt;
  axis_table(src->w, dst_w, true, xt);
  axis_table(src->h, dst_h, false, yt);
  ta_staging st;
  const size_t o_x = st.put(xt), o_y = st.put(yt);      // an xtab row is 16 bytes: ytab follows xtab without a gap
  TA_TRY(st.commit(ctx));
  const size_t total = (size_t)src->n * dst_h * dst_w;
  if (total) {
    ta_prof_scope scope(ctx, 2, (double)total * 3 * 5);
    size_t g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(resize_linear_kernel, dim3((int)g), dim3(256), 0, ctx->stream, src->dev, src->n, src->h, src->w,
                       (*out)->dev, dst_h, dst_w, st.dev<const int32_t>(o_x), st.dev<const int32_t>(o_y));
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned/scratch tables are reused by later calls
  return TA_OK;
}

int ta_frames_paste(ta_ctx* ctx, const ta_frames* src, int src_index, ta_frames* dst, int dst_index, int top, int left) {
  ta_enter(ctx);
  if (!ctx || !src || !dst || src_index < 0 || src_index >= src->n || dst_index < 0 || dst_index >= dst->n ||
      top < 0 || left < 0 || top + src->h > dst->h || left + src->w > dst->w)
    return ta_fail(ctx, TA_E_INVALID, "frames_paste: bad args");
  const size_t total = (size_t)src->h * src->w * 3;
  size_t g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(paste_kernel, dim3((int)g), dim3(256), 0, ctx->stream,
                     src->dev + (size_t)src_index * src->h * src->w * 3, src->h, src->w,
                     dst->dev + (size_t)dst_index * dst->h * dst->w * 3, dst->h, dst->w, top, left);
  TA_HIP(ctx, hipGetLastError());
  return TA_OK;
}

}  // extern "C"

int ta_frames_alloc_uninit(ta_ctx* ctx, int n, int h, int w, ta_frames** out) {
  ta_enter(ctx);
  return frames_alloc(ctx, n, h, w, false, out);
}
