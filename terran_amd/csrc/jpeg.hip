// Baseline JPEG, device half: dequantisation + 8x8 inverse DCT (libjpeg's JDCT_ISLOW, jidctint.c's arithmetic and
// range-limit table) over every block of every image of a call in ONE launch, then fancy upsampling + YCbCr -> RGB
// (jdsample.c / jdcolor.c arithmetic) into the resident uint8 NHWC frames in one more.  Pure integer code: the result
// equals libjpeg-turbo's default decode bit for bit (tests/jpeg_model.py restates it, tests/test_jpeg_cpu.py pins that
// against Pillow).  The host half -- markers and Huffman -- is jpeg_host.hip.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>

#include "jpeg.h"
#include "ta_internal.h"

namespace {

// one component plane of one image (the IDCT kernel): its blocks are blocks [block0, next plane's block0) of the call
struct jd_plane {
  int64_t block0;
  int64_t plane_off;     // bytes into the plane buffer
  int32_t bw;            // blocks per row
  int32_t stride;        // bytes per plane row (8 bw)
  int32_t qt;            // quantisation table (row of the call's table array)
  int32_t pad_;
};

// one image (the colour kernel); ncomp == 0: a fallback image, written as zeros
struct jd_image {
  int64_t plane_off[3];
  int32_t stride[3], dw[3], dh[3], rh[3], rv[3];
  int32_t ncomp, pad_;
};

// one output batch: images [image0, image0 + n) of h x w; its pixels in groups of 4 are groups [group0, ...) of the call
struct jd_output {
  uint8_t* dst;
  int64_t group0;
  int32_t n, h, w, image0;
};

static_assert(sizeof(jd_plane) == 32 && sizeof(jd_image) == 96 && sizeof(jd_output) == 32, "descriptor layout");

#define JD_BLOCKS_PER_WG 32                 // 256 threads: 8 lanes per block, 8 blocks per wave
#define JD_LDS_STRIDE 72                    // ints per block in LDS: column reads of the 8 blocks of a wave hit 64 banks

// jidctint.c constants (CONST_BITS = 13)
#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// One 1-D islow IDCT of 8 values in T (int or int64_t); `shift` is the pass's descale (11, then 18).  In place; the
// results are stored as int, as jidctint.c stores its workspace and takes its range-limit index.
template <typename T>
__device__ __forceinline__ void idct8(int v[8], int shift) {
  T z2 = v[2], z3 = v[6];
  T z1 = (z2 + z3) * FIX_0_541196100;
  T tmp2 = z1 - z3 * FIX_1_847759065;
  T tmp3 = z1 + z2 * FIX_0_765366865;
  z2 = v[0];
  z3 = v[4];
  T tmp0 = (z2 + z3) * 8192;
  T tmp1 = (z2 - z3) * 8192;
  const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = v[7];
  tmp1 = v[5];
  tmp2 = v[3];
  tmp3 = v[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  T z4 = tmp1 + tmp3;
  const T z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 = z3 * -FIX_1_961570560 + z5;
  z4 = z4 * -FIX_0_390180644 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const T r = (T)1 << (shift - 1);
  v[0] = (int)((tmp10 + tmp3 + r) >> shift);
  v[7] = (int)((tmp10 - tmp3 + r) >> shift);
  v[1] = (int)((tmp11 + tmp2 + r) >> shift);
  v[6] = (int)((tmp11 - tmp2 + r) >> shift);
  v[2] = (int)((tmp12 + tmp1 + r) >> shift);
  v[5] = (int)((tmp12 - tmp1 + r) >> shift);
  v[3] = (int)((tmp13 + tmp0 + r) >> shift);
  v[4] = (int)((tmp13 - tmp0 + r) >> shift);
}

// Every sum and product of idct8 stays below 61214 x max|input| + 2^17 (the largest row L1 norm of the integer
// transform): up to this input magnitude 32-bit arithmetic cannot overflow, and it is the only path real 8-bit images
// take.  Larger inputs -- crafted coefficients, 16-bit quantisation tables -- take the 64-bit path of jidctint.c's C code.
#define JD_NARROW_MAX 35000u

__device__ __forceinline__ void idct8_exact(int v[8], int shift) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) m = max(m, v[k] < 0 ? 0u - (uint32_t)v[k] : (uint32_t)v[k]);
  if (m <= JD_NARROW_MAX) idct8<int>(v, shift);
  else idct8<int64_t>(v, shift);
}

// libjpeg's IDCT range limit: x & 1023 -> [0,127] x + 128, [128,511] 255, [512,895] 0, [896,1023] x - 896
__device__ __forceinline__ uint32_t range_limit(int x) {
  x &= 1023;
  return x < 128 ? x + 128 : (x < 512 ? 255 : (x < 896 ? 0 : x - 896));
}

// Kernel A.  Thread t of a workgroup: block t / 8 of the workgroup's 32, lane j = t % 8.  It loads row j of its block's
// coefficients (one 16-byte load: the workgroup reads 4 KB contiguously) and row j of the block's quantisation table,
// dequantises into LDS, runs the column pass on column j, then the row pass on row j, and stores that row's 8 samples
// as one 8-byte store into the component plane.
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t* __restrict__ coefs, int64_t n_blocks,
                                                        const jd_plane* __restrict__ planes, int n_planes,
                                                        const uint16_t* __restrict__ quant, uint8_t* __restrict__ out) {
  __shared__ int ws[JD_BLOCKS_PER_WG * JD_LDS_STRIDE];
  const int t = threadIdx.x, lb = t >> 3, j = t & 7;
  const int64_t blk = (int64_t)blockIdx.x * JD_BLOCKS_PER_WG + lb;
  const bool live = blk < n_blocks;
  int* w = ws + lb * JD_LDS_STRIDE;
  jd_plane pl = {};
  if (live) {
    int lo = 0, hi = n_planes - 1;                 // last plane with block0 <= blk
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (planes[mid].block0 <= blk) lo = mid;
      else hi = mid - 1;
    }
    pl = planes[lo];
    const int4 c = *reinterpret_cast<const int4*>(coefs + blk * 64 + j * 8);
    const int4 q = *reinterpret_cast<const int4*>(quant + (int64_t)pl.qt * 64 + j * 8);
    const int cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // libjpeg keeps its dequantisation table as 16-bit signed multipliers: the product always fits in 32 bits
      w[j * 8 + 2 * k] = (int)(int16_t)(cw[k] & 0xFFFF) * (int)(int16_t)(qw[k] & 0xFFFF);
      w[j * 8 + 2 * k + 1] = (int)(int16_t)((uint32_t)cw[k] >> 16) * (int)(int16_t)((uint32_t)qw[k] >> 16);
    }
  }
  __syncthreads();
  if (live) {
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = w[k * 8 + j];
    idct8_exact(v, 11);                                  // pass 1: CONST_BITS - PASS1_BITS
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k * 8 + j] = v[k];
  }
  __syncthreads();
  if (live) {
    int v[8];
    const int4 a = *reinterpret_cast<const int4*>(w + j * 8), b = *reinterpret_cast<const int4*>(w + j * 8 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    idct8_exact(v, 18);                                  // pass 2: CONST_BITS + PASS1_BITS + 3
    const int64_t local = blk - pl.block0;
    const int64_t by = local / pl.bw, bx = local - by * pl.bw;
    uint2 o;
    o.x = range_limit(v[0]) | range_limit(v[1]) << 8 | range_limit(v[2]) << 16 | range_limit(v[3]) << 24;
    o.y = range_limit(v[4]) | range_limit(v[5]) << 8 | range_limit(v[6]) << 16 | range_limit(v[7]) << 24;
    *reinterpret_cast<uint2*>(out + pl.plane_off + (by * 8 + j) * pl.stride + bx * 8) = o;
  }
}

// jdsample.c: fancy upsampling by the component's ratio (rh, rv) in {1, 2}^2, over the real downsampled size dw x dh
// (edge samples replicated); h2v1 / h2v2 fall back to box replication when dw <= 2, as libjpeg does.
__device__ __forceinline__ int upsample(const uint8_t* __restrict__ p, int stride, int dw, int dh, int rh, int rv, int y,
                                        int x) {
  if (rv == 1) {
    const uint8_t* row = p + (int64_t)y * stride;
    if (rh == 1) return row[x];
    const int i = x >> 1;
    if (dw <= 2) return row[i];
    return (x & 1) ? (3 * row[i] + row[min(i + 1, dw - 1)] + 2) >> 2 : (3 * row[i] + row[max(i - 1, 0)] + 1) >> 2;
  }
  const int r = y >> 1, nb = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);
  const uint8_t* a = p + (int64_t)r * stride;
  const uint8_t* b = p + (int64_t)nb * stride;
  if (rh == 1) return (3 * a[x] + b[x] + ((y & 1) ? 2 : 1)) >> 2;
  const int i = x >> 1;
  if (dw <= 2) return a[i];
  const int k = (x & 1) ? min(i + 1, dw - 1) : max(i - 1, 0);
  return (3 * (3 * a[i] + b[i]) + (3 * a[k] + b[k]) + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

// Kernel B.  One thread per 4 consecutive pixels of an output batch (12 bytes: three dword stores, bytes near the
// batch's end stored one by one).
__global__ void __launch_bounds__(256) jpeg_color_kernel(const uint8_t* __restrict__ planes, const jd_image* __restrict__ images,
                                                         const jd_output* __restrict__ outputs, int n_outputs,
                                                         int64_t n_groups) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  int lo = 0, hi = n_outputs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (outputs[mid].group0 <= g) lo = mid;
    else hi = mid - 1;
  }
  const jd_output o = outputs[lo];
  const int64_t hw = (int64_t)o.h * o.w, pixels = o.n * hw, p0 = (g - o.group0) * 4;
  uint32_t px[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    const int64_t q = p0 + k;
    if (q >= pixels) break;
    const int64_t img = q / hw, rem = q - img * hw;
    const int y = (int)(rem / o.w), x = (int)(rem - (int64_t)y * o.w);
    const jd_image& d = images[o.image0 + img];
    if (d.ncomp == 0) continue;
    const int Y = upsample(planes + d.plane_off[0], d.stride[0], d.dw[0], d.dh[0], d.rh[0], d.rv[0], y, x);
    if (d.ncomp == 1) {
      px[k] = Y * 0x010101u;
      continue;
    }
    const int cb = upsample(planes + d.plane_off[1], d.stride[1], d.dw[1], d.dh[1], d.rh[1], d.rv[1], y, x) - 128;
    const int cr = upsample(planes + d.plane_off[2], d.stride[2], d.dw[2], d.dh[2], d.rh[2], d.rv[2], y, x) - 128;
    // jdcolor.c, SCALEBITS = 16: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414)
    const uint32_t R = clamp255(Y + ((91881 * cr + 32768) >> 16));
    const uint32_t G = clamp255(Y + ((-46802 * cr - 22554 * cb + 32768) >> 16));
    const uint32_t B = clamp255(Y + ((116130 * cb + 32768) >> 16));
    px[k] = R | G << 8 | B << 16;
  }
  const uint32_t wd[3] = {px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8};
  const int64_t bytes = pixels * 3, b0 = p0 * 3;
  for (int k = 0; k < 3; ++k) {
    const int64_t at = b0 + 4 * k;
    if (at + 4 <= bytes) {
      *reinterpret_cast<uint32_t*>(o.dst + at) = wd[k];
    } else {
      for (int i = 0; i < 4 && at + i < bytes; ++i) o.dst[at + i] = (uint8_t)(wd[k] >> (8 * i));
    }
  }
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" int ta_jpeg_decode(ta_ctx* ctx, const uint8_t* const* data, const size_t* sizes, int n, int threads, int capacity,
                              ta_frames** out, int32_t* paths, int32_t* required) {
  if (!ctx) return TA_E_INVALID;
  ta_enter(ctx);
  if (n <= 0 || !data || !sizes || !out || !paths || !required || threads < 0)
    return ta_fail(ctx, TA_E_INVALID, "jpeg_decode: bad arguments");
  const auto t_host = std::chrono::steady_clock::now();
  // 1. markers of every image: sizes, paths, the call's layout -- before anything touches the GPU
  std::vector<std::unique_ptr<ta_jpeg_parsed>> parsed(n);
  std::vector<std::string> errs(n);
  int first_bad = -1;
  for (int i = 0; i < n; ++i) {
    parsed[i].reset(new ta_jpeg_parsed());
    if (!data[i]) errs[i] = "null data";
    if (!data[i] || ta_jpeg_parse(data[i], sizes[i], parsed[i].get(), &errs[i]) != TA_OK) {
      paths[i] = TA_JPEG_INVALID;
      if (first_bad < 0) first_bad = i;
      continue;
    }
    paths[i] = parsed[i]->hdr.path;
  }
  // with a malformed image the call fails, but only after the Huffman pass over the others, so that `paths` names
  // every malformed image
  bool same = true;
  for (int i = 1; i < n; ++i)
    same = same && parsed[i]->hdr.width == parsed[0]->hdr.width && parsed[i]->hdr.height == parsed[0]->hdr.height;
  *required = same ? 1 : n;
  if (first_bad < 0 && capacity < *required)
    return ta_fail(ctx, TA_E_CAPACITY, "jpeg_decode: %d output batches needed", *required);

  std::vector<jd_plane> planes;
  std::vector<jd_image> images(n);
  std::vector<jd_output> outputs;
  std::vector<int> dev_images;                                    // images decoded here, in call order
  std::vector<int64_t> coef_block0(n, 0);                         // first block of image i in the call's coefficients
  int64_t blocks = 0, plane_bytes = 0;
  for (int i = 0; i < n; ++i) {
    memset(&images[i], 0, sizeof(jd_image));
    const ta_jpeg_parsed& p = *parsed[i];
    if (paths[i] != TA_JPEG_DEVICE) continue;                     // fallback, or malformed (TA_JPEG_INVALID)
    const int qbase = 4 * (int)dev_images.size();
    dev_images.push_back(i);
    coef_block0[i] = blocks;
    jd_image& d = images[i];
    d.ncomp = p.hdr.components;
    for (int c = 0; c < p.hdr.components; ++c) {
      const int hs = p.hdr.h_samp[c], vs = p.hdr.v_samp[c];
      jd_plane pl = {};
      pl.block0 = blocks + p.hdr.block_offset[c];
      pl.plane_off = plane_bytes;
      pl.bw = p.hdr.blocks_w[c];
      pl.stride = 8 * pl.bw;
      pl.qt = qbase + p.hdr.quant_index[c];
      planes.push_back(pl);
      d.plane_off[c] = plane_bytes;
      d.stride[c] = pl.stride;
      d.dw[c] = (int)(((int64_t)p.hdr.width * hs + p.hmax - 1) / p.hmax);
      d.dh[c] = (int)(((int64_t)p.hdr.height * vs + p.vmax - 1) / p.vmax);
      d.rh[c] = p.hmax / hs;
      d.rv[c] = p.vmax / vs;
      plane_bytes = align_up(plane_bytes + (int64_t)p.hdr.blocks_h[c] * 8 * pl.stride, 256);
    }
    blocks += p.hdr.blocks_total;
  }
  int64_t groups = 0;
  for (int i = 0; i < (same ? 1 : n); ++i) {
    jd_output o = {};
    o.group0 = groups;
    o.n = same ? n : 1;
    o.h = parsed[i]->hdr.height;
    o.w = parsed[i]->hdr.width;
    o.image0 = i;
    groups += ((int64_t)o.n * o.h * o.w + 3) / 4;
    outputs.push_back(o);
  }
  // staging (pinned) and its device copy: [coefficients][quant tables][planes][images][outputs]; then the sample planes
  const int64_t off_quant = align_up(blocks * 128, 256);
  const int64_t off_planes = align_up(off_quant + (int64_t)dev_images.size() * 4 * 64 * 2, 256);
  const int64_t off_images = align_up(off_planes + (int64_t)planes.size() * (int64_t)sizeof(jd_plane), 256);
  const int64_t off_outputs = align_up(off_images + (int64_t)n * (int64_t)sizeof(jd_image), 256);
  const int64_t staged = align_up(off_outputs + (int64_t)outputs.size() * (int64_t)sizeof(jd_output), 256);
  void* pin = nullptr;
  TA_TRY(ta_pinned(ctx, (size_t)staged, &pin));
  uint8_t* host = (uint8_t*)pin;

  // 2. Huffman streams on up to 16 host threads, straight into the staging
  const int n_dev = (int)dev_images.size();
  int nt = threads ? threads : std::min(n_dev, 16);
  nt = std::max(1, std::min(std::min(nt, 16), std::max(n_dev, 1)));
  std::atomic<int> next{0};
  auto work = [&]() {
    for (int k; (k = next.fetch_add(1)) < n_dev;) {
      const int i = dev_images[k];                              // every image has its own paths / errs slot
      if (ta_jpeg_entropy_decode(parsed[i].get(), (int16_t*)(host + coef_block0[i] * 128), &errs[i]) != TA_OK)
        paths[i] = TA_JPEG_INVALID;
    }
  };
  if (nt <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (int k = 0; k < nt; ++k) pool.emplace_back(work);
    for (auto& th : pool) th.join();
  }
  for (int i = 0; i < n; ++i)
    if (paths[i] == TA_JPEG_INVALID) return ta_fail(ctx, TA_E_INVALID, "jpeg_decode: image %d: %s", i, errs[i].c_str());
  for (int k = 0; k < n_dev; ++k)
    memcpy(host + off_quant + (int64_t)k * 512, parsed[dev_images[k]]->hdr.quant, 512);
  if (!planes.empty()) memcpy(host + off_planes, planes.data(), planes.size() * sizeof(jd_plane));
  memcpy(host + off_images, images.data(), images.size() * sizeof(jd_image));
  const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();

  // 3. outputs, device scratch, one copy, two launches
  std::vector<ta_frames*> frames;
  auto release = [&](int rc) {
    for (ta_frames* f : frames) ta_frames_free(f);
    return rc;
  };
  for (jd_output& o : outputs) {
    ta_frames* f = nullptr;
    int rc = ta_frames_alloc_uninit(ctx, o.n, o.h, o.w, &f);
    if (rc != TA_OK) return release(rc);
    frames.push_back(f);
    o.dst = f->dev;
  }
  memcpy(host + off_outputs, outputs.data(), outputs.size() * sizeof(jd_output));
  void* scr = nullptr;
  int rc = ta_scratch(ctx, (size_t)(staged + plane_bytes), &scr);
  if (rc != TA_OK) return release(rc);
  uint8_t* dev = (uint8_t*)scr;
  hipEvent_t ev[5] = {};
  const bool timed = ctx->profiling;
  if (timed)
    for (auto& e : ev)
      if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  auto mark = [&](int k) {
    if (timed && ev[k]) (void)hipEventRecord(ev[k], ctx->stream);
  };
  mark(0);
  hipError_t e = hipMemcpyAsync(dev, host, (size_t)staged, hipMemcpyHostToDevice, ctx->stream);
  mark(1);
  if (e == hipSuccess && blocks > 0) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + JD_BLOCKS_PER_WG - 1) / JD_BLOCKS_PER_WG)), dim3(256), 0,
                       ctx->stream, (const int16_t*)dev, blocks, (const jd_plane*)(dev + off_planes), (int)planes.size(),
                       (const uint16_t*)(dev + off_quant), dev + staged);
    e = hipGetLastError();
  }
  mark(2);
  if (e == hipSuccess && groups > 0) {
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, ctx->stream, dev + staged,
                       (const jd_image*)(dev + off_images), (const jd_output*)(dev + off_outputs), (int)outputs.size(),
                       groups);
    e = hipGetLastError();
  }
  mark(3);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging is reused by the next call
  double ms[4] = {host_ms, 0, 0, 0};
  if (timed) {
    for (int k = 0; k < 3; ++k) {
      float f = 0;
      if (ev[k] && ev[k + 1] && hipEventElapsedTime(&f, ev[k], ev[k + 1]) == hipSuccess) ms[k + 1] = f;
    }
    for (auto& x : ev)
      if (x) (void)hipEventDestroy(x);
  }
  if (e != hipSuccess) return release(ta_fail(ctx, TA_E_DEVICE, "jpeg_decode: %s", hipGetErrorString(e)));
  memcpy(ctx->jpeg_ms, ms, sizeof(ms));
  ctx->jpeg_counts[0] = n_dev;
  ctx->jpeg_counts[1] = blocks;
  ctx->jpeg_counts[2] = staged;
  ctx->jpeg_counts[3] = n - n_dev;
  for (size_t k = 0; k < frames.size(); ++k) out[k] = frames[k];
  return TA_OK;
}

extern "C" int ta_jpeg_last_stats(const ta_ctx* ctx, double* ms, int64_t* counts) {
  if (!ctx) return TA_E_INVALID;
  if (ms) memcpy(ms, ctx->jpeg_ms, sizeof(ctx->jpeg_ms));
  if (counts) memcpy(counts, ctx->jpeg_counts, sizeof(ctx->jpeg_counts));
  return TA_OK;
}
