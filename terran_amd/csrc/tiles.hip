// Cut many tiles out of many resident frames in ONE launch (ta_frames_tiles): tile i of the new batch (n, th, tw, 3) is
// src[frame, y : y + th, x : x + tw], byte for byte.  The front of tiled detection (terran_amd/tiles.py).
//
// A row of a tile is 3 tw bytes that start at byte 3 x of a frame row of 3 W bytes, and lands at byte (i th + r) 3 tw of
// the new batch: both sides sit at any byte alignment.  A wave takes one row of one tile and walks the 16-byte blocks of
// the DESTINATION that the row touches: a block that lies wholly inside the row is one aligned 16-byte store, put together
// in registers (v_alignbyte_b32) from the one or two aligned 16-byte blocks of the source that cover its bytes; the row's
// first and last block, when the row only covers a part of them, are written byte by byte by the lane that owns them
// (their other bytes belong to the neighbouring rows).  A covering source block holds a byte of the source batch, and a
// batch is allocated in multiples of 16 bytes at an aligned address (frames_alloc), so no load leaves the allocation;
// every store lies inside the row.  Consecutive lanes take consecutive blocks: a wave's loads and stores cover contiguous
// bytes.  All byte offsets are 64-bit (a batch of 1 024 tiles of 640 x 640 is 1.2 GB, 32 frames of 2160p are 0.8 GB).
#include "frame_regions.h"

namespace {

constexpr int TILE_THREADS = 256;          // four waves = four tile rows per workgroup

// the 16 bytes at `s`, of any alignment, out of the aligned 16-byte blocks that cover them
__device__ inline uint4 fetch16(const uint8_t* s) {
  const uint32_t mis = (uint32_t)(uintptr_t)s & 15u;
  const uint4* b = (const uint4*)(s - mis);
  const uint4 lo = b[0];
  uint4 hi = make_uint4(0u, 0u, 0u, 0u);
  if (mis) hi = b[1];                        // byte s + 15 lies in the second block exactly when s is not aligned
  const uint32_t k = mis >> 2, sh = mis & 3u;
  // dwords k .. k + 4 of lo | hi
  const uint32_t w0 = k == 0 ? lo.x : k == 1 ? lo.y : k == 2 ? lo.z : lo.w;
  const uint32_t w1 = k == 0 ? lo.y : k == 1 ? lo.z : k == 2 ? lo.w : hi.x;
  const uint32_t w2 = k == 0 ? lo.z : k == 1 ? lo.w : k == 2 ? hi.x : hi.y;
  const uint32_t w3 = k == 0 ? lo.w : k == 1 ? hi.x : k == 2 ? hi.y : hi.z;
  const uint32_t w4 = k == 0 ? hi.x : k == 1 ? hi.y : k == 2 ? hi.z : hi.w;
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                    __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// rows: n th tile rows, one per wave
__global__ __launch_bounds__(TILE_THREADS) void tiles_kernel(const uint8_t* __restrict__ src, int H, int W, const ta_tile* __restrict__ tiles, long long rows,
                                                             int th, int tw, uint8_t* __restrict__ dst) {
  const long long gr = (long long)blockIdx.x * (TILE_THREADS / 64) + (threadIdx.x >> 6);
  if (gr >= rows) return;
  const int lane = threadIdx.x & 63;
  const long long i = gr / th;
  const int r = (int)(gr - i * th);
  const ta_tile t = tiles[i];
  const size_t len = (size_t)3 * tw;
  const uint8_t* s = src + (((size_t)t.frame * H + (size_t)(t.y + r)) * W + (size_t)t.x) * 3;
  uint8_t* d = dst + (size_t)gr * len;
  const size_t head = (size_t)((uintptr_t)d & 15u);            // the row starts `head` bytes into its first block
  const size_t blocks = (head + len + 15) >> 4;
  for (size_t b = lane; b < blocks; b += 64) {
    const long long lo = (long long)(b << 4) - (long long)head;   // the block covers bytes lo .. lo + 15 of the row
    if (lo >= 0 && (size_t)lo + 16 <= len) {
      *(uint4*)(d + lo) = fetch16(s + lo);
    } else {
      const size_t a = lo < 0 ? 0 : (size_t)lo, e = (size_t)(lo + 16) < len ? (size_t)(lo + 16) : len;
      for (size_t k = a; k < e; ++k) d[k] = s[k];
    }
  }
}

}  // namespace

extern "C" int ta_frames_tiles(ta_ctx* ctx, const ta_frames* src, const ta_tile* tiles, int n, int th, int tw, ta_frames** out) {
  ta_enter(ctx);
  if (!ctx || !out) return ta_fail(ctx, TA_E_INVALID, "frames_tiles: bad args");
  *out = nullptr;
  TA_TRY(ta_check_batch(ctx, "frames_tiles", src, tiles, n));
  if (th <= 0 || tw <= 0) return ta_fail(ctx, TA_E_INVALID, "frames_tiles: a tile of %d x %d", tw, th);
  for (int i = 0; i < n; ++i) {
    const ta_tile& t = tiles[i];
    if (t.frame < 0 || t.frame >= src->n) return ta_fail(ctx, TA_E_INVALID, "frames_tiles: tile %d: frame %d out of range [0, %d)", i, t.frame, src->n);
    if (t.x < 0 || t.y < 0 || (long long)t.x + tw > src->w || (long long)t.y + th > src->h)
      return ta_fail(ctx, TA_E_INVALID, "frames_tiles: tile %d: %d x %d at (x %d, y %d) is not inside the %d x %d frame", i, tw, th, t.x, t.y, src->w, src->h);
  }
  if (n == 0) return TA_OK;
  const long long rows = (long long)n * th;
  const long long grid = (rows + TILE_THREADS / 64 - 1) / (TILE_THREADS / 64);
  if (grid > 0x7fffffffLL) return ta_fail(ctx, TA_E_OVERFLOW, "frames_tiles: %lld tile rows exceed the limit of %lld in one launch", rows, 0x7fffffffLL * (TILE_THREADS / 64));
  ta_staging st;
  const size_t o_tiles = st.put(tiles, (size_t)n * sizeof(ta_tile));
  TA_TRY(st.commit(ctx));
  ta_frames* f = nullptr;
  TA_TRY(ta_frames_alloc_uninit(ctx, n, th, tw, &f));
  {
    ta_prof_scope scope(ctx, 2, (double)rows * tw * 3 * 2);
    hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)grid), dim3(TILE_THREADS), 0, ctx->stream, (const uint8_t*)src->dev, src->h, src->w,
                       st.dev<const ta_tile>(o_tiles), rows, th, tw, f->dev);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);    // the staged tile list is reused by the next call
  if (e != hipSuccess) {
    ta_frames_free(f);
    return ta_fail(ctx, TA_E_DEVICE, "frames_tiles: %s", hipGetErrorString(e));
  }
  *out = f;
  return TA_OK;
}
