// A device-resident gallery of face embeddings with top-k cosine search (examples/match.py:38 asked of a watch-list).
//  * rows are stored L2-normalised (l2norm_kernel's arithmetic, arcface_post.hip) at a stride of `ld` = dim rounded up to
//    64 floats, the tail zero: the search needs no K edge and every row starts on a 256-byte line;
//  * one int32 id per row, id < 0 = removed;
//  * search pass 1 (gallery_scan_kernel) streams the rows once per group of up to 64 queries: dot(query, row) on the exact-f32
//    MFMA (32 rows x 32 queries x 2 k per instruction; A = rows straight from global memory into registers -- a wave owns its
//    32 rows, nothing to share --, B = the queries, resident in LDS for the whole pass), distance = 1 - dot, and per query
//    the k smallest keys (distance, row) a workgroup has seen over ALL its tiles;
//  * pass 2 (gallery_merge_kernel) merges the workgroups' lists per query by the same key.
// The key is a total order (rows are distinct), so the k smallest are one set whatever the tile size, the number of
// workgroups or the order in which waves offer their candidates: results are reproducible bit for bit.
// Compiled with -ffp-contract=off (the normalisation must round like l2norm_kernel; an MFMA is not contracted anyway).
#include <string.h>

#include <algorithm>

#include "gallery.h"

#define GAL_G 32     // queries per MFMA group (lib.py: GALLERY_QUERY_GROUP)
#define GAL_KMAX 16  // largest k
#define GAL_C 16     // candidate slots per query and selection round
#define GAL_LDQ_PAD 4

#define GAL_EMPTY 0xFFFFFFFFFFFFFFFFull

// float32 -> uint32 with the same order (and back)
__device__ __forceinline__ unsigned gal_ord(float d) {
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gal_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// c into the ascending list L (static indices only: L lives in registers); the largest element falls out
__device__ __forceinline__ void gal_insert(gal_u64 (&L)[GAL_KMAX], gal_u64 c) {
#pragma unroll
  for (int i = 0; i < GAL_KMAX; ++i) {
    const gal_u64 lo = c < L[i] ? c : L[i];
    c = c < L[i] ? L[i] : c;
    L[i] = lo;
  }
}
__device__ __forceinline__ gal_u64 gal_kth(const gal_u64 (&L)[GAL_KMAX], int k) {
  gal_u64 v = L[0];
#pragma unroll
  for (int i = 1; i < GAL_KMAX; ++i)
    if (i == k - 1) v = L[i];
  return v;
}

// l2norm_kernel with a row stride: one wavefront per row, a zero row stays zero
__global__ __launch_bounds__(256) void gallery_norm_kernel(float* x, long long n, int dim, int ld) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  float* r = x + (size_t)row * ld;
  float s = 0.f;
  for (int i = lane; i < dim; i += 64) s += r[i] * r[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  float nrm = sqrtf(s);
  if (nrm == 0.f) nrm = 1.f;
  for (int i = lane; i < dim; i += 64) r[i] = r[i] / nrm;
}

// rows whose id is in `sorted` (n ascending ids) become tombstones; *removed counts them
__global__ __launch_bounds__(256) void gallery_remove_kernel(int32_t* ids, long long nrows, const int32_t* sorted, int n, int* removed) {
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += (long long)gridDim.x * blockDim.x) {
    const int id = ids[row];
    if (id < 0) continue;
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo < n && sorted[lo] == id) {
      ids[row] = -1;
      atomicAdd(removed, 1);
    }
  }
}

// Pass 1.  NG = query groups of 32 a pass holds in LDS (2 while a row is at most 512 floats, else 1).
// lists: [gridDim.x][nq][k] keys, ascending, GAL_EMPTY where a workgroup saw fewer than k live rows.
// rows / ids are allocated in whole tiles: every address of a tile is valid memory, rows >= nrows are masked out.
template <int NG>
__global__ __launch_bounds__(256) void gallery_scan_kernel(const float* __restrict__ rows, const int32_t* __restrict__ ids, long long nrows, int ld,
                                                           const float* __restrict__ queries, int nq, int k, gal_u64* __restrict__ lists) {
  extern __shared__ float4 gal_smem[];
  const int ldq = ld + GAL_LDQ_PAD;
  float* qs = (float*)gal_smem;                                   // [NG * 32][ldq]
  gal_u64* cand = (gal_u64*)(qs + (size_t)NG * 32 * ldq);         // [NG * 32][GAL_C]
  gal_u64* thr = cand + NG * 32 * GAL_C;                          // [NG * 32]: the k-th smallest key so far
  unsigned* cnt = (unsigned*)(thr + NG * 32);                     // [NG * 32]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const long long ntiles = (nrows + GAL_T - 1) / GAL_T;
  const int nch = ld >> 6, ld4 = ld >> 2;
  const float4* rows4 = (const float4*)rows;
  const float4* q4 = (const float4*)queries;

  for (int q0 = 0; q0 < nq; q0 += NG * 32) {
    for (int i = tid; i < NG * 32 * ld4; i += 256) {
      const int q = i / ld4, c4 = i - q * ld4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q0 + q < nq) v = q4[(size_t)(q0 + q) * ld4 + c4];
      *(float4*)(qs + (size_t)q * ldq + 4 * c4) = v;
    }
    gal_u64 L[GAL_KMAX];
#pragma unroll
    for (int i = 0; i < GAL_KMAX; ++i) L[i] = GAL_EMPTY;
    gal_u64 Lk = GAL_EMPTY;
    if (tid < NG * 32) {
      thr[tid] = GAL_EMPTY;
      cnt[tid] = 0;
    }
    __syncthreads();

    float4 a[8];
    gal_load8(a, rows4 + ((size_t)blockIdx.x * GAL_T + wave * 32 + r) * ld4 + h);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const long long rowbase = tile * GAL_T + wave * 32;
      const float4* ap = rows4 + (size_t)(rowbase + r) * ld4 + h;
      const long long next_tile = tile + gridDim.x;
      gal_f32x16 acc[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
      for (int c = 0; c < nch; ++c) {
        // the next 64 floats of the row -- or the first 64 of this wave's rows in the workgroup's next tile -- are in flight
        // while this chunk's MFMAs run
        float4 an[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) an[j] = a[j];
        if (c + 1 < nch) gal_load8(an, ap + (c + 1) * 16);
        else if (next_tile < ntiles) gal_load8(an, rows4 + (size_t)(next_tile * GAL_T + wave * 32 + r) * ld4 + h);
        // lane (r, h) holds k = 64 c + 8 j + 4 h + e of row r in a[j][e]; the query operand takes the same k from LDS
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const float4 b = *(const float4*)(qs + (size_t)(g * 32 + r) * ldq + 64 * c + 8 * j + 4 * h);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, b.x, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, b.y, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, b.z, acc[g], 0, 0, 0);
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, b.w, acc[g], 0, 0, 0);
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = an[j];
      }

      // selection: lane (r, h) holds, for query g * 32 + r, rows rowbase + 8 (i >> 2) + 4 h + (i & 3), i = 0..15
      int4 idv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) idv[i] = *(const int4*)(ids + rowbase + 8 * i + 4 * h);
      unsigned pend = 0;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const gal_u64 t = thr[g * 32 + r];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const long long row = rowbase + 8 * (i >> 2) + 4 * h + (i & 3);
          const int4 iv = idv[i >> 2];
          const int id = (i & 3) == 0 ? iv.x : ((i & 3) == 1 ? iv.y : ((i & 3) == 2 ? iv.z : iv.w));
          const gal_u64 key = ((gal_u64)gal_ord(1.0f - acc[g][i]) << 32) | (unsigned)row;
          if (row < nrows && id >= 0 && key < t) pend |= 1u << (g * 16 + i);
        }
      }
      // rounds: every lane offers its pending candidates to the query's owner thread through GAL_C slots; what does not fit
      // waits for the next round and is measured against the owner's new k-th key first
      while (__syncthreads_or(pend != 0)) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if ((pend >> (g * 16)) & 0xffffu) {
            const int q = g * 32 + r;
            const gal_u64 t = thr[q];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const unsigned bit = 1u << (g * 16 + i);
              if (pend & bit) {
                const long long row = rowbase + 8 * (i >> 2) + 4 * h + (i & 3);
                const gal_u64 key = ((gal_u64)gal_ord(1.0f - acc[g][i]) << 32) | (unsigned)row;
                if (key < t) {
                  const unsigned slot = atomicAdd(&cnt[q], 1u);
                  if (slot < GAL_C) {
                    cand[q * GAL_C + slot] = key;
                    pend &= ~bit;
                  }
                } else {
                  pend &= ~bit;
                }
              }
            }
          }
        }
        __syncthreads();
        if (tid < NG * 32) {
          const unsigned n = cnt[tid] < GAL_C ? cnt[tid] : GAL_C;
          for (unsigned s = 0; s < n; ++s) {
            const gal_u64 c = cand[tid * GAL_C + s];
            if (c < Lk) {
              gal_insert(L, c);
              Lk = gal_kth(L, k);
            }
          }
          thr[tid] = Lk;
          cnt[tid] = 0;
        }
      }
    }
    if (tid < NG * 32 && q0 + tid < nq) {
      gal_u64* dst = lists + ((size_t)blockIdx.x * nq + q0 + tid) * k;
#pragma unroll
      for (int i = 0; i < GAL_KMAX; ++i)
        if (i < k) dst[i] = L[i];
    }
    __syncthreads();
  }
}

// Pass 2: one wavefront per query merges nlists lists of k keys and writes k results (row, id, distance)
__global__ __launch_bounds__(64) void gallery_merge_kernel(const gal_u64* __restrict__ lists, int nlists, int nq, int k, const int32_t* __restrict__ ids,
                                                           int32_t* out_row, int32_t* out_id, float* out_dist) {
  const int q = blockIdx.x, lane = threadIdx.x;
  gal_u64 L[GAL_KMAX];
#pragma unroll
  for (int i = 0; i < GAL_KMAX; ++i) L[i] = GAL_EMPTY;
  const long long total = (long long)nlists * k;
  for (long long i = lane; i < total; i += 64) {
    const long long l = i / k;
    const int e = (int)(i - l * k);
    const gal_u64 c = lists[((size_t)l * nq + q) * k + e];
    if (c < L[GAL_KMAX - 1]) gal_insert(L, c);
  }
  for (int j = 0; j < k; ++j) {
    gal_u64 m = L[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const gal_u64 v = __shfl_xor(m, o);
      m = v < m ? v : m;
    }
    if (m != GAL_EMPTY && L[0] == m) {               // keys are distinct (one row each): exactly one lane pops
#pragma unroll
      for (int i = 0; i + 1 < GAL_KMAX; ++i) L[i] = L[i + 1];
      L[GAL_KMAX - 1] = GAL_EMPTY;
    }
    if (lane == 0) {
      const size_t o = (size_t)q * k + j;
      if (m == GAL_EMPTY) {
        out_row[o] = -1;
        out_id[o] = -1;
        out_dist[o] = __uint_as_float(0x7f800000u);
      } else {
        const unsigned row = (unsigned)(m & 0xffffffffu);
        out_row[o] = (int32_t)row;
        out_id[o] = ids[row];
        out_dist[o] = gal_unord((unsigned)(m >> 32));
      }
    }
  }
}

static size_t gal_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// capacity of at least `want` rows (want <= INT32_MAX); the old rows move with a device copy on the context's stream
static int gal_reserve(ta_gallery* g, int64_t want) {
  ta_ctx* ctx = g->ctx;
  if (want <= g->cap) return TA_OK;
  int64_t cap = std::max<int64_t>(want, 2 * g->cap);
  cap = (int64_t)gal_up((size_t)std::max<int64_t>(cap, GAL_T), GAL_T);
  float* rows = nullptr;
  int32_t* ids = nullptr;
  const size_t row_bytes = (size_t)g->ld * sizeof(float);
  TA_HIP(ctx, hipMalloc(&rows, (size_t)cap * row_bytes));
  hipError_t e = hipMalloc(&ids, (size_t)cap * sizeof(int32_t));
  if (e != hipSuccess) {
    (void)hipFree(rows);
    return ta_fail(ctx, TA_E_DEVICE, "gallery: hipMalloc of %lld ids failed: %s", (long long)cap, hipGetErrorString(e));
  }
  e = hipMemsetAsync(rows, 0, (size_t)cap * row_bytes, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ids, 0xff, (size_t)cap * sizeof(int32_t), ctx->stream);
  if (e == hipSuccess && g->size) e = hipMemcpyAsync(rows, g->rows, (size_t)g->size * row_bytes, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess && g->size) e = hipMemcpyAsync(ids, g->ids, (size_t)g->size * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(rows);
    (void)hipFree(ids);
    return ta_fail(ctx, TA_E_DEVICE, "gallery: growing to %lld rows failed: %s", (long long)cap, hipGetErrorString(e));
  }
  if (g->rows) (void)hipFree(g->rows);
  if (g->ids) (void)hipFree(g->ids);
  g->rows = rows;
  g->ids = ids;
  g->cap = cap;
  return TA_OK;
}

// host rows (n, dim) -> device rows of stride ld (the tail of the destination is zero already and stays so)
static int gal_upload(ta_ctx* ctx, float* dst, int ld, const float* src, int dim, int64_t n) {
  if (ld == dim) TA_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  else TA_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)ld * sizeof(float), src, (size_t)dim * sizeof(float), (size_t)dim * sizeof(float), (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  return TA_OK;
}

extern "C" {

int ta_gallery_create(ta_ctx* ctx, int dim, int64_t reserve_rows, ta_gallery** out) {
  ta_enter(ctx);
  if (!ctx || !out) return TA_E_INVALID;
  *out = nullptr;
  if (dim < 1 || dim > 1024) return ta_fail(ctx, TA_E_INVALID, "gallery: dim %d is outside 1..1024", dim);
  if (reserve_rows < 0 || reserve_rows > INT32_MAX) return ta_fail(ctx, TA_E_INVALID, "gallery: cannot reserve %lld rows (0..2^31-1)", (long long)reserve_rows);
  ta_gallery* g = new ta_gallery();
  g->ctx = ctx;
  g->dim = dim;
  g->ld = (int)gal_up((size_t)dim, 64);
  g->cap = g->size = g->live = 0;
  g->rows = nullptr;
  g->ids = nullptr;
  g->n_cu = 0;
  if (hipDeviceGetAttribute(&g->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || g->n_cu < 1) g->n_cu = 256;
  if (reserve_rows) {
    const int rc = gal_reserve(g, reserve_rows);
    if (rc != TA_OK) {
      delete g;
      return rc;
    }
  }
  *out = g;
  return TA_OK;
}

void ta_gallery_free(ta_gallery* g) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return;
  (void)hipStreamSynchronize(g->ctx->stream);
  if (g->rows) (void)hipFree(g->rows);
  if (g->ids) (void)hipFree(g->ids);
  delete g;
}

int ta_gallery_add(ta_gallery* g, const float* rows, const int32_t* ids, int64_t n, int normalize) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  ta_ctx* ctx = g->ctx;
  if (n < 0) return ta_fail(ctx, TA_E_INVALID, "gallery: n < 0");
  if (n == 0) return TA_OK;
  if (!rows || !ids) return ta_fail(ctx, TA_E_INVALID, "gallery: null pointer");
  if (n > INT32_MAX || g->size + n > INT32_MAX) return ta_fail(ctx, TA_E_INVALID, "gallery: %lld + %lld rows exceed 2^31-1", (long long)g->size, (long long)n);
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0) return ta_fail(ctx, TA_E_INVALID, "gallery: ids[%lld] = %d is negative (negative ids mark removed rows)", (long long)i, ids[i]);
  TA_TRY(gal_reserve(g, g->size + n));
  float* dst = g->rows + (size_t)g->size * g->ld;
  TA_TRY(gal_upload(ctx, dst, g->ld, rows, g->dim, n));
  TA_HIP(ctx, hipMemcpyAsync(g->ids + g->size, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  if (normalize) {
    ta_prof_scope scope(ctx, 3, (double)n * g->dim * 8);
    hipLaunchKernelGGL(gallery_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, dst, (long long)n, g->dim, g->ld);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  g->size += n;
  g->live += n;
  return TA_OK;
}

int ta_gallery_remove(ta_gallery* g, const int32_t* ids, int n, int64_t* removed) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  ta_ctx* ctx = g->ctx;
  if (removed) *removed = 0;
  if (n < 0) return ta_fail(ctx, TA_E_INVALID, "gallery: n < 0");
  if (n == 0 || g->size == 0) return TA_OK;
  if (!ids) return ta_fail(ctx, TA_E_INVALID, "gallery: null pointer");
  std::vector<int32_t> sorted(ids, ids + n);
  std::sort(sorted.begin(), sorted.end());
  char* scr = nullptr;
  TA_TRY(ta_scratch(ctx, 256 + (size_t)n * sizeof(int32_t), (void**)&scr));
  int count = 0;
  TA_HIP(ctx, hipMemsetAsync(scr, 0, 256, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(scr + 256, sorted.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  const unsigned blocks = (unsigned)std::min<int64_t>((g->size + 255) / 256, 8192);
  hipLaunchKernelGGL(gallery_remove_kernel, dim3(blocks), dim3(256), 0, ctx->stream, g->ids, (long long)g->size, (const int32_t*)(scr + 256), n, (int*)scr);
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipMemcpyAsync(&count, scr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  g->live -= count;
  if (removed) *removed = count;
  return TA_OK;
}

int ta_gallery_clear(ta_gallery* g) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  g->size = g->live = 0;                              // the buffers stay; only columns [0, dim) are ever written, the tail stays zero
  return TA_OK;
}

int ta_gallery_size(const ta_gallery* g, int64_t* rows, int64_t* live) {
  if (!g) return TA_E_INVALID;
  if (rows) *rows = g->size;
  if (live) *live = g->live;
  return TA_OK;
}

int ta_gallery_download(const ta_gallery* g, float* rows_out, int32_t* ids_out) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  ta_ctx* ctx = g->ctx;
  if (g->size == 0) return TA_OK;
  if (!rows_out || !ids_out) return ta_fail(ctx, TA_E_INVALID, "gallery: null pointer");
  if (g->ld == g->dim) TA_HIP(ctx, hipMemcpyAsync(rows_out, g->rows, (size_t)g->size * g->dim * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  else TA_HIP(ctx, hipMemcpy2DAsync(rows_out, (size_t)g->dim * sizeof(float), g->rows, (size_t)g->ld * sizeof(float), (size_t)g->dim * sizeof(float), (size_t)g->size, hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(ids_out, g->ids, (size_t)g->size * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}

int ta_gallery_search(ta_gallery* g, const float* queries, int nq, int k, int normalize, int32_t* out_row, int32_t* out_id, float* out_dist) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  ta_ctx* ctx = g->ctx;
  if (nq < 0) return ta_fail(ctx, TA_E_INVALID, "gallery: nq < 0");
  if (k < 1 || k > GAL_KMAX) return ta_fail(ctx, TA_E_INVALID, "gallery: k = %d is outside 1..%d", k, GAL_KMAX);
  if (nq == 0) return TA_OK;
  if (!queries || !out_row || !out_id || !out_dist) return ta_fail(ctx, TA_E_INVALID, "gallery: null pointer");
  const size_t nres = (size_t)nq * k;
  if (g->size == 0) {                                 // nothing to search: every slot is padding, no device work
    for (size_t i = 0; i < nres; ++i) {
      out_row[i] = -1;
      out_id[i] = -1;
      out_dist[i] = HUGE_VALF;
    }
    return TA_OK;
  }
  const int64_t ntiles = (g->size + GAL_T - 1) / GAL_T;
  const int nwg = (int)std::min<int64_t>(ntiles, g->n_cu);
  const int ng = g->ld <= 512 ? 2 : 1;
  const size_t q_bytes = gal_up((size_t)nq * g->ld * sizeof(float), 256);
  const size_t list_bytes = gal_up((size_t)nwg * nres * sizeof(gal_u64), 256);
  const size_t res_bytes = gal_up(nres * sizeof(int32_t), 256);
  char* scr = nullptr;
  TA_TRY(ta_scratch(ctx, q_bytes + list_bytes + 3 * res_bytes, (void**)&scr));
  float* q_dev = (float*)scr;
  gal_u64* lists = (gal_u64*)(scr + q_bytes);
  int32_t* row_dev = (int32_t*)(scr + q_bytes + list_bytes);
  int32_t* id_dev = (int32_t*)(scr + q_bytes + list_bytes + res_bytes);
  float* dist_dev = (float*)(scr + q_bytes + list_bytes + 2 * res_bytes);
  if (g->ld != g->dim) TA_HIP(ctx, hipMemsetAsync(q_dev, 0, (size_t)nq * g->ld * sizeof(float), ctx->stream));
  TA_TRY(gal_upload(ctx, q_dev, g->ld, queries, g->dim, nq));
  if (normalize) {
    hipLaunchKernelGGL(gallery_norm_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, q_dev, (long long)nq, g->dim, g->ld);
    TA_HIP(ctx, hipGetLastError());
  }
  // LDS of a pass: the queries, the candidate slots, the k-th keys and the slot counters; the most either instance can ask for
  // (2 groups of 512 floats, 1 group of 1024) is what its attribute is set to, once
  auto lds_of = [](int groups, int ld) { return (size_t)groups * 32 * ((size_t)(ld + GAL_LDQ_PAD) * sizeof(float) + GAL_C * sizeof(gal_u64) + sizeof(gal_u64) + sizeof(unsigned)); };
  const size_t lds = lds_of(ng, g->ld);
  {
    ta_prof_scope scope(ctx, 3, 2.0 * (double)g->size * nq * g->dim);
    if (ng == 2) {
      TA_SET_LDS_ATTR(ctx, gallery_scan_kernel<2>, lds_of(2, 512));
      hipLaunchKernelGGL(gallery_scan_kernel<2>, dim3(nwg), dim3(256), lds, ctx->stream, (const float*)g->rows, (const int32_t*)g->ids, (long long)g->size, g->ld,
                         (const float*)q_dev, nq, k, lists);
    } else {
      TA_SET_LDS_ATTR(ctx, gallery_scan_kernel<1>, lds_of(1, 1024));
      hipLaunchKernelGGL(gallery_scan_kernel<1>, dim3(nwg), dim3(256), lds, ctx->stream, (const float*)g->rows, (const int32_t*)g->ids, (long long)g->size, g->ld,
                         (const float*)q_dev, nq, k, lists);
    }
    TA_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(nq), dim3(64), 0, ctx->stream, (const gal_u64*)lists, nwg, nq, k, (const int32_t*)g->ids, row_dev, id_dev, dist_dev);
    TA_HIP(ctx, hipGetLastError());
  }
  TA_HIP(ctx, hipMemcpyAsync(out_row, row_dev, nres * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_id, id_dev, nres * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipMemcpyAsync(out_dist, dist_dev, nres * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TA_OK;
}

}  // extern "C"
