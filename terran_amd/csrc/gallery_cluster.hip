// Which rows of a gallery are the same person?  DBSCAN over the stored rows (ta_gallery_cluster), all of it on the device
// but the last renumbering.
//
//  edge      i ~ j  iff both rows are live and 1.0f - dot(row_i, row_j) < threshold (float32, ta_gallery_search's distance)
//  degree    number of j with i ~ j (the row itself counts); core iff degree >= min_samples
//  clusters  connected components of ~ among core rows, numbered by ascending smallest core row; a live non-core row with
//            a core neighbour joins the lowest-numbered cluster among its core neighbours'; everything else is -1
//
//  1. gallery_adj_kernel: the self-join.  One workgroup per upper-triangular pair (I, J >= I) of 128-row tiles (more pairs
//     than workgroups: a workgroup walks the list); dot on the exact-f32 MFMA as in gallery_scan_kernel (a wave's 32 rows
//     of tile I straight from global memory into registers, tile J's 128 rows staged through LDS in 64-float chunks, two
//     buffers, one barrier per chunk); every unordered pair of rows is decided ONCE, from one accumulator, and its bit is
//     written to both rows: block (I, J) row-major and block (J, I) transposed, and on a diagonal pair the upper triangle
//     (local row <= local column) is decided and mirrored.  The 128 x 128 bits of a pair are put together in LDS (one
//     writer per word: ballots for the row-major words, a lane's 16 accumulators plus the other half-wave's for the
//     transposed ones) and leave as one 16-byte store per row and block, so every word of the matrix has exactly one
//     writer in the whole grid: no atomics, no zeroing.  Rows >= size and removed rows get no bit on either side.
//  2. gallery_core_kernel: popcount per row -> degree, the core bit mask, label[i] = i for core rows.
//  3. gallery_propagate_kernel, one round: a wave per core row takes the smallest label among its core neighbours and its
//     own, follows l = label[l] a few times, and stores the result if it is smaller than what the row had.
//  4. gallery_border_kernel: a non-core row takes the smallest label among its core neighbours, or -1.
//
// Why the rounds end at the right answer, whatever the order of the waves.  Only row i's wave writes label[i], and only
// smaller values, so labels fall monotonically from label[i] = i; every value a row ever holds is a core row of its own
// component (it starts as itself, and takes either a neighbour's label or the label of a row that is in the component by
// the same argument), hence label[i] >= m(i), the smallest core row of i's component, and label[x] <= x always (which is
// why following l = label[l] can only go down).  A wave may read a label another wave is lowering in the same round, or an
// old copy of it from its cache: either value is one that row held, so both properties survive.  A round that stores
// nothing read only final values (nothing was written after the previous kernel ended), so label[i] <= label[j] over
// every edge, in both directions: labels are constant on a component, the constant c is a row of it with label[c] = c,
// and label[m] = m for the component's minimum forces c = m.  So the fixed point is unique.  A round that does store
// lowers at least one label, and without any luck in the order it does at least what a synchronous min-propagation
// round does, which needs at most size - 1 rounds: the host stops after the first silent round and gives up
// (TA_E_DEVICE) past size + 1 rounds.  Labels being component minima, "lowest-numbered cluster" is "smallest label".
//
// Compiled with -ffp-contract=off like gallery.hip (nothing here contracts: the dot is MFMA, the distance one subtraction).
#include <string.h>

#include <algorithm>

#include "gallery.h"
#include "gallery_cluster_host.h"

#define GAL_ADJ_LDB 68                 // floats per staged row of a chunk: 64 + 4, so that 16 rows' float4s cover all 64 banks
#define GAL_NOLABEL 0x7fffffff         // label of a row that is not core
#define GAL_ROUNDS_PER_READ 4          // propagation rounds launched per read of their flags
#define GAL_JUMPS 4                    // l = label[l] steps per round

// pair p of the list (0,0) (0,1) ... (0,nt-1) (1,1) ... : row I starts at s(I) = I nt - I (I - 1) / 2
__device__ __forceinline__ long long gal_pair_start(int i, int nt) { return (long long)i * nt - (long long)i * (i - 1) / 2; }
__device__ __forceinline__ void gal_pair(long long p, int nt, int& I, int& J) {
  const double b = 2.0 * nt + 1.0;
  int i = (int)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  i = i < 0 ? 0 : (i > nt - 1 ? nt - 1 : i);
  while (i + 1 < nt && gal_pair_start(i + 1, nt) <= p) ++i;
  while (i > 0 && gal_pair_start(i, nt) > p) --i;
  I = i;
  J = i + (int)(p - gal_pair_start(i, nt));
}

// adj: [ntiles * 128 rows][ntiles * 4 words of 32 bits], bit (j & 31) of word j >> 5 of row i = (i ~ j).
// rows / ids are allocated in whole tiles: every address of a tile is valid memory, rows >= nrows are masked out.
__global__ __launch_bounds__(256) void gallery_adj_kernel(const float* __restrict__ rows, const int32_t* __restrict__ ids, long long nrows, int ld, int ntiles,
                                                          long long npairs, float threshold, unsigned* __restrict__ adj) {
  extern __shared__ float4 gal_adj_smem[];
  float* bs = (float*)gal_adj_smem;                          // [2][GAL_T][GAL_ADJ_LDB]: tile J, one chunk per buffer
  unsigned* bits_rm = (unsigned*)(bs + 2 * GAL_T * GAL_ADJ_LDB);  // [GAL_T][4]: rows of I x columns of J
  unsigned* bits_tr = bits_rm + GAL_T * 4;                   // [GAL_T][4]: rows of J x columns of I
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nch = ld >> 6, ld4 = ld >> 2;
  const size_t w32 = (size_t)ntiles * 4;
  const float4* rows4 = (const float4*)rows;
  const int srow = tid >> 4, sc4 = tid & 15;                 // staging: float4 sc4 of rows srow + 16 q, q = 0..7, of a chunk

  long long p = blockIdx.x;
  if (p >= npairs) return;
  int I, J;
  gal_pair(p, ntiles, I, J);
  const float4* ap = rows4 + ((size_t)I * GAL_T + wave * 32 + r) * ld4 + h;
  const float4* bp = rows4 + ((size_t)J * GAL_T + srow) * ld4 + sc4;
  float4 a[8], bn[8];
  gal_load8(a, ap);
#pragma unroll
  for (int q = 0; q < 8; ++q) bn[q] = bp[(size_t)16 * q * ld4];
#pragma unroll
  for (int q = 0; q < 8; ++q) *(float4*)(bs + (srow + 16 * q) * GAL_ADJ_LDB + 4 * sc4) = bn[q];
  __syncthreads();
  int buf = 0;

  for (;;) {
    const long long pn = p + gridDim.x;
    const bool more = pn < npairs;
    int In = I, Jn = J;
    if (more) gal_pair(pn, ntiles, In, Jn);
    const float4* apn = rows4 + ((size_t)In * GAL_T + wave * 32 + r) * ld4 + h;
    const float4* bpn = rows4 + ((size_t)Jn * GAL_T + srow) * ld4 + sc4;
    gal_f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;

    for (int c = 0; c < nch; ++c) {
      // the next chunk of both tiles -- or the first chunk of the workgroup's next pair; behind the last pair, this pair's
      // first chunk once more, which nobody reads -- is in flight while this chunk's MFMAs run: the address is selected,
      // the loads are unconditional
      const bool last = c + 1 == nch;
      const float4* anp = last ? apn : ap + (c + 1) * 16;
      const float4* bnp = last ? bpn : bp + (c + 1) * 16;
      float4 an[8];
      gal_load8(an, anp);
#pragma unroll
      for (int q = 0; q < 8; ++q) bn[q] = bnp[(size_t)16 * q * ld4];
      // lane (r, h) holds k = 64 c + 8 j + 4 h + e of its row of I in a[j][e] and takes the same k of row 32 g + r of J from LDS
      const float* b = bs + buf * (GAL_T * GAL_ADJ_LDB);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 bv = *(const float4*)(b + (g * 32 + r) * GAL_ADJ_LDB + 8 * j + 4 * h);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, bv.x, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, bv.y, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, bv.z, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, bv.w, acc[g], 0, 0, 0);
        }
      }
      // the other buffer was last read one chunk ago, in front of the barrier every wave has passed since
      float* bw = bs + (buf ^ 1) * (GAL_T * GAL_ADJ_LDB);
#pragma unroll
      for (int q = 0; q < 8; ++q) *(float4*)(bw + (srow + 16 * q) * GAL_ADJ_LDB + 4 * sc4) = bn[q];
      __syncthreads();
      buf ^= 1;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = an[j];
    }

    // lane (r, h) holds, for row 32 g + r of J, rows 32 wave + 8 (i >> 2) + 4 h + (i & 3) of I, i = 0..15
    const bool diag = I == J;
    const long long rowI0 = (long long)I * GAL_T + wave * 32;
    int4 idv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) idv[i] = *(const int4*)(ids + rowI0 + 8 * i + 4 * h);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cj = g * 32 + r;
      const long long rowJ = (long long)J * GAL_T + cj;
      const bool liveJ = rowJ < nrows && ids[rowJ] >= 0;
      unsigned tm = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ri = wave * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
        const int4 iv = idv[i >> 2];
        const int id = (i & 3) == 0 ? iv.x : ((i & 3) == 1 ? iv.y : ((i & 3) == 2 ? iv.z : iv.w));
        bool e = liveJ && (long long)I * GAL_T + ri < nrows && id >= 0 && (1.0f - acc[g][i] < threshold);
        if (diag) e = e && ri <= cj;                      // the upper triangle decides; the transposed words mirror it
        const gal_u64 m = __ballot(e);                      // bits 0..31: row ri of the lanes with h = 0, 32..63: of those with h = 1
        if (r == 0) bits_rm[ri * 4 + g] = h ? (unsigned)(m >> 32) : (unsigned)m;
        tm |= e ? 1u << (ri & 31) : 0u;
      }
      tm |= (unsigned)__shfl_xor((int)tm, 32);              // the two half-waves hold disjoint rows of I for the same row of J
      if (h == 0) bits_tr[cj * 4 + wave] = tm;
    }
    __syncthreads();
    // (the next pair writes these words again behind at least one more barrier)
    if (tid < GAL_T) {
      uint4 v = *(const uint4*)(bits_rm + tid * 4);
      if (diag) {
        const uint4 t = *(const uint4*)(bits_tr + tid * 4);
        v.x |= t.x;
        v.y |= t.y;
        v.z |= t.z;
        v.w |= t.w;
      }
      *(uint4*)(adj + ((size_t)I * GAL_T + tid) * w32 + (size_t)J * 4) = v;
    } else if (!diag) {
      const int x = tid - GAL_T;
      *(uint4*)(adj + ((size_t)J * GAL_T + x) * w32 + (size_t)I * 4) = *(const uint4*)(bits_tr + x * 4);
    }
    if (!more) break;
    p = pn;
    I = In;
    J = Jn;
    ap = apn;
    bp = bpn;
  }
}

// One workgroup per 64 rows (a wave takes 16 of them, one after the other): degree, core bit, first label.
// adj: [gridDim.x * 64 rows][w64 words of 64 bits]; degree / label: nrows; core: gridDim.x words.
__global__ __launch_bounds__(256) void gallery_core_kernel(const gal_u64* __restrict__ adj, long long w64, long long nrows, int min_samples,
                                                           int32_t* __restrict__ degree, int32_t* __restrict__ label, gal_u64* __restrict__ core) {
  __shared__ int is_core[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = 0; k < 16; ++k) {
    const int lr = wave * 16 + k;
    const long long row = (long long)blockIdx.x * 64 + lr;
    const gal_u64* a = adj + (size_t)row * w64;
    int d = 0;
    for (long long w = lane; w < w64; w += 64) d += __popcll(a[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (lane == 0) {
      const bool c = row < nrows && d >= min_samples;
      is_core[lr] = c;
      if (row < nrows) {
        degree[row] = d;
        label[row] = c ? (int32_t)row : GAL_NOLABEL;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    const gal_u64 m = __ballot(is_core[lane] != 0);
    if (lane == 0) core[blockIdx.x] = m;
  }
}

// the smallest label among the core neighbours of `row` (GAL_NOLABEL: none), the same value in every lane
__device__ __forceinline__ int gal_min_core_label(const gal_u64* __restrict__ a, const gal_u64* __restrict__ core, long long w64, const int32_t* label, int lane) {
  int best = GAL_NOLABEL;
  for (long long w = lane; w < w64; w += 64) {
    gal_u64 m = a[w] & core[w];
    while (m) {
      const int bit = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int l = label[w * 64 + bit];
      best = l < best ? l : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int v = __shfl_xor(best, o);
    best = v < best ? v : best;
  }
  return best;
}

// One round, one wave per core row (see the header).  *changed is raised by every row that got a smaller label.
__global__ __launch_bounds__(256) void gallery_propagate_kernel(const gal_u64* __restrict__ adj, long long w64, long long nrows, const gal_u64* __restrict__ core,
                                                                int32_t* label, int* changed) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrows || !((core[row >> 6] >> (row & 63)) & 1)) return;
  const int own = label[row];
  int best = gal_min_core_label(adj + (size_t)row * w64, core, w64, label, lane);
  best = best < own ? best : own;
  for (int j = 0; j < GAL_JUMPS; ++j) best = label[best];   // label[x] <= x, and x is a core row: never GAL_NOLABEL
  if (best < own && lane == 0) {
    label[row] = best;
    *changed = 1;
  }
}

// One wave per row that is not core: the smallest label among its core neighbours, or -1
__global__ __launch_bounds__(256) void gallery_border_kernel(const gal_u64* __restrict__ adj, long long w64, long long nrows, const gal_u64* __restrict__ core,
                                                             int32_t* label) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrows || ((core[row >> 6] >> (row & 63)) & 1)) return;
  const int best = gal_min_core_label(adj + (size_t)row * w64, core, w64, label, lane);   // reads core rows' labels only; those are final
  if (lane == 0) label[row] = best == GAL_NOLABEL ? -1 : best;
}

namespace {
// the call's device memory: freed on every way out (hipFree waits for the device, so nothing still reads it)
struct gal_blocks {
  void* adj = nullptr;
  void* aux = nullptr;
  ~gal_blocks() {
    if (adj) (void)hipFree(adj);
    if (aux) (void)hipFree(aux);
  }
};
}  // namespace

extern "C" int ta_gallery_cluster(ta_gallery* g, float threshold, int min_samples, int32_t* labels_out, int32_t* degree_out, int32_t* n_clusters,
                                  int32_t* rounds) {
  ta_enter(g ? g->ctx : nullptr);
  if (!g) return TA_E_INVALID;
  ta_ctx* ctx = g->ctx;
  if (n_clusters) *n_clusters = 0;
  if (rounds) *rounds = 0;
  char msg[192];
  if (gal_cluster_check(threshold, min_samples, (long long)g->size, labels_out, msg, sizeof(msg))) return ta_fail(ctx, TA_E_INVALID, "%s", msg);
  if (g->size == 0) return TA_OK;

  const long long n = g->size;
  const int ntiles = (int)((n + GAL_T - 1) / GAL_T);
  const long long npairs = (long long)ntiles * (ntiles + 1) / 2;
  const long long w64 = (long long)ntiles * 2, padded = (long long)ntiles * GAL_T;
  const size_t adj_bytes = (size_t)padded * w64 * sizeof(gal_u64);
  const size_t lab_bytes = (size_t)padded * sizeof(int32_t), core_bytes = (size_t)w64 * sizeof(gal_u64);
  gal_blocks mem;
  hipError_t e = hipMalloc(&mem.adj, adj_bytes);
  if (e == hipSuccess) e = hipMalloc(&mem.aux, 2 * lab_bytes + core_bytes + 256);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return ta_fail(ctx, TA_E_DEVICE, "gallery: hipMalloc of the %zu-byte adjacency of %lld rows failed: %s", adj_bytes, n, hipGetErrorString(e));
  }
  int32_t* label = (int32_t*)mem.aux;
  int32_t* degree = (int32_t*)((char*)mem.aux + lab_bytes);
  gal_u64* core = (gal_u64*)((char*)mem.aux + 2 * lab_bytes);
  int* flags = (int*)((char*)mem.aux + 2 * lab_bytes + core_bytes);   // GAL_ROUNDS_PER_READ of them

  const size_t lds = (size_t)(2 * GAL_T * GAL_ADJ_LDB) * sizeof(float) + 2 * GAL_T * 4 * sizeof(unsigned);
  {
    const double flops = 2.0 * (double)npairs * GAL_T * GAL_T * g->ld;
    ta_prof_scope scope(ctx, 3, flops);
    ctx->cur_flops = flops;
    ctx->note_kernel("gallery_adj_kernel");
    TA_SET_LDS_ATTR(ctx, gallery_adj_kernel, lds);
    const unsigned grid = (unsigned)std::min<long long>(npairs, g->n_cu);   // 300 registers a lane: one workgroup per CU
    hipLaunchKernelGGL(gallery_adj_kernel, dim3(grid), dim3(256), lds, ctx->stream, (const float*)g->rows, (const int32_t*)g->ids, n, g->ld, ntiles, npairs, threshold,
                       (unsigned*)mem.adj);
    TA_HIP(ctx, hipGetLastError());
  }
  const unsigned row_blocks = (unsigned)((n + 3) / 4);
  ctx->cur_flops = 0;
  {
    ta_prof_scope scope(ctx, 3, (double)adj_bytes);
    ctx->note_kernel("gallery_core_kernel");
    hipLaunchKernelGGL(gallery_core_kernel, dim3((unsigned)w64), dim3(256), 0, ctx->stream, (const gal_u64*)mem.adj, w64, n, min_samples, degree, label, core);
    TA_HIP(ctx, hipGetLastError());
  }
  int total = 0;
  for (bool settled = false; !settled;) {
    if (total >= n + 1) return ta_fail(ctx, TA_E_DEVICE, "gallery: the labels of %lld rows did not settle within %lld rounds", n, n + 1);
    int changed[GAL_ROUNDS_PER_READ];
    {
      ta_prof_scope scope(ctx, 3, 0.0);
      ctx->note_kernel("gallery_propagate_kernel");
      TA_HIP(ctx, hipMemsetAsync(flags, 0, sizeof(changed), ctx->stream));
      for (int k = 0; k < GAL_ROUNDS_PER_READ; ++k) {
        hipLaunchKernelGGL(gallery_propagate_kernel, dim3(row_blocks), dim3(256), 0, ctx->stream, (const gal_u64*)mem.adj, w64, n, (const gal_u64*)core, label, flags + k);
        TA_HIP(ctx, hipGetLastError());
      }
    }
    TA_HIP(ctx, hipMemcpyAsync(changed, flags, sizeof(changed), hipMemcpyDeviceToHost, ctx->stream));
    TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < GAL_ROUNDS_PER_READ && !settled; ++k) {
      ++total;                                          // rounds up to and including the first that changed nothing
      settled = !changed[k];
    }
  }
  {
    ta_prof_scope scope(ctx, 3, 0.0);
    ctx->note_kernel("gallery_border_kernel");
    hipLaunchKernelGGL(gallery_border_kernel, dim3(row_blocks), dim3(256), 0, ctx->stream, (const gal_u64*)mem.adj, w64, n, (const gal_u64*)core, label);
    TA_HIP(ctx, hipGetLastError());
  }
  std::vector<int32_t> root((size_t)n);
  TA_HIP(ctx, hipMemcpyAsync(root.data(), label, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (degree_out) TA_HIP(ctx, hipMemcpyAsync(degree_out, degree, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long count = gal_renumber(root.data(), n, labels_out);
  if (count < 0) return ta_fail(ctx, TA_E_DEVICE, "gallery: the labels that came back are not component minima");
  if (n_clusters) *n_clusters = (int32_t)count;
  if (rounds) *rounds = total;
  return TA_OK;
}
