// What gallery.hip (storage, search) and gallery_cluster.hip (self-join, clustering) share: the gallery itself and the
// register layout of a row operand of the exact-f32 MFMA.
#pragma once
#include "ta_internal.h"

#define GAL_T 128    // rows per tile: 4 waves x 32 (lib.py: GALLERY_ROW_TILE)

typedef float gal_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long gal_u64;

struct ta_gallery {
  ta_ctx* ctx;
  int dim, ld;            // ld: floats per stored row (dim rounded up to 64)
  int64_t cap, size, live;  // rows allocated (a multiple of GAL_T) / used (tombstones included) / used and not removed
  float* rows;
  int32_t* ids;
  int n_cu;
};

// 64 floats of a row for lane (r, h) = (lane & 31, lane >> 5): a[j][e] = float 8 j + 4 h + e, p = the row's float4s + h
__device__ __forceinline__ void gal_load8(float4 (&a)[8], const float4* p) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = p[2 * j];
}
