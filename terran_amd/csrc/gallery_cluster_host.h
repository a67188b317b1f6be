// The host half of ta_gallery_cluster (gallery_cluster.hip): argument checks and the renumbering of the component roots.
// Plain C++ with no device code, so that tests/native/cluster_host_check.cpp can run it under a sanitizer.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define GAL_CLUSTER_MAX_ROWS (1ll << 18)  // lib.py: GALLERY_CLUSTER_MAX_ROWS; the adjacency bit matrix of 2^18 rows is 8 GiB

// The row limit of a call: 2^18, or what TA_GALLERY_CLUSTER_MAX_ROWS (tests only) lowers it to.
static inline long long gal_cluster_limit() {
  long long limit = GAL_CLUSTER_MAX_ROWS;
  const char* e = getenv("TA_GALLERY_CLUSTER_MAX_ROWS");
  if (e && e[0]) {
    const long long v = atoll(e);
    if (v >= 0 && v < limit) limit = v;
  }
  return limit;
}

// nullptr if the arguments are fine, else what is wrong with them (written into msg)
static inline const char* gal_cluster_check(float threshold, int min_samples, long long size, const int32_t* labels_out, char* msg, size_t cap) {
  if (min_samples < 1) {
    snprintf(msg, cap, "gallery: min_samples = %d is below 1", min_samples);
    return msg;
  }
  if (!isfinite(threshold)) {
    snprintf(msg, cap, "gallery: the threshold is not finite");
    return msg;
  }
  const long long limit = gal_cluster_limit();
  if (size > limit) {
    snprintf(msg, cap, "gallery: %lld rows are more than the %lld that can be clustered (the limit is 2^18 rows, an adjacency of 8 GiB)", size, limit);
    return msg;
  }
  if (size > 0 && !labels_out) {
    snprintf(msg, cap, "gallery: null pointer");
    return msg;
  }
  return nullptr;
}

// root[i]: the smallest core row of row i's cluster (root[r] == r exactly for the roots themselves), or < 0 for noise.
// labels[i] = the rank of root[i] among the roots in ascending order, or -1; returns the number of clusters, or -1 if
// root[] is not of that form (a label out of range, or one that is no root).
static inline long long gal_renumber(const int32_t* root, long long n, int32_t* labels) {
  std::vector<int32_t> number((size_t)n, -1);
  int32_t count = 0;
  for (long long i = 0; i < n; ++i)
    if (root[i] == i) number[(size_t)i] = count++;
  for (long long i = 0; i < n; ++i) {
    const int32_t r = root[i];
    if (r < 0) {
      labels[i] = -1;
      continue;
    }
    if (r >= n || number[(size_t)r] < 0) return -1;
    labels[i] = number[(size_t)r];
  }
  return count;
}
