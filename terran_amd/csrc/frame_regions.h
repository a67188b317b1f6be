// The host half that the frame region operations share (draw, blur, pixelate / resample, transform, histogram / point /
// saturate, filter): the checks of a call's regions, the rounds of in-place work, the ellipse span tables and the staging
// of a call's records and tables.  Host code; the kernels' side of the row strips is in pixel_walk.h.
#pragma once
#include "ta_internal.h"

#include <assert.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

// ---- checks ----------------------------------------------------------------------------------------------------------
// Every check of a call runs before anything is allocated or launched.
inline int ta_check_batch(ta_ctx* ctx, const char* who, const ta_frames* frames, const void* items, int n) {
  if (!frames || n < 0 || (n > 0 && !items)) return ta_fail(ctx, TA_E_INVALID, "%s: bad args", who);
  if (frames->ctx->device != ctx->device) return ta_fail(ctx, TA_E_INVALID, "%s: the batch lives on another device", who);
  return TA_OK;
}
inline int ta_check_frame(ta_ctx* ctx, const char* who, int i, int frame, int N) {
  if (frame < 0 || frame >= N) return ta_fail(ctx, TA_E_INVALID, "%s: region %d: frame %d out of range [0, %d)", who, i, frame, N);
  return TA_OK;
}

// What is wrong with a region whatever its frame (ta_blur_plan, ta_filter_plan have none): the box, the shape, then
// own(region), the call's own defect or nullptr.  R: int32 frame, the half-open box [x0, x1) x [y0, y1), shape.
template <class R, class F>
const char* ta_region_defect(const R& q, F own) {
  if (q.x1 <= q.x0 || q.y1 <= q.y0) return "empty or inverted box";
  if (q.shape != TA_BLUR_BOX && q.shape != TA_BLUR_ELLIPSE) return "unknown shape";
  return own(q);
}

// The boxes of an in-place call on `frames`, after ta_check_batch: per region its frame, ta_region_defect, the box inside
// the frame and no side longer than max_side.
template <class R, class F>
int ta_check_boxes(ta_ctx* ctx, const char* who, const ta_frames* frames, const R* regions, int n, int max_side, F own) {
  const int N = frames->n, H = frames->h, W = frames->w;
  for (int i = 0; i < n; ++i) {
    const R& q = regions[i];
    TA_TRY(ta_check_frame(ctx, who, i, q.frame, N));
    if (const char* why = ta_region_defect(q, own)) return ta_fail(ctx, TA_E_INVALID, "%s: region %d: %s", who, i, why);
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > W || q.y1 > H)
      return ta_fail(ctx, TA_E_INVALID, "%s: region %d: [%d, %d) x [%d, %d) is not inside the %d x %d frame", who, i, q.x0, q.x1, q.y0, q.y1, W, H);
    if (q.x1 - q.x0 > max_side || q.y1 - q.y0 > max_side) return ta_fail(ctx, TA_E_INVALID, "%s: region %d: a side longer than %d", who, i, max_side);
  }
  return TA_OK;
}

template <class R, class F>
int ta_check_regions(ta_ctx* ctx, const char* who, const ta_frames* frames, const R* regions, int n, int max_side, F own) {
  TA_TRY(ta_check_batch(ctx, who, frames, regions, n));
  return ta_check_boxes(ctx, who, frames, regions, n, max_side, own);
}

// ---- rounds ----------------------------------------------------------------------------------------------------------
// Regions of one frame apply in list order, so a region runs one round after the latest round of an earlier region of its
// frame that it intersects; the regions of one round are pairwise disjoint within their frame and run in one set of
// launches.
template <class R>
int ta_plan_rounds(const R* regions, int n, std::vector<int32_t>& round) {
  round.assign(n, 0);
  std::map<int32_t, std::vector<int>> of_frame;
  int rounds = 0;
  for (int i = 0; i < n; ++i) {
    const R& q = regions[i];
    std::vector<int>& earlier = of_frame[q.frame];
    for (int j : earlier) {
      const R& e = regions[j];
      if (q.x0 < e.x1 && e.x0 < q.x1 && q.y0 < e.y1 && e.y0 < q.y1) round[i] = std::max(round[i], round[j] + 1);
    }
    earlier.push_back(i);
    rounds = std::max(rounds, round[i] + 1);
  }
  return rounds;
}

// Round by round: each(region) for the regions of the round, in list order, then close() once.  Returns the rounds.
template <class R, class E, class C>
int ta_each_round(const R* regions, int n, E each, C close) {
  std::vector<int32_t> round;
  const int rounds = ta_plan_rounds(regions, n, round);
  for (int k = 0; k < rounds; ++k) {
    for (int i = 0; i < n; ++i)
      if (round[i] == k) each(regions[i]);
    close();
  }
  return rounds;
}

// ---- row strips ------------------------------------------------------------------------------------------------------
// Appends the strips of rows of recs[first ..] (records with w and h), one workgroup each, as items {record, first row,
// rows}: about strip_pixels pixels, min_rows at least (a row per wave).  Returns how many.
template <class I, class Q>
int ta_add_strips(std::vector<I>& items, const std::vector<Q>& recs, size_t first, int min_rows, int strip_pixels) {
  const size_t at = items.size();
  for (size_t j = first; j < recs.size(); ++j) {
    const int rows = std::max(min_rows, strip_pixels / recs[j].w);
    for (int y = 0; y < recs[j].h; y += rows) items.push_back({(int32_t)j, y, std::min(rows, recs[j].h - y)});
  }
  return (int)(items.size() - at);
}

// ---- ellipse span tables ---------------------------------------------------------------------------------------------
// Rows 0 .. h - 1 of ellipse([0, 0, w - 1, h - 1]) as TA_DRAW_DISC fills it (ta_disc_rows, draw.hip): row y covers pixels
// x .. y of its int2, nothing when x > y.  Equal sizes share one copy; `clamp` cuts every span to 0 .. w - 1, so that a
// kernel may walk it without looking at the box again.
struct ta_span_tables {
  explicit ta_span_tables(bool clamp = true) : clamp(clamp) {}

  int of(int w, int h) {                                // the first row of the w x h ellipse
    auto it = first.find({w, h});
    if (it == first.end()) {
      const size_t at = rows.size();
      it = first.emplace(std::make_pair(w, h), (int)at).first;
      ta_disc_rows(w - 1, h - 1, rows);                 // appends h rows
      for (size_t k = at; clamp && k < rows.size(); ++k) rows[k] = make_int2(std::max(rows[k].x, 0), std::min(rows[k].y, w - 1));
    }
    return it->second;
  }
  const std::vector<int2>& table() {                    // never empty: a kernel's pointer to it is valid
    if (rows.empty()) rows.push_back(make_int2(1, 0));
    return rows;
  }

 private:
  bool clamp;
  std::vector<int2> rows;
  std::map<std::pair<int, int>, int> first;
};

// ---- staging ---------------------------------------------------------------------------------------------------------
// What a call sends to the device, laid out once: put() the parts in order, then the areas that are not copied, then
// commit().  The parts go through the context's pinned block into its scratch block in ONE host-to-device copy on the
// context's stream; both blocks are reused by the next call, so a call synchronises the stream before it returns.
struct ta_staging {
  size_t slack = 0;          // bytes added to both blocks' sizes

  // `bytes` at `p`, which must stay valid and unchanged until commit(); returns the part's byte offset
  size_t put(const void* p, size_t bytes, size_t align = 16) {
    assert(!dev_end && !host_end);                      // an area lies behind ALL parts: a later part would overlap it
    const size_t at = (staged + align - 1) & ~(align - 1);
    parts.push_back({p, bytes, at});
    staged = at + bytes;
    return at;
  }
  template <class T>
  size_t put(const std::vector<T>& v, size_t align = 16) {
    return put(v.data(), v.size() * sizeof(T), align);
  }
  // 256-byte aligned areas behind the staged parts: of the scratch block, of the pinned block (for a read-back)
  size_t device_only(size_t bytes) { return area(&dev_end, bytes); }
  size_t host_only(size_t bytes) { return area(&host_end, bytes); }

  int commit(ta_ctx* ctx) {
    void *scr = nullptr, *pin = nullptr;
    TA_TRY(ta_scratch(ctx, std::max(dev_end, staged) + slack, &scr));
    TA_TRY(ta_pinned(ctx, std::max(host_end, staged) + slack, &pin));
    dp = (char*)scr, hp = (char*)pin;
    for (const part& p : parts)
      if (p.bytes) memcpy(hp + p.at, p.src, p.bytes);
    TA_HIP(ctx, hipMemcpyAsync(scr, pin, staged, hipMemcpyHostToDevice, ctx->stream));
    return TA_OK;
  }
  template <class T>
  T* dev(size_t at) const { return (T*)(dp + at); }
  template <class T>
  T* host(size_t at) const { return (T*)(hp + at); }

 private:
  struct part {
    const void* src;
    size_t bytes, at;
  };
  size_t area(size_t* end, size_t bytes) {
    const size_t at = (std::max(*end, staged) + 255) & ~(size_t)255;
    *end = at + bytes;
    return at;
  }
  std::vector<part> parts;
  size_t staged = 0, dev_end = 0, host_end = 0;
  char *dp = nullptr, *hp = nullptr;
};
