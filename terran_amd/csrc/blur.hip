// ta_frames_blur: Pillow's `region = im.crop(box).filter(ImageFilter.GaussianBlur(radius)); im.paste(region, box)` on
// rectangles of a resident frame batch, in place, bit for bit.  The passes, their weights and the planning of a round are
// in blur_passes.h (ta_frames_filter's unsharp mask runs them too); here: the checks, the rounds and the launches.
#include "blur_passes.h"
#include "region_rounds.h"

namespace {
using namespace gauss;

const char* check_region(const ta_blur_region& q) {
  if (q.x1 <= q.x0 || q.y1 <= q.y0) return "empty or inverted box";
  if (q.shape != TA_BLUR_BOX && q.shape != TA_BLUR_ELLIPSE) return "unknown shape";
  if (!radius_ok(q.radius)) return "radius negative, not finite or above 1024";
  return nullptr;
}

// round by round (a radius of 0 changes nothing, as in Pillow: no record)
void plan_work(const ta_blur_region* regions, int n, blur_work& w) {
  std::vector<int32_t> round;
  const int rounds = ta_plan_rounds(regions, n, round);
  std::vector<blur_job> jobs;
  for (int k = 0; k < rounds; ++k) {
    jobs.clear();
    for (int i = 0; i < n; ++i) {
      const ta_blur_region& q = regions[i];
      if (round[i] == k && q.radius != 0.f) jobs.push_back({q.frame, q.x0, q.y0, q.x1, q.y1, q.shape, q.radius, 0, 0});
    }
    w.add_round(jobs);
  }
}

}  // namespace

extern "C" int ta_blur_plan(const ta_blur_region* regions, int n, int32_t* rounds, float* box_radius, uint32_t* weights) {
  if (n < 0 || (n > 0 && !regions)) return TA_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (check_region(regions[i])) return TA_E_INVALID;
  std::vector<int32_t> round;
  ta_plan_rounds(regions, n, round);
  for (int i = 0; i < n; ++i) {
    float fr;
    int32_t r;
    uint32_t ww, fw;
    box_params(regions[i].radius, &fr, &r, &ww, &fw);
    if (rounds) rounds[i] = round[i];
    if (box_radius) box_radius[i] = fr;
    if (weights) weights[2 * i] = ww, weights[2 * i + 1] = fw;
  }
  return TA_OK;
}

extern "C" int ta_frames_blur(ta_ctx* ctx, ta_frames* frames, const ta_blur_region* regions, int n) {
  ta_enter(ctx);
  if (!ctx) return TA_E_INVALID;
  if (!frames || n < 0 || (n > 0 && !regions)) return ta_fail(ctx, TA_E_INVALID, "frames_blur: bad args");
  if (frames->ctx->device != ctx->device) return ta_fail(ctx, TA_E_INVALID, "frames_blur: the batch lives on another device");
  const int N = frames->n, H = frames->h, W = frames->w;
  for (int i = 0; i < n; ++i) {
    const ta_blur_region& q = regions[i];
    if (q.frame < 0 || q.frame >= N) return ta_fail(ctx, TA_E_INVALID, "frames_blur: region %d: frame %d out of range [0, %d)", i, q.frame, N);
    if (const char* why = check_region(q)) return ta_fail(ctx, TA_E_INVALID, "frames_blur: region %d: %s", i, why);
    if (q.x0 < 0 || q.y0 < 0 || q.x1 > W || q.y1 > H)
      return ta_fail(ctx, TA_E_INVALID, "frames_blur: region %d: [%d, %d) x [%d, %d) is not inside the %d x %d frame", i, q.x0, q.x1, q.y0, q.y1, W, H);
    if (q.x1 - q.x0 > MAX_SIDE || q.y1 - q.y0 > MAX_SIDE)
      return ta_fail(ctx, TA_E_INVALID, "frames_blur: region %d: a side longer than %d", i, MAX_SIDE);
  }
  if (n == 0) return TA_OK;

  blur_work w;
  plan_work(regions, n, w);
  const std::vector<blur_rec>& recs = w.recs;
  const std::vector<blur_item>& items = w.items;
  std::vector<int2>& tab = w.tab;
  const size_t pixels = w.pixels;
  if (recs.empty()) return TA_OK;
  if (tab.empty()) tab.push_back(make_int2(1, 0));

  const size_t b_rec = recs.size() * sizeof(blur_rec), b_item = items.size() * sizeof(blur_item), b_tab = tab.size() * sizeof(int2);
  const size_t o_item = (b_rec + 15) & ~(size_t)15, o_tab = (o_item + b_item + 15) & ~(size_t)15;
  const size_t staged = o_tab + b_tab, o_pix = (staged + 255) & ~(size_t)255;
  void *scr = nullptr, *pin = nullptr;
  TA_TRY(ta_scratch(ctx, o_pix + pixels, &scr));
  TA_TRY(ta_pinned(ctx, staged, &pin));
  char* hp = (char*)pin;
  memcpy(hp, recs.data(), b_rec);
  memcpy(hp + o_item, items.data(), b_item);
  memcpy(hp + o_tab, tab.data(), b_tab);
  TA_HIP(ctx, hipMemcpyAsync(scr, pin, staged, hipMemcpyHostToDevice, ctx->stream));
  char* dp = (char*)scr;
  TA_SET_LDS_ATTR(ctx, blur_rows, LDS_BUDGET);
  TA_SET_LDS_ATTR(ctx, blur_cols<false>, LDS_BUDGET);
  for (const blur_launch& L : w.launches)
    launch_round<false>(ctx->stream, frames->dev, H, W, L, (const blur_rec*)dp, (const blur_item*)(dp + o_item), (const int2*)(dp + o_tab),
                        (uint8_t*)(dp + o_pix));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
