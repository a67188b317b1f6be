// ta_frames_blur: Pillow's `region = im.crop(box).filter(ImageFilter.GaussianBlur(radius)); im.paste(region, box)` on
// rectangles of a resident frame batch, in place, bit for bit.  The passes, their weights and the planning of a round are
// in blur_passes.h (ta_frames_filter's unsharp mask runs them too); here: the checks, the rounds and the launches.
#include "blur_passes.h"

namespace {
using namespace gauss;

const char* check_radius(const ta_blur_region& q) { return radius_ok(q.radius) ? nullptr : "radius negative, not finite or above 1024"; }

}  // namespace

extern "C" int ta_blur_plan(const ta_blur_region* regions, int n, int32_t* rounds, float* box_radius, uint32_t* weights) {
  if (n < 0 || (n > 0 && !regions)) return TA_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (ta_region_defect(regions[i], check_radius)) return TA_E_INVALID;
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
  TA_TRY(ta_check_regions(ctx, "frames_blur", frames, regions, n, MAX_SIDE, check_radius));
  if (n == 0) return TA_OK;

  // round by round (a radius of 0 changes nothing, as in Pillow: no record)
  blur_work w;
  std::vector<blur_job> jobs;
  ta_each_round(
      regions, n,
      [&](const ta_blur_region& q) {
        if (q.radius != 0.f) jobs.push_back({q.frame, q.x0, q.y0, q.x1, q.y1, q.shape, q.radius, 0, 0});
      },
      [&] {
        w.add_round(jobs);
        jobs.clear();
      });
  if (w.recs.empty()) return TA_OK;

  ta_staging st;                                    // one H2D copy; the pixel scratch behind it
  w.put(st);
  const size_t o_pix = st.device_only(w.pixels);
  TA_TRY(st.commit(ctx));
  TA_SET_LDS_ATTR(ctx, blur_rows, LDS_BUDGET);
  TA_SET_LDS_ATTR(ctx, blur_cols<false>, LDS_BUDGET);
  for (size_t k = 0; k < w.launches.size(); ++k) w.launch_round<false>(ctx->stream, frames->dev, frames->h, frames->w, k, st, st.dev<uint8_t>(o_pix));
  TA_HIP(ctx, hipGetLastError());
  TA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // pinned / scratch staging is reused by the next call
  return TA_OK;
}
