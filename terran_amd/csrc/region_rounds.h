// Rounds of in-place region work (ta_frames_blur, ta_frames_pixelate): regions of one frame apply in list order, so a
// region runs one round after the latest round of an earlier region of its frame that it intersects; the regions of one
// round are pairwise disjoint within their frame and run in one set of launches.  Host code.
// R: a record with int32 frame and the half-open box [x0, x1) x [y0, y1).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

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
