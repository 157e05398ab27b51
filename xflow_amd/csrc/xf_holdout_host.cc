// xf_holdout_host.cc — the host side of held-out validation that needs no GPU: the exported
// decision of a row (xf_holdout.h) and the early-stop rule.  Plain C++: it also builds into a
// stand-alone program under the host sanitizers (tools/holdout_host_check.cc).
#include <math.h>

#include "xf_common.h"
#include "xf_holdout.h"

extern "C" int xf_holdout_held(uint64_t seed, uint64_t stream, uint64_t ordinal, float share) {
  if (!(share >= 0.0f && share < 1.0f)) return 0;
  return xf::holdout_held_row(xf::holdout_base(seed, stream), ordinal,
                              xf::holdout_threshold((double)share)) ? 1 : 0;
}

// The curve is walked once, epoch by epoch, as a worker that calls this after every validated
// epoch sees it: `since` counts the epochs after the best one that did not improve on it.
extern "C" int xf_holdout_should_stop(const double *logloss, int n, int patience, double delta,
                                      int *best) {
  if (best) *best = -1;
  if (n <= 0 || !logloss || !(delta >= 0.0)) return 0;
  int at = -1, since = 0;
  double low = INFINITY;
  for (int i = 0; i < n; ++i) {
    const double L = logloss[i];
    if (isnan(L)) continue;  // neither an improvement nor an epoch without one
    if (L < low - delta) {   // (strict: a tie is no improvement; the first finite value improves)
      low = L;
      at = i;
      since = 0;
    } else {
      ++since;
    }
  }
  if (best) *best = at;
  return patience > 0 && since >= patience && !isnan(logloss[n - 1]) ? 1 : 0;
}
