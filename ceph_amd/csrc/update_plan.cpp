// update_plan.cpp — see update_plan.h.
#include "update_plan.h"

namespace ecx {

bool plan_update(int k, int m, const uint64_t *masks, long n, UpdatePlan &p) {
  const uint64_t data = k >= 64 ? ~0ull : ((1ull << k) - 1);
  p.new_base.assign((size_t)n, 0);
  p.active.clear();
  p.total_new = 0;
  for (long s = 0; s < n; s++) {
    if (masks[s] & ~data) return false;
    p.new_base[(size_t)s] = (int32_t)p.total_new;
    if (masks[s]) {
      p.active.push_back((int32_t)s);
      p.total_new += __builtin_popcountll(masks[s]);
    }
  }
  p.launches =
      p.active.empty() ? 0 : (m + UPDATE_MAX_OUT - 1) / UPDATE_MAX_OUT;
  return true;
}

}  // namespace ecx
