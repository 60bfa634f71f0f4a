// locate_plan.cpp — see locate_plan.h.
#include "locate_plan.h"

namespace ecx {

VerifyStatus plan_locate(int k, int m, uint64_t present_mask,
                         const VerifyResolve &resolve, LocatePlan &lp) {
  const int cps = k + m;
  const uint64_t all = cps >= 64 ? ~0ull : ((1ull << cps) - 1);
  if (present_mask & ~all) return VERIFY_INVAL;
  const int n_present = __builtin_popcountll(present_mask);
  if (n_present < k) return VERIFY_IO;
  if (n_present < k + 2) return VERIFY_INVAL;
  VerifyStatus st = plan_verify(k, m, present_mask, resolve, lp.base);
  if (st != VERIFY_OK) return st;
  lp.cand.assign((size_t)k, VerifyPlan());
  for (int i = 0; i < k; i++) {
    st = plan_verify(k, m, present_mask & ~(1ull << lp.base.survivors[i]),
                     resolve, lp.cand[i]);
    if (st != VERIFY_OK) return st;
  }
  return VERIFY_OK;
}

}  // namespace ecx
