// locate_plan.h — host-side preparation for naming the corrupt chunk of an
// inconsistent stripe (ecx_locate_batch / ecx_locate_chunks_host /
// ecx_repair_batch) and its CPU-only probes. Plain C++ like
// verify_plan.h: no HIP, no device state, one code path for the library and
// the probe.
//
// Definition: bit x of a stripe's culprit word is set exactly when x is
// present and the check of present_mask & ~(1 << x) would report 0 — leaving
// chunk x out makes the remaining chunks agree with each other.
//
// Leaving out a checked chunk j keeps the survivors and their rows, so that
// candidate's word is simply bad & ~(1 << j): no plan, no launch. Leaving out
// survivor s_i changes the survivors to the others plus checked[0]; that
// candidate is the verify plan of present_mask & ~(1 << s_i) and checks the
// remaining n_checked - 1 chunks.
#pragma once

#include <cstdint>
#include <vector>

#include "verify_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECX_LOCATE_FN __host__ __device__ inline
#else
#define ECX_LOCATE_FN inline
#endif

namespace ecx {

struct LocatePlan {
  VerifyPlan base;               // the plan of present_mask itself
  std::vector<VerifyPlan> cand;  // [i]: the plan without base.survivors[i]
};

// Plan the location for present_mask. lp is unspecified unless VERIFY_OK is
// returned. VERIFY_INVAL for a mask bit at k+m or above and for fewer than
// two checked chunks (every present chunk would qualify); VERIFY_IO for fewer
// than k present chunks and for a base or candidate mask that does not
// resolve.
VerifyStatus plan_locate(int k, int m, uint64_t present_mask,
                         const VerifyResolve &resolve, LocatePlan &lp);

// The finish rule, shared by ec_locate_finish_kernel and the host.
// refuted: bit s_i set when the candidate without survivor s_i found a
// difference in this stripe.
ECX_LOCATE_FN uint64_t locate_word(uint64_t present_mask,
                                   uint64_t survivor_mask, uint64_t bad,
                                   uint64_t refuted) {
  if (bad == 0) return present_mask;
  // a checked chunk j qualifies when (bad & ~(1 << j)) == 0: it is the only
  // one flagged
  const uint64_t only = (bad & (bad - 1)) == 0 ? bad : 0;
  return (survivor_mask & ~refuted) | (only & present_mask & ~survivor_mask);
}

}  // namespace ecx
