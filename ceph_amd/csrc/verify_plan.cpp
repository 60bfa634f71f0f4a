// verify_plan.cpp — see verify_plan.h.
#include "verify_plan.h"

#include <cstring>

namespace ecx {

VerifyStatus plan_verify(int k, int m, uint64_t present_mask,
                         const VerifyResolve &resolve, VerifyPlan &p) {
  const int cps = k + m;
  const uint64_t all = cps >= 64 ? ~0ull : ((1ull << cps) - 1);
  if (present_mask & ~all) return VERIFY_INVAL;
  p.survivors.clear();
  p.checked.clear();
  p.rows.clear();
  uint64_t surv_mask = 0;
  for (int i = 0; i < cps; i++) {
    if (!(present_mask >> i & 1)) continue;
    if ((int)p.survivors.size() < k) {
      p.survivors.push_back(i);
      surv_mask |= 1ull << i;
    } else {
      p.checked.push_back(i);
    }
  }
  if ((int)p.survivors.size() < k) return VERIFY_IO;

  // every non-survivor is "erased" under the survivors-only mask
  std::vector<int> sv, er;
  std::vector<uint8_t> rw;
  if (!resolve(surv_mask, sv, er, rw)) return VERIFY_IO;
  if (sv != p.survivors || rw.size() != er.size() * (size_t)k)
    return VERIFY_IO;  // a resolver that does not follow the survivor rule
  p.rows.resize(p.checked.size() * (size_t)k);
  size_t e = 0;
  for (size_t j = 0; j < p.checked.size(); j++) {
    // both lists ascend, so one forward scan finds every checked id
    while (e < er.size() && er[e] != p.checked[j]) e++;
    if (e == er.size()) return VERIFY_IO;
    std::memcpy(&p.rows[j * (size_t)k], &rw[e * (size_t)k], (size_t)k);
  }
  return VERIFY_OK;
}

}  // namespace ecx
