// decode_multi.cpp — see decode_multi.h.
#include "decode_multi.h"

#include <unordered_map>

namespace ecx {

bool group_decode_masks(int k, int m, const uint64_t *masks, long n,
                        const std::function<bool(uint64_t)> &resolve,
                        MultiGrouping &g) {
  const int cps = k + m;
  const uint64_t all = cps >= 64 ? ~0ull : ((1ull << cps) - 1);
  g.masks.clear();
  g.n_erased.clear();
  g.launches.clear();
  g.plan_of_stripe.assign((size_t)n, -1);
  g.n_pass = 0;

  std::unordered_map<uint64_t, int> seen;  // mask -> plan index (or -1)
  for (long s = 0; s < n; s++) {
    const uint64_t mask = masks[s] & all;
    auto it = seen.find(mask);
    if (it == seen.end()) {
      int plan = -1;
      const int e = __builtin_popcountll(all & ~mask);
      if (e > 0) {
        if (e > m || !resolve(mask)) return false;
        plan = (int)g.masks.size();
        g.masks.push_back(mask);
        g.n_erased.push_back(e);
        const int passes = (e + MULTI_MAX_OUT - 1) / MULTI_MAX_OUT;
        if (passes > g.n_pass) g.n_pass = passes;
      }
      it = seen.emplace(mask, plan).first;
    }
    g.plan_of_stripe[(size_t)s] = it->second;
  }

  // bucket[pass][n_out-1]; stripes are visited in order, so member lists
  // come out ascending
  std::vector<MultiLaunch> bucket((size_t)g.n_pass * MULTI_MAX_OUT);
  for (int p = 0; p < g.n_pass; p++)
    for (int o = 0; o < MULTI_MAX_OUT; o++) {
      bucket[(size_t)p * MULTI_MAX_OUT + o].pass = p;
      bucket[(size_t)p * MULTI_MAX_OUT + o].n_out = o + 1;
    }
  for (long s = 0; s < n; s++) {
    const int plan = g.plan_of_stripe[(size_t)s];
    if (plan < 0) continue;  // fully present: in no launch, never touched
    const int e = g.n_erased[(size_t)plan];
    for (int p = 0; p * MULTI_MAX_OUT < e; p++) {
      const int rest = e - p * MULTI_MAX_OUT;
      const int no = rest < MULTI_MAX_OUT ? rest : MULTI_MAX_OUT;
      bucket[(size_t)p * MULTI_MAX_OUT + no - 1].members.push_back((int)s);
    }
  }
  for (auto &b : bucket)
    if (!b.members.empty()) g.launches.push_back(std::move(b));
  return true;
}

}  // namespace ecx
