// update_plan.h — host-side preparation for the batch parity-delta write
// (ecx_update_batch) and its CPU-only probe. Plain C++: no HIP, no device
// state, so the probe and the real call run literally the same code and it
// can be tested (and sanitized) on a GPU-less box.
//
// A write queue hands over stripes that each overwrite their own set of data
// chunks: write_masks[s] bit j = data chunk j of stripe s is replaced. The
// new chunks arrive packed, stripe ascending then chunk id ascending, so
// stripe s's first new chunk sits at index new_base[s] = sum of the
// popcounts before it. Unlike the per-stripe decode (decode_multi.h) nothing
// is grouped by pattern or by output count: every touched stripe corrects
// all m parities, so a call is ceil(m/4) launches over the list of touched
// stripes, whatever the masks are.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ecx {

constexpr int UPDATE_MAX_OUT = 4;  // parities per pass (kernel NOUT <= 4)

struct UpdatePlan {
  std::vector<int32_t> new_base;  // per stripe: index of its first new chunk
  std::vector<int32_t> active;    // stripes with a nonzero mask, ascending
  long total_new = 0;             // new chunks in the call
  int launches = 0;               // ceil(m/4) if any stripe is active, else 0
};

// Plan n per-stripe write masks for a k-data, m-parity code. Returns false —
// with p unspecified — as soon as one mask has a bit at position k or above.
// n is bounded by the caller (the packed index must fit 32 bits: n * k).
bool plan_update(int k, int m, const uint64_t *masks, long n, UpdatePlan &p);

}  // namespace ecx
