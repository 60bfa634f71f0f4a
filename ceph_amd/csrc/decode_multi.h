// decode_multi.h — host-side grouping for the per-stripe-pattern decode
// entries (ecx_decode_batch_multi / ecx_decode_slices_multi) and their
// CPU-only probe. Plain C++: no HIP, no device state, so the probe and the
// real calls run literally the same code and it can be tested (and
// sanitized) on a GPU-less box.
//
// A recovery batching shim hands over stripes whose neighbours miss
// different chunks. The kernels are templated on the output count, so the
// call is cut into launches by (pass, outputs-in-pass) — never by pattern:
//   * pass p of a stripe with e erasures reconstructs erased[4p .. 4p+3]
//     (the same <= 4-output split run_matmul applies to a uniform call);
//   * launch (p, n_out) lists every stripe whose pass p has n_out outputs.
// Pass p can have 1..min(4, m-4p) outputs, so a call makes at most m
// launches however many distinct patterns it holds.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace ecx {

constexpr int MULTI_MAX_OUT = 4;  // outputs per pass (kernel NOUT <= 4)

struct MultiLaunch {
  int pass;                  // outputs erased[4*pass ..] of each member
  int n_out;                 // 1..MULTI_MAX_OUT
  std::vector<int> members;  // stripe (or slice) ids, ascending
};

struct MultiGrouping {
  // distinct masks with >= 1 erasure, in first-appearance order, reduced
  // to their low k+m bits
  std::vector<uint64_t> masks;
  std::vector<int> n_erased;        // per distinct mask
  std::vector<int> plan_of_stripe;  // index into masks, -1 = nothing erased
  std::vector<MultiLaunch> launches;  // ordered by (pass, n_out)
  int n_pass = 0;  // passes of the most-erased mask = records per plan
};

// Group n per-stripe masks. resolve(mask) is called once per distinct mask
// that erases something and returns false if the mask is undecodable (the
// real calls back it with the decode-plan LRU, the probe with a bare
// compose_decode_rows). Returns false — with g unspecified — as soon as
// one mask is undecodable.
bool group_decode_masks(int k, int m, const uint64_t *masks, long n,
                        const std::function<bool(uint64_t)> &resolve,
                        MultiGrouping &g);

}  // namespace ecx
