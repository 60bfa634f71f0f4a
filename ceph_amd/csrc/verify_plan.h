// verify_plan.h — host-side preparation for the consistency check
// (ecx_verify_batch / ecx_verify_chunks_host) and its CPU-only probe. Plain
// C++: no HIP, no device state, so the probe and the real calls run literally
// the same code and it can be tested (and sanitized) on a GPU-less box.
//
// A scrub hands over stripes and the set of chunks it holds (present_mask).
// The first k present chunks in id order are the survivors — the rule of
// ecx_decode_batch and ErasureCode.cc:154-170 — and determine the stripe;
// every further present chunk, data or parity, is "checked": recomputed from
// the survivors and compared with what is stored. No new algebra: the decode
// plan of the mask that holds only the k survivor bits treats every other
// chunk as erased, so it already has one coefficient row per non-survivor;
// the rows of the checked ids are picked out of it.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace ecx {

constexpr int VERIFY_MAX_OUT = 4;  // checked chunks per pass (kernel NOUT <= 4)

enum VerifyStatus {
  VERIFY_OK = 0,
  VERIFY_INVAL,  // a mask bit at position k+m or above
  VERIFY_IO,     // fewer than k chunks present, or survivors do not invert
};

struct VerifyPlan {
  std::vector<int> survivors;  // first k set bits of the mask
  std::vector<int> checked;    // the remaining set bits, ascending
  std::vector<uint8_t> rows;   // n_checked x k coefficients over survivors
};

// Decode plan of a mask: survivors[k], erased[] ascending, rows
// (n_erased x k). Returns false if the mask is undecodable. The library backs
// it with the decode-plan LRU, the probe with a bare compose_decode_rows.
using VerifyResolve =
    std::function<bool(uint64_t mask, std::vector<int> &survivors,
                       std::vector<int> &erased, std::vector<uint8_t> &rows)>;

// Plan the check of present_mask for a k-data, m-parity code (k + m <= 64).
// p is unspecified unless VERIFY_OK is returned. Exactly k bits: VERIFY_OK
// with nothing checked (resolve is still asked, so survivors that do not
// invert are refused whether or not anything would be checked).
VerifyStatus plan_verify(int k, int m, uint64_t present_mask,
                         const VerifyResolve &resolve, VerifyPlan &p);

}  // namespace ecx
