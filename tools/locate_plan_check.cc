// locate_plan_check.cc — stand-alone check of the locate planner and finish
// rule (ceph_amd/csrc/locate_plan.{h,cpp} over verify_plan.cpp and gf.cpp),
// meant to be built with the host sanitizers; all of it is plain C++, so no
// GPU and no HIP is involved. Build and run from the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/locate_plan_check.cc ceph_amd/csrc/locate_plan.cpp ceph_amd/csrc/verify_plan.cpp ceph_amd/csrc/gf.cpp -o /tmp/locate_plan_check && /tmp/locate_plan_check
//
// For every mask of RS(4,3) and RS(8,3) (all three w=8 matrix techniques) and
// of reed_sol_van RS(4,6) it plans the location and checks the status against
// the number of present chunks. For every planned mask it then plays the device's part on the
// host: a generator-encoded stripe, clean, with each single chunk damaged and
// with two chunks damaged in different byte columns; the verify word from
// the base plan's rows, the refuted word from the candidates' rows, and
// locate_word() must give present_mask, 1 << x (present_mask if x is absent)
// and 0. Exit status 0 only if every answer is right.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ceph_amd/csrc/gf.h"
#include "../ceph_amd/csrc/locate_plan.h"

static int failures = 0;

#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");          \
      failures++;                          \
    }                                      \
  } while (0)

typedef std::vector<std::vector<uint8_t>> Stripe;

// Bits of the plan's checked chunks that differ from rows x survivors.
static uint64_t verify_word(const ecx::VerifyPlan& p, const Stripe& st, int k) {
  const ecx::GF8& f = ecx::gf8();
  uint64_t word = 0;
  for (size_t j = 0; j < p.checked.size(); j++)
    for (size_t b = 0; b < st[0].size(); b++) {
      uint8_t s = 0;
      for (int i = 0; i < k; i++)
        s ^= f.mul(p.rows[j * (size_t)k + i], st[p.survivors[i]][b]);
      if (s != st[p.checked[j]][b]) {
        word |= 1ull << p.checked[j];
        break;
      }
    }
  return word;
}

static uint64_t locate(const ecx::LocatePlan& lp, const Stripe& st, int k,
                       uint64_t mask, uint64_t* bad_out) {
  uint64_t surv = 0, refuted = 0;
  for (int s : lp.base.survivors) surv |= 1ull << s;
  const uint64_t bad = verify_word(lp.base, st, k);
  for (int i = 0; i < k; i++)
    if (verify_word(lp.cand[i], st, k)) refuted |= 1ull << lp.base.survivors[i];
  *bad_out = bad;
  return ecx::locate_word(mask, surv, bad, refuted);
}

static long check_code(int technique, int k, int m) {
  const ecx::GF8& f = ecx::gf8();
  const int n = k + m, C = 32;
  std::vector<uint8_t> gen;
  CHECK(ecx::gen_matrix(technique, gen, k, m), "gen_matrix %d", technique);
  Stripe chunk(n, std::vector<uint8_t>(C));
  uint32_t x = 0x9E3779B9u * (uint32_t)(technique + 7 * k + 1);
  for (int i = 0; i < k; i++)
    for (int b = 0; b < C; b++) {
      x = x * 1664525u + 1013904223u;
      chunk[i][b] = (uint8_t)(x >> 24);
    }
  for (int i = k; i < n; i++)
    for (int b = 0; b < C; b++) {
      uint8_t s = 0;
      for (int j = 0; j < k; j++) s ^= f.mul(gen[(size_t)i * k + j], chunk[j][b]);
      chunk[i][b] = s;
    }

  const ecx::VerifyResolve resolve =
      [&gen, k, m](uint64_t mask, std::vector<int>& sv, std::vector<int>& er,
                   std::vector<uint8_t>& rw) {
        return ecx::compose_decode_rows(gen, k, m, mask, sv, er, rw);
      };
  long planned = 0;
  for (uint64_t mask = 0; mask < (1ull << n); mask++) {
    ecx::LocatePlan lp;
    const ecx::VerifyStatus st = ecx::plan_locate(k, m, mask, resolve, lp);
    const int bits = __builtin_popcountll(mask);
    const ecx::VerifyStatus want = bits < k       ? ecx::VERIFY_IO
                                   : bits < k + 2 ? ecx::VERIFY_INVAL
                                                  : ecx::VERIFY_OK;
    CHECK(st == want, "t%d (%d,%d) mask %llx: status %d, want %d", technique,
          k, m, (unsigned long long)mask, (int)st, (int)want);
    if (st != ecx::VERIFY_OK) continue;
    planned++;
    CHECK((int)lp.cand.size() == k, "candidates");
    for (int i = 0; i < k; i++) {
      const ecx::VerifyPlan& cp = lp.cand[i];
      CHECK(cp.checked.size() + 1 == lp.base.checked.size() &&
                cp.rows.size() == cp.checked.size() * (size_t)k,
            "candidate %d sizes", i);
      for (int s : cp.survivors)
        CHECK(s != lp.base.survivors[i], "candidate %d keeps its survivor", i);
    }
    uint64_t bad;
    CHECK(locate(lp, chunk, k, mask, &bad) == mask && bad == 0,
          "mask %llx: clean stripe", (unsigned long long)mask);
    for (int d = 0; d < n; d++) {
      Stripe s1 = chunk;
      s1[d][(7 * d + 3) % C] ^= (uint8_t)(1 + d);
      const uint64_t got = locate(lp, s1, k, mask, &bad);
      const uint64_t exp = (mask >> d & 1) ? 1ull << d : mask;
      CHECK(got == exp && (bad != 0) == ((mask >> d & 1) != 0),
            "t%d (%d,%d) mask %llx chunk %d: culprit %llx, want %llx",
            technique, k, m, (unsigned long long)mask, d,
            (unsigned long long)got, (unsigned long long)exp);
      // a second present chunk, in another byte column
      const int e = (d + 2) % n;
      if (!(mask >> d & 1) || !(mask >> e & 1)) continue;
      s1[e][(7 * d + 4) % C] ^= 0x80;
      CHECK(locate(lp, s1, k, mask, &bad) == 0 && bad != 0,
            "mask %llx chunks %d,%d: located", (unsigned long long)mask, d, e);
    }
  }
  // a mask bit at k+m
  ecx::LocatePlan lp;
  CHECK(ecx::plan_locate(k, m, (1ull << n) | ((1ull << n) - 1), resolve, lp) ==
            ecx::VERIFY_INVAL,
        "bit at k+m");
  return planned;
}

int main() {
  long planned = 0;
  for (int technique : {0, 1, 2}) {
    planned += check_code(technique, 4, 3);
    planned += check_code(technique, 8, 3);
  }
  planned += check_code(0, 4, 6);  // candidates with five checked chunks
  // the finish rule on its documented cases
  CHECK(ecx::locate_word(0x7F, 0x0F, 0, 0x3) == 0x7F, "bad == 0");
  CHECK(ecx::locate_word(0x7F, 0x0F, 0x70, 0xB) == 0x04, "one survivor left");
  CHECK(ecx::locate_word(0x7F, 0x0F, 0x20, 0xF) == 0x20, "one checked bit");
  CHECK(ecx::locate_word(0x7F, 0x0F, 0x30, 0xF) == 0, "two checked bits");
  // (4,3): 1 + 7 masks with >= 6 bits; (8,3): 1 + 11 masks with >= 10 bits;
  // (4,6): 386 masks with >= 6 bits
  CHECK(planned == 3 * (8 + 12) + 386, "planned %ld masks", planned);
  if (failures) {
    std::fprintf(stderr, "locate_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("locate_plan_check: ok (%ld masks planned)\n", planned);
  return 0;
}
