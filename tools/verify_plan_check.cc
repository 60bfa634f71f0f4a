// verify_plan_check.cc — stand-alone check of the verify planner
// (ceph_amd/csrc/verify_plan.cpp over gf.cpp), meant to be built with the
// host sanitizers; both files are plain C++, so no GPU and no HIP is involved.
// Build and run from the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/verify_plan_check.cc ceph_amd/csrc/verify_plan.cpp ceph_amd/csrc/gf.cpp -o /tmp/verify_plan_check && /tmp/verify_plan_check
//
// For every mask of RS(4,3) and RS(8,3) with at least k chunks present (all
// three w=8 matrix techniques) it plans the check, then recomputes every
// checked chunk of a generator-encoded stripe from the survivors with the
// plan's rows and compares. It also calls the three refusals. Exit status 0
// only if every answer is right.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ceph_amd/csrc/gf.h"
#include "../ceph_amd/csrc/verify_plan.h"

static int failures = 0;

#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");          \
      failures++;                          \
    }                                      \
  } while (0)

static ecx::VerifyResolve resolver(const std::vector<uint8_t>& gen, int k,
                                   int m) {
  return [&gen, k, m](uint64_t mask, std::vector<int>& sv,
                      std::vector<int>& er, std::vector<uint8_t>& rw) {
    return ecx::compose_decode_rows(gen, k, m, mask, sv, er, rw);
  };
}

static long check_code(int technique, int k, int m) {
  const ecx::GF8& f = ecx::gf8();
  const int n = k + m, C = 48;
  std::vector<uint8_t> gen;
  CHECK(ecx::gen_matrix(technique, gen, k, m), "gen_matrix %d", technique);
  // one stripe: pseudo-random data, every chunk = generator row x data
  std::vector<std::vector<uint8_t>> chunk(n, std::vector<uint8_t>(C));
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

  const ecx::VerifyResolve resolve = resolver(gen, k, m);
  long planned = 0;
  for (uint64_t mask = 0; mask < (1ull << n); mask++) {
    const int bits = __builtin_popcountll(mask);
    ecx::VerifyPlan p;
    const ecx::VerifyStatus st = ecx::plan_verify(k, m, mask, resolve, p);
    if (bits < k) {
      CHECK(st == ecx::VERIFY_IO, "mask %llx: %d bits not refused",
            (unsigned long long)mask, bits);
      continue;
    }
    planned++;
    CHECK(st == ecx::VERIFY_OK, "mask %llx refused", (unsigned long long)mask);
    if (st != ecx::VERIFY_OK) continue;
    std::vector<int> present;
    for (int i = 0; i < n; i++)
      if (mask >> i & 1) present.push_back(i);
    CHECK((int)p.survivors.size() == k && (int)p.checked.size() == bits - k &&
              p.rows.size() == p.checked.size() * (size_t)k,
          "mask %llx: sizes", (unsigned long long)mask);
    for (int i = 0; i < k; i++)
      CHECK(p.survivors[i] == present[i], "mask %llx: survivor %d",
            (unsigned long long)mask, i);
    for (size_t j = 0; j < p.checked.size(); j++) {
      CHECK(p.checked[j] == present[k + j], "mask %llx: checked %zu",
            (unsigned long long)mask, j);
      for (int b = 0; b < C; b++) {
        uint8_t s = 0;
        for (int i = 0; i < k; i++)
          s ^= f.mul(p.rows[j * k + i], chunk[p.survivors[i]][b]);
        if (s != chunk[p.checked[j]][b]) {
          CHECK(false, "mask %llx: chunk %d byte %d",
                (unsigned long long)mask, p.checked[j], b);
          break;
        }
      }
    }
  }
  return planned;
}

int main() {
  for (int technique = 0; technique < 3; technique++) {
    CHECK(check_code(technique, 4, 3) == 64, "RS(4,3): mask count");
    CHECK(check_code(technique, 8, 3) == 232, "RS(8,3): mask count");
  }

  // the three refusals, and the boundary next to each
  std::vector<uint8_t> gen;
  ecx::gen_matrix(0, gen, 8, 3);
  const ecx::VerifyResolve resolve = resolver(gen, 8, 3);
  ecx::VerifyPlan p;
  CHECK(ecx::plan_verify(8, 3, 1ull << 11 | 0x7ff, resolve, p) ==
            ecx::VERIFY_INVAL, "bit at k+m accepted");
  CHECK(ecx::plan_verify(8, 3, 1ull << 63 | 0x7ff, resolve, p) ==
            ecx::VERIFY_INVAL, "bit 63 accepted");
  CHECK(ecx::plan_verify(8, 3, 0x7f, resolve, p) == ecx::VERIFY_IO,
        "k-1 chunks accepted");
  CHECK(ecx::plan_verify(8, 3, 0xff, resolve, p) == ecx::VERIFY_OK &&
            p.checked.empty() && p.rows.empty(),
        "exactly k chunks: not an empty plan");
  // survivors that do not invert: two equal coding rows, both among the
  // survivors once data chunks 0 and 1 are absent
  std::vector<uint8_t> bad = gen;
  for (int j = 0; j < 8; j++) bad[(size_t)9 * 8 + j] = bad[(size_t)8 * 8 + j];
  const ecx::VerifyResolve resolve_bad = resolver(bad, 8, 3);
  CHECK(ecx::plan_verify(8, 3, 0x7fc, resolve_bad, p) == ecx::VERIFY_IO,
        "singular survivors accepted");
  CHECK(ecx::plan_verify(8, 3, 0x4ff, resolve_bad, p) == ecx::VERIFY_OK &&
            p.checked.size() == 1 && p.checked[0] == 10,
        "data survivors with a doubled coding row refused");
  // k + m = 64: the whole mask is legal
  ecx::gen_matrix(0, gen, 32, 32);
  const ecx::VerifyResolve resolve64 = resolver(gen, 32, 32);
  CHECK(ecx::plan_verify(32, 32, ~0ull, resolve64, p) == ecx::VERIFY_OK &&
            p.checked.size() == 32 && p.checked.back() == 63,
        "k+m = 64 full mask");

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("verify_plan_check OK\n");
  return 0;
}
