// crc_plan_check.cc — stand-alone check of the CRC-32C host side
// (ceph_amd/csrc/crc_plan.cpp: the launch plan, the host hash and the shift),
// meant to be built with the host sanitizers; the file is plain C++, so no
// GPU and no HIP is involved. Build and run from the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/crc_plan_check.cc ceph_amd/csrc/crc_plan.cpp -o /tmp/crc_plan_check && /tmp/crc_plan_check
//
// Known answers of the hash; both host paths against a bit-at-a-time loop at
// every length 0..300 and every alignment 0..8; the combine identity and the
// composition of shifts; for every chunk size that is a multiple of 16 up to
// 64 KiB + 48 (and a few large ones) the end-aligned tiling of the plan,
// replayed on the host exactly as the kernel combines it (lane segments from
// state 0, times the kernel's constants) against the plain hash; the chain
// scan's constants replayed the same way; the refusals. Exit status 0 only
// if every answer is right.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ceph_amd/csrc/crc_plan.h"

static int failures = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      failures++;                                 \
    }                                             \
  } while (0)

static uint32_t bitwise(uint32_t crc, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    crc ^= p[i];
    for (int b = 0; b < 8; b++)
      crc = (crc >> 1) ^ ((crc & 1) ? ecx::CRC32C_POLY : 0);
  }
  return crc;
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}

// The chunk hashed the way the kernel does it: blocks and segments from the
// end, every segment from state 0, multiplied by the constants of CrcCombine.
static uint32_t kernel_way(uint32_t seed, const uint8_t* p, size_t C,
                           const ecx::CrcPlan& pl) {
  static const ecx::CrcCombine comb;
  const long L = pl.seg_bytes, T = pl.segs_per_block, B = L * T;
  const long bpc = pl.blocks_per_chunk;
  uint32_t word = ecx::crc_mulmod(seed, ecx::crc_xpow8(C));
  size_t covered = 0;
  for (long b = 0; b < bpc; b++) {
    const long long base = (long long)C - (long long)(bpc - b) * B;
    uint32_t blk = 0;
    for (long t = 0; t < T; t++) {
      long long s0 = base + t * L, s1 = s0 + L;
      if (s1 <= 0) continue;
      if (s0 < 0) s0 = 0;
      CHECK(s1 <= (long long)C, "segment past the end, C=%zu", C);
      covered += (size_t)(s1 - s0);
      blk ^= ecx::crc_mulmod(
          ecx::crc32c_host_tables(0, p + s0, (size_t)(s1 - s0)), comb.seg[t]);
    }
    unsigned long after = (unsigned long)(bpc - 1 - b);
    for (int i = 0; after; after >>= 1, i++)
      if (after & 1) blk = ecx::crc_mulmod(blk, comb.blk[i]);
    word ^= blk;
  }
  CHECK(covered == C, "segments cover %zu of %zu bytes", covered, C);
  return word;
}

int main() {
  // known answers
  {
    const uint8_t nine[] = "123456789";
    CHECK(~ecx::crc32c_host(~0u, nine, 9) == 0xE3069283u, "check value");
    uint8_t v[32];
    std::memset(v, 0, 32);
    CHECK(~ecx::crc32c_host(~0u, v, 32) == 0x8A9136AAu, "iSCSI zeros");
    std::memset(v, 0xFF, 32);
    CHECK(~ecx::crc32c_host(~0u, v, 32) == 0x62A8AB43u, "iSCSI ones");
    for (int i = 0; i < 32; i++) v[i] = (uint8_t)i;
    CHECK(~ecx::crc32c_host(~0u, v, 32) == 0x46DD794Eu, "iSCSI ascending");
    for (int i = 0; i < 32; i++) v[i] = (uint8_t)(31 - i);
    CHECK(~ecx::crc32c_host(~0u, v, 32) == 0x113FDB5Cu, "iSCSI descending");
    const uint8_t foo[] = "foo bar baz";
    CHECK(ecx::crc32c_host(0, foo, 11) == 4119623852u, "ceph seed 0");
    CHECK(ecx::crc32c_host(1234, foo, 11) == 881700046u, "ceph seed 1234");
  }
  // both paths, every short length and alignment
  {
    std::vector<uint8_t> buf(320);
    for (auto& x : buf) x = (uint8_t)rnd();
    for (size_t off = 0; off <= 8; off++)
      for (size_t n = 0; n + off <= 308; n++) {
        const uint32_t seed = rnd();
        const uint32_t want = bitwise(seed, buf.data() + off, n);
        CHECK(ecx::crc32c_host(seed, buf.data() + off, n) == want,
              "host off=%zu n=%zu", off, n);
        CHECK(ecx::crc32c_host_tables(seed, buf.data() + off, n) == want,
              "tables off=%zu n=%zu", off, n);
      }
  }
  // shifts
  {
    CHECK(ecx::crc32c_shift(0xDEADBEEFu, 0) == 0xDEADBEEFu, "shift by 0");
    const uint8_t zeros[64] = {};
    for (size_t n = 0; n <= 64; n++) {
      const uint32_t c = rnd();
      CHECK(ecx::crc32c_shift(c, n) == bitwise(c, zeros, n), "shift %zu", n);
    }
    const uint64_t big[] = {1, 4096, 1ull << 20, (1ull << 32) + 7,
                            (1ull << 40) + 12345};
    for (uint64_t a : big)
      for (uint64_t b : big) {
        const uint32_t c = rnd();
        CHECK(ecx::crc32c_shift(ecx::crc32c_shift(c, a), b) ==
                  ecx::crc32c_shift(c, a + b),
              "shifts compose");
      }
  }
  // the plan, replayed
  {
    const size_t max_c = (1u << 20) + 16;
    std::vector<uint8_t> buf(max_c);
    for (auto& x : buf) x = (uint8_t)rnd();
    std::vector<size_t> sizes;
    for (size_t c = 16; c <= 65536 + 48; c += 16) sizes.push_back(c);
    sizes.push_back(1u << 20);
    sizes.push_back((1u << 20) + 16);
    for (size_t C : sizes) {
      ecx::CrcPlan pl;
      CHECK(ecx::plan_crc(C, 3, 5, pl), "plan refused C=%zu", C);
      const long B = pl.seg_bytes * pl.segs_per_block;
      CHECK(pl.blocks_per_chunk == (long)((C + B - 1) / B), "bpc C=%zu", C);
      CHECK(pl.grid == 15 * pl.blocks_per_chunk, "grid C=%zu", C);
      CHECK(pl.threads == pl.segs_per_block && pl.launches == 2 &&
                pl.lds_bytes <= 160 * 1024 / 4,
            "shape C=%zu", C);
      // the big sweep at a stride, the interesting sizes always
      if (C > 4096 && C % 1040 && C % (size_t)B > 32 && (C + 16) % B > 32 &&
          C < 65536)
        continue;
      const uint32_t seed = rnd();
      const uint8_t* p = buf.data() + (max_c - C);  // ends at the buffer's end
      CHECK(kernel_way(seed, p, C, pl) == ecx::crc32c_host(seed, p, C),
            "kernel-way hash C=%zu", C);
    }
  }
  // the chain scan's constants
  for (long S : {1L, 2L, 5L, 257L, 1024L, 1025L, 65535L}) {
    const size_t C = 4112;
    ecx::CrcChainPlan cp;
    ecx::plan_crc_chain(C, S, cp);
    const long lanes = 1L << ecx::CRC_CHAIN_LOG2;
    CHECK((long)cp.run * lanes >= S && ((long)cp.run - 1) * lanes < S,
          "chain run S=%ld", S);
    CHECK(cp.x_chunk == ecx::crc32c_shift(ecx::CRC_ONE, C), "x_chunk");
    for (int i = 0; i < ecx::CRC_CHAIN_LOG2; i++)
      CHECK(cp.x_step[i] == ecx::crc32c_shift(
                                ecx::CRC_ONE, (uint64_t)C * cp.run << i),
            "x_step[%d] S=%ld", i, S);
  }
  // refusals
  {
    ecx::CrcPlan pl;
    CHECK(!ecx::plan_crc(0, 1, 1, pl), "C=0");
    CHECK(!ecx::plan_crc(24, 1, 1, pl), "C=24");
    CHECK(!ecx::plan_crc(16, 0, 1, pl), "S=0");
    CHECK(!ecx::plan_crc(16, 65536, 1, pl), "S=65536");
    CHECK(!ecx::plan_crc(16, 1, 0, pl), "n=0");
    CHECK(!ecx::plan_crc(16, 1, 65, pl), "n=65");
    CHECK(!ecx::plan_crc((size_t)1 << 40, 65535, 64, pl), "grid overflow");
    CHECK(ecx::plan_crc(16, 65535, 64, pl), "largest word count");
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("crc_plan_check: ok\n");
  return 0;
}
