// crc_plan.cpp — see crc_plan.h.
#include "crc_plan.h"

#include <cstring>

namespace ecx {

namespace {

constexpr CrcTables kTab{};

#if defined(__x86_64__)
__attribute__((target("sse4.2"))) uint32_t crc32c_sse42(uint32_t crc,
                                                        const uint8_t *p,
                                                        size_t len) {
  // head to 8-byte alignment, 8 bytes per instruction, byte tail
  while (len && ((uintptr_t)p & 7)) {
    crc = __builtin_ia32_crc32qi(crc, *p++);
    len--;
  }
  uint64_t c = crc;
  for (; len >= 8; p += 8, len -= 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);
    c = __builtin_ia32_crc32di(c, w);
  }
  crc = (uint32_t)c;
  for (; len; len--) crc = __builtin_ia32_crc32qi(crc, *p++);
  return crc;
}

bool have_sse42() {
  static const bool v = __builtin_cpu_supports("sse4.2");
  return v;
}
#endif

}  // namespace

uint32_t crc32c_host_tables(uint32_t crc, const void *data, size_t len) {
  const uint8_t *p = (const uint8_t *)data;
  for (; len >= 4; p += 4, len -= 4) {
    uint32_t x = crc ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 |
                        (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    crc = kTab.t[3][x & 255] ^ kTab.t[2][(x >> 8) & 255] ^
          kTab.t[1][(x >> 16) & 255] ^ kTab.t[0][x >> 24];
  }
  for (; len; len--) crc = (crc >> 8) ^ kTab.t[0][(crc ^ *p++) & 255];
  return crc;
}

uint32_t crc32c_host(uint32_t seed, const void *data, size_t len, int *path) {
#if defined(__x86_64__)
  if (have_sse42()) {
    if (path) *path = 1;
    return crc32c_sse42(seed, (const uint8_t *)data, len);
  }
#endif
  if (path) *path = 0;
  return crc32c_host_tables(seed, data, len);
}

uint32_t crc32c_shift(uint32_t crc, uint64_t nbytes) {
  return crc_mulmod(crc, crc_xpow8(nbytes));
}

bool plan_crc(size_t chunk_bytes, long n_stripes, int n_chunks, CrcPlan &p) {
  if (chunk_bytes == 0 || chunk_bytes % 16 || n_stripes < 1 ||
      n_stripes > 65535 || n_chunks < 1 || n_chunks > 64)
    return false;
  const uint64_t bpc = (chunk_bytes + CRC_BLOCK_BYTES - 1) / CRC_BLOCK_BYTES;
  const uint64_t words = (uint64_t)n_stripes * (uint64_t)n_chunks;
  if (bpc > 0x7fffffffull / words) return false;
  p.seg_bytes = CRC_SEG_BYTES;
  p.segs_per_block = CRC_THREADS;
  p.blocks_per_chunk = (long)bpc;
  p.grid = (long)(words * bpc);
  p.threads = CRC_THREADS;
  p.lds_bytes = CRC_LDS_BYTES;
  p.launches = 2;
  return true;
}

void plan_crc_chain(size_t chunk_bytes, long n_stripes, CrcChainPlan &c) {
  constexpr long lanes = 1L << CRC_CHAIN_LOG2;
  c.run = (uint32_t)((n_stripes + lanes - 1) / lanes);
  c.x_chunk = crc_xpow8(chunk_bytes);
  uint32_t s = crc_xpow8((uint64_t)chunk_bytes * c.run);
  for (int i = 0; i < CRC_CHAIN_LOG2; i++) {
    c.x_step[i] = s;
    s = crc_mulmod(s, s);
  }
}

}  // namespace ecx
