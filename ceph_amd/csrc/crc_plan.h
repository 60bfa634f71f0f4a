// crc_plan.h — host side of the per-shard CRC-32C (ecx_crc32c_batch) and its
// CPU-only probes. Plain C++: no HIP, no device state, so the probes and the
// launcher run literally the same code and it can be tested (and sanitized)
// on a GPU-less box. The constant tables of the kernel are constexpr here, so
// the host routines and the device code cannot drift apart.
//
// The hash is ceph_crc32c(seed, data, len): the Castagnoli polynomial,
// reflected (0x82F63B78), no inversion of the seed or of the result. A CRC
// state is a polynomial over GF(2) modulo P; bit 31 of the word is x^0 and
// bit 0 is x^31. Feeding n zero bytes multiplies the state by x^(8n), and the
// hash is linear in (state, data), which gives the combine identity
//
//   f(seed, A||B) = shift(f(seed, A), |B|) ^ f(0, B),
//   shift(c, n)   = c * x^(8n) mod P.
//
// Leading zero bytes leave a zero state at zero, so a chunk may be thought of
// as padded IN FRONT to a whole number of blocks: the kernel's segments are
// aligned to the END of the chunk. Segment j from the end covers
// [C - (j+1)*L, C - j*L) (cut at 0), block j from the end [C - (j+1)*B,
// C - j*B); every segment is followed by a whole number of segments, so all
// combine constants are compile-time powers of x^(8L) and x^(8B).
#pragma once

#include <cstddef>
#include <cstdint>

namespace ecx {

constexpr uint32_t CRC32C_POLY = 0x82F63B78u;
constexpr uint32_t CRC_ONE = 0x80000000u;  // the polynomial 1

constexpr int CRC_SEG_BYTES = 128;  // L: bytes one lane hashes
constexpr int CRC_THREADS = 256;    // lanes (= segments) per block
constexpr int CRC_BLOCK_BYTES = CRC_SEG_BYTES * CRC_THREADS;  // B = 32 KiB
// LDS image of a block: segments at a stride of L + 16 bytes (conflict-free
// ds_read_b128 across lanes), then the four slice-by-4 tables.
constexpr int CRC_SEG_STRIDE = CRC_SEG_BYTES + 16;
constexpr int CRC_LDS_BYTES = CRC_SEG_STRIDE * CRC_THREADS + 4 * 256 * 4;

// a * b mod P
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 32; i++) {
    if (b & (CRC_ONE >> i)) r ^= a;
    a = (a >> 1) ^ ((a & 1) ? CRC32C_POLY : 0);  // a * x
  }
  return r;
}

// x^(8 * nbytes) mod P, by square and multiply
constexpr uint32_t crc_xpow8(uint64_t nbytes) {
  uint32_t r = CRC_ONE, b = CRC_ONE >> 8;  // x^8
  for (; nbytes; nbytes >>= 1) {
    if (nbytes & 1) r = crc_mulmod(r, b);
    b = crc_mulmod(b, b);
  }
  return r;
}

// Slice-by-4 tables: t[j][n] = the state after byte n and j zero bytes, from
// state 0. One dword w into state c: x = c ^ w;
// c' = t[3][x & 255] ^ t[2][(x >> 8) & 255] ^ t[1][(x >> 16) & 255] ^ t[0][x >> 24].
struct CrcTables {
  uint32_t t[4][256];
  constexpr CrcTables() : t{} {
    for (uint32_t n = 0; n < 256; n++) {
      uint32_t c = n;
      for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1) ? CRC32C_POLY : 0);
      t[0][n] = c;
    }
    for (int j = 1; j < 4; j++)
      for (int n = 0; n < 256; n++)
        t[j][n] = (t[j - 1][n] >> 8) ^ t[0][t[j - 1][n] & 255];
  }
};

// What the kernel multiplies partial hashes by: seg[t] = x^(8L(T-1-t)), the
// bytes that follow lane t's segment inside its block; blk[i] = x^(8B*2^i),
// from which a block raises x^(8B) to the number of blocks that follow it.
struct CrcCombine {
  uint32_t seg[CRC_THREADS];
  uint32_t blk[32];
  constexpr CrcCombine() : seg{}, blk{} {
    const uint32_t xl = crc_xpow8(CRC_SEG_BYTES);
    seg[CRC_THREADS - 1] = CRC_ONE;
    for (int t = CRC_THREADS - 2; t >= 0; t--)
      seg[t] = crc_mulmod(seg[t + 1], xl);
    blk[0] = crc_xpow8(CRC_BLOCK_BYTES);
    for (int i = 1; i < 32; i++) blk[i] = crc_mulmod(blk[i - 1], blk[i - 1]);
  }
};

// ceph_crc32c on the host: the SSE4.2 crc32 instruction where the CPU has it,
// slice-by-4 tables otherwise. *path (if given) = 1 for the instruction, 0
// for the tables.
uint32_t crc32c_host(uint32_t seed, const void *data, size_t len,
                     int *path = nullptr);
// The table path alone (what crc32c_host falls back to).
uint32_t crc32c_host_tables(uint32_t seed, const void *data, size_t len);
// crc * x^(8 nbytes) mod P
uint32_t crc32c_shift(uint32_t crc, uint64_t nbytes);

struct CrcPlan {
  long seg_bytes;          // L
  long segs_per_block;     // lanes per block
  long blocks_per_chunk;   // ceil(C / B), end-aligned
  long grid;               // n_stripes * n_chunks * blocks_per_chunk
  long threads;
  long lds_bytes;
  long launches;           // seed pass + hash pass (chain mode adds its scan)
};

// Plan the hash of n_chunks chunks of chunk_bytes in each of n_stripes
// stripes. False (p unspecified) for chunk_bytes 0 or not a multiple of 16,
// n_stripes outside 1..65535, n_chunks outside 1..64, or a grid that does not
// fit 31 bits.
bool plan_crc(size_t chunk_bytes, long n_stripes, int n_chunks, CrcPlan &p);

// The constants of the chain scan (one block of 2^CRC_CHAIN_LOG2 lanes per
// shard, each lane a run of `run` consecutive stripes): x^(8C), and
// x^(8C*run*2^i) for the log-step scan over the lanes' totals.
constexpr int CRC_CHAIN_LOG2 = 10;
struct CrcChainPlan {
  uint32_t run;      // stripes per lane = ceil(n_stripes / 2^CRC_CHAIN_LOG2)
  uint32_t x_chunk;  // x^(8C)
  uint32_t x_step[CRC_CHAIN_LOG2];
};
void plan_crc_chain(size_t chunk_bytes, long n_stripes, CrcChainPlan &c);

}  // namespace ecx
