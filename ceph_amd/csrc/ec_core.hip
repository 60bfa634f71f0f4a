// ec_core.hip — MI355X (gfx950, CDNA4) erasure-coding core:
// GF(2^8) matrix x stripe kernels + the C-ABI of include/ec_mi355x.h.
//
// This file REPLACES the reference's GF region libraries on the hot path
// (jerasure_matrix_encode / jerasure_matrix_decode, isa-l ec_encode_data —
// call sites src/erasure-code/jerasure/ErasureCodeJerasure.cc:382-396 and
// src/erasure-code/isa/ErasureCodeIsa.cc:289-300,566) with a CDNA4-native
// design. It is NOT a port: the reference libraries are CPU SIMD (pshufb
// split tables); here the same GF(2^8) linear algebra is laid out for
// 64-lane wavefronts and HBM3E streaming:
//
//  * One generic kernel shape: out[r][b] = XOR_i gfmul(C[r][i], src[i][b])
//    over a batch of stripes. Encode, decode (after host-side survivor
//    matrix inversion, mirroring ErasureCodeIsa.cc:510-567) and parity
//    delta-apply are all instances of it.
//  * GF(2^8) multiply by a wavefront-uniform coefficient c decomposes over
//    the XOR of disjoint bit groups: c*x = c*(x&7) ^ c*(x&8) ^ c*(x&0x70)
//    ^ c*(x&0x80). Each term is a <=8-entry byte lookup done 4 bytes at a
//    time with v_perm_b32 (__builtin_amdgcn_perm) from per-coefficient
//    tables staged in LDS — the CDNA analogue of the CPU pshufb approach,
//    but shaped so one lane processes 16 B per source per step with ~5
//    VALU ops per input byte, leaving the kernel HBM-bound (roofline:
//    (k+m)/k bytes moved per input byte).
//  * Coalesced 16 B/lane loads of the k data chunks and 16 B/lane stores of
//    parity; a 2-D grid (x = position tiles, y = stripes) so no per-thread
//    division; grid-stride so any chunk size >= 16 B multiple works.
//
// MFMA is deliberately unused: this is byte-table XOR arithmetic with no
// dense FP contraction.

#include <hip/hip_runtime.h>


#include <atomic>
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <list>
#include <map>
#include <chrono>
#include <condition_variable>
#include <thread>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ec_mi355x.h"
#include "gf.h"
#include "decode_multi.h"
#include "update_plan.h"
#include "verify_plan.h"
#include "locate_plan.h"
#include "crc_plan.h"
#include "slice_plan.h"
#include "bit_plan.h"
#include "stream_walk.h"

// ---------------------------------------------------------------------------
// Kernel-side
// ---------------------------------------------------------------------------

#define ECX_MAX_K 32     // matches isa MAX_K (ErasureCodeIsa.h:48)
#define ECX_MAX_OUT 8    // outputs per launch; host splits larger n_out

// the bitmatrix job headers are filled by bit_plan.cpp, which cannot see
// the two limits above
using ecx::EcBitParams;
using ecx::EcBitRegParams;
static_assert(ecx::BIT_MAX_K == ECX_MAX_K && ecx::BIT_MAX_OUT == ECX_MAX_OUT,
              "bit_plan.h restates ECX_MAX_K / ECX_MAX_OUT");

// Per-launch parameter block, copied to device scratch before each launch.
struct EcLaunchParams {
  int n_src;
  int n_out;
  int src_ids[ECX_MAX_K];
  int out_ids[ECX_MAX_OUT];
  // class per (out j, src i): 0 = skip (coeff 0 or zeros-chunk source),
  // 1 = plain XOR (coeff 1), 2 = table multiply
  uint8_t cls[ECX_MAX_OUT * ECX_MAX_K];
  // 6 dwords per (j,i): {lo03, lo47, lo8, hi03, hi47, hi8} (see lut16())
  uint32_t tabs[ECX_MAX_OUT * ECX_MAX_K * 6];
};

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// GF(2^8) multiply by wave-uniform c over 4 packed bytes, as three
// v_perm lookups (v_perm sel byte 0..3 picks from src1, 4..7 from src0):
//   c*x = T7l[x&7] ^ T7h[(x>>4)&7] ^ W[bit3(x) + 2*bit7(x)]
// where W[s] = c*(8*s0 ^ 128*s1) is a fused 4-entry table covering both
// high bits in ONE perm (saves a perm + xor per coefficient-dword vs the
// two 2-entry lookups).
__device__ __forceinline__ uint32_t ecx_gfmul4(uint32_t l0, uint32_t l1,
                                               uint32_t h0, uint32_t h1,
                                               uint32_t w, uint32_t i7l,
                                               uint32_t i7h, uint32_t i8) {
  return __builtin_amdgcn_perm(l1, l0, i7l) ^
         __builtin_amdgcn_perm(h1, h0, i7h) ^
         __builtin_amdgcn_perm(0u, w, i8);
}

// ---- shared pieces of the four table kernels (ec_gf_matmul_kernel,
// ec_gf_slices_kernel and their *_multi forms) ----

// Stage one launch record into the kernel's own LDS arrays. Rec is
// EcLaunchParams or EcMultiRec (same field names, different capacities).
template <int NOUT, class Rec>
__device__ __forceinline__ void ecx_stage_rec(const Rec* __restrict__ pb,
                                              int n_src, uint32_t* s_tabs,
                                              int* s_src, int* s_out,
                                              uint8_t* s_cls) {
  for (int t = threadIdx.x; t < NOUT * n_src * 6; t += blockDim.x)
    s_tabs[t] = pb->tabs[t];
  for (int t = threadIdx.x; t < n_src; t += blockDim.x)
    s_src[t] = pb->src_ids[t];
  for (int t = threadIdx.x; t < NOUT; t += blockDim.x)
    s_out[t] = pb->out_ids[t];
  for (int t = threadIdx.x; t < NOUT * n_src; t += blockDim.x)
    s_cls[t] = pb->cls[t];
  __syncthreads();
}

template <bool NT>
__device__ __forceinline__ v4u ecx_ld16(const uint8_t* p) {
  const v4u* p4 = reinterpret_cast<const v4u*>(p);
  return NT ? __builtin_nontemporal_load(p4) : *p4;
}

template <bool NT>
__device__ __forceinline__ void ecx_st16(uint8_t* p, v4u o) {
  v4u* p4 = reinterpret_cast<v4u*>(p);
  if (NT)
    __builtin_nontemporal_store(o, p4);
  else
    *p4 = o;
}

// One source vector into one output's accumulator by its class: 0 skip,
// 1 XOR, 2 table multiply. The accumulator goes in and out by value and is
// only ever touched whole: behind a reference, or updated dword by dword,
// the compiler fuses all NOUT of them into one wide vector that it copies
// at every class branch (+5 to +15 VGPRs at NOUT >= 3).
__device__ __forceinline__ v4u ecx_gf_out(int cls, const uint32_t* T, v4u d,
                                          v4u i7l, v4u i7h, v4u i8, v4u a) {
  if (cls == 1) {
    a ^= d;
  } else if (cls != 0) {
    const uint32_t l0 = T[0], l1 = T[1], h0 = T[2], h1 = T[3], w8 = T[4];
    v4u t;
#pragma unroll
    for (int q = 0; q < 4; q++)
      t[q] = ecx_gfmul4(l0, l1, h0, h1, w8, i7l[q], i7h[q], i8[q]);
    a ^= t;
  }
  return a;
}

// Source i's 16 B vector d into all NOUT accumulators: the index split of
// ecx_gfmul4 once per source, then ecx_gf_out per output.
template <int NOUT>
__device__ __forceinline__ void ecx_gf_source(const uint32_t* s_tabs,
                                              const uint8_t* s_cls, int n_src,
                                              int i, v4u d,
                                              v4u (&acc)[NOUT]) {
  const v4u i7l = d & 0x07070707u, i7h = (d >> 4) & 0x07070707u;
  const v4u i8 = ((d >> 3) & 0x01010101u) | ((d >> 6) & 0x02020202u);
#pragma unroll
  for (int j = 0; j < NOUT; j++)
    // cls is uniform across the wave (one record per block); readfirstlane
    // makes the branch a scalar s_cbranch instead of an exec-mask dance
    acc[j] = ecx_gf_out(__builtin_amdgcn_readfirstlane(s_cls[j * n_src + i]),
                        &s_tabs[(j * n_src + i) * 6], d, i7l, i7h, i8, acc[j]);
}

// Contiguous-batch body: one stripe (sbase/obase), grid-stride over its
// 16 B positions. PF = 1: one-ahead source prefetch — source i+1's load is
// issued before computing on source i, so each wave keeps a load in flight
// across the compute body (the i-loop otherwise serialises load -> use).
// Costs 4 VGPRs; targeted at the NOUT=4 shapes where the all-ones probe
// measured 15-20% of wall as VALU not hidden behind the stream. nthr is
// blockDim.x, read by the kernel ahead of the staging barrier (read here it
// costs a second, per-lane fetch after the barrier).
template <int NOUT, bool ACCUM, bool NT, int PF>
__device__ __forceinline__ void ecx_batch_body(
    const uint8_t* __restrict__ sbase, uint8_t* __restrict__ obase,
    long chunk_bytes, long vecs_per_chunk, int n_src, unsigned nthr,
    const uint32_t* s_tabs, const int* s_src, const int* s_out,
    const uint8_t* s_cls) {
  for (long p = (long)blockIdx.x * nthr + threadIdx.x; p < vecs_per_chunk;
       p += (long)gridDim.x * nthr) {
    const long off = p << 4;
    v4u acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      acc[j] = ACCUM ? *reinterpret_cast<const v4u*>(
                           obase + (long)s_out[j] * chunk_bytes + off)
                     : v4u{0, 0, 0, 0};
    v4u nxt = {0, 0, 0, 0};
    if (PF) nxt = ecx_ld16<NT>(sbase + (long)s_src[0] * chunk_bytes + off);
    for (int i = 0; i < n_src; i++) {
      v4u d;
      if (PF) {
        d = nxt;
        if (i + 1 < n_src)
          nxt = ecx_ld16<NT>(sbase + (long)s_src[i + 1] * chunk_bytes + off);
      } else {
        d = ecx_ld16<NT>(sbase + (long)s_src[i] * chunk_bytes + off);
      }
      ecx_gf_source<NOUT>(s_tabs, s_cls, n_src, i, d, acc);
    }
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      ecx_st16<NT>(obase + (long)s_out[j] * chunk_bytes + off, acc[j]);
  }
}

template <int NOUT, bool ACCUM, bool NT, int PF>
__global__ __launch_bounds__(256, 2) void ec_gf_matmul_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const EcLaunchParams* __restrict__ pb, long chunk_bytes,
    int chunks_per_stripe, long vecs_per_chunk) {
  __shared__ uint32_t s_tabs[ECX_MAX_OUT * ECX_MAX_K * 6];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MAX_OUT];
  __shared__ uint8_t s_cls[ECX_MAX_OUT * ECX_MAX_K];
  const int n_src = pb->n_src;
  const unsigned nthr = blockDim.x;
  ecx_stage_rec<NOUT>(pb, n_src, s_tabs, s_src, s_out, s_cls);
  const long sbytes = (long)blockIdx.y * chunks_per_stripe * chunk_bytes;
  ecx_batch_body<NOUT, ACCUM, NT, PF>(buf + sbytes, obuf + sbytes,
                                      chunk_bytes, vecs_per_chunk, n_src, nthr,
                                      s_tabs, s_src, s_out, s_cls);
}

// ---------------------------------------------------------------------------
// Streaming kernel for the non-accumulating batch matmul
// (DESIGN.md §4.1). Same arithmetic as ec_gf_matmul_kernel, different
// skeleton: every launch-uniform value (chunk offsets, coefficient classes,
// tables) lives in a by-value argument block, so it reaches the wave through
// scalar loads — no LDS staging, no barrier, no readfirstlane, and no
// device-side parameter buffer for the host to upload.
// ---------------------------------------------------------------------------

#define ECX_STREAM_MAX_OUT 4

struct EcStreamParams {
  // byte offset of each source / output chunk inside a stripe
  // (chunk id * chunk_bytes, formed on the host in 64 bits); padded because
  // the kernel fetches offsets two sources ahead of the one it computes
  uint64_t src_off[ECX_MAX_K + 2];
  uint64_t out_off[ECX_STREAM_MAX_OUT];
  // per output, one bit per source: coefficient == 1 / general coefficient
  // (neither bit: coefficient 0 or a zeros-chunk source)
  uint32_t one_mask[ECX_STREAM_MAX_OUT];
  uint32_t mul_mask[ECX_STREAM_MAX_OUT];
  // 5 dwords per (source, output), see build_tabs332(); zero where the
  // coefficient is not a general one
  uint32_t tabs[ECX_MAX_K][ECX_STREAM_MAX_OUT][5];
  int n_src;
  // ec_gf_verify_kernel only: chunk id of each output (< 64), the bit it
  // reports under. Sits in what was tail padding, so the block keeps its size
  // and the stream kernel its argument layout.
  uint8_t out_id[ECX_STREAM_MAX_OUT];
};
static_assert(sizeof(EcStreamParams) <= 4096,
              "EcStreamParams must fit the kernel argument segment");
static_assert(ECX_MAX_K <= 32, "source classes are 32-bit masks");
static_assert(offsetof(EcStreamParams, out_id) + ECX_STREAM_MAX_OUT ==
                  sizeof(EcStreamParams),
              "out_id fills the tail padding");

// One source's contribution to every output accumulator. The byte is split
// into the contiguous bit groups 0-2, 3-5, 6-7 (5 VALU per dword):
//   c*x = A[x & 7] ^ B[(x >> 3) & 7] ^ W[x >> 6]
template <int NOUT>
__device__ __forceinline__ void ecx_stream_source(
    const EcStreamParams& p, const uint32_t (&one_mask)[NOUT],
    const uint32_t (&mul_mask)[NOUT], int i, v4u d,
    uint32_t (&acc)[NOUT][4]) {
  uint32_t T[NOUT][5];
#pragma unroll
  for (int j = 0; j < NOUT; j++)
#pragma unroll
    for (int q = 0; q < 5; q++) T[j][q] = p.tabs[i][j][q];
  const uint32_t x[4] = {d.x, d.y, d.z, d.w};
  uint32_t ia[4], ib[4], ic[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    ia[q] = x[q] & 0x07070707u;
    ib[q] = (x[q] >> 3) & 0x07070707u;
    ic[q] = (x[q] >> 6) & 0x03030303u;
  }
  const uint32_t bit = 1u << i;
#pragma unroll
  for (int j = 0; j < NOUT; j++) {
    // the classes merge in a 4-register term, never in the accumulators:
    // merging acc itself makes the compiler copy all of them per source
    uint32_t t[4];
    if (mul_mask[j] & bit) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        t[q] = __builtin_amdgcn_perm(T[j][1], T[j][0], ia[q]) ^
               __builtin_amdgcn_perm(T[j][3], T[j][2], ib[q]) ^
               __builtin_amdgcn_perm(0u, T[j][4], ic[q]);
    } else {
      const uint32_t keep = (one_mask[j] & bit) ? ~0u : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) t[q] = x[q] & keep;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) acc[j][q] ^= t[q];
  }
}

// All n_src sources of one tile position (sb = tile base, voff = the lane's
// 16 B) into the accumulators: the source loop of ec_gf_stream_kernel and
// ec_gf_verify_kernel.
// One-ahead prefetch over two load buffers used alternately: the load of
// source i + 1 is in flight while source i is computed. Every load in the
// loop is unconditional (the last one or two sources are peeled), so each
// wait leaves exactly one load outstanding, and no loaded register is ever
// copied (a copy would wait for its load). The offset of the load after next
// is fetched (a scalar load) while the current one is issued, and the
// scheduling barrier keeps each vector load ahead of the compute it
// overlaps: without it the compiler hoists the compute's head above the load
// to cover the offset fetch, and the wait for the previous load goes with it.
template <int NOUT>
__device__ __forceinline__ void ecx_stream_sources(
    const EcStreamParams& p, const uint32_t (&one_mask)[NOUT],
    const uint32_t (&mul_mask)[NOUT], int n_src, const uint8_t* sb,
    uint32_t voff, uint32_t (&acc)[NOUT][4]) {
#define ECX_STREAM_LD(dst_, next_)                                        \
  do {                                                                    \
    dst_ = __builtin_nontemporal_load(                                    \
        reinterpret_cast<const v4u*>(sb + so + voff));                    \
    so = p.src_off[next_];                                                \
    __builtin_amdgcn_sched_barrier(0);                                    \
  } while (0)
  uint64_t so = p.src_off[0];
  v4u d0, d1;
  ECX_STREAM_LD(d0, 1);
  int i = 0;
  for (; i + 2 < n_src; i += 2) {
    ECX_STREAM_LD(d1, i + 2);
    ecx_stream_source<NOUT>(p, one_mask, mul_mask, i, d0, acc);
    ECX_STREAM_LD(d0, i + 3);  // src_off is padded: index <= n_src + 1
    ecx_stream_source<NOUT>(p, one_mask, mul_mask, i + 1, d1, acc);
  }
  if (i + 1 < n_src) {
    ECX_STREAM_LD(d1, 0);
    ecx_stream_source<NOUT>(p, one_mask, mul_mask, i, d0, acc);
    ecx_stream_source<NOUT>(p, one_mask, mul_mask, i + 1, d1, acc);
  } else {
    ecx_stream_source<NOUT>(p, one_mask, mul_mask, i, d0, acc);
  }
#undef ECX_STREAM_LD
}

// A tile is 256 lanes x 16 B of one chunk position range of one stripe.
// Which tiles a block takes, and in which order, is the walk of
// stream_walk.h: every value of it is launch-uniform and host-computed, the
// position lives in SGPRs and a step is three adds with carries. The grid
// may be anything from one block per tile to a persistent one.
// Register budget: 8 waves/SIMD (<= 64 VGPRs) for NOUT <= 3; NOUT = 4 needs
// about 73 and would spill at 64, so it is asked for 6.
template <int NOUT>
__global__ __launch_bounds__(256, NOUT < 4 ? 8 : 6) void ec_gf_stream_kernel(
    const uint8_t* buf, uint8_t* obuf, const EcStreamParams p,
    uint64_t stripe_bytes, uint64_t vecs_per_chunk, const EcxWalk walk) {
  const uint32_t voff = threadIdx.x << 4;
  const int n_src = p.n_src;
  uint32_t one_mask[NOUT], mul_mask[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; j++) {
    one_mask[j] = p.one_mask[j];
    mul_mask[j] = p.mul_mask[j];
  }
  EcxWalkPos pos = ecx_walk_start(walk, blockIdx.x);
  while (ecx_walk_live(walk, pos)) {
    const uint32_t stripe = ecx_walk_stripe(walk, pos);
    const uint32_t tile = pos.t;
    // wave-uniform 64-bit base; the per-lane part stays a 32-bit offset
    const uint64_t tbase =
        (uint64_t)stripe * stripe_bytes + ((uint64_t)tile << 12);
    // stripe >= n_stripes: the skipped end of a last, narrower stripe group
    if (stripe < walk.n_stripes &&
        ((uint64_t)tile << 8) + threadIdx.x < vecs_per_chunk) {
      const uint8_t* sb = buf + tbase;
      uint32_t acc[NOUT][4];
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0u;
      ecx_stream_sources<NOUT>(p, one_mask, mul_mask, n_src, sb, voff, acc);
      uint8_t* ob = obuf + tbase;
#pragma unroll
      for (int j = 0; j < NOUT; j++) {
        v4u o;
        o.x = acc[j][0]; o.y = acc[j][1]; o.z = acc[j][2]; o.w = acc[j][3];
        __builtin_nontemporal_store(
            o, reinterpret_cast<v4u*>(ob + p.out_off[j] + voff));
      }
    }
    ecx_walk_next(walk, pos);
  }
}

// Consistency check (ecx_verify_batch): the stream kernel
// with another epilogue. The NOUT "outputs" are stored chunks; each is
// recomputed from the sources as above, then the stored vector is loaded and
// compared where the stream kernel would store. A wave in which any lane
// differs sets bit out_id[j] of the stripe's word with one atomicOr from one
// lane; a clean tile issues no atomic and no store at all. The batch is only
// read. bad[] is zeroed by the host ahead of the launch.
// The ballot sits inside the tile guard, so lanes beyond the chunk (partial
// last tile) and the skipped end of a narrow last stripe group do not vote.
// The stored chunks are not sources: they are loaded by out_off after the
// source loop, when its two load buffers are free, so k = 32 keeps its 32
// source-class bits.
template <int NOUT>
__global__ __launch_bounds__(256, NOUT < 4 ? 8 : 6) void ec_gf_verify_kernel(
    const uint8_t* buf, unsigned long long* bad, const EcStreamParams p,
    uint64_t stripe_bytes, uint64_t vecs_per_chunk, const EcxWalk walk) {
  const uint32_t voff = threadIdx.x << 4;
  const int n_src = p.n_src;
  uint32_t one_mask[NOUT], mul_mask[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; j++) {
    one_mask[j] = p.one_mask[j];
    mul_mask[j] = p.mul_mask[j];
  }
  EcxWalkPos pos = ecx_walk_start(walk, blockIdx.x);
  while (ecx_walk_live(walk, pos)) {
    const uint32_t stripe = ecx_walk_stripe(walk, pos);
    const uint32_t tile = pos.t;
    const uint64_t tbase =
        (uint64_t)stripe * stripe_bytes + ((uint64_t)tile << 12);
    if (stripe < walk.n_stripes &&
        ((uint64_t)tile << 8) + threadIdx.x < vecs_per_chunk) {
      const uint8_t* sb = buf + tbase;
      uint32_t acc[NOUT][4];
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0u;
      ecx_stream_sources<NOUT>(p, one_mask, mul_mask, n_src, sb, voff, acc);
      // all NOUT stored vectors in flight together, then compared
      v4u st[NOUT];
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        st[j] = __builtin_nontemporal_load(
            reinterpret_cast<const v4u*>(sb + p.out_off[j] + voff));
#pragma unroll
      for (int j = 0; j < NOUT; j++) {
        const uint32_t diff = (acc[j][0] ^ st[j].x) | (acc[j][1] ^ st[j].y) |
                              (acc[j][2] ^ st[j].z) | (acc[j][3] ^ st[j].w);
        // wave-uniform, so the branch is scalar
        const unsigned long long vote = __ballot(diff != 0u);
        if (vote != 0ull) {
          // The bit is formed behind the branch: the empty asm keeps the
          // compiler from hoisting 1 << id out of the tile loop into a VGPR
          // pair per output, which is 12 B/lane of scratch at NOUT = 3.
          uint32_t id = p.out_id[j];
          asm volatile("" : "+s"(id));
          // the first differing lane (it voted, so it is active) reports
          if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)vote) - 1u)
            atomicOr(&bad[stripe], 1ull << id);
        }
      }
    }
    ecx_walk_next(walk, pos);
  }
}

// Variable-size slice batch: one launch over N independent
// slices of differing length, each with its own k+m device chunk pointers.
// Blocks are pre-assigned (slice id, vec offset) by the host so there is no
// per-thread search; a NULL data pointer means a zeros chunk for that slice
// only (wave-uniform skip).
template <int NOUT, bool NT>
__device__ __forceinline__ void ecx_slices_body(
    const uint64_t* __restrict__ chunk_ptrs,
    const int* __restrict__ block_slice, const long* __restrict__ block_voff,
    const long* __restrict__ slice_vecs, int cps, int vecs_per_block,
    int n_src, const uint32_t* s_tabs, const int* s_src, const int* s_out,
    const uint8_t* s_cls) {
  const int sl = block_slice[blockIdx.x];
  const long v0 = block_voff[blockIdx.x];
  const long nv = slice_vecs[sl];
  const long vend = v0 + vecs_per_block < nv ? v0 + vecs_per_block : nv;
  const uint64_t* ptrs = chunk_ptrs + (long)sl * cps;

  for (long p = v0 + threadIdx.x; p < vend; p += blockDim.x) {
    const long off = p << 4;
    v4u acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; j++) acc[j] = v4u{0, 0, 0, 0};
    for (int i = 0; i < n_src; i++) {
      const uint8_t* sp = (const uint8_t*)ptrs[s_src[i]];
      if (sp == nullptr) continue;  // zeros chunk for this slice
      ecx_gf_source<NOUT>(s_tabs, s_cls, n_src, i, ecx_ld16<NT>(sp + off),
                          acc);
    }
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      ecx_st16<NT>((uint8_t*)ptrs[s_out[j]] + off, acc[j]);
  }
}

template <int NOUT, bool NT>
__global__ __launch_bounds__(256, 2) void ec_gf_slices_kernel(
    const uint64_t* __restrict__ chunk_ptrs,  // [n_slices * cps]
    const int* __restrict__ block_slice,      // [gridDim.x]
    const long* __restrict__ block_voff,      // [gridDim.x]
    const long* __restrict__ slice_vecs,      // [n_slices]
    const EcLaunchParams* __restrict__ pb, int cps, int vecs_per_block) {
  __shared__ uint32_t s_tabs[ECX_MAX_OUT * ECX_MAX_K * 6];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MAX_OUT];
  __shared__ uint8_t s_cls[ECX_MAX_OUT * ECX_MAX_K];
  const int n_src = pb->n_src;
  ecx_stage_rec<NOUT>(pb, n_src, s_tabs, s_src, s_out, s_cls);
  ecx_slices_body<NOUT, NT>(chunk_ptrs, block_slice, block_voff, slice_vecs,
                            cps, vecs_per_block, n_src, s_tabs, s_src, s_out,
                            s_cls);
}

// ---- per-stripe erasure patterns (ecx_decode_*_multi) ----
// A recovery batching shim collects degraded reads from many placement
// groups, so neighbouring stripes of one batch miss different chunks. The
// kernels above take ONE parameter block per launch; these variants take a
// device-resident table of compact launch records and let every block pick
// its own: blockIdx.y -> stripe_list[y] -> plan_of_stripe[stripe] -> record.
// The host buckets stripes by output count (NOUT is a template parameter),
// so the number of launches is independent of how many patterns the call
// holds (decode_multi.h). Record load costs the same as the load from `pb`
// above; cls stays wave-uniform because the record is per block.
#define ECX_MULTI_OUT 4  // == ecx::MULTI_MAX_OUT

// One <= 4-output pass of one erasure pattern: fill_params' output cut down
// to the 4 outputs a launch can carry (3.3 KB instead of 7.3 KB — the table
// holds one per distinct pattern and pass and is uploaded per call).
struct EcMultiRec {
  int src_ids[ECX_MAX_K];
  int out_ids[ECX_MULTI_OUT];
  uint8_t cls[ECX_MULTI_OUT * ECX_MAX_K];        // [j * n_src + i]
  uint32_t tabs[ECX_MULTI_OUT * ECX_MAX_K * 6];  // [(j * n_src + i) * 6]
};

// Decode is in place: sources (survivors) and outputs (erased) of a stripe
// are disjoint chunks, so buf/obuf may both be __restrict__ and passes of
// one stripe do not interfere.
template <int NOUT, bool NT, int PF>
__global__ __launch_bounds__(256, 2) void ec_gf_matmul_multi_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const EcMultiRec* __restrict__ recs,       // [n_plans * n_pass]
    const int* __restrict__ plan_of_stripe,    // [n_stripes]
    const int* __restrict__ stripe_list,       // [gridDim.y]
    int n_src, int pass, int n_pass, long chunk_bytes, int chunks_per_stripe,
    long vecs_per_chunk) {
  __shared__ uint32_t s_tabs[ECX_MULTI_OUT * ECX_MAX_K * 6];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MULTI_OUT];
  __shared__ uint8_t s_cls[ECX_MULTI_OUT * ECX_MAX_K];
  const long stripe = stripe_list[blockIdx.y];
  const unsigned nthr = blockDim.x;
  ecx_stage_rec<NOUT>(recs + ((long)plan_of_stripe[stripe] * n_pass + pass),
                      n_src, s_tabs, s_src, s_out, s_cls);
  const long sbytes = stripe * chunks_per_stripe * chunk_bytes;
  ecx_batch_body<NOUT, false, NT, PF>(buf + sbytes, obuf + sbytes,
                                      chunk_bytes, vecs_per_chunk, n_src, nthr,
                                      s_tabs, s_src, s_out, s_cls);
}

// Slices form: the per-block (slice, voff) table gains the record index;
// the host buckets the block lists by output count like the stripe lists
// above. A NULL survivor pointer still means zeros for that slice only.
template <int NOUT, bool NT>
__global__ __launch_bounds__(256, 2) void ec_gf_slices_multi_kernel(
    const uint64_t* __restrict__ chunk_ptrs,  // [n_slices * cps]
    const int* __restrict__ block_slice,      // [gridDim.x]
    const long* __restrict__ block_voff,      // [gridDim.x]
    const int* __restrict__ block_rec,        // [gridDim.x]
    const long* __restrict__ slice_vecs,      // [n_slices]
    const EcMultiRec* __restrict__ recs, int n_src, int cps,
    int vecs_per_block) {
  __shared__ uint32_t s_tabs[ECX_MULTI_OUT * ECX_MAX_K * 6];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MULTI_OUT];
  __shared__ uint8_t s_cls[ECX_MULTI_OUT * ECX_MAX_K];
  ecx_stage_rec<NOUT>(recs + block_rec[blockIdx.x], n_src, s_tabs, s_src,
                      s_out, s_cls);
  ecx_slices_body<NOUT, NT>(chunk_ptrs, block_slice, block_voff, slice_vecs,
                            cps, vecs_per_block, n_src, s_tabs, s_src, s_out,
                            s_cls);
}

// ---- parity-delta writes over a batch (ecx_update_batch) ----
// A write queue overwrites a different set of data chunks in every stripe:
// P_r ^= G[k+r][j] * (old_j ^ new_j) for each written chunk j, then chunk j
// takes its new content (matrix_apply_delta over the batch,
// ErasureCodeJerasure.cc:285-331 / ErasureCodeIsa.cc:333-366). The record is
// the ENCODE record of one <= 4-parity pass (k sources), the same for every
// stripe; a block resolves blockIdx.y -> active[y] -> stripe -> write mask
// and stages only the columns of the chunks its stripe writes, so the source
// loop is popcount(mask) long and unwritten data chunks are never read.
// cls stays wave-uniform because the staged record is per block.
//
// The data stores alias the old-data loads (same address, same lane, load
// first) and the parity stores alias the parity loads, so buf carries no
// __restrict__; d_new lies outside the batch (checked by the host). The
// delta cannot be re-formed once the old data is gone: with m > 4 only the
// last pass (LAST) stores the new data, earlier passes read old and new
// again and leave the data alone.
template <int NOUT, bool NT, bool LAST>
__global__ __launch_bounds__(256, 2) void ec_gf_update_kernel(
    uint8_t* buf, const uint8_t* __restrict__ d_new,
    const EcMultiRec* __restrict__ rec,        // this pass, k sources
    const uint64_t* __restrict__ write_masks,  // [n_stripes]
    const int* __restrict__ new_base,          // [n_stripes]
    const int* __restrict__ active,            // [gridDim.y]
    int k, long chunk_bytes, int chunks_per_stripe, long vecs_per_chunk) {
  __shared__ uint32_t s_tabs[ECX_MULTI_OUT * ECX_MAX_K * 6];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MULTI_OUT];
  __shared__ uint8_t s_cls[ECX_MULTI_OUT * ECX_MAX_K];
  const long stripe = active[blockIdx.y];
  const uint32_t mask = (uint32_t)write_masks[stripe];  // bits < k <= 32
  const int n_src = __builtin_popcount(mask);
  const unsigned nthr = blockDim.x;
  // one (output j, written chunk t) column per thread: at most 4 * 32
  for (int c = threadIdx.x; c < NOUT * n_src; c += nthr) {
    const int j = c / n_src, t = c - j * n_src;
    uint32_t rest = mask;
    for (int i = 0; i < t; i++) rest &= rest - 1;  // drop the t lowest bits
    const int id = __builtin_ctz(rest);
    const uint32_t* T = &rec->tabs[(j * k + id) * 6];
#pragma unroll
    for (int q = 0; q < 6; q++) s_tabs[c * 6 + q] = T[q];
    s_cls[c] = rec->cls[j * k + id];
    if (j == 0) s_src[t] = id;
  }
  for (int t = threadIdx.x; t < NOUT; t += nthr) s_out[t] = rec->out_ids[t];
  __syncthreads();

  uint8_t* sb = buf + stripe * chunks_per_stripe * chunk_bytes;
  const uint8_t* nb = d_new + (long)new_base[stripe] * chunk_bytes;
  for (long p = (long)blockIdx.x * nthr + threadIdx.x; p < vecs_per_chunk;
       p += (long)gridDim.x * nthr) {
    const long off = p << 4;
    // the body is short (one or two sources): parity and the first source's
    // two loads are all in flight before the first use
    v4u acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      acc[j] = ecx_ld16<NT>(sb + (long)s_out[j] * chunk_bytes + off);
    v4u old = ecx_ld16<NT>(sb + (long)s_src[0] * chunk_bytes + off);
    v4u nw = ecx_ld16<NT>(nb + off);
    for (int t = 0; t < n_src; t++) {
      const v4u d = old ^ nw, keep = nw;
      if (t + 1 < n_src) {
        old = ecx_ld16<NT>(sb + (long)s_src[t + 1] * chunk_bytes + off);
        nw = ecx_ld16<NT>(nb + (long)(t + 1) * chunk_bytes + off);
      }
      ecx_gf_source<NOUT>(s_tabs, s_cls, n_src, t, d, acc);
      if (LAST) ecx_st16<NT>(sb + (long)s_src[t] * chunk_bytes + off, keep);
    }
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      ecx_st16<NT>(sb + (long)s_out[j] * chunk_bytes + off, acc[j]);
  }
}

// ---- GF(2^16) (w=16 jerasure RS-van) path ----
// Symbols are u16 LE (galois_w16_region_multiply semantics). A coefficient
// multiply decomposes over the four nibbles of x plus the two fused
// bit3/bit7-style tables per 8-bit half:
//   c*x = T0[n0&7] ^ T1[n1&7] ^ T2[n2&7] ^ T3[n3&7]
//         ^ W01[b3+2*b7] ^ W23[b11+2*b15]
// Each term is a u16; its lo/hi byte planes are looked up with separate
// v_perms into separate plane accumulators (selector bytes are replicated
// per symbol), merged once per output dword with a constant-selector perm.
// ~24 VALU per coefficient-dword => compute-bound (~1.7-2 TB/s) — w=16 is
// a compatibility technique, not the fast path.
struct EcLaunch16 {
  int n_src;
  int n_out;
  int src_ids[ECX_MAX_K];
  int out_ids[ECX_MAX_OUT];
  uint8_t cls[ECX_MAX_OUT * ECX_MAX_K];
  // 20 dwords per (j,i): per plane P in {lo,hi}:
  //  [T0 pair][T1 pair][T2 pair][T3 pair][W01][W23] = 10 dwords
  uint32_t tabs[ECX_MAX_OUT * ECX_MAX_K * 20];
};

#define ECX_PLANE_MERGE_SEL 0x07020500u  // out = [L.b0, H.b1, L.b2, H.b3]

template <int NOUT, bool ACCUM, bool NT>
__global__ __launch_bounds__(256, 2) void ec_gf16_matmul_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const uint8_t* __restrict__ blob, long chunk_bytes,
    int chunks_per_stripe, long vecs_per_chunk) {
  const EcLaunch16* pb = (const EcLaunch16*)blob;
  __shared__ uint32_t s_tabs[ECX_MAX_OUT * ECX_MAX_K * 20];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[ECX_MAX_OUT];
  __shared__ uint8_t s_cls[ECX_MAX_OUT * ECX_MAX_K];
  const int n_src = pb->n_src;
  for (int t = threadIdx.x; t < NOUT * n_src * 20; t += blockDim.x)
    s_tabs[t] = pb->tabs[t];
  for (int t = threadIdx.x; t < n_src; t += blockDim.x)
    s_src[t] = pb->src_ids[t];
  for (int t = threadIdx.x; t < NOUT; t += blockDim.x)
    s_out[t] = pb->out_ids[t];
  for (int t = threadIdx.x; t < NOUT * n_src; t += blockDim.x)
    s_cls[t] = pb->cls[t];
  __syncthreads();

  const long stripe = blockIdx.y;
  const uint8_t* sbase = buf + stripe * chunks_per_stripe * chunk_bytes;
  uint8_t* obase = obuf + stripe * chunks_per_stripe * chunk_bytes;

  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
       p < vecs_per_chunk; p += (long)gridDim.x * blockDim.x) {
    const long off = p << 4;
    uint32_t aL[NOUT][4], aH[NOUT][4], aX[NOUT][4];
#pragma unroll
    for (int j = 0; j < NOUT; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        aL[j][q] = aH[j][q] = 0u;
        if (ACCUM) {
          const v4u o = *reinterpret_cast<const v4u*>(
              obase + (long)s_out[j] * chunk_bytes + off);
          aX[j][q] = o[q];
        } else {
          aX[j][q] = 0u;
        }
      }

    for (int i = 0; i < n_src; i++) {
      const uint8_t* sp = sbase + (long)s_src[i] * chunk_bytes;
      const v4u* p4 = reinterpret_cast<const v4u*>(sp + off);
      const v4u d = NT ? __builtin_nontemporal_load(p4) : *p4;
      const uint32_t dq[4] = {d.x, d.y, d.z, d.w};
      // selectors (shared across output rows)
      uint32_t i7[4][4], w01[4], w23[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int np = 0; np < 4; np++) {
          uint32_t nv = (dq[q] >> (4 * np)) & 0x000F000Fu;
          nv |= nv << 8;
          i7[np][q] = nv & 0x07070707u;
        }
        uint32_t w = ((dq[q] >> 3) & 0x00010001u) |
                     ((dq[q] >> 6) & 0x00020002u);
        w01[q] = w | (w << 8);
        w = ((dq[q] >> 11) & 0x00010001u) | ((dq[q] >> 14) & 0x00020002u);
        w23[q] = w | (w << 8);
      }
#pragma unroll
      for (int j = 0; j < NOUT; j++) {
        const int cls = __builtin_amdgcn_readfirstlane(s_cls[j * n_src + i]);
        if (cls == 0) continue;
        if (cls == 1) {
#pragma unroll
          for (int q = 0; q < 4; q++) aX[j][q] ^= dq[q];
        } else {
          const uint32_t* T = &s_tabs[(j * n_src + i) * 20];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            uint32_t l = __builtin_amdgcn_perm(T[1], T[0], i7[0][q]) ^
                         __builtin_amdgcn_perm(T[3], T[2], i7[1][q]) ^
                         __builtin_amdgcn_perm(T[5], T[4], i7[2][q]) ^
                         __builtin_amdgcn_perm(T[7], T[6], i7[3][q]) ^
                         __builtin_amdgcn_perm(0u, T[8], w01[q]) ^
                         __builtin_amdgcn_perm(0u, T[9], w23[q]);
            uint32_t h = __builtin_amdgcn_perm(T[11], T[10], i7[0][q]) ^
                         __builtin_amdgcn_perm(T[13], T[12], i7[1][q]) ^
                         __builtin_amdgcn_perm(T[15], T[14], i7[2][q]) ^
                         __builtin_amdgcn_perm(T[17], T[16], i7[3][q]) ^
                         __builtin_amdgcn_perm(0u, T[18], w01[q]) ^
                         __builtin_amdgcn_perm(0u, T[19], w23[q]);
            aL[j][q] ^= l;
            aH[j][q] ^= h;
          }
        }
      }
    }

#pragma unroll
    for (int j = 0; j < NOUT; j++) {
      v4u o;
#pragma unroll
      for (int q = 0; q < 4; q++)
        o[q] = aX[j][q] ^ __builtin_amdgcn_perm(aH[j][q], aL[j][q],
                                                ECX_PLANE_MERGE_SEL);
      v4u* dp = reinterpret_cast<v4u*>(obase + (long)s_out[j] * chunk_bytes +
                                       off);
      if (NT)
        __builtin_nontemporal_store(o, dp);
      else
        *dp = o;
    }
  }
}

// ---- jerasure bitmatrix (Cauchy-original) path ----
// Packet-sliced XOR gather: each chunk is a stream of superwords (w packets
// of `pkt` bytes); coding packet row r = XOR of the data packets its bit
// row selects (companion-basis GF(2^8), see gf.cpp matrix_to_bitmatrix).
// A naive gather would re-read each data packet ~m*w/2 times from HBM; this
// kernel stages a q-byte window of all k*w packets in LDS once and computes
// every output row from LDS, keeping HBM traffic algorithmic ((k+m)/k) —
// the CDNA-native answer to jerasure's CPU XOR schedules.
// EcBitParams (the job header both LDS kernels read) is in bit_plan.h.

// One wave's DMA of the 64 consecutive window items from t0 into an LDS
// image (global_load_lds_dwordx4): the image is lane-linear in the item
// index (byte offset = t*16), exactly the wave-uniform-base + lane*16
// layout the instruction writes. Unlike the v1 register-staged loop (1
// outstanding load per thread -> the chip sat latency-starved: PMC
// SQ_WAIT_ANY/WAVE 0.79, LDS 4% active), every load of the phase is in
// flight at once and there is no ds_write pass. aux=2 (nt) on the NT path:
// each window is read once by exactly one workgroup. Item t is 16 B vector
// v of packet c of source j, t = ((j*w + c) << vq_shift) + v.
template <bool NT>
__device__ __forceinline__ void ecx_bit_glds(
    const EcBitParams* bp, const uint8_t* sbase, long chunk_bytes,
    long sw_off, int pkt, int w, int vq_shift, uint8_t* image, int t0,
    int lane) {
  const int t = t0 + lane;
  const int jc = t >> vq_shift;
  const int v = t - (jc << vq_shift);
  const int j = jc / w, c = jc - j * w;
  const uint8_t* src = sbase + (long)bp->src_ids[j] * chunk_bytes + sw_off +
                       (long)c * pkt + (long)v * 16;
  auto gsrc = (const __attribute__((address_space(1))) uint32_t*)src;
  auto ldst =
      (__attribute__((address_space(3))) uint32_t*)(image + (size_t)t0 * 16);
  if (NT)
    __builtin_amdgcn_global_load_lds(gsrc, ldst, 16, 0, 2);
  else
    __builtin_amdgcn_global_load_lds(gsrc, ldst, 16, 0, 0);
}

// The output rows of window `win` of superword `sw` from its LDS image and
// the staged op list. Item-parallel (one 16B vec of one output row per
// item): A/B showed this beats a row-per-wave readlane variant — with q=512
// the row-per-wave form idles half of each wave (vq=32) and larger q
// collapses residency; LDS op reads broadcast cheaply.
template <bool NT, bool ACCUM>
__device__ __forceinline__ void ecx_bit_rows(
    const EcBitParams* bp, uint8_t* obase, long chunk_bytes, long sw, int win,
    int pkt, int w, int q, int vq, int vq_shift, int n_rows,
    const uint8_t* image, const uint16_t* s_ops) {
  for (int t = threadIdx.x; t < n_rows * vq; t += blockDim.x) {
    const int r = t >> vq_shift;
    const int v = t - (r << vq_shift);
    const int orig = bp->row_map[r];
    v4u* dst = reinterpret_cast<v4u*>(
        obase + (long)bp->out_ids[orig / w] * chunk_bytes +
        sw * (long)w * pkt + (long)(orig % w) * pkt + (long)win * q +
        (long)v * 16);
    // ACCUM = parity-delta apply (schedule_apply_delta semantics,
    // ErasureCodeJerasure.cc:348-377): XOR into the existing parity
    v4u acc = ACCUM ? *dst : v4u{0, 0, 0, 0};
    const int b0 = bp->row_off[r], b1 = bp->row_off[r + 1];
    for (int o = b0; o < b1; o++) {
      const int jc = s_ops[o];
      const v4u d = *reinterpret_cast<const v4u*>(image + (size_t)jc * q +
                                                  (size_t)v * 16);
      acc.x ^= d.x; acc.y ^= d.y; acc.z ^= d.z; acc.w ^= d.w;
    }
    if (NT)
      __builtin_nontemporal_store(acc, dst);
    else
      *dst = acc;
  }
}

// VQS >= 0 specialises the window geometry at compile time (w = 8,
// q = 16 << VQS): the generic form's runtime divisions/shifts and
// loop bounds cost ~15% against the measured ladder probe of the same
// structure (tools/membench.hip stage_pattern: static 4.94 TB/s vs the
// generic kernel's 4.23 at the same HBM pattern).
template <bool NT, bool ACCUM = false, int VQS = -1>
__global__ __launch_bounds__(256, 2) void ec_bitmatrix_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const uint8_t* __restrict__ blob, long chunk_bytes, int cps,
    int windows_per_sw, int wpb, long n_windows, int stagger, int xcdmap) {
  // Optional start-phase stagger (knob ECX_BITSTAGGER): co-resident
  // blocks otherwise run their DMA-wait / compute phases in lockstep
  // (dispatched together, identical per-window timing), leaving HBM idle
  // during every block's compute segment — PMC shows 73% wave-parked
  // with LDS/VALU both < 20% busy. A one-time per-block phase offset
  // breaks the convoy; offsets persist because the cycle time is uniform.
  if (stagger) {
    const int ph = (int)(blockIdx.x + blockIdx.y) & 7;
    for (int i = 0; i < ph * stagger; i++) __builtin_amdgcn_s_sleep(8);
  }
  const EcBitParams* bp = (const EcBitParams*)blob;
  const uint32_t* g_ops = (const uint32_t*)(blob + sizeof(EcBitParams));
  extern __shared__ uint8_t smem[];
  const int n_src = bp->n_src, pkt = bp->pkt;
  const int w = VQS >= 0 ? 8 : bp->w;
  const int q = VQS >= 0 ? (16 << VQS) : bp->q;
  const int vq = q >> 4, vq_shift = VQS >= 0 ? VQS : bp->vq_shift;
  const int n_rows = bp->n_out * w;
  uint8_t* s_data = smem;                       // n_src*w*q bytes
  uint16_t* s_ops = (uint16_t*)(smem + (size_t)n_src * w * q);
  const int n_ops = bp->row_off[n_rows];
  // ops staged once per block (dword copies; host pads the blob), then
  // reused across all wpb windows — v1/v2 re-read and re-wrote the blob
  // per window (one window per block)
  for (int t = threadIdx.x; t < (n_ops + 1) / 2; t += blockDim.x)
    reinterpret_cast<uint32_t*>(s_ops)[t] = g_ops[t];

  const uint8_t* sbase = buf + (long)blockIdx.y * cps * chunk_bytes;
  uint8_t* obase = obuf + (long)blockIdx.y * cps * chunk_bytes;
  const int total_items = n_src * w * vq;
  const long w_begin = (long)blockIdx.x * wpb;

  for (long it = 0; it < wpb; it++) {
    int win;
    long sw;
    if (xcdmap) {
      // XCD-cooperative mapping (knob ECX_BITXCD; host enables only when
      // windows_per_sw == 8 and the grid divides cleanly): consecutive
      // blocks land on XCDs b % 8, so blocks b..b+63 — dispatched
      // together — cover 8 superwords x 8 window slots with each XCD's 8
      // blocks reading the SAME superword at different 256 B offsets.
      // Their requests arrive temporally clustered, so DRAM sees whole
      // 2 KiB rows instead of 1-of-8 row churn (membench: strided-granule
      // reads are the gap between this kernel and the copy ceiling).
      const int x = (int)(blockIdx.x & 7);
      const int slot = (int)((blockIdx.x >> 3) & 7);
      const long tg = (long)(blockIdx.x >> 6);
      sw = (tg * wpb + it) * 8 + x;
      win = slot;
      if (sw >= (n_windows >> 3)) break;
    } else {
      const long wt = w_begin + it;
      if (wt >= n_windows) break;
      win = (int)(wt % windows_per_sw);
      sw = wt / windows_per_sw;
    }
    const long sw_off = sw * (long)w * pkt + (long)win * q;
    // all waves done computing the previous window before its LDS image
    // is overwritten (first window: orders the ops staging)
    __syncthreads();

    // Window staging: ecx_bit_glds per wave-chunk; __syncthreads() drains
    // the DMA (its fence emits vmcnt(0) while a glds is pending).
    if ((total_items & 63) == 0) {
      const int lane = threadIdx.x & 63;
      const int nwaves = blockDim.x >> 6;
      for (int t0 = (int)(threadIdx.x >> 6) * 64; t0 < total_items;
           t0 += nwaves * 64)
        ecx_bit_glds<NT>(bp, sbase, chunk_bytes, sw_off, pkt, w, vq_shift,
                         s_data, t0, lane);
    } else {
      // odd shapes (q < 128 with small k): register staging as in v1
      for (int t = threadIdx.x; t < total_items; t += blockDim.x) {
        const int jc = t >> vq_shift;
        const int v = t - (jc << vq_shift);
        const int j = jc / w, c = jc - j * w;
        const v4u* src = reinterpret_cast<const v4u*>(
            sbase + (long)bp->src_ids[j] * chunk_bytes + sw_off +
            (long)c * pkt + (long)v * 16);
        const v4u d = NT ? __builtin_nontemporal_load(src) : *src;
        *reinterpret_cast<v4u*>(s_data + (size_t)jc * q + (size_t)v * 16) =
            d;
      }
    }
    __syncthreads();

    ecx_bit_rows<NT, ACCUM>(bp, obase, chunk_bytes, sw, win, pkt, w, q, vq,
                            vq_shift, n_rows, s_data, s_ops);
  }
}

// Register-accumulator bitmatrix variant (v3): no LDS data staging, no
// barrier — the matmul kernel's continuous-stream structure applied to
// the bitmatrix map. Each thread owns one 16 B position v of a superword
// sw and streams ALL k*w source packets once, XOR-ing each into the
// NR = n_out*w output-row accumulators its column selects; column masks
// are wave-uniform (readfirstlane -> scalar branch per statically
// unrolled row, no divergence). Rationale: the LDS-window kernel's
// barrier-phased bursts cap at ~4.9-5.1 TB/s while the matmul kernel
// sustains 5.97 at the same 2.67:1 R/W mix — the mix is not the
// ceiling, the burst structure is (membench ladder + bench r2).
// NR <= 32 (n_out <= 4); larger n_out falls back to the LDS kernel.
// Job header: EcBitRegParams (bit_plan.h).
template <bool NT, bool ACCUM, int NR>
__global__ __launch_bounds__(256, 2) void ec_bitmatrix_reg_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const uint8_t* __restrict__ blob, long chunk_bytes, int cps,
    long n_pos) {
  const EcBitRegParams* bp = (const EcBitRegParams*)blob;
  __shared__ uint32_t s_cm[ECX_MAX_K * 8];
  __shared__ int s_src[ECX_MAX_K];
  __shared__ int s_out[4];
  const int n_src = bp->n_src;
  const int pkt = bp->pkt;
  for (int t = threadIdx.x; t < n_src * 8; t += blockDim.x)
    s_cm[t] = bp->colmask[t];
  for (int t = threadIdx.x; t < n_src; t += blockDim.x)
    s_src[t] = bp->src_ids[t];
  for (int t = threadIdx.x; t < NR / 8; t += blockDim.x)
    s_out[t] = bp->out_ids[t];
  __syncthreads();

  const long vp_sw = (long)pkt >> 4;  // 16B vecs per packet
  const uint8_t* sbase = buf + (long)blockIdx.y * cps * chunk_bytes;
  uint8_t* obase = obuf + (long)blockIdx.y * cps * chunk_bytes;

  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n_pos;
       p += (long)gridDim.x * blockDim.x) {
    const long sw = p / vp_sw;
    const long v = p - sw * vp_sw;
    const long sw_off = sw * 8 * (long)pkt + (v << 4);
    v4u acc[NR];
    if (ACCUM) {
#pragma unroll
      for (int r = 0; r < NR; r++)
        acc[r] = *reinterpret_cast<const v4u*>(
            obase + (long)s_out[r >> 3] * chunk_bytes + sw_off +
            (long)(r & 7) * pkt);
    } else {
#pragma unroll
      for (int r = 0; r < NR; r++) acc[r] = v4u{0, 0, 0, 0};
    }
    for (int j = 0; j < n_src; j++) {
      const uint8_t* sj = sbase + (long)s_src[j] * chunk_bytes + sw_off;
      const uint32_t* cmj = s_cm + j * 8;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const v4u d =
            NT ? __builtin_nontemporal_load(
                     reinterpret_cast<const v4u*>(sj + (long)c * pkt))
               : *reinterpret_cast<const v4u*>(sj + (long)c * pkt);
        const uint32_t m8 = __builtin_amdgcn_readfirstlane(cmj[c]);
#pragma unroll
        for (int r = 0; r < NR; r++) {
          if (m8 & (1u << r)) {
            acc[r].x ^= d.x; acc[r].y ^= d.y;
            acc[r].z ^= d.z; acc[r].w ^= d.w;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NR; r++) {
      v4u* dst = reinterpret_cast<v4u*>(obase +
                                        (long)s_out[r >> 3] * chunk_bytes +
                                        sw_off + (long)(r & 7) * pkt);
      if (NT)
        __builtin_nontemporal_store(acc[r], dst);
      else
        *dst = acc[r];
    }
  }
}

// Software-pipelined bitmatrix variant: two LDS window buffers; each wave
// issues its glds batch for window t+1, then waits ONLY for window t's
// batch (counted s_waitcnt vmcnt(G) — vmcnt retires in order) and
// computes t while t+1 streams in. Costs 2x data LDS (half the block
// residency) but overlaps the load latency the barrier otherwise
// serialises; raw s_barrier + lgkmcnt-only waits so the in-flight glds
// survives the barrier (hipcc's __syncthreads would drain vmcnt(0)).
#define ECX_WAITV(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
__device__ __forceinline__ void ecx_wait_vmcnt(int g) {
  switch (g) {
    case 0: ECX_WAITV(0); break;
    case 1: ECX_WAITV(1); break;
    case 2: ECX_WAITV(2); break;
    case 3: ECX_WAITV(3); break;
    case 4: ECX_WAITV(4); break;
    case 5: ECX_WAITV(5); break;
    case 6: ECX_WAITV(6); break;
    case 7: ECX_WAITV(7); break;
    case 8: ECX_WAITV(8); break;
    case 9: ECX_WAITV(9); break;
    case 10: ECX_WAITV(10); break;
    case 11: ECX_WAITV(11); break;
    case 12: ECX_WAITV(12); break;
    case 13: ECX_WAITV(13); break;
    case 14: ECX_WAITV(14); break;
    case 15: ECX_WAITV(15); break;
    default: ECX_WAITV(16); break;
  }
}
__device__ __forceinline__ void ecx_raw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

template <bool NT, bool ACCUM = false>
__global__ __launch_bounds__(256, 2) void ec_bitmatrix_pipe_kernel(
    const uint8_t* __restrict__ buf, uint8_t* __restrict__ obuf,
    const uint8_t* __restrict__ blob, long chunk_bytes, int cps,
    int windows_per_sw, int wpb, long n_windows) {
  const EcBitParams* bp = (const EcBitParams*)blob;
  const uint32_t* g_ops = (const uint32_t*)(blob + sizeof(EcBitParams));
  extern __shared__ uint8_t smem[];
  const int n_src = bp->n_src, w = bp->w, pkt = bp->pkt, q = bp->q;
  const int vq = q >> 4, vq_shift = bp->vq_shift;
  const int n_rows = bp->n_out * w;
  const size_t buf_bytes = (size_t)n_src * w * q;
  uint8_t* s_buf0 = smem;
  uint8_t* s_buf1 = smem + buf_bytes;
  uint16_t* s_ops = (uint16_t*)(smem + 2 * buf_bytes);
  const int n_ops = bp->row_off[n_rows];
  for (int t = threadIdx.x; t < (n_ops + 1) / 2; t += blockDim.x)
    reinterpret_cast<uint32_t*>(s_ops)[t] = g_ops[t];

  const uint8_t* sbase = buf + (long)blockIdx.y * cps * chunk_bytes;
  uint8_t* obase = obuf + (long)blockIdx.y * cps * chunk_bytes;
  const int total_items = n_src * w * vq;  // host guarantees %64 == 0
  const int chunks = total_items >> 6;
  const int lane = threadIdx.x & 63;
  const int wave = (int)(threadIdx.x >> 6);
  const int nwaves = (int)(blockDim.x >> 6);
  // uniform per-wave glds count: tail waves re-issue a wrapped chunk
  // (same source -> same LDS bytes; racing identical writes are benign)
  const int G = (chunks + nwaves - 1) / nwaves;
  const long w_begin = (long)blockIdx.x * wpb;
  const long w_end = w_begin + wpb < n_windows ? w_begin + wpb : n_windows;
  if (w_begin >= w_end) return;

  auto issue = [&](long wt, uint8_t* dstbuf) {
    const int win = (int)(wt % windows_per_sw);
    const long sw = wt / windows_per_sw;
    const long sw_off = sw * (long)w * pkt + (long)win * q;
    for (int g = 0; g < G; g++) {
      int chunk = wave + g * nwaves;
      // wrap (duplicate, benign); modulo, since with fewer chunks than
      // waves (64 items: one chunk) one subtraction leaves waves 2-3 past
      // the window image
      if (chunk >= chunks) chunk %= chunks;
      ecx_bit_glds<NT>(bp, sbase, chunk_bytes, sw_off, pkt, w, vq_shift,
                       dstbuf, chunk << 6, lane);
    }
  };

  issue(w_begin, s_buf0);
  for (long wt = w_begin; wt < w_end; wt++) {
    uint8_t* cur = (wt - w_begin) & 1 ? s_buf1 : s_buf0;
    if (wt + 1 < w_end) {
      issue(wt + 1, (wt + 1 - w_begin) & 1 ? s_buf1 : s_buf0);
      ecx_wait_vmcnt(G);  // window wt landed; wt+1 still streaming
    } else {
      ecx_wait_vmcnt(0);
    }
    ecx_raw_barrier();  // every wave's window-wt DMA landed; s_ops staged

    const int win = (int)(wt % windows_per_sw);
    const long sw = wt / windows_per_sw;
    ecx_bit_rows<NT, ACCUM>(bp, obase, chunk_bytes, sw, win, pkt, w, q, vq,
                            vq_shift, n_rows, cur, s_ops);
    ecx_raw_barrier();  // all reads of `cur` done before wt+2 overwrites it
  }
}

// delta = a ^ b (encode_delta; replaces galois_region_xor / xor_gen).
__global__ __launch_bounds__(256) void ec_xor_kernel(
    const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    uint8_t* __restrict__ out, long n_vecs) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n_vecs;
       p += (long)gridDim.x * blockDim.x) {
    const uint4 va = reinterpret_cast<const uint4*>(a)[p];
    const uint4 vb = reinterpret_cast<const uint4*>(b)[p];
    uint4 o;
    o.x = va.x ^ vb.x; o.y = va.y ^ vb.y; o.z = va.z ^ vb.z; o.w = va.w ^ vb.w;
    reinterpret_cast<uint4*>(out)[p] = o;
  }
}

// Deterministic device-side fill (splitmix64 of the word index) so bench
// inputs need no 32 GiB PCIe upload. Random bytes, fixed seed — BASELINE.md
// requires non-constant fill (constant data would mask a broken kernel).
__device__ __forceinline__ uint64_t ecx_splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void ec_fill_random_kernel(
    uint64_t* __restrict__ out, long n_words, uint64_t seed) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n_words;
       p += (long)gridDim.x * blockDim.x)
    out[p] = ecx_splitmix64(seed ^ (uint64_t)p);
}

// ---------------------------------------------------------------------------
// Per-shard CRC-32C (ecx_crc32c_batch; constants and the
// end-aligned tiling: crc_plan.h)
// ---------------------------------------------------------------------------
__constant__ ecx::CrcTables ecx_crc_tab{};
__constant__ ecx::CrcCombine ecx_crc_comb{};

constexpr int ECX_CRC_CHAIN_T = 1024;  // lanes of the chain scan
static_assert(ECX_CRC_CHAIN_T == 1 << ecx::CRC_CHAIN_LOG2, "chain plan split");

// What the three CRC kernels share about a call.
struct EcCrcArgs {
  uint32_t ids[64];      // chunk id of the j-th masked chunk
  uint32_t n_ids;        // masked chunks per stripe
  uint32_t n_chunks;     // k + m
  uint32_t bpc;          // blocks per chunk
  uint32_t x_chunk;      // x^(8 * chunk_bytes)
  uint64_t chunk_bytes;
};

// a * b mod P, branch-free (ecx::crc_mulmod is the readable form)
__device__ __forceinline__ uint32_t ecx_crc_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    r ^= a & (uint32_t)((int32_t)(b << i) >> 31);
    a = (a >> 1) ^ (ecx::CRC32C_POLY & (0u - (a & 1)));
  }
  return r;
}

// First launch: every masked word becomes the term its seed contributes,
// shift(seed, chunk_bytes) — or 0 in chain mode, where the scan brings the
// seed in. d_seed may be d_crc itself (each word is read, then written, by
// one lane).
template <int = 0>
__global__ __launch_bounds__(256) void ec_crc32c_seed_kernel(
    const uint32_t* d_seed, uint32_t* d_crc, EcCrcArgs a, uint32_t n_words,
    int chain) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_words) return;
  const size_t w = (size_t)(i / a.n_ids) * a.n_chunks + a.ids[i % a.n_ids];
  uint32_t v = 0;
  if (!chain) v = ecx_crc_mul(d_seed ? d_seed[w] : 0xFFFFFFFFu, a.x_chunk);
  d_crc[w] = v;
}

// One block = CRC_BLOCK_BYTES of one chunk, counted from the chunk's END
// (the first block of a chunk may start before byte 0; what lies there is
// skipped, leading zeros do not move a zero state). Coalesced 16-byte loads
// into an LDS image with one padded row per lane; each lane then hashes its
// own CRC_SEG_BYTES from state 0 by slice-by-4 lookups in LDS tables,
// multiplies by x^(8 * bytes that follow it in the block), the block XORs
// its lanes together, multiplies by x^(8 * bytes that follow the block) and
// XORs the result into the chunk's word. XOR commutes, so the word does not
// depend on the order in which a chunk's blocks arrive.
template <bool NT>
__global__ __launch_bounds__(ecx::CRC_THREADS) void ec_crc32c_kernel(
    const uint8_t* __restrict__ buf, uint32_t* d_crc, EcCrcArgs a) {
  constexpr int L = ecx::CRC_SEG_BYTES, T = ecx::CRC_THREADS;
  constexpr int STRIDE = ecx::CRC_SEG_STRIDE, NV = L / 16;
  __shared__ __attribute__((aligned(16))) uint8_t lds[ecx::CRC_LDS_BYTES];
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(lds + STRIDE * T);
  // the waves' totals go into the pad of row 0, which staging never writes:
  // one more LDS object would cost the fourth block per CU
  uint32_t* s_red = reinterpret_cast<uint32_t*>(lds + L);
  static_assert(T / 64 * 4 <= STRIDE - L, "wave totals fit the row pad");
  const uint32_t t = threadIdx.x;
  const uint32_t b = blockIdx.x % a.bpc, cj = blockIdx.x / a.bpc;
  const uint32_t stripe = cj / a.n_ids, chunk = a.ids[cj % a.n_ids];
  const size_t word = (size_t)stripe * a.n_chunks + chunk;
  const uint8_t* src = buf + word * a.chunk_bytes;
  // offset in the chunk of this block's first byte; < 0 only for b == 0
  const int64_t base = (int64_t)(b + 1) * ecx::CRC_BLOCK_BYTES -
                       (int64_t)a.bpc * ecx::CRC_BLOCK_BYTES +
                       (int64_t)a.chunk_bytes - ecx::CRC_BLOCK_BYTES;

#pragma unroll
  for (int q = 0; q < 4; q++)
    s_tab[t + T * q] = (&ecx_crc_tab.t[0][0])[t + T * q];
  // items before byte 0 load byte 0's vector instead and are never read
#pragma unroll
  for (int j = 0; j < NV; j++) {
    const uint32_t i = t + T * j;
    const int64_t off = base + (int64_t)i * 16;
    const v4u d = ecx_ld16<NT>(src + (off < 0 ? 0 : off));
    *reinterpret_cast<v4u*>(lds + (i / NV) * STRIDE + (i % NV) * 16) = d;
  }
  __syncthreads();

  const int64_t seg0 = base + (int64_t)t * L;
  const int first = seg0 >= 0 ? 0 : (int)((-seg0 > L ? L : -seg0) / 16);
  uint32_t crc = 0;
#pragma unroll
  for (int q = 0; q < NV; q++) {
    if (q < first) continue;
    const v4u d = *reinterpret_cast<const v4u*>(lds + t * STRIDE + q * 16);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const uint32_t x = crc ^ d[e];
      crc = s_tab[768 + (x & 255)] ^ s_tab[512 + ((x >> 8) & 255)] ^
            s_tab[256 + ((x >> 16) & 255)] ^ s_tab[x >> 24];
    }
  }

  uint32_t v = ecx_crc_mul(crc, ecx_crc_comb.seg[t]);
#pragma unroll
  for (int o = 32; o; o >>= 1) v ^= __shfl_xor(v, o);
  if ((t & 63) == 0) s_red[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    v = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
    uint32_t after = a.bpc - 1 - b;  // blocks that follow in the chunk
    for (int i = 0; after; after >>= 1, i++)
      if (after & 1) v = ecx_crc_mul(v, ecx_crc_comb.blk[i]);
    atomicXor(&d_crc[word], v);
  }
}
static_assert(ecx::CRC_THREADS == 256, "s_red sum and table fill assume 256");

// Chain mode, after the hash pass: d_crc[s][c] holds f(0, chunk c of stripe
// s); make it the hash of stripes 0..s of shard c concatenated, from the
// shard's seed. One block per masked shard. Lane t owns `run` consecutive
// stripes and folds them in order; the lanes' totals go through a log-step
// scan in LDS with the constants x^(8C * run * 2^i); each lane then adds what
// precedes its run, advanced by one chunk per stripe.
template <int = 0>
__global__ __launch_bounds__(ECX_CRC_CHAIN_T) void ec_crc32c_chain_kernel(
    const uint32_t* __restrict__ d_seed, uint32_t* __restrict__ d_crc,
    EcCrcArgs a, ecx::CrcChainPlan cp, uint32_t n_stripes) {
  __shared__ uint32_t s_tot[ECX_CRC_CHAIN_T];
  const uint32_t t = threadIdx.x, c = a.ids[blockIdx.x];
  const uint32_t s0 = min(t * cp.run, n_stripes);
  const uint32_t s1 = min(s0 + cp.run, n_stripes);
  uint32_t* col = d_crc + c;
  uint32_t acc = t == 0 ? (d_seed ? d_seed[c] : 0xFFFFFFFFu) : 0;
  for (uint32_t s = s0; s < s1; s += 8) {
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; e++)
      h[e] = s + e < s1 ? col[(size_t)(s + e) * a.n_chunks] : 0;
#pragma unroll
    for (int e = 0; e < 8; e++)
      if (s + e < s1) {
        acc = ecx_crc_mul(acc, a.x_chunk) ^ h[e];
        col[(size_t)(s + e) * a.n_chunks] = acc;
      }
  }
  s_tot[t] = acc;
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < ecx::CRC_CHAIN_LOG2; i++) {
    const uint32_t d = 1u << i;
    const uint32_t up = t >= d ? ecx_crc_mul(s_tot[t - d], cp.x_step[i]) : 0;
    __syncthreads();
    s_tot[t] ^= up;
    __syncthreads();
  }
  uint32_t carry = t ? s_tot[t - 1] : 0;
  for (uint32_t s = s0; s < s1; s++) {
    carry = ecx_crc_mul(carry, a.x_chunk);
    col[(size_t)s * a.n_chunks] ^= carry;
  }
}

// ---------------------------------------------------------------------------
// Locating the corrupt chunk (ecx_locate_batch). Templates,
// launched from the end of the file like the CRC kernels.
// ---------------------------------------------------------------------------

#define ECX_LOCATE_LIST_T 1024

// The stripes ec_gf_verify_kernel flagged, as a list: list[0] = how many,
// list[1..] = their indices in no particular order. One block: the count is
// formed in LDS and written once, so the list needs no clearing and a clean
// batch costs one pass over n_stripes words. A wave reserves its entries
// with one LDS atomic.
template <int = 0>
__global__ __launch_bounds__(ECX_LOCATE_LIST_T) void ec_locate_list_kernel(
    const unsigned long long* __restrict__ bad, uint32_t* __restrict__ list,
    uint32_t n_stripes) {
  __shared__ uint32_t s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  // whole waves stay in the loop together: the ballot needs every lane
  for (uint32_t s0 = threadIdx.x - lane; s0 < n_stripes;
       s0 += ECX_LOCATE_LIST_T) {
    const uint32_t s = s0 + lane;
    const bool flagged = s < n_stripes && bad[s] != 0ull;
    const unsigned long long vote = __ballot(flagged);
    if (vote == 0ull) continue;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&s_count, (uint32_t)__popcll(vote));
    base = __shfl(base, 0);
    if (flagged)
      list[1 + base + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull))] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) list[0] = s_count;
}

// One candidate "survivor cand is the damaged one", checked on the flagged
// stripes only: the verify computation (sources = the candidate's survivors,
// outputs = its checked chunks) over tiles numbered
//     (index into the flagged list, tile in chunk)
// with the tile fastest. The count of flagged stripes is known only on the
// device, so the grid is sized by the host for residency and strides over
// count x tpc; the step is split on the host into (list entries, tiles) so
// the device adds and carries. With nothing flagged a block leaves after one
// scalar load. A wave in which any lane differs in any output sets bit cand
// of the stripe's refuted word with one atomicOr from one lane.
template <int NOUT>
__global__ __launch_bounds__(256, NOUT < 4 ? 8 : 6) void ec_gf_locate_kernel(
    const uint8_t* buf, unsigned long long* refuted,
    const uint32_t* __restrict__ list, const EcStreamParams p,
    uint64_t stripe_bytes, uint64_t vecs_per_chunk, uint32_t tpc,
    uint32_t step_e, uint32_t step_t, uint32_t cand) {
  const uint32_t count = list[0];
  if (count == 0u) return;
  const uint32_t voff = threadIdx.x << 4;
  const int n_src = p.n_src;
  uint32_t one_mask[NOUT], mul_mask[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; j++) {
    one_mask[j] = p.one_mask[j];
    mul_mask[j] = p.mul_mask[j];
  }
  uint32_t e = blockIdx.x / tpc, tile = blockIdx.x % tpc;
  while (e < count) {
    const uint32_t stripe = list[1 + e];
    const uint64_t tbase =
        (uint64_t)stripe * stripe_bytes + ((uint64_t)tile << 12);
    if (((uint64_t)tile << 8) + threadIdx.x < vecs_per_chunk) {
      const uint8_t* sb = buf + tbase;
      uint32_t acc[NOUT][4];
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0u;
      ecx_stream_sources<NOUT>(p, one_mask, mul_mask, n_src, sb, voff, acc);
      v4u st[NOUT];
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        st[j] = __builtin_nontemporal_load(
            reinterpret_cast<const v4u*>(sb + p.out_off[j] + voff));
      uint32_t diff = 0u;
#pragma unroll
      for (int j = 0; j < NOUT; j++)
        diff |= (acc[j][0] ^ st[j].x) | (acc[j][1] ^ st[j].y) |
                (acc[j][2] ^ st[j].z) | (acc[j][3] ^ st[j].w);
      // wave-uniform, so the branch is scalar
      const unsigned long long vote = __ballot(diff != 0u);
      if (vote != 0ull &&
          (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)vote) - 1u)
        atomicOr(&refuted[stripe], 1ull << cand);
    }
    // e + step_e stays far below 2^32: both are at most 65535 + 2^23
    e += step_e;
    tile += step_t;
    if (tile >= tpc) {
      tile -= tpc;
      e++;
    }
  }
}

// d_culprit has collected the refuted bits; one lane per stripe turns it
// into the culprit word (locate_word of locate_plan.h).
template <int = 0>
__global__ __launch_bounds__(256) void ec_locate_finish_kernel(
    const unsigned long long* __restrict__ bad, unsigned long long* culprit,
    uint64_t present_mask, uint64_t survivor_mask, uint32_t n_stripes) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_stripes) return;
  culprit[s] =
      ecx::locate_word(present_mask, survivor_mask, bad[s], culprit[s]);
}

// ---------------------------------------------------------------------------
// Host-side: context, streams, decode-row LRU, launches
// ---------------------------------------------------------------------------

namespace {

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // around last kernel
  hipEvent_t ev_param = nullptr;  // param upload completion (ring of 1)
  EcLaunchParams* h_params = nullptr;  // pinned
  EcLaunchParams* d_params = nullptr;
  // variable-size slice batch scratch (job table), grown on demand
  hipEvent_t ev_jobs = nullptr;
  uint8_t* h_jobs = nullptr;  // pinned
  uint8_t* d_jobs = nullptr;
  size_t jobs_bytes = 0;
  // host-path staging stripe buffer, grown on demand
  uint8_t* d_stage = nullptr;
  size_t stage_bytes = 0;
  // ecx_locate_batch: the count of flagged stripes and their indices, grown
  // on demand (at most 1 + 65535 words)
  uint32_t* d_loc = nullptr;
  size_t loc_words = 0;
  // pipelined host-path: pinned+device double buffer and resident
  // per-group launch params (see pipelined_matmul_host below)
  uint8_t* h_pipe = nullptr;  // pinned, 2 x cps x tile
  uint8_t* d_pipe = nullptr;
  size_t pipe_bytes = 0;
  EcLaunchParams* h_pparams = nullptr;  // pinned, 8 groups
  EcLaunchParams* d_pparams = nullptr;
  // what d_pparams currently holds: 1 = full-encode tables (gen rows,
  // no zeros-chunks) — the hot repeated case; 0 = anything else.
  // Invalidated by ecx_set_matrix.
  int pparams_kind = 0;
  hipEvent_t ev_pipe[2] = {nullptr, nullptr};
  double last_ms = -1.0;
  bool timed = false;
  // captured single-tile host-call graphs, keyed by (tl, n_src, n_out)
  std::map<uint64_t, hipGraphExec_t> graphs;
  std::recursive_mutex mu;
};

// Decode plan for one present mask, in the context's technique.
struct DecodePlan {
  std::vector<int> survivors;
  std::vector<int> erased;
  // w=8: n_erased x k coefficients; bitmatrix: (n_erased*w) x (k*w) bits
  std::vector<uint8_t> rows;
  std::vector<uint16_t> rows16;  // w=16: n_erased x k u16
};

// The rows of a coded job, in the context's technique.
struct CodeRows {
  const uint8_t* r8;    // w=8 coefficients, or bitmatrix bit rows
  const uint16_t* r16;  // w=16 coefficients
};

}  // namespace

struct ecx_ctx {
  int k = 0, m = 0, technique = 0, device = 0;
  int w = 8, pkt = 2048;  // bitmatrix techniques only (jerasure packetsize)
  std::vector<uint8_t> gen;      // (k+m) x k (w=8 techniques)
  std::vector<uint16_t> gen16;   // (k+m) x k (w=16 technique)
  std::vector<uint8_t> bitmat;   // (m*w) x (k*w) bits (bitmatrix techniques)
  std::vector<Slot> slots;
  // decode-plan LRU keyed by present_mask (exact signature for fixed
  // (k,m,technique) — the analogue of ErasureCodeIsaTableCache's
  // "k%dm%da+..e-.." string key). Depth mirrors the reference's 2516-entry
  // comfort zone scaled down: plans here are tiny, keep 4096.
  std::mutex lru_mu;
  std::map<uint64_t, std::pair<DecodePlan, std::list<uint64_t>::iterator>> lru;
  std::list<uint64_t> lru_order;
  static constexpr size_t LRU_DEPTH = 4096;
  // host-pointer calls round-robin the stream slots so concurrent plugin
  // threads (the OSD's PG workers) overlap instead of serialising on one
  // stream's mutex
  std::atomic<unsigned> rr{0};
  // grid sizing for ec_gf_stream_kernel, queried from the runtime on first
  // use (racing callers store the same values): CU count, and resident
  // blocks per CU for NOUT 1..4 (the persistent grid, ECX_STREAM_BPC=0)
  std::atomic<int> stream_cus{0};
  std::atomic<int> stream_occ[5] = {};
  // the same for ec_gf_verify_kernel, whose instances need not stay resident
  // in the same numbers
  std::atomic<int> verify_occ[5] = {};
  // and for ec_gf_locate_kernel, whose grid is always the resident one
  std::atomic<int> locate_occ[5] = {};

  bool is_bitmatrix() const {
    return technique == ECX_T_CAUCHY_ORIG_JERASURE ||
           technique == ECX_T_CAUCHY_GOOD_JERASURE;
  }
  bool is_w16() const { return technique == ECX_T_RS_VAN_JERASURE_W16; }
  bool is_table8() const { return !is_w16() && !is_bitmatrix(); }
  // the coding rows of the generator
  CodeRows gen_rows() const {
    if (is_bitmatrix()) return {bitmat.data(), nullptr};
    if (is_w16()) return {nullptr, gen16.data() + (size_t)k * k};
    return {gen.data() + (size_t)k * k, nullptr};
  }
};

static int map_hip(hipError_t e) {
  if (e == hipSuccess) return ECX_OK;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return ECX_ERR_NO_GPU;
  if (e == hipErrorOutOfMemory) return ECX_ERR_NOMEM;
  return ECX_ERR_HIP;
}

#define HIP_TRY(x)                        \
  do {                                    \
    hipError_t _e = (x);                  \
    if (_e != hipSuccess) return map_hip(_e); \
  } while (0)

extern "C" {

const char* ecx_version(void) { return "ec-mi355x 0.1.0"; }

int ecx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ecx_create2(int k, int m, int technique, int w, int packetsize,
                int device, int n_streams, ecx_ctx** out) {
  const bool want16 = (technique == ECX_T_RS_VAN_JERASURE_W16);
  if (!out || k < 2 || m < 1 || k > ECX_MAX_K || m > ECX_MAX_K ||
      n_streams < 1 || n_streams > 64 || w != (want16 ? 16 : 8))
    return ECX_ERR_INVAL;
  if ((technique == ECX_T_CAUCHY_ORIG_JERASURE ||
       technique == ECX_T_CAUCHY_GOOD_JERASURE) &&
      (packetsize < 16 || packetsize % 16 || k > 16))
    return ECX_ERR_INVAL;
  // cauchy_good m==2: jerasure would use its precomputed cbest tables
  // (cauchy.c), which cannot be faithfully restated here — refuse rather
  // than silently diverge from the reference's parity bytes.
  if (technique == ECX_T_CAUCHY_GOOD_JERASURE && m == 2) return ECX_ERR_INVAL;
  if (ecx_device_count() <= device) return ECX_ERR_NO_GPU;

  auto ctx = new ecx_ctx();
  ctx->k = k;
  ctx->m = m;
  ctx->technique = technique;
  ctx->device = device;
  ctx->w = w;
  ctx->pkt = packetsize;
  if (want16) {
    if (!ecx::gen_matrix_rs_van_jerasure_w16(ctx->gen16, k, m)) {
      delete ctx;
      return ECX_ERR_INVAL;
    }
  } else if (!ecx::gen_matrix(technique, ctx->gen, k, m)) {
    delete ctx;
    return ECX_ERR_INVAL;
  }
  if (ctx->is_bitmatrix())
    ecx::matrix_to_bitmatrix(ctx->gen.data() + (size_t)k * k, k, m, w,
                             ctx->bitmat);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete ctx;
    return map_hip(e);
  }
  ctx->slots = std::vector<Slot>(n_streams);
  for (auto& s : ctx->slots) {
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&s.ev_start) != hipSuccess ||
        hipEventCreate(&s.ev_stop) != hipSuccess ||
        hipEventCreate(&s.ev_param) != hipSuccess ||
        hipEventCreate(&s.ev_jobs) != hipSuccess ||
        hipEventCreate(&s.ev_pipe[0]) != hipSuccess ||
        hipEventCreate(&s.ev_pipe[1]) != hipSuccess ||
        hipHostMalloc(&s.h_params, sizeof(EcLaunchParams)) != hipSuccess ||
        hipMalloc(&s.d_params, sizeof(EcLaunchParams)) != hipSuccess) {
      ecx_destroy(ctx);
      return ECX_ERR_HIP;
    }
  }
  *out = ctx;
  return ECX_OK;
}

int ecx_create(int k, int m, int technique, int device, int n_streams,
               ecx_ctx** out) {
  return ecx_create2(k, m, technique, 8, 2048, device, n_streams, out);
}

void ecx_destroy(ecx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (auto& s : ctx->slots) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.ev_start) (void)hipEventDestroy(s.ev_start);
    if (s.ev_stop) (void)hipEventDestroy(s.ev_stop);
    if (s.ev_param) (void)hipEventDestroy(s.ev_param);
    if (s.ev_jobs) (void)hipEventDestroy(s.ev_jobs);
    if (s.ev_pipe[0]) (void)hipEventDestroy(s.ev_pipe[0]);
    if (s.ev_pipe[1]) (void)hipEventDestroy(s.ev_pipe[1]);
    if (s.h_jobs) (void)hipHostFree(s.h_jobs);
    if (s.d_jobs) (void)hipFree(s.d_jobs);
    if (s.h_params) (void)hipHostFree(s.h_params);
    if (s.d_params) (void)hipFree(s.d_params);
    if (s.d_stage) (void)hipFree(s.d_stage);
    if (s.d_loc) (void)hipFree(s.d_loc);
    if (s.h_pipe) (void)hipHostFree(s.h_pipe);
    if (s.d_pipe) (void)hipFree(s.d_pipe);
    if (s.h_pparams) (void)hipHostFree(s.h_pparams);
    if (s.d_pparams) (void)hipFree(s.d_pparams);
    for (auto& [k, ge] : s.graphs) {
      (void)k;
      (void)hipGraphExecDestroy(ge);
    }
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  delete ctx;
}

int ecx_k(const ecx_ctx* ctx) { return ctx ? ctx->k : ECX_ERR_INVAL; }
int ecx_m(const ecx_ctx* ctx) { return ctx ? ctx->m : ECX_ERR_INVAL; }

int ecx_get_matrix(const ecx_ctx* ctx, uint8_t* out) {
  if (!ctx || !out || ctx->is_w16()) return ECX_ERR_INVAL;
  std::memcpy(out, ctx->gen.data(), ctx->gen.size());
  return ECX_OK;
}

int ecx_get_matrix16(const ecx_ctx* ctx, uint16_t* out) {
  if (!ctx || !out || !ctx->is_w16()) return ECX_ERR_INVAL;
  std::memcpy(out, ctx->gen16.data(), ctx->gen16.size() * 2);
  return ECX_OK;
}

unsigned ecx_chunk_size(const ecx_ctx* ctx, unsigned stripe_width) {
  if (!ctx) return 0;
  if (ctx->is_bitmatrix()) {
    // ErasureCodeJerasureCauchy::get_alignment (per_chunk_alignment=false):
    // stripe aligned to k*w*packetsize*sizeof(int) => chunk is a multiple
    // of w*packetsize*4 (ErasureCodeJerasure.cc:522-536)
    unsigned align = (unsigned)ctx->k * ctx->w * ctx->pkt * 4u;
    unsigned tail = stripe_width % align;
    unsigned padded = stripe_width + (tail ? align - tail : 0);
    return padded / ctx->k;
  }
  if (ctx->technique == ECX_T_RS_VAN_JERASURE || ctx->is_w16()) {
    // ErasureCodeJerasure.cc:85-108, per_chunk_alignment=false
    unsigned align = (unsigned)ctx->k * ctx->w * 4u;
    unsigned tail = stripe_width % align;
    unsigned padded = stripe_width + (tail ? align - tail : 0);
    return padded / ctx->k;
  }
  // ErasureCodeIsa.cc:65-79: ceil(width/k) rounded up to 32
  unsigned chunk = (stripe_width + ctx->k - 1) / ctx->k;
  unsigned mod = chunk % 32u;
  if (mod) chunk += 32u - mod;
  return chunk;
}

int ecx_minimum_to_decode(const ecx_ctx* ctx, uint64_t want_mask,
                          uint64_t avail_mask, uint64_t* minimum_mask) {
  // ErasureCode.cc:154-170: want if all available, else first k available.
  if (!ctx || !minimum_mask) return ECX_ERR_INVAL;
  if ((want_mask & avail_mask) == want_mask) {
    *minimum_mask = want_mask;
    return __builtin_popcountll(want_mask);
  }
  uint64_t min_mask = 0;
  int cnt = 0;
  for (int i = 0; i < ctx->k + ctx->m && cnt < ctx->k; i++) {
    if (avail_mask & (1ull << i)) {
      min_mask |= 1ull << i;
      cnt++;
    }
  }
  if (cnt < ctx->k) return ECX_ERR_IO;
  *minimum_mask = min_mask;
  return cnt;
}

int ecx_dbuf_alloc(ecx_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc(dptr, bytes));
  return ECX_OK;
}

int ecx_dbuf_free(ecx_ctx* ctx, void* dptr) {
  if (!ctx) return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipFree(dptr));
  return ECX_OK;
}

int ecx_upload(ecx_ctx* ctx, void* dptr, const void* host, size_t bytes,
               int slot, int blocking) {
  if (!ctx || slot < 0 || slot >= (int)ctx->slots.size()) return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice,
                         ctx->slots[slot].stream));
  if (blocking) HIP_TRY(hipStreamSynchronize(ctx->slots[slot].stream));
  return ECX_OK;
}

int ecx_download(ecx_ctx* ctx, void* host, const void* dptr, size_t bytes,
                 int slot, int blocking) {
  if (!ctx || slot < 0 || slot >= (int)ctx->slots.size()) return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost,
                         ctx->slots[slot].stream));
  if (blocking) HIP_TRY(hipStreamSynchronize(ctx->slots[slot].stream));
  return ECX_OK;
}

int ecx_dbuf_fill_random(ecx_ctx* ctx, void* dptr, size_t bytes, uint64_t seed,
                         int slot) {
  if (!ctx || slot < 0 || slot >= (int)ctx->slots.size() || (bytes & 7))
    return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  long n_words = (long)(bytes >> 3);
  int blocks = (int)std::min<long>((n_words + 255) / 256, 8192);
  hipLaunchKernelGGL(ec_fill_random_kernel, dim3(blocks), dim3(256), 0,
                     ctx->slots[slot].stream, (uint64_t*)dptr, n_words, seed);
  HIP_TRY(hipGetLastError());
  return ECX_OK;
}

}  // extern "C"

// Build the 6-dword v_perm tables for one coefficient: T[0..1] = c*x for
// x in 0..7 (low-3-bit table), T[2..3] = c*(x<<4) for x in 0..7
// (bits 4-6), T[4] = the fused W table (bit3/bit7 combinations), T[5]
// unused (kept so the stride stays a friendly 6 dwords).
static void build_tabs(const ecx::GF8& f, uint8_t c, uint32_t* T) {
  uint8_t lo[8], hi[8];
  for (int x = 0; x < 8; x++) {
    lo[x] = f.mul(c, (uint8_t)x);
    hi[x] = f.mul(c, (uint8_t)(x << 4));
  }
  T[0] = lo[0] | (lo[1] << 8) | (lo[2] << 16) | ((uint32_t)lo[3] << 24);
  T[1] = lo[4] | (lo[5] << 8) | (lo[6] << 16) | ((uint32_t)lo[7] << 24);
  T[2] = hi[0] | (hi[1] << 8) | (hi[2] << 16) | ((uint32_t)hi[3] << 24);
  T[3] = hi[4] | (hi[5] << 8) | (hi[6] << 16) | ((uint32_t)hi[7] << 24);
  uint8_t c8 = f.mul(c, 8), c128 = f.mul(c, 128);
  T[4] = 0u | ((uint32_t)c8 << 8) | ((uint32_t)c128 << 16) |
         ((uint32_t)(uint8_t)(c8 ^ c128) << 24);
  T[5] = 0;
}

// The 5-dword v_perm tables of ec_gf_stream_kernel for one coefficient,
// over the contiguous bit groups 0-2 / 3-5 / 6-7: T[0..1] = c*x for x in
// 0..7, T[2..3] = c*(x<<3) for x in 0..7, T[4] = c*(x<<6) for x in 0..3.
// GF(2^8) multiplication is linear over XOR, so the three lookups XORed
// give c*x exactly.
static void build_tabs332(const ecx::GF8& f, uint8_t c, uint32_t* T) {
  for (int t = 0; t < 5; t++) T[t] = 0;
  for (int x = 0; x < 8; x++) {
    T[x >> 2] |= (uint32_t)f.mul(c, (uint8_t)x) << (8 * (x & 3));
    T[2 + (x >> 2)] |= (uint32_t)f.mul(c, (uint8_t)(x << 3)) << (8 * (x & 3));
  }
  for (int x = 0; x < 4; x++)
    T[4] |= (uint32_t)f.mul(c, (uint8_t)(x << 6)) << (8 * x);
}

// Fill the fields EcLaunchParams and EcMultiRec share from a coefficient
// matrix (n_out x n_src over source ids src_ids); src_null[i] marks
// zeros-chunk sources to skip (the reference's zeros-buffer convention,
// ErasureCodeJerasure.cc:146-157).
template <class Rec>
static void fill_rec(Rec* p, const int* src_ids, int n_src,
                     const int* out_ids, int n_out,
                     const uint8_t* coeff /* n_out x n_src */,
                     const bool* src_null) {
  const ecx::GF8& f = ecx::gf8();
  for (int i = 0; i < n_src; i++) p->src_ids[i] = src_ids[i];
  for (int j = 0; j < n_out; j++) p->out_ids[j] = out_ids[j];
  for (int j = 0; j < n_out; j++)
    for (int i = 0; i < n_src; i++) {
      uint8_t c = coeff[(size_t)j * n_src + i];
      uint8_t cls = (c == 0 || (src_null && src_null[i])) ? 0 : (c == 1 ? 1 : 2);
      p->cls[j * n_src + i] = cls;
      if (cls == 2) build_tabs(f, c, &p->tabs[(j * n_src + i) * 6]);
    }
}

static void fill_params(EcLaunchParams* p, const int* src_ids, int n_src,
                        const int* out_ids, int n_out, const uint8_t* coeff,
                        const bool* src_null) {
  p->n_src = n_src;
  p->n_out = n_out;
  fill_rec(p, src_ids, n_src, out_ids, n_out, coeff, src_null);
}

// Chunk ids of a job whose sources lead the stripe: 0..n_src-1, the outputs
// behind them (an encode: data, then parity).
static void stripe_ids(int n_src, int n_out, int* src_ids, int* out_ids) {
  for (int i = 0; i < n_src; i++) src_ids[i] = i;
  for (int j = 0; j < n_out; j++) out_ids[j] = n_src + j;
}

// Knobs are read once per process (A/B-able via env on the GPU box).
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// The same for byte counts, which need not fit an int.
static size_t env_size(const char* name, size_t dflt) {
  const char* e = getenv(name);
  return e ? (size_t)std::max(0L, atol(e)) : dflt;
}

// Blocking hipEventSynchronize/hipStreamSynchronize park the thread in
// the driver (~37 us each measured on MI355X, r1 profiles) — ruinous for
// sub-ms host calls (the OSD's real call shape is many small calls,
// ECUtil.cc:485-514). A bounded hipEventQuery/hipStreamQuery spin costs
// ~1-2 us when the work is already done or finishes soon; fall back to
// the blocking wait after ~500 us so large calls still park politely.
// ECX_SPINWAIT=0 disables.
static int env_spinwait() {
  static const int v = env_int("ECX_SPINWAIT", 1);
  return v;
}

static hipError_t wait_event(hipEvent_t ev) {
  if (env_spinwait()) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      hipError_t e = hipEventQuery(ev);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::steady_clock::now() - t0 >
          std::chrono::microseconds(500))
        break;
    }
  }
  return hipEventSynchronize(ev);
}

static hipError_t wait_stream(hipStream_t st) {
  if (env_spinwait()) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      hipError_t e = hipStreamQuery(st);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::steady_clock::now() - t0 >
          std::chrono::microseconds(500))
        break;
    }
  }
  return hipStreamSynchronize(st);
}

// ECX_NT=1 (nontemporal loads/stores) measured +7% encode bandwidth —
// streaming data with zero reuse should not occupy L1/L2
// (profiles/rocprof_r01_summary.md).
static bool env_nt() {
  static const int v = env_int("ECX_NT", 1);
  return v != 0;
}

// One-ahead source prefetch (PF template argument) for an n_out-output
// launch. ECX_PF: 0 = never, 1 = always, 2/unset = auto (NOUT >= 4, where
// the all-ones probe measured 15-20% exposed VALU; the NOUT <= 3 shapes are
// already at their memory floor). 3 selected the removed depth-2 experiment
// and now means 1.
static bool matmul_pf(int n_out) {
  static const int v = env_int("ECX_PF", 2);
  return v == 1 || v == 3 || (v == 2 && n_out >= 4);
}

// Grid/variant selection for the matmul kernel, shared by the slot-staged
// launch_matmul and the pipelined host path (which keeps params resident).
struct MatmulCfg {
  dim3 grid;
  bool nt;
};

static MatmulCfg matmul_cfg(long vecs, long n_stripes) {
  // ECX_TILE = target vectors per thread per launch. With NT on, TILE=2 won
  // the round-1 grid-shape sweep (6.0 TB/s encode,
  // profiles/rocprof_r01_summary.md).
  static const int env_tile = env_int("ECX_TILE", 2);
  const long loops = env_tile >= 1 ? env_tile : 2;
  const long tiles = (vecs + 255) / 256;
  int gx = (int)std::min<long>((tiles + loops - 1) / loops, 1024);
  if (gx < 1) gx = 1;
  // if few stripes, widen x so total blocks cover 256 CUs * a few waves
  while ((long)gx * n_stripes < 2048 && gx < tiles) gx *= 2;
  MatmulCfg c;
  c.grid = dim3(gx, (unsigned)n_stripes);
  c.nt = env_nt();
  return c;
}

// Runtime n_out (1-4) and flags to template arguments: fn is called with
// std::integral_constant<int, n_out> and one std::bool_constant per flag.
// Returns false (fn not called) when n_out is out of range.
template <class F>
static void dispatch_flags(F&& fn) {
  fn();
}
template <class F, class... Rest>
static void dispatch_flags(F&& fn, bool b, Rest... rest) {
  if (b)
    dispatch_flags([&](auto... c) { fn(std::true_type{}, c...); }, rest...);
  else
    dispatch_flags([&](auto... c) { fn(std::false_type{}, c...); }, rest...);
}
template <class F, class... Flags>
static bool dispatch_nout(int n_out, F&& fn, Flags... flags) {
#define ECX_NOUT_CASE(N)                                                  \
  case N:                                                                 \
    dispatch_flags(                                                       \
        [&](auto... c) { fn(std::integral_constant<int, N>{}, c...); },   \
        flags...);                                                        \
    return true;
  switch (n_out) {
    ECX_NOUT_CASE(1)
    ECX_NOUT_CASE(2)
    ECX_NOUT_CASE(3)
    ECX_NOUT_CASE(4)
  }
#undef ECX_NOUT_CASE
  return false;
}

// Launch for one output group (n_out <= 4) with params already resident on
// the device.
static int matmul_dispatch(hipStream_t stream, const uint8_t* d_buf,
                           uint8_t* d_obuf, const EcLaunchParams* d_params,
                           int n_out, bool accum, const MatmulCfg& c,
                           size_t chunk_bytes, int cps) {
  const bool ok = dispatch_nout(
      n_out,
      [&](auto NO, auto AC, auto NTF, auto PFD) {
        hipLaunchKernelGGL((ec_gf_matmul_kernel<NO(), AC(), NTF(), PFD()>),
                           c.grid, dim3(256), 0, stream, d_buf, d_obuf,
                           d_params, (long)chunk_bytes, cps,
                           (long)(chunk_bytes >> 4));
      },
      accum, c.nt, matmul_pf(n_out));
  if (!ok) return ECX_ERR_INVAL;
  HIP_TRY(hipGetLastError());
  return ECX_OK;
}

// Upload one launch record to the slot's device copy (a ring of one: waits
// for the previous upload before the pinned copy is rewritten).
static int upload_params(Slot& s, const EcLaunchParams& params) {
  HIP_TRY(wait_event(s.ev_param));
  std::memcpy(s.h_params, &params, sizeof(EcLaunchParams));
  HIP_TRY(hipMemcpyAsync(s.d_params, s.h_params, sizeof(EcLaunchParams),
                         hipMemcpyHostToDevice, s.stream));
  HIP_TRY(hipEventRecord(s.ev_param, s.stream));
  return ECX_OK;
}

// The event pair ecx_last_kernel_ms reads, around the launches between the
// two calls; `on` = this launch is the one the caller wants timed.
static hipError_t timer_start(Slot& s, bool on = true) {
  return on ? hipEventRecord(s.ev_start, s.stream) : hipSuccess;
}
static hipError_t timer_stop(Slot& s, bool on = true) {
  if (!on) return hipSuccess;
  const hipError_t e = hipEventRecord(s.ev_stop, s.stream);
  if (e == hipSuccess) s.timed = true;
  return e;
}

// Launch the matmul kernel for one output group (n_out <= 4).
static int launch_matmul(ecx_ctx* ctx, Slot& s, const uint8_t* d_buf,
                         uint8_t* d_obuf, const EcLaunchParams& params,
                         long n_stripes, size_t chunk_bytes, bool accum,
                         bool time_it) {
  if (chunk_bytes % 16 || n_stripes <= 0 || n_stripes > 65535)
    return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  int r = upload_params(s, params);
  if (r != ECX_OK) return r;

  const MatmulCfg c = matmul_cfg((long)(chunk_bytes >> 4), n_stripes);
  HIP_TRY(timer_start(s, time_it));
  r = matmul_dispatch(s.stream, d_buf, d_obuf, s.d_params, params.n_out,
                      accum, c, chunk_bytes, ctx->k + ctx->m);
  if (r != ECX_OK) return r;
  HIP_TRY(timer_stop(s, time_it));
  return ECX_OK;
}

// ---- streaming kernel (non-accumulating batch matmul) ----

// ECX_STREAM: unset/1 = ec_gf_stream_kernel for the non-accumulating batch
// matmul, 0 = ec_gf_matmul_kernel as before (A/B within one process lease).
static int env_stream() {
  static const int v = env_int("ECX_STREAM", 1);
  return v;
}

// ECX_STREAM_BPC: grid size. Unset = the measured default: one block per
// tile (1,048,576 blocks at the flagship shape; beyond 2^23 tiles the blocks
// grid-stride). N >= 1 = N blocks per CU (grid = min(tiles, CUs x N), each
// block grid-strides over its tiles); 0 = the persistent grid, as many
// blocks per CU as the occupancy query says stay resident. Measured at the
// flagship shape, grids of many short blocks beat every persistent grid by
// 4-5% on both legs (profiles/stream_kernel_summary.md), and under the
// XCD-contiguous mapping one tile per block beats two
// (profiles/stream_walk_summary.md).
static int env_stream_bpc() {
  static const int v =
      std::max(-1, std::min(env_int("ECX_STREAM_BPC", -1), 65536));
  return v;
}

// ECX_STREAM_ORDER: tile walk, 0/unset = tile-in-chunk fastest (concurrent
// blocks cover a few whole stripes), 1 = stripe fastest. These are the two
// ends of ECX_STREAM_W (widths 1 and n_stripes), which overrides it.
static int env_stream_order() {
  static const int v = env_int("ECX_STREAM_ORDER", 0);
  return v;
}

// ECX_STREAM_W: stripe-group width of the tile walk (stream_walk.h). N >= 1:
// tiles are walked (group of N stripes, tile in chunk, stripe in group);
// anything above the batch's stripe count means all of it. Unset: the width
// ECX_STREAM_ORDER stands for.
static int env_stream_w() {
  static const int v = std::max(-1, env_int("ECX_STREAM_W", -1));
  return v;
}

// ECX_STREAM_XCD: unset/1 = XCD-contiguous block mapping (each of the 8
// compute dies walks one contiguous eighth of the tile order instead of every
// 8th block of it), 0 = blocks in hardware order. Together with one tile per
// block it is worth 3-5% on both legs at the flagship shape
// (profiles/stream_walk_summary.md).
static int env_stream_xcd() {
  static const int v = env_int("ECX_STREAM_XCD", 1);
  return v;
}

template <int NO>
static hipError_t stream_occupancy(int* n, bool verify) {
  return verify ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      n, ec_gf_verify_kernel<NO>, 256, 0)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      n, ec_gf_stream_kernel<NO>, 256, 0);
}

// Grid size for n_tiles tiles (see ECX_STREAM_BPC). Both runtime figures
// (CU count, resident blocks per CU of the NOUT instance of the stream or the
// verify kernel) are cached in the context.
static int stream_grid(ecx_ctx* ctx, bool verify, int n_out, uint64_t n_tiles,
                       uint32_t* grid) {
  int cus = ctx->stream_cus.load();
  if (cus <= 0) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    cus = std::max(1, prop.multiProcessorCount);
    ctx->stream_cus.store(cus);
  }
  int bpc = env_stream_bpc();
  uint64_t g;
  if (bpc < 0) {
    g = n_tiles;
  } else {
    if (bpc == 0) {
      std::atomic<int>& occ =
          verify ? ctx->verify_occ[n_out] : ctx->stream_occ[n_out];
      bpc = occ.load();
      if (bpc <= 0) {
        hipError_t e = n_out == 1   ? stream_occupancy<1>(&bpc, verify)
                       : n_out == 2 ? stream_occupancy<2>(&bpc, verify)
                       : n_out == 3 ? stream_occupancy<3>(&bpc, verify)
                                    : stream_occupancy<4>(&bpc, verify);
        HIP_TRY(e);
        bpc = std::max(1, bpc);
        occ.store(bpc);
      }
    }
    g = (uint64_t)cus * (uint64_t)bpc;
  }
  // one block per tile at most, at least one block, and grid x 256 threads
  // well inside 32 bits
  g = std::min<uint64_t>(std::min<uint64_t>(g, n_tiles), 1ull << 23);
  *grid = (uint32_t)std::max<uint64_t>(1, g);
  return ECX_OK;
}

// Everything a launch of ec_gf_stream_kernel or ec_gf_verify_kernel passes
// besides its pointers.
struct StreamLaunch {
  EcStreamParams p;
  uint64_t stripe_bytes, vecs;
  uint32_t grid;
  EcxWalk walk;
};

// Argument block, grid and walk for one output group (n_out <= 4) of the
// stream kernel or, with `verify`, of the verify kernel, where the outputs
// are the checked chunks. coeff is n_out x n_src.
static int stream_prepare(ecx_ctx* ctx, bool verify, const int* src_ids,
                          int n_src, const int* out_ids, int n_out,
                          const uint8_t* coeff, const bool* src_null,
                          long n_stripes, size_t chunk_bytes,
                          StreamLaunch& L) {
  if (chunk_bytes % 16 || n_stripes <= 0 || n_stripes > 65535 || n_out < 1 ||
      n_out > ECX_STREAM_MAX_OUT)
    return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));

  const ecx::GF8& f = ecx::gf8();
  EcStreamParams& p = L.p;
  std::memset(&p, 0, sizeof(p));
  p.n_src = n_src;
  for (int i = 0; i < n_src; i++)
    p.src_off[i] = (uint64_t)src_ids[i] * chunk_bytes;
  for (int j = 0; j < n_out; j++) {
    p.out_off[j] = (uint64_t)out_ids[j] * chunk_bytes;
    p.out_id[j] = (uint8_t)out_ids[j];
    for (int i = 0; i < n_src; i++) {
      const uint8_t c = coeff[(size_t)j * n_src + i];
      if (c == 0 || (src_null && src_null[i])) continue;
      if (c == 1) {
        p.one_mask[j] |= 1u << i;
      } else {
        p.mul_mask[j] |= 1u << i;
        build_tabs332(f, c, p.tabs[i][j]);
      }
    }
  }

  L.vecs = chunk_bytes >> 4;
  const uint64_t tpc = (L.vecs + 255) / 256;  // tiles per chunk
  const uint64_t n_tiles = tpc * (uint64_t)n_stripes;
  L.grid = 1;
  int r = stream_grid(ctx, verify, n_out, n_tiles, &L.grid);
  if (r != ECX_OK) return r;
  int width = env_stream_w();
  if (width < 1) width = env_stream_order() == 1 ? (int)n_stripes : 1;
  L.walk =
      ecx_walk_make((uint32_t)n_stripes, (uint32_t)std::max<uint64_t>(1, tpc),
                    (uint32_t)width, env_stream_xcd() == 1, L.grid);
  L.stripe_bytes = (uint64_t)(ctx->k + ctx->m) * chunk_bytes;
  return ECX_OK;
}

// Launch ec_gf_stream_kernel for one output group (n_out <= 4). Nothing is
// staged on the device: the argument block is the launch's own kernarg.
static int launch_stream(ecx_ctx* ctx, Slot& s, const uint8_t* d_buf,
                         uint8_t* d_obuf, const int* src_ids, int n_src,
                         const int* out_ids, int n_out, const uint8_t* coeff,
                         const bool* src_null, long n_stripes,
                         size_t chunk_bytes, bool time_it) {
  StreamLaunch L;
  int r = stream_prepare(ctx, false, src_ids, n_src, out_ids, n_out, coeff,
                         src_null, n_stripes, chunk_bytes, L);
  if (r != ECX_OK) return r;
  HIP_TRY(timer_start(s, time_it));
  dispatch_nout(n_out, [&](auto NO) {
    hipLaunchKernelGGL((ec_gf_stream_kernel<NO()>), dim3(L.grid), dim3(256),
                       0, s.stream, d_buf, d_obuf, L.p, L.stripe_bytes,
                       L.vecs, L.walk);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(timer_stop(s, time_it));
  return ECX_OK;
}

// Run a full n_out job, splitting into groups of <= 4 outputs per launch.
static int run_matmul(ecx_ctx* ctx, int slot_i, const uint8_t* d_buf,
                      uint8_t* d_obuf, const int* src_ids, int n_src,
                      const int* out_ids, int n_out, const uint8_t* coeff,
                      const bool* src_null, long n_stripes, size_t chunk_bytes,
                      bool accum) {
  if (!ctx || slot_i < 0 || slot_i >= (int)ctx->slots.size() || n_src < 1 ||
      n_src > ECX_MAX_K || n_out < 1)
    return ECX_ERR_INVAL;
  Slot& s = ctx->slots[slot_i];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  // non-accumulating jobs go to the streaming kernel (its tile
  // counters are 32-bit; no real chunk comes near 2^31 tiles)
  const bool stream = !accum && env_stream() != 0 &&
                      (chunk_bytes >> 12) < 0x7fffffffull;
  for (int j0 = 0; j0 < n_out; j0 += 4) {
    int nj = std::min(4, n_out - j0);
    if (stream) {
      // rows j0..j0+nj of coeff are contiguous: n_out x n_src row-major
      int r = launch_stream(ctx, s, d_buf, d_obuf, src_ids, n_src,
                            out_ids + j0, nj, coeff + (size_t)j0 * n_src,
                            src_null, n_stripes, chunk_bytes, j0 == 0);
      if (r != ECX_OK) return r;
      continue;
    }
    EcLaunchParams p;
    fill_params(&p, src_ids, n_src, out_ids + j0, nj,
                coeff + (size_t)j0 * n_src, src_null);
    // time only the first group (the dominant kernel for bench)
    int r = launch_matmul(ctx, s, d_buf, d_obuf, p, n_stripes, chunk_bytes,
                          accum, j0 == 0);
    if (r != ECX_OK) return r;
  }
  return ECX_OK;
}

static int ensure_jobs(ecx_ctx* ctx, Slot& s, size_t bytes) {
  if (s.jobs_bytes >= bytes) return ECX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(wait_event(s.ev_jobs));
  if (s.h_jobs) (void)hipHostFree(s.h_jobs);
  if (s.d_jobs) (void)hipFree(s.d_jobs);
  s.h_jobs = nullptr;
  s.d_jobs = nullptr;
  s.jobs_bytes = 0;
  size_t want = bytes + bytes / 2 + 4096;  // grow with headroom
  HIP_TRY(hipHostMalloc(&s.h_jobs, want));
  HIP_TRY(hipMalloc(&s.d_jobs, want));
  s.jobs_bytes = want;
  return ECX_OK;
}

// The slot's job blob is a ring of one. open_jobs: room for `bytes`, and the
// previous upload has left the pinned copy — s.h_jobs may be written.
// send_jobs: s.h_jobs[0, bytes) to s.d_jobs on the slot's stream.
static int open_jobs(ecx_ctx* ctx, Slot& s, size_t bytes) {
  int r = ensure_jobs(ctx, s, bytes);
  if (r != ECX_OK) return r;
  HIP_TRY(wait_event(s.ev_jobs));
  return ECX_OK;
}

static int send_jobs(Slot& s, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(s.d_jobs, s.h_jobs, bytes, hipMemcpyHostToDevice,
                         s.stream));
  HIP_TRY(hipEventRecord(s.ev_jobs, s.stream));
  return ECX_OK;
}

using ecx::SLICE_VPB;
using ecx::slice_blocks;

// Device addresses of a slice job table, and its extent in s.h_jobs.
struct SliceJobs {
  const uint64_t* ptrs;    // [n_slices * cps]
  const long* slice_vecs;  // [n_slices]
  const long* block_voff;  // [n_blocks]
  const int* block_slice;  // [n_blocks]
  const int* block_rec;    // [n_blocks], only when recs are given
  long n_blocks;
  size_t bytes;
};

// Build the slice kernels' job table (slice_plan.h) in s.h_jobs behind `head`
// bytes the caller keeps for launch records. Blocks are assigned to the
// slices order[0..n_order) in that order (order == NULL: every slice once);
// recs[i], when given, is the record index of the blocks of order[i]. The
// caller has checked the arguments and uploads s.h_jobs[0, bytes).
static int build_slice_jobs(ecx_ctx* ctx, Slot& s, size_t head,
                            void* const* d_chunks, const size_t* bytes,
                            int n_slices, const int* order, const int* recs,
                            size_t n_order, SliceJobs* out) {
  const int cps = ctx->k + ctx->m;
  ecx::SliceLayout L;
  if (!ecx::plan_slice_layout(cps, bytes, n_slices, order, n_order,
                              recs != nullptr, head, L))
    return ECX_ERR_INVAL;
  int r = open_jobs(ctx, s, L.bytes);
  if (r != ECX_OK) return r;
  ecx::fill_slice_tables((uint8_t*)s.h_jobs, L, cps, d_chunks, bytes,
                         n_slices, order, recs, n_order);
  *out = {(const uint64_t*)(s.d_jobs + L.off_ptrs),
          (const long*)(s.d_jobs + L.off_vecs),
          (const long*)(s.d_jobs + L.off_voff),
          (const int*)(s.d_jobs + L.off_bslice),
          (const int*)(s.d_jobs + L.off_brec),
          L.n_blocks,
          L.bytes};
  return ECX_OK;
}

// Launch the variable-size slice kernel in groups of <= 4 outputs. The
// caller has validated the slot and the arrays (slice_call_ok, check_slices);
// the one refusal left, too many blocks, precedes the first enqueue too.
static int run_slices(ecx_ctx* ctx, int slot_i, void* const* d_chunks,
                      const size_t* bytes, int n_slices, const int* src_ids,
                      int n_src, const int* out_ids, int n_out,
                      const uint8_t* coeff) {
  if (n_src < 1 || n_src > ECX_MAX_K || n_out < 1) return ECX_ERR_INVAL;
  const int cps = ctx->k + ctx->m;
  Slot& s = ctx->slots[slot_i];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));

  SliceJobs jt;
  int r = build_slice_jobs(ctx, s, 0, d_chunks, bytes, n_slices, nullptr,
                           nullptr, (size_t)n_slices, &jt);
  if (r != ECX_OK) return r;
  r = send_jobs(s, jt.bytes);
  if (r != ECX_OK) return r;

  for (int j0 = 0; j0 < n_out; j0 += 4) {
    int nj = std::min(4, n_out - j0);
    EcLaunchParams p;
    // per-slice NULL chunks are handled inside the kernel, not via cls
    fill_params(&p, src_ids, n_src, out_ids + j0, nj,
                coeff + (size_t)j0 * n_src, nullptr);
    r = upload_params(s, p);
    if (r != ECX_OK) return r;
    dispatch_nout(
        nj,
        [&](auto NO, auto NTF) {
          hipLaunchKernelGGL((ec_gf_slices_kernel<NO(), NTF()>),
                             dim3((unsigned)jt.n_blocks), dim3(256), 0,
                             s.stream, jt.ptrs, jt.block_slice, jt.block_voff,
                             jt.slice_vecs, s.d_params, cps, SLICE_VPB);
        },
        env_nt());
    HIP_TRY(hipGetLastError());
  }
  return ECX_OK;
}

// The ECX_BIT* knobs that bit_plan() acts on (bit_plan.h), as given.
static const ecx::BitKnobs& env_bit_knobs() {
  static const ecx::BitKnobs kn = {
      env_int("ECX_BITQ", 16),   env_int("ECX_BITW", 8),
      env_int("ECX_BITREG", 2),  env_int("ECX_BITPIPE", 0),
      env_int("ECX_BITT", 256),  env_int("ECX_BITXCD", 0)};
  return kn;
}

// Launch the bitmatrix kernel for <= ECX_MAX_OUT output chunks whose bit
// rows (n_out*w x n_src*w) are given over the source chunk ids. Which
// kernel, window, grid and LDS size: bit_plan().
static int run_bitmatrix(ecx_ctx* ctx, int slot_i, const uint8_t* d_buf,
                         uint8_t* d_obuf, const int* src_ids, int n_src,
                         const int* out_ids, int n_out,
                         const uint8_t* bit_rows, long n_stripes,
                         size_t chunk_bytes, bool time_it,
                         bool accum = false) {
  const int w = ctx->w, pkt = ctx->pkt, cps = ctx->k + ctx->m;
  // bit_rows is only as large as an admissible n_src x n_out makes it
  if (n_src < 1 || n_src > ecx::BIT_MAX_SRC || n_out < 1 ||
      n_out > ECX_MAX_OUT || n_stripes <= 0 || n_stripes > 65535)
    return ECX_ERR_INVAL;
  const size_t n_ops = ecx::bit_count_ops(bit_rows, w, n_src, n_out);
  ecx::BitPlan p;
  int r = ecx::bit_plan(env_bit_knobs(), w, pkt, n_src, n_out, n_ops,
                        chunk_bytes, &p);
  if (r != ECX_OK) return r;
  Slot& s = ctx->slots[slot_i];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));

  const bool reg = p.kernel == ecx::BIT_REG;
  const size_t blob =
      reg ? sizeof(EcBitRegParams) : ecx::bit_lds_blob_bytes(n_ops);
  r = open_jobs(ctx, s, blob);
  if (r != ECX_OK) return r;
  if (reg)
    ecx::bit_fill_reg_blob(pkt, src_ids, n_src, out_ids, n_out, bit_rows,
                           (EcBitRegParams*)s.h_jobs);
  else
    ecx::bit_fill_lds_blob(p, w, pkt, src_ids, n_src, out_ids, n_out,
                           bit_rows, s.h_jobs);
  r = send_jobs(s, blob);
  if (r != ECX_OK) return r;

  static const int stagger = env_int("ECX_BITSTAGGER", 0);
  const dim3 grid((unsigned)p.grid_x, (unsigned)n_stripes);
  HIP_TRY(timer_start(s, time_it));
  dispatch_flags(
      [&](auto NTF, auto AC) {
        constexpr bool NT = decltype(NTF)::value, A = decltype(AC)::value;
        auto lds = [&](auto VQS) {
          hipLaunchKernelGGL(
              (ec_bitmatrix_kernel<NT, A, decltype(VQS)::value>), grid,
              dim3(p.threads), p.lds_bytes, s.stream, d_buf, d_obuf, s.d_jobs,
              (long)chunk_bytes, cps, p.windows_per_sw, p.wpb, p.n_windows,
              stagger, p.xcdmap);
        };
        if (reg)
          dispatch_nout(n_out, [&](auto NO) {
            hipLaunchKernelGGL(
                (ec_bitmatrix_reg_kernel<NT, A, 8 * decltype(NO)::value>),
                grid, dim3(256), 0, s.stream, d_buf, d_obuf, s.d_jobs,
                (long)chunk_bytes, cps, p.n_pos);
          });
        else if (p.kernel == ecx::BIT_PIPE)
          hipLaunchKernelGGL((ec_bitmatrix_pipe_kernel<NT, A>), grid,
                             dim3(256), p.lds_bytes, s.stream, d_buf, d_obuf,
                             s.d_jobs, (long)chunk_bytes, cps,
                             p.windows_per_sw, p.wpb, p.n_windows);
        else
          switch (p.vqs) {
            case 3: lds(std::integral_constant<int, 3>{}); break;
            case 4: lds(std::integral_constant<int, 4>{}); break;
            case 5: lds(std::integral_constant<int, 5>{}); break;
            default: lds(std::integral_constant<int, -1>{}); break;
          }
      },
      env_nt(), accum);
  HIP_TRY(hipGetLastError());
  HIP_TRY(timer_stop(s, time_it));
  return ECX_OK;
}

// w=16 tables: 20 dwords per coefficient (see EcLaunch16).
static void build_tabs16(const ecx::GF16& f, uint16_t c, uint32_t* T) {
  for (int plane = 0; plane < 2; plane++) {
    uint32_t* P = T + plane * 10;
    for (int np = 0; np < 4; np++) {
      uint8_t e[8];
      for (int v = 0; v < 8; v++) {
        uint16_t r = f.mul(c, (uint16_t)(v << (4 * np)));
        e[v] = plane ? (uint8_t)(r >> 8) : (uint8_t)r;
      }
      P[np * 2] = e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)e[3] << 24);
      P[np * 2 + 1] =
          e[4] | (e[5] << 8) | (e[6] << 16) | ((uint32_t)e[7] << 24);
    }
    uint16_t w01[4] = {0, f.mul(c, 8), f.mul(c, 128),
                       (uint16_t)(f.mul(c, 8) ^ f.mul(c, 128))};
    uint16_t w23[4] = {0, f.mul(c, (uint16_t)(1u << 11)),
                       f.mul(c, (uint16_t)(1u << 15)),
                       (uint16_t)(f.mul(c, (uint16_t)(1u << 11)) ^
                                  f.mul(c, (uint16_t)(1u << 15)))};
    uint32_t a = 0, b = 0;
    for (int sidx = 0; sidx < 4; sidx++) {
      a |= (uint32_t)(plane ? (w01[sidx] >> 8) : (w01[sidx] & 0xff))
           << (8 * sidx);
      b |= (uint32_t)(plane ? (w23[sidx] >> 8) : (w23[sidx] & 0xff))
           << (8 * sidx);
    }
    P[8] = a;
    P[9] = b;
  }
}

// Launch the w=16 kernel for <= 4 output rows per group.
static int run_matmul16(ecx_ctx* ctx, int slot_i, const uint8_t* d_buf,
                        uint8_t* d_obuf, const int* src_ids, int n_src,
                        const int* out_ids, int n_out,
                        const uint16_t* coeff, long n_stripes,
                        size_t chunk_bytes, bool accum, bool time_all) {
  if (!ctx || slot_i < 0 || slot_i >= (int)ctx->slots.size() || n_src < 1 ||
      n_src > ECX_MAX_K || n_out < 1)
    return ECX_ERR_INVAL;
  if (chunk_bytes % 16 || n_stripes <= 0 || n_stripes > 65535)
    return ECX_ERR_INVAL;
  Slot& s = ctx->slots[slot_i];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));
  const ecx::GF16& f = ecx::gf16();
  const long vecs = (long)(chunk_bytes >> 4);
  int gx = (int)std::min<long>((vecs + 256 * 2 - 1) / (256 * 2), 1024);
  if (gx < 1) gx = 1;
  long tiles = (vecs + 255) / 256;
  while ((long)gx * n_stripes < 2048 && gx < tiles) gx *= 2;
  dim3 grid(gx, (unsigned)n_stripes);
  const int cps = ctx->k + ctx->m;

  for (int j0 = 0; j0 < n_out; j0 += 4) {
    int nj = std::min(4, n_out - j0);
    EcLaunch16 p;
    std::memset(&p, 0, sizeof(p));
    p.n_src = n_src;
    p.n_out = nj;
    for (int i = 0; i < n_src; i++) p.src_ids[i] = src_ids[i];
    for (int j = 0; j < nj; j++) p.out_ids[j] = out_ids[j0 + j];
    for (int j = 0; j < nj; j++)
      for (int i = 0; i < n_src; i++) {
        uint16_t c = coeff[(size_t)(j0 + j) * n_src + i];
        uint8_t cls = (c == 0) ? 0 : (c == 1 ? 1 : 2);
        p.cls[j * n_src + i] = cls;
        if (cls == 2) build_tabs16(f, c, &p.tabs[(j * n_src + i) * 20]);
      }
    size_t blob = sizeof(EcLaunch16);
    int r = open_jobs(ctx, s, blob);
    if (r != ECX_OK) return r;
    std::memcpy(s.h_jobs, &p, blob);
    r = send_jobs(s, blob);
    if (r != ECX_OK) return r;
    HIP_TRY(timer_start(s, j0 == 0 && time_all));
    dispatch_nout(
        nj,
        [&](auto NO, auto AC, auto NTF) {
          hipLaunchKernelGGL((ec_gf16_matmul_kernel<NO(), AC(), NTF()>), grid,
                             dim3(256), 0, s.stream, d_buf, d_obuf, s.d_jobs,
                             (long)chunk_bytes, cps, vecs);
        },
        accum, env_nt());
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer_stop(s, time_all));
  }
  return ECX_OK;
}

// Apply rows (n_out x n_src, in the context's technique) to the stripes of
// d_buf in place: the one technique dispatch of the batch and the
// host-pointer calls. src_null marks zeros-chunk sources for the w=8
// kernels; the other two read every source. time_it goes to the bitmatrix
// and w=16 launchers; run_matmul always times its first group.
static int run_coded(ecx_ctx* ctx, int slot_i, uint8_t* d_buf,
                     const int* src_ids, int n_src, const int* out_ids,
                     int n_out, CodeRows rows, const bool* src_null,
                     long n_stripes, size_t chunk_bytes, bool time_it) {
  if (slot_i < 0 || slot_i >= (int)ctx->slots.size()) return ECX_ERR_INVAL;
  if (ctx->is_bitmatrix()) {
    const size_t out_bits = (size_t)ctx->w * n_src * ctx->w;  // per output
    for (int j0 = 0; j0 < n_out; j0 += ECX_MAX_OUT) {
      int r = run_bitmatrix(ctx, slot_i, d_buf, d_buf, src_ids, n_src,
                            out_ids + j0, std::min(ECX_MAX_OUT, n_out - j0),
                            rows.r8 + j0 * out_bits, n_stripes, chunk_bytes,
                            time_it);
      if (r != ECX_OK) return r;
    }
    return ECX_OK;
  }
  if (ctx->is_w16())
    return run_matmul16(ctx, slot_i, d_buf, d_buf, src_ids, n_src, out_ids,
                        n_out, rows.r16, n_stripes, chunk_bytes, false,
                        time_it);
  return run_matmul(ctx, slot_i, d_buf, d_buf, src_ids, n_src, out_ids, n_out,
                    rows.r8, src_null, n_stripes, chunk_bytes, false);
}

// Decode plan for a mask through the context's LRU, composed for the
// context's technique on a miss.
static int get_decode_plan(ecx_ctx* ctx, uint64_t present_mask,
                           DecodePlan& out) {
  std::lock_guard<std::mutex> g(ctx->lru_mu);
  auto it = ctx->lru.find(present_mask);
  if (it != ctx->lru.end()) {
    ctx->lru_order.erase(it->second.second);
    ctx->lru_order.push_front(present_mask);
    it->second.second = ctx->lru_order.begin();
    out = it->second.first;
    return ECX_OK;
  }
  DecodePlan plan;
  const int k = ctx->k, m = ctx->m;
  const bool ok =
      ctx->is_w16()
          ? ecx::compose_decode_rows16(ctx->gen16, k, m, present_mask,
                                       plan.survivors, plan.erased,
                                       plan.rows16)
      : ctx->is_bitmatrix()
          ? ecx::compose_bit_decode_rows(ctx->bitmat, k, m, ctx->w,
                                         present_mask, plan.survivors,
                                         plan.erased, plan.rows)
          : ecx::compose_decode_rows(ctx->gen, k, m, present_mask,
                                     plan.survivors, plan.erased, plan.rows);
  if (!ok) return ECX_ERR_IO;
  ctx->lru_order.push_front(present_mask);
  ctx->lru.emplace(present_mask,
                   std::make_pair(plan, ctx->lru_order.begin()));
  if (ctx->lru.size() > ecx_ctx::LRU_DEPTH) {
    ctx->lru.erase(ctx->lru_order.back());
    ctx->lru_order.pop_back();
  }
  out = plan;
  return ECX_OK;
}

// ---- per-stripe erasure patterns: host side ----
static_assert(ECX_MULTI_OUT == ecx::MULTI_MAX_OUT, "kernel/grouping split");
static_assert(ECX_MULTI_OUT == ecx::UPDATE_MAX_OUT, "kernel/update-plan split");
static_assert(sizeof(EcMultiRec) % 8 == 0, "8-byte arrays follow the table");

// Group a call's masks (decode_multi.h) and fetch every distinct mask's
// plan through the LRU; plans[i] belongs to g.masks[i]. ECX_ERR_IO if any
// mask is undecodable — before anything is staged or launched.
static int multi_resolve(ecx_ctx* ctx, const uint64_t* masks, long n,
                         ecx::MultiGrouping& g,
                         std::vector<DecodePlan>& plans) {
  plans.clear();
  auto resolve = [&](uint64_t mask) {
    DecodePlan p;
    if (get_decode_plan(ctx, mask, p) != ECX_OK) return false;
    plans.push_back(std::move(p));
    return true;
  };
  if (!ecx::group_decode_masks(ctx->k, ctx->m, masks, n, resolve, g))
    return ECX_ERR_IO;
  return ECX_OK;
}

// Launch records [plan * n_pass + pass]; passes a plan does not have stay
// zeroed and are never referenced.
static void multi_fill_recs(EcMultiRec* recs, const ecx::MultiGrouping& g,
                            const std::vector<DecodePlan>& plans, int k) {
  std::memset(recs, 0, sizeof(EcMultiRec) * plans.size() * g.n_pass);
  for (size_t pl = 0; pl < plans.size(); pl++) {
    const DecodePlan& dp = plans[pl];
    const int e = (int)dp.erased.size();
    for (int j0 = 0; j0 < e; j0 += ECX_MULTI_OUT)
      fill_rec(&recs[pl * g.n_pass + j0 / ECX_MULTI_OUT], dp.survivors.data(),
               k, dp.erased.data() + j0, std::min(ECX_MULTI_OUT, e - j0),
               dp.rows.data() + (size_t)j0 * k, nullptr);
  }
}

// ---- consistency check: host side ----
static_assert(ECX_STREAM_MAX_OUT == ecx::VERIFY_MAX_OUT,
              "kernel/verify-plan split");

static int verify_err(ecx::VerifyStatus st) {
  return st == ecx::VERIFY_OK      ? ECX_OK
         : st == ecx::VERIFY_INVAL ? ECX_ERR_INVAL
                                   : ECX_ERR_IO;
}

// What both verify calls refuse about the context and the shape (the tile
// counters of the kernel are 32-bit, as for the stream kernel).
static int verify_check_args(const ecx_ctx* ctx, long n_stripes,
                             size_t chunk_bytes) {
  if (!ctx->is_table8() || chunk_bytes == 0 || chunk_bytes % 16 ||
      (chunk_bytes >> 12) >= 0x7fffffffull || n_stripes <= 0 ||
      n_stripes > 65535)
    return ECX_ERR_INVAL;
  return ECX_OK;
}

// Verify plan of a mask (verify_plan.h), its decode plan through the LRU.
static int get_verify_plan(ecx_ctx* ctx, uint64_t present_mask,
                           ecx::VerifyPlan& vp) {
  auto resolve = [&](uint64_t mask, std::vector<int>& sv, std::vector<int>& er,
                     std::vector<uint8_t>& rw) {
    DecodePlan dp;
    if (get_decode_plan(ctx, mask, dp) != ECX_OK) return false;
    sv = std::move(dp.survivors);
    er = std::move(dp.erased);
    rw = std::move(dp.rows);
    return true;
  };
  return verify_err(
      ecx::plan_verify(ctx->k, ctx->m, present_mask, resolve, vp));
}

// Zero d_bad, then check the plan's chunks in passes of <= 4, back to back
// under one event pair. Arguments are validated and the slot is locked by the
// caller; every pass is prepared before anything is enqueued.
static int run_verify(ecx_ctx* ctx, Slot& s, const uint8_t* d_buf,
                      long n_stripes, size_t chunk_bytes,
                      const ecx::VerifyPlan& vp, uint64_t* d_bad) {
  const int k = ctx->k, n = (int)vp.checked.size();
  std::vector<StreamLaunch> passes((size_t)(n + ECX_STREAM_MAX_OUT - 1) /
                                   ECX_STREAM_MAX_OUT);
  for (int j0 = 0; j0 < n; j0 += ECX_STREAM_MAX_OUT) {
    int r = stream_prepare(ctx, true, vp.survivors.data(), k,
                           vp.checked.data() + j0,
                           std::min(ECX_STREAM_MAX_OUT, n - j0),
                           vp.rows.data() + (size_t)j0 * k, nullptr, n_stripes,
                           chunk_bytes, passes[j0 / ECX_STREAM_MAX_OUT]);
    if (r != ECX_OK) return r;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(d_bad, 0, (size_t)n_stripes * 8, s.stream));
  if (n == 0) return ECX_OK;  // nothing to check: zeros, nothing launched
  HIP_TRY(timer_start(s));
  for (int j0 = 0; j0 < n; j0 += ECX_STREAM_MAX_OUT) {
    const StreamLaunch& L = passes[j0 / ECX_STREAM_MAX_OUT];
    dispatch_nout(std::min(ECX_STREAM_MAX_OUT, n - j0), [&](auto NO) {
      hipLaunchKernelGGL((ec_gf_verify_kernel<NO()>), dim3(L.grid), dim3(256),
                         0, s.stream, d_buf, (unsigned long long*)d_bad, L.p,
                         L.stripe_bytes, L.vecs, L.walk);
    });
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(timer_stop(s));
  return ECX_OK;
}

extern "C" {

int ecx_encode_batch(ecx_ctx* ctx, void* dptr, long n_stripes,
                     size_t chunk_bytes, int slot) {
  if (!ctx || !dptr) return ECX_ERR_INVAL;
  // the bitmatrix batch calls take their outputs in one launch
  if (ctx->is_bitmatrix() && ctx->m > ECX_MAX_OUT) return ECX_ERR_INVAL;
  int src_ids[ECX_MAX_K], out_ids[ECX_MAX_K];
  stripe_ids(ctx->k, ctx->m, src_ids, out_ids);
  return run_coded(ctx, slot, (uint8_t*)dptr, src_ids, ctx->k, out_ids,
                   ctx->m, ctx->gen_rows(), nullptr, n_stripes, chunk_bytes,
                   /*time_it=*/true);
}

int ecx_decode_batch(ecx_ctx* ctx, void* dptr, long n_stripes,
                     size_t chunk_bytes, uint64_t present_mask, int slot) {
  if (!ctx || !dptr) return ECX_ERR_INVAL;
  // a bad slot is refused before the plan, as it always was for bitmatrix
  if (ctx->is_bitmatrix() && (slot < 0 || slot >= (int)ctx->slots.size()))
    return ECX_ERR_INVAL;
  DecodePlan plan;
  int r = get_decode_plan(ctx, present_mask, plan);
  if (r != ECX_OK) return r;
  if (plan.erased.empty()) return ECX_OK;
  // the bitmatrix batch calls take their outputs in one launch
  if (ctx->is_bitmatrix() && plan.erased.size() > ECX_MAX_OUT)
    return ECX_ERR_INVAL;
  return run_coded(ctx, slot, (uint8_t*)dptr, plan.survivors.data(), ctx->k,
                   plan.erased.data(), (int)plan.erased.size(),
                   {plan.rows.data(), plan.rows16.data()}, nullptr, n_stripes,
                   chunk_bytes, /*time_it=*/true);
}

int ecx_encode_delta_dev(ecx_ctx* ctx, const void* d_old, const void* d_new,
                         void* d_delta, size_t bytes, int slot) {
  if (!ctx || slot < 0 || slot >= (int)ctx->slots.size() || (bytes & 15))
    return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  long n_vecs = (long)(bytes >> 4);
  int blocks = (int)std::min<long>((n_vecs + 255) / 256, 8192);
  hipLaunchKernelGGL(ec_xor_kernel, dim3(blocks), dim3(256), 0,
                     ctx->slots[slot].stream, (const uint8_t*)d_old,
                     (const uint8_t*)d_new, (uint8_t*)d_delta, n_vecs);
  HIP_TRY(hipGetLastError());
  return ECX_OK;
}

int ecx_apply_delta_dev(ecx_ctx* ctx, const void* d_delta, int data_shard,
                        int coding_shard, void* d_parity, size_t bytes,
                        int slot) {
  // parity ^= gen[coding_shard][data_shard] * delta
  // (matrix_apply_delta, ErasureCodeJerasure.cc:285-331 / isa
  // ec_encode_data_update one-row form, ErasureCodeIsa.cc:356-362)
  if (!ctx || data_shard < 0 || data_shard >= ctx->k || coding_shard < ctx->k ||
      coding_shard >= ctx->k + ctx->m)
    return ECX_ERR_INVAL;
  if (ctx->is_w16()) {
    uint16_t c16 = ctx->gen16[(size_t)coding_shard * ctx->k + data_shard];
    int sids[1] = {0}, oids[1] = {0};
    uint16_t cf[1] = {c16};
    return run_matmul16(ctx, slot, (const uint8_t*)d_delta,
                        (uint8_t*)d_parity, sids, 1, oids, 1, cf, 1, bytes,
                        true, false);
  }
  if (ctx->is_bitmatrix()) {
    // schedule-delta apply (schedule_apply_delta filtered to one
    // (datashard, codingshard) pair, ErasureCodeJerasure.cc:348-377):
    // the pair's w x w bitmatrix block applied per superword, XORed into
    // the existing parity. Extract block (i, j) as w bit rows over one
    // source chunk.
    const int w = ctx->w, W = ctx->k * w;
    const int i = coding_shard - ctx->k, j = data_shard;
    std::vector<uint8_t> rows((size_t)w * w);
    for (int r = 0; r < w; r++)
      for (int c = 0; c < w; c++)
        rows[(size_t)r * w + c] =
            ctx->bitmat[(size_t)(i * w + r) * W + j * w + c];
    int sids[1] = {0}, oids[1] = {0};
    return run_bitmatrix(ctx, slot, (const uint8_t*)d_delta,
                         (uint8_t*)d_parity, sids, 1, oids, 1, rows.data(),
                         1, bytes, false, /*accum=*/true);
  }
  uint8_t c = ctx->gen[(size_t)coding_shard * ctx->k + data_shard];
  int src_ids[1] = {0};
  int out_ids[1] = {0};
  uint8_t coeff[1] = {c};
  // Treat delta and parity as 1-chunk "stripes" at the given pointers:
  // chunk_bytes = bytes, chunks_per_stripe irrelevant with single stripe.
  return run_matmul(ctx, slot, (const uint8_t*)d_delta, (uint8_t*)d_parity,
                    src_ids, 1, out_ids, 1, coeff, nullptr, 1, bytes, true);
}

// What every slice call refuses before it looks at the arrays' contents.
static bool slice_call_ok(ecx_ctx* ctx, void* const* d_chunks,
                          const size_t* bytes, int slot) {
  return ctx && d_chunks && bytes && slot >= 0 &&
         slot < (int)ctx->slots.size() && !ctx->is_bitmatrix() &&
         !ctx->is_w16();
}

static uint64_t low_mask(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

int ecx_encode_slices(ecx_ctx* ctx, void* const* d_chunks,
                      const size_t* bytes, int n_slices, int slot) {
  if (!slice_call_ok(ctx, d_chunks, bytes, slot)) return ECX_ERR_INVAL;
  int k = ctx->k, m = ctx->m;
  // parity chunks k..k+m-1 of every slice are written
  const uint64_t written = low_mask(k + m) & ~low_mask(k);
  if (!ecx::check_slices(k + m, d_chunks, bytes, n_slices, &written, 0))
    return ECX_ERR_INVAL;
  int src_ids[ECX_MAX_K], out_ids[ECX_MAX_K];
  stripe_ids(k, m, src_ids, out_ids);
  return run_slices(ctx, slot, d_chunks, bytes, n_slices, src_ids, k,
                    out_ids, m, ctx->gen.data() + (size_t)k * k);
}

int ecx_decode_slices(ecx_ctx* ctx, void* const* d_chunks,
                      const size_t* bytes, int n_slices,
                      uint64_t present_mask, int slot) {
  if (!slice_call_ok(ctx, d_chunks, bytes, slot) ||
      !ecx::check_slice_sizes(bytes, n_slices))
    return ECX_ERR_INVAL;
  DecodePlan plan;
  int r = get_decode_plan(ctx, present_mask, plan);
  if (r != ECX_OK) return r;
  // the erased chunks of every slice are written; a full mask still has its
  // pointers checked before it returns
  uint64_t written = 0;
  for (int e : plan.erased) written |= 1ull << e;
  if (!ecx::check_slice_ptrs(ctx->k + ctx->m, d_chunks, n_slices, &written,
                             0))
    return ECX_ERR_INVAL;
  if (plan.erased.empty()) return ECX_OK;
  return run_slices(ctx, slot, d_chunks, bytes, n_slices,
                    plan.survivors.data(), ctx->k, plan.erased.data(),
                    (int)plan.erased.size(), plan.rows.data());
}

int ecx_decode_batch_multi(ecx_ctx* ctx, void* dptr, long n_stripes,
                           size_t chunk_bytes, const uint64_t* present_masks,
                           int slot) {
  if (!ctx || !dptr || !present_masks || slot < 0 ||
      slot >= (int)ctx->slots.size() || ctx->is_bitmatrix() ||
      ctx->is_w16() || chunk_bytes == 0 || chunk_bytes % 16 ||
      n_stripes <= 0 || n_stripes > 65535)
    return ECX_ERR_INVAL;
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));

  // every mask is resolved (and refused) before anything is staged
  ecx::MultiGrouping grp;
  std::vector<DecodePlan> plans;
  int r = multi_resolve(ctx, present_masks, n_stripes, grp, plans);
  if (r != ECX_OK) return r;
  if (grp.launches.empty()) return ECX_OK;  // nothing erased anywhere

  // blob: [records][plan_of_stripe i32][stripe lists i32, launch order]
  const size_t n_recs = plans.size() * (size_t)grp.n_pass;
  size_t n_listed = 0;
  for (const auto& l : grp.launches) n_listed += l.members.size();
  const size_t off_pos = n_recs * sizeof(EcMultiRec);
  const size_t off_list = off_pos + (size_t)n_stripes * 4;
  const size_t blob = off_list + n_listed * 4;
  r = open_jobs(ctx, s, blob);
  if (r != ECX_OK) return r;
  multi_fill_recs((EcMultiRec*)s.h_jobs, grp, plans, ctx->k);
  std::memcpy(s.h_jobs + off_pos, grp.plan_of_stripe.data(),
              (size_t)n_stripes * 4);
  {
    int* list = (int*)(s.h_jobs + off_list);
    for (const auto& l : grp.launches) {
      std::memcpy(list, l.members.data(), l.members.size() * 4);
      list += l.members.size();
    }
  }
  r = send_jobs(s, blob);
  if (r != ECX_OK) return r;

  uint8_t* buf = (uint8_t*)dptr;
  const EcMultiRec* d_recs = (const EcMultiRec*)s.d_jobs;
  const int* d_pos = (const int*)(s.d_jobs + off_pos);
  const int* d_list = (const int*)(s.d_jobs + off_list);
  const long vecs = (long)(chunk_bytes >> 4);
  // one event pair around the whole call, launches back to back
  HIP_TRY(timer_start(s));
  for (const auto& l : grp.launches) {
    const MatmulCfg c = matmul_cfg(vecs, (long)l.members.size());
    const bool ok = dispatch_nout(
        l.n_out,
        [&](auto NO, auto NTF, auto PFD) {
          hipLaunchKernelGGL(
              (ec_gf_matmul_multi_kernel<NO(), NTF(), PFD()>), c.grid,
              dim3(256), 0, s.stream, buf, buf, d_recs, d_pos, d_list, ctx->k,
              l.pass, grp.n_pass, (long)chunk_bytes, ctx->k + ctx->m, vecs);
        },
        c.nt, matmul_pf(l.n_out));
    if (!ok) return ECX_ERR_INVAL;
    HIP_TRY(hipGetLastError());
    d_list += l.members.size();
  }
  HIP_TRY(timer_stop(s));
  return ECX_OK;
}

int ecx_decode_slices_multi(ecx_ctx* ctx, void* const* d_chunks,
                            const size_t* bytes, int n_slices,
                            const uint64_t* present_masks, int slot) {
  if (!slice_call_ok(ctx, d_chunks, bytes, slot) || !present_masks ||
      !ecx::check_slice_sizes(bytes, n_slices))
    return ECX_ERR_INVAL;
  const int k = ctx->k, cps = ctx->k + ctx->m;
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));

  ecx::MultiGrouping grp;
  std::vector<DecodePlan> plans;
  int r = multi_resolve(ctx, present_masks, n_slices, grp, plans);
  if (r != ECX_OK) return r;
  // an erased chunk is written: it needs a buffer (NULL only ever means a
  // zeros SOURCE)
  {
    std::vector<uint64_t> written((size_t)n_slices);
    for (int i = 0; i < n_slices; i++)
      written[i] = ~present_masks[i] & low_mask(cps);
    if (!ecx::check_slice_ptrs(cps, d_chunks, n_slices, written.data(), 1))
      return ECX_ERR_INVAL;
  }
  if (grp.launches.empty()) return ECX_OK;

  // job table behind the records, block tables in launch order
  std::vector<int> order, rec_of;
  for (const auto& l : grp.launches)
    for (int sl : l.members) {
      order.push_back(sl);
      rec_of.push_back(grp.plan_of_stripe[sl] * grp.n_pass + l.pass);
    }
  const size_t n_recs = plans.size() * (size_t)grp.n_pass;
  SliceJobs jt;
  r = build_slice_jobs(ctx, s, n_recs * sizeof(EcMultiRec), d_chunks, bytes,
                       n_slices, order.data(), rec_of.data(), order.size(),
                       &jt);
  if (r != ECX_OK) return r;
  multi_fill_recs((EcMultiRec*)s.h_jobs, grp, plans, k);
  r = send_jobs(s, jt.bytes);
  if (r != ECX_OK) return r;

  HIP_TRY(timer_start(s));
  long b0 = 0;
  for (const auto& l : grp.launches) {
    long nb = 0;
    for (int sl : l.members) nb += slice_blocks(bytes[sl]);
    const bool ok = dispatch_nout(
        l.n_out,
        [&](auto NO, auto NTF) {
          hipLaunchKernelGGL((ec_gf_slices_multi_kernel<NO(), NTF()>),
                             dim3((unsigned)nb), dim3(256), 0, s.stream,
                             jt.ptrs, jt.block_slice + b0, jt.block_voff + b0,
                             jt.block_rec + b0, jt.slice_vecs,
                             (const EcMultiRec*)s.d_jobs, k, cps, SLICE_VPB);
        },
        env_nt());
    if (!ok) return ECX_ERR_INVAL;
    HIP_TRY(hipGetLastError());
    b0 += nb;
  }
  HIP_TRY(timer_stop(s));
  return ECX_OK;
}

int ecx_decode_multi_plan_probe(int technique, int k, int m,
                                const uint64_t* present_masks, long n,
                                int* plan_of_stripe, int* n_plans) {
  // CPU-only: the grouping the two calls above perform (same
  // group_decode_masks, plans composed directly instead of via a context's
  // LRU). Outputs are written only on success.
  if (!present_masks || !plan_of_stripe || !n_plans || n <= 0 ||
      n > 0x7fffffffL || k < 1 || m < 1 || k + m > 64)
    return ECX_ERR_INVAL;
  if (technique != ECX_T_RS_VAN_ISA && technique != ECX_T_CAUCHY_ISA &&
      technique != ECX_T_RS_VAN_JERASURE)
    return ECX_ERR_INVAL;  // w=8 matrix techniques only, like the calls
  std::vector<uint8_t> gen;
  if (!ecx::gen_matrix(technique, gen, k, m)) return ECX_ERR_INVAL;
  auto resolve = [&](uint64_t mask) {
    std::vector<int> sv, er;
    std::vector<uint8_t> rw;
    return ecx::compose_decode_rows(gen, k, m, mask, sv, er, rw);
  };
  ecx::MultiGrouping grp;
  if (!ecx::group_decode_masks(k, m, present_masks, n, resolve, grp))
    return ECX_ERR_IO;
  std::memcpy(plan_of_stripe, grp.plan_of_stripe.data(), (size_t)n * 4);
  *n_plans = (int)grp.masks.size();
  return (int)grp.launches.size();
}

int ecx_slice_plan_probe(int cps, void* const* chunks, const size_t* bytes,
                         int n_slices, const uint64_t* written_masks,
                         const int* order, const int* recs, long n_order,
                         size_t head, long out[8], void* blob,
                         size_t blob_cap) {
  // CPU-only: the check, the layout and the table fill of the slice calls
  // (slice_plan.h), into a host buffer of exactly the blob's size. Outputs
  // are written only on success.
  if (!out || cps < 1 || cps > 64 || (recs && !order) ||
      (order && n_order < 0) || (blob_cap && !blob))
    return ECX_ERR_INVAL;
  if (!ecx::check_slices(cps, chunks, bytes, n_slices, written_masks, 1))
    return ECX_ERR_INVAL;
  ecx::SliceLayout L;
  if (!ecx::plan_slice_layout(cps, bytes, n_slices, order, (size_t)n_order,
                              recs != nullptr, head, L))
    return ECX_ERR_INVAL;
  if (blob_cap) {
    std::vector<uint8_t> tab(L.bytes, 0);
    ecx::fill_slice_tables(tab.data(), L, cps, chunks, bytes, n_slices, order,
                           recs, (size_t)n_order);
    std::memcpy(blob, tab.data(), std::min(blob_cap, L.bytes));
  }
  const long o[8] = {SLICE_VPB,          L.n_blocks,
                     (long)L.off_ptrs,   (long)L.off_vecs,
                     (long)L.off_voff,   (long)L.off_bslice,
                     (long)L.off_brec,   (long)L.bytes};
  std::memcpy(out, o, sizeof(o));
  return ECX_OK;
}

int ecx_update_batch(ecx_ctx* ctx, void* dptr, long n_stripes,
                     size_t chunk_bytes, const void* d_new,
                     const uint64_t* write_masks, int slot) {
  if (!ctx || !dptr || !d_new || !write_masks || slot < 0 ||
      slot >= (int)ctx->slots.size() || ctx->is_bitmatrix() ||
      ctx->is_w16() || chunk_bytes == 0 || chunk_bytes % 16 ||
      n_stripes <= 0 || n_stripes > 65535)
    return ECX_ERR_INVAL;
  const int k = ctx->k, m = ctx->m, cps = k + m;
  // every mask is checked before anything is staged
  ecx::UpdatePlan plan;
  if (!ecx::plan_update(k, m, write_masks, n_stripes, plan))
    return ECX_ERR_INVAL;
  // the new chunks are read while the batch is written: no overlap
  const uintptr_t b0 = (uintptr_t)dptr, n0 = (uintptr_t)d_new;
  const uintptr_t b1 = b0 + (uintptr_t)n_stripes * cps * chunk_bytes;
  const uintptr_t n1 = n0 + (uintptr_t)plan.total_new * chunk_bytes;
  if (n0 < b1 && b0 < n1) return ECX_ERR_INVAL;
  if (plan.launches == 0) return ECX_OK;  // nothing written anywhere

  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  HIP_TRY(hipSetDevice(ctx->device));

  // blob: [encode record per pass][write_masks u64][new_base i32][active i32]
  const int n_pass = plan.launches;
  const size_t n_act = plan.active.size();
  const size_t off_mask = (size_t)n_pass * sizeof(EcMultiRec);
  const size_t off_base = off_mask + (size_t)n_stripes * 8;
  const size_t off_act = off_base + (size_t)n_stripes * 4;
  const size_t blob = off_act + n_act * 4;
  int r = open_jobs(ctx, s, blob);
  if (r != ECX_OK) return r;
  {
    EcMultiRec* recs = (EcMultiRec*)s.h_jobs;
    std::memset(recs, 0, off_mask);
    int src_ids[ECX_MAX_K], out_ids[ECX_MAX_K];
    stripe_ids(k, m, src_ids, out_ids);
    const uint8_t* rows = ctx->gen.data() + (size_t)k * k;
    for (int p = 0; p < n_pass; p++)
      fill_rec(&recs[p], src_ids, k, out_ids + p * ECX_MULTI_OUT,
               std::min(ECX_MULTI_OUT, m - p * ECX_MULTI_OUT),
               rows + (size_t)p * ECX_MULTI_OUT * k, nullptr);
  }
  std::memcpy(s.h_jobs + off_mask, write_masks, (size_t)n_stripes * 8);
  std::memcpy(s.h_jobs + off_base, plan.new_base.data(),
              (size_t)n_stripes * 4);
  std::memcpy(s.h_jobs + off_act, plan.active.data(), n_act * 4);
  r = send_jobs(s, blob);
  if (r != ECX_OK) return r;

  const EcMultiRec* d_recs = (const EcMultiRec*)s.d_jobs;
  const uint64_t* d_masks = (const uint64_t*)(s.d_jobs + off_mask);
  const int* d_base = (const int*)(s.d_jobs + off_base);
  const int* d_act = (const int*)(s.d_jobs + off_act);
  const long vecs = (long)(chunk_bytes >> 4);
  const MatmulCfg c = matmul_cfg(vecs, (long)n_act);
  // one event pair around the whole call, launches back to back
  HIP_TRY(timer_start(s));
  for (int p = 0; p < n_pass; p++) {
    const bool ok = dispatch_nout(
        std::min(ECX_MULTI_OUT, m - p * ECX_MULTI_OUT),
        [&](auto NO, auto NTF, auto LASTF) {
          hipLaunchKernelGGL(
              (ec_gf_update_kernel<NO(), NTF(), LASTF()>), c.grid, dim3(256),
              0, s.stream, (uint8_t*)dptr, (const uint8_t*)d_new, d_recs + p,
              d_masks, d_base, d_act, k, (long)chunk_bytes, cps, vecs);
        },
        c.nt, p == n_pass - 1);
    if (!ok) return ECX_ERR_INVAL;
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(timer_stop(s));
  return ECX_OK;
}

int ecx_update_plan_probe(int k, int m, const uint64_t* write_masks, long n,
                          long* new_base, int* active, int* n_active) {
  // CPU-only: the preparation ecx_update_batch performs (same plan_update).
  // Outputs are written only on success.
  if (!write_masks || !new_base || !active || !n_active || n <= 0 ||
      n > 65535 || k < 1 || m < 1 || k > ECX_MAX_K || m > ECX_MAX_K)
    return ECX_ERR_INVAL;
  ecx::UpdatePlan plan;
  if (!ecx::plan_update(k, m, write_masks, n, plan)) return ECX_ERR_INVAL;
  std::copy(plan.new_base.begin(), plan.new_base.end(), new_base);
  std::copy(plan.active.begin(), plan.active.end(), active);
  *n_active = (int)plan.active.size();
  return plan.launches;
}

int ecx_verify_batch(ecx_ctx* ctx, const void* dptr, long n_stripes,
                     size_t chunk_bytes, uint64_t present_mask,
                     uint64_t* d_bad, int slot) {
  if (!ctx || !dptr || !d_bad || slot < 0 || slot >= (int)ctx->slots.size())
    return ECX_ERR_INVAL;
  int r = verify_check_args(ctx, n_stripes, chunk_bytes);
  if (r != ECX_OK) return r;
  if ((uintptr_t)d_bad & 7) return ECX_ERR_INVAL;
  // the words are written while the batch is read: no overlap
  const uintptr_t b0 = (uintptr_t)dptr, w0 = (uintptr_t)d_bad;
  const uintptr_t b1 =
      b0 + (uintptr_t)n_stripes * (ctx->k + ctx->m) * chunk_bytes;
  const uintptr_t w1 = w0 + (uintptr_t)n_stripes * 8;
  if (w0 < b1 && b0 < w1) return ECX_ERR_INVAL;
  ecx::VerifyPlan vp;
  r = get_verify_plan(ctx, present_mask, vp);
  if (r != ECX_OK) return r;
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  return run_verify(ctx, s, (const uint8_t*)dptr, n_stripes, chunk_bytes, vp,
                    d_bad);
}

int ecx_verify_plan_probe(int technique, int k, int m, uint64_t present_mask,
                          int* survivors, int* checked, uint8_t* rows) {
  // CPU-only: the planning ecx_verify_batch performs (same plan_verify, the
  // decode plan composed directly instead of via a context's LRU). Outputs
  // are written only on success.
  if (!survivors || !checked || !rows || k < 1 || m < 1 || k + m > 64)
    return ECX_ERR_INVAL;
  if (technique != ECX_T_RS_VAN_ISA && technique != ECX_T_CAUCHY_ISA &&
      technique != ECX_T_RS_VAN_JERASURE)
    return ECX_ERR_INVAL;  // w=8 matrix techniques only, like the calls
  std::vector<uint8_t> gen;
  if (!ecx::gen_matrix(technique, gen, k, m)) return ECX_ERR_INVAL;
  auto resolve = [&](uint64_t mask, std::vector<int>& sv, std::vector<int>& er,
                     std::vector<uint8_t>& rw) {
    return ecx::compose_decode_rows(gen, k, m, mask, sv, er, rw);
  };
  ecx::VerifyPlan vp;
  const int r = verify_err(ecx::plan_verify(k, m, present_mask, resolve, vp));
  if (r != ECX_OK) return r;
  std::copy(vp.survivors.begin(), vp.survivors.end(), survivors);
  std::copy(vp.checked.begin(), vp.checked.end(), checked);
  std::copy(vp.rows.begin(), vp.rows.end(), rows);
  return (int)vp.checked.size();
}

int ecx_bitmatrix_plan_probe(const int knobs[6], int w, int pkt, int n_src,
                             int n_out, long n_ops, size_t chunk_bytes,
                             int out[16]) {
  // CPU-only: the plan run_bitmatrix launches by (same bit_plan). out is
  // written only on success; every figure of an admitted chunk fits an int.
  if (!knobs || !out || n_ops < 0 || chunk_bytes >> 35) return ECX_ERR_INVAL;
  const ecx::BitKnobs kn = {knobs[0], knobs[1], knobs[2],
                            knobs[3], knobs[4], knobs[5]};
  ecx::BitPlan p;
  int r = ecx::bit_plan(kn, w, pkt, n_src, n_out, (size_t)n_ops, chunk_bytes,
                        &p);
  if (r != ECX_OK) return r;
  const long f[16] = {p.kernel, p.nr, p.n_pos, p.q, p.vq_shift, p.vqs, p.dma,
                      p.items, p.windows_per_sw, p.n_windows, p.wpb, p.grid_x,
                      p.threads, (long)p.lds_bytes, p.xcdmap, 0};
  for (int i = 0; i < 16; i++) out[i] = (int)f[i];
  return ECX_OK;
}

int ecx_set_matrix(ecx_ctx* ctx, const uint8_t* coding_rows) {
  if (!ctx || !coding_rows || ctx->is_bitmatrix() || ctx->is_w16())
    return ECX_ERR_INVAL;
  // Take EVERY slot mutex before mutating ctx->gen: encode paths read the
  // generator under only their own slot mutex, so rewriting it under
  // lru_mu alone could expose a torn matrix to a concurrent encode on
  // another slot. Slot locks are acquired in slot order (the only place
  // more than one is held), so this cannot deadlock against per-call
  // single-slot locking.
  std::vector<std::unique_lock<std::recursive_mutex>> slot_locks;
  slot_locks.reserve(ctx->slots.size());
  for (auto& s : ctx->slots) slot_locks.emplace_back(s.mu);
  std::lock_guard<std::mutex> g(ctx->lru_mu);
  std::memcpy(ctx->gen.data() + (size_t)ctx->k * ctx->k, coding_rows,
              (size_t)ctx->m * ctx->k);
  ctx->lru.clear();
  ctx->lru_order.clear();
  for (auto& s : ctx->slots) s.pparams_kind = 0;  // resident tables stale
  return ECX_OK;
}

int ecx_gen_matrix_probe(int technique, int k, int m, uint8_t* out) {
  // CPU-only matrix readback (no GPU context): lets tests pin the core's
  // generator constructions against the oracle's on a GPU-less box.
  if (!out || k < 1 || m < 1 || k + m > 64) return ECX_ERR_INVAL;
  if (technique == ECX_T_CAUCHY_GOOD_JERASURE && m == 2)
    return ECX_ERR_INVAL;  // cbest tables unsourceable
  std::vector<uint8_t> a;
  if (!ecx::gen_matrix(technique, a, k, m)) return ECX_ERR_INVAL;
  std::memcpy(out, a.data(), a.size());
  return ECX_OK;
}

int ecx_cauchy_n_ones_probe(int e) {
  if (e < 0 || e > 255) return ECX_ERR_INVAL;
  return ecx::cauchy_n_ones((uint8_t)e);
}

int ecx_decode_rows_probe(int technique, int k, int m, uint64_t present_mask,
                          int* survivors, int* erased, uint8_t* rows) {
  // CPU-only probe of the decode-plan composition (survivor selection +
  // submatrix inversion + per-erasure coefficient rows, gf.cpp
  // compose_decode_rows — the math behind get_decode_plan's LRU).
  // Fills survivors[k], erased[<=m], rows[n_erased*k]; returns n_erased
  // or a negative errno. Lets CPU tests pin the plan math against the
  // oracle's decode composition without a GPU context.
  if (!survivors || !erased || !rows || k < 1 || m < 1 || k + m > 64)
    return ECX_ERR_INVAL;
  std::vector<uint8_t> gen;
  if (!ecx::gen_matrix(technique, gen, k, m)) return ECX_ERR_INVAL;
  std::vector<int> sv, er;
  std::vector<uint8_t> rw;
  if (!ecx::compose_decode_rows(gen, k, m, present_mask, sv, er, rw))
    return ECX_ERR_IO;
  for (int i = 0; i < k; i++) survivors[i] = sv[i];
  for (size_t i = 0; i < er.size(); i++) erased[i] = er[i];
  std::memcpy(rows, rw.data(), rw.size());
  return (int)er.size();
}

int ecx_shec_matrix(int k, int m, int c, int single, uint8_t* out) {
  if (!out) return ECX_ERR_INVAL;
  std::vector<uint8_t> coding;
  if (!ecx::shec_matrix(coding, k, m, c, single != 0)) return ECX_ERR_INVAL;
  std::memcpy(out, coding.data(), coding.size());
  return ECX_OK;
}

int ecx_gf8_tabs332_probe(uint8_t c, uint32_t out[5]) {
  if (!out) return ECX_ERR_INVAL;
  build_tabs332(ecx::gf8(), c, out);
  return ECX_OK;
}

int ecx_stream_walk_probe(uint32_t n_stripes, uint32_t tiles_per_chunk,
                          uint32_t width, int xcd, uint32_t grid,
                          uint32_t hw_block, uint32_t* stripes,
                          uint32_t* tiles, int cap) {
  if (n_stripes < 1 || n_stripes > 65535 || tiles_per_chunk < 1 ||
      tiles_per_chunk >= 0x7fffffffu || grid < 1 || grid > (1u << 23) ||
      hw_block >= grid || cap < 0 || (cap > 0 && (!stripes || !tiles)))
    return ECX_ERR_INVAL;
  const EcxWalk w = ecx_walk_make(n_stripes, tiles_per_chunk, width, xcd, grid);
  long n = 0;
  for (EcxWalkPos pos = ecx_walk_start(w, hw_block); ecx_walk_live(w, pos);
       ecx_walk_next(w, pos)) {
    const uint32_t stripe = ecx_walk_stripe(w, pos);
    if (stripe >= n_stripes) continue;  // as the kernel skips it
    if (n < cap) {
      stripes[n] = stripe;
      tiles[n] = pos.t;
    }
    if (++n > 0x7fffffffL) return ECX_ERR_INVAL;
  }
  return (int)n;
}

int ecx_matmul_batch(ecx_ctx* ctx, void* dptr, long n_stripes,
                     size_t chunk_bytes, const int* src_ids, int n_src,
                     const int* out_ids, int n_out, const uint8_t* rows,
                     int slot) {
  if (!ctx || !dptr || !src_ids || !out_ids || !rows || ctx->is_bitmatrix() ||
      ctx->is_w16())
    return ECX_ERR_INVAL;
  // chunk ids must lie within the batch stripe (k+m chunks)
  for (int i = 0; i < n_src; i++)
    if (src_ids[i] < 0 || src_ids[i] >= ctx->k + ctx->m) return ECX_ERR_INVAL;
  for (int j = 0; j < n_out; j++)
    if (out_ids[j] < 0 || out_ids[j] >= ctx->k + ctx->m) return ECX_ERR_INVAL;
  return run_matmul(ctx, slot, (const uint8_t*)dptr, (uint8_t*)dptr, src_ids,
                    n_src, out_ids, n_out, rows, nullptr, n_stripes,
                    chunk_bytes, false);
}

int ecx_sync(ecx_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= (int)ctx->slots.size()) return ECX_ERR_INVAL;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->slots[slot].stream));
  return ECX_OK;
}

int ecx_last_kernel_ms(ecx_ctx* ctx, int slot, double* ms) {
  if (!ctx || !ms || slot < 0 || slot >= (int)ctx->slots.size())
    return ECX_ERR_INVAL;
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  if (!s.timed) return ECX_ERR_INVAL;
  HIP_TRY(hipEventSynchronize(s.ev_stop));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, s.ev_start, s.ev_stop));
  *ms = (double)f;
  return ECX_OK;
}

}  // extern "C"

// ---- host-pointer (plugin) path ----
// A call is described once (HostJob) and handed to host_call, which picks
// one of three stagers: pipelined tiles (w=8 table rows), single-shot pinned
// (w16 and bitmatrix up to ECX_HPIPE_MAX), or the legacy per-chunk copies
// (ECX_HOSTPIPE=0, and w16/bitmatrix above ECX_HPIPE_MAX).

struct HostJob {
  const uint8_t* src[ECX_MAX_K];  // NULL = zeros chunk
  uint8_t* out[ECX_MAX_K];        // NULL = do not scatter (encode only)
  // chunk position in the stripe buffer and chunk id of the launch. The
  // pipelined stager packs its tiles itself: sources first, outputs behind.
  int src_slot[ECX_MAX_K], out_slot[ECX_MAX_K];
  int n_src, n_out, n_slots;
  size_t chunk_bytes;
  CodeRows rows;
  // rows.r8 are GF(2^8) coefficients for the table kernel, whatever the
  // context's technique (ecx_matmul_chunks_host)
  bool table8;
  int cache_kind;  // see pparams_kind; 1 only for the full encode
};

// Job over packed chunks, rows from the generator (encode) or the caller.
static void job_from_rows(HostJob& job, const uint8_t* const* srcs, int n_src,
                          uint8_t* const* outs, int n_out, CodeRows rows,
                          bool table8, size_t chunk_bytes, int cache_kind) {
  std::copy(srcs, srcs + n_src, job.src);
  std::copy(outs, outs + n_out, job.out);
  stripe_ids(n_src, n_out, job.src_slot, job.out_slot);
  job.n_src = n_src;
  job.n_out = n_out;
  job.n_slots = n_src + n_out;
  job.chunk_bytes = chunk_bytes;
  job.rows = rows;
  job.table8 = table8;
  job.cache_kind = cache_kind;
}

// Decode job: the plan's survivors rebuild its erased chunks, each at its
// own position in the stripe. A NULL survivor is a zeros source
// (ErasureCodeIsa.cc:212-226); an erased chunk is written, so it needs a
// buffer.
static int job_from_plan(const ecx_ctx* ctx, const DecodePlan& plan,
                         uint8_t* const* chunks, size_t chunk_bytes,
                         HostJob& job) {
  job.n_src = ctx->k;
  job.n_out = (int)plan.erased.size();
  job.n_slots = ctx->k + ctx->m;
  for (int i = 0; i < job.n_src; i++) {
    job.src_slot[i] = plan.survivors[i];
    job.src[i] = chunks[plan.survivors[i]];
  }
  for (int j = 0; j < job.n_out; j++) {
    job.out_slot[j] = plan.erased[j];
    job.out[j] = chunks[plan.erased[j]];
    if (!job.out[j]) return ECX_ERR_INVAL;
  }
  job.chunk_bytes = chunk_bytes;
  job.rows = {plan.rows.data(), plan.rows16.data()};
  job.table8 = ctx->is_table8();
  job.cache_kind = 0;
  return ECX_OK;
}

static int ensure_stage(ecx_ctx* ctx, Slot& s, size_t bytes) {
  if (s.stage_bytes >= bytes) return ECX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (s.d_stage) HIP_TRY(hipFree(s.d_stage));
  s.d_stage = nullptr;
  s.stage_bytes = 0;
  HIP_TRY(hipMalloc(&s.d_stage, bytes));
  s.stage_bytes = bytes;
  return ECX_OK;
}

// ---- pipelined host-pointer staging ---------------------------------------
// The PCIe probe (tools/pcie_probe.py, profiles/rocprof_r01_summary.md)
// measured 53 GiB/s per direction with pageable ~ pinned and no duplex
// gain — but the legacy per-chunk pageable hipMemcpyAsync path pays ~50 us
// of fixed cost PER COPY, so k+m copies per call capped the drop-in path at
// 8.5 GiB/s (k=8 m=3, 1 MiB chunks). This path instead gathers the chunks
// into a pinned double buffer with a parallel CPU memcpy (29 GiB/s per
// core measured on the box), issues ONE H2D and ONE D2H DMA per stripe
// tile, keeps the per-group launch params resident across tiles, and
// overlaps the CPU gather/scatter of tile t with the DMA+kernel of tile
// t-1. Knobs: ECX_HOSTPIPE=0 reverts to the legacy path, ECX_HPIPE_TILE
// sets per-chunk tile bytes (default 256 KiB), ECX_HPIPE_THREADS the CPU
// copy threads.

static int env_hostpipe() {
  static const int v = env_int("ECX_HOSTPIPE", 1);
  return v;
}

static size_t env_hpipe_tile() {
  // 4 MiB default: the tile sweeps (profiles/rocprof_r01_summary.md)
  // showed throughput monotonically rising with tile size at every
  // chunk size tried — per-tile event syncs (~37 us each) cost more
  // than cross-tile overlap buys, so prefer single-shot staging up to
  // 4 MiB/chunk (pinned buffer: 2 x (k+m) x tile, grown on demand)
  static const size_t v =
      std::max<size_t>(env_size("ECX_HPIPE_TILE", 4 << 20), 16 << 10) &
      ~(size_t)15;
  return v;
}

struct CopyOp {
  uint8_t* dst;
  const uint8_t* src;
  size_t n;
};

// Shared copy pool for the pinned-staging gather/scatter. Per-caller
// OpenMP teams were measured and rejected (profiles summary): with the
// default spin-wait, 8 concurrent plugin callers meant 64 spinning
// workers fighting the DMA-submit threads (8.7 GiB/s aggregate vs 39.8
// serial); with parked workers (blocktime 0) the single caller paid 8
// futex wakeups per region (11.3 vs 17 GiB/s). One process-wide pool
// avoids both: helpers stay hot while ANY caller has work (no wakeups in
// steady state, no idle spin against the HIP runtime), and callers drain
// the queue themselves, so the serial memcpy rate is the floor.
class CopyPool {
 public:
  static CopyPool& inst() {
    static CopyPool p;
    return p;
  }

  void run(const std::vector<CopyOp>& ops) {
    constexpr size_t PIECE = 1 << 20;
    size_t n_items = 0;
    for (const auto& o : ops) n_items += (o.n + PIECE - 1) / PIECE;
    std::atomic<size_t> remaining{n_items};
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (const auto& o : ops)
        for (size_t off = 0; off < o.n; off += PIECE)
          q_.push_back({o.dst + off, o.src + off,
                        std::min(PIECE, o.n - off), &remaining});
      pending_.fetch_add(n_items, std::memory_order_release);
    }
    // spinning helpers see pending_ without the lock; wake only the ones
    // that actually parked (notify_all costs the CALLER a futex syscall
    // per parked helper — measured as a single-caller regression)
    if (parked_.load(std::memory_order_acquire) > 0) cv_.notify_all();
    // help drain (possibly other callers' pieces — work conservation)
    for (;;) {
      Item it;
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (!pop(it)) break;
      }
      do_copy(it);
    }
    // our pieces may still be in helpers' hands
    while (remaining.load(std::memory_order_acquire) != 0) relax();
  }

 private:
  struct Item {
    uint8_t* dst;
    const uint8_t* src;
    size_t n;
    std::atomic<size_t>* done;
  };

  CopyPool() {
    int x = env_int("ECX_HPIPE_THREADS", 7);  // helpers; the caller is the +1
    n_workers_ = x < 0 ? 0 : (x > 63 ? 63 : x);
    for (int i = 0; i < n_workers_; i++)
      workers_.emplace_back([this] { loop(); });
  }

  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& w : workers_) w.join();
  }

  static void relax() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }

  bool pop(Item& it) {
    if (qhead_ >= q_.size()) return false;
    it = q_[qhead_++];
    pending_.fetch_sub(1, std::memory_order_relaxed);
    if (qhead_ == q_.size()) {
      q_.clear();
      qhead_ = 0;
    }
    return true;
  }

  static void do_copy(const Item& it) {
    std::memcpy(it.dst, it.src, it.n);
    it.done->fetch_sub(1, std::memory_order_acq_rel);
  }

  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      if (stop_) return;
      Item it;
      if (pop(it)) {
        lk.unlock();
        do_copy(it);
        lk.lock();
        continue;
      }
      // unlocked spin ~2 ms: single-caller stripes arrive ~1 ms apart,
      // so staying hot through the gap beats a park/wake round trip; an
      // idle context parks all helpers after the window
      lk.unlock();
      int spins = 60000;
      while (--spins > 0 && pending_.load(std::memory_order_relaxed) == 0)
        relax();
      lk.lock();
      if (pending_.load(std::memory_order_relaxed) == 0 && !stop_) {
        parked_.fetch_add(1, std::memory_order_release);
        cv_.wait_for(lk, std::chrono::milliseconds(50));
        parked_.fetch_sub(1, std::memory_order_release);
      }
    }
  }

  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Item> q_;
  size_t qhead_ = 0;
  std::atomic<size_t> pending_{0};
  std::atomic<int> parked_{0};
  bool stop_ = false;
  int n_workers_ = 0;
  std::vector<std::thread> workers_;
};

static void par_copy(const std::vector<CopyOp>& ops) {
  size_t total = 0;
  for (const auto& o : ops) total += o.n;
  if (total < (256 << 10)) {
    for (const auto& o : ops) std::memcpy(o.dst, o.src, o.n);
    return;
  }
  CopyPool::inst().run(ops);
}

static int ensure_pipe(ecx_ctx* ctx, Slot& s, size_t bytes) {
  if (s.pipe_bytes >= bytes) return ECX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(wait_event(s.ev_pipe[0]));
  HIP_TRY(wait_event(s.ev_pipe[1]));
  // captured single-tile graphs bake in the h_pipe/d_pipe addresses:
  // reallocating invalidates every one of them
  for (auto& [k, ge] : s.graphs) {
    (void)k;
    (void)hipGraphExecDestroy(ge);
  }
  s.graphs.clear();
  if (s.h_pipe) (void)hipHostFree(s.h_pipe);
  if (s.d_pipe) (void)hipFree(s.d_pipe);
  s.h_pipe = nullptr;
  s.d_pipe = nullptr;
  s.pipe_bytes = 0;
  HIP_TRY(hipHostMalloc(&s.h_pipe, bytes));
  hipError_t e = hipMalloc(&s.d_pipe, bytes);
  if (e != hipSuccess) {
    (void)hipHostFree(s.h_pipe);
    s.h_pipe = nullptr;
    return map_hip(e);
  }
  s.pipe_bytes = bytes;
  return ECX_OK;
}

static int ensure_pparams(ecx_ctx* ctx, Slot& s) {
  if (s.h_pparams) return ECX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipHostMalloc(&s.h_pparams, 8 * sizeof(EcLaunchParams)));
  hipError_t e = hipMalloc(&s.d_pparams, 8 * sizeof(EcLaunchParams));
  if (e != hipSuccess) {
    (void)hipHostFree(s.h_pparams);
    s.h_pparams = nullptr;
    return map_hip(e);
  }
  return ECX_OK;
}

static size_t env_hpipe_max() {
  static const size_t v =
      std::max<size_t>(env_size("ECX_HPIPE_MAX", (size_t)256 << 20), 1 << 20);
  return v;
}

// Single-shot pinned staging for the legacy-launcher host paths (w16 and
// bitmatrix techniques): gather chunks into the pinned pipe buffer at
// their slot offsets (NULL source => zeros chunk), ONE H2D DMA over the
// source span, run the technique's launcher on the device pipe buffer,
// per-output D2H, scatter. Same measured rationale as
// pipelined_matmul_host: per-chunk pageable copies pay ~50 us each.
// Caller holds the slot lock and bounds the size by env_hpipe_max().
static int staged_host_call(ecx_ctx* ctx, int slot_i, const HostJob& job) {
  Slot& s = ctx->slots[slot_i];
  const size_t cb = job.chunk_bytes;
  int r = ensure_pipe(ctx, s, (size_t)job.n_slots * cb);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(wait_event(s.ev_pipe[0]));
  HIP_TRY(wait_event(s.ev_pipe[1]));
  std::vector<CopyOp> ops;
  int lo = job.n_slots, hi = 0;
  for (int i = 0; i < job.n_src; i++) {
    const int sl = job.src_slot[i];
    lo = std::min(lo, sl);
    hi = std::max(hi, sl + 1);
    if (job.src[i])
      ops.push_back({s.h_pipe + (size_t)sl * cb, job.src[i], cb});
    else
      std::memset(s.h_pipe + (size_t)sl * cb, 0, cb);
  }
  par_copy(ops);
  HIP_TRY(hipMemcpyAsync(s.d_pipe + (size_t)lo * cb,
                         s.h_pipe + (size_t)lo * cb, (size_t)(hi - lo) * cb,
                         hipMemcpyHostToDevice, s.stream));
  // the launchers keep per-call param staging, so no tiling
  r = run_coded(ctx, slot_i, s.d_pipe, job.src_slot, job.n_src, job.out_slot,
                job.n_out, job.rows, nullptr, 1, cb, false);
  if (r != ECX_OK) {
    (void)hipStreamSynchronize(s.stream);  // quiesce before buffer reuse
    return r;
  }
  for (int j = 0; j < job.n_out; j++) {
    if (!job.out[j]) continue;
    HIP_TRY(hipMemcpyAsync(s.h_pipe + (size_t)job.out_slot[j] * cb,
                           s.d_pipe + (size_t)job.out_slot[j] * cb, cb,
                           hipMemcpyDeviceToHost, s.stream));
  }
  HIP_TRY(wait_stream(s.stream));
  ops.clear();
  for (int j = 0; j < job.n_out; j++)
    if (job.out[j])
      ops.push_back({job.out[j], s.h_pipe + (size_t)job.out_slot[j] * cb, cb});
  par_copy(ops);
  return ECX_OK;
}

// Generic host-pointer matmul (w=8 table techniques): srcs[i] == NULL is
// the zeros-chunk convention (skipped via cls), outs[j] == NULL skips the
// scatter of that output. Caller holds the slot lock.
static int pipelined_matmul_host(ecx_ctx* ctx, Slot& s, const HostJob& job) {
  const uint8_t* const* srcs = job.src;
  uint8_t* const* outs = job.out;
  const int n_src = job.n_src, n_out = job.n_out;
  const uint8_t* rows = job.rows.r8;
  const size_t chunk_bytes = job.chunk_bytes;
  if (n_src < 1 || n_src > ECX_MAX_K || n_out < 1 || n_out > ECX_MAX_K ||
      !chunk_bytes || chunk_bytes % 16)
    return ECX_ERR_INVAL;
  const int cps = n_src + n_out;
  const size_t TS = std::min(env_hpipe_tile(), chunk_bytes);
  int r = ensure_pipe(ctx, s, 2 * (size_t)cps * TS);
  if (r != ECX_OK) return r;
  r = ensure_pparams(ctx, s);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));

  bool src_null[ECX_MAX_K] = {};
  for (int i = 0; i < n_src; i++) src_null[i] = (srcs[i] == nullptr);
  int src_ids[ECX_MAX_K], out_ids[ECX_MAX_K];
  stripe_ids(n_src, n_out, src_ids, out_ids);

  // one tile's sources into hbuf packed at tl spacing, and its outputs back
  // out of it; off is the tile's offset in the chunks
  std::vector<CopyOp> ops;
  ops.reserve(cps);
  auto gather = [&](uint8_t* hbuf, size_t off, size_t tl) {
    ops.clear();
    for (int i = 0; i < n_src; i++)
      if (srcs[i]) ops.push_back({hbuf + (size_t)i * tl, srcs[i] + off, tl});
    par_copy(ops);
  };
  auto scatter = [&](const uint8_t* hbuf, size_t off, size_t tl) {
    ops.clear();
    for (int j = 0; j < n_out; j++)
      if (outs[j])
        ops.push_back({outs[j] + off, hbuf + ((size_t)n_src + j) * tl, tl});
    par_copy(ops);
  };

  // coefficient tables are tile-invariant: build and upload them ONCE,
  // then every tile's kernels reference the resident copies. For the hot
  // repeated case — full encode with no zeros-chunk sources, whose params
  // depend only on the fixed generator — the resident copy from the
  // previous call is reused outright (cache_kind 1, invalidated by
  // ecx_set_matrix).
  const int groups = (n_out + 3) / 4;
  if (groups > 8) return ECX_ERR_INVAL;
  bool any_null = false;
  for (int i = 0; i < n_src; i++) any_null |= src_null[i];
  const int want_kind =
      (job.cache_kind != 0 && !any_null) ? job.cache_kind : 0;
  if (want_kind == 0 || s.pparams_kind != want_kind) {
    // a previous successful call drained both pipe events, but an errored
    // one may not have: make the pinned param area provably safe to rewrite
    HIP_TRY(wait_event(s.ev_pipe[0]));
    HIP_TRY(wait_event(s.ev_pipe[1]));
    s.pparams_kind = 0;
    for (int g = 0; g < groups; g++) {
      const int j0 = 4 * g, nj = std::min(4, n_out - j0);
      fill_params(&s.h_pparams[g], src_ids, n_src, out_ids + j0, nj,
                  rows + (size_t)j0 * n_src, src_null);
    }
    HIP_TRY(hipMemcpyAsync(s.d_pparams, s.h_pparams,
                           (size_t)groups * sizeof(EcLaunchParams),
                           hipMemcpyHostToDevice, s.stream));
    // cover the in-flight upload so the next call's safety syncs see it
    // even if this call errors out before the first tile's record
    HIP_TRY(hipEventRecord(s.ev_pipe[0], s.stream));
    s.pparams_kind = want_kind;
  }

  const long T = (long)((chunk_bytes + TS - 1) / TS);

  // Single-tile small-call fast path: capture the (H2D, kernels, D2H)
  // chain once per (tl, n_src, n_out) into a hipGraph and replay it —
  // one submit (~10-16 us replay floor) instead of 3-5 driver calls.
  // Addresses are stable (pinned h_pipe / d_pipe / resident d_pparams),
  // and the captured work is content-independent, so the graph stays
  // valid across calls and across param-table rewrites. ECX_HGRAPH=0
  // disables. (DESIGN: the OSD call shape is many small calls.)
  static const int env_hg = env_int("ECX_HGRAPH", 1);
  // Graph replay wins where per-call submit overhead dominates and loses
  // where hipGraphLaunch's runtime serialisation bites (measured, one
  // box: 64 KiB x1 +25%, 64 KiB x8 callers -12%, 256 KiB x1 -9%,
  // 1 MiB x8 -21%). Default: small calls only.
  static const size_t env_hg_max = env_size("ECX_HGRAPH_MAX", 128 << 10);
  if (T == 1 && env_hg && chunk_bytes <= env_hg_max) {
    const size_t tl = chunk_bytes;
    uint8_t* hbuf = s.h_pipe;
    uint8_t* dbuf = s.d_pipe;
    HIP_TRY(wait_event(s.ev_pipe[0]));
    HIP_TRY(wait_event(s.ev_pipe[1]));
    gather(hbuf, 0, tl);
    const uint64_t key =
        (uint64_t)tl | ((uint64_t)n_src << 44) | ((uint64_t)n_out << 52);
    auto it = s.graphs.find(key);
    if (it == s.graphs.end()) {
      HIP_TRY(
          hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal));
      int rc = ECX_OK;
      hipError_t he = hipMemcpyAsync(dbuf, hbuf, (size_t)n_src * tl,
                                     hipMemcpyHostToDevice, s.stream);
      if (he != hipSuccess) rc = map_hip(he);
      const MatmulCfg c = matmul_cfg((long)(tl >> 4), 1);
      for (int g = 0; g < groups && rc == ECX_OK; g++) {
        const int nj = std::min(4, n_out - 4 * g);
        rc = matmul_dispatch(s.stream, dbuf, dbuf, s.d_pparams + g, nj, false,
                             c, tl, cps);
      }
      if (rc == ECX_OK) {
        he = hipMemcpyAsync(hbuf + (size_t)n_src * tl,
                            dbuf + (size_t)n_src * tl, (size_t)n_out * tl,
                            hipMemcpyDeviceToHost, s.stream);
        if (he != hipSuccess) rc = map_hip(he);
      }
      hipGraph_t g = nullptr;
      he = hipStreamEndCapture(s.stream, &g);
      if (he != hipSuccess) return map_hip(he);
      if (rc != ECX_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      hipGraphExec_t ge = nullptr;
      he = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (he != hipSuccess) return map_hip(he);
      it = s.graphs.emplace(key, ge).first;
    }
    HIP_TRY(hipGraphLaunch(it->second, s.stream));
    HIP_TRY(hipEventRecord(s.ev_pipe[0], s.stream));
    HIP_TRY(wait_event(s.ev_pipe[0]));
    scatter(hbuf, 0, tl);
    return ECX_OK;
  }

  size_t tl_of[2] = {0, 0}, off_of[2] = {0, 0};
  for (long t = 0; t < T; t++) {
    const int b = (int)(t & 1);
    const size_t off = (size_t)t * TS;
    const size_t tl = std::min(TS, chunk_bytes - off);
    uint8_t* hbuf = s.h_pipe + (size_t)b * cps * TS;
    uint8_t* dbuf = s.d_pipe + (size_t)b * cps * TS;
    // buffer b holds tile t-2 until its D2H lands; wait, scatter it out,
    // then refill — the CPU work here overlaps tile t-1's DMA + kernels
    HIP_TRY(wait_event(s.ev_pipe[b]));
    if (t >= 2) scatter(hbuf, off_of[b], tl_of[b]);
    // gather tile t's sources packed at tl spacing (gaps where srcs[i] is
    // NULL are never read: cls==0 skips those sources in the kernel), then
    // ONE H2D DMA. Per-source interleaved copy+DMA was measured SLOWER
    // (15.3 vs 19.0 GiB/s at 1 MiB chunks): the extra DMA submissions and
    // OpenMP fork/joins cost more than the overlap hides.
    gather(hbuf, off, tl);
    HIP_TRY(hipMemcpyAsync(dbuf, hbuf, (size_t)n_src * tl,
                           hipMemcpyHostToDevice, s.stream));
    const MatmulCfg c = matmul_cfg((long)(tl >> 4), 1);
    for (int g = 0; g < groups; g++) {
      const int nj = std::min(4, n_out - 4 * g);
      int rr = matmul_dispatch(s.stream, dbuf, dbuf, s.d_pparams + g, nj,
                               false, c, tl, cps);
      if (rr != ECX_OK) {
        (void)hipStreamSynchronize(s.stream);  // quiesce in-flight tiles
        return rr;
      }
    }
    HIP_TRY(hipMemcpyAsync(hbuf + (size_t)n_src * tl,
                           dbuf + (size_t)n_src * tl, (size_t)n_out * tl,
                           hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.ev_pipe[b], s.stream));
    tl_of[b] = tl;
    off_of[b] = off;
  }
  // drain the last one or two in-flight tiles
  for (long t = std::max(0L, T - 2); t < T; t++) {
    const int b = (int)(t & 1);
    HIP_TRY(wait_event(s.ev_pipe[b]));
    scatter(s.h_pipe + (size_t)b * cps * TS, off_of[b], tl_of[b]);
  }
  return ECX_OK;
}

// Legacy per-chunk staging, every technique: one pageable hipMemcpyAsync per
// source into the slot's stage buffer, the launches, one copy per output,
// then wait. A zeros-chunk source is skipped by class mask for the w=8 table
// kernel and materialised in the stage buffer for w16 and bitmatrix, which
// read every source. Caller holds the slot lock.
static int legacy_host_call(ecx_ctx* ctx, int slot_i, const HostJob& job) {
  Slot& s = ctx->slots[slot_i];
  const size_t cb = job.chunk_bytes;
  int r = ensure_stage(ctx, s, (size_t)job.n_slots * cb);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  bool src_null[ECX_MAX_K] = {};
  for (int i = 0; i < job.n_src; i++) {
    uint8_t* d = s.d_stage + (size_t)job.src_slot[i] * cb;
    if (job.src[i])
      HIP_TRY(hipMemcpyAsync(d, job.src[i], cb, hipMemcpyHostToDevice,
                             s.stream));
    else if (job.table8)
      src_null[i] = true;  // zeros chunk (ErasureCodeJerasure.cc:146-157)
    else
      HIP_TRY(hipMemsetAsync(d, 0, cb, s.stream));
  }
  if (job.table8) {
    // the table kernel, as this path always launched (run_matmul may pick
    // the stream kernel)
    for (int j0 = 0; j0 < job.n_out && r == ECX_OK; j0 += 4) {
      EcLaunchParams p;
      fill_params(&p, job.src_slot, job.n_src, job.out_slot + j0,
                  std::min(4, job.n_out - j0),
                  job.rows.r8 + (size_t)j0 * job.n_src, src_null);
      r = launch_matmul(ctx, s, s.d_stage, s.d_stage, p, 1, cb, false, false);
    }
  } else {
    r = run_coded(ctx, slot_i, s.d_stage, job.src_slot, job.n_src,
                  job.out_slot, job.n_out, job.rows, nullptr, 1, cb, false);
  }
  if (r != ECX_OK) {
    (void)hipStreamSynchronize(s.stream);  // quiesce before buffer reuse
    return r;
  }
  for (int j = 0; j < job.n_out; j++) {
    if (!job.out[j]) continue;
    HIP_TRY(hipMemcpyAsync(job.out[j],
                           s.d_stage + (size_t)job.out_slot[j] * cb, cb,
                           hipMemcpyDeviceToHost, s.stream));
  }
  HIP_TRY(wait_stream(s.stream));
  return ECX_OK;
}

// Run a host job on slot slot_i (lock held by the caller) through the stager
// for its rows and size. Arguments the launchers would refuse only after
// copies were enqueued are refused here.
static int host_call(ecx_ctx* ctx, int slot_i, const HostJob& job) {
  if (!job.table8 && ctx->is_bitmatrix() &&
      (job.chunk_bytes == 0 ||
       job.chunk_bytes % ((size_t)ctx->w * ctx->pkt)))
    return ECX_ERR_INVAL;
  if (!env_hostpipe()) return legacy_host_call(ctx, slot_i, job);
  if (job.table8) return pipelined_matmul_host(ctx, ctx->slots[slot_i], job);
  if ((size_t)job.n_slots * job.chunk_bytes <= env_hpipe_max())
    return staged_host_call(ctx, slot_i, job);
  return legacy_host_call(ctx, slot_i, job);
}

extern "C" {

int ecx_encode_chunks_host(ecx_ctx* ctx, const uint8_t* const* data,
                           uint8_t* const* parity, size_t chunk_bytes) {
  if (!ctx || !data || !parity || chunk_bytes % 16) return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  std::lock_guard<std::recursive_mutex> g(ctx->slots[si].mu);
  HostJob job;
  job_from_rows(job, data, ctx->k, parity, ctx->m, ctx->gen_rows(),
                ctx->is_table8(), chunk_bytes, /*cache_kind=*/1);
  return host_call(ctx, si, job);
}

int ecx_decode_chunks_host(ecx_ctx* ctx, uint8_t* const* chunks,
                           uint64_t present_mask, size_t chunk_bytes) {
  if (!ctx || !chunks || chunk_bytes % 16) return ECX_ERR_INVAL;
  DecodePlan plan;
  int r = get_decode_plan(ctx, present_mask, plan);
  if (r != ECX_OK) return r;
  if (plan.erased.empty()) return ECX_OK;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  std::lock_guard<std::recursive_mutex> g(ctx->slots[si].mu);
  HostJob job;
  r = job_from_plan(ctx, plan, chunks, chunk_bytes, job);
  if (r != ECX_OK) return r;
  return host_call(ctx, si, job);
}

int ecx_verify_chunks_host(ecx_ctx* ctx, const uint8_t* const* chunks,
                           uint64_t present_mask, size_t chunk_bytes,
                           uint64_t* bad) {
  if (!ctx || !chunks || !bad) return ECX_ERR_INVAL;
  int r = verify_check_args(ctx, 1, chunk_bytes);
  if (r != ECX_OK) return r;
  ecx::VerifyPlan vp;
  r = get_verify_plan(ctx, present_mask, vp);
  if (r != ECX_OK) return r;
  // unlike decode, a present chunk that is not given cannot be vouched for
  const int cps = ctx->k + ctx->m;
  for (int i = 0; i < cps; i++)
    if ((present_mask >> i & 1) && !chunks[i]) return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  Slot& s = ctx->slots[si];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  // one stripe in the staging buffer, its word behind it (8-byte aligned:
  // chunk_bytes is a multiple of 16); absent positions stay unwritten and
  // are never read
  const size_t cb = chunk_bytes, word_off = (size_t)cps * cb;
  r = ensure_stage(ctx, s, word_off + 8);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  for (int i = 0; i < cps; i++)
    if (present_mask >> i & 1)
      HIP_TRY(hipMemcpyAsync(s.d_stage + (size_t)i * cb, chunks[i], cb,
                             hipMemcpyHostToDevice, s.stream));
  uint64_t* d_word = (uint64_t*)(s.d_stage + word_off);
  r = run_verify(ctx, s, s.d_stage, 1, cb, vp, d_word);
  if (r != ECX_OK) {
    (void)hipStreamSynchronize(s.stream);  // quiesce before buffer reuse
    return r;
  }
  uint64_t word = 0;
  HIP_TRY(hipMemcpyAsync(&word, d_word, 8, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));
  *bad = word;
  return ECX_OK;
}

int ecx_matmul_chunks_host(ecx_ctx* ctx, const uint8_t* const* srcs,
                           int n_src, uint8_t* const* outs, int n_out,
                           const uint8_t* rows, size_t bytes) {
  if (!ctx || !srcs || !outs || !rows || n_src < 1 || n_src > ECX_MAX_K ||
      n_out < 1 || n_out > ECX_MAX_K || bytes % 16)
    return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  std::lock_guard<std::recursive_mutex> g(ctx->slots[si].mu);
  HostJob job;
  job_from_rows(job, srcs, n_src, outs, n_out, {rows, nullptr},
                /*table8=*/true, bytes, /*cache_kind=*/0);
  return host_call(ctx, si, job);
}

int ecx_encode_delta_host(ecx_ctx* ctx, const uint8_t* old_data,
                          const uint8_t* new_data, uint8_t* delta,
                          size_t bytes) {
  if (!ctx || !old_data || !new_data || !delta || bytes % 16)
    return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  Slot& s = ctx->slots[si];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  int r = ensure_stage(ctx, s, 3 * bytes);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(s.d_stage, old_data, bytes, hipMemcpyHostToDevice,
                         s.stream));
  HIP_TRY(hipMemcpyAsync(s.d_stage + bytes, new_data, bytes,
                         hipMemcpyHostToDevice, s.stream));
  r = ecx_encode_delta_dev(ctx, s.d_stage, s.d_stage + bytes,
                           s.d_stage + 2 * bytes, bytes, si);
  if (r != ECX_OK) return r;
  HIP_TRY(hipMemcpyAsync(delta, s.d_stage + 2 * bytes, bytes,
                         hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));
  return ECX_OK;
}

int ecx_apply_delta_host(ecx_ctx* ctx, const uint8_t* delta, int data_shard,
                         int coding_shard, uint8_t* parity, size_t bytes) {
  if (!ctx || !delta || !parity || bytes % 16) return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  Slot& s = ctx->slots[si];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  int r = ensure_stage(ctx, s, 2 * bytes);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(s.d_stage, delta, bytes, hipMemcpyHostToDevice,
                         s.stream));
  HIP_TRY(hipMemcpyAsync(s.d_stage + bytes, parity, bytes,
                         hipMemcpyHostToDevice, s.stream));
  r = ecx_apply_delta_dev(ctx, s.d_stage, data_shard, coding_shard,
                          s.d_stage + bytes, bytes, si);
  if (r != ECX_OK) return r;
  HIP_TRY(hipMemcpyAsync(parity, s.d_stage + bytes, bytes,
                         hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));
  return ECX_OK;
}

int ecx_apply_deltas_host(ecx_ctx* ctx, const uint8_t* const* deltas,
                          const int* data_shards, int n_in,
                          uint8_t* const* parities, const int* coding_shards,
                          int n_out, size_t bytes) {
  // every (delta, parity) pair of one apply_delta call in one staged round
  // trip: parities[j] ^= XOR_i gen[coding_shards[j]][data_shards[i]] *
  // deltas[i] (the whole loop of ErasureCodeIsa.cc:333-366 /
  // ErasureCodeJerasure.cc:285-331), each buffer over PCIe once
  if (!ctx || !deltas || !data_shards || !parities || !coding_shards ||
      n_in < 1 || n_in > ctx->k || n_out < 1 || n_out > ctx->m || bytes % 16)
    return ECX_ERR_INVAL;
  const int k = ctx->k;
  for (int i = 0; i < n_in; i++)
    if (!deltas[i] || data_shards[i] < 0 || data_shards[i] >= k)
      return ECX_ERR_INVAL;
  for (int j = 0; j < n_out; j++)
    if (!parities[j] || coding_shards[j] < k || coding_shards[j] >= k + ctx->m)
      return ECX_ERR_INVAL;
  // refused by the bitmatrix launcher, but only after the uploads
  if (ctx->is_bitmatrix() && bytes % ((size_t)ctx->w * ctx->pkt))
    return ECX_ERR_INVAL;
  if (bytes == 0) return ECX_OK;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  Slot& s = ctx->slots[si];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  int r = ensure_stage(ctx, s, (size_t)(n_in + n_out) * bytes);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  // one "stripe" in the stage buffer: the deltas, the parities behind them
  int src_ids[ECX_MAX_K], out_ids[ECX_MAX_K];
  stripe_ids(n_in, n_out, src_ids, out_ids);
  for (int i = 0; i < n_in; i++)
    HIP_TRY(hipMemcpyAsync(s.d_stage + (size_t)i * bytes, deltas[i], bytes,
                           hipMemcpyHostToDevice, s.stream));
  for (int j = 0; j < n_out; j++)
    HIP_TRY(hipMemcpyAsync(s.d_stage + (size_t)out_ids[j] * bytes,
                           parities[j], bytes, hipMemcpyHostToDevice,
                           s.stream));
  if (ctx->is_bitmatrix()) {
    // the schedule-delta kernel takes one w x w block: per-pair launches,
    // all inside this one staged call
    for (int i = 0; i < n_in && r == ECX_OK; i++)
      for (int j = 0; j < n_out && r == ECX_OK; j++)
        r = ecx_apply_delta_dev(ctx, s.d_stage + (size_t)i * bytes,
                                data_shards[i], coding_shards[j],
                                s.d_stage + (size_t)out_ids[j] * bytes, bytes,
                                si);
  } else if (ctx->is_w16()) {
    std::vector<uint16_t> cf((size_t)n_out * n_in);
    for (int j = 0; j < n_out; j++)
      for (int i = 0; i < n_in; i++)
        cf[(size_t)j * n_in + i] =
            ctx->gen16[(size_t)coding_shards[j] * k + data_shards[i]];
    r = run_matmul16(ctx, si, s.d_stage, s.d_stage, src_ids, n_in, out_ids,
                     n_out, cf.data(), 1, bytes, /*accum=*/true, false);
  } else {
    std::vector<uint8_t> cf((size_t)n_out * n_in);
    for (int j = 0; j < n_out; j++)
      for (int i = 0; i < n_in; i++)
        cf[(size_t)j * n_in + i] =
            ctx->gen[(size_t)coding_shards[j] * k + data_shards[i]];
    r = run_matmul(ctx, si, s.d_stage, s.d_stage, src_ids, n_in, out_ids,
                   n_out, cf.data(), nullptr, 1, bytes, /*accum=*/true);
  }
  if (r != ECX_OK) {
    (void)hipStreamSynchronize(s.stream);  // quiesce before buffer reuse
    return r;
  }
  for (int j = 0; j < n_out; j++)
    HIP_TRY(hipMemcpyAsync(parities[j], s.d_stage + (size_t)out_ids[j] * bytes,
                           bytes, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));
  return ECX_OK;
}

}  // extern "C"

// ---- per-shard CRC-32C: host side ----
// Kept at the end of the file, and every CRC kernel a template: kernels are
// emitted where they are first used, so the code of every other kernel
// stays at the offset it had before these existed.
// Seed pass, hash pass and (chain mode) the scan, back to back under one
// event pair. Arguments are validated and the slot is locked by the caller.
static int run_crc(ecx_ctx* ctx, Slot& s, const uint8_t* d_buf,
                   long n_stripes, const EcCrcArgs& a, const ecx::CrcPlan& p,
                   const uint32_t* d_seed, int chain, uint32_t* d_crc) {
  const uint32_t n_words = (uint32_t)n_stripes * a.n_ids;
  ecx::CrcChainPlan cp;
  if (chain) ecx::plan_crc_chain(a.chunk_bytes, n_stripes, cp);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(timer_start(s));
  hipLaunchKernelGGL(ec_crc32c_seed_kernel<>, dim3((n_words + 255) / 256),
                     dim3(256), 0, s.stream, d_seed, d_crc, a, n_words, chain);
  HIP_TRY(hipGetLastError());
  if (env_nt())
    hipLaunchKernelGGL(ec_crc32c_kernel<true>, dim3((unsigned)p.grid),
                       dim3(ecx::CRC_THREADS), 0, s.stream, d_buf, d_crc, a);
  else
    hipLaunchKernelGGL(ec_crc32c_kernel<false>, dim3((unsigned)p.grid),
                       dim3(ecx::CRC_THREADS), 0, s.stream, d_buf, d_crc, a);
  HIP_TRY(hipGetLastError());
  if (chain) {
    hipLaunchKernelGGL(ec_crc32c_chain_kernel<>, dim3(a.n_ids),
                       dim3(ECX_CRC_CHAIN_T), 0, s.stream, d_seed, d_crc, a,
                       cp, (uint32_t)n_stripes);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(timer_stop(s));
  return ECX_OK;
}

extern "C" {

int ecx_crc32c_batch(ecx_ctx* ctx, const void* dptr, long n_stripes,
                     size_t chunk_bytes, uint64_t chunk_mask,
                     const uint32_t* d_seed, int chain, uint32_t* d_crc,
                     int slot) {
  if (!ctx || !dptr || !d_crc || slot < 0 || slot >= (int)ctx->slots.size())
    return ECX_ERR_INVAL;
  const int n = ctx->k + ctx->m;
  if (n < 64 && (chunk_mask >> n)) return ECX_ERR_INVAL;
  EcCrcArgs a = {};
  for (int c = 0; c < n; c++)
    if (chunk_mask >> c & 1) a.ids[a.n_ids++] = (uint32_t)c;
  // sizes are judged as for a full mask, so a refusal does not depend on it
  ecx::CrcPlan p;
  if (!ecx::plan_crc(chunk_bytes, n_stripes, n, p)) return ECX_ERR_INVAL;
  if (((uintptr_t)d_crc | (uintptr_t)d_seed) & 3) return ECX_ERR_INVAL;
  // the words are written while the batch is read, and seeds are read while
  // words are written: no overlap, but for the in-place append
  const uintptr_t b0 = (uintptr_t)dptr, w0 = (uintptr_t)d_crc,
                  s0 = (uintptr_t)d_seed;
  const uintptr_t b1 = b0 + (uintptr_t)n_stripes * n * chunk_bytes;
  const uintptr_t w1 = w0 + (uintptr_t)n_stripes * n * 4;
  const uintptr_t s1 = s0 + (uintptr_t)(chain ? 1 : n_stripes) * n * 4;
  if (w0 < b1 && b0 < w1) return ECX_ERR_INVAL;
  if (d_seed) {
    if (s0 < b1 && b0 < s1) return ECX_ERR_INVAL;
    if (s0 < w1 && w0 < s1 && !(s0 == w0 && !chain)) return ECX_ERR_INVAL;
  }
  if (a.n_ids == 0) return ECX_OK;  // nothing to hash, nothing launched
  ecx::plan_crc(chunk_bytes, n_stripes, (int)a.n_ids, p);
  a.n_chunks = (uint32_t)n;
  a.bpc = (uint32_t)p.blocks_per_chunk;
  a.chunk_bytes = chunk_bytes;
  a.x_chunk = ecx::crc_xpow8(chunk_bytes);
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  return run_crc(ctx, s, (const uint8_t*)dptr, n_stripes, a, p, d_seed, chain,
                 d_crc);
}

int ecx_crc32c_probe(uint32_t seed, const void* data, size_t len,
                     uint32_t* out) {
  if (!out || (!data && len)) return ECX_ERR_INVAL;
  int path = 0;
  *out = ecx::crc32c_host(seed, data, len, &path);
  return path;
}

int ecx_crc32c_shift_probe(uint32_t crc, uint64_t nbytes, uint32_t* out) {
  if (!out) return ECX_ERR_INVAL;
  *out = ecx::crc32c_shift(crc, nbytes);
  return ECX_OK;
}

int ecx_crc32c_plan_probe(size_t chunk_bytes, long n_stripes, int n_chunks,
                          long out[8]) {
  ecx::CrcPlan p;
  if (!out || !ecx::plan_crc(chunk_bytes, n_stripes, n_chunks, p))
    return ECX_ERR_INVAL;
  const long v[8] = {p.seg_bytes, p.segs_per_block, p.blocks_per_chunk,
                     p.grid,      p.threads,        p.lds_bytes,
                     p.launches,  0};
  std::copy(v, v + 8, out);
  return ECX_OK;
}

}  // extern "C"

// ---- locating the corrupt chunk: host side ----
// At the end of the file for the reason given above run_crc.

template <int NO>
static hipError_t locate_occupancy(int* n) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      n, ec_gf_locate_kernel<NO>, 256, 0);
}

// One launch of ec_gf_locate_kernel: a pass of <= 4 checked chunks of one
// candidate.
struct LocateLaunch {
  StreamLaunch L;  // argument block and sizes; its grid and walk are unused
  uint32_t grid, tpc, step_e, step_t, cand;
  int n_out;
};

// Locate plan of a mask (locate_plan.h), its decode plans through the LRU.
static int get_locate_plan(ecx_ctx* ctx, uint64_t present_mask,
                           ecx::LocatePlan& lp) {
  auto resolve = [&](uint64_t mask, std::vector<int>& sv, std::vector<int>& er,
                     std::vector<uint8_t>& rw) {
    DecodePlan dp;
    if (get_decode_plan(ctx, mask, dp) != ECX_OK) return false;
    sv = std::move(dp.survivors);
    er = std::move(dp.erased);
    rw = std::move(dp.rows);
    return true;
  };
  return verify_err(
      ecx::plan_locate(ctx->k, ctx->m, present_mask, resolve, lp));
}

// Argument block and grid of one candidate pass. The host does not know how
// many stripes are flagged, so the grid is what stays resident (CUs x blocks
// per CU of this instance), capped by the tiles of the whole batch.
static int locate_prepare(ecx_ctx* ctx, const ecx::VerifyPlan& cp, int j0,
                          uint32_t cand, long n_stripes, size_t chunk_bytes,
                          LocateLaunch& q) {
  const int k = ctx->k, n = (int)cp.checked.size();
  q.n_out = std::min(ECX_STREAM_MAX_OUT, n - j0);
  q.cand = cand;
  int r = stream_prepare(ctx, true, cp.survivors.data(), k,
                         cp.checked.data() + j0, q.n_out,
                         cp.rows.data() + (size_t)j0 * k, nullptr, n_stripes,
                         chunk_bytes, q.L);
  if (r != ECX_OK) return r;
  int bpc = ctx->locate_occ[q.n_out].load();
  if (bpc <= 0) {
    hipError_t e = q.n_out == 1   ? locate_occupancy<1>(&bpc)
                   : q.n_out == 2 ? locate_occupancy<2>(&bpc)
                   : q.n_out == 3 ? locate_occupancy<3>(&bpc)
                                  : locate_occupancy<4>(&bpc);
    HIP_TRY(e);
    bpc = std::max(1, bpc);
    ctx->locate_occ[q.n_out].store(bpc);
  }
  const uint64_t tpc = (q.L.vecs + 255) / 256;  // < 2^31 (verify_check_args)
  const uint64_t g = std::min<uint64_t>(
      {tpc * (uint64_t)n_stripes,
       (uint64_t)ctx->stream_cus.load() * (uint64_t)bpc, 1ull << 23});
  q.grid = (uint32_t)std::max<uint64_t>(1, g);
  q.tpc = (uint32_t)tpc;
  q.step_e = q.grid / q.tpc;
  q.step_t = q.grid % q.tpc;
  return ECX_OK;
}

static int ensure_loc(ecx_ctx* ctx, Slot& s, size_t words) {
  if (s.loc_words >= words) return ECX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (s.d_loc) {
    // earlier calls on this slot may still read the old list
    HIP_TRY(hipStreamSynchronize(s.stream));
    HIP_TRY(hipFree(s.d_loc));
  }
  s.d_loc = nullptr;
  s.loc_words = 0;
  HIP_TRY(hipMalloc(&s.d_loc, words * 4));
  s.loc_words = words;
  return ECX_OK;
}

// Both word arrays cleared, the verify passes into d_bad, the list of flagged
// stripes, every candidate over that list, the finish rule; all on the slot's
// stream with no host synchronisation. Arguments are validated and the slot
// is locked by the caller; every pass is prepared before anything is
// enqueued.
static int run_locate(ecx_ctx* ctx, Slot& s, const uint8_t* d_buf,
                      long n_stripes, size_t chunk_bytes,
                      uint64_t present_mask, const ecx::LocatePlan& lp,
                      uint64_t* d_bad, uint64_t* d_culprit) {
  const int k = ctx->k;
  std::vector<LocateLaunch> passes;
  for (int i = 0; i < k; i++) {
    const ecx::VerifyPlan& cp = lp.cand[i];
    for (int j0 = 0; j0 < (int)cp.checked.size(); j0 += ECX_STREAM_MAX_OUT) {
      passes.emplace_back();
      int r = locate_prepare(ctx, cp, j0, (uint32_t)lp.base.survivors[i],
                             n_stripes, chunk_bytes, passes.back());
      if (r != ECX_OK) return r;
    }
  }
  uint64_t survivor_mask = 0;
  for (int sv : lp.base.survivors) survivor_mask |= 1ull << sv;
  int r = ensure_loc(ctx, s, (size_t)n_stripes + 1);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(d_culprit, 0, (size_t)n_stripes * 8, s.stream));
  // clears d_bad and records the start event ahead of its first launch
  r = run_verify(ctx, s, d_buf, n_stripes, chunk_bytes, lp.base, d_bad);
  if (r != ECX_OK) return r;
  auto* bad = (unsigned long long*)d_bad;
  auto* cul = (unsigned long long*)d_culprit;
  hipLaunchKernelGGL(ec_locate_list_kernel<>, dim3(1),
                     dim3(ECX_LOCATE_LIST_T), 0, s.stream, bad, s.d_loc,
                     (uint32_t)n_stripes);
  HIP_TRY(hipGetLastError());
  for (const LocateLaunch& q : passes) {
    dispatch_nout(q.n_out, [&](auto NO) {
      hipLaunchKernelGGL((ec_gf_locate_kernel<NO()>), dim3(q.grid), dim3(256),
                         0, s.stream, d_buf, cul, s.d_loc, q.L.p,
                         q.L.stripe_bytes, q.L.vecs, q.tpc, q.step_e, q.step_t,
                         q.cand);
    });
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ec_locate_finish_kernel<>,
                     dim3(((uint32_t)n_stripes + 255) / 256), dim3(256), 0,
                     s.stream, bad, cul, present_mask, survivor_mask,
                     (uint32_t)n_stripes);
  HIP_TRY(hipGetLastError());
  HIP_TRY(timer_stop(s));  // moves the stop event behind the last launch
  return ECX_OK;
}

// Refusals of ecx_locate_batch that concern the two word arrays.
static int locate_check_arrays(const ecx_ctx* ctx, const void* dptr,
                               long n_stripes, size_t chunk_bytes,
                               const uint64_t* d_bad,
                               const uint64_t* d_culprit) {
  if (!d_bad || !d_culprit) return ECX_ERR_INVAL;
  if (((uintptr_t)d_bad | (uintptr_t)d_culprit) & 7) return ECX_ERR_INVAL;
  const uintptr_t b0 = (uintptr_t)dptr;
  const uintptr_t b1 =
      b0 + (uintptr_t)n_stripes * (ctx->k + ctx->m) * chunk_bytes;
  const uintptr_t w0 = (uintptr_t)d_bad, c0 = (uintptr_t)d_culprit;
  const uintptr_t wn = (uintptr_t)n_stripes * 8;
  if (w0 < b1 && b0 < w0 + wn) return ECX_ERR_INVAL;
  if (c0 < b1 && b0 < c0 + wn) return ECX_ERR_INVAL;
  if (w0 < c0 + wn && c0 < w0 + wn) return ECX_ERR_INVAL;
  return ECX_OK;
}

extern "C" {

int ecx_locate_batch(ecx_ctx* ctx, const void* dptr, long n_stripes,
                     size_t chunk_bytes, uint64_t present_mask,
                     uint64_t* d_bad, uint64_t* d_culprit, int slot) {
  if (!ctx || !dptr || slot < 0 || slot >= (int)ctx->slots.size())
    return ECX_ERR_INVAL;
  int r = verify_check_args(ctx, n_stripes, chunk_bytes);
  if (r != ECX_OK) return r;
  r = locate_check_arrays(ctx, dptr, n_stripes, chunk_bytes, d_bad, d_culprit);
  if (r != ECX_OK) return r;
  ecx::LocatePlan lp;
  r = get_locate_plan(ctx, present_mask, lp);
  if (r != ECX_OK) return r;
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  return run_locate(ctx, s, (const uint8_t*)dptr, n_stripes, chunk_bytes,
                    present_mask, lp, d_bad, d_culprit);
}

int ecx_locate_chunks_host(ecx_ctx* ctx, const uint8_t* const* chunks,
                           uint64_t present_mask, size_t chunk_bytes,
                           uint64_t* bad, uint64_t* culprit) {
  if (!ctx || !chunks || !bad || !culprit) return ECX_ERR_INVAL;
  int r = verify_check_args(ctx, 1, chunk_bytes);
  if (r != ECX_OK) return r;
  ecx::LocatePlan lp;
  r = get_locate_plan(ctx, present_mask, lp);
  if (r != ECX_OK) return r;
  const int cps = ctx->k + ctx->m;
  for (int i = 0; i < cps; i++)
    if ((present_mask >> i & 1) && !chunks[i]) return ECX_ERR_INVAL;
  const int si = (int)(ctx->rr++ % ctx->slots.size());
  Slot& s = ctx->slots[si];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  // one stripe in the staging buffer, its two words behind it
  const size_t cb = chunk_bytes, word_off = (size_t)cps * cb;
  r = ensure_stage(ctx, s, word_off + 16);
  if (r != ECX_OK) return r;
  HIP_TRY(hipSetDevice(ctx->device));
  for (int i = 0; i < cps; i++)
    if (present_mask >> i & 1)
      HIP_TRY(hipMemcpyAsync(s.d_stage + (size_t)i * cb, chunks[i], cb,
                             hipMemcpyHostToDevice, s.stream));
  uint64_t* d_words = (uint64_t*)(s.d_stage + word_off);
  r = run_locate(ctx, s, s.d_stage, 1, cb, present_mask, lp, d_words,
                 d_words + 1);
  if (r != ECX_OK) {
    (void)hipStreamSynchronize(s.stream);  // quiesce before buffer reuse
    return r;
  }
  uint64_t words[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(words, d_words, 16, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));
  *bad = words[0];
  *culprit = words[1];
  return ECX_OK;
}

int ecx_locate_plan_probe(int technique, int k, int m, uint64_t present_mask,
                          int* survivors, int* checked, int* cand_survivors,
                          int* cand_checked, uint8_t* cand_rows) {
  // CPU-only: the planning ecx_locate_batch performs (same plan_locate, the
  // decode plans composed directly instead of via a context's LRU). Outputs
  // are written only on success.
  if (!survivors || !checked || !cand_survivors || !cand_checked ||
      !cand_rows || k < 1 || m < 1 || k + m > 64)
    return ECX_ERR_INVAL;
  if (technique != ECX_T_RS_VAN_ISA && technique != ECX_T_CAUCHY_ISA &&
      technique != ECX_T_RS_VAN_JERASURE)
    return ECX_ERR_INVAL;  // w=8 matrix techniques only, like the calls
  std::vector<uint8_t> gen;
  if (!ecx::gen_matrix(technique, gen, k, m)) return ECX_ERR_INVAL;
  auto resolve = [&](uint64_t mask, std::vector<int>& sv, std::vector<int>& er,
                     std::vector<uint8_t>& rw) {
    return ecx::compose_decode_rows(gen, k, m, mask, sv, er, rw);
  };
  ecx::LocatePlan lp;
  const int r = verify_err(ecx::plan_locate(k, m, present_mask, resolve, lp));
  if (r != ECX_OK) return r;
  const size_t n = lp.base.checked.size();
  std::copy(lp.base.survivors.begin(), lp.base.survivors.end(), survivors);
  std::copy(lp.base.checked.begin(), lp.base.checked.end(), checked);
  for (int i = 0; i < k; i++) {
    const ecx::VerifyPlan& cp = lp.cand[i];
    std::copy(cp.survivors.begin(), cp.survivors.end(),
              cand_survivors + (size_t)i * k);
    std::copy(cp.checked.begin(), cp.checked.end(),
              cand_checked + (size_t)i * (n - 1));
    std::copy(cp.rows.begin(), cp.rows.end(),
              cand_rows + (size_t)i * (n - 1) * k);
  }
  return (int)n;
}

uint64_t ecx_locate_word_probe(uint64_t present_mask, uint64_t survivor_mask,
                               uint64_t bad, uint64_t refuted) {
  return ecx::locate_word(present_mask, survivor_mask, bad, refuted);
}

int ecx_repair_batch(ecx_ctx* ctx, void* dptr, long n_stripes,
                     size_t chunk_bytes, uint64_t present_mask,
                     uint64_t* d_bad, uint64_t* d_culprit, long* n_repaired,
                     long* n_unlocatable, int slot) {
  if (!ctx || !n_repaired || !n_unlocatable || slot < 0 ||
      slot >= (int)ctx->slots.size())
    return ECX_ERR_INVAL;
  // one lock over locate, the download and the decode, so that no other call
  // on the slot comes between them
  Slot& s = ctx->slots[slot];
  std::lock_guard<std::recursive_mutex> g(s.mu);
  int r = ecx_locate_batch(ctx, dptr, n_stripes, chunk_bytes, present_mask,
                           d_bad, d_culprit, slot);
  if (r != ECX_OK) return r;
  std::vector<uint64_t> words((size_t)n_stripes * 2);
  uint64_t* bad = words.data();
  uint64_t* cul = bad + n_stripes;
  HIP_TRY(hipMemcpyAsync(bad, d_bad, (size_t)n_stripes * 8,
                         hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipMemcpyAsync(cul, d_culprit, (size_t)n_stripes * 8,
                         hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(wait_stream(s.stream));  // the one synchronisation of the call
  const int cps = ctx->k + ctx->m;
  const uint64_t all = cps >= 64 ? ~0ull : ((1ull << cps) - 1);
  long rep = 0, unl = 0;
  // per stripe: the mask without its culprit, or every chunk present (nothing
  // to rebuild, never written); the downloaded culprit words are reused
  for (long i = 0; i < n_stripes; i++) {
    const uint64_t c = cul[i];
    const bool located = bad[i] != 0 && c != 0 && (c & (c - 1)) == 0;
    rep += located;
    unl += bad[i] != 0 && !located;
    cul[i] = located ? present_mask & ~c : all;
  }
  *n_repaired = rep;
  *n_unlocatable = unl;
  if (rep == 0) return ECX_OK;  // nothing located, nothing launched
  return ecx_decode_batch_multi(ctx, dptr, n_stripes, chunk_bytes, cul, slot);
}

}  // extern "C"
