// Tile walk of ec_gf_stream_kernel, shared by the kernel,
// the bandwidth probe (tools/membench.hip) and the CPU walk probe
// (ecx_stream_walk_probe), so that all three enumerate the same schedule.
//
// A tile is 4 KiB (256 lanes x 16 B) of one chunk position range of one
// stripe. Stripes are cut into groups of `width` consecutive stripes and
// tiles are numbered
//     (stripe group, tile in chunk, stripe in group)
// with the last index fastest: width 1 walks a stripe's tiles before the
// next stripe's (tile fastest), width n_stripes walks one tile position of
// every stripe first (stripe fastest). When width does not divide n_stripes
// the last group is walked at full width and the positions past the last
// stripe are skipped, so the walk needs no division and no second shape.
//
// Logical block b visits tile numbers b, b + grid, b + 2 grid, ...; the step
// is split on the host into (groups, tiles, stripes) so the device adds and
// carries. The logical block is the hardware block id, or with `xcd` set the
// remapped one: the hardware deals consecutive block ids round-robin to the
// ECX_WALK_XCDS compute dies, and
//     logical = (id % X) * (grid / X) + min(id % X, grid % X) + id / X
// hands each die one contiguous run of the logical order. For a grid that is
// a multiple of X this is (id % X) * (grid / X) + id / X; the min() term
// keeps it a bijection on [0, grid) otherwise.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECX_WALK_FN __host__ __device__ inline
#else
#define ECX_WALK_FN inline
#endif

#define ECX_WALK_XCDS 8u

// Launch-uniform, host-computed (ecx_walk_make).
struct EcxWalk {
  uint32_t n_stripes;
  uint32_t tpc;        // tiles per chunk
  uint32_t width;      // stripes per group, 1..n_stripes
  uint32_t n_groups;   // ceil(n_stripes / width)
  uint32_t group_sz;   // tpc * width, saturated (only divides block ids)
  uint32_t step_g, step_t, step_s;  // grid split over (group, tile, stripe)
  uint32_t xcd;        // 1: XCD-contiguous block mapping
  uint32_t xcd_q, xcd_r;            // grid / X, grid % X
};

// Where a block stands: tile `t` of stripe `g * width + s`.
struct EcxWalkPos {
  uint32_t g, t, s;
};

// grid >= 1 blocks, n_stripes >= 1, tpc >= 1. width 0 or > n_stripes means
// n_stripes.
inline EcxWalk ecx_walk_make(uint32_t n_stripes, uint32_t tpc, uint32_t width,
                             int xcd, uint32_t grid) {
  EcxWalk w;
  w.n_stripes = n_stripes;
  w.tpc = tpc;
  w.width = (width == 0 || width > n_stripes) ? n_stripes : width;
  w.n_groups = (n_stripes + w.width - 1) / w.width;
  const uint64_t gs = (uint64_t)tpc * w.width;
  // block ids are 32-bit, so a saturated group size still puts every start
  // in group 0 with the id itself as remainder
  w.group_sz = gs > 0xffffffffull ? 0xffffffffu : (uint32_t)gs;
  w.step_g = (uint32_t)(grid / gs);
  const uint32_t rem = (uint32_t)(grid % gs);
  w.step_t = rem / w.width;
  w.step_s = rem % w.width;
  w.xcd = xcd ? 1u : 0u;
  w.xcd_q = grid / ECX_WALK_XCDS;
  w.xcd_r = grid % ECX_WALK_XCDS;
  return w;
}

// First position of hardware block `hw_block` (the only divisions of a
// block's life, by launch-uniform values).
ECX_WALK_FN EcxWalkPos ecx_walk_start(const EcxWalk& w, uint32_t hw_block) {
  uint32_t lb = hw_block;
  if (w.xcd) {
    const uint32_t x = hw_block % ECX_WALK_XCDS;
    lb = x * w.xcd_q + (x < w.xcd_r ? x : w.xcd_r) + hw_block / ECX_WALK_XCDS;
  }
  EcxWalkPos p;
  p.g = lb / w.group_sz;
  const uint32_t rem = lb - p.g * w.group_sz;
  p.t = rem / w.width;
  p.s = rem - p.t * w.width;
  return p;
}

// The walk is over once this is false.
ECX_WALK_FN bool ecx_walk_live(const EcxWalk& w, const EcxWalkPos& p) {
  return p.g < w.n_groups;
}

// Stripe of a live position; >= n_stripes in the skipped part of the last
// group.
ECX_WALK_FN uint32_t ecx_walk_stripe(const EcxWalk& w, const EcxWalkPos& p) {
  return p.g * w.width + p.s;
}

// One grid step on: add and carry, each carry at most once.
ECX_WALK_FN void ecx_walk_next(const EcxWalk& w, EcxWalkPos& p) {
  p.s += w.step_s;
  if (p.s >= w.width) {
    p.s -= w.width;
    p.t++;
  }
  p.t += w.step_t;
  if (p.t >= w.tpc) {
    p.t -= w.tpc;
    p.g++;
  }
  p.g += w.step_g;
}
