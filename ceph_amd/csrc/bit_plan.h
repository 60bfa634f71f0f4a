// bit_plan.h — host-side launch plan and job blobs of the jerasure bitmatrix
// path (cauchy_orig, cauchy_good) and its CPU-only probe. Plain C++: no HIP,
// no device state, so run_bitmatrix and ecx_bitmatrix_plan_probe run
// literally the same code and the tests can ask on a GPU-less box which
// kernel instance, window, grid and LDS size a shape gets.
//
// A launch applies n_out*w bit rows over n_src*w source packets. Three
// kernels can take it: the LDS-window kernel (a q-byte window of every
// source packet staged in LDS, compile-time geometry for q = 128/256/512 at
// w = 8), its two-buffer software-pipelined variant, and the
// register-accumulator kernel (no LDS, n_out <= 4). Every ECX_BIT* knob that
// chooses among them, or sizes a window, block or grid, acts here and
// nowhere else.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ecx {

constexpr int BIT_MAX_K = 32;    // = ECX_MAX_K (slots in the id arrays)
constexpr int BIT_MAX_SRC = 16;  // sources one launch takes
constexpr int BIT_MAX_OUT = 8;   // = ECX_MAX_OUT, outputs per launch

// ---- device-visible job headers (layouts are the kernels' ABI) ----

struct EcBitParams {
  int n_src;   // k
  int n_out;   // output chunks this launch (rows = n_out*w)
  int w;
  int pkt;     // packetsize bytes
  int q;       // LDS window bytes (power-of-two divisor of pkt)
  int vq_shift;  // log2(q/16)
  int src_ids[BIT_MAX_K];
  int out_ids[BIT_MAX_OUT];
  uint16_t row_off[BIT_MAX_OUT * 8 + 1];  // prefix offsets into ops[]
  // rows are stored sorted by op count so the 4 rows sharing a wave have
  // similar lengths (divergence waste 5.6-7.8% -> 0.6-3.5% measured);
  // row_map[r] = original row id (output chunk out_ids[orig/w], packet
  // orig%w)
  uint8_t row_map[BIT_MAX_OUT * 8];
  // blob continues with uint16 ops[row_off[n_rows]]: values j*w+c
};

struct EcBitRegParams {
  int n_src;
  int pkt;
  int src_ids[BIT_MAX_K];
  int out_ids[4];
  uint32_t colmask[BIT_MAX_K * 8];  // bit r of colmask[j*8+c]: row r uses (j,c)
};

// ---- the plan ----

// The knobs as given (unset: the default), before clamping.
struct BitKnobs {
  int bitq_kib = 16;  // ECX_BITQ: LDS window budget, clamped to 8..120 KiB
  int wpb = 8;        // ECX_BITW: windows per block, clamped to 1..4096
  int reg = 2;        // ECX_BITREG: 0 never, 1 always (n_out <= 4), 2 auto
  int pipe = 0;       // ECX_BITPIPE: two-buffer pipelined LDS kernel
  int threads = 256;  // ECX_BITT: LDS kernel block size, 64/128/256 else 256
  int xcd = 0;        // ECX_BITXCD: XCD-cooperative window mapping
};

enum BitKernel { BIT_LDS = 0, BIT_REG = 1, BIT_PIPE = 2 };

struct BitPlan {
  int kernel;   // BitKernel
  int nr;       // BIT_REG: accumulator rows (8 * n_out), else 0
  long n_pos;   // BIT_REG: 16 B positions per chunk, else 0
  int q;        // LDS window bytes
  int vq_shift;  // log2(q / 16)
  int vqs;      // BIT_LDS: compile-time instance 3/4/5, or -1 (generic)
  int dma;      // window items % 64 == 0: LDS-DMA staging, else via registers
  int items;    // 16 B items per window (n_src * w * q / 16)
  int windows_per_sw;
  long n_windows;  // per chunk
  int wpb;         // windows per block
  long grid_x;     // grid.y is the stripe count
  int threads;
  size_t lds_bytes;  // dynamic LDS of the launch
  int xcdmap;
};

// Plan one launch: n_ops is the number of set bits in its rows. Returns 0,
// or ECX_ERR_INVAL (p unspecified) for n_src outside 1..16, n_out outside
// 1..8, w outside 1..8, pkt no positive multiple of 16, chunk_bytes no
// positive multiple of w*pkt, or an op list past 65535 entries.
int bit_plan(const BitKnobs &kn, int w, int pkt, int n_src, int n_out,
             size_t n_ops, size_t chunk_bytes, BitPlan *p);

// ---- the job blobs, as pure functions of the bit rows ----

// Set bits of the (n_out*w) x (n_src*w) row-major rows (one byte per bit).
size_t bit_count_ops(const uint8_t *bit_rows, int w, int n_src, int n_out);

// LDS and pipe kernels: EcBitParams followed by the u16 op list, padded to
// whole dwords (the kernels copy it as dwords).
size_t bit_lds_blob_bytes(size_t n_ops);
void bit_fill_lds_blob(const BitPlan &p, int w, int pkt, const int *src_ids,
                       int n_src, const int *out_ids, int n_out,
                       const uint8_t *bit_rows, uint8_t *blob);

// Register kernel (w = 8): one EcBitRegParams.
void bit_fill_reg_blob(int pkt, const int *src_ids, int n_src,
                       const int *out_ids, int n_out, const uint8_t *bit_rows,
                       EcBitRegParams *hdr);

}  // namespace ecx
