// bit_plan.cpp — see bit_plan.h.
#include "bit_plan.h"

#include <algorithm>
#include <cstring>
#include <utility>

#include "../../include/ec_mi355x.h"

namespace ecx {

int bit_plan(const BitKnobs &kn, int w, int pkt, int n_src, int n_out,
             size_t n_ops, size_t chunk_bytes, BitPlan *p) {
  if (n_src < 1 || n_src > BIT_MAX_SRC || n_out < 1 || n_out > BIT_MAX_OUT)
    return ECX_ERR_INVAL;
  // what a context can hold (ecx_create2): row_map and row_off have room
  // for w <= 8, and every kernel moves whole 16 B vectors of a packet
  if (w < 1 || w > 8 || pkt < 16 || pkt % 16) return ECX_ERR_INVAL;
  if (chunk_bytes == 0 || chunk_bytes % ((size_t)w * pkt))
    return ECX_ERR_INVAL;
  *p = BitPlan{};
  p->vqs = -1;

  // LDS window: largest power-of-two divisor of pkt within the LDS budget
  // (ECX_BITQ KB). Default 16 from the MI355X sweep: small windows keep
  // 8+ blocks/CU resident and beat large windows by ~19%
  // (profiles/rocprof_r01_summary.md).
  const size_t lds_budget = (size_t)std::clamp(kn.bitq_kib, 8, 120) * 1024;
  int q = 16;
  while (q * 2 <= pkt && pkt % (q * 2) == 0 &&
         (size_t)n_src * w * q * 2 <= lds_budget)
    q *= 2;
  int vq_shift = 0;
  while ((1 << vq_shift) < q / 16) vq_shift++;
  if ((16 << vq_shift) != q) return ECX_ERR_INVAL;
  p->q = q;
  p->vq_shift = vq_shift;

  // v3 register-accumulator path (no LDS staging, no barrier): measured
  // policy — at n_out == 1 (single-erasure decode, delta apply) the LDS
  // kernel idles most of each block's compute items while v3 keeps every
  // lane busy (7.13 vs 7.64 ms); at n_out >= 2 the LDS kernel wins
  // (n_out=2 decode 8.02 vs 11.04; m=3 encode 10.43 vs 10.85).
  // ECX_BITREG: 0 = never, 1 = always (n_out <= 4), 2/unset = auto.
  const bool use_reg =
      kn.reg == 1 ? n_out <= 4 : (kn.reg == 2 ? n_out == 1 : false);
  if (use_reg && w == 8) {
    p->kernel = BIT_REG;
    p->nr = n_out * 8;
    p->n_pos = (long)(chunk_bytes >> 7);  // 16B vecs, 8 pkts/sw
    p->grid_x = std::min<long>((p->n_pos + 255) / 256, 16384);
    p->threads = 256;
    return ECX_OK;
  }

  if (n_ops > 0xffff) return ECX_ERR_INVAL;  // row_off is u16
  const long sw_per_chunk = (long)(chunk_bytes / ((size_t)w * pkt));
  p->windows_per_sw = pkt / q;
  p->n_windows = sw_per_chunk * p->windows_per_sw;
  // windows per block: amortizes the ops staging and block start/drain
  // over several LDS-window rounds without growing the LDS footprint
  // (q stays small => 8 blocks/CU residency); MI355X sweep default 8.
  p->wpb = std::clamp(kn.wpb, 1, 4096);
  p->grid_x = (p->n_windows + p->wpb - 1) / p->wpb;
  const size_t data_bytes = (size_t)n_src * w * q;
  const size_t ops_bytes = (((n_ops + 1) & ~(size_t)1) * 2 + 15) & ~(size_t)15;
  p->items = n_src * w * (q >> 4);
  p->dma = (p->items & 63) == 0;
  // 2-buffer glds pipeline: measured SLOWER (18.0 vs 10.9 ms at wpb=8,
  // profiles r2) — halved residency outweighs the in-block overlap at
  // 8-blocks/CU occupancy, as the CDNA guide's regime note predicts.
  // Kept behind the knob as a recorded negative.
  const bool pipe = kn.pipe && p->wpb > 1 && p->dma &&
                    2 * data_bytes + ops_bytes <= 160 * 1024;
  p->lds_bytes = (pipe ? 2 * data_bytes : data_bytes) + ops_bytes;
  if (pipe) {
    p->kernel = BIT_PIPE;
    p->threads = 256;
    return ECX_OK;
  }
  p->kernel = BIT_LDS;
  // block size: 128-thread blocks double the independent blocks per CU
  // (16 at q=128) so co-resident blocks interleave DMA-wait and compute
  // phases more finely
  p->threads = (kn.threads == 64 || kn.threads == 128) ? kn.threads : 256;
  if (w == 8 && vq_shift >= 3 && vq_shift <= 5) p->vqs = vq_shift;
  p->xcdmap = kn.xcd && p->windows_per_sw == 8 &&
              p->n_windows % ((long)p->wpb * 64) == 0 && p->grid_x % 64 == 0;
  return ECX_OK;
}

size_t bit_count_ops(const uint8_t *bit_rows, int w, int n_src, int n_out) {
  const size_t n = (size_t)n_out * w * n_src * w;
  size_t ops = 0;
  for (size_t i = 0; i < n; i++) ops += bit_rows[i] != 0;
  return ops;
}

size_t bit_lds_blob_bytes(size_t n_ops) {
  return sizeof(EcBitParams) + ((n_ops + 1) & ~(size_t)1) * 2;
}

void bit_fill_lds_blob(const BitPlan &p, int w, int pkt, const int *src_ids,
                       int n_src, const int *out_ids, int n_out,
                       const uint8_t *bit_rows, uint8_t *blob) {
  const int n_rows = n_out * w, W = n_src * w;
  EcBitParams hdr;
  std::memset(&hdr, 0, sizeof(hdr));
  hdr.n_src = n_src;
  hdr.n_out = n_out;
  hdr.w = w;
  hdr.pkt = pkt;
  hdr.q = p.q;
  hdr.vq_shift = p.vq_shift;
  for (int i = 0; i < n_src; i++) hdr.src_ids[i] = src_ids[i];
  for (int j = 0; j < n_out; j++) hdr.out_ids[j] = out_ids[j];
  // sort rows by op count (waves span several rows; uniform lengths kill
  // the max-over-rows divergence in the compute loop)
  std::pair<int, int> order[BIT_MAX_OUT * 8];
  for (int r = 0; r < n_rows; r++) {
    int cnt = 0;
    const uint8_t *row = bit_rows + (size_t)r * W;
    for (int c = 0; c < W; c++) cnt += row[c] != 0;
    order[r] = {cnt, r};
  }
  std::sort(order, order + n_rows);
  uint16_t *ops = (uint16_t *)(blob + sizeof(hdr));
  size_t n = 0;
  for (int rr = 0; rr < n_rows; rr++) {
    const int r = order[rr].second;
    hdr.row_map[rr] = (uint8_t)r;
    hdr.row_off[rr] = (uint16_t)n;
    const uint8_t *row = bit_rows + (size_t)r * W;
    for (int c = 0; c < W; c++)
      if (row[c]) ops[n++] = (uint16_t)c;
  }
  hdr.row_off[n_rows] = (uint16_t)n;
  if (n & 1) ops[n] = 0;  // pad: kernel copies ops as dwords
  std::memcpy(blob, &hdr, sizeof(hdr));
}

void bit_fill_reg_blob(int pkt, const int *src_ids, int n_src,
                       const int *out_ids, int n_out, const uint8_t *bit_rows,
                       EcBitRegParams *hdr) {
  std::memset(hdr, 0, sizeof(*hdr));
  hdr->n_src = n_src;
  hdr->pkt = pkt;
  for (int i = 0; i < n_src; i++) hdr->src_ids[i] = src_ids[i];
  for (int j = 0; j < n_out; j++) hdr->out_ids[j] = out_ids[j];
  const int W8 = n_src * 8, nr = n_out * 8;
  for (int j = 0; j < n_src; j++)
    for (int c = 0; c < 8; c++) {
      uint32_t mbits = 0;
      for (int r = 0; r < nr; r++)
        if (bit_rows[(size_t)r * W8 + j * 8 + c]) mbits |= 1u << r;
      hdr->colmask[j * 8 + c] = mbits;
    }
}

}  // namespace ecx
