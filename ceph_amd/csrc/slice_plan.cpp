// slice_plan.cpp — see slice_plan.h
#include "slice_plan.h"

namespace ecx {

static_assert(sizeof(long) == 8 && sizeof(void *) == 8,
              "the kernels read the i64 arrays as long, the pointers as u64");

bool check_slice_sizes(const size_t *bytes, int n_slices) {
  if (!bytes || n_slices < 1) return false;
  size_t bad = 0;
  for (int i = 0; i < n_slices; i++) {
    if (bytes[i] == 0) return false;
    bad |= bytes[i];
  }
  return (bad & 15) == 0;
}

bool check_slice_ptrs(int cps, void *const *chunks, int n_slices,
                      const uint64_t *written, size_t written_stride) {
  if (!chunks || n_slices < 1 || cps < 1 || cps > 64) return false;
  uintptr_t low = 0;
  for (int i = 0; i < n_slices; i++) {
    void *const *p = chunks + (size_t)i * cps;
    uint64_t null_mask = 0;
    for (int c = 0; c < cps; c++) {
      low |= (uintptr_t)p[c];
      null_mask |= (uint64_t)(p[c] == nullptr) << c;
    }
    if (written && (null_mask & written[(size_t)i * written_stride]))
      return false;
  }
  return (low & 15) == 0;
}

bool check_slices(int cps, void *const *chunks, const size_t *bytes,
                  int n_slices, const uint64_t *written,
                  size_t written_stride) {
  return check_slice_sizes(bytes, n_slices) &&
         check_slice_ptrs(cps, chunks, n_slices, written, written_stride);
}

bool plan_slice_layout(int cps, const size_t *bytes, int n_slices,
                       const int *order, size_t n_order, bool with_recs,
                       size_t head, SliceLayout &L) {
  if (!bytes || n_slices < 1 || cps < 1 || head % 8) return false;
  if (!order) n_order = (size_t)n_slices;
  long n_blocks = 0;
  for (size_t i = 0; i < n_order; i++) {
    const int sl = order ? order[i] : (int)i;
    if (sl < 0 || sl >= n_slices) return false;
    n_blocks += slice_blocks(bytes[sl]);
    if (n_blocks > SLICE_MAX_BLOCKS) return false;
  }
  L.n_blocks = n_blocks;
  L.off_ptrs = head;
  L.off_vecs = head + (size_t)n_slices * cps * 8;
  L.off_voff = L.off_vecs + (size_t)n_slices * 8;
  L.off_bslice = L.off_voff + (size_t)n_blocks * 8;
  L.off_brec = L.off_bslice + (size_t)n_blocks * 4;
  L.bytes = L.off_brec + (with_recs ? (size_t)n_blocks * 4 : 0);
  return true;
}

void fill_slice_tables(uint8_t *blob, const SliceLayout &L, int cps,
                       void *const *chunks, const size_t *bytes, int n_slices,
                       const int *order, const int *recs, size_t n_order) {
  uint64_t *ptrs = (uint64_t *)(blob + L.off_ptrs);
  long *svecs = (long *)(blob + L.off_vecs);
  long *bvoff = (long *)(blob + L.off_voff);
  int *bslice = (int *)(blob + L.off_bslice);
  int *brec = (int *)(blob + L.off_brec);
  const size_t n_ptrs = (size_t)n_slices * cps;
  for (size_t i = 0; i < n_ptrs; i++) ptrs[i] = (uint64_t)chunks[i];
  for (int i = 0; i < n_slices; i++) svecs[i] = (long)(bytes[i] >> 4);
  if (!order) n_order = (size_t)n_slices;
  long b = 0;
  for (size_t i = 0; i < n_order; i++) {
    const int sl = order ? order[i] : (int)i;
    for (long v = 0; v < svecs[sl]; v += SLICE_VPB) {
      bslice[b] = sl;
      bvoff[b] = v;
      if (recs) brec[b] = recs[i];
      b++;
    }
  }
}

}  // namespace ecx
