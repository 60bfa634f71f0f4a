// slice_plan.h — host side of the variable-size slice calls
// (ecx_encode_slices / ecx_decode_slices / ecx_decode_slices_multi) and their
// CPU-only probe. Plain C++: no HIP, no device state, so the probe and the
// real calls run literally the same code and it can be tested (and
// sanitized) on a GPU-less box.
//
// A call hands over n_slices slices of k+m chunk pointers each and one length
// per slice. Before anything is enqueued the host
//   1. checks the arguments (check_slices): the kernels load and store 16 B
//      vectors through the pointers as given, so a size or a pointer that is
//      no multiple of 16, or a NULL pointer for a chunk that is written, must
//      never reach them. NULL stays legal for a chunk that is only read: it
//      means a chunk of zeros for that slice;
//   2. cuts every slice into blocks of SLICE_VPB vectors and lays the job
//      table out behind `head` bytes the caller keeps for launch records
//      (plan_slice_layout):
//        [ptrs u64 n_slices*cps][slice_vecs i64 n_slices]
//        [block_voff i64 n_blocks][block_slice i32 n_blocks]
//        [block_rec i32 n_blocks, only with records]
//   3. fills the table in the order the kernels read it (fill_slice_tables).
#pragma once

#include <cstddef>
#include <cstdint>

namespace ecx {

constexpr int SLICE_THREADS = 256;
constexpr int SLICE_VPB = SLICE_THREADS * 4;  // 16 B vectors per block
constexpr long SLICE_MAX_BLOCKS = 1L << 30;

inline long slice_blocks(size_t bytes) {
  return (long)((bytes >> 4) + SLICE_VPB - 1) / SLICE_VPB;
}

// n_slices >= 1 and every size a nonzero multiple of 16.
bool check_slice_sizes(const size_t *bytes, int n_slices);

// Every non-NULL pointer a multiple of 16, and no NULL pointer for a chunk
// that is written: chunk c of slice s is written if bit c of
// written[s * written_stride] is set (stride 0: one mask for the whole call;
// written == NULL: nothing is written). cps = k + m <= 64.
bool check_slice_ptrs(int cps, void *const *chunks, int n_slices,
                      const uint64_t *written, size_t written_stride);

// Both of the above.
bool check_slices(int cps, void *const *chunks, const size_t *bytes,
                  int n_slices, const uint64_t *written,
                  size_t written_stride);

struct SliceLayout {
  size_t off_ptrs;    // == head
  size_t off_vecs;
  size_t off_voff;
  size_t off_bslice;
  size_t off_brec;    // == bytes when there are no records
  size_t bytes;       // the whole blob, head included
  long n_blocks;
};

// Blocks are assigned to the slices order[0..n_order) in that order (order
// == NULL: every slice once, n_order ignored). False — L unspecified — for
// more than SLICE_MAX_BLOCKS blocks, an order entry outside 0..n_slices-1, or
// a head that is no multiple of 8: the 8-byte arrays come first, so they are
// aligned exactly when head is, and the layout never pads.
bool plan_slice_layout(int cps, const size_t *bytes, int n_slices,
                       const int *order, size_t n_order, bool with_recs,
                       size_t head, SliceLayout &L);

// Fill blob[L.off_ptrs, L.bytes); blob[0, head) is not touched. recs[i],
// when given, is the record index of the blocks of order[i] (recs needs the
// layout planned with_recs).
void fill_slice_tables(uint8_t *blob, const SliceLayout &L, int cps,
                       void *const *chunks, const size_t *bytes, int n_slices,
                       const int *order, const int *recs, size_t n_order);

}  // namespace ecx
