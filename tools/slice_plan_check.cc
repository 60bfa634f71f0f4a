// slice_plan_check.cc — stand-alone check of the host side of the slice calls
// (ceph_amd/csrc/slice_plan.cpp alone), meant to be built with the host
// sanitizers; the file is plain C++, so no GPU and no HIP is involved.
// Build and run from the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/slice_plan_check.cc ceph_amd/csrc/slice_plan.cpp -o /tmp/slice_plan_check && /tmp/slice_plan_check
//
// Every job table is filled into a heap buffer of exactly the planned size
// (the head in front poisoned, and required untouched), so a fill that runs
// past the plan is the sanitizer's to report; the tables are then compared
// with a restatement of the rule: slice s has ceil(vecs / VPB) blocks, in
// the order given, block b of a slice starts at vector b * VPB. Size lists:
// the block-edge sizes of the GPU tests, the same under permuted and
// repeating order lists with records, many tiny slices, a head in front.
// Every refusal is called next to the nearest accepted input. Exit status 0
// only if every answer is right.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../ceph_amd/csrc/slice_plan.h"

static int failures = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      failures++;                                 \
    }                                             \
  } while (0)

static const uint8_t HEAD_POISON = 0x5A;

static std::vector<void*> fake_ptrs(int n_slices, int cps, uint32_t seed) {
  // multiples of 16, some NULL; never followed
  std::vector<void*> p((size_t)n_slices * cps);
  uint32_t x = seed;
  for (auto& v : p) {
    x = x * 1664525u + 1013904223u;
    v = (x >> 28) == 0 ? nullptr : (void*)(uintptr_t)((uint64_t)x << 4);
  }
  return p;
}

// Plan, fill a buffer of exactly the planned size, compare with the rule.
static void check_tables(const char* what, int cps,
                         const std::vector<size_t>& bytes,
                         const std::vector<int>* order,
                         const std::vector<int>* recs, size_t head) {
  const int n = (int)bytes.size();
  const std::vector<void*> ptrs = fake_ptrs(n, cps, 0xEC + (uint32_t)n);
  const int* ord = order ? order->data() : nullptr;
  const int* rec = recs ? recs->data() : nullptr;
  const size_t n_order = order ? order->size() : (size_t)n;
  ecx::SliceLayout L;
  const bool ok = ecx::plan_slice_layout(cps, bytes.data(), n, ord, n_order,
                                         rec != nullptr, head, L);
  CHECK(ok, "%s: layout refused", what);
  if (!ok) return;

  const long V = ecx::SLICE_VPB;
  long want_blocks = 0;
  for (size_t i = 0; i < n_order; i++) {
    const long vecs = (long)(bytes[ord ? ord[i] : (int)i] / 16);
    want_blocks += (vecs + V - 1) / V;
  }
  CHECK(L.n_blocks == want_blocks, "%s: %ld blocks, want %ld", what,
        L.n_blocks, want_blocks);
  CHECK(L.off_ptrs == head && L.off_vecs == head + (size_t)n * cps * 8 &&
            L.off_voff == L.off_vecs + (size_t)n * 8 &&
            L.off_bslice == L.off_voff + (size_t)want_blocks * 8 &&
            L.off_brec == L.off_bslice + (size_t)want_blocks * 4 &&
            L.bytes == L.off_brec + (rec ? (size_t)want_blocks * 4 : 0),
        "%s: offsets", what);
  CHECK(L.off_ptrs % 8 == 0 && L.off_vecs % 8 == 0 && L.off_voff % 8 == 0 &&
            L.off_bslice % 4 == 0 && L.off_brec % 4 == 0,
        "%s: an array is misaligned", what);

  std::unique_ptr<uint8_t[]> blob(new uint8_t[L.bytes]);  // exactly
  std::memset(blob.get(), HEAD_POISON, L.bytes);
  ecx::fill_slice_tables(blob.get(), L, cps, ptrs.data(), bytes.data(), n, ord,
                         rec, n_order);
  for (size_t i = 0; i < head; i++)
    if (blob[i] != HEAD_POISON) {
      CHECK(false, "%s: head byte %zu written", what, i);
      break;
    }
  const uint64_t* tp = (const uint64_t*)(blob.get() + L.off_ptrs);
  const int64_t* tv = (const int64_t*)(blob.get() + L.off_vecs);
  const int64_t* tvo = (const int64_t*)(blob.get() + L.off_voff);
  const int32_t* tbs = (const int32_t*)(blob.get() + L.off_bslice);
  const int32_t* tbr = (const int32_t*)(blob.get() + L.off_brec);
  for (size_t i = 0; i < ptrs.size(); i++)
    CHECK(tp[i] == (uint64_t)(uintptr_t)ptrs[i], "%s: ptr %zu", what, i);
  for (int i = 0; i < n; i++)
    CHECK(tv[i] == (int64_t)(bytes[i] / 16), "%s: slice_vecs %d", what, i);
  long b = 0;
  for (size_t i = 0; i < n_order && b <= L.n_blocks; i++) {
    const int sl = ord ? ord[i] : (int)i;
    const long vecs = (long)(bytes[sl] / 16);
    for (long j = 0; j * V < vecs; j++, b++) {
      if (b >= L.n_blocks) break;
      CHECK(tbs[b] == sl && tvo[b] == j * V, "%s: block %ld", what, b);
      // the block is not empty and does not start past its slice
      CHECK(tvo[b] < tv[tbs[b]], "%s: block %ld starts past its slice", what,
            b);
      if (rec) CHECK(tbr[b] == rec[i], "%s: record of block %ld", what, b);
    }
  }
  CHECK(b == L.n_blocks, "%s: %ld blocks filled", what, b);
}

int main() {
  const size_t B = (size_t)ecx::SLICE_VPB * 16, T = ecx::SLICE_THREADS * 16;
  CHECK(B == 16384 && T == 4096, "block constants");
  // one vector; around a thread sweep; around a block; a second block one
  // past a sweep; a third block of one vector
  const std::vector<size_t> edge = {16,     T - 16, T,          T + 16, B - 16,
                                    B,      B + 16, B + T + 16, 2 * B + 16};
  for (size_t sz : edge)
    CHECK(ecx::slice_blocks(sz) == (long)((sz + B - 1) / B), "slice_blocks %zu",
          sz);
  CHECK(ecx::slice_blocks(B) == 1 && ecx::slice_blocks(B + 16) == 2 &&
            ecx::slice_blocks(2 * B + 16) == 3,
        "slice_blocks at the edges");

  for (int cps : {4, 6, 10, 11}) {
    check_tables("edge sizes", cps, edge, nullptr, nullptr, 0);
    check_tables("edge sizes behind a head", cps, edge, nullptr, nullptr,
                 3344);
    // reversed, with records
    std::vector<int> rev, rrec;
    for (int i = (int)edge.size() - 1; i >= 0; i--) {
      rev.push_back(i);
      rrec.push_back(100 + 7 * i);
    }
    check_tables("reversed order", cps, edge, &rev, &rrec, 2 * 3344);
    // a subset, out of order, one slice twice (two passes of one slice)
    const std::vector<int> sub = {8, 0, 7, 8, 3, 6};
    const std::vector<int> srec = {1, 0, 2, 5, 3, 4};
    check_tables("subset with a repeat", cps, edge, &sub, &srec, 8);
    check_tables("subset, no records", cps, edge, &sub, nullptr, 0);
    // an order that lists nothing: no blocks, the per-slice arrays alone
    const int none[1] = {0};
    ecx::SliceLayout L0;
    CHECK(ecx::plan_slice_layout(cps, edge.data(), (int)edge.size(), none, 0,
                                 true, 16, L0) &&
              L0.n_blocks == 0 &&
              L0.bytes == 16 + edge.size() * (size_t)(cps + 1) * 8,
          "empty order");
  }
  {  // the job-blob growth sizes: 64 slices, 6000 tiny ones, 8 of 3 blocks
    std::vector<size_t> many;
    for (int i = 0; i < 6000; i++) many.push_back(16 * (size_t)(1 + i % 4));
    check_tables("6000 tiny slices", 6, many, nullptr, nullptr, 0);
    check_tables("8 x 32784", 6, std::vector<size_t>(8, 2 * B + 16), nullptr,
                 nullptr, 0);
    std::vector<size_t> mid;
    for (int i = 0; i < 64; i++) mid.push_back(edge[(size_t)i % edge.size()]);
    check_tables("64 slices", 6, mid, nullptr, nullptr, 0);
  }

  // ---- refusals, each next to the nearest accepted call ----
  const int cps = 6;
  std::vector<size_t> bytes = {16, 4112};
  alignas(16) static uint8_t arena[16 * 16];
  std::vector<void*> p;
  for (int i = 0; i < 2 * cps; i++) p.push_back(arena + 16 * i);
  const uint64_t parity = 0x30;  // chunks 4, 5 written
  const uint64_t per_slice[2] = {0x30, 0x03};
  CHECK(ecx::check_slices(cps, p.data(), bytes.data(), 2, &parity, 0),
        "valid call refused");
  CHECK(ecx::check_slices(cps, p.data(), bytes.data(), 2, nullptr, 0),
        "valid call, nothing written, refused");
  CHECK(ecx::check_slices(cps, p.data(), bytes.data(), 2, per_slice, 1),
        "valid call, per-slice masks, refused");
  CHECK(!ecx::check_slices(cps, p.data(), bytes.data(), 0, &parity, 0),
        "n_slices 0 accepted");
  CHECK(!ecx::check_slices(cps, p.data(), bytes.data(), -1, &parity, 0),
        "n_slices -1 accepted");
  CHECK(!ecx::check_slices(cps, nullptr, bytes.data(), 2, &parity, 0) &&
            !ecx::check_slices(cps, p.data(), nullptr, 2, &parity, 0),
        "NULL array accepted");
  for (size_t bad : {(size_t)0, (size_t)8, (size_t)24, (size_t)4097}) {
    for (int at = 0; at < 2; at++) {
      std::vector<size_t> bb = bytes;
      bb[at] = bad;
      CHECK(!ecx::check_slices(cps, p.data(), bb.data(), 2, &parity, 0),
            "size %zu at %d accepted", bad, at);
    }
  }
  for (int at : {0, 3, 4, 2 * cps - 1}) {  // read and written chunks alike
    std::vector<void*> q = p;
    q[at] = (uint8_t*)q[at] + 8;
    CHECK(!ecx::check_slices(cps, q.data(), bytes.data(), 2, &parity, 0),
          "pointer %d at offset 8 accepted", at);
    q[at] = (uint8_t*)p[at] + 1;
    CHECK(!ecx::check_slices(cps, q.data(), bytes.data(), 2, nullptr, 0),
          "pointer %d at offset 1 accepted", at);
  }
  for (int sl = 0; sl < 2; sl++)
    for (int c = 0; c < cps; c++) {
      std::vector<void*> q = p;
      q[sl * cps + c] = nullptr;
      // uniform mask: NULL data is zeros, NULL parity is refused
      CHECK(ecx::check_slices(cps, q.data(), bytes.data(), 2, &parity, 0) ==
                (c < 4),
            "uniform mask: NULL chunk %d of slice %d", c, sl);
      // per-slice masks: the written set is the slice's own
      CHECK(ecx::check_slices(cps, q.data(), bytes.data(), 2, per_slice, 1) ==
                !(per_slice[sl] >> c & 1),
            "per-slice mask: NULL chunk %d of slice %d", c, sl);
      CHECK(ecx::check_slices(cps, q.data(), bytes.data(), 2, nullptr, 0),
            "nothing written: NULL chunk %d of slice %d refused", c, sl);
    }
  {  // every chunk of a slice NULL and none written: all zeros sources
    std::vector<void*> q(2 * cps, nullptr);
    const uint64_t zero = 0;
    CHECK(ecx::check_slices(cps, q.data(), bytes.data(), 2, &zero, 0),
          "all-NULL sources refused");
  }
  CHECK(!ecx::check_slice_ptrs(0, p.data(), 2, nullptr, 0) &&
            !ecx::check_slice_ptrs(65, p.data(), 2, nullptr, 0),
        "cps outside 1..64 accepted");

  ecx::SliceLayout L;
  CHECK(ecx::plan_slice_layout(cps, bytes.data(), 2, nullptr, 0, false, 0, L),
        "valid layout refused");
  // a head that is no multiple of 8 would misalign the u64 / i64 arrays that
  // follow it, and the layout never pads (the kernels' view of the table is
  // the offsets as computed): refused
  for (size_t head : {(size_t)1, (size_t)4, (size_t)12, (size_t)3340})
    CHECK(!ecx::plan_slice_layout(cps, bytes.data(), 2, nullptr, 0, true, head,
                                  L),
          "head %zu accepted", head);
  const int bad_order[3][2] = {{0, 2}, {-1, 0}, {1, 1 << 30}};
  for (const auto& o : bad_order)
    CHECK(!ecx::plan_slice_layout(cps, bytes.data(), 2, o, 2, true, 0, L),
          "order {%d, %d} accepted", o[0], o[1]);
  CHECK(!ecx::plan_slice_layout(cps, bytes.data(), 0, nullptr, 0, false, 0, L),
        "layout of no slices accepted");
  {  // 2^30 blocks are the most; one more is refused (planned, never filled)
    const size_t most = (size_t)ecx::SLICE_MAX_BLOCKS * B;
    std::vector<size_t> big = {most};
    CHECK(ecx::plan_slice_layout(cps, big.data(), 1, nullptr, 0, false, 0,
                                 L) &&
              L.n_blocks == ecx::SLICE_MAX_BLOCKS,
          "2^30 blocks refused");
    big[0] = most + 16;
    CHECK(!ecx::plan_slice_layout(cps, big.data(), 1, nullptr, 0, false, 0, L),
          "2^30 + 1 blocks accepted");
    big = {most, 16};
    CHECK(!ecx::plan_slice_layout(cps, big.data(), 2, nullptr, 0, false, 0, L),
          "2^30 + 1 blocks over two slices accepted");
    const int twice[2] = {0, 0};
    big = {most / 2 + B};
    CHECK(!ecx::plan_slice_layout(cps, big.data(), 1, twice, 2, true, 0, L),
          "2^30 + 2 blocks through a repeating order accepted");
  }

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("slice_plan_check: ok\n");
  return 0;
}
