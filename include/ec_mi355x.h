/* ec_mi355x.h — C-ABI of the MI355X-native erasure-coding core
 * (libec_mi355x_core.so).
 *
 * This is the drop-in boundary between host code (C++ plugin glue, Python
 * ctypes, or a real Ceph build) and the GPU backend. It sits exactly where
 * the reference crosses from its plugin glue into the GF library:
 *
 *   reference interface replaced                     where cited
 *   ------------------------------------------------ -------------------------
 *   jerasure_matrix_encode(k,m,w,matrix,data,coding, src/erasure-code/jerasure/
 *     blocksize) / isa ec_encode_data(len,k,m,tbls,    ErasureCodeJerasure.cc:382-387,
 *     data,coding)                                     src/erasure-code/isa/ErasureCodeIsa.cc:289-300
 *     -> ecx_encode()                                  (and the host-batch forms below)
 *   jerasure_matrix_decode(...)/isa_decode(...)      ErasureCodeJerasure.cc:389-396,
 *     -> ecx_decode()                                  ErasureCodeIsa.cc:371-570
 *   galois_region_xor / isa xor_gen (encode_delta)   ErasureCodeJerasure.cc:258-268,
 *     -> ecx_encode_delta()                            ErasureCodeIsa.cc:317-328
 *   galois_w08_region_multiply accumulate /          ErasureCodeJerasure.cc:285-331,
 *     isa ec_encode_data_update (apply_delta)          ErasureCodeIsa.cc:333-366
 *     -> ecx_apply_delta()                           (whole call fused:
 *                                                    ecx_apply_deltas_host; over a
 *                                                    batch: ecx_update_batch)
 *   scrub's re-encode-and-compare (encode_chunks     src/erasure-code/ErasureCodeInterface.h
 *     into a second buffer, then a compare pass)       encode_chunks, as used by the OSD
 *     -> ecx_verify_batch()                            scrub path
 *   naming and rebuilding the wrong shard of an      (no counterpart where the pool
 *     inconsistent stripe                              keeps no HashInfo)
 *     -> ecx_locate_batch(), ecx_repair_batch()
 *   ceph_crc32c over each shard                      src/osd/ECUtil.cc
 *     (ECUtil::HashInfo::append, EC deep scrub)        HashInfo::append
 *     -> ecx_crc32c_batch()
 *   minimum_to_decode survivor choice                src/erasure-code/ErasureCode.cc:154-170
 *     -> ecx_minimum_to_decode()
 *   get_chunk_size / get_alignment                   ErasureCodeIsa.cc:65-79,
 *     -> ecx_chunk_size()                              ErasureCodeJerasure.cc:85-108
 *
 * All compute runs on the GPU (hand-written HIP for gfx950). There is NO CPU
 * fallback: every entry point returns ECX_ERR_NO_GPU if no HIP device is
 * available. Host-side work is limited to matrix derivation (integers, once
 * per (k,m,technique)) and decode-table composition with an LRU cache
 * mirroring ErasureCodeIsaTableCache (src/erasure-code/isa/
 * ErasureCodeIsaTableCache.h:46-48).
 *
 * Conventions: int returns, 0 on success, negative errno-style on failure
 * (ErasureCodeInterface.h:29-35). Plain pointers and sizes only — no torch
 * or HIP types cross this boundary. Thread safety: one ecx_ctx may be used
 * from many threads concurrently (mirrors the reference's stateless-
 * after-prepare() plugin contract, ErasureCodeInterface.h:414-449); stream
 * slots are internally synchronised.
 */
#ifndef EC_MI355X_H
#define EC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECX_API __attribute__((visibility("default")))

/* Techniques (profile "technique" values of the mi355x plugin):
 *   reed_sol_van          -> ECX_T_RS_VAN_ISA  (bit-compatible with plugin=isa
 *                            technique=reed_sol_van matrix construction)
 *   cauchy                -> ECX_T_CAUCHY_ISA  (isa gf_gen_cauchy1_matrix)
 *   jerasure_reed_sol_van -> ECX_T_RS_VAN_JERASURE (jerasure w=8 matrix)
 * Values must match oracle/ec_ref.h enum ecref_technique. */
enum ecx_technique {
  ECX_T_RS_VAN_ISA = 0,
  ECX_T_CAUCHY_ISA = 1,
  ECX_T_RS_VAN_JERASURE = 2,
  /* jerasure cauchy_orig: bitmatrix/packet layout (w=8), profile key
   * packetsize (default 2048, ErasureCodeJerasure.h DEFAULT_PACKETSIZE);
   * chunk sizes must be multiples of w*packetsize
   * (ErasureCodeJerasureCauchy::get_alignment, ErasureCodeJerasure.cc:522-536) */
  ECX_T_CAUCHY_ORIG_JERASURE = 3,
  /* jerasure reed_sol_van with w=16: GF(2^16) over gf-complete's 0x1100B,
   * u16 LE symbols (galois_w16_region_multiply semantics). Select via
   * ecx_create2(..., w=16, ...) with this id. Compute-bound compatibility
   * technique; chunk sizes are multiples of k*w*4 / k = 64 B. */
  ECX_T_RS_VAN_JERASURE_W16 = 4,
  /* jerasure cauchy_good: cauchy_original + the n_ones-minimising improve
   * pass (jerasure cauchy.c cauchy_good_general_coding_matrix general
   * branch; ErasureCodeJerasure.cc:537-555). Same bitmatrix/packet layout
   * and chunk-size rule as ECX_T_CAUCHY_ORIG_JERASURE. m == 2 is refused
   * at this layer: jerasure's m==2 path reads precomputed cbest tables
   * that cannot be faithfully restated here. */
  ECX_T_CAUCHY_GOOD_JERASURE = 5,
};

enum ecx_err {
  ECX_OK = 0,
  ECX_ERR_INVAL = -22,      /* EINVAL */
  ECX_ERR_NOMEM = -12,      /* ENOMEM */
  ECX_ERR_IO = -5,          /* EIO: too many erasures / singular matrix */
  ECX_ERR_NO_GPU = -19,     /* ENODEV: no HIP device — no CPU fallback */
  ECX_ERR_HIP = -71,        /* EPROTO: unexpected HIP runtime failure */
};

typedef struct ecx_ctx ecx_ctx;

/* Version string of this ABI ("ec-mi355x <semver>"). The plugin shim's
 * __erasure_code_version() (ErasureCodePlugin.cc:162-171 gate) is provided
 * by the shim, not here. */
ECX_API const char *ecx_version(void);

/* Number of visible HIP devices (0 => every compute call fails ECX_ERR_NO_GPU). */
ECX_API int ecx_device_count(void);

/* Create a context for one (k, m, technique) on one device.
 * n_streams >= 1 internal HIP streams (round-robin per call).
 * Builds the generator matrix host-side and uploads lookup tables once,
 * mirroring prepare() (ErasureCodeIsa.cc:637-697). */
ECX_API int ecx_create(int k, int m, int technique, int device, int n_streams,
                       ecx_ctx **out);
/* Extended form: w (must be 8) and packetsize (bitmatrix techniques only;
 * ignored for matrix techniques). */
ECX_API int ecx_create2(int k, int m, int technique, int w, int packetsize,
                        int device, int n_streams, ecx_ctx **out);
ECX_API void ecx_destroy(ecx_ctx *ctx);

ECX_API int ecx_k(const ecx_ctx *ctx);
ECX_API int ecx_m(const ecx_ctx *ctx);

/* Generator matrix readback for tests/verification: fills (k+m)*k bytes
 * (identity top, coding rows below), isa-l row-major layout. */
ECX_API int ecx_get_matrix(const ecx_ctx *ctx, uint8_t *out);
/* w=16 variant: fills (k+m)*k u16 entries; EINVAL on w=8 contexts (and
 * vice versa for ecx_get_matrix). */
ECX_API int ecx_get_matrix16(const ecx_ctx *ctx, uint16_t *out);

/* Chunk-size rule of the technique (a7 in SURVEY §8):
 * ECX_T_*_ISA: ceil(width/k) rounded up to 32 (ErasureCodeIsa.cc:65-79);
 * ECX_T_RS_VAN_JERASURE: stripe padded to k*w*4, w=8
 * (ErasureCodeJerasure.cc:85-108). Both are multiples of 16 as the kernels
 * require. */
ECX_API unsigned ecx_chunk_size(const ecx_ctx *ctx, unsigned stripe_width);

/* Survivor selection (ErasureCode.cc:154-170): given bitmask of available
 * chunk ids (bit i = chunk i available) and wanted ids, fill minimum with
 * the chunk ids to fetch; returns count or negative errno. */
ECX_API int ecx_minimum_to_decode(const ecx_ctx *ctx, uint64_t want_mask,
                                  uint64_t avail_mask, uint64_t *minimum_mask);

/* ---------------- device-resident batch API (the hot path) ----------------
 * A batch buffer holds n_stripes stripes, each (k+m) chunks of chunk_bytes:
 * chunk c of stripe s lives at offset (s*(k+m) + c)*chunk_bytes. Chunks
 * 0..k-1 are data, k..k+m-1 parity. chunk_bytes must be a multiple of 16.
 */

/* Allocate/free a device buffer (returned handle is the device pointer). */
ECX_API int ecx_dbuf_alloc(ecx_ctx *ctx, size_t bytes, void **dptr);
ECX_API int ecx_dbuf_free(ecx_ctx *ctx, void *dptr);

/* Host<->device copies on a stream slot (slot < n_streams; blocking=1 syncs). */
ECX_API int ecx_upload(ecx_ctx *ctx, void *dptr, const void *host, size_t bytes,
                       int slot, int blocking);
ECX_API int ecx_download(ecx_ctx *ctx, void *host, const void *dptr,
                         size_t bytes, int slot, int blocking);

/* Fill a device buffer with deterministic pseudo-random bytes (seeded),
 * for bench/tests without 32 GiB PCIe uploads. */
ECX_API int ecx_dbuf_fill_random(ecx_ctx *ctx, void *dptr, size_t bytes,
                                 uint64_t seed, int slot);

/* Encode the batch in place: parity chunks k..k+m-1 of every stripe are
 * computed from data chunks 0..k-1. Replaces ec_encode_data /
 * jerasure_matrix_encode over the whole batch in one (or few) kernel
 * launches. */
ECX_API int ecx_encode_batch(ecx_ctx *ctx, void *dptr, long n_stripes,
                             size_t chunk_bytes, int slot);

/* Decode the batch in place under a uniform erasure pattern:
 * present_mask bit i set => chunk i of every stripe is intact. Erased
 * chunks are reconstructed (bit-exact re-encode for lost parity). Decode
 * rows are composed host-side and LRU-cached per erasure signature
 * (ErasureCodeIsa.cc:460-567). */
ECX_API int ecx_decode_batch(ecx_ctx *ctx, void *dptr, long n_stripes,
                             size_t chunk_bytes, uint64_t present_mask,
                             int slot);

/* Parity-delta batch ops (a6 in SURVEY §8):
 * delta = old ^ new over a device region; */
ECX_API int ecx_encode_delta_dev(ecx_ctx *ctx, const void *d_old,
                                 const void *d_new, void *d_delta,
                                 size_t bytes, int slot);
/* parity ^= M[coding_shard-k][data_shard] * delta (galois region multiply
 * accumulate) over a device region. */
ECX_API int ecx_apply_delta_dev(ecx_ctx *ctx, const void *d_delta,
                                int data_shard, int coding_shard,
                                void *d_parity, size_t bytes, int slot);

/* ---------------- variable-size slice batch (caller-shaped) --
 * The OSD write path calls encode_chunks once per page-aligned slice with
 * varying blocksize (shard_extent_map_t::encode, src/osd/ECUtil.cc:485-514,
 * EC_ALIGN_SIZE=4096) — many small calls. This entry point batches N such
 * slices into ONE kernel launch over device-resident chunk pointers.
 * Arrays are host-side, length n_slices:
 *   d_chunks[s*(k+m)+c] = device pointer to chunk c of slice s (data
 *     0..k-1 may be NULL => zeros);
 *   bytes[s] = slice length (nonzero multiple of 16).
 * Encode: parity pointers k..k+m-1 are written.
 * The kernels load and store 16 B vectors through the pointers as given, so
 * every non-NULL chunk pointer must be a multiple of 16. NULL is legal only
 * for a chunk the call reads (it then stands for a chunk of zeros, for that
 * slice alone); a chunk the call writes needs a buffer: for encode the
 * parity chunks k..k+m-1 of every slice. All validation precedes the first
 * enqueue, and a refused call launches nothing: ECX_ERR_INVAL for a NULL
 * array, a slot out of range, a bitmatrix or w=16 context, n_slices < 1, a
 * size that is 0 or no multiple of 16, a misaligned pointer, or a NULL
 * pointer for a written chunk.
 */
ECX_API int ecx_encode_slices(ecx_ctx *ctx, void *const *d_chunks,
                              const size_t *bytes, int n_slices, int slot);

/* Same for decode under a per-call uniform erasure pattern: the chunks
 * absent from present_mask are written in every slice and must not be NULL;
 * a present chunk may be NULL (zeros). Refusals as above, checked in the
 * order slot and arrays, sizes, mask (ECX_ERR_IO if undecodable), pointers —
 * all before the first enqueue, and also when the mask erases nothing (such
 * a valid call returns ECX_OK and launches nothing). */
ECX_API int ecx_decode_slices(ecx_ctx *ctx, void *const *d_chunks,
                              const size_t *bytes, int n_slices,
                              uint64_t present_mask, int slot);

/* ---------------- per-stripe erasure patterns (recovery batching) --------
 * A shim that batches degraded reads / recovery ops from many placement
 * groups holds stripes that miss DIFFERENT chunks. These forms take one
 * mask per stripe (per slice) instead of one per call:
 * present_masks[s] is stripe s's mask; same layout/semantics as
 * ecx_decode_batch applied to each stripe on its own — byte-identical
 * result, present chunks never written, a stripe with nothing erased never
 * touched. The number of kernel launches does not depend on how many
 * distinct patterns the call holds and is at most m (stripes are grouped
 * by how many chunks they lose, not by which). All validation precedes the
 * first launch: ECX_ERR_IO if ANY mask is undecodable, ECX_ERR_INVAL for a
 * NULL pointer, bad slot, chunk_bytes % 16, n_stripes outside 1..65535, a
 * bitmatrix or w=16 context (as for ecx_*_slices) or, for slices, a size
 * that is 0 or no multiple of 16, a chunk pointer that is no multiple of 16
 * or a NULL pointer for an erased chunk of that slice's mask (a present
 * chunk may be NULL: zeros) — in each case nothing has been launched. For
 * slices the order is slot and arrays, sizes, masks, pointers.
 * ecx_last_kernel_ms then covers the whole call (first launch to last). */
ECX_API int ecx_decode_batch_multi(ecx_ctx *ctx, void *dptr, long n_stripes,
                                   size_t chunk_bytes,
                                   const uint64_t *present_masks, int slot);
ECX_API int ecx_decode_slices_multi(ecx_ctx *ctx, void *const *d_chunks,
                                    const size_t *bytes, int n_slices,
                                    const uint64_t *present_masks, int slot);
/* CPU-only (no GPU context): the host-side grouping the two calls above
 * perform. plan_of_stripe[n] = index of the stripe's mask among distinct
 * masks in first-appearance order, -1 if nothing is erased; *n_plans =
 * number of distinct masks that erase something. Returns the number of
 * kernel launches, or -errno (ECX_ERR_IO if any mask is undecodable;
 * outputs are then left unwritten). */
ECX_API int ecx_decode_multi_plan_probe(int technique, int k, int m,
                                        const uint64_t *present_masks, long n,
                                        int *plan_of_stripe, int *n_plans);
/* CPU-only (no GPU context): the host side of the three slice calls before
 * anything is enqueued — the argument check, the cut into blocks and the job
 * table. cps = k + m; chunks[n_slices * cps] and bytes[n_slices] as for the
 * calls (the pointers are only looked at, never followed); written_masks[s]
 * bit c set => the call writes chunk c of slice s (NULL: nothing written).
 * Blocks are assigned to the slices order[0..n_order) in that order (NULL:
 * every slice once); recs[i], if given, is the launch record of the blocks
 * of order[i]; head = bytes kept in front of the table for the records, a
 * multiple of 8. out = {vectors per block, n_blocks, offsets of ptrs,
 * slice_vecs, block_voff, block_slice, block_rec in the table, table bytes};
 * the first min(blob_cap, table bytes) bytes of the table go to blob (head
 * zeroed). ECX_ERR_INVAL for whatever the calls refuse on these arguments,
 * an order entry outside 0..n_slices-1, recs without order, more than 2^30
 * blocks or a head that is no multiple of 8 (outputs are then left
 * unwritten). */
ECX_API int ecx_slice_plan_probe(int cps, void *const *chunks,
                                 const size_t *bytes, int n_slices,
                                 const uint64_t *written_masks,
                                 const int *order, const int *recs,
                                 long n_order, size_t head, long out[8],
                                 void *blob, size_t blob_cap);

/* ---------------- per-stripe write sets (write batching) ------------------
 * The partial-write counterpart of the per-stripe erasure patterns above: a
 * shim that batches small overwrites holds stripes that each replace a
 * DIFFERENT set of data chunks. dptr is the standard batch buffer with the
 * old data and old parity; write_masks[s] bit j (j < k) set => data chunk j
 * of stripe s is overwritten, 0 => the stripe is not touched at all. d_new
 * is a device buffer of the new chunks packed, stripe ascending then chunk
 * id ascending, chunk_bytes each: stripe s's first new chunk has index
 * new_base[s] = sum of the popcounts of the masks before s. Per stripe, for
 * each set bit j and each parity row r:
 *   P_r ^= G[k+r][j] * (old_j ^ new_j), then chunk j takes its new content
 * — encode_delta + apply_delta of every (data, coding) pair
 * (ErasureCodeIsa.cc:333-366, ErasureCodeJerasure.cc:285-331) over the whole
 * batch in ceil(m/4) launches whatever the masks are. Delta semantics: the
 * parity is read and corrected, never recomputed (a parity that was
 * inconsistent stays off by exactly the same bytes), and data chunks that
 * did not change are not read. All validation precedes the first launch:
 * ECX_ERR_INVAL for a NULL pointer, bad slot, chunk_bytes % 16, n_stripes
 * outside 1..65535, a mask bit at position k or above, a bitmatrix or w=16
 * context (as for ecx_*_slices and *_multi), or a d_new range that
 * intersects the batch. Every mask 0: ECX_OK, nothing launched.
 * ecx_last_kernel_ms covers the whole call (first launch to last). */
ECX_API int ecx_update_batch(ecx_ctx *ctx, void *dptr, long n_stripes,
                             size_t chunk_bytes, const void *d_new,
                             const uint64_t *write_masks, int slot);
/* CPU-only (no GPU context): the host-side preparation of the call above.
 * new_base[n] as defined there; active[] = ascending list of the stripes
 * with a nonzero mask (room for n), *n_active = how many. Returns the number
 * of kernel launches (ceil(m/4), 0 if no stripe is active), or
 * ECX_ERR_INVAL for a mask bit at position k or above (outputs are then
 * left unwritten). */
ECX_API int ecx_update_plan_probe(int k, int m, const uint64_t *write_masks,
                                  long n, long *new_base, int *active,
                                  int *n_active);

/* ---------------- consistency check (scrub) --------------------------------
 * Are the stored chunks still consistent with each other? The reference has
 * no call for it: deep scrub and the check after recovery re-encode the
 * stripe into a second buffer and compare (encode_chunks of
 * ErasureCodeInterface.h as used by the OSD scrub path), which costs another
 * m/(k+m) of the allocation and a second pass over the parities. This call
 * only reads: k + (checked chunks) chunk reads per stripe and one 8-byte
 * word written. dptr is the standard batch buffer; present_mask bit i set =>
 * chunk i of every stripe is held. The first k present chunks in id order
 * are the survivors (the rule of ecx_decode_batch, ErasureCode.cc:154-170)
 * and determine the stripe; every further present chunk, data or parity, is
 * checked: recomputed from the survivors and compared with what is stored.
 * d_bad is a device array of n_stripes 64-bit words, 8-byte aligned and
 * outside the batch. On success every word has been written: bit i of
 * d_bad[s] is set exactly when checked chunk i of stripe s differs in at
 * least one byte from its recomputed value; bits of survivors and of absent
 * chunks are always 0. A mask of exactly k chunks checks nothing: zeros,
 * nothing launched. The batch is never written. ceil(checked/4) launches
 * back to back; ecx_last_kernel_ms covers the whole call (first launch to
 * last). All validation precedes any GPU work: ECX_ERR_INVAL for a NULL
 * pointer, bad slot, chunk_bytes 0 or not a multiple of 16, n_stripes
 * outside 1..65535, d_bad not 8-byte aligned, a d_bad range that intersects
 * the batch, a mask bit at position k+m or above, or a bitmatrix or w=16
 * context (as for ecx_*_slices, *_multi and ecx_update_batch); ECX_ERR_IO
 * for fewer than k present chunks or survivors that do not invert (possible
 * after ecx_set_matrix). A refused call writes nothing to d_bad. */
ECX_API int ecx_verify_batch(ecx_ctx *ctx, const void *dptr, long n_stripes,
                             size_t chunk_bytes, uint64_t present_mask,
                             uint64_t *d_bad, int slot);
/* CPU-only (no GPU context): the planning of the call above. survivors[k] =
 * the first k set bits of the mask; checked[] = the remaining set bits,
 * ascending (room for m); rows[n_checked*k] = one coefficient row per
 * checked chunk over the survivors, taken from the decode-plan composition
 * of the survivors-only mask. Returns n_checked or -errno as above (outputs
 * are then left unwritten); w=8 matrix techniques only, the others return
 * ECX_ERR_INVAL. */
ECX_API int ecx_verify_plan_probe(int technique, int k, int m,
                                  uint64_t present_mask, int *survivors,
                                  int *checked, uint8_t *rows);

/* ---------------- locate and repair (scrub) --------------------------------
 * ecx_verify_batch says that a stripe is inconsistent, not which chunk is
 * wrong: a damaged checked chunk sets its own bit, a damaged survivor sets
 * every bit. Pools that keep per-shard hashes (HashInfo, ecx_crc32c_batch)
 * answer "which shard" from those; pools with EC overwrites keep none. With
 * two or more redundant chunks the code itself answers it. The whole
 * contract, for survivors and checked chunks as ecx_verify_batch defines
 * them:
 *   bit x of d_culprit[s] is set exactly when x is present and
 *   ecx_verify_batch under present_mask & ~(1 << x) would report 0 for
 *   stripe s
 * (leaving chunk x out makes the remaining chunks agree with each other),
 * and d_bad[s] is exactly the word ecx_verify_batch writes under
 * present_mask. For the MDS techniques this means: a clean stripe has
 * d_bad 0 and d_culprit == present_mask; exactly one damaged chunk x,
 * damaged anywhere and in any number of bytes, gives d_culprit == 1 << x;
 * two chunks damaged in different byte columns give d_culprit == 0; and with
 * d_bad != 0 the culprit word never has more than one bit. After
 * ecx_set_matrix the code need not be MDS: the definition still holds, more
 * than one bit is then possible, and callers treat that as "not located".
 * What the algebra cannot see: with exactly two checked chunks, two chunks
 * damaged in the same byte columns imitate a single damaged third chunk if,
 * in every damaged column, the second error is the one value of 255 that
 * fits the first; with three or more checked chunks two damaged chunks never
 * look like one.
 *
 * Both arrays are device arrays of n_stripes 64-bit words, 8-byte aligned,
 * outside the batch and disjoint from each other; the batch is never
 * written. Work, all on the slot's stream with no host synchronisation:
 * both arrays cleared, the passes of ecx_verify_batch, one launch that lists
 * the flagged stripes, then for each of the k survivors ceil((checked-1)/4)
 * launches that check "this survivor is the culprit" on the flagged stripes
 * only (a clean batch: every block leaves after one load), one launch that
 * forms the words. Leaving out a checked chunk needs no launch: its answer
 * is d_bad without that bit. ecx_last_kernel_ms covers first launch to last.
 * All validation precedes any GPU work and a refused call writes neither
 * array: every refusal of ecx_verify_batch, applied to each array, and
 * ECX_ERR_INVAL for arrays that overlap or are equal and for fewer than two
 * checked chunks (every present chunk would qualify); ECX_ERR_IO for fewer
 * than k present chunks and for a present_mask, or a present_mask less one
 * survivor, whose first k chunks do not invert (possible after
 * ecx_set_matrix). */
ECX_API int ecx_locate_batch(ecx_ctx *ctx, const void *dptr, long n_stripes,
                             size_t chunk_bytes, uint64_t present_mask,
                             uint64_t *d_bad, uint64_t *d_culprit, int slot);
/* CPU-only (no GPU context): the planning of the call above. survivors[k]
 * and checked[] (room for m) as ecx_verify_plan_probe. Candidate i leaves
 * out survivors[i]: cand_survivors[i*k ..] = its k survivors (the others
 * plus checked[0], ascending), cand_checked[i*(n-1) ..] = the n-1 chunks it
 * checks, cand_rows[(i*(n-1)+j)*k ..] = the row of its j-th checked chunk
 * over its survivors, n = n_checked. Returns n_checked or -errno as the call
 * (outputs are then left unwritten); w=8 matrix techniques only, the others
 * return ECX_ERR_INVAL. */
ECX_API int ecx_locate_plan_probe(int technique, int k, int m,
                                  uint64_t present_mask, int *survivors,
                                  int *checked, int *cand_survivors,
                                  int *cand_checked, uint8_t *cand_rows);
/* CPU-only: the rule the last launch applies per stripe. refuted has bit s
 * set when the candidate without survivor s found a difference. Returns
 * present_mask if bad == 0; otherwise (survivor_mask & ~refuted) together
 * with every checked bit j for which (bad & ~(1 << j)) == 0. */
ECX_API uint64_t ecx_locate_word_probe(uint64_t present_mask,
                                       uint64_t survivor_mask, uint64_t bad,
                                       uint64_t refuted);
/* Check, locate and repair in one call. Runs ecx_locate_batch into the two
 * arrays, then WAITS for the slot and downloads both (the one host
 * synchronisation of the batch API besides ecx_sync; 16 bytes per stripe),
 * and hands ecx_decode_batch_multi one mask per stripe on the same slot:
 * present_mask & ~d_culprit[s] where d_bad[s] != 0 and the culprit word has
 * exactly one bit, all k+m chunks otherwise. It returns with that decode
 * enqueued, as ecx_decode_batch_multi does. A located stripe gets its
 * culprit rebuilt, and its absent chunks too, as ecx_decode_batch would
 * under that mask; clean and unlocatable stripes are never written. Nothing
 * located: nothing more is launched. *n_repaired = the located stripes,
 * *n_unlocatable = the stripes with d_bad != 0 that were not. The arrays
 * keep the words of ecx_locate_batch, i.e. the state before the repair.
 * Refusals as ecx_locate_batch, and ECX_ERR_INVAL for a NULL count pointer;
 * after ecx_set_matrix a located stripe whose mask does not decode makes the
 * call return ECX_ERR_IO with the arrays written and the batch untouched. */
ECX_API int ecx_repair_batch(ecx_ctx *ctx, void *dptr, long n_stripes,
                             size_t chunk_bytes, uint64_t present_mask,
                             uint64_t *d_bad, uint64_t *d_culprit,
                             long *n_repaired, long *n_unlocatable, int slot);

/* ---------------- per-shard CRC-32C ----------------------------------------
 * The hash the OSD keeps per shard: ECUtil::HashInfo::append runs
 * ceph_crc32c(old_hash, shard_bytes, len) over each of the k+m shards of a
 * write (cumulative hashes start at -1), and EC deep scrub hashes each stored
 * shard again and compares. f(seed, data, len) = ceph_crc32c: the Castagnoli
 * polynomial, reflected (0x82F63B78), NO inversion of the seed or of the
 * result (the standard CRC-32C of a buffer is ~f(~0, buf)). The hash does
 * not depend on the code: every technique and w is accepted.
 *
 * dptr is the standard batch buffer. d_crc is a device array of
 * n_stripes*(k+m) 32-bit words; the word of chunk c of stripe s is
 * d_crc[s*(k+m)+c]. Exactly the words of the chunks in chunk_mask are
 * written, all others are left as they were.
 *   chain == 0: every chunk is hashed on its own. d_seed NULL seeds every
 *     hash with 0xFFFFFFFF; otherwise d_seed has the layout of d_crc, one
 *     seed per word. d_seed == d_crc is allowed: "append one more chunk to
 *     each running hash", in place.
 *   chain != 0: the stripes are consecutive stripes of one object (a
 *     HashInfo append of a multi-stripe write). d_seed is NULL or k+m words,
 *     one per shard; d_crc[s][c] = the hash of shard c's chunks of stripes
 *     0..s concatenated, from that shard's seed, so row n_stripes-1 is the
 *     new cumulative_shard_hashes.
 * The batch is never written. Two launches whatever the mask (a seed pass
 * over the words, then the hash pass), a third in chain mode (a log-step
 * scan over the words, not a loop over stripes); ecx_last_kernel_ms covers
 * the whole call, first launch to last. All validation precedes any GPU
 * work and a refused call writes nothing: ECX_ERR_INVAL for a NULL ctx, dptr
 * or d_crc, a bad slot, chunk_bytes 0 or not a multiple of 16, n_stripes
 * outside 1..65535, d_crc or d_seed not 4-byte aligned, a d_crc or d_seed
 * range that intersects the batch, a d_seed range that overlaps d_crc (other
 * than d_seed == d_crc with chain == 0), a mask bit at position k+m or
 * above, or a shape whose n_stripes*(k+m)*ceil(chunk_bytes/32768) blocks do
 * not fit 31 bits. A mask of 0 returns ECX_OK with nothing launched. There
 * is no host-pointer form: a chunk in host memory is hashed faster by the
 * host's own crc32 instruction than PCIe can deliver it. */
ECX_API int ecx_crc32c_batch(ecx_ctx *ctx, const void *dptr, long n_stripes,
                             size_t chunk_bytes, uint64_t chunk_mask,
                             const uint32_t *d_seed, int chain,
                             uint32_t *d_crc, int slot);
/* CPU-only (no GPU context). The library's host implementation of f: the
 * SSE4.2 crc32 instruction where the CPU has it, slice-by-4 tables
 * otherwise. *out = f(seed, data, len); returns 1 when the instruction was
 * used, 0 for the tables, ECX_ERR_INVAL for a NULL out (or NULL data with
 * len > 0). */
ECX_API int ecx_crc32c_probe(uint32_t seed, const void *data, size_t len,
                             uint32_t *out);
/* CPU-only. *out = crc * x^(8*nbytes) mod P: the state after nbytes zero
 * bytes. The one host routine the kernel's combine constants come from;
 * f(seed, A||B) = shift(f(seed, A), |B|) ^ f(0, B). */
ECX_API int ecx_crc32c_shift_probe(uint32_t crc, uint64_t nbytes,
                                   uint32_t *out);
/* CPU-only: what the launcher would launch for n_chunks masked chunks of
 * chunk_bytes in each of n_stripes stripes. out[0..7] = bytes per lane
 * segment L, segments per block, blocks per chunk, grid, threads, LDS bytes,
 * launches (chain mode adds one), 0. Segments and blocks are aligned to the
 * END of the chunk: segment j from the end is [C-(j+1)L, C-jL) cut at 0, a
 * block is `segments per block` of them. ECX_ERR_INVAL as the launcher for
 * bad sizes, n_chunks outside 1..64 or a NULL out. */
ECX_API int ecx_crc32c_plan_probe(size_t chunk_bytes, long n_stripes,
                                  int n_chunks, long out[8]);

/* CPU-only (no GPU context): what the bitmatrix launcher (cauchy_orig,
 * cauchy_good) would launch for n_out outputs over n_src sources of
 * chunk_bytes each, at word size w and packet size pkt, when the rows have
 * n_ops set bits. knobs = the values of ECX_BITQ, ECX_BITW, ECX_BITREG,
 * ECX_BITPIPE, ECX_BITT, ECX_BITXCD as given (unset: 16, 8, 2, 0, 256, 0);
 * the clamps are applied here as in the launcher. out[0..15] =
 *   0 kernel (0 LDS window, 1 register, 2 pipelined LDS window)
 *   1 register kernel: accumulator rows NR   2 register kernel: positions
 *   3 window bytes q      4 log2(q/16)       5 VQS instance (3/4/5, else -1)
 *   6 LDS-DMA staging (0: through registers) 7 16 B items per window
 *   8 windows per superword                  9 windows per chunk
 *  10 windows per block  11 grid x           12 threads per block
 *  13 dynamic LDS bytes  14 XCD mapping on   15 reserved (0)
 * with 6..10, 13 and 14 zero for the register kernel. Returns ECX_OK, or
 * ECX_ERR_INVAL exactly where the launcher refuses: n_src outside 1..16,
 * n_out outside 1..8, w outside 1..8, pkt no positive multiple of 16,
 * chunk_bytes no positive multiple of w*pkt (here also: 32 GiB or more), or
 * more than 65535 set bits on the LDS kernels. */
ECX_API int ecx_bitmatrix_plan_probe(const int knobs[6], int w, int pkt,
                                     int n_src, int n_out, long n_ops,
                                     size_t chunk_bytes, int out[16]);

/* Replace the coding rows of the generator with a custom m x k matrix
 * (clears decode-plan caches). Lets composed codecs — SHEC's shingled
 * matrix (src/erasure-code/shec/ErasureCodeShec.cc:700-768), custom
 * research codes — reuse every standard entry point. Matrix techniques
 * only (not bitmatrix). */
ECX_API int ecx_set_matrix(ecx_ctx *ctx, const uint8_t *coding_rows);

/* Generic GF(2^8) matmul over host chunks: outs[j] = XOR_i rows[j*n_src+i]
 * * srcs[i]. The primitive behind jerasure_matrix_dotprod
 * (used by SHEC decode, ErasureCodeShec.cc:1030-1046); srcs may be NULL
 * (zeros). Stages over PCIe and runs the standard kernel. */
ECX_API int ecx_matmul_chunks_host(ecx_ctx *ctx,
                                   const uint8_t *const *srcs, int n_src,
                                   uint8_t *const *outs, int n_out,
                                   const uint8_t *rows, size_t bytes);

/* SHEC shingled coding matrix (m x k), restated from the reference's
 * in-tree shec_reedsolomon_coding_matrix (ErasureCodeShec.cc:700-768);
 * single != 0 selects the SINGLE technique. */
ECX_API int ecx_shec_matrix(int k, int m, int c, int single, uint8_t *out);

/* CPU-only probes (no GPU context; usable on a GPU-less box for tests):
 * generator readback for any technique id — fills (k+m)*k bytes, identity
 * top — and jerasure cauchy.c's cauchy_n_ones(e, w=8). */
ECX_API int ecx_gen_matrix_probe(int technique, int k, int m, uint8_t *out);
ECX_API int ecx_cauchy_n_ones_probe(int e);
/* decode-plan composition probe: survivors[k], erased[<=m],
 * rows[n_erased*k]; returns n_erased or -errno. */
ECX_API int ecx_decode_rows_probe(int technique, int k, int m,
                                  uint64_t present_mask, int *survivors,
                                  int *erased, uint8_t *rows);

/* CPU-only probe of the streaming batch kernel's table builder: the five
 * v_perm table dwords for coefficient c over the bit groups 0-2 / 3-5 / 6-7.
 * Byte x&7 of {out[0], out[1]} ^ byte (x>>3)&7 of {out[2], out[3]} ^ byte
 * x>>6 of out[4] (little-endian byte order) is c*x in GF(2^8). */
ECX_API int ecx_gf8_tabs332_probe(uint8_t c, uint32_t out[5]);

/* CPU-only probe of the streaming batch kernel's tile walk: the (stripe,
 * tile in chunk) pairs that hardware block `hw_block` of a `grid`-block
 * launch visits, in order, for a batch of n_stripes stripes of
 * tiles_per_chunk 4 KiB tiles, under stripe-group width `width` (0 or more
 * than n_stripes: all stripes) and, with xcd != 0, the XCD-contiguous block
 * mapping. Runs the kernel's own start/step code. Writes at most `cap`
 * pairs and returns how many the block visits, or -errno. */
ECX_API int ecx_stream_walk_probe(uint32_t n_stripes, uint32_t tiles_per_chunk,
                                  uint32_t width, int xcd, uint32_t grid,
                                  uint32_t hw_block, uint32_t *stripes,
                                  uint32_t *tiles, int cap);

/* Generic device-batch GF(2^8) matmul over the standard batch layout:
 * out chunk ids = XOR_i rows[j*n_src+i] * src chunk ids, per stripe. The
 * composition primitive for layered codes (LRC layers, custom research
 * codes) on device-resident batches; w=8 matrix techniques only. */
ECX_API int ecx_matmul_batch(ecx_ctx *ctx, void *dptr, long n_stripes,
                             size_t chunk_bytes, const int *src_ids,
                             int n_src, const int *out_ids, int n_out,
                             const uint8_t *rows, int slot);

/* Synchronise a stream slot. */
ECX_API int ecx_sync(ecx_ctx *ctx, int slot);

/* Milliseconds of the most recent kernel on this slot (hipEvent pair
 * recorded around the kernel on ITS stream — bench.py's roofline source). */
ECX_API int ecx_last_kernel_ms(ecx_ctx *ctx, int slot, double *ms);

/* ---------------- host-pointer API (plugin path) ----------------
 * Mirrors the reference glue's char** marshalling
 * (ErasureCodeJerasure.cc:124-159, ErasureCodeIsa.cc:118-165): k data
 * pointers (NULL => chunk of zeros, the zeros-buffer convention) and m
 * parity pointers. Stages over PCIe, runs the same kernels, copies back.
 * One stripe per call; for throughput use the batch API. */
ECX_API int ecx_encode_chunks_host(ecx_ctx *ctx,
                                   const uint8_t *const *data /* [k] */,
                                   uint8_t *const *parity /* [m] */,
                                   size_t chunk_bytes);

/* decode_chunks semantics (ErasureCodeIsa.cc:167-243): chunks[] has k+m
 * entries; present_mask marks intact chunks; chunks[i] for erased ids must
 * be valid writable buffers (NULL allowed for intact ids the caller does
 * not have — treated as zeros, matching the reference's invented-zeros
 * buffers at ErasureCodeIsa.cc:212-226). */
ECX_API int ecx_decode_chunks_host(ecx_ctx *ctx, uint8_t *const *chunks,
                                   uint64_t present_mask, size_t chunk_bytes);

/* ecx_verify_batch for a scrub caller with one stripe in host memory:
 * chunks[] has k+m entries, entries of absent ids are ignored, *bad receives
 * the stripe's word. A NULL entry for a present id is ECX_ERR_INVAL — unlike
 * decode, a chunk that is not given cannot be vouched for. Uploads the
 * present chunks, downloads 8 bytes; same refusals as the batch call. */
ECX_API int ecx_verify_chunks_host(ecx_ctx *ctx, const uint8_t *const *chunks,
                                   uint64_t present_mask, size_t chunk_bytes,
                                   uint64_t *bad);

/* ecx_locate_batch for one stripe in host memory, built like the call above:
 * *bad and *culprit receive the stripe's two words. A NULL entry for a
 * present id is ECX_ERR_INVAL. Uploads the present chunks, downloads 16
 * bytes; same refusals as the batch call. */
ECX_API int ecx_locate_chunks_host(ecx_ctx *ctx, const uint8_t *const *chunks,
                                   uint64_t present_mask, size_t chunk_bytes,
                                   uint64_t *bad, uint64_t *culprit);

ECX_API int ecx_encode_delta_host(ecx_ctx *ctx, const uint8_t *old_data,
                                  const uint8_t *new_data, uint8_t *delta,
                                  size_t bytes);
ECX_API int ecx_apply_delta_host(ecx_ctx *ctx, const uint8_t *delta,
                                 int data_shard, int coding_shard,
                                 uint8_t *parity, size_t bytes);
/* Fused form of ecx_apply_delta_host for a whole apply_delta call
 * (ErasureCodeIsa.cc:333-366, ErasureCodeJerasure.cc:285-331): for every j,
 *   parities[j] ^= XOR_i G[coding_shards[j]][data_shards[i]] * deltas[i]
 * with every delta and every parity uploaded once, one accumulating launch
 * (w=16: per <= 4 parities; bitmatrix: one per pair), every parity
 * downloaded once and a single wait at the end. Bytes identical to looping
 * ecx_apply_delta_host over the pairs, for every technique. ECX_ERR_INVAL
 * for NULL pointers, shard ids out of range, n_in outside 1..k, n_out
 * outside 1..m or bytes % 16. */
ECX_API int ecx_apply_deltas_host(ecx_ctx *ctx, const uint8_t *const *deltas,
                                  const int *data_shards, int n_in,
                                  uint8_t *const *parities,
                                  const int *coding_shards, int n_out,
                                  size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* EC_MI355X_H */
