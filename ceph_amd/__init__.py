"""ceph_amd — Python bindings for the MI355X-native erasure-coding core.

Product path: thin ctypes over the C-ABI of include/ec_mi355x.h
(libec_mi355x_core.so, hand-written HIP for gfx950). There is NO CPU
fallback anywhere in this package: if the extension is missing or no GPU is
visible, calls raise, loudly.
"""
import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libec_mi355x_core.so")

T_RS_VAN_ISA = 0
T_CAUCHY_ISA = 1
T_RS_VAN_JERASURE = 2
T_CAUCHY_ORIG_JERASURE = 3
T_RS_VAN_JERASURE_W16 = 4
T_CAUCHY_GOOD_JERASURE = 5
TECHNIQUES = {
    "reed_sol_van": T_RS_VAN_ISA,
    "cauchy": T_CAUCHY_ISA,
    "jerasure_reed_sol_van": T_RS_VAN_JERASURE,
    "cauchy_orig": T_CAUCHY_ORIG_JERASURE,
    "jerasure_reed_sol_van_w16": T_RS_VAN_JERASURE_W16,
    "cauchy_good": T_CAUCHY_GOOD_JERASURE,
}

_ERR = {
    -22: "EINVAL", -12: "ENOMEM", -5: "EIO (too many erasures / singular)",
    -19: "ENODEV (no GPU — the mi355x EC core has no CPU fallback)",
    -71: "EPROTO (HIP runtime failure)",
}


class EcError(RuntimeError):
    pass


def _lib():
    if not os.path.exists(_SO):
        raise EcError(
            f"{_SO} not built. Run `make core` at the repo root (or "
            "python -c 'import __graft_entry__; __graft_entry__.build()').")
    lib = ctypes.CDLL(_SO)
    lib.ecx_version.restype = ctypes.c_char_p
    lib.ecx_device_count.restype = ctypes.c_int
    lib.ecx_create.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_void_p)]
    lib.ecx_create2.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_void_p)]
    lib.ecx_chunk_size.restype = ctypes.c_uint
    lib.ecx_chunk_size.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    lib.ecx_minimum_to_decode.argtypes = [
        ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
        ctypes.POINTER(ctypes.c_uint64)]
    lib.ecx_dbuf_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_void_p)]
    lib.ecx_dbuf_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ecx_upload.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_int, ctypes.c_int]
    lib.ecx_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_int, ctypes.c_int]
    lib.ecx_dbuf_fill_random.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_uint64,
                                         ctypes.c_int]
    lib.ecx_encode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_int]
    lib.ecx_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_int]
    lib.ecx_encode_delta_dev.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 3 + [
        ctypes.c_size_t, ctypes.c_int]
    lib.ecx_apply_delta_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_int]
    lib.ecx_encode_slices.argtypes = [ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_size_t),
                                      ctypes.c_int, ctypes.c_int]
    lib.ecx_decode_slices.argtypes = [ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_size_t),
                                      ctypes.c_int, ctypes.c_uint64,
                                      ctypes.c_int]
    lib.ecx_decode_batch_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_long, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.c_int]
    lib.ecx_decode_slices_multi.argtypes = [ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_size_t),
                                            ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_int]
    lib.ecx_decode_multi_plan_probe.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(ctypes.c_uint64), ctypes.c_long,
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.ecx_slice_plan_probe.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_int), ctypes.c_long, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_long), ctypes.c_void_p, ctypes.c_size_t]
    lib.ecx_update_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_uint64),
                                     ctypes.c_int]
    lib.ecx_update_plan_probe.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_long, ctypes.POINTER(ctypes.c_long),
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.ecx_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_int]
    lib.ecx_verify_plan_probe.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ctypes.c_void_p]
    lib.ecx_verify_chunks_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint64)]
    lib.ecx_locate_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_int]
    lib.ecx_locate_chunks_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]
    lib.ecx_locate_plan_probe.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
        ctypes.c_void_p]
    lib.ecx_locate_word_probe.restype = ctypes.c_uint64
    lib.ecx_locate_word_probe.argtypes = [ctypes.c_uint64] * 4
    lib.ecx_repair_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_long),
                                     ctypes.POINTER(ctypes.c_long),
                                     ctypes.c_int]
    lib.ecx_crc32c_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_int]
    lib.ecx_crc32c_probe.argtypes = [ctypes.c_uint32, ctypes.c_void_p,
                                     ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_uint32)]
    lib.ecx_crc32c_shift_probe.argtypes = [ctypes.c_uint32, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_uint32)]
    lib.ecx_crc32c_plan_probe.argtypes = [ctypes.c_size_t, ctypes.c_long,
                                          ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_long)]
    lib.ecx_bitmatrix_plan_probe.argtypes = [
        ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int)]
    lib.ecx_apply_deltas_host.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
        ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
        ctypes.c_int, ctypes.c_size_t]
    lib.ecx_set_matrix.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ecx_matmul_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_int),
                                     ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_int),
                                     ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_int]
    lib.ecx_shec_matrix.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_void_p]
    lib.ecx_gf8_tabs332_probe.argtypes = [ctypes.c_uint8,
                                          ctypes.POINTER(ctypes.c_uint32)]
    lib.ecx_stream_walk_probe.argtypes = [
        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
        ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    lib.ecx_sync.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ecx_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_double)]
    lib.ecx_get_matrix.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ecx_get_matrix16.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ecx_encode_chunks_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_size_t]
    lib.ecx_decode_chunks_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_size_t]
    lib.ecx_encode_delta_host.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 3 + [
        ctypes.c_size_t]
    lib.ecx_apply_delta_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_size_t]
    return lib


_cached_lib = None


def lib():
    global _cached_lib
    if _cached_lib is None:
        _cached_lib = _lib()
    return _cached_lib


def version():
    return lib().ecx_version().decode()


def device_count():
    return lib().ecx_device_count()


def shec_matrix(k, m, c, single=False):
    """SHEC shingled coding matrix (host-side; no GPU needed)."""
    out = np.zeros((m, k), dtype=np.uint8)
    _ck(lib().ecx_shec_matrix(k, m, c, int(single),
                              out.ctypes.data_as(ctypes.c_void_p)),
        "ecx_shec_matrix")
    return out


def gf8_tabs332_probe(c):
    """CPU-only: the streaming batch kernel's five table dwords for
    coefficient c (bit groups 0-2 / 3-5 / 6-7), as a uint32 array."""
    out = np.zeros(5, dtype=np.uint32)
    _ck(lib().ecx_gf8_tabs332_probe(
        c, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
        "ecx_gf8_tabs332_probe")
    return out


def stream_walk_probe(n_stripes, tiles_per_chunk, width, xcd, grid, hw_block):
    """CPU-only: the (stripe, tile) pairs, as an (n, 2) uint32 array in visit
    order, that one hardware block of the streaming batch kernel takes under
    stripe-group width `width` and the XCD-contiguous mapping `xcd`."""
    # the walk rounds the stripe count up to whole groups: under 2x the tiles
    cap = (2 * n_stripes * tiles_per_chunk) // max(1, grid) + 2
    st = np.zeros(cap, dtype=np.uint32)
    ti = np.zeros(cap, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    n = _ck(lib().ecx_stream_walk_probe(
        n_stripes, tiles_per_chunk, width, int(bool(xcd)), grid, hw_block,
        st.ctypes.data_as(u32p), ti.ctypes.data_as(u32p), cap),
        "ecx_stream_walk_probe")
    if n > cap:
        raise EcError(f"ecx_stream_walk_probe: block visits {n} > {cap} tiles")
    return np.stack([st[:n], ti[:n]], axis=1)


def _ck(r, what):
    if isinstance(r, int) and r < 0:
        raise EcError(f"{what}: {_ERR.get(r, r)}")
    return r


def _mask_array(masks, n, what):
    """Per-stripe present masks (any integer sequence or a np.uint64
    array) as a contiguous uint64 array of exactly n entries."""
    a = np.asarray(masks)
    if a.size and (a.dtype.kind not in "iu" or
                   (a.dtype.kind == "i" and a.min() < 0)):
        raise EcError(f"{what}: present_masks must be integers that fit "
                      f"uint64 (got dtype {a.dtype})")
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 1 or a.shape[0] != n:
        raise EcError(f"{what}: need {n} present_masks (one per stripe or "
                      f"slice), got shape {a.shape}")
    return a


def _u64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def decode_multi_plan_probe(technique, k, m, masks):
    """CPU-only: how decode_batch_multi / decode_slices_multi would group
    these per-stripe masks. Returns (n_launches, plan_of_stripe, n_plans);
    plan_of_stripe[s] is the index of stripe s's mask among the distinct
    masks in first-appearance order, -1 if nothing is erased."""
    t = TECHNIQUES[technique] if isinstance(technique, str) else technique
    a = _mask_array(masks, len(masks), "ecx_decode_multi_plan_probe")
    pos = np.zeros(max(len(a), 1), dtype=np.int32)
    n_plans = ctypes.c_int()
    r = _ck(lib().ecx_decode_multi_plan_probe(
        t, k, m, _u64p(a), len(a),
        pos.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        ctypes.byref(n_plans)), "ecx_decode_multi_plan_probe")
    return r, pos[:len(a)], n_plans.value


def slice_plan_probe(cps, chunk_ptrs, sizes, written_masks=None, order=None,
                     recs=None, head=0):
    """CPU-only: what the slice calls do on the host before anything is
    enqueued, for n slices of cps chunk addresses each (integers, None or 0 =
    NULL; never followed) and their sizes. written_masks[s] bit c = the call
    writes chunk c of slice s. Raises EINVAL for what the calls refuse.
    Returns a dict: vecs_per_block, n_blocks, the offsets off_* and bytes of
    the job table behind `head`, and the table's arrays ptrs, slice_vecs,
    block_voff, block_slice, block_rec (None without recs) and the whole
    `blob` as the kernels would read them."""
    what = "ecx_slice_plan_probe"
    n = len(sizes)
    arr = (ctypes.c_void_p * max(len(chunk_ptrs), 1))()
    for i, p in enumerate(chunk_ptrs):
        arr[i] = None if p in (None, 0) else int(p)
    sz = (ctypes.c_size_t * max(n, 1))(*sizes)
    wr = None
    if written_masks is not None:
        wa = _mask_array(written_masks, n, what)
        wr = _u64p(wa)
    i32p = ctypes.POINTER(ctypes.c_int)
    oa = ra = None
    if order is not None:
        oa = np.ascontiguousarray(order, dtype=np.int32)
    if recs is not None:
        ra = np.ascontiguousarray(recs, dtype=np.int32)
        if oa is None or len(ra) != len(oa):
            raise EcError(f"{what}: recs needs an order of the same length")
    op = None if oa is None else oa.ctypes.data_as(i32p)
    rp = None if ra is None else ra.ctypes.data_as(i32p)
    n_order = 0 if oa is None else len(oa)
    out = (ctypes.c_long * 8)()
    _ck(lib().ecx_slice_plan_probe(cps, arr, sz, n, wr, op, rp, n_order,
                                   head, out, None, 0), what)
    blob = np.zeros(out[7], dtype=np.uint8)
    _ck(lib().ecx_slice_plan_probe(cps, arr, sz, n, wr, op, rp, n_order,
                                   head, out, blob.ctypes.data_as(
                                       ctypes.c_void_p), blob.nbytes), what)
    g = dict(zip(("vecs_per_block", "n_blocks", "off_ptrs", "off_vecs",
                  "off_voff", "off_bslice", "off_brec", "bytes"), out))
    nb = g["n_blocks"]

    def view(off, count, dt):
        return blob[off:off + count * np.dtype(dt).itemsize].view(dt)

    g.update(blob=blob,
             ptrs=view(g["off_ptrs"], n * cps, np.uint64),
             slice_vecs=view(g["off_vecs"], n, np.int64),
             block_voff=view(g["off_voff"], nb, np.int64),
             block_slice=view(g["off_bslice"], nb, np.int32),
             block_rec=None if ra is None else view(g["off_brec"], nb,
                                                    np.int32))
    return g


def update_plan_probe(k, m, masks):
    """CPU-only: how update_batch would prepare these per-stripe write
    masks. Returns (n_launches, new_base, active): new_base[s] is the index
    of stripe s's first new chunk in the packed d_new, active the ascending
    stripes with a nonzero mask."""
    a = _mask_array(masks, len(masks), "ecx_update_plan_probe")
    base = np.zeros(max(len(a), 1), dtype=np.int64)
    act = np.zeros(max(len(a), 1), dtype=np.int32)
    n_act = ctypes.c_int()
    r = _ck(lib().ecx_update_plan_probe(
        k, m, _u64p(a), len(a),
        base.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
        act.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        ctypes.byref(n_act)), "ecx_update_plan_probe")
    return r, base[:len(a)], act[:n_act.value]


def verify_plan_probe(technique, k, m, present_mask):
    """CPU-only: how verify_batch would plan this present mask. Returns
    (survivors, checked, rows): the first k present chunk ids, the remaining
    present ids ascending, and one coefficient row per checked chunk over
    the survivors (an (n_checked, k) uint8 array)."""
    t = TECHNIQUES[technique] if isinstance(technique, str) else technique
    sv = np.zeros(max(k, 1), dtype=np.int32)
    ck = np.zeros(max(m, 1), dtype=np.int32)
    rows = np.zeros((max(m, 1), max(k, 1)), dtype=np.uint8)
    n = _ck(lib().ecx_verify_plan_probe(
        t, k, m, present_mask,
        sv.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        ck.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        rows.ctypes.data_as(ctypes.c_void_p)), "ecx_verify_plan_probe")
    return sv[:k], ck[:n], rows.reshape(-1)[:n * k].reshape(n, k)


def locate_plan_probe(technique, k, m, present_mask):
    """CPU-only: how locate_batch would plan this present mask. Returns
    (survivors, checked, cand_survivors, cand_checked, cand_rows): the base
    plan as verify_plan_probe gives it, and for candidate i (survivor i left
    out) its k survivors, the n_checked - 1 chunks it checks and one row per
    such chunk over its survivors; shapes (k, k), (k, n-1) and (k, n-1, k)."""
    t = TECHNIQUES[technique] if isinstance(technique, str) else technique
    k1, m1 = max(k, 1), max(m, 1)
    ip = ctypes.POINTER(ctypes.c_int)
    sv = np.zeros(k1, dtype=np.int32)
    ck = np.zeros(m1, dtype=np.int32)
    csv = np.zeros(k1 * k1, dtype=np.int32)
    cck = np.zeros(k1 * m1, dtype=np.int32)
    rows = np.zeros(k1 * m1 * k1, dtype=np.uint8)
    n = _ck(lib().ecx_locate_plan_probe(
        t, k, m, present_mask, sv.ctypes.data_as(ip), ck.ctypes.data_as(ip),
        csv.ctypes.data_as(ip), cck.ctypes.data_as(ip),
        rows.ctypes.data_as(ctypes.c_void_p)), "ecx_locate_plan_probe")
    return (sv[:k], ck[:n], csv.reshape(k, k),
            cck[:k * (n - 1)].reshape(k, n - 1),
            rows[:k * (n - 1) * k].reshape(k, n - 1, k))


def locate_word_probe(present_mask, survivor_mask, bad, refuted):
    """CPU-only: the culprit word locate_batch forms for one stripe from its
    verify word and the survivor candidates that were refuted."""
    return int(lib().ecx_locate_word_probe(int(present_mask),
                                           int(survivor_mask), int(bad),
                                           int(refuted)))


def crc32c_probe(seed, data, with_path=False):
    """CPU-only: ceph_crc32c(seed, data) by the library's host routine (no
    inversion of seed or result). data is bytes or a uint8 array (any
    offset, contiguous). with_path=True returns (crc, path), path "sse4.2"
    or "tables"."""
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(
        data, (bytes, bytearray, memoryview)) else np.asarray(data)
    if a.dtype != np.uint8 or a.ndim != 1 or (a.size and a.strides[0] != 1):
        raise EcError("ecx_crc32c_probe: need contiguous uint8 data")
    out = ctypes.c_uint32()
    r = _ck(lib().ecx_crc32c_probe(
        int(seed) & 0xFFFFFFFF, a.ctypes.data if a.size else None, a.size,
        ctypes.byref(out)), "ecx_crc32c_probe")
    return (out.value, "sse4.2" if r else "tables") if with_path else out.value


def crc32c_shift_probe(crc, nbytes):
    """CPU-only: crc * x^(8*nbytes) mod P, the CRC state after nbytes zero
    bytes: f(seed, A+B) == shift(f(seed, A), len(B)) ^ f(0, B)."""
    out = ctypes.c_uint32()
    _ck(lib().ecx_crc32c_shift_probe(int(crc) & 0xFFFFFFFF, nbytes,
                                     ctypes.byref(out)),
        "ecx_crc32c_shift_probe")
    return out.value


_CRC_PLAN_FIELDS = ("seg_bytes", "segs_per_block", "blocks_per_chunk", "grid",
                    "threads", "lds_bytes", "launches", "reserved")


def crc32c_plan_probe(chunk_bytes, n_stripes, n_chunks):
    """CPU-only: what crc32c_batch would launch for n_chunks masked chunks,
    as a dict. Segments and blocks are aligned to the END of a chunk."""
    out = (ctypes.c_long * 8)()
    _ck(lib().ecx_crc32c_plan_probe(chunk_bytes, n_stripes, n_chunks, out),
        "ecx_crc32c_plan_probe")
    return dict(zip(_CRC_PLAN_FIELDS, (int(v) for v in out)))


_BIT_KNOBS = (("ECX_BITQ", 16), ("ECX_BITW", 8), ("ECX_BITREG", 2),
              ("ECX_BITPIPE", 0), ("ECX_BITT", 256), ("ECX_BITXCD", 0))


def bitmatrix_plan_probe(n_src, n_out, pkt, chunk_bytes, n_ops, knobs=None,
                         w=8):
    """CPU-only: what the bitmatrix launcher would launch for n_out outputs
    over n_src sources of chunk_bytes each, whose bit rows have n_ops set
    bits. knobs maps ECX_BIT* names to values as the environment would give
    them (missing: the default). Returns a dict: kernel ("lds", "reg" or
    "pipe"), nr, n_pos, grid, threads, q, vq_shift and, for the two LDS
    kernels, vqs, staging ("dma" or "reg"), items, wps, n_windows, wpb,
    lds_bytes, xcdmap."""
    knobs = knobs or {}
    kn = (ctypes.c_int * 6)(*[int(knobs.get(n, d)) for n, d in _BIT_KNOBS])
    out = (ctypes.c_int * 16)()
    _ck(lib().ecx_bitmatrix_plan_probe(kn, w, pkt, n_src, n_out, n_ops,
                                       chunk_bytes, out),
        "ecx_bitmatrix_plan_probe")
    kernel = ("lds", "reg", "pipe")[out[0]]
    g = dict(kernel=kernel, grid=out[11], threads=out[12], q=out[3],
             vq_shift=out[4])
    if kernel == "reg":
        g.update(nr=out[1], n_pos=out[2])
    else:
        g.update(vqs=out[5], staging="dma" if out[6] else "reg",
                 items=out[7], wps=out[8], n_windows=out[9], wpb=out[10],
                 lds_bytes=out[13], xcdmap=bool(out[14]))
    return g


def _ptr_array(bufs):
    arr = (ctypes.c_void_p * len(bufs))()
    for i, b in enumerate(bufs):
        arr[i] = None if b is None else b.ctypes.data_as(ctypes.c_void_p).value
    return arr


class EcContext:
    """One (k, m, technique) codec bound to one GPU, mirroring a plugin
    instance after init()/prepare() (ErasureCodeIsa.cc:637-697)."""

    def __init__(self, k, m, technique="reed_sol_van", device=0,
                 n_streams=2, packetsize=2048, w=8):
        t = TECHNIQUES[technique] if isinstance(technique, str) else technique
        if t == T_RS_VAN_JERASURE_W16:
            w = 16
        self._h = ctypes.c_void_p()
        self.k, self.m, self.technique = k, m, technique
        self.packetsize = packetsize
        _ck(lib().ecx_create2(k, m, t, w, packetsize, device, n_streams,
                              ctypes.byref(self._h)), "ecx_create2")

    def close(self):
        if self._h:
            lib().ecx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def matrix(self):
        if TECHNIQUES.get(self.technique) == T_RS_VAN_JERASURE_W16:
            a = np.zeros((self.k + self.m, self.k), dtype=np.uint16)
            _ck(lib().ecx_get_matrix16(
                self._h, a.ctypes.data_as(ctypes.c_void_p)),
                "ecx_get_matrix16")
            return a
        a = np.zeros((self.k + self.m, self.k), dtype=np.uint8)
        _ck(lib().ecx_get_matrix(self._h, a.ctypes.data_as(ctypes.c_void_p)),
            "ecx_get_matrix")
        return a

    def chunk_size(self, stripe_width):
        return lib().ecx_chunk_size(self._h, stripe_width)

    def minimum_to_decode(self, want_mask, avail_mask):
        out = ctypes.c_uint64()
        _ck(lib().ecx_minimum_to_decode(self._h, want_mask, avail_mask,
                                        ctypes.byref(out)),
            "ecx_minimum_to_decode")
        return out.value

    # ---- device-resident batch API ----
    def dbuf_alloc(self, nbytes):
        p = ctypes.c_void_p()
        _ck(lib().ecx_dbuf_alloc(self._h, nbytes, ctypes.byref(p)),
            "ecx_dbuf_alloc")
        return p

    def dbuf_free(self, dptr):
        _ck(lib().ecx_dbuf_free(self._h, dptr), "ecx_dbuf_free")

    def upload(self, dptr, arr, slot=0, blocking=True):
        _ck(lib().ecx_upload(self._h, dptr,
                             arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes,
                             slot, int(blocking)), "ecx_upload")

    def download(self, arr, dptr, slot=0, blocking=True):
        _ck(lib().ecx_download(self._h,
                               arr.ctypes.data_as(ctypes.c_void_p), dptr,
                               arr.nbytes, slot, int(blocking)),
            "ecx_download")

    def fill_random(self, dptr, nbytes, seed, slot=0):
        _ck(lib().ecx_dbuf_fill_random(self._h, dptr, nbytes, seed, slot),
            "ecx_dbuf_fill_random")

    def encode_batch(self, dptr, n_stripes, chunk_bytes, slot=0):
        _ck(lib().ecx_encode_batch(self._h, dptr, n_stripes, chunk_bytes,
                                   slot), "ecx_encode_batch")

    def decode_batch(self, dptr, n_stripes, chunk_bytes, present_mask, slot=0):
        _ck(lib().ecx_decode_batch(self._h, dptr, n_stripes, chunk_bytes,
                                   present_mask, slot), "ecx_decode_batch")

    def _slice_args(self, chunk_ptrs, sizes):
        n = len(sizes)
        assert len(chunk_ptrs) == n * (self.k + self.m)
        arr = (ctypes.c_void_p * len(chunk_ptrs))()
        for i, p in enumerate(chunk_ptrs):
            arr[i] = None if p in (None, 0) else int(p)
        sz = (ctypes.c_size_t * n)(*sizes)
        return arr, sz, n

    def encode_slices(self, chunk_ptrs, sizes, slot=0):
        """Variable-size slice batch: chunk_ptrs is a flat list
        of n*(k+m) device addresses, multiples of 16 (None => zeros data
        chunk; a parity address must not be None); sizes is the per-slice
        byte length (multiples of 16). One kernel launch per <= 4 parity
        chunks. A refused call (EINVAL) has launched nothing."""
        arr, sz, n = self._slice_args(chunk_ptrs, sizes)
        _ck(lib().ecx_encode_slices(self._h, arr, sz, n, slot),
            "ecx_encode_slices")

    def decode_slices(self, chunk_ptrs, sizes, present_mask, slot=0):
        """encode_slices' counterpart under one present mask for the call:
        the absent chunks of every slice are written (their addresses must
        not be None); a present chunk may be None (zeros)."""
        arr, sz, n = self._slice_args(chunk_ptrs, sizes)
        _ck(lib().ecx_decode_slices(self._h, arr, sz, n, present_mask,
                                    slot), "ecx_decode_slices")

    def decode_batch_multi(self, dptr, n_stripes, chunk_bytes, present_masks,
                           slot=0):
        """decode_batch with one present mask PER STRIPE (recovery batches
        whose neighbouring stripes miss different chunks). Launch count is
        independent of the number of distinct masks, at most m."""
        a = _mask_array(present_masks, n_stripes, "ecx_decode_batch_multi")
        _ck(lib().ecx_decode_batch_multi(self._h, dptr, n_stripes,
                                         chunk_bytes, _u64p(a), slot),
            "ecx_decode_batch_multi")

    def decode_slices_multi(self, chunk_ptrs, sizes, present_masks, slot=0):
        """decode_slices with one present mask per slice."""
        if len(chunk_ptrs) != len(sizes) * (self.k + self.m):
            raise EcError(f"ecx_decode_slices_multi: {len(sizes)} slices "
                          f"need {len(sizes) * (self.k + self.m)} chunk "
                          f"pointers, got {len(chunk_ptrs)}")
        a = _mask_array(present_masks, len(sizes), "ecx_decode_slices_multi")
        arr, sz, n = self._slice_args(chunk_ptrs, sizes)
        _ck(lib().ecx_decode_slices_multi(self._h, arr, sz, n, _u64p(a),
                                          slot), "ecx_decode_slices_multi")

    def update_batch(self, dptr, n_stripes, chunk_bytes, d_new, write_masks,
                     slot=0):
        """Parity-delta write over a batch: write_masks[s] bit j = data
        chunk j of stripe s is replaced by its new content from the packed
        device buffer d_new (stripe ascending, then chunk id ascending);
        every parity of a touched stripe is corrected in place. ceil(m/4)
        launches whatever the masks are."""
        a = _mask_array(write_masks, n_stripes, "ecx_update_batch")
        _ck(lib().ecx_update_batch(self._h, dptr, n_stripes, chunk_bytes,
                                   d_new, _u64p(a), slot), "ecx_update_batch")

    def verify_batch(self, dptr, n_stripes, chunk_bytes, present_mask=None,
                     d_bad=None, slot=0):
        """Consistency check of a batch: the first k present chunks of each
        stripe vouch for every further present one. Returns a uint64 array
        of n_stripes words, bit i of word s set when checked chunk i of
        stripe s differs from its recomputed value. present_mask None = all
        k+m chunks; d_bad None = a temporary device array of n_stripes
        words. The batch is only read."""
        if present_mask is None:
            present_mask = (1 << (self.k + self.m)) - 1
        words = np.zeros(max(int(n_stripes), 0), dtype=np.uint64)
        own = d_bad is None
        if own:
            d_bad = self.dbuf_alloc(max(words.nbytes, 8))
        try:
            _ck(lib().ecx_verify_batch(self._h, dptr, n_stripes, chunk_bytes,
                                       present_mask, d_bad, slot),
                "ecx_verify_batch")
            self.download(words, d_bad, slot)
        finally:
            if own:
                self.dbuf_free(d_bad)
        return words

    def _locate_call(self, n_stripes, present_mask, d_bad, d_culprit, slot,
                     call):
        """Shared by locate_batch and repair_batch: default mask, temporary
        device arrays where none are given, call(mask, d_bad, d_culprit),
        then both arrays downloaded."""
        if present_mask is None:
            present_mask = (1 << (self.k + self.m)) - 1
        n = max(int(n_stripes), 0)
        bad = np.zeros(n, dtype=np.uint64)
        culprit = np.zeros(n, dtype=np.uint64)
        temps = []
        try:
            if d_bad is None:
                d_bad = self.dbuf_alloc(max(bad.nbytes, 8))
                temps.append(d_bad)
            if d_culprit is None:
                d_culprit = self.dbuf_alloc(max(culprit.nbytes, 8))
                temps.append(d_culprit)
            out = call(present_mask, d_bad, d_culprit)
            self.download(bad, d_bad, slot)
            self.download(culprit, d_culprit, slot)
        finally:
            for p in temps:
                self.dbuf_free(p)
        return bad, culprit, out

    def locate_batch(self, dptr, n_stripes, chunk_bytes, present_mask=None,
                     d_bad=None, d_culprit=None, slot=0):
        """verify_batch plus the culprit: returns (bad, culprit), two uint64
        arrays of n_stripes words. bad is verify_batch's result; bit x of
        culprit[s] is set when leaving present chunk x out makes the rest of
        stripe s consistent. Clean stripe: culprit == present_mask; one
        damaged chunk x: 1 << x; not locatable: 0. Needs at least k + 2
        present chunks. The batch is only read."""
        def call(mask, db, dc):
            _ck(lib().ecx_locate_batch(self._h, dptr, n_stripes, chunk_bytes,
                                       mask, db, dc, slot),
                "ecx_locate_batch")
        return self._locate_call(n_stripes, present_mask, d_bad, d_culprit,
                                 slot, call)[:2]

    def repair_batch(self, dptr, n_stripes, chunk_bytes, present_mask=None,
                     d_bad=None, d_culprit=None, slot=0):
        """locate_batch, then every stripe whose culprit is a single chunk
        gets that chunk (and its absent chunks) rebuilt in place; all other
        stripes are not written. Returns (bad, culprit, n_repaired,
        n_unlocatable) — the words describe the batch before the repair."""
        def call(mask, db, dc):
            rep, unl = ctypes.c_long(), ctypes.c_long()
            _ck(lib().ecx_repair_batch(self._h, dptr, n_stripes, chunk_bytes,
                                       mask, db, dc, ctypes.byref(rep),
                                       ctypes.byref(unl), slot),
                "ecx_repair_batch")
            return rep.value, unl.value
        bad, culprit, (rep, unl) = self._locate_call(
            n_stripes, present_mask, d_bad, d_culprit, slot, call)
        return bad, culprit, rep, unl

    def crc32c_batch(self, dptr, n_stripes, chunk_bytes, chunk_mask=None,
                     seeds=None, chain=False, d_crc=None, slot=0):
        """ceph_crc32c of every chunk of a batch in chunk_mask (None = all
        k+m), as an (n_stripes, k+m) uint32 array. seeds: None (0xFFFFFFFF),
        a numpy array uploaded for the call, or a device pointer — one word
        per output word, or k+m words when chain. chain=True: row s is the
        hash of each shard's chunks of stripes 0..s concatenated. d_crc None
        = a temporary zeroed device array (unmasked columns come back 0);
        otherwise a device array of n_stripes*(k+m) words, whose unmasked
        words are kept. The batch is only read."""
        n = self.k + self.m
        if chunk_mask is None:
            chunk_mask = (1 << n) - 1
        words = np.zeros((max(int(n_stripes), 0), n), dtype=np.uint32)
        temps = []
        try:
            if d_crc is None:
                d_crc = self.dbuf_alloc(max(words.nbytes, 4))
                temps.append(d_crc)
                self.upload(d_crc, words, slot)
            if isinstance(seeds, np.ndarray):
                want = n if chain else words.size
                h = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
                if h.size != want:
                    raise EcError(f"ecx_crc32c_batch: need {want} seeds, "
                                  f"got {h.size}")
                seeds = self.dbuf_alloc(max(h.nbytes, 4))
                temps.append(seeds)
                self.upload(seeds, h, slot)
            _ck(lib().ecx_crc32c_batch(self._h, dptr, n_stripes, chunk_bytes,
                                       chunk_mask, seeds, int(bool(chain)),
                                       d_crc, slot), "ecx_crc32c_batch")
            self.download(words, d_crc, slot)
        finally:
            for p in temps:
                self.dbuf_free(p)
        return words

    def matmul_batch(self, dptr, n_stripes, chunk_bytes, src_ids, out_ids,
                     rows, slot=0):
        """Generic device-batch GF matmul over chunk ids (LRC layer
        composition primitive)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.shape == (len(out_ids), len(src_ids))
        sa = (ctypes.c_int * len(src_ids))(*src_ids)
        oa = (ctypes.c_int * len(out_ids))(*out_ids)
        _ck(lib().ecx_matmul_batch(self._h, dptr, n_stripes, chunk_bytes,
                                   sa, len(src_ids), oa, len(out_ids),
                                   rows.ctypes.data_as(ctypes.c_void_p),
                                   slot), "ecx_matmul_batch")

    def set_matrix(self, coding_rows):
        """Replace the coding rows (custom-matrix codecs, e.g. SHEC)."""
        rows = np.ascontiguousarray(coding_rows, dtype=np.uint8)
        assert rows.shape == (self.m, self.k)
        _ck(lib().ecx_set_matrix(self._h,
                                 rows.ctypes.data_as(ctypes.c_void_p)),
            "ecx_set_matrix")

    def sync(self, slot=0):
        _ck(lib().ecx_sync(self._h, slot), "ecx_sync")

    def last_kernel_ms(self, slot=0):
        ms = ctypes.c_double()
        _ck(lib().ecx_last_kernel_ms(self._h, slot, ctypes.byref(ms)),
            "ecx_last_kernel_ms")
        return ms.value

    # ---- host-pointer (plugin) path ----
    def encode_chunks(self, data, chunk_bytes=None, out=None):
        """data: list of k uint8 arrays (None => zeros chunk). Returns m
        parity arrays. Mirrors encode_chunks marshalling
        (ErasureCodeJerasure.cc:121-164)."""
        sizes = {d.nbytes for d in data if d is not None}
        if chunk_bytes is not None:
            sizes.add(chunk_bytes)
        assert len(sizes) == 1, "equal-length chunks required (pass " \
            "chunk_bytes when every chunk is a zeros sentinel)"
        n = sizes.pop()
        if out is None:
            out = [np.zeros(n, dtype=np.uint8) for _ in range(self.m)]
        _ck(lib().ecx_encode_chunks_host(self._h, _ptr_array(data),
                                         _ptr_array(out), n),
            "ecx_encode_chunks_host")
        return out

    def decode_chunks(self, chunks, present):
        """chunks: list of k+m uint8 arrays; erased entries (present[i]
        false) are filled in place. Mirrors decode_chunks
        (ErasureCodeIsa.cc:167-243)."""
        n = chunks[0].nbytes
        mask = 0
        for i, p in enumerate(present):
            if p:
                mask |= 1 << i
        _ck(lib().ecx_decode_chunks_host(self._h, _ptr_array(chunks), mask, n),
            "ecx_decode_chunks_host")
        return chunks

    def verify_chunks(self, chunks, present=None):
        """chunks: list of k+m uint8 arrays of one stripe (entries of absent
        ids are ignored and may be None). Returns the stripe's word as an
        int: bit i set when checked chunk i differs from its value
        recomputed from the first k present chunks. A present entry that is
        None raises EINVAL."""
        if present is None:
            present = [True] * (self.k + self.m)
        mask = 0
        for i, p in enumerate(present):
            if p:
                mask |= 1 << i
        sizes = {c.nbytes for c, p in zip(chunks, present)
                 if p and c is not None}
        if len(sizes) > 1:
            raise EcError("ecx_verify_chunks_host: equal-length chunks "
                          f"required, got sizes {sorted(sizes)}")
        word = ctypes.c_uint64()
        _ck(lib().ecx_verify_chunks_host(
            self._h, _ptr_array(list(chunks)), mask,
            sizes.pop() if sizes else 0, ctypes.byref(word)),
            "ecx_verify_chunks_host")
        return word.value

    def locate_chunks(self, chunks, present=None):
        """locate_batch for one stripe in host memory, arguments as
        verify_chunks. Returns (bad, culprit) as ints."""
        if present is None:
            present = [True] * (self.k + self.m)
        mask = 0
        for i, p in enumerate(present):
            if p:
                mask |= 1 << i
        sizes = {c.nbytes for c, p in zip(chunks, present)
                 if p and c is not None}
        if len(sizes) > 1:
            raise EcError("ecx_locate_chunks_host: equal-length chunks "
                          f"required, got sizes {sorted(sizes)}")
        bad, culprit = ctypes.c_uint64(), ctypes.c_uint64()
        _ck(lib().ecx_locate_chunks_host(
            self._h, _ptr_array(list(chunks)), mask,
            sizes.pop() if sizes else 0, ctypes.byref(bad),
            ctypes.byref(culprit)), "ecx_locate_chunks_host")
        return bad.value, culprit.value

    def encode_delta(self, old, new):
        delta = np.zeros_like(old)
        _ck(lib().ecx_encode_delta_host(
            self._h, old.ctypes.data_as(ctypes.c_void_p),
            new.ctypes.data_as(ctypes.c_void_p),
            delta.ctypes.data_as(ctypes.c_void_p), old.nbytes),
            "ecx_encode_delta_host")
        return delta

    def apply_delta(self, delta, data_shard, coding_shard, parity):
        _ck(lib().ecx_apply_delta_host(
            self._h, delta.ctypes.data_as(ctypes.c_void_p), data_shard,
            coding_shard, parity.ctypes.data_as(ctypes.c_void_p),
            delta.nbytes), "ecx_apply_delta_host")
        return parity

    def apply_deltas(self, deltas, parities):
        """Fused apply_delta: deltas {data shard id: uint8 array}, parities
        {coding shard id: uint8 array}. Every parity is corrected in place
        by every delta in one staged call; returns parities."""
        ds, cs = sorted(deltas), sorted(parities)
        sizes = {a.nbytes for a in deltas.values()} | \
                {a.nbytes for a in parities.values()}
        if len(sizes) > 1:
            raise EcError("ecx_apply_deltas_host: equal-length buffers "
                          f"required, got sizes {sorted(sizes)}")
        _ck(lib().ecx_apply_deltas_host(
            self._h, _ptr_array([deltas[i] for i in ds]),
            (ctypes.c_int * len(ds))(*ds), len(ds),
            _ptr_array([parities[j] for j in cs]),
            (ctypes.c_int * len(cs))(*cs), len(cs),
            sizes.pop() if sizes else 0), "ecx_apply_deltas_host")
        return parities
