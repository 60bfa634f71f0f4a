"""GPU tests for decode with a different erasure pattern per stripe
(ecx_decode_batch_multi / ecx_decode_slices_multi).

Reference: oracle.cpu_encode_batch on the host copy. On the device every
erased chunk is overwritten with 0xA5 bytes (not zeros), so a kernel that
reads an erased chunk or skips a write is caught; the assertion is
whole-buffer equality after download, which also catches stray writes into
present chunks and other stripes. Mask sets come from decode_multi_cases.py
and are proven decodable on the CPU in test_decode_multi_plan.py."""
import ctypes
import functools

import numpy as np
import pytest

import ceph_amd
import oracle
import decode_multi_cases as cases

pytestmark = pytest.mark.gpu

POISON = 0xA5


@functools.lru_cache(maxsize=None)
def reference(tech, k, m, n_stripes, chunk_bytes, seed):
    """Encoded host batch (n_stripes, k+m, chunk_bytes), read-only."""
    n = k + m
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, n_stripes * n * chunk_bytes, dtype=np.uint8)
    oracle.cpu_encode_batch(tech, k, m, buf, n_stripes, chunk_bytes)
    buf = buf.reshape(n_stripes, n, chunk_bytes)
    buf.flags.writeable = False
    return buf


def poisoned(ref, masks):
    n = ref.shape[1]
    dev = ref.copy()
    for s, mk in enumerate(masks):
        for c in cases.erased_of(n, mk):
            dev[s, c, :] = POISON
    return dev


def run_batch_multi(tech, k, m, chunk_bytes, masks, seed=0xEC):
    ref = reference(tech, k, m, len(masks), chunk_bytes, seed)
    dev = poisoned(ref, masks)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = ctx.dbuf_alloc(dev.nbytes)
        ctx.upload(d, dev)
        ctx.decode_batch_multi(d, len(masks), chunk_bytes, masks)
        ctx.sync()
        out = np.empty_like(dev)
        ctx.download(out, d)
        ctx.dbuf_free(d)
    finally:
        ctx.close()
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("chunk_bytes", [16, 4112])
@pytest.mark.parametrize("tech", cases.MATRIX_TECHS)
def test_all_patterns_small_chunks(tech, chunk_bytes):
    # 16 = a single vector; 4112 = 257 vectors, one past a 256-thread block
    run_batch_multi(tech, 4, 3, chunk_bytes, cases.all_patterns_43())


def test_mid_size_chunks():
    run_batch_multi("reed_sol_van", 8, 3, 64 * 1024, cases.mid_83())


def test_extra_passes():
    # 5 and 6 erasures: a second <= 4-output pass over the same stripes
    run_batch_multi("cauchy", 4, 6, 4112, cases.extra_passes_46())


def test_grid_stride_and_tail():
    # > 2048 stripes in one bucket: grid x stays narrow, so each block
    # takes two grid-stride steps, the second a one-vector tail
    run_batch_multi("reed_sol_van", 2, 1, 8208, cases.long_bucket_21())


def test_equivalent_to_per_stripe_decode_batch():
    tech, k, m, C = "reed_sol_van", 8, 3, 64 * 1024
    masks = cases.mid_83()
    S, n = len(masks), k + m
    dev = poisoned(reference(tech, k, m, S, C, 0xEC), masks)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d1 = ctx.dbuf_alloc(dev.nbytes)
        d2 = ctx.dbuf_alloc(dev.nbytes)
        ctx.upload(d1, dev)
        ctx.upload(d2, dev)
        ctx.decode_batch_multi(d1, S, C, masks)
        for s, mk in enumerate(masks):
            ctx.decode_batch(ctypes.c_void_p(d2.value + s * n * C), 1, C, mk)
        ctx.sync()
        out1, out2 = np.empty_like(dev), np.empty_like(dev)
        ctx.download(out1, d1)
        ctx.download(out2, d2)
        ctx.dbuf_free(d1)
        ctx.dbuf_free(d2)
    finally:
        ctx.close()
    assert np.array_equal(out1, out2)


def test_slices_multi():
    tech, k, m = "reed_sol_van", 4, 2
    n = k + m
    sizes, masks = cases.slices_42()
    rng = np.random.default_rng(0x51)
    offs, off = [], 0
    for sz in sizes:
        offs.append(off)
        off += sz * n
    ref = rng.integers(0, 256, off, dtype=np.uint8)
    z = offs[cases.SLICE_NULL] + cases.SLICE_NULL_CHUNK * sizes[cases.SLICE_NULL]
    ref[z:z + sizes[cases.SLICE_NULL]] = 0  # the NULL chunk's true content
    for o, sz in zip(offs, sizes):
        oracle.cpu_encode_batch(tech, k, m, ref[o:o + sz * n], 1, sz)
    dev = ref.copy()
    for o, sz, mk in zip(offs, sizes, masks):
        for c in cases.erased_of(n, mk):
            dev[o + c * sz:o + (c + 1) * sz] = POISON
    # the device copy of the NULL chunk is poisoned too: it must not be read
    dev[z:z + sizes[cases.SLICE_NULL]] = POISON
    want = ref.copy()
    want[z:z + sizes[cases.SLICE_NULL]] = POISON

    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = ctx.dbuf_alloc(dev.nbytes)
        ctx.upload(d, dev)
        ptrs = [d.value + o + c * sz
                for o, sz in zip(offs, sizes) for c in range(n)]
        ptrs[cases.SLICE_NULL * n + cases.SLICE_NULL_CHUNK] = None
        ctx.decode_slices_multi(ptrs, sizes, masks)
        ctx.sync()
        assert ctx.last_kernel_ms() > 0
        out = np.empty_like(dev)
        ctx.download(out, d)

        # an erased chunk with no buffer is refused before any launch
        ctx.upload(d, dev)
        bad = list(ptrs)
        bad[cases.SLICE_NULL * n + 1] = None  # chunk 1 is erased there
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.decode_slices_multi(bad, sizes, masks)
        ctx.sync()
        after = np.empty_like(dev)
        ctx.download(after, d)
        ctx.dbuf_free(d)
    finally:
        ctx.close()
    assert np.array_equal(out, want)
    assert np.array_equal(after, dev)


def test_loud_failures():
    tech, k, m, C = "reed_sol_van", 4, 3, 4112
    masks = cases.all_patterns_43()
    dev = poisoned(reference(tech, k, m, len(masks), C, 0xEC), masks)
    bad = list(masks)
    bad[40] = cases.mask_without(7, [0, 2, 4, 6])  # 3 present < k
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = ctx.dbuf_alloc(dev.nbytes)
        ctx.upload(d, dev)
        with pytest.raises(ceph_amd.EcError, match="EIO"):
            ctx.decode_batch_multi(d, len(bad), C, bad)
        assert ceph_amd.lib().ecx_decode_batch_multi(
            ctx._h, d, len(bad), C,
            (ctypes.c_uint64 * len(bad))(*bad), 0) == -5
        for args in [(d, len(masks), C + 8, masks),      # chunk_bytes % 16
                     (d, 0, C, []),                      # n_stripes range
                     (d, 65536, 16, [0x7f] * 65536),
                     (None, len(masks), C, masks)]:      # NULL buffer
            with pytest.raises(ceph_amd.EcError, match="EINVAL"):
                ctx.decode_batch_multi(*args)
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.decode_batch_multi(d, len(masks), C, masks, slot=9)
        ctx.sync()
        out = np.empty_like(dev)
        ctx.download(out, d)
        ctx.dbuf_free(d)
    finally:
        ctx.close()
    assert np.array_equal(out, dev)  # nothing was launched

    for tech, cb in (("cauchy_orig", 8 * 2048),
                     ("jerasure_reed_sol_van_w16", 4096)):
        ctx = ceph_amd.EcContext(4, 2, tech, device=0)
        try:
            d = ctx.dbuf_alloc(6 * cb)
            with pytest.raises(ceph_amd.EcError, match="EINVAL"):
                ctx.decode_batch_multi(d, 1, cb, [0x3e])
            with pytest.raises(ceph_amd.EcError, match="EINVAL"):
                ctx.decode_slices_multi([d.value + c * cb for c in range(6)],
                                        [cb], [0x3e])
            ctx.dbuf_free(d)
        finally:
            ctx.close()


def test_timing_and_all_full_masks():
    tech, k, m, C = "reed_sol_van", 4, 3, 4112
    masks = cases.all_patterns_43()
    ref = reference(tech, k, m, len(masks), C, 0xEC)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = ctx.dbuf_alloc(ref.nbytes)
        # all masks full: OK, nothing touched (the buffer holds poison)
        junk = np.full_like(ref, POISON)
        ctx.upload(d, junk)
        ctx.decode_batch_multi(d, len(masks), C, [0x7f] * len(masks))
        ctx.sync()
        out = np.empty_like(junk)
        ctx.download(out, d)
        assert np.array_equal(out, junk)
        # one event pair spans the call's launches
        ctx.upload(d, poisoned(ref, masks))
        ctx.decode_batch_multi(d, len(masks), C,
                               np.array(masks, dtype=np.uint64))
        ctx.sync()
        assert ctx.last_kernel_ms() > 0
        ctx.download(out, d)
        assert np.array_equal(out, ref)
        ctx.dbuf_free(d)
    finally:
        ctx.close()
