"""GPU tests for the variable-size slice batch API (the OSD
write path's many small variable-blocksize encode_chunks calls,
shard_extent_map_t::encode, src/osd/ECUtil.cc:485-514 — batched here into
one launch)."""
import ctypes

import numpy as np
import pytest

import ceph_amd
import oracle
import slices_cases as cases
import test_gpu_stream_kernel as t

pytestmark = pytest.mark.gpu


def carve(base, off, n):
    return ctypes.c_void_p(base.value + off)


def test_encode_slices_vs_oracle():
    k, m, tech = 8, 3, "reed_sol_van"
    n = k + m
    sizes = [4096, 64 * 1024, 1 << 20, 16 * 31, 4096 + 16]
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        total = sum(sizes) * n
        d = ctx.dbuf_alloc(total)
        ctx.fill_random(d, total, 0xEC)
        ctx.sync()

        ptrs, offs = [], []
        off = 0
        for sz in sizes:
            offs.append(off)
            for c in range(n):
                ptrs.append(d.value + off + c * sz)
            off += sz * n

        ctx.encode_slices(ptrs, sizes)
        ctx.sync()

        import bench
        for si, sz in enumerate(sizes):
            host = np.zeros(sz * n, dtype=np.uint8)
            ctx.download(host, carve(d, offs[si], 0))
            data = [host[i * sz:(i + 1) * sz] for i in range(k)]
            # data region must equal the deterministic fill
            exp = bench.expected_fill(offs[si], k * sz, 0xEC)
            assert np.array_equal(host[:k * sz], exp), si
            want = oracle.encode(tech, k, m, data)
            for j in range(m):
                got = host[(k + j) * sz:(k + j + 1) * sz]
                assert np.array_equal(got, want[j]), (si, j)
    finally:
        ctx.close()


def test_encode_slices_null_data_is_zeros():
    k, m = 4, 2
    n = k + m
    sz = 8192
    ctx = ceph_amd.EcContext(k, m, "reed_sol_van", device=0)
    try:
        d = ctx.dbuf_alloc(sz * n)
        ctx.fill_random(d, sz * n, 7)
        ctx.sync()
        ptrs = [d.value + c * sz for c in range(n)]
        ptrs[2] = None  # zeros chunk
        ctx.encode_slices(ptrs, [sz])
        ctx.sync()
        host = np.zeros(sz * n, dtype=np.uint8)
        ctx.download(host, d)
        data = [host[i * sz:(i + 1) * sz] for i in range(k)]
        data[2] = None
        want = oracle.encode("reed_sol_van", k, m, data, chunk_bytes=sz)
        for j in range(m):
            assert np.array_equal(host[(k + j) * sz:(k + j + 1) * sz],
                                  want[j]), j
    finally:
        ctx.close()


def test_decode_slices_round_trip():
    k, m, tech = 6, 3, "cauchy"
    n = k + m
    sizes = [16 * 1024, 4096, 256 * 1024]
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        total = sum(sizes) * n
        d = ctx.dbuf_alloc(total)
        ctx.fill_random(d, total, 0xD)
        ctx.sync()
        ptrs = []
        off = 0
        offs = []
        for sz in sizes:
            offs.append(off)
            for c in range(n):
                ptrs.append(d.value + off + c * sz)
            off += sz * n
        ctx.encode_slices(ptrs, sizes)
        ctx.sync()
        ref = np.zeros(total, dtype=np.uint8)
        ctx.download(ref, d)

        # erase chunks 1, 7, 8 in every slice (zero the regions)
        erased = [1, 7, 8]
        mask = (1 << n) - 1
        for e in erased:
            mask &= ~(1 << e)
        for si, sz in enumerate(sizes):
            z = np.zeros(sz, dtype=np.uint8)
            for e in erased:
                ctx.upload(ctypes.c_void_p(d.value + offs[si] + e * sz), z)
        ctx.decode_slices(ptrs, sizes, mask)
        ctx.sync()
        out = np.zeros(total, dtype=np.uint8)
        ctx.download(out, d)
        assert np.array_equal(out, ref)
    finally:
        ctx.close()


def test_slices_reject_bad_sizes():
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0)
    try:
        d = ctx.dbuf_alloc(4096)
        ptrs = [d.value] * 6
        with pytest.raises(ceph_amd.EcError):
            ctx.encode_slices(ptrs, [24])  # not a multiple of 16
    finally:
        ctx.close()


# ---- scattered arenas against the host model (slices_cases.py) ----
# Every comparison below is the whole arena, bit-exact: the bytes between the
# chunks, the sources and the outputs at once. test_slices_cases.py shows on
# the CPU that these inputs tell a wrong kernel from a right one.


class OnDev:
    """An arena's image on the device, and its chunk pointers."""

    def __init__(self, ctx, arena, image):
        self.arena = arena
        self.dev = t.Dev(ctx, image)
        self.base = self.dev.d.value
        self.ptrs = arena.ptrs(self.base)

    def put(self, image):
        self.dev.ctx.upload(self.dev.d, np.ascontiguousarray(image))

    def get(self):
        return self.dev.get((self.arena.nbytes,))

    def free(self):
        self.dev.free()


def same(got, want, what=None):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first differing byte", int(bad[0]),
                           "of", int(bad.size))


@pytest.mark.parametrize("k,m,tech", cases.ENCODE_CODES)
def test_encode_every_output_count(k, m, tech):
    """1, 2, 3, 4 outputs in one launch, and 4+1, 4+2, 4+4 in two."""
    arena, want = cases.encode_case(k, m, tech)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = OnDev(ctx, arena, cases.encode_image(arena, k))
        ctx.encode_slices(d.ptrs, arena.sizes)
        ctx.sync()
        same(d.get(), want)
        d.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["custom", "shec"])
def test_encode_coefficient_classes(which):
    """Coding rows with zeros and ones; an all-zero row's output is written
    (zeros), not left as it was."""
    rows = cases.CLASS_ROWS if which == "custom" else \
        ceph_amd.shec_matrix(4, 3, 2)
    arena, want = cases.class_case(rows)
    ctx = ceph_amd.EcContext(4, 3, "reed_sol_van", device=0)
    try:
        ctx.set_matrix(rows)
        d = OnDev(ctx, arena, cases.encode_image(arena, 4))
        ctx.encode_slices(d.ptrs, arena.sizes)
        ctx.sync()
        got = d.get()
        d.free()
    finally:
        ctx.close()
    same(got, want)
    if which == "custom":
        for s in range(arena.n):
            assert not arena.chunk(got, s, 4 + cases.CLASS_ZERO_ROW).any()


def test_encode_null_data_differs_per_slice():
    arena, want = cases.null_case()
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0)
    try:
        d = OnDev(ctx, arena, cases.encode_image(arena, 4))
        assert d.ptrs.count(None) == sum(len(s) for s in cases.NULL_SETS)
        ctx.encode_slices(d.ptrs, arena.sizes)
        ctx.sync()
        got = d.get()
        d.free()
    finally:
        ctx.close()
    same(got, want)
    for c in (4, 5):  # every data chunk NULL: parity zeros
        assert not arena.chunk(got, cases.NULL_ALL, c).any()


def test_encode_shared_sources():
    arena, want = cases.shared_case()
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0)
    try:
        d = OnDev(ctx, arena, cases.encode_image(arena, 4))
        assert d.ptrs[:4] == d.ptrs[6:10]
        ctx.encode_slices(d.ptrs, arena.sizes)
        ctx.sync()
        same(d.get(), want)
        d.free()
    finally:
        ctx.close()


def check_decode_masks(k, m, tech, arena, truth, masks):
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = OnDev(ctx, arena, truth)
        for mk in masks:
            d.put(cases.erase(arena, truth, [mk] * arena.n))
            ctx.decode_slices(d.ptrs, arena.sizes, mk)
            ctx.sync()
            same(d.get(), truth, hex(mk))
        d.free()
    finally:
        ctx.close()


def test_decode_slices_every_mask_42():
    arena, truth = cases.decode_42_case()
    check_decode_masks(4, 2, "reed_sol_van", arena, truth,
                       cases.DECODE_42_MASKS)


def test_decode_slices_second_launch_46():
    """5 and 6 chunks lost: a second launch of 1 and of 2 outputs."""
    arena, truth = cases.decode_46_case()
    check_decode_masks(4, 6, "cauchy", arena, truth, cases.DECODE_46_MASKS)


def test_decode_slices_null_survivor_in_some_slices():
    arena, truth = cases.decode_null_case()
    check_decode_masks(4, 2, "reed_sol_van", arena, truth,
                       [cases.DECODE_NULL_MASK])


def test_decode_slices_multi_46_and_slice_by_slice():
    arena, truth, masks = cases.multi_case()
    n = arena.cps
    image = cases.erase(arena, truth, masks)
    ctx = ceph_amd.EcContext(4, 6, "cauchy", device=0)
    try:
        d = OnDev(ctx, arena, image)
        ctx.decode_slices_multi(d.ptrs, arena.sizes, masks)
        ctx.sync()
        assert ctx.last_kernel_ms() > 0
        first = d.get()
        same(first, truth, "multi")
        # the same arena again, one decode_slices call per slice
        d.put(image)
        for s, mk in enumerate(masks):
            ctx.decode_slices(d.ptrs[s * n:(s + 1) * n], [arena.sizes[s]], mk)
        ctx.sync()
        same(d.get(), first, "slice by slice")
        d.free()
    finally:
        ctx.close()


def test_job_blob_grows_while_earlier_calls_run():
    """Three calls on one slot with no sync between; the second needs a far
    larger job table than the first left behind."""
    runs = cases.growth_cases()
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0)
    try:
        devs = [OnDev(ctx, a, cases.encode_image(a, 4)) for a, _ in runs]
        for d in devs:
            ctx.encode_slices(d.ptrs, d.arena.sizes)
        ctx.sync()
        for i, (d, (_, want)) in enumerate(zip(devs, runs)):
            same(d.get(), want, i)
            d.free()
    finally:
        ctx.close()


def test_two_slots_interleaved():
    runs = cases.slot_cases()
    poison = np.full(max(cases.EDGE_SIZES), cases.POISON, dtype=np.uint8)
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0, n_streams=2)
    try:
        devs = [OnDev(ctx, a, cases.encode_image(a, 4)) for a, _ in runs]
        for slot, d in enumerate(devs):
            ctx.encode_slices(d.ptrs, d.arena.sizes, slot=slot)
        for slot, d in enumerate(devs):
            for s, mk in enumerate(cases.SLOT_MASKS[slot]):
                for c in cases.erased_of(6, mk):
                    ctx.upload(ctypes.c_void_p(d.ptrs[s * 6 + c]),
                               poison[:d.arena.sizes[s]], slot=slot,
                               blocking=False)
        for slot, d in enumerate(devs):
            ctx.decode_slices_multi(d.ptrs, d.arena.sizes,
                                    cases.SLOT_MASKS[slot], slot=slot)
        for slot in range(2):
            ctx.sync(slot)
        for slot, (d, (_, truth)) in enumerate(zip(devs, runs)):
            same(d.get(), truth, slot)
            d.free()
    finally:
        ctx.close()


# ---- refusals: the arena stays as it was, the next call is right ----

EINVAL, EIO = "EINVAL", "EIO"


class Refusals:
    """(4,2) over the decode_42 arena, parity pre-poisoned. refuse(call,
    err): the call raises err, the arena is byte for byte what it was, and
    a valid encode on the same slot then gives the model's arena."""

    def __init__(self):
        self.arena, self.want = cases.decode_42_case()
        self.image = cases.encode_image(self.arena, 4)
        self.ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0,
                                      n_streams=2)
        self.d = OnDev(self.ctx, self.arena, self.image)
        self.sizes = list(self.arena.sizes)

    def refuse(self, call, err, slot=0):
        with pytest.raises(ceph_amd.EcError, match=err):
            call()
        self.ctx.sync(slot)
        same(self.d.get(), self.image, "a refused call wrote")
        self.ctx.encode_slices(self.d.ptrs, self.sizes, slot=slot)
        self.ctx.sync(slot)
        same(self.d.get(), self.want, "the call after a refusal")
        self.d.put(self.image)

    def close(self):
        self.d.free()
        self.ctx.close()


def test_refusals_leave_the_arena_alone():
    r = Refusals()
    ctx, ptrs, sizes = r.ctx, r.d.ptrs, r.sizes
    full, one_lost = 0x3F, cases.mask_without(6, [1])
    try:
        for bad in (0, 24):
            for at in range(3):
                sz = list(sizes)
                sz[at] = bad
                r.refuse(lambda: ctx.encode_slices(ptrs, sz), EINVAL)
                r.refuse(lambda: ctx.decode_slices(ptrs, sz, one_lost), EINVAL)
                # a full mask with a bad size: refused, not "nothing to do"
                r.refuse(lambda: ctx.decode_slices(ptrs, sz, full), EINVAL)
                r.refuse(lambda: ctx.decode_slices_multi(
                    ptrs, sz, [one_lost, full, full]), EINVAL)
        # n_slices 0 (the wrapper passes the length of the size list)
        r.refuse(lambda: ctx.encode_slices([], []), EINVAL)
        r.refuse(lambda: ctx.decode_slices([], [], one_lost), EINVAL)
        r.refuse(lambda: ctx.decode_slices([], [], full), EINVAL)
        for slot in (-1, 2, 1 << 20):
            r.refuse(lambda: ctx.encode_slices(ptrs, sizes, slot=slot), EINVAL)
            r.refuse(lambda: ctx.decode_slices(ptrs, sizes, one_lost,
                                               slot=slot), EINVAL)
            r.refuse(lambda: ctx.decode_slices(ptrs, sizes, full, slot=slot),
                     EINVAL)
            r.refuse(lambda: ctx.decode_slices_multi(
                ptrs, sizes, [one_lost] * 3, slot=slot), EINVAL)
        # the other slot is as good as the first after all that
        r.refuse(lambda: ctx.encode_slices(ptrs, [16, 24, 16]), EINVAL, slot=1)
        # undecodable: three chunks present of k = 4
        gone = cases.mask_without(6, [0, 2, 5])
        r.refuse(lambda: ctx.decode_slices(ptrs, sizes, gone), EIO)
        r.refuse(lambda: ctx.decode_slices_multi(
            ptrs, sizes, [one_lost, gone, full]), EIO)
        # a valid full mask is not an error, and writes nothing
        ctx.decode_slices(ptrs, sizes, full)
        ctx.decode_slices_multi(ptrs, sizes, [full] * 3)
        ctx.sync()
        same(r.d.get(), r.image, "full masks")
        # contexts the slice calls do not serve
        for tech in ("cauchy_orig", "jerasure_reed_sol_van_w16"):
            other = ceph_amd.EcContext(4, 2, tech, device=0)
            try:
                r.refuse(lambda: other.encode_slices(ptrs, sizes), EINVAL)
                r.refuse(lambda: other.decode_slices(ptrs, sizes, one_lost),
                         EINVAL)
                r.refuse(lambda: other.decode_slices_multi(
                    ptrs, sizes, [one_lost] * 3), EINVAL)
            finally:
                other.close()
    finally:
        r.close()


def test_refusals_null_output_and_misaligned_pointers():
    """A NULL pointer for a chunk the call writes, and a pointer that is no
    multiple of 16: refused by the host check before anything is enqueued
    (test_slices_cases.py pins that check on the CPU). NULL stays legal for
    a chunk that is only read."""
    r = Refusals()
    ctx, sizes = r.ctx, r.sizes
    lost = [1, 4]
    mask = cases.mask_without(6, lost)
    try:
        for s in range(3):
            for c in (4, 5):  # a parity pointer of an encode
                p = list(r.d.ptrs)
                p[s * 6 + c] = None
                r.refuse(lambda: ctx.encode_slices(p, sizes), EINVAL)
            for c in lost:    # an erased chunk of a decode
                p = list(r.d.ptrs)
                p[s * 6 + c] = None
                r.refuse(lambda: ctx.decode_slices(p, sizes, mask), EINVAL)
                r.refuse(lambda: ctx.decode_slices_multi(
                    p, sizes, [0x3F, 0x3F, 0x3F][:s] + [mask] * (3 - s)),
                    EINVAL)
        for at in (0, 5, 6 + 2, 12 + 4):  # sources and outputs alike
            p = list(r.d.ptrs)
            p[at] += 8
            r.refuse(lambda: ctx.encode_slices(p, sizes), EINVAL)
            r.refuse(lambda: ctx.decode_slices(p, sizes, mask), EINVAL)
            r.refuse(lambda: ctx.decode_slices(p, sizes, 0x3F), EINVAL)
            r.refuse(lambda: ctx.decode_slices_multi(p, sizes, [mask] * 3),
                     EINVAL)
        # the erased set is the slice's own: NULL where another slice's
        # mask erases is a zeros source here. Chunk 1 of slice 0 is NULL and
        # present there; slices 1 and 2 lose chunk 1.
        p = list(r.d.ptrs)
        p[1] = None
        arena = r.arena
        image = r.want.copy()
        arena.chunk(image, 0, 1)[:] = 0
        truth = cases.encode_want(arena, 4, cases.coding_rows(
            "reed_sol_van", 4, 2), image=image)
        masks = [cases.mask_without(6, [0]), cases.mask_without(6, [1]),
                 cases.mask_without(6, [1, 5])]
        r.d.put(cases.erase(arena, truth, masks))
        ctx.decode_slices_multi(p, sizes, masks)
        ctx.sync()
        same(r.d.get(), truth, "NULL present chunk under per-slice masks")
    finally:
        r.close()
