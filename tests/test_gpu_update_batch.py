"""GPU tests for parity-delta writes over a batch (ecx_update_batch) and the
fused host call (ecx_apply_deltas_host).

Expectation: update_cases.delta_expect — the oracle alone (oracle.matrix
coefficients through oracle.region_mul_xor on old ^ new); where the old
parity was consistent it is also checked against oracle.encode of the new
data. test_update_plan.py proves the two agree on the CPU. The assertion is
whole-buffer equality after download: the batch with a 4 KiB guard behind it
(unchanged data chunks, untouched stripes, stray writes) and d_new with its
own guard (the call must leave it as it was)."""
import ctypes
import functools

import numpy as np
import pytest

import ceph_amd
import oracle
import update_cases as cases

pytestmark = pytest.mark.gpu

GUARD = np.full(4096, 0x5A, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def scenario(tech, k, m, chunk_bytes, masks, garbage=False, seed=0xEC):
    """(old batch + guard, new chunks + guard, expected batch + guard) as
    flat read-only arrays; masks is a tuple. garbage: parity chunks hold
    random bytes instead of the encode."""
    S, n, C = len(masks), k + m, chunk_bytes
    rng = np.random.default_rng(seed)
    old = rng.integers(0, 256, (S, n, C), dtype=np.uint8)
    if not garbage:
        oracle.cpu_encode_batch(tech, k, m, old.reshape(-1), S, C)
    new = rng.integers(0, 256, (cases.total_new(masks), C), dtype=np.uint8)
    want = cases.delta_expect(tech, k, m, old, new, masks)
    if not garbage:
        for s in range(S):
            enc = oracle.encode(tech, k, m,
                                [want[s, j].copy() for j in range(k)])
            for r in range(m):
                assert np.array_equal(want[s, k + r], enc[r]), (s, r)
    out = tuple(np.concatenate([a.reshape(-1), GUARD]) for a in (old, new, want))
    for a in out:
        a.flags.writeable = False
    return out


def run_update(tech, k, m, chunk_bytes, masks, **kw):
    old, new, want = scenario(tech, k, m, chunk_bytes, tuple(masks), **kw)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d, dn = ctx.dbuf_alloc(old.nbytes), ctx.dbuf_alloc(new.nbytes)
        ctx.upload(d, old)
        ctx.upload(dn, new)
        ctx.update_batch(d, len(masks), chunk_bytes, dn, masks)
        ctx.sync()
        ms = ctx.last_kernel_ms() if any(masks) else None
        got, got_new = np.empty_like(old), np.empty_like(new)
        ctx.download(got, d)
        ctx.download(got_new, dn)
        ctx.dbuf_free(d)
        ctx.dbuf_free(dn)
    finally:
        ctx.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_new, new)
    return ms


@pytest.mark.parametrize("tech", cases.MATRIX_TECHS)
def test_all_write_masks(tech):
    # 4112 = 257 vectors: one full 256-lane tile plus a one-vector tail
    ms = run_update(tech, 4, 3, 4112, cases.all_masks_43())
    assert ms > 0  # one event pair spans the call


def test_mid_size_chunks():
    run_update("reed_sol_van", 8, 3, 8208, cases.mid_83())


def test_two_passes_keep_old_data_until_the_last():
    # m = 6: rows 4 and 5 are wrong if pass 0 overwrites the data
    run_update("cauchy", 4, 6, 4112, cases.two_passes_46())


def test_grid_stride_and_tail():
    # > 2048 active stripes: grid x stays narrow, so each block takes two
    # grid-stride steps, the second a one-vector tail
    run_update("reed_sol_van", 2, 1, 8208, cases.long_list_21())


def test_garbage_parity_is_corrected_not_recomputed():
    run_update("reed_sol_van", 8, 3, 8208, cases.mid_83(), garbage=True)


def test_all_masks_zero():
    assert run_update("reed_sol_van", 4, 3, 4112, [0] * 64) is None


def test_smallest_chunk_and_adjacent_d_new():
    # C = 16: a single vector. One allocation [batch][new][guard]: d_new
    # starts exactly where the batch ends, which is no overlap
    tech, k, m, C = "reed_sol_van", 4, 2, 16
    masks = cases.smallest_42()
    old, new, want = scenario(tech, k, m, C, tuple(masks))
    nb = old.nbytes - GUARD.nbytes
    dev = np.concatenate([old[:nb], new])
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d = ctx.dbuf_alloc(dev.nbytes)
        ctx.upload(d, dev)
        ctx.update_batch(d, len(masks), C, ctypes.c_void_p(d.value + nb),
                         masks)
        ctx.sync()
        got = np.empty_like(dev)
        ctx.download(got, d)
        ctx.dbuf_free(d)
    finally:
        ctx.close()
    assert np.array_equal(got, np.concatenate([want[:nb], new]))


def test_refusals():
    tech, k, m, C = "reed_sol_van", 4, 3, 4112
    masks = cases.all_masks_43()
    S = len(masks)
    old, new, _ = scenario(tech, k, m, C, tuple(masks))
    lib = ceph_amd.lib()
    u64 = ctypes.c_uint64
    arr = (u64 * S)(*masks)
    high = list(masks)
    high[40] |= 1 << k
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        d, dn = ctx.dbuf_alloc(old.nbytes), ctx.dbuf_alloc(new.nbytes)
        ctx.upload(d, old)
        ctx.upload(dn, new)
        last = ctypes.c_void_p(d.value + (S * (k + m) - 1) * C)
        raw = [(None, d, S, C, dn, arr, 0),            # NULL ctx
               (ctx._h, None, S, C, dn, arr, 0),       # NULL batch
               (ctx._h, d, S, C, None, arr, 0),        # NULL d_new
               (ctx._h, d, S, C, dn, None, 0),         # NULL masks
               (ctx._h, d, S, C, dn, arr, 9),          # bad slot
               (ctx._h, d, S, C, dn, arr, -1),
               (ctx._h, d, S, C + 8, dn, arr, 0),      # chunk_bytes % 16
               (ctx._h, d, 0, C, dn, arr, 0),          # n_stripes range
               (ctx._h, d, 65536, 16, dn, (u64 * 65536)(), 0),
               (ctx._h, d, S, C, dn, (u64 * S)(*high), 0),  # bit at k
               (ctx._h, d, S, C, d, arr, 0),           # d_new inside batch
               (ctx._h, d, S, C, last, arr, 0)]        # ... over its end
        for args in raw:
            assert lib.ecx_update_batch(*args) == -22, args[1:]
            ctx.sync()
            got, got_new = np.empty_like(old), np.empty_like(new)
            ctx.download(got, d)
            ctx.download(got_new, dn)
            assert np.array_equal(got, old), args[1:]  # nothing was launched
            assert np.array_equal(got_new, new), args[1:]
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.update_batch(d, S, C, dn, high)
        with pytest.raises(ceph_amd.EcError):
            ctx.update_batch(d, S, C, dn, masks[:-1])  # one mask per stripe
        ctx.dbuf_free(d)
        ctx.dbuf_free(dn)
    finally:
        ctx.close()

    for tech, cb in (("cauchy_orig", 8 * 2048),
                     ("jerasure_reed_sol_van_w16", 4096)):
        ctx = ceph_amd.EcContext(4, 2, tech, device=0)
        try:
            d, dn = ctx.dbuf_alloc(6 * cb), ctx.dbuf_alloc(cb)
            with pytest.raises(ceph_amd.EcError, match="EINVAL"):
                ctx.update_batch(d, 1, cb, dn, [1])
            ctx.dbuf_free(d)
            ctx.dbuf_free(dn)
        finally:
            ctx.close()


# ---- fused host call ----

FAMILIES = [
    # (technique, k, m, context kwargs, smallest legal chunk, a larger one)
    ("reed_sol_van", 4, 2, {}, 16, 4112),
    ("jerasure_reed_sol_van_w16", 4, 3, {}, 64, 4160),
    ("cauchy_orig", 4, 3, {"packetsize": 32}, 8 * 32, 17 * 8 * 32),
]


@pytest.mark.parametrize("tech,k,m,kw,small,large", FAMILIES,
                         ids=[f[0] for f in FAMILIES])
def test_apply_deltas_equals_pair_loop(tech, k, m, kw, small, large):
    ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
    try:
        for C in (small, large):
            rng = np.random.default_rng(C)
            deltas = {j: rng.integers(0, 256, C, dtype=np.uint8)
                      for j in (0, 2)}
            start = {k + r: rng.integers(0, 256, C, dtype=np.uint8)
                     for r in range(m)}
            loop = {c: p.copy() for c, p in start.items()}
            for j, dl in deltas.items():
                for c, p in loop.items():
                    ctx.apply_delta(dl, j, c, p)
            fused = {c: p.copy() for c, p in start.items()}
            keep = {j: dl.copy() for j, dl in deltas.items()}
            assert ctx.apply_deltas(deltas, fused) is fused
            for c in start:
                assert np.array_equal(fused[c], loop[c]), (C, c)
            for j in deltas:
                assert np.array_equal(deltas[j], keep[j])
            if tech == "reed_sol_van":
                gen = oracle.matrix(tech, k, m)
                for c, p in start.items():
                    want = p.copy()
                    for j, dl in deltas.items():
                        oracle.region_mul_xor(int(gen[c, j]), dl, want)
                    assert np.array_equal(fused[c], want), (C, c)
    finally:
        ctx.close()


@pytest.mark.parametrize("tech,k,m,kw,small,large", FAMILIES,
                         ids=[f[0] for f in FAMILIES])
def test_apply_deltas_refusals(tech, k, m, kw, small, large):
    C = small
    dl = {0: np.full(C, 1, np.uint8), 2: np.full(C, 2, np.uint8)}
    par = {k + r: np.full(C, 3, np.uint8) for r in range(m)}
    lib = ceph_amd.lib()
    ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
    try:
        bad = [({}, par),                                       # n_in = 0
               (dl, {}),                                        # n_out = 0
               ({0: dl[0], k: dl[2]}, par),                     # data id >= k
               (dl, {k - 1: par[k]}),                           # coding id < k
               (dl, {k + m: par[k]}),                           # coding id past m
               ({j: a[:8] for j, a in dl.items()},
                {c: a[:8] for c, a in par.items()})]            # bytes % 16
        if tech == "cauchy_orig":                               # not w * pkt
            bad.append(({j: a[:16] for j, a in dl.items()},
                        {c: a[:16] for c, a in par.items()}))
        for deltas, parities in bad:
            with pytest.raises(ceph_amd.EcError, match="EINVAL"):
                ctx.apply_deltas(deltas, parities)
        # n_in > k, n_out > m, NULL arrays and NULL entries
        ptrs = ceph_amd._ptr_array
        ds, cs = (ctypes.c_int * 8)(*([0] * 8)), (ctypes.c_int * 8)(*([k] * 8))
        dp, pp = ptrs([dl[0]] * 8), ptrs([par[k]] * 8)
        for args in [(ctx._h, dp, ds, k + 1, pp, cs, 1, C),
                     (ctx._h, dp, ds, 1, pp, cs, m + 1, C),
                     (None, dp, ds, 1, pp, cs, 1, C),
                     (ctx._h, None, ds, 1, pp, cs, 1, C),
                     (ctx._h, dp, None, 1, pp, cs, 1, C),
                     (ctx._h, dp, ds, 1, None, cs, 1, C),
                     (ctx._h, dp, ds, 1, pp, None, 1, C),
                     (ctx._h, ptrs([None]), ds, 1, pp, cs, 1, C),
                     (ctx._h, dp, ds, 1, ptrs([None]), cs, 1, C)]:
            assert lib.ecx_apply_deltas_host(*args) == -22, args[1:]
        for a in par.values():
            assert (a == 3).all()  # nothing was written back
    finally:
        ctx.close()
