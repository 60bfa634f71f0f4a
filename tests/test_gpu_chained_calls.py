"""Calls chained on a slot with no sync between them. The library orders a
slot's work by single-entry rings (the launch-record upload and its event,
the job blob and its event), by the hipMemsetAsync of the verify words and
by the CRC seed pass; each has to sit on the slot's stream in the right
place. Here every call of a round is enqueued back to back — fill, encode,
crc, update, verify, poison uploads, verify, decode_batch_multi, verify, crc
in place — and only then one sync and the downloads. Masks and seeds differ
per round, so every ring entry changes between calls; a ring wait that was
dropped or a memset on another stream shows as a stale record or a stale
word in what is downloaded.

cauchy (4, 6), C = 64 KiB + 16, S = 1024 (671 MB): update, verify and the
five- and six-erasure decodes take two passes each, so launches follow each
other inside a call as well as between calls. The size is chosen so that a
kernel is plausibly still running while the host prepares the next call;
that overlap cannot be asserted, and nothing here takes a time.

The expectation is the host model of cross_call_cases.chain_model, held
against the oracle on the CPU in test_cross_call_cases.py."""
import ctypes
import threading

import numpy as np
import pytest

import ceph_amd
import oracle
import crc_cases
import cross_call_cases as cc
from decode_multi_cases import erased_of, mask_without
from test_gpu_stream_kernel import mul_table
from test_gpu_verify import expected_word

pytestmark = pytest.mark.gpu

FF64 = 0xFFFFFFFFFFFFFFFF


def ck(r, what):
    if r < 0:
        raise ceph_amd.EcError(f"{what}: {r}")


class Lane:
    """One batch on one slot of a context: its device buffers, the steps of
    a round as a generator (one library call per step, never a sync), and
    the checks after the round's sync."""

    def __init__(self, ctx, slot, S, lane=0):
        self.tech, self.k, self.m, self.C = (
            cc.CHAIN[x] for x in ("tech", "k", "m", "C"))
        self.ctx, self.slot, self.S, self.lane = ctx, slot, S, lane
        self.n = self.k + self.m
        self.full = (1 << self.n) - 1
        self.stripes = cc.chain_sample(S, lane)
        self.nbytes = S * self.n * self.C
        self.d = ctx.dbuf_alloc(self.nbytes)
        self.d_new = ctx.dbuf_alloc(S * self.k * self.C)
        self.d_crc = ctx.dbuf_alloc(4 * S * self.n)
        self.d_bad = [ctx.dbuf_alloc(8 * S) for _ in range(3)]
        self.poison = np.full(self.C, cc.POISON, np.uint8)
        # the host arrays of the non-blocking uploads live as long as the lane
        self.ones = np.full(S, FF64, np.uint64)

    def free(self):
        for p in [self.d, self.d_new, self.d_crc] + self.d_bad:
            self.ctx.dbuf_free(p)

    def at(self, s, c):
        return ctypes.c_void_p(self.d.value + (s * self.n + c) * self.C)

    def crc(self, seed):
        ck(ceph_amd.lib().ecx_crc32c_batch(
            self.ctx._h, self.d, self.S, self.C, self.full, seed, 0,
            self.d_crc, self.slot), "ecx_crc32c_batch")

    def verify(self, i):
        # the words start as all ones: the call's own zeroing has to come
        # after this upload and before its kernels
        self.ctx.upload(self.d_bad[i], self.ones, self.slot, blocking=False)
        ck(ceph_amd.lib().ecx_verify_batch(
            self.ctx._h, self.d, self.S, self.C, self.full, self.d_bad[i],
            self.slot), "ecx_verify_batch")

    def steps(self, rnd):
        ctx, slot, S, C = self.ctx, self.slot, self.S, self.C
        self.seeds = cc.chain_seeds(rnd, self.lane)
        self.wm = cc.chain_write_masks(rnd, S, self.k, self.lane)
        self.dm = cc.chain_decode_masks(rnd, S, self.n, self.lane)
        total_new = cc.new_bases(self.wm)[1]
        ctx.fill_random(self.d, self.nbytes, self.seeds[0], slot)
        yield
        ctx.fill_random(self.d_new, total_new * C, self.seeds[1], slot)
        yield
        ctx.encode_batch(self.d, S, C, slot)
        yield
        self.crc(None)
        yield
        ctx.update_batch(self.d, S, C, self.d_new, self.wm, slot)
        yield
        self.verify(0)
        yield
        for s in self.stripes:
            for c in erased_of(self.n, self.dm[s]):
                ctx.upload(self.at(s, c), self.poison, slot, blocking=False)
        yield
        self.verify(1)
        yield
        ctx.decode_batch_multi(self.d, S, C, self.dm, slot)
        yield
        self.verify(2)
        yield
        self.crc(self.d_crc)
        yield

    def check(self, rnd):
        """The round's one sync, then the downloads."""
        ctx, slot, S, n, C = self.ctx, self.slot, self.S, self.n, self.C
        ctx.sync(slot)
        mod = cc.chain_model(self.tech, self.k, self.m, C, self.stripes,
                             self.seeds, self.wm, self.dm)
        got = np.zeros((len(self.stripes), n, C), np.uint8)
        for i, s in enumerate(self.stripes):
            ctx.download(got[i], self.at(s, 0), slot)
        bad = [np.zeros(S, np.uint64) for _ in range(3)]
        for i in range(3):
            ctx.download(bad[i], self.d_bad[i], slot)
        words = np.zeros((S, n), np.uint32)
        ctx.download(words, self.d_crc, slot)

        where = (self.lane, rnd)
        for i, s in enumerate(self.stripes):
            assert np.array_equal(got[i], mod["upd"][i]), (where, s)
        assert not bad[0].any(), (where, np.flatnonzero(bad[0]))
        assert not bad[2].any(), (where, np.flatnonzero(bad[2]))
        ref = np.zeros(S, np.uint64)
        for i, s in enumerate(self.stripes):
            ref[s] = expected_word(self.tech, self.k, self.m,
                                   list(mod["poisoned"][i]), self.full)
            assert (ref[s] != 0) == bool(erased_of(n, self.dm[s]))
        assert ref.any()
        assert np.array_equal(bad[1], ref), \
            (where, np.flatnonzero(bad[1] != ref))
        first = crc_cases.crc_many(0xFFFFFFFF, mod["enc"].reshape(-1, C))
        both = crc_cases.crc_many(first, mod["upd"].reshape(-1, C))
        assert np.array_equal(words[self.stripes].reshape(-1), both), where


def drain(steps):
    for _ in steps:
        pass


def test_one_slot_three_rounds():
    ctx = ceph_amd.EcContext(cc.CHAIN["k"], cc.CHAIN["m"], cc.CHAIN["tech"],
                             device=0, n_streams=2)
    lane = Lane(ctx, 0, cc.CHAIN["S"])
    try:
        for rnd in range(cc.CHAIN_ROUNDS):
            drain(lane.steps(rnd))
            lane.check(rnd)
    finally:
        ctx.sync(0)
        lane.free()
        ctx.close()


def two_lanes():
    ctx = ceph_amd.EcContext(cc.CHAIN["k"], cc.CHAIN["m"], cc.CHAIN["tech"],
                             device=0, n_streams=2)
    return ctx, [Lane(ctx, slot, cc.CHAIN["S"] // 2, lane=1 + slot)
                 for slot in (0, 1)]


def test_two_slots_one_thread():
    """Two batches with different seeds, every call alternating between
    slot 0 and slot 1, one sync per slot at the end of a round."""
    ctx, lanes = two_lanes()
    try:
        for rnd in range(cc.CHAIN_ROUNDS):
            for _ in zip(lanes[0].steps(rnd), lanes[1].steps(rnd)):
                pass
            for lane in lanes:
                lane.check(rnd)
    finally:
        for lane in lanes:
            ctx.sync(lane.slot)
            lane.free()
        ctx.close()


def test_two_threads_one_slot_each():
    mul_table()  # the reference's lazily built table, ahead of the threads
    ctx, lanes = two_lanes()
    errors = []

    def work(lane):
        try:
            for rnd in range(cc.CHAIN_ROUNDS):
                drain(lane.steps(rnd))
                lane.check(rnd)
        except BaseException as e:  # reported by the test's own thread
            errors.append((lane.lane, repr(e)))

    try:
        threads = [threading.Thread(target=work, args=(lane,))
                   for lane in lanes]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
    finally:
        for lane in lanes:
            ctx.sync(lane.slot)
            lane.free()
        ctx.close()


# ---- the contexts that take only encode, decode and crc ---------------------

def family_encoded(tech, kw, k, m, stripes, C, seed):
    buf = cc.filled_stripes(stripes, k + m, C, seed).copy()
    for st in buf:
        data = [st[i] for i in range(k)]
        par = (oracle.encode_w16(k, m, data) if not kw else
               oracle.bitmatrix_encode(k, m, data, kw["packetsize"]))
        for r in range(m):
            st[k + r] = par[r]
    return buf


@pytest.mark.parametrize("tech,kw,C,S", cc.CHAIN_FAMILIES,
                         ids=[f[0] for f in cc.CHAIN_FAMILIES])
def test_family_short_chain(tech, kw, C, S):
    """encode, crc, poison uploads, decode with one two-erasure mask, crc in
    place, sync: these contexts refuse the other calls."""
    k, m = 4, 2
    n, full = k + m, (1 << (k + m)) - 1
    stripes = cc.chain_sample(S)
    seed = cc.chain_seeds(0, lane=3)[0]
    enc = family_encoded(tech, kw, k, m, stripes, C, seed)
    poison = np.full(C, cc.POISON, np.uint8)
    ctx = ceph_amd.EcContext(k, m, tech, device=0, n_streams=2, **kw)
    d = ctx.dbuf_alloc(S * n * C)
    d_crc = ctx.dbuf_alloc(4 * S * n)
    lib = ceph_amd.lib()
    try:
        ctx.fill_random(d, S * n * C, seed)
        ctx.encode_batch(d, S, C)
        ck(lib.ecx_crc32c_batch(ctx._h, d, S, C, full, None, 0, d_crc, 0),
           "ecx_crc32c_batch")
        for s in stripes:
            for c in cc.FAMILY_ERASED:
                ctx.upload(ctypes.c_void_p(d.value + (s * n + c) * C), poison,
                           blocking=False)
        ctx.decode_batch(d, S, C, mask_without(n, cc.FAMILY_ERASED))
        ck(lib.ecx_crc32c_batch(ctx._h, d, S, C, full, d_crc, 0, d_crc, 0),
           "ecx_crc32c_batch")
        ctx.sync()
        got = np.zeros((len(stripes), n, C), np.uint8)
        for i, s in enumerate(stripes):
            ctx.download(got[i], ctypes.c_void_p(d.value + s * n * C))
        words = np.zeros((S, n), np.uint32)
        ctx.download(words, d_crc)
    finally:
        ctx.sync()
        ctx.dbuf_free(d)
        ctx.dbuf_free(d_crc)
        ctx.close()
    for i, s in enumerate(stripes):
        assert np.array_equal(got[i], enc[i]), s
    first = crc_cases.crc_many(0xFFFFFFFF, enc.reshape(-1, C))
    both = crc_cases.crc_many(first, enc.reshape(-1, C))
    assert np.array_equal(words[stripes].reshape(-1), both)
