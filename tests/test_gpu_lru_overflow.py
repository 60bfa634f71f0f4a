"""More decode plans than the context's plan cache holds. multi_resolve
fetches every distinct mask of one decode_batch_multi call through the
cache, so a call with more distinct masks than LRU_DEPTH evicts plans while
it is still collecting them; decode_batch and verify_batch then find some
plans resident and some long evicted. cauchy (16, 4), C = 16, one stripe per
pattern of 1..4 erasures: 6195 stripes, about 2 MB.
test_cross_call_cases.py proves on the CPU that every mask is decodable and
that 6195 is more than the cache's depth."""
import ctypes

import numpy as np
import pytest

import ceph_amd
import oracle
import cross_call_cases as cc
from decode_multi_cases import erased_of
from test_gpu_stream_kernel import ref_matmul
from test_gpu_verify import expected_words

pytestmark = pytest.mark.gpu

TECH, K, M, C = (cc.LRU[x] for x in ("tech", "k", "m", "C"))
N = K + M
MASKS = cc.lru_masks()
S = len(MASKS)


def poisoned(orig, masks):
    """orig's stripes with the erased chunks of their masks overwritten."""
    host = orig[:len(masks)].copy()
    for s, mk in enumerate(masks):
        for c in erased_of(N, mk):
            host[s, c] = cc.POISON
    return host


class Rig:
    def __init__(self):
        self.orig = np.random.default_rng(0x164).integers(
            0, 256, (S, N, C), dtype=np.uint8)
        ref_matmul(self.orig, list(range(K)), list(range(K, N)),
                   oracle.matrix(TECH, K, M)[K:])
        self.orig.flags.writeable = False
        self.dirty = poisoned(self.orig, MASKS)
        self.ctx = ceph_amd.EcContext(K, M, TECH, device=0)
        self.d = self.ctx.dbuf_alloc(self.orig.nbytes)
        self.multi = None

    def at(self, s):
        return ctypes.c_void_p(self.d.value + s * N * C)

    def get(self, ctx, n=S, first=0):
        out = np.zeros((n, N, C), np.uint8)
        ctx.download(out, self.at(first))
        return out

    def overflowed(self):
        """One decode_batch_multi call over all 6195 masks, made once: the
        state of the cache that the other cases start from."""
        if self.multi is None:
            self.ctx.upload(self.d, self.dirty)
            self.ctx.decode_batch_multi(self.d, S, C, MASKS)
            self.ctx.sync()
            self.multi = self.get(self.ctx)
        return self.multi

    def decode_each(self, ctx, which):
        """decode_batch with one mask per call on that mask's own stripe,
        poisoned anew; every stripe must come back as it was."""
        for i in which:
            ctx.upload(self.at(i), self.dirty[i])
            ctx.decode_batch(self.at(i), 1, C, MASKS[i])
        ctx.sync()
        for i in which:
            got = self.get(ctx, 1, i)
            assert np.array_equal(got[0], self.orig[i]), (i, hex(MASKS[i]))

    def close(self):
        self.ctx.dbuf_free(self.d)
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def test_one_call_with_more_masks_than_the_cache(rig):
    got = rig.overflowed()
    diff = [s for s in range(S) if not np.array_equal(got[s], rig.orig[s])]
    assert not diff, (len(diff), diff[:8], [hex(MASKS[s]) for s in diff[:8]])


def test_decode_batch_after_the_overflow(rig):
    """The first masks of the list are long evicted, the last resident."""
    rig.overflowed()
    first, last = list(range(16)), list(range(S - 16, S))
    rig.decode_each(rig.ctx, first)
    rig.decode_each(rig.ctx, last)
    rig.decode_each(rig.ctx, first)


def test_decode_batch_through_every_mask(rig):
    """A fresh context, one decode_batch per mask, so the cache fills and
    then turns over one plan per call; then the first masks again."""
    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    try:
        ctx.upload(rig.d, rig.dirty)
        for s, mk in enumerate(MASKS):
            ctx.decode_batch(rig.at(s), 1, C, mk)
        ctx.sync()
        got = rig.get(ctx)
        diff = [s for s in range(S)
                if not np.array_equal(got[s], rig.orig[s])]
        assert not diff, (len(diff), diff[:8])
        rig.decode_each(ctx, list(range(16)))
    finally:
        ctx.close()


def test_verify_batch_shares_the_cache(rig):
    """verify_batch takes its rows from the same cache (get_verify_plan): 64
    degraded masks on 64 stripes, one changed byte in each stripe."""
    rig.overflowed()
    n = 64
    host = rig.orig[:n].copy()
    for s in range(n):
        host[s, (7 * s) % N, s % C] ^= 1 + s
    rig.ctx.upload(rig.d, host)
    for mk in cc.lru_verify_masks(n):
        words = rig.ctx.verify_batch(rig.d, n, C, mk)
        want = expected_words(TECH, K, M, host, mk)
        assert np.array_equal(words, want), \
            (hex(mk), np.flatnonzero(words != want))
    assert np.array_equal(rig.get(rig.ctx, n), host), "the batch was written"
