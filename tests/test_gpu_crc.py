"""ecx_crc32c_batch: ceph_crc32c of every chunk of a device batch. Every
expected word comes from crc_cases.py alone (numpy, from the polynomial); the
library's host routines are used only to read the launch plan, from which
the chunk sizes are chosen: one lane segment is L bytes, one block covers B
bytes of a chunk, both counted from the END of the chunk.

The kernel has no ECX_CRC* knob. The one environment variable that selects
another instance of it is the library-wide ECX_NT (plain instead of
nontemporal loads); run as a script, this file is the child process of the
test of ECX_NT=0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child: no conftest has set the path
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import ceph_amd  # noqa: E402
import crc_cases as cases  # noqa: E402
import oracle  # noqa: E402

gpu = pytest.mark.gpu
TECH = "reed_sol_van"
M32 = 0xFFFFFFFF
FILL = 0xA5C3F00D  # what the word array holds before every call

PLAN = ceph_amd.crc32c_plan_probe(16, 1, 1)
L = PLAN["seg_bytes"]
B = L * PLAN["segs_per_block"]
SIZES = [16, 48, L, L + 16, 3 * L - 16, B - 16, B, B + 16, 2 * B + 48,
         65536 + 48]
BIG = (1 << 20) + 16


def full(k, m):
    return (1 << (k + m)) - 1


def random_batch(S, n, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (S, n, C),
                                                dtype=np.uint8)


class Rig:
    """A context, a device batch and a device word array that holds FILL in
    every word before each call."""

    def __init__(self, k, m, tech=TECH, **kw):
        self.k, self.m, self.n = k, m, k + m
        self.ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
        self.d = self.d_crc = self.d_seed = None
        self.shape = None

    def load(self, host):
        host = np.ascontiguousarray(host)
        if self.shape != host.shape:
            self.free()
            self.shape = host.shape
            self.S = host.shape[0]
            self.d = self.ctx.dbuf_alloc(host.nbytes)
            self.d_crc = self.ctx.dbuf_alloc(4 * self.S * self.n)
            self.d_seed = self.ctx.dbuf_alloc(4 * self.S * self.n)
        self.ctx.upload(self.d, host)

    def get(self):
        out = np.zeros(self.shape, np.uint8)
        self.ctx.download(out, self.d)
        return out

    def fill(self, words=None):
        w = np.full((self.S, self.n), FILL, np.uint32) if words is None \
            else np.ascontiguousarray(words, dtype=np.uint32)
        self.ctx.upload(self.d_crc, w)

    def words(self):
        out = np.zeros((self.S, self.n), np.uint32)
        self.ctx.download(out, self.d_crc)
        return out

    def crc(self, prefill=True, **kw):
        """crc32c_batch into the rig's own word array."""
        if prefill:
            self.fill()
        kw.setdefault("d_crc", self.d_crc)
        C = kw.pop("C", self.shape[2])
        S = kw.pop("S", self.S)
        return self.ctx.crc32c_batch(kw.pop("dptr", self.d), S, C, **kw)

    def free(self):
        for p in (self.d, self.d_crc, self.d_seed):
            if p is not None:
                self.ctx.dbuf_free(p)
        self.d = self.d_crc = self.d_seed = None

    def close(self):
        self.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig42():
    r = Rig(4, 2, n_streams=2)
    yield r
    r.close()


def test_sizes_follow_the_plan():
    """CPU only: the sizes above sit where the plan says the paths change."""
    assert L % 16 == 0 and B % L == 0 and 3 * L - 16 < B - 16
    bpc = [ceph_amd.crc32c_plan_probe(C, 1, 1)["blocks_per_chunk"]
           for C in SIZES + [BIG]]
    assert bpc[:7] == [1] * 7 and bpc[7] == 2 and bpc[8] == 3
    assert bpc[10] == -(-BIG // B) > 3


# ---- random data -----------------------------------------------------------

def check_random(rig, S, C, seed):
    host = random_batch(S, rig.n, C, seed)
    rig.load(host)
    got = rig.crc()
    want = cases.batch_ref(host)
    assert np.array_equal(got, want), (S, C, np.argwhere(got != want)[:4])


@gpu
@pytest.mark.parametrize("C", SIZES)
@pytest.mark.parametrize("S", [1, 3, 257])
def test_random_data(rig42, S, C):
    check_random(rig42, S, C, seed=S * 131 + C)


@gpu
def test_random_data_production_size():
    """1 MiB + 16: many blocks per chunk, the first of them a 16-byte one."""
    rig = Rig(2, 1)
    try:
        check_random(rig, 2, BIG, seed=0xB16)
    finally:
        rig.close()


# ---- position sensitivity --------------------------------------------------

def positions(C):
    plan = ceph_amd.crc32c_plan_probe(C, 1, 1)
    ps = {0, 15, 16, C - 1}
    for b in cases.borders(plan, C) + cases.block_borders(plan, C):
        ps |= {b - 1, b}
    return sorted(p for p in ps if 0 <= p < C)


@gpu
@pytest.mark.parametrize("C", SIZES)
def test_one_byte_at_every_border(rig42, C):
    """All-zero chunks but one byte 0x80, seed 0: the word is that byte's
    hash moved over what follows it. A wrong combine constant shows here
    whichever segment it belongs to."""
    ps = positions(C)
    n = rig42.n
    S = -(-len(ps) // n)
    host = np.zeros((S, n, C), np.uint8)
    want = np.zeros((S, n), np.uint32)
    one = cases.crc(0, b"\x80")
    for i, p in enumerate(ps):
        host[i // n, i % n, p] = 0x80
        want[i // n, i % n] = cases.crc_shift(one, C - 1 - p)
    rig42.load(host)
    got = rig42.crc(seeds=np.zeros((S, n), np.uint32))
    bad = np.argwhere(got != want)
    assert not len(bad), (C, [ps[s * n + c] for s, c in bad[:6]
                              if s * n + c < len(ps)])


@gpu
@pytest.mark.parametrize("C", [16, L + 16, B + 16, 2 * B + 48])
def test_zero_chunks(rig42, C):
    host = np.zeros((3, rig42.n, C), np.uint8)
    rig42.load(host)
    got = rig42.crc()
    want = cases.batch_ref(host)
    assert want.all() and np.array_equal(got, want)
    if C == 16:
        assert (got == 0xBD8F6515).all()
    assert not rig42.crc(seeds=np.zeros((3, rig42.n), np.uint32)).any()


# ---- seeds, masks ----------------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [48, B + 16])
def test_seeds_and_in_place(rig42, C):
    S, n = 5, rig42.n
    host = random_batch(S, n, C, seed=C + 9)
    seeds = np.random.default_rng(C).integers(0, 1 << 32, (S, n),
                                              dtype=np.uint32)
    want = cases.batch_ref(host, seeds)
    rig42.load(host)
    assert np.array_equal(rig42.crc(seeds=seeds), want)
    # the same seeds from a device array of their own
    rig42.ctx.upload(rig42.d_seed, seeds)
    assert np.array_equal(rig42.crc(seeds=rig42.d_seed), want)
    # in place: the word array holds the seeds
    rig42.fill(seeds)
    assert np.array_equal(rig42.crc(prefill=False, seeds=rig42.d_crc), want)
    # and once more appends the same chunks to the running hashes
    twice = cases.batch_ref(host, want)
    assert np.array_equal(rig42.crc(prefill=False, seeds=rig42.d_crc), twice)
    dbl = np.concatenate([host, host], axis=2)
    assert np.array_equal(twice, cases.batch_ref(dbl, seeds))


@gpu
@pytest.mark.parametrize("mask", [0x0F, 0x30, 0x04, 0x21])
def test_masks_keep_other_words(rig42, mask):
    S, n, C = 3, rig42.n, B + 16
    host = random_batch(S, n, C, seed=mask)
    want = cases.batch_ref(host)
    rig42.load(host)
    got = rig42.crc(chunk_mask=mask)
    for c in range(n):
        if mask >> c & 1:
            assert np.array_equal(got[:, c], want[:, c]), c
        else:
            assert (got[:, c] == FILL).all(), c
    # the temporary array: unmasked columns come back 0
    got = rig42.ctx.crc32c_batch(rig42.d, S, C, chunk_mask=mask)
    for c in range(n):
        assert np.array_equal(got[:, c], want[:, c] if mask >> c & 1
                              else np.zeros(S, np.uint32))


@gpu
def test_mask_zero_is_ok_and_writes_nothing(rig42):
    rig42.load(random_batch(2, rig42.n, 48, seed=1))
    assert (rig42.crc(chunk_mask=0) == FILL).all()
    assert (rig42.crc(chunk_mask=0, chain=True) == FILL).all()


# ---- chain mode ------------------------------------------------------------

@gpu
@pytest.mark.parametrize("S", [1, 2, 5, 257])
def test_chain(rig42, S):
    C, n = 4112, rig42.n
    host = random_batch(S, n, C, seed=S)
    shard_seeds = np.random.default_rng(S + 50).integers(
        0, 1 << 32, n, dtype=np.uint32)
    rig42.load(host)
    for seeds, ref_seeds in ((shard_seeds, shard_seeds), (None, M32)):
        want = cases.chain_ref(host, ref_seeds)
        # the reference rows are the hash of the concatenation, literally
        for s in sorted({0, S // 2, S - 1}):
            cat = host[:s + 1].transpose(1, 0, 2).reshape(n, -1)
            assert np.array_equal(cases.crc_many(ref_seeds, cat), want[s])
        got = rig42.crc(seeds=seeds, chain=True)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # chaining stripe by stripe with in-place seeds ends at the same row
    run = np.broadcast_to(shard_seeds, (1, n)).copy()
    d_run = rig42.ctx.dbuf_alloc(4 * n)
    try:
        rig42.ctx.upload(d_run, run)
        for s in range(S):
            at = ctypes.c_void_p(rig42.d.value + s * n * C)
            run = rig42.ctx.crc32c_batch(at, 1, C, seeds=d_run, d_crc=d_run)
        want = cases.chain_ref(host, shard_seeds)
        assert np.array_equal(run[0], want[S - 1])
    finally:
        rig42.ctx.dbuf_free(d_run)


@gpu
def test_chain_masked_and_multi_block(rig42):
    S, n, C, mask = 3, rig42.n, B + 16, 0x15
    host = random_batch(S, n, C, seed=77)
    rig42.load(host)
    got = rig42.crc(chunk_mask=mask, chain=True)
    want = cases.chain_ref(host)
    for c in range(n):
        assert np.array_equal(got[:, c], want[:, c] if mask >> c & 1
                              else np.full(S, FILL, np.uint32)), c


# ---- the hash ignores the code ---------------------------------------------

@gpu
@pytest.mark.parametrize("tech,k,m,kw", [
    ("cauchy_good", 4, 3, {"packetsize": 32}),
    ("jerasure_reed_sol_van_w16", 4, 2, {}),
])
def test_every_technique_family(tech, k, m, kw):
    rig = Rig(k, m, tech, **kw)
    try:
        check_random(rig, 3, 8448, seed=k * m)
    finally:
        rig.close()


@gpu
def test_after_encode_on_the_same_slot(rig42):
    k, m, S, C = 4, 2, 5, B + 16
    host = random_batch(S, k + m, C, seed=0xE)
    flat = host.copy().reshape(-1)
    oracle.cpu_encode_batch(TECH, k, m, flat, S, C)
    want = cases.batch_ref(flat.reshape(S, k + m, C))
    rig42.load(host)  # parity columns still random
    rig42.fill()
    rig42.ctx.encode_batch(rig42.d, S, C, slot=1)
    got = rig42.crc(prefill=False, slot=1)
    assert np.array_equal(got, want)
    assert not np.array_equal(want[:, k:], cases.batch_ref(host)[:, k:])


@gpu
def test_deterministic_and_read_only(rig42):
    host = random_batch(7, rig42.n, 2 * B + 48, seed=3)
    rig42.load(host)
    a = rig42.crc()
    b = rig42.crc()
    assert np.array_equal(a, b) and np.array_equal(a, cases.batch_ref(host))
    assert np.array_equal(rig42.get(), host)


# ---- refusals --------------------------------------------------------------

def refused(rig, **kw):
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        rig.crc(**kw)
    assert (rig.words() == FILL).all(), kw


@gpu
def test_refusals(rig42):
    S, n, C = 3, rig42.n, 4112
    host = random_batch(S, n, C, seed=5)
    rig42.load(host)
    raw = ceph_amd.lib().ecx_crc32c_batch
    rig42.fill()
    assert raw(None, rig42.d, S, C, 0x3F, None, 0, rig42.d_crc, 0) == -22
    refused(rig42, dptr=None)
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        rig42.ctx.crc32c_batch(rig42.d, S, C, d_crc=ctypes.c_void_p(0))
    refused(rig42, slot=-1)
    refused(rig42, slot=2)  # n_streams is 2
    refused(rig42, C=0)
    refused(rig42, C=4104)
    refused(rig42, S=0)
    refused(rig42, S=-1)
    refused(rig42, S=65536)
    refused(rig42, chunk_mask=1 << n)
    refused(rig42, chunk_mask=1 << 63 | 1)

    def at(p, off):
        return ctypes.c_void_p(p.value + off)

    refused(rig42, d_crc=at(rig42.d_crc, 2))
    refused(rig42, seeds=at(rig42.d_seed, 1))
    refused(rig42, seeds=at(rig42.d_seed, 2), chain=True)
    for inside in (0, C, S * n * C - 4):  # words or seeds inside the batch
        refused(rig42, d_crc=at(rig42.d, inside))
        refused(rig42, seeds=at(rig42.d, inside))
        refused(rig42, seeds=at(rig42.d, inside), chain=True)
    # seeds that overlap the words without being them
    refused(rig42, seeds=at(rig42.d_crc, 4))
    refused(rig42, seeds=at(rig42.d_crc, 4 * n), chain=True)
    refused(rig42, seeds=rig42.d_crc, chain=True)
    refused(rig42, S=1, seeds=rig42.d_crc, chain=True)
    assert np.array_equal(rig42.get(), host)
    # and the same arguments, legal, are accepted
    assert np.array_equal(rig42.crc(slot=1), cases.batch_ref(host))


# ---- the plain-load instance (ECX_NT=0), in a process of its own -----------

def child():
    rig = Rig(4, 2)
    try:
        for S in (1, 3, 257):
            check_random(rig, S, 2 * B + 48, seed=S)
    finally:
        rig.close()
    print("CRC_CHILD_OK")


@gpu
def test_plain_load_instance():
    env = dict(os.environ, ECX_NT="0")
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CRC_CHILD_OK" in r.stdout, \
        r.stdout + r.stderr


if __name__ == "__main__":
    child()
