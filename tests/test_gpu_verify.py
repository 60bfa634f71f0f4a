"""ecx_verify_batch / ecx_verify_chunks_host: are the stored chunks of a
stripe consistent with each other? Every expected word comes from the oracle
alone (expected_word below): the stripe's survivors — the first k present
chunks — rebuild every other chunk through oracle.decode, and a checked chunk
is expected to be flagged exactly when its rebuild differs from what is
stored. The library's own rows are never used. Shapes are the smallest at
which the kernel can go wrong: a tile is 256 lanes x 16 B = 4096 B of one
chunk, so C = 4112 has a full tile and a 16-byte tail tile.

Run as a script, this file is the child process of the knob test."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child: no conftest has set the path
    sys.path.insert(0, os.path.dirname(HERE))

import ceph_amd  # noqa: E402
import oracle  # noqa: E402

gpu = pytest.mark.gpu
TECH = "reed_sol_van"
FF = 0xFFFFFFFFFFFFFFFF


# ---- the reference ---------------------------------------------------------

def expected_word(tech, k, m, stripe, mask):
    """stripe: k+m uint8 arrays as stored. Bit i is set exactly when i is in
    the mask, is not a survivor, and differs from its rebuild out of the
    survivors alone."""
    n = k + m
    present = [i for i in range(n) if mask >> i & 1]
    surv = present[:k]
    chunks = [np.ascontiguousarray(c).copy() for c in stripe]
    oracle.decode(tech, k, m, chunks, [int(i in surv) for i in range(n)])
    word = 0
    for i in present[k:]:
        if not np.array_equal(chunks[i], stripe[i]):
            word |= 1 << i
    return word


def expected_words(tech, k, m, host, mask, stripes=None):
    """host: (S, k+m, C). Words of the given stripes (default all); the
    others are 0 in the returned array."""
    want = np.zeros(host.shape[0], dtype=np.uint64)
    for s in (range(host.shape[0]) if stripes is None else stripes):
        want[s] = expected_word(tech, k, m, list(host[s]), mask)
    return want


def encoded_batch(tech, k, m, S, C, seed):
    """A consistent (S, k+m, C) batch, encoded by the oracle."""
    host = np.random.default_rng(seed).integers(
        0, 256, (S, k + m, C), dtype=np.uint8)
    flat = host.reshape(-1)
    oracle.cpu_encode_batch(tech, k, m, flat, S, C)
    return flat.reshape(S, k + m, C)


def full(k, m):
    return (1 << (k + m)) - 1


def test_reference_flags_nothing_on_an_encoded_stripe():
    """CPU only: the reference is silent on oracle-encoded stripes under
    full and degraded masks, speaks when a byte is changed, and splits a
    mask into survivors and checked chunks as the library's planner does."""
    for tech, k, m in ((TECH, 4, 2), ("cauchy", 4, 3), (TECH, 8, 3)):
        host = encoded_batch(tech, k, m, 2, 4112, seed=k * m)
        n = k + m
        for mask in (full(k, m), full(k, m) & ~1, full(k, m) & ~(1 << k),
                     full(k, m) >> 1 << 1 & ~(1 << (n - 1))):
            if bin(mask).count("1") < k:
                continue
            assert not expected_words(tech, k, m, host, mask).any()
            # the reference's split of the mask is the library's (ids only:
            # the library's rows take no part in any expectation)
            present = [i for i in range(n) if mask >> i & 1]
            sv, ck, _ = ceph_amd.verify_plan_probe(tech, k, m, mask)
            assert (list(sv), list(ck)) == (present[:k], present[k:])
        host[1, n - 1, 7] ^= 1
        assert list(expected_words(tech, k, m, host, full(k, m))) == \
            [0, 1 << (n - 1)]


# ---- device helpers --------------------------------------------------------

class Rig:
    """A context, a device batch and a device word array pre-filled with
    0xFF bytes before every call."""

    def __init__(self, k, m, tech=TECH, rows=None, **kw):
        self.k, self.m, self.tech = k, m, tech
        self.ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
        if rows is not None:
            self.ctx.set_matrix(rows)
        self.d = self.d_bad = None
        self.nbytes = self.S = 0

    def load(self, host):
        host = np.ascontiguousarray(host)
        if self.d is None or host.nbytes != self.nbytes or \
                host.shape[0] != self.S:
            self.free()
            self.nbytes, self.S = host.nbytes, host.shape[0]
            self.d = self.ctx.dbuf_alloc(self.nbytes)
            self.d_bad = self.ctx.dbuf_alloc(8 * self.S)
        self.shape = host.shape
        self.ctx.upload(self.d, host)

    def get(self):
        out = np.zeros(self.shape, np.uint8)
        self.ctx.download(out, self.d)
        return out

    def fill_bad(self):
        self.ctx.upload(self.d_bad, np.full(self.S, FF, dtype=np.uint64))

    def read_bad(self):
        out = np.zeros(self.S, dtype=np.uint64)
        self.ctx.download(out, self.d_bad)
        return out

    def verify(self, mask=None, S=None, C=None, d_bad=None, slot=0):
        self.fill_bad()
        return self.ctx.verify_batch(
            self.d, self.S if S is None else S,
            self.shape[2] if C is None else C, mask,
            self.d_bad if d_bad is None else d_bad, slot)

    def free(self):
        if self.d is not None:
            self.ctx.dbuf_free(self.d)
            self.ctx.dbuf_free(self.d_bad)
            self.d = self.d_bad = None

    def close(self):
        self.free()
        self.ctx.close()


@pytest.fixture
def rig42():
    r = Rig(4, 2)
    yield r
    r.close()


# ---- clean batches, single flipped bits ------------------------------------

@gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [16, 48, 4096, 4112, 12272])
def test_clean_batch_encoded_on_device(rig42, C, S):
    host = np.random.default_rng(C + S).integers(
        0, 256, (S, 6, C), dtype=np.uint8)
    rig42.load(host)
    rig42.ctx.encode_batch(rig42.d, S, C)
    rig42.ctx.sync()
    before = rig42.get()
    words = rig42.verify()
    assert words.dtype == np.uint64 and words.shape == (S,)
    assert not words.any(), words
    assert np.array_equal(rig42.get(), before), "the batch was written"


_FLIP_BASE = {}


def flip_base():
    if "h" not in _FLIP_BASE:
        _FLIP_BASE["h"] = encoded_batch(TECH, 4, 2, 3, 4112, seed=0xF1)
        _FLIP_BASE["h"].setflags(write=False)
    return _FLIP_BASE["h"]


@gpu
@pytest.mark.parametrize("chunk", [0, 3, 5])
@pytest.mark.parametrize("off", [0, 15, 16, 1023, 1024, 4095, 4096, 4111])
def test_one_flipped_bit(rig42, off, chunk):
    """Lane, wave and tile edges and the 16-byte tail tile, in a data chunk
    at either end and in a parity; stripe 1 only."""
    host = flip_base().copy()
    host[1, chunk, off] ^= 1 << (off % 8)
    rig42.load(host)
    words = rig42.verify()
    want = expected_word(TECH, 4, 2, list(host[1]), full(4, 2))
    print(f"chunk {chunk} off {off}: got {words}, want word1 {want:#x}")
    assert want != 0
    assert list(words) == [0, want, 0]
    assert np.array_equal(rig42.get(), host), "the batch was written"


# ---- coefficient classes ---------------------------------------------------

CLASS_ROWS = np.array([[0, 1, 7, 1, 200],
                       [1, 0, 1, 33, 2],
                       [9, 1, 0, 1, 1]], dtype=np.uint8)


@gpu
def test_coefficient_classes():
    """Custom rows with 0, 1 and general coefficients in every row. The
    oracle's decode knows the technique's matrix only, so the rebuild of
    the reference is oracle.encode_with_rows over the data chunks, which
    are the survivors of the full mask. A parity whose coefficient for the
    corrupted chunk is 0 must stay unflagged."""
    k, m, S, C = 5, 3, 2, 4112
    for r in range(m):
        assert {0, 1} < set(CLASS_ROWS[r].tolist()) and CLASS_ROWS[r].max() > 1
    host = np.random.default_rng(0xC1).integers(
        0, 256, (S, k + m, C), dtype=np.uint8)
    for s in range(S):
        par = oracle.encode_with_rows(
            CLASS_ROWS, [host[s, i].copy() for i in range(k)])
        for r in range(m):
            host[s, k + r] = par[r]
    rig = Rig(k, m, rows=CLASS_ROWS)
    try:
        rig.load(host)
        assert not rig.verify().any()
        for d in range(k):
            bad = host.copy()
            bad[1, d, 4100] ^= 0x5A
            rebuilt = oracle.encode_with_rows(
                CLASS_ROWS, [bad[1, i].copy() for i in range(k)])
            want = sum(1 << (k + r) for r in range(m)
                       if not np.array_equal(rebuilt[r], bad[1, k + r]))
            assert want == sum(1 << (k + r) for r in range(m)
                               if CLASS_ROWS[r, d] != 0)
            rig.load(bad)
            words = rig.verify()
            assert list(words) == [0, want], (d, words, want)
    finally:
        rig.close()


# ---- degraded masks --------------------------------------------------------

def degraded_case(tech, k, m, base, mask, rng):
    """Stripe 0 clean, stripe 1 with one byte changed in a chunk drawn from
    the whole stripe: a survivor, a checked chunk or an absent one."""
    host = base.copy()
    chunk = int(rng.integers(k + m))
    off = int(rng.integers(base.shape[2]))
    host[1, chunk, off] ^= int(rng.integers(1, 256))
    return host, chunk


@gpu
@pytest.mark.parametrize("tech", ["reed_sol_van", "cauchy"])
def test_degraded_masks(tech):
    k, m, S, C = 4, 3, 2, 4112
    base = encoded_batch(tech, k, m, S, C, seed=0xD6)
    rng = np.random.default_rng(0xD7)
    masks = [mk for mk in range(1 << (k + m)) if bin(mk).count("1") >= k]
    assert len(masks) == 64
    rig = Rig(k, m, tech)
    kinds = set()
    try:
        for mask in masks:
            host, chunk = degraded_case(tech, k, m, base, mask, rng)
            present = [i for i in range(k + m) if mask >> i & 1]
            kinds.add("absent" if chunk not in present else
                      "survivor" if chunk in present[:k] else "checked")
            rig.load(host)
            words = rig.verify(mask)
            want = expected_words(tech, k, m, host, mask)
            assert want[0] == 0
            assert np.array_equal(words, want), (hex(mask), chunk, words, want)
            if len(present) == k:
                assert not words.any(), hex(mask)
    finally:
        rig.close()
    assert kinds == {"absent", "survivor", "checked"}


# ---- more than one pass, k = 32 --------------------------------------------

@gpu
def test_two_passes():
    """m = 6: parities 4..7 in the first pass, 8 and 9 in the second."""
    k, m, S, C = 4, 6, 2, 4112
    base = encoded_batch(TECH, k, m, S, C, seed=0x26)
    rig = Rig(k, m)
    try:
        host = base.copy()
        host[1, 9, 4097] ^= 0x80
        rig.load(host)
        want = expected_words(TECH, k, m, host, full(k, m))
        assert list(want) == [0, 1 << 9]
        assert np.array_equal(rig.verify(), want)

        host = base.copy()
        host[0, 2, 33] ^= 0x01
        rig.load(host)
        want = expected_words(TECH, k, m, host, full(k, m))
        assert list(want) == [0x3F << 4, 0]
        assert np.array_equal(rig.verify(), want)
    finally:
        rig.close()


@gpu
@pytest.mark.parametrize("C", [16, 4112])
def test_argument_block_bound_k32(C):
    """k = 32 fills the source offsets and both class masks; the checked
    chunks must not need a source bit of their own."""
    k, m, S = 32, 4, 2
    base = encoded_batch(TECH, k, m, S, C, seed=0x32 + C)
    rig = Rig(k, m)
    try:
        rig.load(base)
        assert not rig.verify().any()
        for chunk in (31, 35):
            host = base.copy()
            host[1, chunk, C - 1] ^= 0x10
            rig.load(host)
            want = expected_words(TECH, k, m, host, full(k, m))
            assert want[0] == 0 and want[1] == \
                (0xF << 32 if chunk == 31 else 1 << 35)
            assert np.array_equal(rig.verify(), want), chunk
    finally:
        rig.close()


# ---- more tiles than blocks ------------------------------------------------

def many_tiles_case(S):
    """(8,3), C = 4112 (two tiles per chunk): bytes changed in the tail tile
    of the first, the middle and the last two stripes."""
    k, m, C = 8, 3, 4112
    host = encoded_batch(TECH, k, m, S, C, seed=0x83)
    hit = [0, S // 2 - 1, S - 2, S - 1]
    for n, s in enumerate(hit):
        host[s, (3 * n + 1) % (k + m), 4100] ^= 0x40 >> n
    # the reference runs on the changed stripes and two clean ones; the
    # other stripes are oracle-encoded and untouched
    want = expected_words(TECH, k, m, host, full(k, m),
                          stripes=hit + [1, S // 2])
    assert sorted(np.flatnonzero(want)) == hit
    return host, want


def check_many_tiles(S):
    host, want = many_tiles_case(S)
    rig = Rig(8, 3)
    try:
        rig.load(host)
        words = rig.verify()
        assert np.array_equal(words, want), \
            (np.flatnonzero(words != want), words[words != want])
    finally:
        rig.close()


@gpu
def test_more_tiles_than_blocks():
    """1200 stripes x 2 tiles = 2400 tiles: more than stay resident, so
    under a persistent grid blocks walk on; by default one block per tile."""
    check_many_tiles(1200)


# ---- knobs (one child process per setting) ---------------------------------

KNOBS = [
    {"ECX_STREAM_ORDER": "1"},
    {"ECX_STREAM_BPC": "0"},
    {"ECX_STREAM_BPC": "3", "ECX_STREAM_ORDER": "1"},
    {"ECX_STREAM_W": "3"},
    {"ECX_STREAM_XCD": "0"},
    {"ECX_STREAM": "0"},
]


def child():
    # 300 stripes x 2 tiles = 600 tiles: more than 3 blocks per CU hold, and
    # width 3 does not divide a walk step
    check_many_tiles(300)
    k, m, S, C = 4, 3, 5, 4112
    host = encoded_batch("cauchy", k, m, S, C, seed=0x71)
    host[3, 6, 4111] ^= 2
    host[4, 1, 0] ^= 2
    mask = 0b1110110  # chunks 0 and 3 absent: survivors 1, 2, 4, 5
    rig = Rig(k, m, "cauchy")
    try:
        rig.load(host)
        want = expected_words("cauchy", k, m, host, mask)
        assert want[3] == 1 << 6 and want[4] == 1 << 6 and not want[:3].any()
        assert np.array_equal(rig.verify(mask), want)
    finally:
        rig.close()
    print("KNOBS_OK")


@gpu
@pytest.mark.parametrize("knobs", KNOBS,
                         ids=lambda d: ",".join(f"{k}={v}"
                                                for k, v in d.items()))
def test_verify_knob_setting(knobs):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("ECX_STREAM")}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KNOBS_OK" in r.stdout, r.stdout + r.stderr


# ---- refusals --------------------------------------------------------------

def refused(rig, match, **kw):
    """The call raises and leaves every pre-filled word as it was."""
    with pytest.raises(ceph_amd.EcError, match=match):
        rig.verify(**kw)
    assert (rig.read_bad() == FF).all(), kw


@gpu
def test_refusals_write_nothing(rig42):
    k, m, S, C = 4, 2, 3, 4112
    host = encoded_batch(TECH, k, m, S, C, seed=0xEF)
    rig42.load(host)
    refused(rig42, "EIO", mask=0b000111)            # k - 1 present
    refused(rig42, "EINVAL", mask=1 << 6 | 0x3F)    # a bit at k + m
    refused(rig42, "EINVAL", mask=1 << 63 | 0x3F)
    refused(rig42, "EINVAL", C=24)
    refused(rig42, "EINVAL", C=0)
    refused(rig42, "EINVAL", S=0)
    refused(rig42, "EINVAL", S=65536)
    refused(rig42, "EINVAL", slot=-1)
    refused(rig42, "EINVAL", slot=2)                # n_streams is 2
    # word array not 8-byte aligned
    refused(rig42, "EINVAL", d_bad=ctypes.c_void_p(rig42.d_bad.value + 4))
    # a word array inside the batch: neither it nor the batch is written
    for inside in (0, C, S * (k + m) * C - 8):
        refused(rig42, "EINVAL", d_bad=ctypes.c_void_p(rig42.d.value + inside))
    assert np.array_equal(rig42.get(), host)
    # and the same arguments, legal, are accepted
    assert not rig42.verify(mask=0x3F, slot=1).any()


@gpu
@pytest.mark.parametrize("tech", ["cauchy_orig", "jerasure_reed_sol_van_w16"])
def test_other_techniques_refused(tech):
    k, m, S, C = 4, 2, 2, 16384
    rig = Rig(k, m, tech)
    try:
        rig.load(np.zeros((S, k + m, C), dtype=np.uint8))
        refused(rig, "EINVAL")
        chunks = [np.zeros(C, dtype=np.uint8) for _ in range(k + m)]
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            rig.ctx.verify_chunks(chunks)
    finally:
        rig.close()


# ---- host-pointer form -----------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [4096, 65536])
def test_host_form(C):
    k, m = 8, 3
    n = k + m
    base = encoded_batch(TECH, k, m, 1, C, seed=C)[0]
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        def chunks_of(a, absent=()):
            return [None if i in absent else a[i].copy() for i in range(n)]

        assert ctx.verify_chunks(chunks_of(base)) == 0

        bad = base.copy()
        bad[9, C - 1] ^= 1
        want = expected_word(TECH, k, m, list(bad), full(k, m))
        assert want == 1 << 9
        assert ctx.verify_chunks(chunks_of(bad)) == want

        bad = base.copy()
        bad[4, C // 2] ^= 0x21
        want = expected_word(TECH, k, m, list(bad), full(k, m))
        assert want == 0b111 << 8
        assert ctx.verify_chunks(chunks_of(bad)) == want

        # chunk 2 absent and passed as None: survivors 0, 1, 3..8, checked
        # 9 and 10; the changed byte sits in survivor 8
        bad = base.copy()
        bad[8, 5] ^= 0xFF
        present = [i != 2 for i in range(n)]
        mask = full(k, m) & ~(1 << 2)
        want = expected_word(TECH, k, m, list(bad), mask)
        assert want == 0b11 << 9
        assert ctx.verify_chunks(chunks_of(bad, absent=(2,)), present) == want
        assert ctx.verify_chunks(chunks_of(base, absent=(2,)), present) == 0

        # a present chunk that is not given cannot be vouched for
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.verify_chunks(chunks_of(base, absent=(2,)))
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.verify_chunks(chunks_of(base, absent=(10,)), present)
        with pytest.raises(ceph_amd.EcError, match="EIO"):
            ctx.verify_chunks(chunks_of(base), [i < k - 1 for i in range(n)])
    finally:
        ctx.close()


if __name__ == "__main__":
    child()
