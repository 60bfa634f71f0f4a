"""ecx_locate_batch / ecx_locate_chunks_host / ecx_repair_batch: which chunk
of an inconsistent stripe is the wrong one? Every expected word comes from
locate_cases.py, i.e. from the oracle alone: bit x of the culprit word is
expected exactly when x is present and the stripe is consistent without it.
Shapes are the smallest at which the kernels can go wrong: a tile is 256
lanes x 16 B = 4096 B of one chunk, so C = 4112 has a full tile and a 16-byte
tail tile.

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
    sys.path.insert(0, HERE)

import ceph_amd  # noqa: E402
import locate_cases as cases  # noqa: E402
from locate_cases import TECH, encoded_batch, expected, full  # noqa: E402

gpu = pytest.mark.gpu
FF = 0xFFFFFFFFFFFFFFFF


class Rig:
    """A context, a device batch and the two device word arrays, pre-filled
    with 0xFF bytes before every call."""

    def __init__(self, k, m, tech=TECH, rows=None, **kw):
        self.k, self.m, self.tech = k, m, tech
        self.ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
        if rows is not None:
            self.ctx.set_matrix(rows)
        self.d = self.d_bad = self.d_cul = None
        self.nbytes = self.S = 0

    def load(self, host):
        host = np.ascontiguousarray(host)
        if self.d is None or host.nbytes != self.nbytes or \
                host.shape[0] != self.S:
            self.free()
            self.nbytes, self.S = host.nbytes, host.shape[0]
            self.d = self.ctx.dbuf_alloc(self.nbytes)
            # one allocation, so that the arrays can be made to overlap
            self.d_words = self.ctx.dbuf_alloc(16 * self.S)
            self.d_bad = ctypes.c_void_p(self.d_words.value)
            self.d_cul = ctypes.c_void_p(self.d_words.value + 8 * self.S)
        self.shape = host.shape
        self.ctx.upload(self.d, host)

    def get(self):
        out = np.zeros(self.shape, np.uint8)
        self.ctx.download(out, self.d)
        return out

    def fill_words(self):
        self.ctx.upload(self.d_words,
                        np.full(2 * self.S, FF, dtype=np.uint64))

    def read_words(self):
        out = np.zeros(2 * self.S, dtype=np.uint64)
        self.ctx.download(out, self.d_words)
        return out

    def _args(self, mask, S, C, d_bad, d_cul, slot):
        return (self.d, self.S if S is None else S,
                self.shape[2] if C is None else C, mask,
                self.d_bad if d_bad is None else d_bad,
                self.d_cul if d_cul is None else d_cul, slot)

    def locate(self, mask=None, S=None, C=None, d_bad=None, d_cul=None,
               slot=0):
        self.fill_words()
        return self.ctx.locate_batch(*self._args(mask, S, C, d_bad, d_cul,
                                                 slot))

    def repair(self, mask=None, S=None, C=None, d_bad=None, d_cul=None,
               slot=0):
        self.fill_words()
        return self.ctx.repair_batch(*self._args(mask, S, C, d_bad, d_cul,
                                                 slot))

    def verify(self, mask=None):
        return self.ctx.verify_batch(self.d, self.S, self.shape[2], mask)

    def free(self):
        if self.d is not None:
            self.ctx.dbuf_free(self.d)
            self.ctx.dbuf_free(self.d_words)
            self.d = self.d_bad = self.d_cul = None

    def close(self):
        self.free()
        self.ctx.close()


def check(rig, host, mask=None, **kw):
    """locate on host under mask; both arrays equal the reference on every
    stripe and the batch is unchanged. Returns the reference."""
    m_ = full(rig.k, rig.m) if mask is None else mask
    rig.load(host)
    bad, cul = rig.locate(mask, **kw)
    want_bad, want_cul = expected(rig.tech, rig.k, rig.m, host, m_)
    print(f"mask {m_:#x}: bad {bad} culprit {cul}; want {want_bad} "
          f"{want_cul}")
    assert bad.dtype == np.uint64 and cul.dtype == np.uint64
    assert np.array_equal(bad, want_bad), (hex(m_), bad, want_bad)
    assert np.array_equal(cul, want_cul), (hex(m_), cul, want_cul)
    assert np.array_equal(rig.get(), host), "the batch was written"
    return want_bad, want_cul


@pytest.fixture
def rig42():
    r = Rig(4, 2)
    yield r
    r.close()


# ---- 1. clean --------------------------------------------------------------

@gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [16, 48, 4096, 4112, 12272])
def test_clean_batch(rig42, C, S):
    host = encoded_batch(TECH, 4, 2, S, C, seed=C + S)
    rig42.load(host)
    bad, cul = rig42.locate()
    assert bad.shape == (S,) and cul.shape == (S,)
    assert not bad.any(), bad
    assert (cul == 0x3F).all(), cul
    assert np.array_equal(rig42.get(), host), "the batch was written"


# ---- 2. one chunk damaged --------------------------------------------------

_BASE = {}


def base42():
    if "h" not in _BASE:
        _BASE["h"] = encoded_batch(TECH, 4, 2, 3, 4112, seed=0xF1)
        _BASE["h"].setflags(write=False)
    return _BASE["h"]


@gpu
@pytest.mark.parametrize("chunk", range(6))
@pytest.mark.parametrize("off", [0, 4095, 4096, 4111])
def test_one_damaged_chunk(rig42, off, chunk):
    """Tile edges and the 16-byte tail tile, every chunk; stripe 1 only."""
    host = base42().copy()
    host[1, chunk, off] ^= 1 << (off % 8)
    bad, cul = check(rig42, host)
    assert bad[1] != 0 and list(cul) == [0x3F, 1 << chunk, 0x3F]


# ---- 3. across tiles -------------------------------------------------------

@gpu
def test_across_tiles(rig42):
    """A stripe's word gathers every tile of the stripe: damage to one chunk
    in both tiles is still located; damage to two chunks, one per tile, is
    not. A kernel that judged each tile alone would locate both."""
    for chunk in (1, 4):
        host = base42().copy()
        host[1, chunk, 5] ^= 0x11
        host[1, chunk, 4100] ^= 0x80
        _, cul = check(rig42, host)
        assert list(cul) == [0x3F, 1 << chunk, 0x3F]
    for x, y in ((0, 2), (1, 5), (4, 5), (4, 3)):
        host = base42().copy()
        host[1, x, 5] ^= 0x11
        host[1, y, 4100] ^= 0x80
        bad, cul = check(rig42, host)
        assert bad[1] != 0 and list(cul) == [0x3F, 0, 0x3F], (x, y)


# ---- 4. degraded masks -----------------------------------------------------

@gpu
@pytest.mark.parametrize("tech", ["reed_sol_van", "cauchy"])
def test_degraded_masks(tech):
    k, m, S, C = 4, 3, 3, 4112
    n = k + m
    base = encoded_batch(tech, k, m, S, C, seed=0xD6)
    rng = np.random.default_rng(0xD7)
    by_bits = {b: [mk for mk in range(1 << n) if bin(mk).count("1") == b]
               for b in range(n + 1)}
    kinds = set()
    rig = Rig(k, m, tech)
    try:
        assert len(by_bits[6]) + len(by_bits[7]) == 8
        for i, mask in enumerate(by_bits[7] + by_bits[6]):
            host = base.copy()
            # stripe 0 clean; one random byte in stripe 1 in a chunk drawn
            # from the whole stripe, absent chunks included, and in stripe 2
            # in a chunk that walks the stripe so that every kind occurs
            present = [c for c in range(n) if mask >> c & 1]
            chunks = (int(rng.integers(n)), (3 * i + 1) % n)
            want = [mask]
            for s, chunk in zip((1, 2), chunks):
                host[s, chunk, int(rng.integers(C))] ^= \
                    int(rng.integers(1, 256))
                want.append(1 << chunk if chunk in present else mask)
            kinds.add("absent" if chunks[1] not in present else
                      "survivor" if chunks[1] in present[:k] else "checked")
            _, cul = check(rig, host, mask)
            assert list(cul) == want, (hex(mask), chunks)
        assert kinds == {"absent", "survivor", "checked"}
        rig.load(base)
        for bits in range(6):
            for mask in by_bits[bits]:
                refused(rig, "EINVAL" if bits >= k else "EIO", mask=mask)
    finally:
        rig.close()


# ---- 5. more than four checked chunks --------------------------------------

@gpu
def test_two_passes():
    """m = 6: the base checks 4..7 and 8, 9 in two passes; each candidate
    checks five chunks, 5..8 and 9, in two."""
    k, m, S, C = 4, 6, 2, 4112
    base = encoded_batch(TECH, k, m, S, C, seed=0x26)
    rig = Rig(k, m)
    try:
        host = base.copy()
        host[0, 2, 33] ^= 0x01
        bad, cul = check(rig, host)
        assert list(bad) == [0x3F << 4, 0] and list(cul) == [1 << 2, 0x3FF]

        host = base.copy()
        host[1, 9, 4097] ^= 0x80
        bad, cul = check(rig, host)
        assert list(bad) == [0, 1 << 9] and list(cul) == [0x3FF, 1 << 9]

        host[1, 2, 33] ^= 0x01
        bad, cul = check(rig, host)
        assert list(bad) == [0, 0x3F << 4] and list(cul) == [0x3FF, 0]
    finally:
        rig.close()


# ---- 6. k = 32 -------------------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [16, 4112])
def test_k32(C):
    k, m, S = 32, 4, 2
    base = encoded_batch(TECH, k, m, S, C, seed=0x32 + C)
    rig = Rig(k, m)
    try:
        for chunk in (31, 35):
            host = base.copy()
            host[1, chunk, C - 1] ^= 0x10
            _, cul = check(rig, host)
            assert list(cul) == [full(k, m), 1 << chunk]
    finally:
        rig.close()


# ---- 7. more flagged tiles than blocks -------------------------------------

def check_many_flagged(S):
    host, want_bad, want_cul = cases.many_flagged(S)
    rig = Rig(8, 3)
    try:
        rig.load(host)
        bad, cul = rig.locate()
        for got, want in ((bad, want_bad), (cul, want_cul)):
            assert np.array_equal(got, want), \
                (np.flatnonzero(got != want)[:20], got[got != want][:20])
    finally:
        rig.close()
    return want_bad, want_cul


@gpu
def test_more_flagged_tiles_than_blocks():
    """1200 stripes, 1028 of them flagged, two tiles each: 2056 flagged
    tiles per candidate pass against a grid that cannot exceed what stays
    resident, so blocks walk on through the list. Every word of both arrays
    is compared."""
    bad, cul = check_many_flagged(1200)
    one = (cul & (cul - np.uint64(1))) == 0
    assert int((bad == 0).sum()) == 172
    assert int(((bad != 0) & (cul == 0)).sum()) == 79
    assert int(((bad != 0) & (cul != 0) & one).sum()) == 949
    assert (cul[bad == 0] == full(8, 3)).all()


# ---- 8. knobs (one child process per setting) ------------------------------

KNOBS = [
    {"ECX_STREAM_ORDER": "1"},
    {"ECX_STREAM_BPC": "0"},
    {"ECX_STREAM_BPC": "3", "ECX_STREAM_ORDER": "1"},
    {"ECX_STREAM_W": "3"},
    {"ECX_STREAM_XCD": "0"},
    {"ECX_STREAM": "0"},
]


def child():
    check_many_flagged(300)
    k, m, S, C = 4, 3, 5, 4112
    host = encoded_batch("cauchy", k, m, S, C, seed=0x71)
    host[3, 6, 4111] ^= 2
    host[4, 1, 0] ^= 2
    host[2, 0, 9] ^= 2  # absent
    mask = 0b1111110  # chunk 0 absent: survivors 1, 2, 3, 4
    rig = Rig(k, m, "cauchy")
    try:
        _, cul = check(rig, host, mask)
        assert list(cul) == [mask, mask, mask, 1 << 6, 1 << 1]
    finally:
        rig.close()
    print("KNOBS_OK")


@gpu
@pytest.mark.parametrize("knobs", KNOBS,
                         ids=lambda d: ",".join(f"{k}={v}"
                                                for k, v in d.items()))
def test_locate_knob_setting(knobs):
    """The embedded verify passes follow the ECX_STREAM* settings; the
    result must not."""
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("ECX_STREAM")}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KNOBS_OK" in r.stdout, r.stdout + r.stderr


# ---- 9. refusals -----------------------------------------------------------

def refused(rig, match, **kw):
    """The call raises and leaves every pre-filled word of both arrays as it
    was."""
    with pytest.raises(ceph_amd.EcError, match=match):
        rig.locate(**kw)
    assert (rig.read_words() == FF).all(), kw


def off(p, n):
    return ctypes.c_void_p(p.value + n)


@gpu
def test_refusals_write_nothing(rig42):
    k, m, S, C = 4, 2, 3, 4112
    host = encoded_batch(TECH, k, m, S, C, seed=0xEF)
    rig42.load(host)
    r = rig42
    refused(r, "EIO", mask=0b000111)            # k - 1 present
    refused(r, "EINVAL", mask=0b011111)         # k + 1 present
    refused(r, "EINVAL", mask=0b110110)         # k present
    refused(r, "EINVAL", mask=1 << 6 | 0x3F)    # a bit at k + m
    refused(r, "EINVAL", mask=1 << 63 | 0x3F)
    refused(r, "EINVAL", C=24)
    refused(r, "EINVAL", C=0)
    refused(r, "EINVAL", S=0)
    refused(r, "EINVAL", S=65536)
    refused(r, "EINVAL", slot=-1)
    refused(r, "EINVAL", slot=2)                # n_streams is 2
    batch_end = S * (k + m) * C
    for which in ("d_bad", "d_cul"):
        mine = getattr(r, which)
        refused(r, "EINVAL", **{which: off(mine, 4)})   # not 8-byte aligned
        for inside in (0, C, batch_end - 8):            # inside the batch
            refused(r, "EINVAL", **{which: off(r.d, inside)})
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):  # NULL arrays
        ceph_amd._ck(ceph_amd.lib().ecx_locate_batch(
            r.ctx._h, r.d, S, C, 0x3F, None, r.d_cul, 0), "null d_bad")
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd._ck(ceph_amd.lib().ecx_locate_batch(
            r.ctx._h, r.d, S, C, 0x3F, r.d_bad, None, 0), "null d_culprit")
    # the two arrays equal, and overlapping by one word either way
    refused(r, "EINVAL", d_cul=r.d_bad)
    refused(r, "EINVAL", d_cul=off(r.d_bad, 8 * (S - 1)))
    refused(r, "EINVAL", d_bad=off(r.d_bad, 8), d_cul=off(r.d_bad, 8 * S))
    assert np.array_equal(r.get(), host)
    # and the same arguments, legal, are accepted
    bad, cul = r.locate(mask=0x3F, slot=1)
    assert not bad.any() and (cul == 0x3F).all()


@gpu
@pytest.mark.parametrize("tech", ["cauchy_orig", "jerasure_reed_sol_van_w16"])
def test_other_techniques_refused(tech):
    k, m, S, C = 4, 2, 2, 16384
    rig = Rig(k, m, tech)
    try:
        rig.load(np.zeros((S, k + m, C), dtype=np.uint8))
        refused(rig, "EINVAL")
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            rig.repair()
        assert (rig.read_words() == FF).all()
        chunks = [np.zeros(C, dtype=np.uint8) for _ in range(k + m)]
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            rig.ctx.locate_chunks(chunks)
    finally:
        rig.close()


# ---- 10. custom matrix -----------------------------------------------------

@gpu
def test_set_matrix_clears_the_plans():
    """A reed_sol_van context given the cauchy rows answers as the reference
    does for cauchy, also for masks it had planned before."""
    import oracle
    k, m, S, C = 4, 3, 2, 4112
    mask = 0b1111101
    host = encoded_batch("cauchy", k, m, S, C, seed=0xCA)
    host[1, 3, 4100] ^= 7
    rig = Rig(k, m, "reed_sol_van")
    try:
        rig.load(host)
        for mk in (None, mask):      # plans of the technique's own matrix
            bad, _ = rig.locate(mk)
            assert bad.all(), "a cauchy stripe is not a reed_sol_van stripe"
        rig.ctx.set_matrix(oracle.matrix("cauchy", k, m)[k:])
        for mk in (None, mask):
            rig.tech = "cauchy"
            _, cul = check(rig, host, mk)
            assert list(cul) == [full(k, m) if mk is None else mk, 1 << 3]
    finally:
        rig.close()


@gpu
def test_candidate_that_does_not_invert():
    """(2,2) with rows [[1,0],[1,1]]: chunk 2 is a copy of chunk 0. The full
    mask verifies (survivors 0, 1), but the candidate without chunk 1 has
    survivors {0, 2}: EIO, nothing written."""
    rows = np.array([[1, 0], [1, 1]], dtype=np.uint8)
    S, C = 2, 4112
    host = np.random.default_rng(0x22).integers(0, 256, (S, 4, C), np.uint8)
    host[:, 2] = host[:, 0]
    host[:, 3] = host[:, 0] ^ host[:, 1]
    rig = Rig(2, 2, rows=rows)
    try:
        rig.load(host)
        assert not rig.verify().any()
        refused(rig, "EIO")
        with pytest.raises(ceph_amd.EcError, match="EIO"):
            rig.repair()
        assert (rig.read_words() == FF).all()
        assert np.array_equal(rig.get(), host)
    finally:
        rig.close()


# ---- 11. host form ---------------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [16, 4112])
def test_host_form(C):
    k, m = 4, 3
    n = k + m
    base = encoded_batch(TECH, k, m, 1, C, seed=C)[0]
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        def chunks_of(a, absent=()):
            return [None if i in absent else a[i].copy() for i in range(n)]

        def want(a, mask):
            return (cases.expected_word(TECH, k, m, list(a), mask),
                    cases.culprits(TECH, k, m, list(a), mask))

        assert ctx.locate_chunks(chunks_of(base)) == (0, full(k, m))

        st = base.copy()
        st[2, C - 1] ^= 1                              # a survivor
        assert want(st, full(k, m)) == (0b111 << 4, 1 << 2)
        assert ctx.locate_chunks(chunks_of(st)) == want(st, full(k, m))

        st = base.copy()
        st[5, C // 2] ^= 0x21                          # a parity
        assert want(st, full(k, m)) == (1 << 5, 1 << 5)
        assert ctx.locate_chunks(chunks_of(st)) == want(st, full(k, m))

        # chunk 1 absent and passed as None: survivors 0, 2, 3, 4
        present = [i != 1 for i in range(n)]
        mask = full(k, m) & ~(1 << 1)
        st = base.copy()
        st[4, 5] ^= 0xFF
        assert want(st, mask) == (0b11 << 5, 1 << 4)
        assert ctx.locate_chunks(chunks_of(st, absent=(1,)), present) == \
            want(st, mask)
        assert ctx.locate_chunks(chunks_of(base, absent=(1,)), present) == \
            (0, mask)

        # a present chunk that is not given cannot be judged
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.locate_chunks(chunks_of(base, absent=(1,)))
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.locate_chunks(chunks_of(base, absent=(6,)), present)
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ctx.locate_chunks(chunks_of(base), [i < k + 1 for i in range(n)])
        with pytest.raises(ceph_amd.EcError, match="EIO"):
            ctx.locate_chunks(chunks_of(base), [i < k - 1 for i in range(n)])
    finally:
        ctx.close()


# ---- 12. two slots interleaved ---------------------------------------------

@gpu
def test_two_slots_interleaved():
    """Two batches of different sizes on two slots, enqueued alternately,
    one sync each at the end: the list of flagged stripes is per slot."""
    k, m, C = 4, 2, 4112
    hosts = []
    for S, seed in ((40, 1), (9, 2)):
        h = encoded_batch(TECH, k, m, S, C, seed=seed)
        for s in range(S):
            if s % 3 != seed:
                h[s, (s + seed) % 6, (37 * s) % C] ^= 0x04
        hosts.append(h)
    ctx = ceph_amd.EcContext(k, m, TECH, device=0, n_streams=2)
    bufs = []
    try:
        for h in hosts:
            d = ctx.dbuf_alloc(h.nbytes)
            w = ctx.dbuf_alloc(16 * h.shape[0])
            ctx.upload(d, h)
            bufs.append((d, w))
        lib = ceph_amd.lib()
        for _ in range(2):
            for slot, (h, (d, w)) in enumerate(zip(hosts, bufs)):
                S = h.shape[0]
                ceph_amd._ck(lib.ecx_locate_batch(
                    ctx._h, d, S, C, 0x3F, w,
                    ctypes.c_void_p(w.value + 8 * S), slot), "locate")
        for slot, (h, (d, w)) in enumerate(zip(hosts, bufs)):
            S = h.shape[0]
            ctx.sync(slot)
            got = np.zeros(2 * S, dtype=np.uint64)
            ctx.download(got, w, slot)
            want_bad, want_cul = expected(TECH, k, m, h, 0x3F)
            assert np.array_equal(got[:S], want_bad), slot
            assert np.array_equal(got[S:], want_cul), slot
            assert int((want_cul != 0x3F).sum()) > S // 2
    finally:
        for d, w in bufs:
            ctx.dbuf_free(d)
            ctx.dbuf_free(w)
        ctx.close()


# ---- 13. repair ------------------------------------------------------------

def repair_case(base):
    host = base.copy()
    host[1, 2, 100] ^= 0x5A       # a survivor
    host[2, 5, 4000] ^= 0x01      # a parity
    host[3, 0, 7] ^= 0x10         # two chunks: not locatable
    host[3, 6, 4101] ^= 0x10
    host[5, 3, 4105] ^= 0xFF      # a data chunk, in the tail tile
    return host


@gpu
def test_repair():
    k, m, S, C = 4, 3, 6, 4112
    base = encoded_batch(TECH, k, m, S, C, seed=0x4E)
    host = repair_case(base)
    rig = Rig(k, m)
    try:
        rig.load(host)
        want_bad, want_cul = expected(TECH, k, m, host, full(k, m))
        bad, cul, n_rep, n_unl = rig.repair()
        assert np.array_equal(bad, want_bad)
        assert np.array_equal(cul, want_cul)
        assert list(cul) == [0x7F, 1 << 2, 1 << 5, 0, 0x7F, 1 << 3]
        assert (n_rep, n_unl) == (3, 1)
        after = rig.get()
        for s in (1, 2, 5):
            assert np.array_equal(after[s], base[s]), s
        for s in (0, 3, 4):
            assert np.array_equal(after[s], host[s]), s
        words = rig.verify()
        assert list(np.flatnonzero(words)) == [3]
        # nothing located: the counts say so and nothing is written
        bad, cul, n_rep, n_unl = rig.repair()
        assert (n_rep, n_unl) == (0, 1) and list(np.flatnonzero(bad)) == [3]
        assert np.array_equal(rig.get(), after)

        # chunk 1 absent and holding garbage everywhere
        mask = full(k, m) & ~(1 << 1)
        host2 = host.copy()
        host2[:, 1] = np.random.default_rng(9).integers(0, 256, (S, C),
                                                        np.uint8)
        rig.load(host2)
        want_bad, want_cul = expected(TECH, k, m, host2, mask)
        bad, cul, n_rep, n_unl = rig.repair(mask)
        assert np.array_equal(bad, want_bad)
        assert np.array_equal(cul, want_cul)
        assert list(cul) == [mask, 1 << 2, 1 << 5, 0, mask, 1 << 3]
        assert (n_rep, n_unl) == (3, 1)
        after = rig.get()
        for s in (1, 2, 5):
            assert np.array_equal(after[s], base[s]), s
        for s in (0, 3, 4):
            assert np.array_equal(after[s], host2[s]), s
    finally:
        rig.close()


if __name__ == "__main__":
    child()
