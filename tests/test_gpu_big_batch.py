"""Device batches past 4 GiB: every kernel family that forms a byte offset
into a batch, at k = 4, m = 2, C = 1 MiB + 16, S = 700 (4,404,086,400 bytes;
byte 2^31 lies in stripe 341, byte 2^32 in data chunk 3 of stripe 682). An
offset truncated to 32 bits does not fault: it lands at the start of the
batch. So each case downloads the stripes of cross_call_cases.big_sample
whole — the zone a wrapped offset lands in, the stripes around both lines
and every stripe past 2^32 — and compares them bit for bit with the host
reference, data chunks and everything else the call must not write included.

The batch is filled on the device (nothing of this size is uploaded) and the
data is checked against bench.expected_fill, which also covers
ec_fill_random_kernel past 2^32. One such buffer is alive at a time. Offsets
into d_new past 4 GiB, chain-mode CRC and the slices kernels (one pointer
per chunk, no batch offset) are out of scope: CROSS_CALL_COVERAGE.md.

Run as a script, this file is the child process of the ECX_STREAM=0 case."""
import ctypes
import functools
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
import oracle  # noqa: E402
import crc_cases  # noqa: E402
import cross_call_cases as cc  # noqa: E402
from decode_multi_cases import erased_of, mask_without  # noqa: E402
from test_gpu_verify import expected_word  # noqa: E402

pytestmark = pytest.mark.gpu

TECH = "reed_sol_van"
W16 = "jerasure_reed_sol_van_w16"
K, M, S, C = (cc.BIG[x] for x in "kmSC")
N = K + M
FULL = (1 << N) - 1


@functools.lru_cache(maxsize=None)
def sample(C=C):
    return cc.big_sample(S, N, C)


@functools.lru_cache(maxsize=None)
def w8_want():
    """The sampled stripes as filled and encoded; shared and read-only."""
    want = cc.encoded_stripes(TECH, K, M, sample()[0], C, cc.BIG_SEED)
    want.flags.writeable = False
    return want


# ---- the one big device buffer ---------------------------------------------

class Big:
    """Holds the one big device buffer that may be alive, with its context;
    asking for another family's frees it first."""

    def __init__(self):
        self.key = self.ctx = self.d = None

    def take(self, key, C, *ctx_args, **ctx_kw):
        if self.key != key:
            self.release()
            self.ctx = ceph_amd.EcContext(*ctx_args, device=0, **ctx_kw)
            self.d = self.ctx.dbuf_alloc(S * N * C)
            self.key, self.C = key, C
        return self.ctx, self.d

    def w8_encoded(self):
        """The w = 8 batch, filled and encoded anew: every case starts from
        the same bytes whatever ran before it."""
        ctx, d = self.take("w8", C, K, M, TECH)
        ctx.fill_random(d, S * N * C, cc.BIG_SEED)
        ctx.encode_batch(d, S, C)
        ctx.sync()
        return ctx, d

    def release(self):
        if self.ctx is not None:
            self.ctx.dbuf_free(self.d)
            self.ctx.close()
        self.key = self.ctx = self.d = None


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    b.release()


def at(d, s, c=0, off=0, C=C):
    return ctypes.c_void_p(d.value + (s * N + c) * C + off)


def get(ctx, d, stripes, C=C):
    """The given stripes, downloaded stripe by stripe."""
    out = np.zeros((len(stripes), N, C), np.uint8)
    for i, s in enumerate(stripes):
        ctx.download(out[i], at(d, s, C=C))
    return out


def dirty(ctx, d, stripes, erased_of_stripe, C=C):
    """Poison the erased chunks of the given stripes."""
    poison = np.full(C, cc.POISON, np.uint8)
    for s in stripes:
        for c in erased_of_stripe(s):
            ctx.upload(at(d, s, c, C=C), poison)
    # the poison is where the comparison will look: the last stripe's
    s, back = stripes[-1], np.zeros(C, np.uint8)
    for c in erased_of_stripe(s):
        ctx.download(back, at(d, s, c, C=C))
        assert np.array_equal(back, poison), (s, c)


def same(got, want, stripes, what):
    for i, s in enumerate(stripes):
        assert np.array_equal(got[i], want[i]), \
            (what, "stripe", s, "chunks",
             [c for c in range(N) if not np.array_equal(got[i, c], want[i, c])])


# ---- 1, 2: encode and decode, stream kernel and ec_gf_matmul_kernel ---------

def encode_decode_case(b):
    stripes = sample()[0]
    ctx, d = b.w8_encoded()
    # the data chunks are compared too: the fill kernel past 2^32
    same(get(ctx, d, stripes), w8_want(), stripes, "encode")
    # m = 2 rebuilds two chunks per call: chunks 1, 3 and 5 in two calls,
    # chunk 3 (the one the 2^32 line cuts) in both
    for erased in ((1, 3), (3, 5)):
        dirty(ctx, d, stripes, lambda s: erased)
        ctx.decode_batch(d, S, C, mask_without(N, erased))
        ctx.sync()
        same(get(ctx, d, stripes), w8_want(), stripes, f"decode {erased}")


def test_encode_decode_stream_kernel(big):
    """The control: bench.py runs this kernel past 4 GiB too."""
    encode_decode_case(big)


def test_encode_decode_table_kernel(big):
    """ECX_STREAM=0: ec_gf_matmul_kernel, stripes on blockIdx.y. The knob is
    read once per process, hence the child; the parent's buffer is freed
    first."""
    big.release()
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("ECX_STREAM")}
    env["ECX_STREAM"] = "0"
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BIG_OK" in r.stdout, r.stdout + r.stderr


def child():
    b = Big()
    try:
        encode_decode_case(b)
    finally:
        b.release()
    print("BIG_OK")


# ---- 3: decode_batch_multi ---------------------------------------------------

def test_decode_batch_multi(big):
    stripes, lines, _ = sample()
    masks = cc.big_decode_masks(S, N, stripes, lines)
    s32, c32, _ = lines[cc.LINE32]
    assert c32 in erased_of(N, masks[s32])
    assert len(erased_of(N, masks[S - 1])) == 2
    assert all(1 <= len(erased_of(N, masks[s])) <= 2 for s in stripes)
    ctx, d = big.w8_encoded()
    dirty(ctx, d, stripes, lambda s: erased_of(N, masks[s]))
    ctx.decode_batch_multi(d, S, C, masks)
    ctx.sync()
    same(get(ctx, d, stripes), w8_want(), stripes, "decode_batch_multi")


# ---- 4: update_batch ---------------------------------------------------------

def test_update_batch(big):
    """d_new is a second, small buffer: offsets into d_new past 4 GiB are
    out of scope."""
    stripes, lines, _ = sample()
    masks = cc.big_write_masks(S, K, stripes, lines)
    assert all(masks[s] for s in stripes)
    assert masks[lines[cc.LINE32][0]] >> lines[cc.LINE32][1] & 1
    total_new = cc.new_bases(masks)[1]
    assert total_new * C < 1 << 31
    # unwritten stripes next to the sampled zones: they must stay as they are
    quiet = [next(s for s in range(lo, S) if not masks[s])
             for lo in (19, 343, 600)]
    quiet_want = cc.encoded_stripes(TECH, K, M, quiet, C, cc.BIG_SEED)
    want = cc.updated_stripes(TECH, K, M, stripes, C, w8_want(), masks,
                              cc.BIG_NEW_SEED)
    ctx, d = big.w8_encoded()
    d_new = ctx.dbuf_alloc(total_new * C)
    try:
        ctx.fill_random(d_new, total_new * C, cc.BIG_NEW_SEED)
        ctx.update_batch(d, S, C, d_new, masks)
        ctx.sync()
        same(get(ctx, d, stripes), want, stripes, "update_batch")
        same(get(ctx, d, quiet), quiet_want, quiet, "update_batch, mask 0")
    finally:
        ctx.dbuf_free(d_new)


# ---- 5: verify_batch ---------------------------------------------------------

def test_verify_batch(big):
    stripes, lines, _ = sample()
    s31 = lines[cc.LINE31][0]
    s32, c32, o32 = lines[cc.LINE32]
    assert (s31, s32, c32) == (341, 682, 3) and 0 < o32 < C
    want = w8_want()
    ctx, d = big.w8_encoded()
    d_bad = ctx.dbuf_alloc(8 * S)

    def put(s, c, off, flip):
        """16-byte upload of the vector around one byte, flipped or as
        encoded."""
        lo = off & ~15
        vec = want[stripes.index(s), c, lo:lo + 16].copy()
        if flip:
            vec[off - lo] ^= 0x40
        ctx.upload(at(d, s, c, lo), vec)

    def verify():
        ctx.upload(d_bad, np.full(S, 0xFFFFFFFFFFFFFFFF, np.uint64))
        return ctx.verify_batch(d, S, C, FULL, d_bad)

    def reference(flips):
        """Unflipped stripes are as encoded (the two cases above hold the
        sampled ones against the host): their word is 0. A flipped stripe's
        word comes from the oracle's rebuild."""
        ref = np.zeros(S, np.uint64)
        for s in {f[0] for f in flips}:
            st = want[stripes.index(s)].copy()
            for fs, c, off in flips:
                if fs == s:
                    st[c, off] ^= 0x40
            ref[s] = expected_word(TECH, K, M, list(st), FULL)
        return ref

    try:
        words = verify()
        assert not words.any(), np.flatnonzero(words)
        # the last byte before the 2^32 line, then the first byte after it
        for off in (o32 - 1, o32):
            flips = [(s31, 4, C // 2), (s32, c32, off), (s32 + 1, 5, 0),
                     (S - 1, 5, C - 1)]
            for f in flips:
                put(*f, flip=True)
            ref = reference(flips)
            assert [int(ref[f[0]]) for f in flips] == [16, 48, 32, 32]
            words = verify()
            assert np.array_equal(words, ref), \
                (off, np.flatnonzero(words != ref), words[words != ref])
            for f in flips:
                put(*f, flip=False)
        assert not verify().any()
    finally:
        ctx.dbuf_free(d_bad)


# ---- 6: crc32c_batch ---------------------------------------------------------

def test_crc32c_batch(big):
    """chain = 0, no seeds, all six chunks. Chain mode is left out: its
    reference would hash 4 GiB in numpy."""
    stripes = sample()[0]
    prefill = 0xDEADBEEF
    ref = crc_cases.crc_many(0xFFFFFFFF, w8_want().reshape(-1, C)).reshape(
        len(stripes), N)
    ctx, d = big.w8_encoded()
    d_crc = ctx.dbuf_alloc(4 * S * N)
    try:
        ctx.upload(d_crc, np.full(S * N, prefill, np.uint32))
        words = ctx.crc32c_batch(d, S, C, FULL, None, False, d_crc)
    finally:
        ctx.dbuf_free(d_crc)
    assert np.array_equal(words[stripes], ref), \
        np.argwhere(words[stripes] != ref)
    assert (words != prefill).all(), np.argwhere(words == prefill)


# ---- 7: w = 16 ----------------------------------------------------------------

def test_w16_encode(big):
    stripes = sample()[0]
    want = cc.filled_stripes(stripes, N, C, cc.BIG_SEED).copy()
    for st in want:
        par = oracle.encode_w16(K, M, [st[i] for i in range(K)])
        for r in range(M):
            st[K + r] = par[r]
    ctx, d = big.take("w16", C, K, M, W16)
    ctx.fill_random(d, S * N * C, cc.BIG_SEED)
    ctx.encode_batch(d, S, C)
    ctx.sync()
    same(get(ctx, d, stripes), want, stripes, "w16 encode")


# ---- 8: the bitmatrix kernels -------------------------------------------------

def test_cauchy_orig_encode_decode(big):
    """Encode and the two-erasure decode take the LDS kernel, the one-erasure
    decode the register kernel; the pipelined kernel runs only under its
    knob (test_gpu_bitmatrix_knobs.py) and shares ecx_bit_glds and
    ecx_bit_rows, where the offsets are formed, with the LDS kernel."""
    Cb, pkt = cc.BIG_BIT["C"], cc.BIG_BIT["pkt"]
    stripes, lines, unchecked = sample(Cb)
    assert not unchecked
    assert lines[cc.LINE31][0] == 341 and lines[cc.LINE32][:2] == (682, 3)
    n_ops = int(np.count_nonzero(oracle.bitmatrix(
        oracle.cauchy_orig_matrix(K, M))))
    # which kernel a call takes does not depend on the op count (only the
    # LDS kernels bound it, at 65535); the decodes are given a full matrix's
    probe = ceph_amd.bitmatrix_plan_probe
    assert probe(K, M, pkt, Cb, n_ops)["kernel"] == "lds"
    assert probe(K, 1, pkt, Cb, 64 * K)["kernel"] == "reg"
    assert probe(K, 2, pkt, Cb, 128 * K)["kernel"] == "lds"

    want = cc.filled_stripes(stripes, N, Cb, cc.BIG_SEED).copy()
    for st in want:
        par = oracle.bitmatrix_encode(K, M, [st[i] for i in range(K)], pkt)
        for r in range(M):
            st[K + r] = par[r]
    ctx, d = big.take("cauchy_orig", Cb, K, M, "cauchy_orig", packetsize=pkt)
    ctx.fill_random(d, S * N * Cb, cc.BIG_SEED)
    ctx.encode_batch(d, S, Cb)
    ctx.sync()
    same(get(ctx, d, stripes, Cb), want, stripes, "cauchy_orig encode")
    for erased in ((3,), (1, 5)):
        dirty(ctx, d, stripes, lambda s: erased, Cb)
        ctx.decode_batch(d, S, Cb, mask_without(N, erased))
        ctx.sync()
        same(get(ctx, d, stripes, Cb), want, stripes,
             f"cauchy_orig decode {erased}")


if __name__ == "__main__":
    child()
