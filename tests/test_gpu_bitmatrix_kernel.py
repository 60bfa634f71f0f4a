"""The bitmatrix kernels (ec_bitmatrix_kernel, ec_bitmatrix_reg_kernel)
behind cauchy_orig and cauchy_good at the launcher's default knobs: every
case is bit-exact against bitmatrix_cases.ref_bit, the packet-XOR gather of
the oracle's bit matrix, at the smallest shapes where the window walk, the
staging paths, the template instances or the row tables can go wrong
(bitmatrix_cases.LDS_SHAPES and what test_kernel_references.py derives for
them). A batch sits between two 4 KiB poison guards in its device buffer and
its outputs start as poison; the guards and every source chunk must come
back unchanged."""
import ctypes

import numpy as np
import pytest

import ceph_amd
import bitmatrix_cases as cases

pytestmark = pytest.mark.gpu

POISON = cases.POISON
GUARD = 4096
ORIG = "cauchy_orig"


class Guarded:
    """A device copy of a host batch with a poison guard on either side;
    .d is the pointer the calls get."""

    def __init__(self, ctx, host):
        self.ctx, self.shape, self.n = ctx, host.shape, host.nbytes
        img = np.full(self.n + 2 * GUARD, POISON, np.uint8)
        img[GUARD:GUARD + self.n] = host.reshape(-1)
        self.raw = ctx.dbuf_alloc(img.nbytes)
        ctx.upload(self.raw, img)
        self.d = ctypes.c_void_p(self.raw.value + GUARD)

    def get(self):
        img = np.zeros(self.n + 2 * GUARD, np.uint8)
        self.ctx.download(img, self.raw)
        assert (img[:GUARD] == POISON).all(), "bytes before the batch changed"
        assert (img[-GUARD:] == POISON).all(), "bytes after the batch changed"
        return img[GUARD:GUARD + self.n].reshape(self.shape).copy()

    def free(self):
        self.ctx.dbuf_free(self.raw)


def check_encode(ctx, want, k, what):
    """Encode want's data on the device over poisoned outputs."""
    S, n, C = want.shape
    host = want.copy()
    host[:, k:, :] = POISON
    dev = Guarded(ctx, host)
    try:
        ctx.encode_batch(dev.d, S, C)
        got = dev.get()
    finally:
        dev.free()
    assert np.array_equal(got[:, :k], want[:, :k]), ("data changed", what)
    assert np.array_equal(got, want), what


def check_decode(ctx, full, erased, what):
    """Erased chunks are poisoned, decoded in place on the device; the whole
    batch must come back equal to the reference-encoded one."""
    S, n, C = full.shape
    host = full.copy()
    for e in erased:
        host[:, e, :] = POISON
    dev = Guarded(ctx, host)
    try:
        ctx.decode_batch(dev.d, S, C, cases.mask_without(n, erased))
        got = dev.get()
    finally:
        dev.free()
    assert np.array_equal(got, full), (what, erased)


@pytest.mark.parametrize("tech,k,m,pkt,n_sw", cases.encode_cases())
def test_encode_shapes_and_output_counts(tech, k, m, pkt, n_sw):
    ctx = ceph_amd.EcContext(k, m, tech, device=0, packetsize=pkt)
    try:
        for S in cases.STRIPES:
            check_encode(ctx, cases.encoded_bit(tech, k, m, pkt, n_sw, S), k,
                         (tech, k, m, pkt, n_sw, S))
    finally:
        ctx.close()


@pytest.mark.parametrize("k,pkt,n_sw", list(cases.LDS_SHAPES))
def test_decode_each_shape(k, pkt, n_sw):
    """Per shape at m = 3: only parities lost, only data lost, three lost."""
    ctx = ceph_amd.EcContext(k, 3, ORIG, device=0, packetsize=pkt)
    try:
        for S in cases.STRIPES:
            full = cases.encoded_bit(ORIG, k, 3, pkt, n_sw, S)
            for er in cases.shape_decode_patterns(k):
                check_decode(ctx, full, er, (k, pkt, n_sw, S))
    finally:
        ctx.close()


@pytest.mark.parametrize("S", cases.STRIPES)
def test_decode_every_pattern_k4_m3(S):
    k, m, pkt, n_sw = 4, 3, 48, 5
    full = cases.encoded_bit(ORIG, k, m, pkt, n_sw, S)
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        for er in cases.patterns(k + m, 3):
            check_decode(ctx, full, er, (k, m, pkt, S))
    finally:
        ctx.close()


@pytest.mark.parametrize("pkt,n_sw", [(48, 5), (2048, 3)])
@pytest.mark.parametrize("erased", cases.PATTERNS_48,
                         ids=lambda e: f"lose{len(e)}")
def test_decode_five_and_eight_outputs(erased, pkt, n_sw):
    k, m = 4, 8
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        for S in cases.STRIPES:
            check_decode(ctx, cases.encoded_bit(ORIG, k, m, pkt, n_sw, S),
                         erased, (k, m, pkt, S))
    finally:
        ctx.close()


@pytest.mark.parametrize("k,m,pkt,n_sw", cases.REG_SHAPES)
def test_register_kernel_single_erasure(k, m, pkt, n_sw):
    """One output: the register kernel. Every chunk lost in turn."""
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        for S in cases.STRIPES:
            full = cases.encoded_bit(ORIG, k, m, pkt, n_sw, S)
            for e in range(k + m):
                check_decode(ctx, full, (e,), (k, m, pkt, S))
    finally:
        ctx.close()


def check_delta(ctx, rows, k, pkt, n_sw, data, coding, seed):
    """parity ^= block(coding, data) . delta, parity random to begin with."""
    C = n_sw * 8 * pkt
    buf = cases.rand_batch(seed, 1, 2, C)  # chunk 0 the delta, 1 the parity
    delta, parity = buf[0, 0].copy(), buf[0, 1].copy()
    j = coding - k
    cases.ref_bit(buf, [0], [1],
                  rows[8 * j:8 * j + 8, 8 * data:8 * data + 8], pkt,
                  accum=True)
    got = ctx.apply_delta(delta, data, coding, parity)
    assert np.array_equal(got, buf[0, 1]), (pkt, n_sw, data, coding)
    assert np.array_equal(delta, buf[0, 0]), "delta changed"


@pytest.mark.parametrize("k,m,pkt,n_sw", cases.REG_SHAPES)
def test_register_kernel_apply_delta_every_pair(k, m, pkt, n_sw):
    rows = cases.encode_rows(ORIG, k, m)
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        for data in range(k):
            for coding in range(k, k + m):
                check_delta(ctx, rows, k, pkt, n_sw, data, coding,
                            seed=pkt + 10 * data + coding)
    finally:
        ctx.close()


def test_host_path_nine_outputs_in_two_launches():
    """m = 9: the host path splits the outputs into launches of 8 and 1;
    then a decode that loses four chunks."""
    h = cases.HOST_PATH
    k, m, pkt = h["k"], h["m"], h["pkt"]
    full = cases.encoded_bit(ORIG, k, m, pkt, h["n_sw"], 1)[0]
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        out = [np.full(full.shape[1], POISON, np.uint8) for _ in range(m)]
        data = [full[i].copy() for i in range(k)]
        got = ctx.encode_chunks(data, out=out)
        for i in range(k):
            assert np.array_equal(data[i], full[i]), i
        for j in range(m):
            assert np.array_equal(got[j], full[k + j]), j
        present = [i not in h["erased"] for i in range(k + m)]
        chunks = [full[i].copy() if present[i]
                  else np.full(full.shape[1], POISON, np.uint8)
                  for i in range(k + m)]
        ctx.decode_chunks(chunks, present)
        for i in range(k + m):
            assert np.array_equal(chunks[i], full[i]), i
    finally:
        ctx.close()


@pytest.mark.parametrize("k,m,tech,pkt", [(4, 3, ORIG, 8), (4, 3, ORIG, 24),
                                          (17, 3, ORIG, 2048),
                                          (4, 2, "cauchy_good", 2048)])
def test_refused_contexts(k, m, tech, pkt):
    with pytest.raises(ceph_amd.EcError):
        ceph_amd.EcContext(k, m, tech, device=0, packetsize=pkt).close()


def test_refused_chunk_size_leaves_the_context_working():
    """A chunk that is no multiple of 8 * pkt is refused by the batch and
    the host calls; the context still encodes correctly afterwards."""
    k, m, pkt, n_sw = 4, 3, 48, 5
    want = cases.encoded_bit(ORIG, k, m, pkt, n_sw, 3)
    S, n, C = want.shape
    ctx = ceph_amd.EcContext(k, m, ORIG, device=0, packetsize=pkt)
    try:
        bad = C - 16
        host = want[:, :, :bad].copy()
        dev = Guarded(ctx, host)
        try:
            with pytest.raises(ceph_amd.EcError):
                ctx.encode_batch(dev.d, S, bad)
            with pytest.raises(ceph_amd.EcError):
                ctx.decode_batch(dev.d, S, bad, cases.mask_without(n, (1,)))
            assert np.array_equal(dev.get(), host), "a refused call wrote"
        finally:
            dev.free()
        with pytest.raises(ceph_amd.EcError):
            ctx.encode_chunks([want[0, i, :bad].copy() for i in range(k)])
        check_encode(ctx, want, k, "after the refusals")
    finally:
        ctx.close()
