"""The streaming kernel behind the non-accumulating device batch
calls (encode_batch / decode_batch / matmul_batch, w=8): every case is
bit-exact against the oracle's GF(2^8) arithmetic, at the smallest shapes
where the tile walk, the coefficient classes or the argument-block bounds
can go wrong. A tile is 256 lanes x 16 B = 4096 B of one chunk."""
from itertools import combinations

import numpy as np
import pytest

import ceph_amd
import oracle

pytestmark = pytest.mark.gpu

TECH = "reed_sol_van"
_MUL = None


def mul_table():
    """256 x 256 product table built once from the oracle's gf_mul."""
    global _MUL
    if _MUL is None:
        _MUL = np.array([[oracle.gf_mul(c, x) for x in range(256)]
                         for c in range(256)], dtype=np.uint8)
    return _MUL


def ref_matmul(buf, src_ids, out_ids, rows):
    """buf: (S, n, C) uint8, updated in place like the device batch:
    chunk out_ids[j] = XOR_i rows[j][i] * chunk src_ids[i], per stripe."""
    mul = mul_table()
    srcs = [buf[:, s, :].copy() for s in src_ids]
    for j, o in enumerate(out_ids):
        acc = np.zeros_like(srcs[0])
        for i, s in enumerate(srcs):
            acc ^= mul[int(rows[j][i])][s]
        buf[:, o, :] = acc


def rand_batch(seed, S, n, C):
    return np.random.default_rng(seed).integers(
        0, 256, (S, n, C), dtype=np.uint8)


class Dev:
    """A device copy of a host batch."""

    def __init__(self, ctx, host):
        self.ctx, self.n = ctx, host.nbytes
        self.d = ctx.dbuf_alloc(self.n)
        ctx.upload(self.d, np.ascontiguousarray(host))

    def get(self, shape):
        out = np.zeros(shape, np.uint8)
        self.ctx.download(out, self.d)
        return out

    def free(self):
        self.ctx.dbuf_free(self.d)


def run_encode(k, m, S, C, seed, rows=None):
    """Encode a random batch on the device; returns (got, want)."""
    n = k + m
    host = rand_batch(seed, S, n, C)  # parity region pre-dirtied
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        if rows is not None:
            ctx.set_matrix(rows)
        else:
            rows = oracle.matrix(TECH, k, m)[k:]
        want = host.copy()
        ref_matmul(want, list(range(k)), list(range(k, n)), rows)
        dev = Dev(ctx, host)
        ctx.encode_batch(dev.d, S, C)
        got = dev.get(host.shape)
        dev.free()
        return got, want
    finally:
        ctx.close()


def test_reference_is_the_oracle():
    """The table-driven reference above equals the oracle's own encode."""
    k, m, C = 5, 3, 256
    rows = np.random.default_rng(1).integers(0, 256, (m, k), dtype=np.uint8)
    buf = rand_batch(2, 1, k + m, C)
    want = oracle.encode_with_rows(rows, [buf[0, i].copy() for i in range(k)])
    ref_matmul(buf, list(range(k)), list(range(k, k + m)), rows)
    for j in range(m):
        assert np.array_equal(buf[0, k + j], want[j])


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [16, 48, 4096, 4112, 12272])
def test_tile_walk_small_and_partial(C, S):
    got, want = run_encode(4, 2, S, C, seed=C * 7 + S)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k,m,S,C", [(8, 3, 5000, 16), (8, 3, 1200, 4112),
                                     (4, 2, 800, 12272)])
def test_tile_walk_more_tiles_than_grid(k, m, S, C):
    """More tiles than blocks (the default grid gives a block two tiles
    once there are more than 8 per CU, and 2048 blocks are the most that
    stay resident): blocks walk on by the grid size. With 3 tiles per chunk
    the step is no multiple of a stripe, so the walk carries from the tile
    index into the stripe index."""
    n = k + m
    host = rand_batch(S ^ C, S, n, C)
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        dev = Dev(ctx, host)
        ctx.encode_batch(dev.d, S, C)
        got = dev.get(host.shape)
        dev.free()
    finally:
        ctx.close()
    assert np.array_equal(got[:, :k], host[:, :k]), "data chunks changed"
    pick = np.random.default_rng(32).choice(np.arange(1, S - 1), 32,
                                            replace=False)
    pick = np.concatenate(([0, S - 1], np.sort(pick)))
    want = host[pick].copy()
    ref_matmul(want, list(range(k)), list(range(k, n)),
               oracle.matrix(TECH, k, m)[k:])
    assert np.array_equal(got[pick], want)


def test_tile_walk_single_tile():
    got, want = run_encode(2, 1, 1, 4096, seed=11)
    assert np.array_equal(got, want)


def test_classes_mixed_rows_and_zero_row():
    """Rows mixing 0, 1 and general coefficients; the all-zero row must
    write zeros over the pre-dirtied output chunk."""
    k, m = 5, 4
    rows = np.array([[1, 0, 7, 1, 0xC3],
                     [0, 0, 0, 0, 0],
                     [0x8E, 1, 1, 0, 0],
                     [0, 0xFF, 0, 2, 1]], dtype=np.uint8)
    got, want = run_encode(k, m, 3, 4112, seed=5, rows=rows)
    assert np.array_equal(got, want)
    assert not got[:, k + 1].any()


def test_classes_all_ones_matrix():
    k, m = 6, 3
    got, want = run_encode(k, m, 2, 4112, seed=6,
                           rows=np.ones((m, k), dtype=np.uint8))
    assert np.array_equal(got, want)


def check_decode(ctx, full, erased, S, C):
    """Erased chunks are dirtied on the host, decoded in place on the
    device; the whole buffer must come back equal to the original."""
    n = full.shape[1]
    host = full.copy()
    mask = (1 << n) - 1
    for e in erased:
        host[:, e, :] = 0xA5
        mask &= ~(1 << e)
    dev = Dev(ctx, host)
    ctx.decode_batch(dev.d, S, C, mask)
    got = dev.get(full.shape)
    dev.free()
    assert np.array_equal(got, full), erased


def encoded_batch(k, m, S, C, seed):
    full = rand_batch(seed, S, k + m, C)
    ref_matmul(full, list(range(k)), list(range(k, k + m)),
               oracle.matrix(TECH, k, m)[k:])
    return full


def test_decode_every_pattern_k4_m2():
    k, m, S, C = 4, 2, 3, 4112
    full = encoded_batch(k, m, S, C, seed=42)
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        for e in range(1, m + 1):
            for er in combinations(range(k + m), e):
                check_decode(ctx, full, er, S, C)
    finally:
        ctx.close()


def test_decode_flagship_pattern():
    k, m, S, C = 8, 3, 3, 12272
    full = encoded_batch(k, m, S, C, seed=83)
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        check_decode(ctx, full, (4, 8, 10), S, C)
    finally:
        ctx.close()


def test_bounds_single_source():
    """k=1 shape: one source, one output. A context needs k >= 2
    (ecx_create2 rejects k=1), so the single-source launch is reached through
    matmul_batch with one source id on a (2, 1) context."""
    S, C = 3, 4112
    host = rand_batch(1, S, 3, C)
    rows = np.array([[0x53]], dtype=np.uint8)
    want = host.copy()
    ref_matmul(want, [1], [2], rows)
    ctx = ceph_amd.EcContext(2, 1, TECH, device=0)
    try:
        dev = Dev(ctx, host)
        ctx.matmul_batch(dev.d, S, C, [1], [2], rows)
        got = dev.get(host.shape)
        dev.free()
    finally:
        ctx.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k,m", [(29, 3), (32, 1), (4, 6)])
def test_bounds_wide_and_grouped(k, m):
    """k=29: source bit 28 and the upper table slots; k=32: the last
    source bit; m=6: two launches of 4 + 2 outputs. Dense random rows so
    every slot carries a general coefficient."""
    rows = np.random.default_rng(k * 100 + m).integers(
        2, 256, (m, k), dtype=np.uint8)
    got, want = run_encode(k, m, 2, 4112, seed=k + m, rows=rows)
    assert np.array_equal(got, want)


def test_matmul_batch_non_monotone_ids():
    """Source ids out of order and an output id below every source id."""
    k, m, S, C = 4, 2, 3, 4112
    host = rand_batch(9, S, k + m, C)
    src_ids, out_ids = [5, 2, 3], [0, 4]
    rows = np.array([[0x1D, 1, 0xB7], [1, 0x02, 0]], dtype=np.uint8)
    want = host.copy()
    ref_matmul(want, src_ids, out_ids, rows)
    ctx = ceph_amd.EcContext(k, m, TECH, device=0)
    try:
        dev = Dev(ctx, host)
        ctx.matmul_batch(dev.d, S, C, src_ids, out_ids, rows)
        got = dev.get(host.shape)
        dev.free()
    finally:
        ctx.close()
    assert np.array_equal(got, want)
