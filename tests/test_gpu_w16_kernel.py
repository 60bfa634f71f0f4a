"""ec_gf16_matmul_kernel (jerasure reed_sol_van, w = 16) through the device
batch calls: every case is bit-exact against bitmatrix_cases.ref16, a
GF(2^16) matrix product over u16 little-endian symbols built from the
oracle's field and matrices, in the guarded, pre-dirtied form of
test_gpu_bitmatrix_kernel.py. A tile is 256 lanes x 16 B = 4096 B of one
chunk; outputs go in groups of at most four per launch. Run as a script,
this file is the ECX_NT=0 child of its last test."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
import ceph_amd  # noqa: E402
import oracle  # noqa: E402
import bitmatrix_cases as cases  # noqa: E402
from test_gpu_bitmatrix_kernel import (  # noqa: E402
    Guarded, check_decode, check_encode)

pytestmark = pytest.mark.gpu

TECH = cases.W16


def context(k, m):
    return ceph_amd.EcContext(k, m, TECH, device=0)


def encode_sizes():
    """(4, 2) at every size of W16_SIZES, one and three stripes."""
    ctx = context(4, 2)
    try:
        for C in cases.W16_SIZES:
            for S in cases.STRIPES:
                check_encode(ctx, cases.encoded16(4, 2, S, C), 4, (C, S))
    finally:
        ctx.close()


def long_walk(L=cases.W16_LONG):
    """Blocks take a second grid-stride trip that ends in a one-vector
    tail: 2 x 256 lanes over 513 vectors."""
    k, m, C, S = L["k"], L["m"], L["C"], L["S"]
    host = cases.rand_batch(0x1610, S, k + m, C)  # parity pre-dirtied
    ctx = context(k, m)
    try:
        dev = Guarded(ctx, host)
        try:
            ctx.encode_batch(dev.d, S, C)
            got = dev.get()
        finally:
            dev.free()
    finally:
        ctx.close()
    assert np.array_equal(got[:, :k], host[:, :k]), "data chunks changed"
    pick = np.random.default_rng(32).choice(np.arange(1, S - 1), 32,
                                            replace=False)
    pick = np.concatenate(([0, S - 1], np.sort(pick)))
    want = host[pick].copy()
    cases.ref16(want, list(range(k)), list(range(k, k + m)),
                oracle.matrix_w16(k, m)[k:])
    assert np.array_equal(got[pick], want)


def test_tile_walk_small_and_partial():
    encode_sizes()


def test_tile_walk_second_trip():
    long_walk()


def test_tile_walk_second_trip_with_tables():
    long_walk(cases.W16_LONG_TABLES)


@pytest.mark.parametrize("pos", range(4))
def test_every_symbol_value(pos):
    """A source chunk holding all 65536 symbol values, at each source
    position in turn."""
    k, m, C = 4, 2, 131072
    want = cases.rand_batch(0x1600 + pos, 1, k + m, C)
    want[0, pos] = np.arange(65536, dtype="<u2").view(np.uint8)
    cases.ref16(want, list(range(k)), list(range(k, k + m)),
                oracle.matrix_w16(k, m)[k:])
    ctx = context(k, m)
    try:
        check_encode(ctx, want, k, pos)
    finally:
        ctx.close()


def test_output_groups_four_and_two():
    """(4, 6): two launches per call; decodes that lose 5 and 6 chunks."""
    k, m, C = 4, 6, 4112
    ctx = context(k, m)
    try:
        for S in cases.STRIPES:
            full = cases.encoded16(k, m, S, C)
            check_encode(ctx, full, k, (k, m, S))
            check_decode(ctx, full, (1, 3, 5, 6, 8), S)
            check_decode(ctx, full, (0, 1, 2, 3, 4, 9), S)
    finally:
        ctx.close()


@pytest.mark.parametrize("S", cases.STRIPES)
def test_decode_every_pattern_k4_m3(S):
    k, m, C = 4, 3, 4112
    full = cases.encoded16(k, m, S, C)
    ctx = context(k, m)
    try:
        for er in cases.patterns(k + m, 3):
            check_decode(ctx, full, er, S)
    finally:
        ctx.close()


@pytest.mark.parametrize("C", cases.W16_DELTA_SIZES)
def test_apply_delta_every_pair(C):
    """parity ^= gen[coding][data] * delta, parity random to begin with."""
    k, m = 3, 2
    gen = oracle.matrix_w16(k, m)
    ctx = context(k, m)
    try:
        for data in range(k):
            for coding in range(k, k + m):
                buf = cases.rand_batch(C + 10 * data + coding, 1, 2, C)
                delta, parity = buf[0, 0].copy(), buf[0, 1].copy()
                cases.ref16(buf, [0], [1], [[gen[coding][data]]], accum=True)
                got = ctx.apply_delta(delta, data, coding, parity)
                assert np.array_equal(got, buf[0, 1]), (data, coding)
                assert np.array_equal(delta, buf[0, 0]), "delta changed"
    finally:
        ctx.close()


@pytest.mark.parametrize("n_out", [2, 3, 4])
def test_apply_deltas_accumulates_into_several_parities(n_out):
    """The accumulating instances with 2, 3 and 4 outputs: apply_deltas of
    two deltas into n_out parities of (3, 4)."""
    k, m, C = 3, 4, 4112
    gen = oracle.matrix_w16(k, m)
    ds, cs = [0, 2], list(range(k, k + n_out))
    buf = cases.rand_batch(0x16A0 + n_out, 1, 2 + n_out, C)
    deltas = {d: buf[0, i].copy() for i, d in enumerate(ds)}
    parities = {c: buf[0, 2 + j].copy() for j, c in enumerate(cs)}
    cases.ref16(buf, [0, 1], list(range(2, 2 + n_out)),
                [[gen[c][d] for d in ds] for c in cs], accum=True)
    ctx = context(k, m)
    try:
        ctx.apply_deltas(deltas, parities)
    finally:
        ctx.close()
    for j, c in enumerate(cs):
        assert np.array_equal(parities[c], buf[0, 2 + j]), c
    for i, d in enumerate(ds):
        assert np.array_equal(deltas[d], buf[0, i]), "delta changed"


def child():
    encode_sizes()
    long_walk()
    print("W16_NT0_OK")


def test_plain_load_store_instances():
    """ECX_NT is read once per process: the plain-load/store instances run
    the tile-walk cases in a child of their own."""
    env = {k: v for k, v in os.environ.items() if k != "ECX_NT"}
    env["ECX_NT"] = "0"
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "W16_NT0_OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    child()
