"""Host-pointer staging path edge cases (pipelined_matmul_host /
staged_host_call / legacy_host_call): the double-buffered tile loop only
engages for chunks above the 4 MiB default tile, and the zeros-chunk
convention must survive the gather. All parity is checked against the CPU
oracle. The staging knobs are read once per process, so each knob setting is
checked in one child process that does every technique family in turn; run
as a script with a mode name, this file is that child."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# one technique per family: w=8 table, w=16, bitmatrix (packetsize 2048, so
# chunks are multiples of w * packetsize = 16 KiB)
FAMILIES = ("reed_sol_van", "jerasure_reed_sol_van_w16", "cauchy_orig")
K, M = 4, 2
PKT = 2048
POISON = 0xA5
EINVAL, EIO = -22, -5


@pytest.fixture(scope="module")
def mods():
    import ceph_amd
    import oracle
    return ceph_amd, oracle


def _roundtrip(ceph_amd, oracle, tech, k, m, C, erase, **kw):
    rng = np.random.default_rng(C ^ k)
    data = [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(k)]
    ctx = ceph_amd.EcContext(k, m, tech, device=0, **kw)
    try:
        par = ctx.encode_chunks(data)
        if tech == "cauchy_orig":
            want = oracle.bitmatrix_encode(k, m, data, 2048)
        elif tech == "jerasure_reed_sol_van_w16":
            want = oracle.encode_w16(k, m, data)
        else:
            want = oracle.encode(tech, k, m, data)
        for j in range(m):
            assert np.array_equal(par[j], want[j]), ("parity", j)
        chunks = [d.copy() for d in data] + [p.copy() for p in par]
        present = [i not in erase for i in range(k + m)]
        for e in erase:
            chunks[e][:] = 0
        ctx.decode_chunks(chunks, present)
        ref = data + par
        for i in range(k + m):
            assert np.array_equal(chunks[i], ref[i]), ("decode", i)
    finally:
        ctx.close()


def test_tiled_pipeline_two_tiles_ragged(mods):
    """chunk > 4 MiB default tile with a ragged last tile: T=2, second
    tile 16 bytes — exercises the double-buffer loop and the drain."""
    ceph_amd, oracle = mods
    _roundtrip(ceph_amd, oracle, "reed_sol_van", 8, 3,
               4 * 1024 * 1024 + 16, erase=(0, 9))


def test_tiled_pipeline_three_tiles(mods):
    """chunk = 9 MiB: T=3, buffer 1 reused — the scatter of tile t-2
    inside the loop runs (t >= 2 branch)."""
    ceph_amd, oracle = mods
    _roundtrip(ceph_amd, oracle, "cauchy", 6, 3, 9 * 1024 * 1024,
               erase=(1, 6, 8))


def test_zeros_chunk_through_gather(mods):
    """data[i] = None is the zeros-chunk convention
    (ErasureCodeJerasure.cc:146-157): the pipelined gather must skip the
    slot and the kernel must treat the source as zeros."""
    ceph_amd, oracle = mods
    k, m, C = 6, 2, 512 * 1024
    rng = np.random.default_rng(7)
    data = [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(k)]
    full = [d.copy() for d in data]
    data[2] = None
    full[2][:] = 0
    ctx = ceph_amd.EcContext(k, m, "reed_sol_van", device=0)
    try:
        par = ctx.encode_chunks(data)
        want = oracle.encode("reed_sol_van", k, m, full)
        for j in range(m):
            assert np.array_equal(par[j], want[j])
    finally:
        ctx.close()


def test_w16_staged_large(mods):
    """w=16 technique through staged_host_call at a size past 4 MiB
    (single-shot staging, no tiling for w16)."""
    ceph_amd, oracle = mods
    _roundtrip(ceph_amd, oracle, "jerasure_reed_sol_van_w16", 5, 3,
               6 * 1024 * 1024, erase=(0, 4, 6))


def test_bitmatrix_staged(mods):
    """cauchy_orig (bitmatrix) through staged_host_call, packetsize-
    aligned chunk."""
    ceph_amd, oracle = mods
    _roundtrip(ceph_amd, oracle, "cauchy_orig", 4, 2, 1024 * 1024,
               erase=(0, 5))


def test_legacy_path_still_correct(mods, monkeypatch):
    """ECX_HOSTPIPE=0 must keep the legacy per-chunk staging path alive
    (it is read once per process, so run it in a subprocess)."""
    import subprocess
    import sys
    code = (
        "import numpy as np, ceph_amd, oracle\n"
        "rng = np.random.default_rng(3)\n"
        "data = [rng.integers(0,256,65536,dtype=np.uint8) for _ in range(4)]\n"
        "ctx = ceph_amd.EcContext(4,2,'reed_sol_van',device=0)\n"
        "par = ctx.encode_chunks(data)\n"
        "want = oracle.encode('reed_sol_van',4,2,data)\n"
        "assert all(np.array_equal(p,w) for p,w in zip(par,want))\n"
        "print('LEGACY_OK')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, env={**__import__('os').environ,
                                        "ECX_HOSTPIPE": "0"})
    assert r.returncode == 0 and "LEGACY_OK" in r.stdout, r.stderr


def test_all_zeros_sentinels_with_explicit_chunk_bytes(mods):
    """Every chunk a zeros sentinel (None): the wrapper cannot infer the
    length, so the explicit chunk_bytes parameter carries it (edge found
    by tools/fuzz_gpu.py); parity of all-zeros data is all zeros
    (the zeroinout property)."""
    ceph_amd, _ = mods
    ctx = ceph_amd.EcContext(4, 2, "reed_sol_van", device=0)
    try:
        par = ctx.encode_chunks([None] * 4, chunk_bytes=65536)
        for p in par:
            assert p.nbytes == 65536 and not p.any()
    finally:
        ctx.close()


def test_graph_replay_across_size_changes(mods):
    """Regression for the round-2 GPU memory fault: single-tile host
    calls replay captured hipGraphs that bake in the pinned/device
    staging addresses; growing the pipe (a bigger call on the same slot)
    reallocates those buffers and must invalidate the cached graphs.
    Alternate small and large calls on ONE context (n_streams=1 pins
    every call to the same slot) and byte-check each against the
    oracle."""
    ceph_amd, oracle = mods
    k, m = 4, 2
    ctx = ceph_amd.EcContext(k, m, "reed_sol_van", device=0, n_streams=1)
    rng = np.random.default_rng(0x6F)
    try:
        for C in (64 << 10, 64 << 10, 1 << 20, 64 << 10, 2 << 20,
                  128 << 10, 64 << 10):
            data = [rng.integers(0, 256, C, dtype=np.uint8)
                    for _ in range(k)]
            par = ctx.encode_chunks(data)
            want = oracle.encode("reed_sol_van", k, m, data)
            for j in range(m):
                assert np.array_equal(par[j], want[j]), (C, j)
    finally:
        ctx.close()


def test_small_calls_many_shapes_one_slot(mods):
    """Graph cache keying: different (n_src, n_out, tl) combinations on
    one slot (decode plans vary n_src/n_out) must not cross-talk."""
    ceph_amd, oracle = mods
    rng = np.random.default_rng(0x51A)
    for (k, m) in ((4, 2), (6, 3), (4, 2)):
        ctx = ceph_amd.EcContext(k, m, "reed_sol_van", device=0,
                                 n_streams=1)
        try:
            C = 64 << 10
            data = [rng.integers(0, 256, C, dtype=np.uint8)
                    for _ in range(k)]
            par = ctx.encode_chunks(data)
            want = oracle.encode("reed_sol_van", k, m, data)
            for j in range(m):
                assert np.array_equal(par[j], want[j])
            # decode with 1..m erasures => varying (n_src, n_out) keys
            for ne in range(1, m + 1):
                chunks = [d.copy() for d in data] + [p.copy() for p in par]
                er = list(range(ne))
                present = [i not in er for i in range(k + m)]
                for e in er:
                    chunks[e][:] = 0
                ctx.decode_chunks(chunks, present)
                ref = data + par
                for i in range(k + m):
                    assert np.array_equal(chunks[i], ref[i]), (k, m, ne, i)
        finally:
            ctx.close()


# ---- every stager, every technique family ----

def _rand_chunks(seed, n, C):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(n)]


def _oracle_parity(oracle, tech, k, m, full):
    if tech == "cauchy_orig":
        return oracle.bitmatrix_encode(k, m, full, PKT)
    if tech == "jerasure_reed_sol_van_w16":
        return oracle.encode_w16(k, m, full)
    return oracle.encode(tech, k, m, full)


def _check_encode(ctx, oracle, data, C):
    """Encode (a None entry is a zeros chunk) against the oracle. Returns the
    k+m reference chunks, parity from the oracle."""
    full = [np.zeros(C, dtype=np.uint8) if d is None else d for d in data]
    want = _oracle_parity(oracle, ctx.technique, ctx.k, ctx.m, full)
    par = ctx.encode_chunks(data, chunk_bytes=C)
    for j in range(ctx.m):
        assert np.array_equal(par[j], want[j]), (ctx.technique, "parity", j)
    return full + want


def _check_decode(ctx, ref, erase):
    """Erase (poison) chunks of the oracle's stripe `ref`, decode, and
    compare every chunk with it."""
    chunks = [c.copy() for c in ref]
    for e in erase:
        chunks[e][:] = POISON
    ctx.decode_chunks(chunks, [i not in erase for i in range(len(ref))])
    for i in range(len(ref)):
        assert np.array_equal(chunks[i], ref[i]), (ctx.technique, erase, i)


def _check_matmul_chunks(ceph_amd, oracle):
    """ecx_matmul_chunks_host through the package's ctypes handle: a 2x4
    coefficient block, one NULL (zeros) source, one NULL (unwanted) output;
    expected bytes from the oracle's GF(2^8) arithmetic."""
    C = 64 << 10
    rows = np.array([[0x01, 0x53, 0x07, 0xCA],
                     [0x02, 0x01, 0x8E, 0x1D]], dtype=np.uint8)
    srcs = _rand_chunks(0x3A7, 4, C)
    srcs[2] = None
    full = [np.zeros(C, dtype=np.uint8) if s is None else s for s in srcs]
    want = oracle.encode_with_rows(rows, full)
    out = np.full(C, POISON, dtype=np.uint8)
    fn = ceph_amd.lib().ecx_matmul_chunks_host
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                   ctypes.c_size_t]
    ctx = ceph_amd.EcContext(K, M, "reed_sol_van", device=0)
    try:
        r = fn(ctx._h, ceph_amd._ptr_array(srcs), 4,
               ceph_amd._ptr_array([None, out]), 2,
               rows.ctypes.data_as(ctypes.c_void_p), C)
    finally:
        ctx.close()
    assert r == 0, r
    assert np.array_equal(out, want[1])


def child(mode):
    sys.path.insert(0, os.path.dirname(HERE))
    import ceph_amd
    import oracle

    def legacy(ctx, n):
        C = 64 << 10
        data = _rand_chunks(0x1E6 + n, K, C)
        ref = _check_encode(ctx, oracle, data, C)
        _check_encode(ctx, oracle, data[:1] + [None] + data[2:], C)
        _check_decode(ctx, ref, (1, K))  # one data, one parity

    def size(ctx, n):
        # 6 x 256 KiB is over the 1 MiB cap: w16 and cauchy_orig take the
        # legacy stager, reed_sol_van still pipelines
        C = 256 << 10
        ref = _check_encode(ctx, oracle, _rand_chunks(0x512 + n, K, C), C)
        _check_decode(ctx, ref, (0, K + 1))

    def tile(ctx, n):
        # four 16 KiB tiles, the last 16 bytes: the t >= 2 in-loop scatter,
        # both buffers' reuse and the two-tile drain
        C = 3 * 16384 + 16
        data = _rand_chunks(0x711 + n, K, C)
        data[2] = None
        ref = _check_encode(ctx, oracle, data, C)
        _check_decode(ctx, ref, (1, K))

    case = {"legacy": legacy, "size": size, "tile": tile}[mode]
    techs = ("reed_sol_van", "cauchy") if mode == "tile" else FAMILIES
    for n, tech in enumerate(techs):
        ctx = ceph_amd.EcContext(K, M, tech, device=0, packetsize=PKT)
        try:
            case(ctx, n)
        finally:
            ctx.close()
    if mode == "legacy":
        _check_matmul_chunks(ceph_amd, oracle)
    print("HOSTPATH_OK", mode)


OWN = ("ECX_HOSTPIPE", "ECX_HPIPE_", "ECX_HGRAPH", "ECX_SPINWAIT")


@pytest.mark.parametrize("mode,knob", [
    ("legacy", {"ECX_HOSTPIPE": "0"}),
    ("size", {"ECX_HPIPE_MAX": "1048576"}),
    ("tile", {"ECX_HPIPE_TILE": "16384"}),
], ids=["legacy", "size", "tile"])
def test_stager_under_knob(mode, knob):
    """legacy: the per-chunk stager for all three families (encode, encode
    with a zeros chunk, decode) and ecx_matmul_chunks_host. size: w16 and
    bitmatrix fall back to it above ECX_HPIPE_MAX. tile: the pipelined tile
    loop at its smallest tile."""
    env = {k: v for k, v in os.environ.items() if not k.startswith(OWN)}
    env.update(knob)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__), mode], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"HOSTPATH_OK {mode}" in r.stdout, \
        r.stdout + r.stderr


@pytest.mark.parametrize("tech", FAMILIES)
def test_decode_error_codes_leave_context_usable(mods, tech):
    """A NULL buffer for an erased chunk is ECX_ERR_INVAL, more than m
    missing chunks ECX_ERR_IO; after either, the same slot (n_streams=1)
    still decodes correctly."""
    ceph_amd, oracle = mods
    C = 64 << 10
    decode = ceph_amd.lib().ecx_decode_chunks_host
    ctx = ceph_amd.EcContext(K, M, tech, device=0, n_streams=1,
                             packetsize=PKT)
    try:
        ref = _check_encode(ctx, oracle, _rand_chunks(0xE44, K, C), C)
        all_present = (1 << (K + M)) - 1
        chunks = [c.copy() for c in ref]
        chunks[1] = None
        r = decode(ctx._h, ceph_amd._ptr_array(chunks),
                   all_present & ~(1 << 1), C)
        assert r == EINVAL, r
        _check_decode(ctx, ref, (1, K))
        chunks = [c.copy() for c in ref]
        r = decode(ctx._h, ceph_amd._ptr_array(chunks),
                   all_present & ~0b111, C)  # M + 1 missing
        assert r == EIO, r
        _check_decode(ctx, ref, (0, K + 1))
    finally:
        ctx.close()


@pytest.mark.parametrize("tech", FAMILIES)
def test_decode_plan_cache_two_masks_then_first_again(mods, tech):
    """The plan cache is host-only but reached only through a decode: a
    miss, a second miss, then a hit of the first mask."""
    ceph_amd, oracle = mods
    C = 64 << 10
    ctx = ceph_amd.EcContext(K, M, tech, device=0, packetsize=PKT)
    try:
        ref = _check_encode(ctx, oracle, _rand_chunks(0xCAC, K, C), C)
        for erase in ((0, K), (1, 2), (0, K)):
            _check_decode(ctx, ref, erase)
    finally:
        ctx.close()


def test_matmul_chunks_host(mods):
    _check_matmul_chunks(*mods)


if __name__ == "__main__":
    child(sys.argv[1])
