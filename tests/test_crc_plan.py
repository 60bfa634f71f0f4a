"""CPU tests for the host side of ecx_crc32c_batch: the library's host hash
(ecx_crc32c_probe), the shift every combine constant comes from
(ecx_crc32c_shift_probe) and the launch plan (ecx_crc32c_plan_probe), against
known answers and the from-the-polynomial numpy reference of crc_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ceph_amd
import crc_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
f = ceph_amd.crc32c_probe
shift = ceph_amd.crc32c_shift_probe


def test_known_answers():
    assert f(M32, b"123456789") ^ M32 == 0xE3069283
    for buf, want in ((bytes(32), 0x8A9136AA),
                      (b"\xff" * 32, 0x62A8AB43),
                      (bytes(range(32)), 0x46DD794E),
                      (bytes(range(31, -1, -1)), 0x113FDB5C)):
        assert f(M32, buf) ^ M32 == want
    assert f(0, b"foo bar baz") == 4119623852
    assert f(1234, b"foo bar baz") == 881700046
    assert f(M32, bytes(16)) == 0xBD8F6515
    for n in (0, 1, 16, 4096):
        assert f(0, bytes(n)) == 0
    assert f(0x1234ABCD, b"") == 0x1234ABCD


def test_reference_known_answers():
    """The reference itself, on the same vectors (it is what the GPU tests
    trust)."""
    assert cases.crc(M32, b"123456789") ^ M32 == 0xE3069283
    assert cases.crc(0, b"foo bar baz") == 4119623852
    assert cases.crc(1234, b"foo bar baz") == 881700046
    assert cases.crc(M32, bytes(16)) == 0xBD8F6515
    big = np.random.default_rng(1).integers(0, 256, 3 * cases.ROW + 48,
                                            dtype=np.uint8)
    assert cases.crc(77, big) == int(cases.crc_rows(77, big[None, :])[0])


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4097])
def test_probe_equals_reference(n):
    rng = np.random.default_rng(0xC3C + n)
    arena = rng.integers(0, 256, n + 16, dtype=np.uint8)
    for off in (1, 3, 5, 7):  # the instruction path has heads and tails
        seed = int(rng.integers(0, 1 << 32))
        buf = arena[off:off + n]
        assert f(seed, buf) == cases.crc(seed, buf.copy()), (n, off)


def test_probe_reports_its_path():
    crc, path = ceph_amd.crc32c_probe(0, b"abc", with_path=True)
    assert crc == cases.crc(0, b"abc") and path in ("sse4.2", "tables")
    out = ctypes.c_uint32(5)
    assert ceph_amd.lib().ecx_crc32c_probe(0, None, 4, ctypes.byref(out)) == -22
    assert out.value == 5
    assert ceph_amd.lib().ecx_crc32c_probe(0, b"abcd", 4, None) == -22
    assert ceph_amd.lib().ecx_crc32c_shift_probe(1, 1, None) == -22


def test_shift():
    rng = np.random.default_rng(0x5F)
    for n in (0, 1, 3, 16, 128, 4096, 32768, 1 << 20, (1 << 32) + 5,
              (1 << 45) + 9):
        c = int(rng.integers(0, 1 << 32))
        assert shift(c, n) == cases.crc_shift(c, n), n
        assert shift(0, n) == 0
    for c in (0, 1, 0x80000000, 0xDEADBEEF):
        assert shift(c, 0) == c
    # zero bytes are a shift
    assert shift(0xDEADBEEF, 100) == f(0xDEADBEEF, bytes(100))
    # additive, above 2^32 too
    for a, b in ((1, 1), (4096, 17), (1 << 31, 1 << 31), ((1 << 32) + 1, 77),
                 ((1 << 40) + 3, (1 << 33) + 9)):
        c = int(rng.integers(0, 1 << 32))
        assert shift(shift(c, a), b) == shift(c, a + b) == shift(shift(c, b), a)


def test_combine_identity():
    rng = np.random.default_rng(0x1D)
    for la, lb in ((0, 0), (0, 9), (9, 0), (1, 1), (16, 4096), (4097, 33),
                   (100, 12345)):
        seed = int(rng.integers(0, 1 << 32))
        a = rng.integers(0, 256, la, dtype=np.uint8)
        b = rng.integers(0, 256, lb, dtype=np.uint8)
        whole = f(seed, np.concatenate([a, b]))
        assert whole == shift(f(seed, a), lb) ^ f(0, b)
        assert whole == f(f(seed, a), b)


# every chunk size the GPU tests use (relative to the plan), and a sweep
def gpu_sizes():
    p = ceph_amd.crc32c_plan_probe(16, 1, 1)
    L, B = p["seg_bytes"], p["seg_bytes"] * p["segs_per_block"]
    return [16, 48, L, L + 16, 3 * L - 16, B - 16, B, B + 16, 2 * B + 48,
            65536 + 48, 4112, (1 << 20) + 16]


def tiles(plan, C):
    """(start, end) of every lane segment of every block, as the plan's
    end-aligned rule gives them; empty ones left out."""
    L, T, bpc = plan["seg_bytes"], plan["segs_per_block"], \
        plan["blocks_per_chunk"]
    out = []
    for b in range(bpc):
        base = C - (bpc - b) * L * T
        for t in range(T):
            s0, s1 = max(base + t * L, 0), base + (t + 1) * L
            if s1 > 0:
                out.append((s0, s1))
    return out


def test_plan_tiles_the_chunk():
    sizes = sorted(set(gpu_sizes()) | set(range(16, 65536 + 48 + 1, 16)))
    for C in sizes:
        for S, n in ((1, 1), (3, 6), (257, 11)):
            p = ceph_amd.crc32c_plan_probe(C, S, n)
            L, T = p["seg_bytes"], p["segs_per_block"]
            assert L % 16 == 0 and p["threads"] == T and p["reserved"] == 0
            assert p["blocks_per_chunk"] == -(-C // (L * T))
            assert p["grid"] == S * n * p["blocks_per_chunk"]
            assert 0 < p["lds_bytes"] <= 64 * 1024 and p["launches"] == 2
        segs = tiles(p, C)
        assert segs[0][0] == 0 and segs[-1][1] == C
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))  # no gap,
        assert all(0 < e - s <= L for s, e in segs)               # no overlap
        assert all((e - s) == L for s, e in segs[1:])
        assert cases.borders(p, C) == [s for s, _ in segs[1:]][::-1]


def test_plan_refusals():
    raw = ceph_amd.lib().ecx_crc32c_plan_probe
    out = (ctypes.c_long * 8)(*([-7] * 8))
    for C, S, n in ((0, 1, 1), (8, 1, 1), (24, 1, 1), (4097, 1, 1),
                    (16, 0, 1), (16, -1, 1), (16, 65536, 1),
                    (16, 1, 0), (16, 1, 65), (1 << 40, 65535, 64)):
        assert raw(C, S, n, out) == -22, (C, S, n)
        assert list(out) == [-7] * 8
    assert raw(16, 1, 1, None) == -22
    assert raw(16, 65535, 64, out) == 0
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.crc32c_plan_probe(24, 1, 1)


def test_header_and_library_agree():
    with open(os.path.join(ROOT, "include", "ec_mi355x.h")) as fh:
        text = fh.read()
    for sym in ("ecx_crc32c_batch", "ecx_crc32c_probe",
                "ecx_crc32c_shift_probe", "ecx_crc32c_plan_probe"):
        assert f"ECX_API int {sym}(" in text
        assert hasattr(ceph_amd.lib(), sym)


def test_plan_check_tool_under_sanitizers(tmp_path):
    """tools/crc_plan_check.cc (its own main, plain C++) built with
    -fsanitize=address,undefined and run as a process of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++)")
    exe = str(tmp_path / "crc_plan_check")
    # the sanitizer runtimes linked into the program itself: it then runs
    # the same whatever else the environment loads into a process
    subprocess.run(
        [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tools", "crc_plan_check.cc"),
         os.path.join(ROOT, "ceph_amd", "csrc", "crc_plan.cpp"), "-o", exe],
        check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crc_plan_check: ok" in r.stdout
