"""CPU tests for ecx_locate_batch's host side: the reference itself
(locate_cases.py, oracle only) on oracle-encoded stripes, the planner through
its CPU-only probe (the call's own plan_locate) and the finish rule."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ceph_amd
import locate_cases as cases
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("reed_sol_van", 4, 2), ("cauchy", 4, 3), ("reed_sol_van", 8, 3))
C = 48


def one_bit(w):
    return w != 0 and w & (w - 1) == 0


@pytest.mark.parametrize("tech,k,m", SHAPES, ids=lambda v: str(v))
def test_reference_consequences(tech, k, m):
    """What the definition means for an MDS code: clean -> everything
    qualifies; one damaged chunk, anywhere and in any number of bytes -> that
    chunk alone; two chunks damaged in different byte columns -> nothing; and
    never more than one bit on an inconsistent stripe."""
    n = k + m
    mask = cases.full(k, m)
    base = cases.encoded_batch(tech, k, m, 1, C, seed=16 * k + m)[0]
    assert cases.expected_word(tech, k, m, list(base), mask) == 0
    assert cases.culprits(tech, k, m, list(base), mask) == mask
    rng = np.random.default_rng(0x10C + k)
    for x in range(n):
        for offs in ((0,), (C - 1,), (3, 17, C - 2)):
            st = base.copy()
            for o in offs:
                st[x, o] ^= int(rng.integers(1, 256))
            assert cases.expected_word(tech, k, m, list(st), mask) != 0
            assert cases.culprits(tech, k, m, list(st), mask) == 1 << x
    for x, y in itertools.combinations(range(n), 2):
        st = base.copy()
        st[x, 5] ^= 0x21
        st[y, 40] ^= 0x21
        bad = cases.expected_word(tech, k, m, list(st), mask)
        cul = cases.culprits(tech, k, m, list(st), mask)
        assert bad != 0 and cul == 0, (x, y, bad, cul)
    # same byte column: whatever comes out, at most one bit
    for x, y in itertools.combinations(range(n), 2):
        st = base.copy()
        st[x, 9] ^= int(rng.integers(1, 256))
        st[y, 9] ^= int(rng.integers(1, 256))
        cul = cases.culprits(tech, k, m, list(st), mask)
        assert cases.expected_word(tech, k, m, list(st), mask) != 0
        assert cul == 0 or one_bit(cul), (x, y, cul)


def test_reference_degraded_mask():
    """Absent chunks never qualify and damage in them is not seen."""
    tech, k, m = "cauchy", 4, 3
    base = cases.encoded_batch(tech, k, m, 1, C, seed=0xD)[0]
    mask = 0b1111011  # chunk 2 absent
    st = base.copy()
    st[2, 7] ^= 1
    assert cases.culprits(tech, k, m, list(st), mask) == mask
    st[5, 7] ^= 1
    assert cases.culprits(tech, k, m, list(st), mask) == 1 << 5


def masks_43_with_at_least(bits):
    return [mk for mk in range(1 << 7) if bin(mk).count("1") >= bits]


@pytest.mark.parametrize("tech", ["reed_sol_van", "cauchy",
                                  "jerasure_reed_sol_van"])
def test_probe_ids_and_rows(tech):
    """Every mask of (4,3) with at least k + 2 bits: candidate i has the
    base survivors without s_i plus checked[0], checks checked[1:], and its
    rows rebuild those chunks as the oracle's own decode does."""
    k, m = 4, 3
    n = k + m
    rng = np.random.default_rng(0x43)
    data = [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(k)]
    stripe = data + oracle.encode(tech, k, m, data)
    masks = masks_43_with_at_least(k + 2)
    assert len(masks) == 1 + 7
    for mask in masks:
        sv, ck, csv, cck, rows = ceph_amd.locate_plan_probe(tech, k, m, mask)
        present = [i for i in range(n) if mask >> i & 1]
        assert list(sv) == present[:k] and list(ck) == present[k:]
        nck = len(ck)
        assert csv.shape == (k, k) and cck.shape == (k, nck - 1)
        assert rows.shape == (k, nck - 1, k)
        for i in range(k):
            want_sv = sorted(set(present[:k]) - {present[i]} | {present[k]})
            assert list(csv[i]) == want_sv, (hex(mask), i)
            assert list(cck[i]) == present[k + 1:], (hex(mask), i)
            # the oracle's rebuild from the candidate's survivors: an encoded
            # stripe with junk in the other chunks, decoded
            chunks = [c.copy() if j in want_sv else np.full(C, 0xEE, np.uint8)
                      for j, c in enumerate(stripe)]
            oracle.decode(tech, k, m, chunks,
                          [int(j in want_sv) for j in range(n)])
            got = oracle.encode_with_rows(rows[i],
                                          [stripe[j] for j in want_sv])
            for j, cid in enumerate(cck[i]):
                assert np.array_equal(got[j], chunks[cid]), (hex(mask), i, cid)
                assert np.array_equal(got[j], stripe[cid])


def test_probe_larger_shapes():
    for tech, k, m in (("reed_sol_van", 6, 2), ("reed_sol_van", 10, 4),
                       ("cauchy", 8, 3)):
        sv, ck, csv, cck, rows = ceph_amd.locate_plan_probe(
            tech, k, m, cases.full(k, m))
        assert list(sv) == list(range(k))
        assert list(ck) == list(range(k, k + m))
        assert rows.shape == (k, m - 1, k)
        for i in range(k):
            assert list(csv[i]) == [j for j in range(k + 1) if j != i]
            assert list(cck[i]) == list(range(k + 1, k + m))


def np_locate_word(present, surv, bad, refuted):
    out = np.where(bad == 0, present, surv & ~refuted)
    for j in range(64):
        bit = np.uint64(1) << np.uint64(j)
        checked = (present & ~surv & bit) != 0
        alone = (bad & ~bit) == 0
        out = np.where((bad != 0) & checked & alone, out | bit, out)
    return out


def test_locate_word_probe_against_numpy():
    rng = np.random.default_rng(0x10CA7E)
    N = 4000
    words = rng.integers(0, 1 << 64, (4, N), dtype=np.uint64)
    present = words[0]
    surv = words[1] & present
    # sparse, single-bit and zero verify words as well as dense ones
    bad = words[2].copy()
    bad[:N // 4] = 0
    bad[N // 4:N // 2] = np.uint64(1) << (
        rng.integers(0, 64, N // 2 - N // 4).astype(np.uint64))
    bad[N // 2:3 * N // 4] &= present[N // 2:3 * N // 4] & \
        ~surv[N // 2:3 * N // 4]
    refuted = words[3]
    want = np_locate_word(present, surv, bad, refuted)
    for i in range(N):
        got = ceph_amd.locate_word_probe(present[i], surv[i], bad[i],
                                         refuted[i])
        assert got == int(want[i]), (i, hex(got), hex(int(want[i])))
    # the documented cases
    assert ceph_amd.locate_word_probe(0x7F, 0x0F, 0, 0x3) == 0x7F
    assert ceph_amd.locate_word_probe(0x7F, 0x0F, 0x70, 0xB) == 0x04
    assert ceph_amd.locate_word_probe(0x7F, 0x0F, 0x20, 0xF) == 0x20
    assert ceph_amd.locate_word_probe(0x7F, 0x0F, 0x30, 0xF) == 0


def _raw(tech_id, k, m, mask):
    ip = ctypes.POINTER(ctypes.c_int)
    bufs = [np.full(k, -7, np.int32), np.full(m, -7, np.int32),
            np.full(k * k, -7, np.int32), np.full(k * m, -7, np.int32)]
    rows = np.full(k * m * k, 0xA5, dtype=np.uint8)
    r = ceph_amd.lib().ecx_locate_plan_probe(
        tech_id, k, m, mask, *[b.ctypes.data_as(ip) for b in bufs],
        rows.ctypes.data_as(ctypes.c_void_p))
    untouched = all((b == -7).all() for b in bufs) and (rows == 0xA5).all()
    return r, untouched


def test_probe_refusals_leave_outputs_unwritten():
    k, m = 4, 3
    EINVAL, EIO = -22, -5
    t = ceph_amd.TECHNIQUES
    rs = t["reed_sol_van"]
    assert _raw(rs, k, m, 0b0011111) == (EINVAL, True)   # k + 1 present
    assert _raw(rs, k, m, 0b1010101) == (EINVAL, True)   # k present
    assert _raw(rs, k, m, 0b0010101) == (EIO, True)      # k - 1 present
    assert _raw(rs, k, m, 0) == (EIO, True)
    assert _raw(rs, k, m, 0x7F | 1 << 7) == (EINVAL, True)  # a bit at k + m
    assert _raw(rs, k, m, 0x7F | 1 << 63) == (EINVAL, True)
    for name in ("cauchy_orig", "cauchy_good", "jerasure_reed_sol_van_w16"):
        assert _raw(t[name], k, m, 0x7F) == (EINVAL, True), name
    r, untouched = _raw(rs, k, m, 0b1101111)
    assert r == 2 and not untouched
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.locate_plan_probe("reed_sol_van", k, m, 0b0011111)
    with pytest.raises(ceph_amd.EcError, match="EIO"):
        ceph_amd.locate_plan_probe("reed_sol_van", k, m, 0b0000111)


def test_header_and_library_agree():
    with open(os.path.join(ROOT, "include", "ec_mi355x.h")) as fh:
        text = fh.read()
    for sym in ("ecx_locate_batch", "ecx_locate_chunks_host",
                "ecx_locate_plan_probe", "ecx_repair_batch"):
        assert f"ECX_API int {sym}(" in text
        assert hasattr(ceph_amd.lib(), sym)
    assert "ECX_API uint64_t ecx_locate_word_probe(" in text
    assert hasattr(ceph_amd.lib(), "ecx_locate_word_probe")


def test_plan_check_tool_under_sanitizers(tmp_path):
    """tools/locate_plan_check.cc (its own main, plain C++: the planner, the
    finish rule and a host model of the device's part) built with
    -fsanitize=address,undefined and run as a process of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++)")
    exe = str(tmp_path / "locate_plan_check")
    csrc = os.path.join(ROOT, "ceph_amd", "csrc")
    # the sanitizer runtimes linked into the program itself: it then runs
    # the same whatever else the environment loads into a process
    subprocess.run(
        [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tools", "locate_plan_check.cc"),
         os.path.join(csrc, "locate_plan.cpp"),
         os.path.join(csrc, "verify_plan.cpp"),
         os.path.join(csrc, "gf.cpp"), "-o", exe],
        check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "locate_plan_check: ok" in r.stdout
