"""CPU tests for the host-side planning of ecx_verify_batch (the CPU-only
probe runs the call's own plan_verify): which chunks vouch, which are
checked, and that the coefficient rows rebuild every checked chunk of an
oracle-encoded stripe from the survivors."""
import ctypes
import itertools

import numpy as np
import pytest

import ceph_amd
import oracle

TECHS = ("reed_sol_van", "cauchy", "jerasure_reed_sol_van")
SHAPES = ((4, 2), (4, 3), (8, 3), (10, 4))
C = 32


def masks_with_at_least_k(k, m):
    """Every mask over k+m chunks with at most m bits clear."""
    n = k + m
    full = (1 << n) - 1
    for n_clear in range(m + 1):
        for clear in itertools.combinations(range(n), n_clear):
            yield full & ~sum(1 << i for i in clear)


N_MASKS = {(4, 2): 22, (4, 3): 64, (8, 3): 232, (10, 4): 1471}


@pytest.mark.parametrize("k,m", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("tech", TECHS)
def test_every_mask_plan_rebuilds_the_checked_chunks(tech, k, m):
    n = k + m
    rng = np.random.default_rng(0x5C + 16 * k + m)
    data = [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(k)]
    stripe = data + oracle.encode(tech, k, m, data)
    masks = list(masks_with_at_least_k(k, m))
    assert len(set(masks)) == N_MASKS[k, m]
    assert all(bin(mk).count("1") >= k for mk in masks)
    for mask in masks:
        sv, ck, rows = ceph_amd.verify_plan_probe(tech, k, m, mask)
        present = [i for i in range(n) if mask >> i & 1]
        assert list(sv) == present[:k], hex(mask)
        assert list(ck) == present[k:], hex(mask)
        assert rows.shape == (len(ck), k)
        if not len(ck):
            continue
        got = oracle.encode_with_rows(rows, [stripe[i] for i in sv])
        for j, cid in enumerate(ck):
            assert np.array_equal(got[j], stripe[cid]), (hex(mask), cid)


def _raw(tech_id, k, m, mask):
    sv = np.full(k, -7, dtype=np.int32)
    ck = np.full(m, -7, dtype=np.int32)
    rows = np.full(m * k, 0xA5, dtype=np.uint8)
    r = ceph_amd.lib().ecx_verify_plan_probe(
        tech_id, k, m, mask, sv.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        ck.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        rows.ctypes.data_as(ctypes.c_void_p))
    untouched = bool((sv == -7).all() and (ck == -7).all() and
                     (rows == 0xA5).all())
    return r, sv, untouched


@pytest.mark.parametrize("k,m", SHAPES, ids=lambda v: str(v))
def test_return_codes(k, m):
    n = k + m
    exactly_k = sum(1 << i for i in range(m, n))  # the last k chunks
    r, sv, _ = _raw(0, k, m, exactly_k)
    assert r == 0 and list(sv) == list(range(m, n))
    r, _, untouched = _raw(0, k, m, exactly_k & ~(1 << (n - 1)))  # k-1 bits
    assert r == -5 and untouched
    r, _, untouched = _raw(0, k, m, (1 << n) | ((1 << n) - 1))  # bit at k+m
    assert r == -22 and untouched
    for tech_id in (3, 4, 5):
        r, _, untouched = _raw(tech_id, k, m, (1 << n) - 1)
        assert r == -22 and untouched, tech_id


def test_python_wrapper_raises():
    with pytest.raises(ceph_amd.EcError, match="EIO"):
        ceph_amd.verify_plan_probe("reed_sol_van", 8, 3, 0x7F)
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.verify_plan_probe("reed_sol_van", 8, 3, 1 << 11 | 0x7FF)
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.verify_plan_probe("cauchy_orig", 4, 2, 0x3F)
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.verify_plan_probe("jerasure_reed_sol_van_w16", 4, 2, 0x3F)
