"""CPU tests for the host-side preparation of ecx_update_batch (the
CPU-only probe runs the call's own plan_update) and, on the oracle alone,
the identity the GPU file's expectation rests on: correcting a consistent
parity by G * (old ^ new) gives the encode of the updated data."""
import numpy as np
import pytest

import ceph_amd
import oracle
import update_cases as cases

SETS = cases.gpu_mask_sets()
IDS = [f"{t}-{k}-{m}-{len(mk)}" for t, k, m, mk in SETS]


@pytest.mark.parametrize("tech,k,m,masks", SETS, ids=IDS)
def test_plan_matches_numpy(tech, k, m, masks):
    launches, new_base, active = ceph_amd.update_plan_probe(k, m, masks)
    pop = np.array([bin(mk).count("1") for mk in masks], dtype=np.int64)
    assert np.array_equal(new_base, np.cumsum(pop) - pop)
    assert np.array_equal(active, np.flatnonzero(pop))
    assert launches == (-(-m // 4) if pop.any() else 0)


def test_all_zero_masks_launch_nothing():
    launches, new_base, active = ceph_amd.update_plan_probe(8, 3, [0] * 37)
    assert launches == 0 and len(active) == 0 and not new_base.any()


@pytest.mark.parametrize("m,want", [(1, 1), (4, 1), (5, 2), (8, 2), (9, 3)])
def test_launch_count_is_passes_of_four(m, want):
    assert ceph_amd.update_plan_probe(4, m, [0, 5, 0, 15])[0] == want


def test_bit_at_or_above_k_refused():
    for k, bad in ((4, 1 << 4), (4, 1 << 6), (8, 1 << 8), (8, 1 << 63)):
        with pytest.raises(ceph_amd.EcError, match="EINVAL"):
            ceph_amd.update_plan_probe(
                k, 3, np.array([1, 3 | bad, 2], dtype=np.uint64))
    # the highest legal bit is accepted
    assert ceph_amd.update_plan_probe(8, 3, [1 << 7])[0] == 1


def test_refusal_leaves_outputs_unwritten():
    import ctypes
    masks = np.array([3, 1 << 4, 1], dtype=np.uint64)
    base = np.full(3, -7, dtype=np.int64)
    act = np.full(3, -7, dtype=np.int32)
    n_act = ctypes.c_int(-7)
    r = ceph_amd.lib().ecx_update_plan_probe(
        4, 3, masks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 3,
        base.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
        act.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        ctypes.byref(n_act))
    assert r == -22
    assert (base == -7).all() and (act == -7).all() and n_act.value == -7


def test_stripe_count_bounds():
    launches, new_base, active = ceph_amd.update_plan_probe(4, 2, [9])
    assert (launches, list(new_base), list(active)) == (1, [0], [0])
    masks = np.full(65535, 0xff, dtype=np.uint64)
    launches, new_base, active = ceph_amd.update_plan_probe(8, 3, masks)
    assert launches == 1 and len(active) == 65535
    assert new_base[-1] == 8 * 65534


@pytest.mark.parametrize("tech,k,m,masks", SETS, ids=IDS)
def test_delta_update_equals_reencode_on_oracle(tech, k, m, masks):
    C, S = 64, len(masks)
    rng = np.random.default_rng(0xD1)
    old = rng.integers(0, 256, (S, k + m, C), dtype=np.uint8)
    oracle.cpu_encode_batch(tech, k, m, old.reshape(-1), S, C)
    new = rng.integers(0, 256, (cases.total_new(masks), C), dtype=np.uint8)
    got = cases.delta_expect(tech, k, m, old, new, masks)
    for s in range(S):
        want = oracle.encode(tech, k, m, [got[s, j].copy() for j in range(k)])
        for r in range(m):
            assert np.array_equal(got[s, k + r], want[r]), (s, r)
    # and the untouched stripes are exactly as they were
    for s, mk in enumerate(masks):
        if mk == 0:
            assert np.array_equal(got[s], old[s])
