"""CPU tests for the per-stripe-pattern decode grouping
(ecx_decode_multi_plan_probe — the same group_decode_masks the GPU entries
ecx_decode_batch_multi / ecx_decode_slices_multi run before they launch).

What is pinned: plan indices follow first appearance, fully present stripes
map to -1, and the launch count depends on how many chunks stripes lose
(at most m launches), never on how many distinct patterns a call holds."""
import ctypes
import random

import numpy as np
import pytest

import ceph_amd
import decode_multi_cases as cases

EINVAL, EIO = -22, -5


def check_consistent(masks, pos, n_bits):
    """equal masks <-> equal indices, numbered in first-appearance order,
    -1 exactly for masks with nothing erased."""
    full = (1 << n_bits) - 1
    first = {}
    for mk, p in zip(masks, pos):
        if mk & full == full:
            assert p == -1
            continue
        if mk not in first:
            first[mk] = len(first)
        assert p == first[mk], (hex(mk), p, first[mk])
    return len(first)


@pytest.mark.parametrize("tech", cases.MATRIX_TECHS)
def test_all_patterns_43(tech):
    masks = cases.all_patterns_43()
    n_launches, pos, n_plans = ceph_amd.decode_multi_plan_probe(
        tech, 4, 3, masks)
    assert n_plans == 63
    assert n_launches == 3
    assert pos[masks.index(0x7f)] == -1
    assert list(pos).count(-1) == 1
    assert check_consistent(masks, pos, 7) == 63


@pytest.mark.parametrize("tech", cases.MATRIX_TECHS)
def test_launch_count_independent_of_repeats_and_patterns(tech):
    masks = cases.all_patterns_43()
    once = ceph_amd.decode_multi_plan_probe(tech, 4, 3, masks)
    ten = ceph_amd.decode_multi_plan_probe(tech, 4, 3, masks * 10)
    assert (ten[0], ten[2]) == (once[0], once[2]) == (3, 63)
    assert np.array_equal(ten[1], np.tile(once[1], 10))
    # one repeated 2-erasure mask: one launch, one plan
    n_launches, pos, n_plans = ceph_amd.decode_multi_plan_probe(
        tech, 4, 3, [cases.mask_without(7, [2, 5])] * 300)
    assert (n_launches, n_plans) == (1, 1)
    assert not pos.any()


def test_more_than_four_erasures():
    k, m = 4, 6
    rng = random.Random(5)
    masks = [cases.mask_without(10, rng.sample(range(10), e))
             for e in (1, 5, 6)]
    once = ceph_amd.decode_multi_plan_probe("cauchy", k, m, masks)
    many = ceph_amd.decode_multi_plan_probe("cauchy", k, m, masks * 50)
    # passes: 1 -> (0,1); 5 -> (0,4)+(1,1); 6 -> (0,4)+(1,2)
    assert once[0] == many[0] == 4 <= m
    assert once[2] == many[2] == 3
    # every erasure count 1..m at once still stays within m launches
    masks = [cases.mask_without(10, rng.sample(range(10), e))
             for e in range(1, m + 1) for _ in range(3)]
    n_launches, pos, n_plans = ceph_amd.decode_multi_plan_probe(
        "cauchy", k, m, masks)
    assert n_launches == m
    assert check_consistent(masks, pos, 10) == n_plans


def test_accepts_uint64_array_and_ignores_bits_above_n():
    masks = cases.all_patterns_43()
    a = np.array(masks, dtype=np.uint64)
    want = ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3, masks)
    got = ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3, a)
    assert got[0] == want[0] and got[2] == want[2]
    assert np.array_equal(got[1], want[1])
    # bits above k+m carry no chunk: same grouping with them set
    hi = ceph_amd.decode_multi_plan_probe(
        "reed_sol_van", 4, 3, a | np.uint64(0xffff << 48))
    assert hi[0] == want[0] and hi[2] == want[2]
    assert np.array_equal(hi[1], want[1])


def test_one_undecodable_mask_is_eio():
    good = cases.all_patterns_43()
    bad = cases.mask_without(7, [0, 1, 2, 3])  # 3 present < k
    with pytest.raises(ceph_amd.EcError, match="EIO"):
        ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3,
                                         good[:20] + [bad] + good[20:])
    with pytest.raises(ceph_amd.EcError, match="EIO"):
        ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3, [bad])
    # raw return value, and outputs left unwritten
    lib = ceph_amd.lib()
    a = (ctypes.c_uint64 * 1)(bad)
    pos = (ctypes.c_int * 1)(77)
    n_plans = ctypes.c_int(77)
    assert lib.ecx_decode_multi_plan_probe(0, 4, 3, a, 1, pos,
                                           ctypes.byref(n_plans)) == EIO
    assert pos[0] == 77 and n_plans.value == 77


def test_gpu_test_masks_are_decodable():
    """Inputs of tests/test_gpu_decode_multi.py are chosen here, on the
    CPU: every mask must compose a decode plan (ecx_decode_rows_probe, the
    plan math pinned against the oracle in test_cauchy_good.py)."""
    lib = ceph_amd.lib()
    fn = lib.ecx_decode_rows_probe
    fn.restype = ctypes.c_int
    for tech, k, m, masks in cases.gpu_mask_sets():
        n = k + m
        sv = (ctypes.c_int * k)()
        er = (ctypes.c_int * m)()
        rows = (ctypes.c_uint8 * (m * k))()
        for mk in sorted(set(masks)):
            r = fn(ceph_amd.TECHNIQUES[tech], k, m, ctypes.c_uint64(mk),
                   sv, er, rows)
            assert r == len(cases.erased_of(n, mk)), (tech, k, m, hex(mk), r)
        # and the grouping accepts the set as a whole, within m launches
        n_launches, pos, _ = ceph_amd.decode_multi_plan_probe(
            tech, k, m, masks)
        assert 1 <= n_launches <= m
        check_consistent(masks, pos, n)


def test_negative_arguments():
    lib = ceph_amd.lib()
    fn = lib.ecx_decode_multi_plan_probe
    a = (ctypes.c_uint64 * 2)(0x7e, 0x7d)
    pos = (ctypes.c_int * 2)()
    n_plans = ctypes.c_int()
    ok = fn(0, 4, 3, a, 2, pos, ctypes.byref(n_plans))
    assert ok == 1 and n_plans.value == 2 and list(pos) == [0, 1]
    assert fn(0, 4, 3, None, 2, pos, ctypes.byref(n_plans)) == EINVAL
    assert fn(0, 4, 3, a, 2, None, ctypes.byref(n_plans)) == EINVAL
    assert fn(0, 4, 3, a, 2, pos, None) == EINVAL
    assert fn(0, 4, 3, a, 0, pos, ctypes.byref(n_plans)) == EINVAL
    assert fn(0, 4, 3, a, -1, pos, ctypes.byref(n_plans)) == EINVAL
    # the calls refuse bitmatrix and w=16 contexts; so does their probe
    for tech in ("cauchy_orig", "cauchy_good", "jerasure_reed_sol_van_w16"):
        assert fn(ceph_amd.TECHNIQUES[tech], 4, 3, a, 2, pos,
                  ctypes.byref(n_plans)) == EINVAL


def test_python_length_and_type_checks():
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3, [])
    with pytest.raises(ceph_amd.EcError, match="uint64"):
        ceph_amd.decode_multi_plan_probe("reed_sol_van", 4, 3, [-1])
    # length mismatches are caught before the C call: _h is never read
    ctx = object.__new__(ceph_amd.EcContext)
    ctx._h, ctx.k, ctx.m = None, 4, 2
    with pytest.raises(ceph_amd.EcError, match="need 3 present_masks"):
        ctx.decode_batch_multi(None, 3, 16, [0x3f, 0x3e])
    with pytest.raises(ceph_amd.EcError, match="need 2 present_masks"):
        ctx.decode_slices_multi([1] * 12, [16, 16], [0x3f])
    with pytest.raises(ceph_amd.EcError, match="chunk pointers"):
        ctx.decode_slices_multi([1] * 11, [16, 16], [0x3f, 0x3f])


def test_symbols_exported():
    lib = ctypes.CDLL(ceph_amd._SO)
    for sym in ("ecx_decode_batch_multi", "ecx_decode_slices_multi",
                "ecx_decode_multi_plan_probe"):
        assert hasattr(lib, sym), sym
