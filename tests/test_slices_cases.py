"""CPU tests for the host side of the slice calls (ecx_slice_plan_probe: the
argument check, the cut into blocks, the job table) and for the inputs of
the GPU slice tests (slices_cases.py): that every mask decodes, that the
arenas are what they claim to be, that the lists reach the sizes, buckets and
passes they name, and that the whole-arena comparison tells a wrong kernel
from a right one — for each of six mistakes a kernel could make, the model
with that mistake built in must differ from the expected arena."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ceph_amd
import slices_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
BASE = 0x7F0000000000  # a made-up device base: the probe never follows it


def rows_of(tech, k, m):
    """mask -> (survivors, erased, rows) by ecx_decode_rows_probe (pinned
    against the oracle in test_cauchy_good.py)."""
    fn = ceph_amd.lib().ecx_decode_rows_probe
    fn.restype = ctypes.c_int

    def f(mask):
        sv = (ctypes.c_int * k)()
        er = (ctypes.c_int * m)()
        rows = (ctypes.c_uint8 * (m * k))()
        e = fn(ceph_amd.TECHNIQUES[tech], k, m, ctypes.c_uint64(mask), sv, er,
               rows)
        assert e == len(cases.erased_of(k + m, mask)), (tech, hex(mask), e)
        return (list(sv), list(er)[:e],
                [list(rows[j * k:(j + 1) * k]) for j in range(e)])
    return f


def decode_sets():
    """(technique, k, m, masks) of every mask the GPU slice tests decode."""
    return [("reed_sol_van", 4, 2, cases.DECODE_42_MASKS),
            ("cauchy", 4, 6, cases.DECODE_46_MASKS),
            ("reed_sol_van", 4, 2, [cases.DECODE_NULL_MASK]),
            ("cauchy", 4, 6, cases.multi_case()[2]),
            ("cauchy", 4, 6, [cases.knob_decode_case()[2]]),
            ("cauchy", 4, 6, cases.knob_multi_case()[2]),
            ("reed_sol_van", 4, 2, cases.SLOT_MASKS[0] + cases.SLOT_MASKS[1])]


def all_arenas():
    out = [("encode %d,%d %s" % c, cases.encode_case(*c)[0])
           for c in cases.ENCODE_CODES]
    out += [("class", cases.class_case(cases.CLASS_ROWS)[0]),
            ("null", cases.null_case()[0]),
            ("shared", cases.shared_case()[0]),
            ("decode42", cases.decode_42_case()[0]),
            ("decode46", cases.decode_46_case()[0]),
            ("decode null", cases.decode_null_case()[0]),
            ("multi", cases.multi_case()[0]),
            ("knob decode", cases.knob_decode_case()[0]),
            ("knob multi", cases.knob_multi_case()[0])]
    out += [("growth %d" % i, a) for i, (a, _) in
            enumerate(cases.growth_cases())]
    out += [("slot %d" % i, a) for i, (a, _) in enumerate(cases.slot_cases())]
    return out


def test_edge_sizes_follow_the_probed_block():
    g = ceph_amd.slice_plan_probe(2, [BASE, BASE + 16], [16])
    assert g["vecs_per_block"] == cases.VPB == 4 * cases.THREADS
    assert cases.edge_sizes(g["vecs_per_block"]) == cases.EDGE_SIZES == [
        16, 4080, 4096, 4112, 16368, 16384, 16400, 20496, 32784]
    # what each one means, in blocks of the probe's own count
    blocks = [ceph_amd.slice_plan_probe(1, [BASE], [sz])["n_blocks"]
              for sz in cases.EDGE_SIZES]
    assert blocks == [1, 1, 1, 1, 1, 1, 2, 2, 3]


def test_every_mask_is_decodable():
    for tech, k, m, masks in decode_sets():
        f = rows_of(tech, k, m)
        for mk in sorted(set(masks)):
            if cases.erased_of(k + m, mk):
                sv, er, _ = f(mk)
                assert er == cases.erased_of(k + m, mk) and len(sv) == k
    # the NULL survivors are present in their slice's mask, and are data
    arena, _, masks = cases.multi_case()
    for s, c in cases.MULTI_NULL:
        assert masks[s] >> c & 1 and c < 4 and arena.offset(s, c) is None
    assert len({c for _, c in cases.MULTI_NULL}) == 3
    for s, c in cases.DECODE_NULL:
        assert cases.DECODE_NULL_MASK >> c & 1 and c < 4
    arena, _, mk = cases.knob_decode_case()
    assert all(mk >> c & 1 for _, c in arena.null)
    arena, _, masks = cases.knob_multi_case()
    assert all(masks[s] >> c & 1 for s, c in arena.null)


def test_arenas_do_not_overlap():
    for name, a in all_arenas():
        spans = sorted((a.off[sc], a.off[sc] + a.sizes[sc[0]]) for sc in a.own)
        guards = sorted(a.guards)
        assert len(guards) == len(spans) + 1, name
        pos = 0
        for (g0, gl), (c0, c1) in zip(guards, spans):
            assert g0 == pos and gl >= 16 and g0 + gl == c0, name  # no gap,
            assert c0 % 16 == 0 and c1 > c0, name                  # no overlap
            pos = c1
        g0, gl = guards[-1]
        assert g0 == pos and gl >= 16 and g0 + gl == a.nbytes, name
        for g0, gl in guards:
            assert (a.image[g0:g0 + gl] == cases.POISON).all(), name
        for sc in a.null:
            assert a.offset(*sc) is None, name
        # placement is shuffled: ids do not come in address order
        order = [sc for _, sc in sorted((a.off[sc], sc) for sc in a.own)]
        assert order != sorted(order), name
    # chunk starts reach every multiple of 16 mod 256 in the large arenas
    # over all of EDGE_SIZES, and several of them in every arena
    for name, a in all_arenas():
        res = {a.off[sc] % 256 for sc in a.own}
        assert len(res) >= min(len(a.own), 16) // 2, name
        if len(a.own) >= 90 and set(a.sizes) == set(cases.EDGE_SIZES):
            assert res == set(range(0, 256, 16)), name


def test_lists_contain_the_sizes_they_name():
    E, S = cases.EDGE_SIZES, cases.SMALL_SIZES
    for c in cases.ENCODE_CODES:
        assert cases.encode_case(*c)[0].sizes == E
    assert sorted((k, m) for k, m, _ in cases.ENCODE_CODES) == sorted(
        [(3, 1), (4, 2), (4, 2), (4, 2), (5, 3), (5, 4), (4, 5), (4, 6),
         (3, 8)])
    assert {t for k, m, t in cases.ENCODE_CODES if (k, m) == (4, 2)} == set(
        cases.MATRIX_TECHS)
    assert S == [16, 4112, 16400]
    assert cases.class_case(cases.CLASS_ROWS)[0].sizes == S
    assert cases.decode_42_case()[0].sizes == S
    assert len(cases.DECODE_42_MASKS) == 6 + 15
    assert cases.decode_46_case()[0].sizes == E
    lost = [cases.erased_of(10, mk) for mk in cases.DECODE_46_MASKS]
    assert {len(e) for e in lost} == {5, 6}
    assert all(min(e) < 4 for e in lost) and all(max(e) >= 4 for e in lost)
    assert set(cases.multi_case()[0].sizes) == set(E)
    assert set(cases.knob_decode_case()[0].sizes) == set(S)
    assert set(cases.knob_multi_case()[0].sizes) == set(S)
    # NULL data: every position somewhere, all in one slice, none in another
    assert set().union(*cases.NULL_SETS) == {0, 1, 2, 3}
    assert cases.NULL_SETS[cases.NULL_ALL] == {0, 1, 2, 3}
    assert cases.NULL_SETS[cases.NULL_NONE] == set()
    assert len({frozenset(s) for s in cases.NULL_SETS}) == len(cases.NULL_SETS)
    # class rows: a zero, a one, a zero inside a nonzero row, a zero row
    R = cases.CLASS_ROWS
    assert not R[cases.CLASS_ZERO_ROW].any()
    assert any(0 in r and r.any() for r in R) and (R == 1).any()
    shec = ceph_amd.shec_matrix(4, 3, 2)
    assert (shec == 0).any() and all(r.any() for r in shec)
    # shared sources: same data offsets, different sizes, own parity
    a = cases.shared_case()[0]
    assert a.sizes[0] != a.sizes[1]
    assert all(a.offset(0, c) == a.offset(1, c) for c in range(4))
    assert all(a.offset(0, c) != a.offset(1, c) for c in (4, 5))
    # growth: the second table outgrows 1.5x + 4096 of the first
    tabs = [ceph_amd.slice_plan_probe(6, arena.ptrs(BASE), arena.sizes)["bytes"]
            for arena, _ in cases.growth_cases()]
    assert tabs[1] > tabs[0] + tabs[0] // 2 + 4096
    assert [len(a.sizes) for a, _ in cases.growth_cases()] == [64, 6000, 8]
    assert all(16 <= sz <= 64 for sz in cases.growth_cases()[1][0].sizes)
    assert set(cases.growth_cases()[2][0].sizes) == {32784}


def parent_tables(cps, ptrs, sizes, order=None, recs=None, head=0, vpb=1024):
    """The job table as the slice calls have always built it, restated:
    [head][ptrs u64][slice_vecs i64][block_voff i64][block_slice i32]
    [block_rec i32 if recs], blocks in `order`."""
    vecs = [sz >> 4 for sz in sizes]
    bs, bv, br = [], [], []
    for i, sl in enumerate(range(len(sizes)) if order is None else order):
        for v in range(0, vecs[sl], vpb):
            bs.append(sl)
            bv.append(v)
            if recs is not None:
                br.append(recs[i])
    parts = [np.zeros(head, np.uint8),
             np.array([p or 0 for p in ptrs], np.uint64).view(np.uint8),
             np.array(vecs, np.int64).view(np.uint8),
             np.array(bv, np.int64).view(np.uint8),
             np.array(bs, np.int32).view(np.uint8),
             np.array(br, np.int32).view(np.uint8)]
    return np.concatenate(parts), bs, bv, br


def check_probe(cps, arena, order=None, recs=None, head=0, written=None):
    ptrs = arena.ptrs(BASE)
    g = ceph_amd.slice_plan_probe(cps, ptrs, arena.sizes, written, order,
                                  recs, head)
    blob, bs, bv, br = parent_tables(cps, ptrs, arena.sizes, order, recs, head)
    assert g["bytes"] == len(blob) and g["n_blocks"] == len(bs)
    assert np.array_equal(g["blob"], blob)
    assert list(g["block_slice"]) == bs and list(g["block_voff"]) == bv
    if recs is not None:
        assert list(g["block_rec"]) == br
    n = arena.n
    assert (g["off_ptrs"], g["off_vecs"]) == (head, head + 8 * n * cps)
    assert g["off_voff"] == g["off_vecs"] + 8 * n
    assert g["off_bslice"] == g["off_voff"] + 8 * len(bs)
    assert g["off_brec"] == g["off_bslice"] + 4 * len(bs)
    return g


def test_probe_tables_equal_the_restatement():
    for name, a in all_arenas():
        check_probe(a.cps, a)
    # the encode and decode written masks change nothing in the table
    a = cases.null_case()[0]
    check_probe(6, a, written=[0x30] * a.n)
    # multi: launch order, records, the record table in front
    for arena, masks in ((cases.multi_case()[0], cases.multi_case()[2]),
                         (cases.knob_multi_case()[0],
                          cases.knob_multi_case()[2]),
                         (cases.slot_cases()[0][0], cases.SLOT_MASKS[0]),
                         (cases.slot_cases()[1][0], cases.SLOT_MASKS[1])):
        n = arena.cps
        order, recs = cases.multi_order(n, masks)
        written = [~mk & ((1 << n) - 1) for mk in masks]
        for head in (0, 8, 2 * 3344):
            check_probe(n, arena, order, recs, head, written)
    # a permuted order without records, and one that lists a slice twice
    a = cases.decode_46_case()[0]
    check_probe(10, a, order=[8, 0, 7, 8, 3, 6])
    check_probe(10, a, order=list(range(8, -1, -1)), recs=list(range(9)))


def test_multi_list_fills_every_bucket_and_pass():
    arena, _, masks = cases.multi_case()
    n = arena.cps
    assert len(masks) == cases.MULTI_N == 48
    counts = [len(cases.erased_of(n, mk)) for mk in masks]
    assert set(counts) == {0, 1, 4, 5, 6}
    assert all(a != b for a, b in zip(counts, counts[1:]))  # neighbours differ
    plan_of, n_pass, launches = cases.multi_plan(n, masks)
    n_launches, pos, n_plans = ceph_amd.decode_multi_plan_probe(
        "cauchy", 4, 6, masks)
    # the restated grouping is the library's
    assert n_launches == len(launches) and list(pos) == plan_of
    assert n_plans == max(plan_of) + 1 and n_pass == 2
    assert [(p, o) for p, o, _ in launches] == [(0, 1), (0, 4), (1, 1), (1, 2)]
    order, recs = cases.multi_order(n, masks)
    g = ceph_amd.slice_plan_probe(n, arena.ptrs(BASE), arena.sizes,
                                  [~mk & 0x3FF for mk in masks], order, recs,
                                  8)
    one = lambda s: -(-arena.sizes[s] // (16 * g["vecs_per_block"]))
    b0 = 0
    for i, (p, o, members) in enumerate(launches):
        nb = sum(one(s) for s in members)
        # each launch holds a slice of more than one block
        assert any(one(s) > 1 for s in members), (p, o)
        # its block list starts where the previous one ended: not at 0
        assert (b0 > 0) == (i > 0)
        assert list(g["block_slice"][b0:b0 + nb]) == [
            s for s in members for _ in range(one(s))]
        for s in members:  # the record of this slice's plan and this pass
            at = b0 + sum(one(x) for x in members[:members.index(s)])
            assert set(g["block_rec"][at:at + one(s)]) == {
                plan_of[s] * n_pass + p}
        b0 += nb
    assert b0 == g["n_blocks"]


def test_probe_refusals():
    raw = ceph_amd.lib().ecx_slice_plan_probe
    cps, n = 6, 2
    out = (ctypes.c_long * 8)(*([-7] * 8))
    blob = (ctypes.c_uint8 * 4096)(*([0x77] * 4096))

    def call(ptrs, sizes, written=(0x30, 0x30), order=None, recs=None,
             head=0, n_slices=None, cps_=cps):
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        sz = (ctypes.c_size_t * len(sizes))(*sizes)
        wr = None if written is None else (ctypes.c_uint64 * n)(*written)
        o = None if order is None else (ctypes.c_int * len(order))(*order)
        r = None if recs is None else (ctypes.c_int * len(recs))(*recs)
        return raw(cps_, arr, sz, n if n_slices is None else n_slices, wr, o,
                   r, 0 if order is None else len(order), head, out, blob,
                   4096)

    good = [BASE + 64 * i for i in range(n * cps)]
    sizes = [16, 4112]
    assert call(good, sizes) == 0 and out[1] == 2 and blob[0] != 0x77
    for i in range(8):
        out[i] = -7
    for i in range(4096):
        blob[i] = 0x77

    def refused(*a, **kw):
        assert call(*a, **kw) == EINVAL, (a, kw)
        assert list(out) == [-7] * 8 and set(blob) == {0x77}

    refused(good, sizes, n_slices=0)
    refused(good, sizes, n_slices=-1)
    for bad in (0, 8, 24, 4097):
        refused(good, [bad, 4112])
        refused(good, [16, bad])
    for at in (0, 3, 4, 11):
        p = list(good)
        p[at] += 8
        refused(p, sizes)
        refused(p, sizes, written=None)
    for at in range(n * cps):
        p = list(good)
        p[at] = None
        if at % cps >= 4:  # a chunk the call writes
            refused(p, sizes)
        else:              # only read: zeros
            assert call(p, sizes) == 0
            for i in range(8):
                out[i] = -7
            for i in range(4096):
                blob[i] = 0x77
    # the written set is the slice's own
    p = list(good)
    p[0] = None
    refused(p, sizes, written=(0x01, 0x30))
    p = list(good)
    p[cps] = None
    refused(p, sizes, written=(0x30, 0x01))
    # order, records, head
    refused(good, sizes, order=[0, 2])
    refused(good, sizes, order=[-1])
    refused(good, sizes, recs=[0, 0])           # records without an order
    for head in (1, 4, 12, 3340):               # the 8-byte arrays follow it
        refused(good, sizes, order=[1, 0], recs=[0, 1], head=head)
    refused(good, sizes, cps_=0)
    refused(good, sizes, cps_=65)
    # more than 2^30 blocks
    refused(good, [16, ((1 << 30) * 16384)])
    assert raw(cps, None, (ctypes.c_size_t * 2)(16, 16), 2, None, None, None,
               0, 0, out, None, 0) == EINVAL
    assert raw(cps, (ctypes.c_void_p * 12)(*good), None, 2, None, None, None,
               0, 0, out, None, 0) == EINVAL
    assert raw(cps, (ctypes.c_void_p * 12)(*good),
               (ctypes.c_size_t * 2)(16, 16), 2, None, None, None, 0, 0, None,
               None, 0) == EINVAL
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.slice_plan_probe(cps, good, [16, 24])
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.slice_plan_probe(cps, [], [])


def test_header_and_library_agree():
    with open(os.path.join(ROOT, "include", "ec_mi355x.h")) as fh:
        text = fh.read()
    assert "ECX_API int ecx_slice_plan_probe(" in text
    assert hasattr(ceph_amd.lib(), "ecx_slice_plan_probe")


# ---- the cases can tell kernels apart ----

GENERIC = ("stride_k", "next_vecs", "past_vend")


def tells_apart(arena, image, want, blocks, recs, k, mistakes):
    right = cases.simulate(arena, image, blocks, recs)
    assert np.array_equal(right, cases.padded(want)), "model != simulation"
    for mk in mistakes:
        wrong = cases.simulate(arena, image, blocks, recs, mistake=mk, k=k)
        assert not np.array_equal(wrong, right), mk


def encode_recs(k, m, rows):
    return cases.split_recs(range(k), range(k, k + m), [list(r) for r in rows])


@pytest.mark.parametrize("k,m,tech", cases.ENCODE_CODES)
def test_encode_cases_tell_kernels_apart(k, m, tech):
    arena, want = cases.encode_case(k, m, tech)
    recs = encode_recs(k, m, cases.coding_rows(tech, k, m))
    assert len(recs) == -(-m // 4)
    mistakes = GENERIC
    if (k, m) == (3, 1):
        # the one blind spot, stated: the row of (3,1) is 1 1 1, so a vector
        # past a slice's end is poison ^ poison ^ poison = poison, stored
        # into a guard band. The one-output kernel is held to its end by the
        # second launch of (4,5) instead (below, like every other code).
        assert [int(c) for c in recs[0][2][0]] == [1, 1, 1]
        mistakes = ("stride_k", "next_vecs")
    tells_apart(arena, cases.encode_image(arena, k), want,
                cases.uniform_blocks(arena.sizes, len(recs)), recs, k,
                mistakes)
    if (k, m) == (4, 5):  # ... by its second, one-output launch alone
        blocks = cases.uniform_blocks(arena.sizes, 2)
        half = len(blocks) // 2
        first = cases.simulate(arena, cases.encode_image(arena, k),
                               blocks[:half], recs)[:arena.nbytes]
        tells_apart(arena, first, want, blocks[half:], recs, k, GENERIC)


def test_class_null_shared_cases_tell_kernels_apart():
    for rows in (cases.CLASS_ROWS, ceph_amd.shec_matrix(4, 3, 2)):
        arena, want = cases.class_case(rows)
        tells_apart(arena, cases.encode_image(arena, 4), want,
                    cases.uniform_blocks(arena.sizes), encode_recs(4, 3, rows),
                    4, GENERIC + ("cls0_as_1",))
    # the all-zero row's output is zeros in the model
    arena, want = cases.class_case(cases.CLASS_ROWS)
    for s in range(arena.n):
        assert not arena.chunk(want, s, 4 + cases.CLASS_ZERO_ROW).any()
    rows = cases.coding_rows("reed_sol_van", 4, 2)
    arena, want = cases.null_case()
    tells_apart(arena, cases.encode_image(arena, 4), want,
                cases.uniform_blocks(arena.sizes), encode_recs(4, 2, rows), 4,
                GENERIC + ("null_poison",))
    for c in (4, 5):
        assert not arena.chunk(want, cases.NULL_ALL, c).any()
    arena, want = cases.shared_case()
    tells_apart(arena, cases.encode_image(arena, 4), want,
                cases.uniform_blocks(arena.sizes), encode_recs(4, 2, rows), 4,
                GENERIC)


def test_decode_cases_tell_kernels_apart():
    for (arena, truth), masks, tech, k, m, extra in (
            (cases.decode_42_case(), cases.DECODE_42_MASKS, "reed_sol_van", 4,
             2, ()),
            (cases.decode_46_case(), cases.DECODE_46_MASKS, "cauchy", 4, 6,
             ()),
            (cases.decode_null_case(), [cases.DECODE_NULL_MASK],
             "reed_sol_van", 4, 2, ("null_poison",)),
            (cases.knob_decode_case()[:2], [cases.knob_decode_case()[2]],
             "cauchy", 4, 6, ("null_poison",))):
        f = rows_of(tech, k, m)
        for mk in masks:
            recs = cases.split_recs(*f(mk))
            tells_apart(arena, cases.erase(arena, truth, [mk] * arena.n),
                        truth, cases.uniform_blocks(arena.sizes, len(recs)),
                        recs, k, GENERIC + extra)


def test_multi_cases_tell_kernels_apart():
    sets = [cases.multi_case(), cases.knob_multi_case()]
    sets += [(a, tr, cases.SLOT_MASKS[i])
             for i, (a, tr) in enumerate(cases.slot_cases())]
    for i, (arena, truth, masks) in enumerate(sets):
        n = arena.cps
        f = rows_of("cauchy" if n == 10 else "reed_sol_van", 4, n - 4)
        mistakes = GENERIC + ("prev_rec",)
        if arena.null:
            mistakes += ("null_poison",)
        tells_apart(arena, cases.erase(arena, truth, masks), truth,
                    cases.multi_blocks(n, arena.sizes, masks),
                    cases.multi_recs(n, masks, f), 4, mistakes)


def test_growth_cases_model_is_the_simulation():
    rows = cases.coding_rows("reed_sol_van", 4, 2)
    for arena, want in cases.growth_cases():
        tells_apart(arena, cases.encode_image(arena, 4), want,
                    cases.uniform_blocks(arena.sizes), encode_recs(4, 2, rows),
                    4, ("past_vend",))


def test_plan_check_tool_under_sanitizers(tmp_path):
    """tools/slice_plan_check.cc (its own main, plain C++) built with
    -fsanitize=address,undefined and run as a process of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++)")
    exe = str(tmp_path / "slice_plan_check")
    # the sanitizer runtimes linked into the program itself: it then runs
    # the same whatever else the environment loads into a process
    subprocess.run(
        [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tools", "slice_plan_check.cc"),
         os.path.join(ROOT, "ceph_amd", "csrc", "slice_plan.cpp"), "-o", exe],
        check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "slice_plan_check: ok" in r.stdout
