"""CPU checks of tests/bitmatrix_cases.py: the numpy references equal the
oracle's own routines at every shape the GPU tests use, the case tables reach
the kernel instances they claim by the arithmetic restated in
bitmatrix_cases.geometry(), and geometry() agrees with the plan the launcher
itself launches by (ceph_amd.bitmatrix_plan_probe, the bit_plan() of
run_bitmatrix) at every launch of the GPU files. A later change of the
launcher's selection or defaults fails here instead of silently no longer
reaching an instance. Nothing here needs a GPU."""
import numpy as np
import pytest

import ceph_amd
import oracle
import bitmatrix_cases as cases


def gpu_bit_shapes():
    """Every (tech, k, m, pkt) of the GPU files, at one superword."""
    s = {(t, k, m, pkt) for t, k, m, pkt, _ in cases.encode_cases()}
    s |= {(t, k, m, pkt) for t, k, m, pkt, _, _ in cases.KNOB_ENCODES}
    s |= {(t, k, m, pkt) for t, k, m, pkt, _, _, _ in cases.KNOB_DECODES}
    s |= {("cauchy_orig", k, m, pkt) for k, m, pkt, _ in cases.REG_SHAPES}
    s |= {("cauchy_orig", 3, 3, pkt) for pkt, _, _, _ in cases.KNOB_DELTAS}
    s |= {("cauchy_orig", 4, 3, 48), ("cauchy_orig", 4, 8, 48),
          ("cauchy_orig", 4, 8, 2048)}
    h = cases.HOST_PATH
    s.add(("cauchy_orig", h["k"], h["m"], h["pkt"]))
    return sorted(s)


# the shapes at which this reference was first checked against the oracle
ISSUE_SHAPES = [("cauchy_orig", 3, 3, 48), ("cauchy_orig", 5, 3, 16),
                ("cauchy_orig", 8, 3, 16), ("cauchy_orig", 7, 3, 2048),
                ("cauchy_orig", 16, 4, 2048), ("cauchy_orig", 3, 3, 96),
                ("cauchy_orig", 2, 1, 4096), ("cauchy_good", 2, 3, 4096)]


@pytest.mark.parametrize("tech,k,m,pkt",
                         sorted(set(gpu_bit_shapes() + ISSUE_SHAPES)))
def test_ref_bit_is_the_oracle_encode(tech, k, m, pkt):
    n_sw = 2 if pkt <= 256 else 1
    full = cases.encoded_bit(tech, k, m, pkt, n_sw, 1)
    want = oracle.bitmatrix_encode(
        k, m, [full[0, i].copy() for i in range(k)], pkt, technique=tech)
    for j in range(m):
        assert np.array_equal(full[0, k + j], want[j]), j


@pytest.mark.parametrize("tech,k,m,pkt,erased", [
    ("cauchy_orig", 4, 3, 48, (0, 2, 5)),
    ("cauchy_orig", 4, 8, 48, cases.PATTERNS_48[0]),
    ("cauchy_orig", 4, 8, 48, cases.PATTERNS_48[1]),
    ("cauchy_good", 7, 3, 2048, (1, 8)),
    ("cauchy_orig", 4, 9, 48, cases.HOST_PATH["erased"]),
])
def test_ref_bit_round_trips_through_the_oracle_decode(tech, k, m, pkt,
                                                       erased):
    full = cases.encoded_bit(tech, k, m, pkt, 2, 1)
    present = [i not in erased for i in range(k + m)]
    chunks = [full[0, i].copy() if present[i]
              else np.full(full.shape[2], cases.POISON, np.uint8)
              for i in range(k + m)]
    oracle.bitmatrix_decode(k, m, chunks, present, pkt, technique=tech)
    for i in range(k + m):
        assert np.array_equal(chunks[i], full[0, i]), i


def test_ref_bit_accumulates():
    """accum XORs the product into the output's old bytes."""
    pkt, C = 48, 2 * 8 * 48
    rows = cases.encode_rows("cauchy_orig", 3, 3)[8:16, 16:24]
    buf = cases.rand_batch(1, 1, 2, C)
    old = buf[0, 1].copy()
    plain = buf.copy()
    cases.ref_bit(plain, [0], [1], rows, pkt)
    cases.ref_bit(buf, [0], [1], rows, pkt, accum=True)
    assert np.array_equal(buf[0, 1], old ^ plain[0, 1])
    assert np.array_equal(buf[0, 0], plain[0, 0])


def test_gf16_tables_are_the_oracle_field():
    rng = np.random.default_rng(16)
    xs = rng.integers(0, 65536, 64).astype(np.uint16)
    for c in (0, 1, 2, 0x100B, 0xFFFF, 0x8000, 0x1234):
        got = cases.gf16_mul_vec(c, xs)
        assert [int(g) for g in got] == [oracle.gf16_mul(c, int(x))
                                         for x in xs]


@pytest.mark.parametrize("k,m,C", [(4, 2, 4112), (4, 6, 4112), (4, 3, 4112),
                                   (2, 1, 8208), (2, 2, 8208), (3, 2, 16),
                                   (3, 4, 4112)])
def test_ref16_is_the_oracle_encode(k, m, C):
    full = cases.encoded16(k, m, 1, C)
    want = oracle.encode_w16(k, m, [full[0, i].copy() for i in range(k)])
    for j in range(m):
        assert np.array_equal(full[0, k + j], want[j]), j


@pytest.mark.parametrize("k,m,erased", [(4, 3, (0, 3, 5)),
                                        (4, 6, (0, 1, 2, 3, 4, 9)),
                                        (4, 6, (1, 3, 5, 6, 8))])
def test_ref16_round_trips_through_the_oracle_decode(k, m, erased):
    full = cases.encoded16(k, m, 1, 4112)
    present = [i not in erased for i in range(k + m)]
    chunks = [full[0, i].copy() if present[i]
              else np.full(4112, cases.POISON, np.uint8)
              for i in range(k + m)]
    oracle.decode_w16(k, m, chunks, present)
    for i in range(k + m):
        assert np.array_equal(chunks[i], full[0, i]), i


# ---- the case tables against the launcher's arithmetic ----

def test_default_shapes_reach_their_instances():
    for (k, pkt, n_sw), want in cases.LDS_SHAPES.items():
        g = cases.geometry(k, pkt, n_sw)
        assert g["kernel"] == "lds"
        got = {f: g[f] for f in want}
        assert got == want, (k, pkt, n_sw, got)
        assert n_sw * 8 * pkt < 200 * 1024
    # every VQS instance under both stagings of the generic one
    seen = {(v["vqs"], v["staging"]) for v in cases.LDS_SHAPES.values()}
    assert seen == {(-1, "dma"), (-1, "reg"), (3, "dma"), (4, "dma"),
                    (5, "dma")}
    # a window count per superword that is no power of two; q below 32
    assert any(v["wps"] == 3 for v in cases.LDS_SHAPES.values())
    assert any(v["q"] == 16 for v in cases.LDS_SHAPES.values())


def test_default_shapes_walk_edges():
    for (k, pkt, n_sw), (nwin, grid, last) in cases.WALK_EDGES.items():
        assert (k, pkt, n_sw) in cases.LDS_SHAPES
        g = cases.geometry(k, pkt, n_sw)
        assert (g["n_windows"], g["grid"], g["last_block"]) == \
            (nwin, grid, last), (k, pkt, n_sw, g)
    # 14 wave-chunks over 4 waves; 10; one
    assert cases.geometry(7, 2048, 3)["items"] == 14 * 64
    assert cases.geometry(5, 256, 9)["items"] == 10 * 64
    assert cases.geometry(4, 32, 3)["items"] == 64
    assert cases.geometry(8, 16, 1)["items"] == 64
    assert [cases.geometry(k, p, s)["items"] for k, p, s in
            ((3, 48, 5), (3, 96, 2), (5, 16, 3))] == [24, 48, 40]


def test_default_single_output_takes_the_register_kernel():
    want_pos = {(16, 1): 1, (48, 5): 15, (2048, 3): 384}
    for k, m, pkt, n_sw in cases.REG_SHAPES:
        for accum, n_src in ((False, k), (True, 1)):
            g = cases.geometry(n_src, pkt, n_sw, n_out=1, accum=accum)
            assert g["kernel"] == "reg" and g["nr"] == 8
            assert g["n_pos"] == want_pos[(pkt, n_sw)]
    assert cases.geometry(3, 2048, 3, n_out=1)["grid"] == 2
    # two and more outputs do not
    assert cases.geometry(4, 48, 5, n_out=2)["kernel"] == "lds"


def launches(knobs):
    return cases.knob_launches(knobs)


def find(knobs, **want):
    return [g for g in launches(knobs)
            if all(g.get(f) == v for f, v in want.items())]


def test_no_case_needs_more_than_64k_of_lds():
    for knobs in [{}] + cases.KNOBS:
        for g in launches(knobs):
            if g["kernel"] != "reg":
                assert g["lds_bound"] <= 64 * 1024, (knobs, g)
    for (k, pkt, n_sw) in cases.LDS_SHAPES:
        g = cases.geometry(k, pkt, n_sw, n_out=8)
        assert g["lds_bound"] <= 64 * 1024


def test_knob_cases_reach_their_instances():
    K = cases.KNOBS
    # ECX_BITREG=0: accumulation and one output through the LDS kernel; the
    # delta's single source gives q = 2048 (generic) and 8 items (register
    # staging)
    k0 = {"ECX_BITREG": "0"}
    assert k0 in K and not find(k0, kernel="reg")
    assert find(k0, kernel="lds", accum=True, q=2048, vqs=-1, staging="dma")
    assert find(k0, kernel="lds", accum=True, items=8, staging="reg")
    assert find(k0, kernel="lds", accum=False, vqs=4)
    for vqs in (3, 4, 5):  # the delta at pkt 128, 256, 512
        assert find(k0, kernel="lds", accum=True, vqs=vqs, staging="dma")
    for plain in ({"ECX_NT": "0", "ECX_BITREG": "0"},
                  {"ECX_NT": "0", "ECX_BITREG": "1"},
                  {"ECX_BITPIPE": "1", "ECX_NT": "0", "ECX_BITREG": "0"}):
        assert plain in K
    # ECX_BITREG=1: NR 16, 24, 32; five outputs stay on the LDS kernel
    k1 = {"ECX_BITREG": "1"}
    assert k1 in K
    assert {g["nr"] for g in find(k1, kernel="reg")} == {8, 16, 24, 32}
    assert find(k1, kernel="lds")
    assert cases.knob_geometry(k1, 7, 2048, 3, 5)["kernel"] == "lds"
    # ECX_NT=0: both kernels, both ACCUM values of the register kernel
    nt = {"ECX_NT": "0"}
    assert nt in K and find(nt, kernel="lds")
    assert find(nt, kernel="reg", accum=True)
    assert find(nt, kernel="reg", accum=False)
    # ECX_BITW=3: partial last blocks (12, 15 and 24 windows)
    w3 = {"ECX_BITW": "3"}
    assert w3 in K
    assert {(g["n_windows"], g["last_block"]) for g in find(w3, kernel="lds")
            } >= {(12, 3), (15, 3), (24, 3), (16, 1)}
    w1 = {"ECX_BITW": "1"}
    assert w1 in K and all(g["grid"] == g["n_windows"]
                           for g in find(w1, kernel="lds"))
    # ECX_BITQ=8: k = 16 at pkt 2048 leaves the VQS set
    q8 = {"ECX_BITQ": "8"}
    assert q8 in K
    assert cases.knob_geometry(q8, 16, 2048, 1, 3)["q"] == 64
    assert cases.knob_geometry(q8, 16, 2048, 1, 3)["vqs"] == -1
    # ECX_BITPIPE=1: the pipe kernel where the items fill whole waves and a
    # block has more than one window, else the LDS kernel
    p = {"ECX_BITPIPE": "1"}
    assert p in K
    assert find(p, kernel="pipe", items=14 * 64)      # uneven over 4 waves
    assert find(p, kernel="pipe", items=64)           # fewer chunks than waves
    assert find(p, kernel="lds", staging="reg")       # must fall back
    assert not find(p, kernel="pipe", staging="reg")
    p3 = {"ECX_BITPIPE": "1", "ECX_BITW": "3"}
    assert p3 in K
    assert {g["last_block"] for g in find(p3, kernel="pipe")} >= {1, 3}
    p1 = {"ECX_BITPIPE": "1", "ECX_BITW": "1"}
    assert p1 in K and not find(p1, kernel="pipe")
    pa = {"ECX_BITPIPE": "1", "ECX_BITREG": "0"}
    assert pa in K and find(pa, kernel="pipe", accum=True)
    assert find(pa, kernel="lds", accum=True)
    # ECX_BITXCD=1 with ECX_BITW=1: one and two groups of 64 blocks; a
    # three-superword chunk keeps the normal walk
    x = {"ECX_BITXCD": "1", "ECX_BITW": "1"}
    assert x in K
    assert sorted(g["grid"] for g in find(x, xcdmap=True)) == [64, 128]
    g3 = cases.knob_geometry(x, 16, 1024, 3, 3)
    assert (g3["q"], g3["wps"], g3["xcdmap"]) == (128, 8, False)
    for other in ({"ECX_BITT": "128"}, {"ECX_BITT": "64"},
                  {"ECX_BITSTAGGER": "2"},
                  {"ECX_BITPIPE": "1", "ECX_NT": "0"}):
        assert other in K


# ---- geometry() against the launcher's own plan ----
# geometry() is an independent restatement; bitmatrix_plan_probe runs the
# bit_plan() that run_bitmatrix launches by. While the two agree, a case that
# geometry() says reaches an instance does reach it.

REG_FIELDS = ("kernel", "nr", "n_pos", "grid")
LDS_FIELDS = ("kernel", "grid", "q", "vqs", "staging", "items", "wps",
              "n_windows", "xcdmap")


def popcount(rows):
    return int(np.count_nonzero(rows))


def gf_inverse(a):
    """Inverse of a square GF(2^8) matrix, by the oracle's field."""
    n = len(a)
    a = [[int(x) for x in row] + [int(i == j) for j in range(n)]
         for i, row in enumerate(a)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c])
        a[c], a[p] = a[p], a[c]
        inv = oracle.gf_inv(a[c][c])
        a[c] = [oracle.gf_mul(inv, x) for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [x ^ oracle.gf_mul(f, y) for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def decode_rows(tech, k, m, erased):
    """Bit rows that rebuild the erased chunks from the first k present."""
    gen = oracle.matrix(tech, k, m)
    surv = [i for i in range(k + m) if i not in erased][:k]
    inv = gf_inverse([gen[s] for s in surv])
    rows = np.zeros((len(erased), k), np.uint8)
    for j, e in enumerate(erased):
        for c in range(k):
            for i in range(k):
                rows[j, c] ^= oracle.gf_mul(int(gen[e][i]), inv[i][c])
    return oracle.bitmatrix(rows)


def check_plan(g, knobs, n_src, pkt, n_sw, n_out, rows):
    assert np.shape(rows) == (8 * n_out, 8 * n_src)
    got = ceph_amd.bitmatrix_plan_probe(n_src, n_out, pkt, n_sw * 8 * pkt,
                                        popcount(rows), knobs)
    fields = REG_FIELDS if g["kernel"] == "reg" else LDS_FIELDS
    assert {f: got[f] for f in fields} == {f: g[f] for f in fields}, \
        (knobs, n_src, pkt, n_sw, n_out)
    if g["kernel"] != "reg":
        assert got["lds_bytes"] <= g["lds_bound"]


def delta_rows(data, coding):
    return cases.encode_rows("cauchy_orig", 3, 3)[
        8 * (coding - 3):8 * (coding - 2), 8 * data:8 * data + 8]


@pytest.mark.parametrize("knobs", [{}] + cases.KNOBS,
                         ids=lambda kn: "-".join(
                             f"{n[4:]}{v}" for n, v in kn.items()) or "default")
def test_plan_probe_agrees_with_geometry_on_every_knob_launch(knobs):
    want = iter(cases.knob_launches(knobs))
    for tech, k, m, pkt, n_sw, _ in cases.KNOB_ENCODES:
        g = cases.knob_geometry(knobs, k, pkt, n_sw, m)
        assert g == next(want)
        check_plan(g, knobs, k, pkt, n_sw, m, cases.encode_rows(tech, k, m))
    for tech, k, m, pkt, n_sw, _, er in cases.KNOB_DECODES:
        g = cases.knob_geometry(knobs, k, pkt, n_sw, len(er))
        assert g == next(want)
        check_plan(g, knobs, k, pkt, n_sw, len(er),
                   decode_rows(tech, k, m, er))
    for pkt, n_sw, data, coding in cases.KNOB_DELTAS:
        g = cases.knob_geometry(knobs, 1, pkt, n_sw, 1, accum=True)
        assert g == next(want)
        check_plan(g, knobs, 1, pkt, n_sw, 1, delta_rows(data, coding))
    assert next(want, None) is None


def test_plan_probe_agrees_with_geometry_on_the_default_shapes():
    for (k, pkt, n_sw) in cases.LDS_SHAPES:
        for n_out in (1, 2, 3, 5, 8):
            rows = cases.encode_rows("cauchy_orig", k, 8)[:8 * n_out]
            check_plan(cases.geometry(k, pkt, n_sw, n_out=n_out), {}, k, pkt,
                       n_sw, n_out, rows)
    for k, m, pkt, n_sw in cases.REG_SHAPES:
        rows = cases.encode_rows("cauchy_orig", k, m)
        g = cases.geometry(k, pkt, n_sw, n_out=1)
        assert g["kernel"] == "reg"
        check_plan(g, {}, k, pkt, n_sw, 1, rows[:8])
        check_plan(cases.geometry(1, pkt, n_sw, n_out=1, accum=True), {}, 1,
                   pkt, n_sw, 1, rows[:8, :8])
    for pkt, n_sw, data, coding in cases.KNOB_DELTAS:
        check_plan(cases.geometry(1, pkt, n_sw, n_out=1, accum=True), {}, 1,
                   pkt, n_sw, 1, delta_rows(data, coding))


def test_plan_probe_clamps_like_the_launcher():
    """ECX_BITQ 8..120, ECX_BITW 1..4096, ECX_BITT 64/128/256 else 256."""
    def probe(**kn):
        return ceph_amd.bitmatrix_plan_probe(16, 3, 2048, 8 * 2048, 700, kn)
    assert probe(ECX_BITQ=1) == probe(ECX_BITQ=8)
    assert probe(ECX_BITQ=999) == probe(ECX_BITQ=120)
    # 16 sources: the new window's 128 * q bytes within the budget
    assert [probe(ECX_BITQ=b)["q"] for b in (8, 16, 120)] == [64, 128, 512]
    assert probe(ECX_BITW=0) == probe(ECX_BITW=1)
    assert probe(ECX_BITW=5000)["wpb"] == 4096
    assert [probe(ECX_BITT=t)["threads"] for t in (64, 128, 256, 96, 512)] \
        == [64, 128, 256, 256, 256]
    assert probe(ECX_BITPIPE=1, ECX_BITT=64)["threads"] == 256


@pytest.mark.parametrize("n_src,n_out,pkt,chunk", [
    (0, 3, 2048, 16384), (17, 3, 2048, 16384),
    (4, 0, 2048, 16384), (4, 9, 2048, 16384),
    (4, 3, 2048, 16384 + 2048), (4, 3, 2048, 0),
    (4, 3, 8, 64), (4, 3, 24, 192),
])
def test_plan_probe_refuses_what_the_launcher_refuses(n_src, n_out, pkt,
                                                      chunk):
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.bitmatrix_plan_probe(n_src, n_out, pkt, chunk, 100)


def test_plan_probe_refuses_an_op_list_past_u16_on_the_lds_kernels_only():
    with pytest.raises(ceph_amd.EcError, match="EINVAL"):
        ceph_amd.bitmatrix_plan_probe(4, 2, 2048, 16384, 0x10000)
    assert ceph_amd.bitmatrix_plan_probe(4, 2, 2048, 16384, 0xffff)
    assert ceph_amd.bitmatrix_plan_probe(4, 1, 2048, 16384,
                                         0x10000)["kernel"] == "reg"


def test_w16_grids():
    """run_matmul16's grid, restated: the sizes meet a single vector, a
    partial tile, an idle block and a second grid-stride trip."""
    assert cases.w16_grid(16, 1) == (1, 1, 1)
    assert cases.w16_grid(4112, 1) == (2, 2, 1)
    assert cases.w16_grid(12304, 1) == (4, 4, 1)
    assert cases.w16_grid(12272, 3) == (4, 3, 1)   # the doubling overshoots
    L = cases.W16_LONG
    assert cases.w16_grid(L["C"], L["S"]) == (2, 3, 2)
    assert L["C"] // 16 == 2 * 256 + 1             # one-vector tail
    T = cases.W16_LONG_TABLES
    assert cases.w16_grid(T["C"], T["S"]) == (2, 3, 2)
    assert (oracle.matrix_w16(T["k"], T["m"])[T["k"] + 1] > 1).any()
