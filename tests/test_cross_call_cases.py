"""CPU checks of tests/cross_call_cases.py, what test_gpu_big_batch.py,
test_gpu_chained_calls.py and test_gpu_lru_overflow.py are built on: the
sample set of the batch past 4 GiB covers what it claims, the host model of
the chained calls agrees with the oracle, every mask of the cache-overflow
set is decodable, and the set is larger than the cache. Nothing here needs a
GPU."""
import os
import re

import numpy as np

import ceph_amd
import oracle
import cross_call_cases as cc
from decode_multi_cases import erased_of
from test_gpu_verify import expected_word

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the batch past 4 GiB ----------------------------------------------------

def big_shapes():
    return [(cc.BIG["S"], cc.BIG["k"] + cc.BIG["m"], cc.BIG["C"]),
            (cc.BIG_BIT["S"], cc.BIG_BIT["k"] + cc.BIG_BIT["m"],
             cc.BIG_BIT["C"])]


def test_big_sample_covers_lines_alias_zone_and_tail():
    for S, n, C in big_shapes():
        total, sb = S * n * C, n * C
        assert total > cc.LINE32 and sb % 8 == 0
        stripes, lines, unchecked = cc.big_sample(S, n, C)
        assert stripes == sorted(set(stripes))
        # the stripe of each line, by the bytes it spans, and its neighbours
        for line, want_stripe in ((cc.LINE31, 341), (cc.LINE32, 682)):
            s, c, off = lines[line]
            assert s == want_stripe
            assert s * sb <= line < (s + 1) * sb
            assert (s * n + c) * C + off == line and 0 < off < C
            assert {s - 1, s, s + 1} <= set(stripes)
        assert lines[cc.LINE32][1] == 3  # inside data chunk 3
        # every stripe overlapping [0, total - 2^32)
        wrap = total - cc.LINE32
        for s in range(S):
            if s * sb < wrap:
                assert s in stripes, s
        # every stripe reaching past 2^32 is sampled or listed; none is left
        for s in range(S):
            if (s + 1) * sb > cc.LINE32:
                assert s in stripes or s in unchecked, s
        assert unchecked == []
        assert stripes == (list(range(19)) + [340, 341, 342] +
                           list(range(681, 700)))


def test_big_sample_sees_any_offset_cut_to_32_bits():
    """The teeth of the big-batch cases, on the CPU: wherever a kernel might
    cut an offset to 32 bits — the stripe's base, the chunk's offset in the
    batch, or the whole byte offset — every chunk that lies past 2^32 moves
    to another place, and that place is inside a sampled stripe. So the
    wrong bytes of the write, and the missing bytes at the right place, are
    both in stripes the cases compare."""
    for S, n, C in big_shapes():
        sb = n * C
        stripes = set(cc.big_sample(S, n, C)[0])
        moved = 0
        for s in range(S):
            for c in range(n):
                for off in (0, C - 16):
                    true = s * sb + c * C + off
                    cuts = {(s * sb) % cc.LINE32 + c * C + off,
                            ((s * n + c) * C) % cc.LINE32 + off,
                            true % cc.LINE32}
                    for cut in cuts - {true}:
                        moved += 1
                        assert s in stripes, s
                        assert cut // sb in stripes, (s, c, cut // sb)
        assert moved


def test_big_masks():
    S, k, n = cc.BIG["S"], cc.BIG["k"], cc.BIG["k"] + cc.BIG["m"]
    stripes, lines, _ = cc.big_sample(S, n, cc.BIG["C"])
    dm = cc.big_decode_masks(S, n, stripes, lines)
    counts = [len(erased_of(n, mk)) for mk in dm]
    assert set(counts) == {0, 1, 2}
    assert all(counts[s] >= 1 for s in stripes)
    assert 3 in erased_of(n, dm[682]) and counts[699] == 2
    launches, _, _ = ceph_amd.decode_multi_plan_probe("reed_sol_van", k,
                                                      cc.BIG["m"], dm)
    assert launches == 2
    wm = cc.big_write_masks(S, k, stripes, lines)
    assert all(0 < wm[s] < 1 << k for s in stripes) and wm[682] & 8
    rest = [wm[s] for s in range(S) if s not in stripes]
    assert 0 < sum(1 for mk in rest if mk) < len(rest) // 5
    base, total = cc.new_bases(wm)
    _, probe_base, active = ceph_amd.update_plan_probe(k, cc.BIG["m"], wm)
    assert list(probe_base) == [int(b) for b in base]
    assert list(active) == [s for s in range(S) if wm[s]]
    assert total * cc.BIG["C"] < 1 << 31  # d_new stays far under 4 GiB


# ---- chained calls -----------------------------------------------------------

def test_chain_host_model_against_the_oracle():
    """On four stripes: after the modelled update the parity is the oracle's
    encode of the new data, the update wrote the chunks of its mask and no
    others, and the verify reference flags exactly the stripes in which a
    chunk was poisoned."""
    tech, k, m, C, S = (cc.CHAIN[x] for x in ("tech", "k", "m", "C", "S"))
    n = k + m
    for rnd in range(cc.CHAIN_ROUNDS):
        seeds = cc.chain_seeds(rnd)
        wm = cc.chain_write_masks(rnd, S)
        dm = cc.chain_decode_masks(rnd, S)
        # the first stripes that lose 0, 1, 4 and 6 chunks
        stripes = sorted(next(s for s in range(S)
                              if len(erased_of(n, dm[s])) == e)
                         for e in (0, 1, 4, 6))
        mod = cc.chain_model(tech, k, m, C, stripes, seeds, wm, dm)
        new = cc.packed_new(stripes, wm, C, seeds[1])
        at = 0
        for i, s in enumerate(stripes):
            enc, upd = mod["enc"][i], mod["upd"][i]
            par = oracle.encode(tech, k, m, [enc[j].copy() for j in range(k)])
            assert all(np.array_equal(par[r], enc[k + r]) for r in range(m))
            for j in range(k):
                if wm[s] >> j & 1:
                    assert np.array_equal(upd[j], new[at])
                    at += 1
                else:
                    assert np.array_equal(upd[j], enc[j])
            par = oracle.encode(tech, k, m, [upd[j].copy() for j in range(k)])
            assert all(np.array_equal(par[r], upd[k + r]) for r in range(m))
            word = expected_word(tech, k, m, list(mod["poisoned"][i]),
                                 (1 << n) - 1)
            assert (word != 0) == bool(erased_of(n, dm[s])), (rnd, s, word)
            assert expected_word(tech, k, m, list(upd), (1 << n) - 1) == 0
        assert at == len(new)


def test_chain_masks_and_samples():
    S, n = cc.CHAIN["S"], cc.CHAIN["k"] + cc.CHAIN["m"]
    seen = set()
    for lane in range(3):
        smp = cc.chain_sample(S // (2 if lane else 1), lane)
        assert len(set(smp)) == 32 and smp[0] == 0
        for rnd in range(cc.CHAIN_ROUNDS):
            dm = cc.chain_decode_masks(rnd, S, n, lane)
            wm = cc.chain_write_masks(rnd, S, cc.CHAIN["k"], lane)
            assert {len(erased_of(n, mk)) for mk in dm} == {0, 1, 4, 5, 6}
            assert {bin(mk).count("1") for mk in wm} == {0, 1, 2, 3, 4}
            # the poisoned sampled stripes include two-pass decodes
            assert {len(erased_of(n, dm[s])) for s in smp} >= {0, 1, 5, 6}
            seen.add((tuple(dm), tuple(wm)) + cc.chain_seeds(rnd, lane))
    assert len(seen) == 3 * cc.CHAIN_ROUNDS  # every ring entry changes


# ---- more decode plans than the cache holds ---------------------------------

def test_lru_masks_are_decodable_by_the_reference():
    tech, k, m, C = (cc.LRU[x] for x in ("tech", "k", "m", "C"))
    n = k + m
    masks = cc.lru_masks()
    assert len(masks) == len(set(masks)) == 6195
    data = [np.random.default_rng(i).integers(0, 256, C, dtype=np.uint8)
            for i in range(k)]
    stripe = data + oracle.encode(tech, k, m, data)
    for mk in masks:
        er = erased_of(n, mk)
        assert 1 <= len(er) <= m
        chunks = [c.copy() for c in stripe]
        for e in er:
            chunks[e][:] = cc.POISON
        oracle.decode(tech, k, m, chunks, [mk >> i & 1 for i in range(n)])
        assert all(np.array_equal(a, b) for a, b in zip(chunks, stripe)), \
            hex(mk)
    launches, pos, n_plans = ceph_amd.decode_multi_plan_probe(tech, k, m,
                                                              masks)
    assert n_plans == 6195 and launches == m
    assert list(pos) == list(range(6195))
    for mk in cc.lru_verify_masks():
        _, checked, _ = ceph_amd.verify_plan_probe(tech, k, m, mk)
        assert 1 <= len(checked) == m - len(erased_of(n, mk))


def test_lru_mask_set_is_larger_than_the_cache():
    """A later change of the depth fails here instead of turning
    test_gpu_lru_overflow.py into a test of nothing."""
    src = os.path.join(os.path.dirname(HERE), "ceph_amd", "csrc",
                       "ec_core.hip")
    with open(src) as f:
        found = re.findall(r"\bLRU_DEPTH\s*=\s*(\d+)\s*;", f.read())
    assert len(found) == 1, found
    assert len(cc.lru_masks()) > int(found[0])
