"""Shapes, sample sets, masks and the host model shared by
test_gpu_big_batch.py (a batch past 4 GiB), test_gpu_chained_calls.py (calls
chained on a slot with one sync at the end) and test_gpu_lru_overflow.py
(more decode plans than the context's cache holds), and by the CPU tests in
those files that check what is chosen here. Not a test module. Everything is
seeded; nothing here touches the GPU or the code under test. The arithmetic
is the suite's own: test_gpu_stream_kernel.ref_matmul, update_cases.
delta_expect, bench.expected_fill. See CROSS_CALL_COVERAGE.md."""
import random
from itertools import combinations

import numpy as np

import oracle
import update_cases
from bench import expected_fill
from decode_multi_cases import erased_of, mask_without
from test_gpu_stream_kernel import ref_matmul

POISON = 0xA5

# ---------------------------------------------------------------------------
# the batch past 4 GiB
# ---------------------------------------------------------------------------

LINE31, LINE32 = 1 << 31, 1 << 32
# C = 1 MiB + 16: a partial last tile, and no power of two, so both lines
# fall inside a chunk. 700 stripes of 6 chunks are 4,404,086,400 bytes.
BIG = dict(k=4, m=2, S=700, C=(1 << 20) + 16)
# the bitmatrix context: a multiple of w * packetsize = 8 * 16
BIG_BIT = dict(k=4, m=2, S=700, C=(1 << 20) + 128, pkt=16)
BIG_SEED, BIG_NEW_SEED = 0xB16BA7C4, 0x5EC07D


def locate(byte, n, C):
    """(stripe, chunk, offset in the chunk) of a byte offset of the batch."""
    s, r = divmod(byte, n * C)
    return (s,) + divmod(r, C)


def big_sample(S, n, C):
    """The stripes a big-batch test downloads, from the shape alone:
    - the stripes overlapping [0, total - 2^32), where an offset that
      wrapped at 32 bits lands, and one more (a wrapped stripe base plus an
      unwrapped offset inside the stripe ends in it);
    - the stripe holding byte 2^31 and the one holding byte 2^32, each with
      both neighbours;
    - every stripe from the one holding byte 2^32 to the last.
    Returns (stripes ascending, lines, unchecked): lines maps each line to
    its (stripe, chunk, offset), unchecked lists the stripes reaching past
    2^32 that are not in the set."""
    total = S * n * C
    sb = n * C
    pick, lines = {0, S - 1}, {}
    for line in (LINE31, LINE32):
        if line < total:
            lines[line] = locate(line, n, C)
            s = lines[line][0]
            pick.update(x for x in (s - 1, s, s + 1) if 0 <= x < S)
    past = []
    if total > LINE32:
        wrap = total - LINE32
        pick.update(range(min(S, (wrap - 1) // sb + 2)))
        past = list(range(LINE32 // sb, S))
        pick.update(past[-18:])
    stripes = sorted(pick)
    return stripes, lines, [s for s in past if s not in pick]


def big_decode_masks(S, n, stripes, lines):
    """0-2 erasures per stripe; every sampled stripe loses at least one
    chunk, the stripe of the 2^32 line loses the chunk the line cuts, the
    last stripe loses two."""
    rng = random.Random(0xB16D)
    sampled = set(stripes)
    masks = []
    for s in range(S):
        e = rng.randrange(1, 3) if s in sampled else rng.randrange(0, 3)
        er = rng.sample(range(n), e)
        if LINE32 in lines and s == lines[LINE32][0]:
            er = [lines[LINE32][1]] + [c for c in er
                                       if c != lines[LINE32][1]][:e - 1]
        if s == S - 1:
            er = rng.sample(range(n), 2)
        masks.append(mask_without(n, er))
    return masks


def big_write_masks(S, k, stripes, lines):
    """Nonzero on every sampled stripe and on a seeded tenth of the others;
    the stripe of the 2^32 line rewrites the chunk the line cuts when that
    is a data chunk."""
    rng = random.Random(0xB16E)
    sampled = set(stripes)
    masks = []
    for s in range(S):
        mk = rng.randrange(1, 1 << k)
        if s not in sampled and rng.randrange(10):
            mk = 0
        if LINE32 in lines and s == lines[LINE32][0] and lines[LINE32][1] < k:
            mk |= 1 << lines[LINE32][1]
        masks.append(mk)
    return masks


def new_bases(write_masks):
    """Index of each stripe's first new chunk in the packed d_new."""
    counts = [bin(mk).count("1") for mk in write_masks]
    return [0] + list(np.cumsum(counts)[:-1]), sum(counts)


def filled_stripes(stripes, n, C, seed):
    """(len(stripes), n, C): what fill_random(seed) leaves in these stripes
    of a batch."""
    return np.stack([expected_fill(s * n * C, n * C, seed).reshape(n, C)
                     for s in stripes])


def packed_new(stripes, write_masks, C, seed):
    """The new chunks of these stripes, in d_new's order, out of a d_new
    that fill_random(seed) filled."""
    base, _ = new_bases(write_masks)
    out = [expected_fill((base[s] + t) * C, C, seed)
           for s in stripes for t in range(bin(write_masks[s]).count("1"))]
    return np.stack(out) if out else np.zeros((0, C), np.uint8)


def encoded_stripes(tech, k, m, stripes, C, seed):
    """filled_stripes with the parity the technique's w = 8 matrix gives."""
    buf = filled_stripes(stripes, k + m, C, seed).copy()
    ref_matmul(buf, list(range(k)), list(range(k, k + m)),
               oracle.matrix(tech, k, m)[k:])
    return buf


def updated_stripes(tech, k, m, stripes, C, enc, write_masks, new_seed):
    """enc (the stripes as encoded) after update_batch(write_masks)."""
    return update_cases.delta_expect(
        tech, k, m, enc, packed_new(stripes, write_masks, C, new_seed),
        [write_masks[s] for s in stripes])


# ---------------------------------------------------------------------------
# chained calls
# ---------------------------------------------------------------------------

CHAIN = dict(tech="cauchy", k=4, m=6, C=65552, S=1024)
CHAIN_ROUNDS = 3
# (technique, constructor keywords, C, S) of the contexts that take only
# encode, decode and crc
CHAIN_FAMILIES = [
    ("cauchy_orig", dict(packetsize=2048), 65536, 256),
    ("jerasure_reed_sol_van_w16", {}, 65552, 256),
]
FAMILY_ERASED = (1, 4)


def chain_seeds(rnd, lane=0):
    """(batch seed, d_new seed) of a round; lane tells two batches apart."""
    return 0xC4A10000 + 256 * lane + rnd, 0x4E3E0000 + 256 * lane + rnd


def chain_decode_masks(rnd, S, n=10, lane=0):
    """Erasure counts {0, 1, 4, 5, 6} interleaved (decode_multi_cases.
    extra_passes_46 with a fully present stripe added)."""
    rng = random.Random(0x4600 + 16 * lane + rnd)
    return [mask_without(n, rng.sample(range(n), (0, 1, 4, 5, 6)[(s + rnd) % 5]))
            for s in range(S)]


def chain_write_masks(rnd, S, k=4, lane=0):
    """0-4 written chunks per stripe."""
    rng = random.Random(0x5700 + 16 * lane + rnd)
    return [update_cases.mask_of(rng.sample(range(k), rng.randrange(0, k + 1)))
            for _ in range(S)]


def chain_sample(S, lane=0):
    """First, last and 30 seeded stripes."""
    rng = random.Random(0x5A00 + lane)
    return sorted([0, S - 1] + rng.sample(range(1, S - 1), 30))


def chain_model(tech, k, m, C, stripes, seeds, write_masks, decode_masks):
    """The sampled stripes through one round. enc: after fill and encode;
    upd: after the update, which is also what the decode restores; poisoned:
    upd with every erased chunk overwritten."""
    enc = encoded_stripes(tech, k, m, stripes, C, seeds[0])
    upd = updated_stripes(tech, k, m, stripes, C, enc, write_masks, seeds[1])
    poisoned = upd.copy()
    for i, s in enumerate(stripes):
        for c in erased_of(k + m, decode_masks[s]):
            poisoned[i, c] = POISON
    return dict(enc=enc, upd=upd, poisoned=poisoned)


# ---------------------------------------------------------------------------
# more decode plans than the cache holds
# ---------------------------------------------------------------------------

LRU = dict(tech="cauchy", k=16, m=4, C=16)


def lru_masks():
    """(16,4): all 6195 patterns of 1..4 erasures, shuffled."""
    n = LRU["k"] + LRU["m"]
    masks = [mask_without(n, er) for e in range(1, LRU["m"] + 1)
             for er in combinations(range(n), e)]
    random.Random(0x164).shuffle(masks)
    return masks


def lru_verify_masks(count=64):
    """Degraded masks for verify_batch: 1-3 chunks absent, so at least one
    chunk is left to check; seeded, distinct."""
    n = LRU["k"] + LRU["m"]
    rng = random.Random(0x165)
    out = []
    while len(out) < count:
        mk = mask_without(n, rng.sample(range(n), rng.randrange(1, 4)))
        if mk not in out:
            out.append(mk)
    return out
