"""Mask sets shared by test_decode_multi_plan.py (CPU: grouping, and proof
via the reference that every mask is decodable) and test_gpu_decode_multi.py
(GPU: bytes). Not a test module. Everything is seeded; nothing here touches
the GPU or the code under test."""
import random
from itertools import combinations

MATRIX_TECHS = ["reed_sol_van", "cauchy", "jerasure_reed_sol_van"]


def mask_without(n, erased):
    m = (1 << n) - 1
    for e in erased:
        m &= ~(1 << e)
    return m


def erased_of(n, mask):
    return [c for c in range(n) if not (mask >> c) & 1]


def all_patterns_43():
    """(k,m) = (4,3): all 63 masks with 1-3 erasures plus the full mask,
    shuffled with a fixed seed -> 64 stripes, neighbours differ."""
    n = 7
    masks = [mask_without(n, er) for e in (1, 2, 3)
             for er in combinations(range(n), e)]
    assert len(masks) == 63
    masks.append((1 << n) - 1)
    random.Random(0x43).shuffle(masks)
    return masks


def mid_83(n_stripes=200):
    """(8,3): masks drawn with a fixed seed from 0-3 erasures."""
    rng = random.Random(0x83)
    return [mask_without(11, rng.sample(range(11), rng.randrange(0, 4)))
            for _ in range(n_stripes)]


def extra_passes_46(n_stripes=24):
    """(4,6): erasure counts {1, 4, 5, 6} interleaved — 5 and 6 need a
    second <= 4-output pass."""
    rng = random.Random(0x46)
    return [mask_without(10, rng.sample(range(10), (1, 4, 5, 6)[s % 4]))
            for s in range(n_stripes)]


SLICE_SIZES = (16, 4096, 4112, 65536)
SLICE_NULL = 7          # slice whose data chunk SLICE_NULL_CHUNK is NULL
SLICE_NULL_CHUNK = 0    # (present, true content zeros)


def slices_42(n_slices=40):
    """(4,2): sizes cycling through SLICE_SIZES, random 0-2-erasure masks.
    Slice SLICE_NULL keeps chunk SLICE_NULL_CHUNK present (it is passed as
    a NULL pointer = zeros) and loses two others, so the zeros chunk is a
    survivor the kernel must skip."""
    rng = random.Random(0x42)
    sizes = [SLICE_SIZES[i % len(SLICE_SIZES)] for i in range(n_slices)]
    masks = [mask_without(6, rng.sample(range(6), rng.randrange(0, 3)))
             for _ in range(n_slices)]
    masks[SLICE_NULL] = mask_without(6, [1, 4])
    return sizes, masks


def long_bucket_21(n_stripes=2800):
    """(2,1): one output everywhere, > 2048 stripes in the single bucket —
    the shape at which the launch stops widening grid x, so blocks take
    more than one grid-stride step (with a one-vector tail at C = 8208)."""
    return [mask_without(3, [] if s % 4 == 3 else [s % 4])
            for s in range(n_stripes)]


# (technique, k, m, masks) of every mask the GPU file decodes
def gpu_mask_sets():
    sets = [(t, 4, 3, all_patterns_43()) for t in MATRIX_TECHS]
    sets.append(("reed_sol_van", 8, 3, mid_83()))
    sets.append(("cauchy", 4, 6, extra_passes_46()))
    sets.append(("reed_sol_van", 4, 2, slices_42()[1]))
    sets.append(("reed_sol_van", 2, 1, long_bucket_21()))
    return sets
