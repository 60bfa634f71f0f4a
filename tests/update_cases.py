"""Write-mask sets shared by test_update_plan.py (CPU: the host-side plan,
and proof via the reference that correcting parity by delta equals
re-encoding) and test_gpu_update_batch.py (GPU: bytes). Not a test module.
Everything is seeded; nothing here touches the GPU or the code under test."""
import random

import numpy as np

MATRIX_TECHS = ["reed_sol_van", "cauchy", "jerasure_reed_sol_van"]


def mask_of(chunks):
    m = 0
    for c in chunks:
        m |= 1 << c
    return m


def written_of(k, mask):
    return [c for c in range(k) if (mask >> c) & 1]


def all_masks_43():
    """(k,m) = (4,3): all 15 nonzero write masks plus mask 0, each four
    times, shuffled with a fixed seed -> 64 stripes, neighbours differ;
    includes c = k (every data chunk rewritten)."""
    masks = list(range(16)) * 4
    random.Random(0x43).shuffle(masks)
    return masks


def mid_83(n_stripes=200):
    """(8,3): masks of 0-3 chunks drawn with a fixed seed."""
    rng = random.Random(0x83)
    return [mask_of(rng.sample(range(8), rng.randrange(0, 4)))
            for _ in range(n_stripes)]


def two_passes_46(n_stripes=24):
    """(4,6): c cycling through 1..4 — six parities need a second
    <= 4-output pass over the same old data."""
    rng = random.Random(0x46)
    return [mask_of(rng.sample(range(4), 1 + s % 4))
            for s in range(n_stripes)]


def long_list_21(n_stripes=2800):
    """(2,1): three stripes in four active, > 2048 in the launch — the shape
    at which the launch stops widening grid x, so blocks take more than one
    grid-stride step (with a one-vector tail at C = 8208)."""
    return [0 if s % 4 == 3 else 1 + s % 3 for s in range(n_stripes)]


def smallest_42(n_stripes=8):
    """(4,2): 8 stripes for the single-vector chunk, one untouched."""
    rng = random.Random(0x42)
    masks = [mask_of(rng.sample(range(4), rng.randrange(1, 4)))
             for _ in range(n_stripes)]
    masks[5] = 0
    return masks


def total_new(masks):
    return sum(bin(mk).count("1") for mk in masks)


def delta_expect(tech, k, m, old, new, masks):
    """The expectation of both test files, from the oracle alone. old is a
    batch (S, k+m, C), new the packed new chunks (total_new, C), stripe
    ascending then chunk id ascending. Returns the batch after the write:
    P_r ^= G[k+r][j] * (old_j ^ new_j) through oracle.region_mul_xor with
    coefficients from oracle.matrix, written chunks replaced, everything
    else as it was."""
    import oracle
    gen = oracle.matrix(tech, k, m)
    out = old.copy()
    at = 0
    for s, mk in enumerate(masks):
        for j in written_of(k, mk):
            delta = oracle.xor_region(np.ascontiguousarray(old[s, j]),
                                      np.ascontiguousarray(new[at]))
            for r in range(m):
                oracle.region_mul_xor(int(gen[k + r, j]), delta, out[s, k + r])
            out[s, j] = new[at]
            at += 1
    assert at == len(new)
    return out


# (technique, k, m, masks) of every mask set the GPU file writes
def gpu_mask_sets():
    sets = [(t, 4, 3, all_masks_43()) for t in MATRIX_TECHS]
    sets.append(("reed_sol_van", 8, 3, mid_83()))
    sets.append(("cauchy", 4, 6, two_passes_46()))
    sets.append(("reed_sol_van", 2, 1, long_list_21()))
    sets.append(("reed_sol_van", 4, 2, smallest_42()))
    sets.append(("reed_sol_van", 4, 3, [0] * 64))
    return sets
