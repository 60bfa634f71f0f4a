"""The reference of the ecx_locate_* tests, shared by the CPU and the GPU
file. It uses the oracle only; the library's rows never enter an expectation.

Definition under test: bit x of a stripe's culprit word is set exactly when x
is present and the consistency check of the mask without x reports 0.
culprits() below is that sentence, with expected_word() — restated from
tests/test_gpu_verify.py — as the consistency check: an oracle.decode rebuild
from the first k present chunks, compared with what is stored."""
import numpy as np

import oracle

TECH = "reed_sol_van"


def full(k, m):
    return (1 << (k + m)) - 1


def expected_word(tech, k, m, stripe, mask):
    """stripe: k+m uint8 arrays as stored. Bit i is set exactly when i is in
    the mask, is not a survivor, and differs from its rebuild out of the
    survivors alone."""
    n = k + m
    present = [i for i in range(n) if mask >> i & 1]
    surv = present[:k]
    chunks = [np.ascontiguousarray(c).copy() for c in stripe]
    oracle.decode(tech, k, m, chunks, [int(i in surv) for i in range(n)])
    word = 0
    for i in present[k:]:
        if not np.array_equal(chunks[i], stripe[i]):
            word |= 1 << i
    return word


def culprits(tech, k, m, stripe, mask):
    """OR of 1 << x over the present x without which the rest agrees."""
    word = 0
    for x in range(k + m):
        if mask >> x & 1 and \
                expected_word(tech, k, m, stripe, mask & ~(1 << x)) == 0:
            word |= 1 << x
    return word


def expected(tech, k, m, host, mask):
    """host: (S, k+m, C). (bad, culprit) of every stripe, none skipped."""
    S = host.shape[0]
    bad = np.zeros(S, dtype=np.uint64)
    cul = np.zeros(S, dtype=np.uint64)
    for s in range(S):
        stripe = list(host[s])
        bad[s] = expected_word(tech, k, m, stripe, mask)
        cul[s] = culprits(tech, k, m, stripe, mask)
    return bad, cul


def encoded_batch(tech, k, m, S, C, seed):
    """A consistent (S, k+m, C) batch, encoded by the oracle."""
    host = np.random.default_rng(seed).integers(
        0, 256, (S, k + m, C), dtype=np.uint8)
    flat = host.reshape(-1)
    oracle.cpu_encode_batch(tech, k, m, flat, S, C)
    return flat.reshape(S, k + m, C)


def many_flagged_case(S):
    """(8,3), C = 4112 (two tiles per chunk). Stripe s is changed in chunk
    s mod 11 at offset 4100 (the tail tile); every 7th stripe is left clean;
    every 13th is also changed in chunk (s+3) mod 11 at offset 5 (the other
    tile, another byte column: not locatable)."""
    k, m, C = 8, 3, 4112
    host = encoded_batch(TECH, k, m, S, C, seed=0x83)
    for s in range(S):
        if s % 7 == 0:
            continue
        host[s, s % 11, 4100] ^= 1 + s % 255
        if s % 13 == 0:
            host[s, (s + 3) % 11, 5] ^= 0x40
    return host


_MANY = {}


def many_flagged(S):
    """many_flagged_case(S) with its reference, computed once per process
    and read-only."""
    if S not in _MANY:
        host = many_flagged_case(S)
        bad, cul = expected(TECH, 8, 3, host, full(8, 3))
        for a in (host, bad, cul):
            a.setflags(write=False)
        _MANY[S] = (host, bad, cul)
    return _MANY[S]
