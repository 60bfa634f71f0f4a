"""Inputs and host model of the slice-call tests: test_slices_cases.py (CPU:
the cases are what they claim to be, and can tell a wrong kernel from a right
one) and test_gpu_slices.py / test_gpu_table_knobs.py (GPU: bytes). Not a
test module. Everything is seeded; nothing here touches the GPU or the code
under test — the reference is the numpy GF(2^8) matmul of
test_gpu_stream_kernel.py over the oracle's matrices.

An Arena is one flat byte range in which every chunk of every slice sits at
an offset of its own, in shuffled order, with a poison guard band before each
chunk and at the end. Every GPU comparison is the whole arena against the
model's, so bytes between chunks, sources and outputs are all covered."""
import functools
import random
from itertools import combinations

import numpy as np

import oracle
import test_gpu_stream_kernel as t

POISON = 0xA5
THREADS = 256   # lanes of a block: one sweep = THREADS vectors
VPB = 1024      # vectors per block (ecx_slice_plan_probe reports it)
MULTI_OUT = 4   # outputs per launch / pass
MATRIX_TECHS = ["reed_sol_van", "cauchy", "jerasure_reed_sol_van"]


def edge_sizes(vpb=VPB, threads=THREADS):
    """One vector; one short of, exactly, one past a thread sweep; the same
    around a block; a second block that is itself one past a sweep; a third
    block of one vector."""
    T, B = threads * 16, vpb * 16
    return [16, T - 16, T, T + 16, B - 16, B, B + 16, B + T + 16, 2 * B + 16]


EDGE_SIZES = edge_sizes()
SMALL_SIZES = [16, 4112, 16400]  # one vector, past a sweep, past a block


def mask_without(n, erased):
    m = (1 << n) - 1
    for e in erased:
        m &= ~(1 << e)
    return m


def erased_of(n, mask):
    return [c for c in range(n) if not (mask >> c) & 1]


class Arena:
    """cps chunks for each of len(sizes) slices, scattered over one byte
    range. null: (slice, chunk) pairs that get no bytes at all (a NULL
    pointer). share: {(slice, chunk): (slice0, chunk0)} — the chunk is the
    same memory as the other one (its slice must not be longer)."""

    def __init__(self, cps, sizes, seed, null=(), share=None):
        self.cps, self.sizes, self.n = cps, list(sizes), len(sizes)
        self.null = set(null)
        share = dict(share or {})
        rng = np.random.default_rng(seed)
        own = [(s, c) for s in range(self.n) for c in range(cps)
               if (s, c) not in self.null and (s, c) not in share]
        self.off, self.guards, pos = {}, [], 0
        for i, j in enumerate(rng.permutation(len(own))):
            s, c = own[j]
            g = 16 * (1 + i % 5)
            self.guards.append((pos, g))
            pos += g
            self.off[(s, c)] = pos
            pos += self.sizes[s]
        g = 16 * (1 + len(own) % 5)
        self.guards.append((pos, g))
        self.nbytes = pos + g
        self.own = own
        for (s, c), (s0, c0) in share.items():
            assert self.sizes[s] <= self.sizes[s0]
            self.off[(s, c)] = self.off[(s0, c0)]
        self.image = rng.integers(0, 256, self.nbytes, dtype=np.uint8)
        for p, g in self.guards:
            self.image[p:p + g] = POISON

    def offset(self, s, c):
        return self.off.get((s, c))  # None for a NULL chunk

    def flat_offsets(self):
        return [self.offset(s, c) for s in range(self.n)
                for c in range(self.cps)]

    def ptrs(self, base):
        return [None if o is None else base + o for o in self.flat_offsets()]

    def chunk(self, buf, s, c):
        """View of chunk c of slice s in buf (zeros for a NULL chunk)."""
        o = self.offset(s, c)
        if o is None:
            return np.zeros(self.sizes[s], dtype=np.uint8)
        return buf[o:o + self.sizes[s]]

    def poison(self, buf, s, c):
        o = self.offset(s, c)
        buf[o:o + self.sizes[s]] = POISON


# ---- the host model ----

def encode_want(arena, k, rows, image=None):
    """image with chunks k.. of every slice replaced by rows x (chunks 0..k-1)
    — the plain reference, slice by slice."""
    want = (arena.image if image is None else image).copy()
    cps = arena.cps
    for s, sz in enumerate(arena.sizes):
        buf = np.zeros((1, cps, sz), dtype=np.uint8)
        for c in range(k):
            buf[0, c] = arena.chunk(want, s, c)
        t.ref_matmul(buf, list(range(k)), list(range(k, cps)), rows)
        for c in range(k, cps):
            arena.chunk(want, s, c)[:] = buf[0, c]
    return want


def encode_image(arena, k):
    """What goes to the device before an encode: outputs pre-poisoned."""
    img = arena.image.copy()
    for s in range(arena.n):
        for c in range(k, arena.cps):
            arena.poison(img, s, c)
    return img


def erase(arena, truth, masks):
    """What goes to the device before a decode: the reference-encoded arena
    with the chunks missing from each slice's mask poisoned."""
    img = truth.copy()
    for s, mk in enumerate(masks):
        for c in erased_of(arena.cps, mk):
            arena.poison(img, s, c)
    return img


# ---- a block-level restatement of what the kernels do, able to err ----

MISTAKES = ("stride_k", "next_vecs", "past_vend", "prev_rec", "null_poison",
            "cls0_as_1")


def uniform_blocks(sizes, n_recs=1, vpb=VPB):
    """Block list of a uniform call: every slice once in id order, the whole
    list once per <= 4-output launch (record index = launch)."""
    one = [(s, v) for s, sz in enumerate(sizes)
           for v in range(0, sz // 16, vpb)]
    return [(s, v, r) for r in range(n_recs) for s, v in one]


def split_recs(src_ids, out_ids, rows):
    """One (src_ids, out_ids, rows) record per <= 4 outputs."""
    return [(list(src_ids), list(out_ids[j:j + MULTI_OUT]),
             [list(r) for r in rows[j:j + MULTI_OUT]])
            for j in range(0, len(out_ids), MULTI_OUT)]


def multi_plan(n, masks):
    """The grouping of decode_slices_multi restated: distinct masks in
    first-appearance order are the plans; launch (pass, n_out) lists, in
    ascending order, the slices whose pass has n_out outputs; launches are
    ordered by (pass, n_out). Returns (plan_of, n_pass, launches) with
    launches = [(pass, n_out, members)]."""
    plans, plan_of = {}, []
    for mk in masks:
        mk &= (1 << n) - 1
        if not erased_of(n, mk):
            plan_of.append(-1)
            continue
        plan_of.append(plans.setdefault(mk, len(plans)))
    bucket = {}
    for s, mk in enumerate(masks):
        e = len(erased_of(n, mk))
        for p in range(-(-e // MULTI_OUT)):
            bucket.setdefault((p, min(MULTI_OUT, e - p * MULTI_OUT)),
                              []).append(s)
    n_pass = max((p for p, _ in bucket), default=-1) + 1
    return plan_of, n_pass, [(p, o, bucket[(p, o)]) for p, o in sorted(bucket)]


def multi_order(n, masks):
    """(order, recs) as decode_slices_multi hands them to the table fill."""
    plan_of, n_pass, launches = multi_plan(n, masks)
    order = [s for _, _, mem in launches for s in mem]
    recs = [plan_of[s] * n_pass + p for p, _, mem in launches for s in mem]
    return order, recs


def multi_blocks(n, sizes, masks, vpb=VPB):
    order, recs = multi_order(n, masks)
    return [(s, v, r) for s, r in zip(order, recs)
            for v in range(0, sizes[s] // 16, vpb)]


def multi_recs(n, masks, rows_of):
    """Record table [plan * n_pass + pass]; rows_of(mask) -> (survivors,
    erased, rows). Passes a plan does not have stay None."""
    plan_of, n_pass, _ = multi_plan(n, masks)
    n_plans = max(plan_of, default=-1) + 1
    recs = [None] * (n_plans * n_pass)
    for s, pl in enumerate(plan_of):
        if pl < 0 or recs[pl * n_pass] is not None:
            continue
        sv, er, rows = rows_of(masks[s] & ((1 << n) - 1))
        for p, rec in enumerate(split_recs(sv, er, rows)):
            recs[pl * n_pass + p] = rec
    return recs


def simulate(arena, image, blocks, recs, mistake=None, k=None, vpb=VPB):
    """Run the block list over image the way the kernels do: block (slice,
    voff, rec) handles vectors [voff, min(voff + vpb, slice_vecs[slice])) of
    the slice, out = XOR_i rows[j][i] * src_i, a NULL source skipped, a NULL
    output never stored. mistake names one deliberate error (MISTAKES); None
    is the correct kernel. The result is len(image) + 64 KiB long: what a
    wrong kernel writes past the arena lands in the tail (poison before)."""
    assert mistake is None or mistake in MISTAKES
    mul = t.mul_table()
    cps, n = arena.cps, arena.n
    pad = 65536
    buf = np.concatenate([image, np.full(pad, POISON, dtype=np.uint8)])
    flat = arena.flat_offsets()
    vecs = [sz // 16 for sz in arena.sizes]
    stride = k if mistake == "stride_k" else cps
    for b, (sl, v0, r) in enumerate(blocks):
        if mistake == "prev_rec" and b > 0:
            r = blocks[b - 1][2]
        nv = vecs[min(sl + 1, n - 1)] if mistake == "next_vecs" else vecs[sl]
        vend = min(v0 + vpb, nv) + (mistake == "past_vend")
        if vend <= v0:
            continue
        lo, ln = v0 * 16, (vend - v0) * 16
        ptrs = flat[sl * stride:sl * stride + cps]
        src_ids, out_ids, rows = recs[r]
        acc = [np.zeros(ln, dtype=np.uint8) for _ in out_ids]
        for i, sid in enumerate(src_ids):
            if ptrs[sid] is None:
                if mistake != "null_poison":
                    continue
                x = np.full(ln, POISON, dtype=np.uint8)
            else:
                x = buf[ptrs[sid] + lo:ptrs[sid] + lo + ln]
            for j in range(len(out_ids)):
                c = int(rows[j][i])
                if c == 0 and mistake == "cls0_as_1":
                    c = 1
                if c:
                    acc[j] ^= mul[c][x]
        for j, oid in enumerate(out_ids):
            if ptrs[oid] is not None:
                buf[ptrs[oid] + lo:ptrs[oid] + lo + ln] = acc[j]
    return buf


def padded(want):
    return np.concatenate([want, np.full(65536, POISON, dtype=np.uint8)])


# ---- case lists ----

# (k, m, technique): every output count of a launch, and the two-launch path
ENCODE_CODES = [(3, 1, "reed_sol_van"),
                (4, 2, "reed_sol_van"), (4, 2, "cauchy"),
                (4, 2, "jerasure_reed_sol_van"),
                (5, 3, "jerasure_reed_sol_van"),
                (5, 4, "reed_sol_van"),
                (4, 5, "cauchy"), (4, 6, "cauchy"), (3, 8, "cauchy")]


def coding_rows(tech, k, m):
    return np.asarray(oracle.matrix(tech, k, m))[k:]


@functools.lru_cache(maxsize=None)
def encode_case(k, m, tech):
    """All of EDGE_SIZES in one call, scattered."""
    arena = Arena(k + m, EDGE_SIZES, seed=0x5100 + 16 * k + m)
    return arena, encode_want(arena, k, coding_rows(tech, k, m))


# (4,3) rows holding zeros, ones, a zero column inside one row, and one
# all-zero row whose output must come back zeros, not poison
CLASS_ROWS = np.array([[1, 0, 0x8E, 1],
                       [0, 0, 0, 0],
                       [0xC3, 1, 0, 2]], dtype=np.uint8)
CLASS_ZERO_ROW = 1


def class_case(rows, seed=0x5C00):
    """(4,3) under custom coding rows (CLASS_ROWS, or the caller's
    ecx_shec_matrix(4, 3, 2)) over SMALL_SIZES."""
    arena = Arena(7, SMALL_SIZES, seed=seed)
    return arena, encode_want(arena, 4, rows)


# (4,2): NULL sets differ slice by slice — each data position NULL somewhere,
# one slice with every data chunk NULL (parity zeros), one with none
NULL_SIZES = [16, 4112, 16400, 4080, 20496, 4096, 32784]
NULL_SETS = [{0}, {1}, {2}, {3}, {0, 1, 2, 3}, set(), {1, 3}]
NULL_ALL, NULL_NONE = 4, 5


@functools.lru_cache(maxsize=None)
def null_case():
    null = [(s, c) for s, cs in enumerate(NULL_SETS) for c in cs]
    arena = Arena(6, NULL_SIZES, seed=0x5200, null=null)
    return arena, encode_want(arena, 4, coding_rows("reed_sol_van", 4, 2))


# two slices of different sizes over the same k data pointers
SHARED_SIZES = [16400, 4112]


@functools.lru_cache(maxsize=None)
def shared_case():
    arena = Arena(6, SHARED_SIZES, seed=0x5300,
                  share={(1, c): (0, c) for c in range(4)})
    return arena, encode_want(arena, 4, coding_rows("reed_sol_van", 4, 2))


def truth_case(k, m, tech, sizes, seed, null=()):
    """A reference-encoded arena to decode: (arena, truth)."""
    arena = Arena(k + m, sizes, seed=seed, null=null)
    return arena, encode_want(arena, k, coding_rows(tech, k, m))


# decode_slices (4,2) reed_sol_van: every 1- and 2-erasure mask, one call each
DECODE_42_MASKS = [mask_without(6, er) for e in (1, 2)
                   for er in combinations(range(6), e)]


@functools.lru_cache(maxsize=None)
def decode_42_case():
    return truth_case(4, 2, "reed_sol_van", SMALL_SIZES, 0x5400)


# decode_slices (4,6) cauchy: 5 and 6 chunks lost (a second launch of 1 and
# of 2 outputs), data and parity mixed, all of EDGE_SIZES
DECODE_46_MASKS = [mask_without(10, er) for er in
                   ([0, 2, 5, 7, 9], [1, 3, 4, 6, 8, 9], [0, 1, 2, 3, 4, 5],
                    [3, 5, 6, 7, 8, 9], [0, 1, 2, 3, 9])]


@functools.lru_cache(maxsize=None)
def decode_46_case():
    return truth_case(4, 6, "cauchy", EDGE_SIZES, 0x5500)


# decode_slices (4,2): a present survivor passed as NULL (true content zeros)
# in some slices only; chunk 0 in two slices, chunk 3 in another
DECODE_NULL_SIZES = [16, 4112, 16400, 20496, 4096]
DECODE_NULL = [(0, 0), (2, 0), (3, 3)]
DECODE_NULL_MASK = mask_without(6, [1, 4])


@functools.lru_cache(maxsize=None)
def decode_null_case():
    return truth_case(4, 2, "reed_sol_van", DECODE_NULL_SIZES, 0x5600,
                      null=tuple(DECODE_NULL))


# decode_slices_multi (4,6) cauchy: sizes cycle through EDGE_SIZES, erasure
# counts {0, 1, 4, 5, 6} interleaved (9 and 5 are coprime: every size meets
# every count within 45 slices), NULL survivors at three chunk ids
MULTI_N = 48
MULTI_COUNTS = (0, 1, 4, 5, 6)
MULTI_NULL = [(7, 0), (33, 2), (24, 3)]  # counts 4, 5, 6; sizes > one block


def multi_sizes():
    return [EDGE_SIZES[s % len(EDGE_SIZES)] for s in range(MULTI_N)]


def multi_masks():
    rng = random.Random(0x46A)
    keep = dict(MULTI_NULL)
    masks = []
    for s in range(MULTI_N):
        ids = [c for c in range(10) if c != keep.get(s)]
        masks.append(mask_without(10, rng.sample(ids, MULTI_COUNTS[s % 5])))
    return masks


@functools.lru_cache(maxsize=None)
def multi_case():
    arena, truth = truth_case(4, 6, "cauchy", multi_sizes(), 0x5700,
                              null=tuple(MULTI_NULL))
    return arena, truth, multi_masks()


# the ECX_NT=0 child: the same shapes at three sizes only
@functools.lru_cache(maxsize=None)
def knob_decode_case():
    arena, truth = truth_case(4, 6, "cauchy", SMALL_SIZES, 0x5800,
                              null=((1, 2),))
    return arena, truth, mask_without(10, [0, 3, 5, 6, 9])


KNOB_MULTI_N = 15


@functools.lru_cache(maxsize=None)
def knob_multi_case():
    rng = random.Random(0x46B)
    sizes = [SMALL_SIZES[s % 3] for s in range(KNOB_MULTI_N)]
    null = ((8, 1),)  # count 5, 16400 B
    masks = [mask_without(10, rng.sample(
        [c for c in range(10) if (s, c) not in null], MULTI_COUNTS[s % 5]))
        for s in range(KNOB_MULTI_N)]
    arena, truth = truth_case(4, 6, "cauchy", sizes, 0x5900, null=null)
    return arena, truth, masks


# job blob growth: three calls on one slot with no sync between; the second
# table is far more than 1.5x + 4096 B larger than the first
def growth_sizes():
    rng = random.Random(0x6A0)
    return ([[16, 4080, 4112, 48][i % 4] for i in range(64)],
            [16 * rng.randrange(1, 5) for _ in range(6000)],
            [EDGE_SIZES[-1]] * 8)


@functools.lru_cache(maxsize=None)
def growth_cases():
    rows = coding_rows("reed_sol_van", 4, 2)
    out = []
    for i, sizes in enumerate(growth_sizes()):
        arena = Arena(6, sizes, seed=0x5A00 + i)
        out.append((arena, encode_want(arena, 4, rows)))
    return out


# two slots, (4,2): an arena and a mask list each
SLOT_SIZES = ([16, 4112, 16400, 32784], [20496, 4080, 16, 16384])
SLOT_MASKS = ([mask_without(6, er) for er in ([0], [2, 5], [], [1, 3])],
              [mask_without(6, er) for er in ([4, 5], [3], [0, 1], [])])


@functools.lru_cache(maxsize=None)
def slot_cases():
    return [truth_case(4, 2, "reed_sol_van", SLOT_SIZES[i], 0x5B00 + i)
            for i in range(2)]
