"""References and case tables shared by test_kernel_references.py (CPU: the
references against the oracle, the case tables against geometry(), and
geometry() against the launcher's plan probe) and test_gpu_bitmatrix_kernel.py, test_gpu_bitmatrix_knobs.py and
test_gpu_w16_kernel.py (GPU: bytes). Not a test module. Everything is
seeded; nothing here touches the GPU or the code under test.

The references are plain numpy over the oracle's matrices: ref_bit is the
packet-XOR gather of a bit matrix (the jerasure bitmatrix techniques),
ref16 a GF(2^16) matrix product over u16 little-endian symbols."""
import functools
from itertools import combinations

import numpy as np

import oracle

POISON = 0xA5
W = 8  # packets per superword (the bitmatrix techniques run at w = 8)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------

def ref_bit(buf, src_ids, out_ids, rows, pkt, accum=False):
    """buf: (S, n, C) uint8, updated in place like the device batch. Each
    chunk is a run of superwords of 8 packets of pkt bytes; packet r of
    chunk out_ids[j] = XOR over (i, c) with rows[8*j + r][8*i + c] != 0 of
    packet c of chunk src_ids[i] (on top of its old bytes with accum)."""
    S, n, C = buf.shape
    assert buf.flags.c_contiguous and C % (W * pkt) == 0
    rows = np.asarray(rows)
    assert rows.shape == (W * len(out_ids), W * len(src_ids))
    v = buf.reshape(S, n, C // (W * pkt), W, pkt)
    assert np.shares_memory(v, buf)
    srcs = [v[:, s].copy() for s in src_ids]
    for j, o in enumerate(out_ids):
        for r in range(W):
            acc = (v[:, o, :, r, :].copy() if accum
                   else np.zeros((S, C // (W * pkt), pkt), np.uint8))
            for i in range(len(src_ids)):
                for c in range(W):
                    if rows[W * j + r][W * i + c]:
                        acc ^= srcs[i][:, :, c, :]
            v[:, o, :, r, :] = acc


@functools.lru_cache(maxsize=None)
def gf16_tables():
    """(exp, log) of GF(2^16) from the oracle's gf16_mul: exp[i] = 2^i."""
    exp = np.zeros(65535, np.uint16)
    log = np.zeros(65536, np.int64)
    x = 1
    for i in range(65535):
        exp[i] = x
        log[x] = i
        x = oracle.gf16_mul(x, 2)
    assert x == 1 and len(set(exp.tolist())) == 65535, "2 is not primitive"
    return exp, log


def gf16_mul_vec(c, x):
    """c * x in GF(2^16), c a scalar, x a uint16 array."""
    if c == 0:
        return np.zeros_like(x)
    exp, log = gf16_tables()
    out = exp[(log[x] + log[c]) % 65535]
    out[x == 0] = 0
    return out


def ref16(buf, src_ids, out_ids, rows16, accum=False):
    """buf: (S, n, C) uint8, updated in place: chunk out_ids[j] =
    XOR_i rows16[j][i] * chunk src_ids[i] over u16 little-endian symbols (on
    top of its old bytes with accum)."""
    S, n, C = buf.shape
    assert buf.flags.c_contiguous and C % 2 == 0
    v = buf.view("<u2")
    assert np.shares_memory(v, buf)
    srcs = [v[:, s, :].copy() for s in src_ids]
    for j, o in enumerate(out_ids):
        acc = v[:, o, :].copy() if accum else np.zeros((S, C // 2), np.uint16)
        for i, s in enumerate(srcs):
            acc ^= gf16_mul_vec(int(rows16[j][i]), s)
        v[:, o, :] = acc


def rand_batch(seed, S, n, C):
    return np.random.default_rng(seed).integers(
        0, 256, (S, n, C), dtype=np.uint8)


def encode_rows(tech, k, m):
    """(8m x 8k) bit rows of the technique's coding matrix."""
    return oracle.bitmatrix(np.ascontiguousarray(oracle.matrix(tech, k, m)[k:]))


@functools.lru_cache(maxsize=None)
def encoded_bit(tech, k, m, pkt, n_sw, S):
    """A random batch encoded by ref_bit; shared and read-only."""
    C = n_sw * W * pkt
    seed = ((k * 131 + m) * 8191 + pkt) * 31 + n_sw * 7 + S
    full = rand_batch(seed, S, k + m, C)
    ref_bit(full, list(range(k)), list(range(k, k + m)),
            encode_rows(tech, k, m), pkt)
    full.flags.writeable = False
    return full


@functools.lru_cache(maxsize=None)
def encoded16(k, m, S, C, seed=0):
    full = rand_batch((k * 131 + m) * 8191 + C * 3 + S + seed, S, k + m, C)
    ref16(full, list(range(k)), list(range(k, k + m)),
          oracle.matrix_w16(k, m)[k:])
    full.flags.writeable = False
    return full


def mask_without(n, erased):
    m = (1 << n) - 1
    for e in erased:
        m &= ~(1 << e)
    return m


def patterns(n, max_e):
    """Every erasure pattern of 1..max_e chunks out of n."""
    return [er for e in range(1, max_e + 1)
            for er in combinations(range(n), e)]


# ---------------------------------------------------------------------------
# the bitmatrix launcher's arithmetic, restated independently of its plan
# (ceph_amd/csrc/bit_plan.cpp); test_kernel_references.py holds the two
# against each other through ceph_amd.bitmatrix_plan_probe
# ---------------------------------------------------------------------------

def geometry(n_src, pkt, n_sw, n_out=2, accum=False, bitq=16, wpb=8,
             bitreg=2, pipe=0, xcd=0):
    """What the bitmatrix launcher launches for n_src sources and n_out
    outputs of n_sw superwords at packet size pkt under the given knob
    values (the defaults are the launcher's). Returns a dict."""
    use_reg = (n_out <= 4) if bitreg == 1 else (n_out == 1 and bitreg == 2)
    if use_reg:
        n_pos = n_sw * pkt // 16
        return dict(kernel="reg", nr=8 * n_out, accum=accum, n_pos=n_pos,
                    grid=min((n_pos + 255) // 256, 16384))
    budget = min(max(bitq, 8), 120) * 1024
    q = 16
    while q * 2 <= pkt and pkt % (q * 2) == 0 and n_src * W * q * 2 <= budget:
        q *= 2
    vq_shift = (q // 16).bit_length() - 1
    items = n_src * W * (q // 16)
    wps = pkt // q
    n_windows = n_sw * wps
    grid = (n_windows + wpb - 1) // wpb
    data_bytes = n_src * W * q
    use_pipe = bool(pipe) and wpb > 1 and items % 64 == 0
    # the op list is at most one u16 per set bit: bound it by a full matrix
    lds_bound = (2 if use_pipe else 1) * data_bytes + 2 * (W * n_out) * (
        W * n_src) + 16
    g = dict(kernel="pipe" if use_pipe else "lds", accum=accum, q=q,
             vqs=vq_shift if vq_shift in (3, 4, 5) and not use_pipe else -1,
             staging="dma" if items % 64 == 0 else "reg", items=items,
             wps=wps, n_windows=n_windows, grid=grid,
             last_block=n_windows - (grid - 1) * wpb, lds_bound=lds_bound)
    g["xcdmap"] = bool(xcd) and not use_pipe and wps == 8 and \
        n_windows % (wpb * 64) == 0 and grid % 64 == 0
    return g


# ---------------------------------------------------------------------------
# cases at the default knobs (test_gpu_bitmatrix_kernel.py)
# ---------------------------------------------------------------------------

# (k, pkt, superwords per chunk) -> q, VQS instance, staging, windows per
# superword that the launcher derives at its defaults for n_src = k
LDS_SHAPES = {
    (2, 4096, 1): dict(q=1024, vqs=-1, staging="dma", wps=4),
    (4, 2048, 3): dict(q=512, vqs=5, staging="dma", wps=4),
    (7, 2048, 3): dict(q=256, vqs=4, staging="dma", wps=8),
    (16, 2048, 1): dict(q=128, vqs=3, staging="dma", wps=16),
    (5, 256, 9): dict(q=256, vqs=4, staging="dma", wps=1),
    (4, 32, 3): dict(q=32, vqs=-1, staging="dma", wps=1),
    (8, 16, 1): dict(q=16, vqs=-1, staging="dma", wps=1),
    (3, 48, 5): dict(q=16, vqs=-1, staging="reg", wps=3),
    (3, 96, 2): dict(q=32, vqs=-1, staging="reg", wps=3),
    (5, 16, 3): dict(q=16, vqs=-1, staging="reg", wps=1),
}
# the window walk at its edges: (k, pkt, n_sw) -> windows, blocks, windows
# in the last block
WALK_EDGES = {
    (8, 16, 1): (1, 1, 1),     # the smallest legal chunk, 128 B
    (4, 2048, 3): (12, 2, 4),  # last block half full; a block spans sw 1|2
    (3, 48, 5): (15, 2, 7),    # sw boundaries mid-block, wt % 3
    (7, 2048, 3): (24, 3, 8),  # three full blocks
}
ENCODE_M = (2, 3, 4, 5, 8)   # cauchy_orig; 8 fills row_map / row_off
GOOD_M = (3, 5)              # cauchy_good refuses m = 2 by design
STRIPES = (1, 3)

# the register kernel (n_out = 1 at the defaults): (k, m, pkt, n_sw)
REG_SHAPES = [
    (3, 3, 16, 1),     # one position, one live lane
    (3, 3, 48, 5),     # 15 positions, p / 3
    (3, 3, 2048, 3),   # 384 positions: a partial second block
]


def encode_cases():
    """(tech, k, m, pkt, n_sw) of every default-knob encode."""
    out = [("cauchy_orig", k, m, pkt, n_sw)
           for (k, pkt, n_sw) in LDS_SHAPES for m in ENCODE_M]
    out += [("cauchy_good", k, m, pkt, n_sw)
            for (k, pkt, n_sw) in LDS_SHAPES for m in GOOD_M]
    return out


def shape_decode_patterns(k):
    """Per LDS shape at m = 3: only parities lost, only data lost, a mix of
    three."""
    return [(k, k + 2), (0, k - 1), (0, 1, k + 1)]


DECODE_48 = (5, 8)  # erasure counts of the (4, 8) patterns
PATTERNS_48 = [(0, 2, 5, 7, 10), (0, 1, 2, 3, 4, 6, 9, 11)]
HOST_PATH = dict(k=4, m=9, pkt=48, n_sw=5, erased=(0, 2, 5, 12))


# ---------------------------------------------------------------------------
# cases under the knobs (test_gpu_bitmatrix_knobs.py); every setting's child
# runs all of them
# ---------------------------------------------------------------------------

# (tech, k, m, pkt, n_sw, S)
KNOB_ENCODES = [
    ("cauchy_orig", 7, 3, 2048, 3, 3),
    ("cauchy_orig", 4, 4, 2048, 3, 3),
    ("cauchy_orig", 3, 3, 48, 5, 3),
    ("cauchy_orig", 3, 4, 48, 5, 1),
    ("cauchy_orig", 4, 2, 2048, 3, 1),
    ("cauchy_orig", 7, 5, 2048, 3, 1),
    ("cauchy_good", 4, 3, 2048, 3, 3),
    ("cauchy_orig", 16, 3, 2048, 1, 3),   # ECX_BITQ=8: q = 64, generic
    ("cauchy_orig", 16, 3, 1024, 8, 1),   # ECX_BITXCD: one group of 64
    ("cauchy_orig", 16, 3, 1024, 16, 1),  # ECX_BITXCD: two groups
    ("cauchy_orig", 16, 3, 1024, 3, 1),   # ECX_BITXCD refused by the host
    ("cauchy_orig", 4, 3, 32, 3, 3),      # 64 items: one wave-chunk
    ("cauchy_orig", 8, 3, 16, 1, 3),      # 64 items, one window
    ("cauchy_orig", 5, 3, 16, 3, 3),      # register staging: no pipe
    ("cauchy_orig", 2, 3, 4096, 1, 1),    # q = 1024
    ("cauchy_orig", 5, 3, 256, 9, 1),     # one window per superword
]
# (tech, k, m, pkt, n_sw, S, erased)
KNOB_DECODES = [
    ("cauchy_orig", 7, 3, 2048, 3, 3, (2,)),
    ("cauchy_orig", 7, 3, 2048, 3, 3, (1, 8)),
    ("cauchy_orig", 4, 4, 2048, 3, 3, (5,)),
    ("cauchy_orig", 4, 4, 2048, 3, 3, (0, 3)),
    ("cauchy_orig", 4, 4, 2048, 3, 1, (0, 2, 4, 7)),
    ("cauchy_orig", 3, 3, 48, 5, 3, (0,)),
    ("cauchy_orig", 3, 3, 48, 5, 3, (1, 4)),
    ("cauchy_orig", 3, 3, 48, 5, 1, (0, 2, 5)),
    ("cauchy_orig", 4, 3, 32, 3, 3, (1, 6)),
]
# apply_delta on (3, 3): (pkt, n_sw, data shard, coding shard)
KNOB_DELTAS = [
    (2048, 3, 0, 3), (2048, 3, 2, 5),
    (48, 5, 1, 4), (48, 5, 2, 3),
    (16, 1, 0, 5), (16, 1, 1, 3),
    # under ECX_BITREG=0 the single source gives q = pkt: the accumulating
    # VQS 3, 4 and 5 instances
    (128, 2, 0, 4), (256, 2, 1, 5), (512, 2, 2, 4),
]

KNOBS = [
    {"ECX_BITREG": "0"},
    {"ECX_BITREG": "1"},
    {"ECX_NT": "0"},
    {"ECX_NT": "0", "ECX_BITREG": "0"},
    {"ECX_NT": "0", "ECX_BITREG": "1"},
    {"ECX_BITT": "128"},
    {"ECX_BITT": "64"},
    {"ECX_BITW": "1"},
    {"ECX_BITW": "3"},
    {"ECX_BITQ": "8"},
    {"ECX_BITPIPE": "1"},
    {"ECX_BITPIPE": "1", "ECX_BITW": "3"},
    {"ECX_BITPIPE": "1", "ECX_BITW": "1"},
    {"ECX_BITPIPE": "1", "ECX_BITREG": "0"},
    {"ECX_BITPIPE": "1", "ECX_NT": "0"},
    {"ECX_BITPIPE": "1", "ECX_NT": "0", "ECX_BITREG": "0"},
    {"ECX_BITSTAGGER": "2"},
    {"ECX_BITXCD": "1", "ECX_BITW": "1"},
]


def knob_geometry(knobs, n_src, pkt, n_sw, n_out, accum=False):
    """geometry() of one launch under a KNOBS entry."""
    return geometry(n_src, pkt, n_sw, n_out=n_out, accum=accum,
                    bitq=int(knobs.get("ECX_BITQ", 16)),
                    wpb=int(knobs.get("ECX_BITW", 8)),
                    bitreg=int(knobs.get("ECX_BITREG", 2)),
                    pipe=int(knobs.get("ECX_BITPIPE", 0)),
                    xcd=int(knobs.get("ECX_BITXCD", 0)))


def knob_launches(knobs):
    """geometry of every launch a knob child makes."""
    out = []
    for _, k, m, pkt, n_sw, _ in KNOB_ENCODES:
        out.append(knob_geometry(knobs, k, pkt, n_sw, m))
    for _, k, m, pkt, n_sw, _, er in KNOB_DECODES:
        out.append(knob_geometry(knobs, k, pkt, n_sw, len(er)))
    for pkt, n_sw, _, _ in KNOB_DELTAS:
        out.append(knob_geometry(knobs, 1, pkt, n_sw, 1, accum=True))
    return out


# ---------------------------------------------------------------------------
# w = 16 cases (test_gpu_w16_kernel.py)
# ---------------------------------------------------------------------------

W16 = "jerasure_reed_sol_van_w16"
# one vector; three; one tile; a partial second tile; 769 vectors = four
# tiles on a grid of four; 767 vectors = three tiles on a grid of four (the
# doubling overshoots: one idle block)
W16_SIZES = (16, 48, 4096, 4112, 12304, 12272)
W16_LONG = dict(k=2, m=1, C=8208, S=1024)   # second grid-stride trip
# the only parity row of (2, 1) is all ones and takes no table: the same
# walk with a second, general row
W16_LONG_TABLES = dict(k=2, m=2, C=8208, S=1024)
W16_DELTA_SIZES = (16, 4112)


def w16_grid(C, S):
    """Grid x and grid-stride trips of run_matmul16."""
    vecs = C // 16
    gx = max(1, min((vecs + 511) // 512, 1024))
    tiles = (vecs + 255) // 256
    while gx * S < 2048 and gx < tiles:
        gx *= 2
    return gx, tiles, (vecs + gx * 256 - 1) // (gx * 256)
