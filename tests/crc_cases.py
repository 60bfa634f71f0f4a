"""The CRC-32C reference of the ecx_crc32c_* tests: pure numpy and Python
ints, built from the polynomial alone, independent of the library.

f(seed, data) is ceph_crc32c: Castagnoli, reflected (0x82F63B78), no
inversion of the seed or of the result. crc_shift(crc, n) is the state after
n zero bytes, crc * x^(8n) mod P (bit 31 of a word is x^0), so
f(seed, A + B) == crc_shift(f(seed, A), len(B)) ^ f(0, B).

Large buffers are cut into 4 KiB rows, the rows hashed side by side (one
numpy step per byte column) and combined with crc_shift, so a 1 MiB chunk
costs 4096 numpy steps, not a million."""
import numpy as np

POLY = 0x82F63B78
ROW = 4096


def _table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = (t >> 1) ^ np.where(t & 1, np.uint32(POLY), np.uint32(0))
    return t


TABLE = _table()


def crc_rows(seeds, rows):
    """rows: (R, n) uint8, seeds: (R,) or scalar. One CRC per row."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    crc = np.broadcast_to(np.asarray(seeds, dtype=np.uint32),
                          rows.shape[:1]).copy()
    for j in range(rows.shape[1]):
        crc = (crc >> 8) ^ TABLE[(crc ^ rows[:, j]) & 0xFF]
    return crc


def _mul(a, b):
    """a * b mod P on Python ints."""
    r = 0
    for i in range(32):
        if b >> (31 - i) & 1:
            r ^= a
        a = (a >> 1) ^ (POLY if a & 1 else 0)
    return r


def _xpow8(nbytes):
    r, b = 1 << 31, 1 << 23  # 1, x^8
    while nbytes:
        if nbytes & 1:
            r = _mul(r, b)
        b = _mul(b, b)
        nbytes >>= 1
    return r


def crc_shift(crc, nbytes):
    return _mul(int(crc), _xpow8(int(nbytes)))


def _mul_vec(a, const):
    """Every word of uint32 array a times the Python-int constant."""
    a = a.astype(np.uint32).copy()
    r = np.zeros_like(a)
    for i in range(32):
        if const >> (31 - i) & 1:
            r ^= a
        a = (a >> 1) ^ np.where(a & 1, np.uint32(POLY), np.uint32(0))
    return r


def crc_many(seeds, chunks):
    """chunks: (N, C) uint8; seeds: (N,) or scalar. f(seed_i, chunk_i) as a
    (N,) uint32 array."""
    chunks = np.ascontiguousarray(chunks, dtype=np.uint8)
    n, c = chunks.shape
    crc = np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (n,)).copy()
    head = c % ROW
    if head:  # the short piece goes first: the rest is whole rows
        crc = crc_rows(crc, chunks[:, :head])
    r = (c - head) // ROW
    if r:
        parts = crc_rows(0, chunks[:, head:].reshape(n * r, ROW)).reshape(n, r)
        x_row = _xpow8(ROW)
        for j in range(r):  # Horner over the rows, vectorised over chunks
            crc = _mul_vec(crc, x_row) ^ parts[:, j]
    return crc


def crc(seed, data):
    """f(seed, data) of one buffer, as a Python int."""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(
        data, np.ndarray) else data.reshape(-1)
    return int(crc_many(seed, a.reshape(1, -1))[0])


def batch_ref(host, seeds=0xFFFFFFFF):
    """host: (S, n, C). (S, n) words, every chunk on its own."""
    s, n, c = host.shape
    sd = np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (s, n))
    return crc_many(sd.reshape(-1), host.reshape(s * n, c)).reshape(s, n)


def chain_ref(host, seeds=0xFFFFFFFF):
    """host: (S, n, C); seeds (n,) or scalar. Row s = the hash of each
    shard's chunks of stripes 0..s concatenated."""
    s, n, c = host.shape
    own = batch_ref(host, 0)
    x_c = _xpow8(c)
    run = np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (n,)).copy()
    out = np.zeros((s, n), dtype=np.uint32)
    for i in range(s):
        run = _mul_vec(run, x_c) ^ own[i]
        out[i] = run
    return out


def borders(plan, c):
    """Offsets in a chunk of c bytes where a lane segment or a block of the
    plan begins, other than 0: both are aligned to the END of the chunk."""
    seg = plan["seg_bytes"]
    return [c - j * seg for j in range(1, (c + seg - 1) // seg) if c - j * seg > 0]


def block_borders(plan, c):
    blk = plan["seg_bytes"] * plan["segs_per_block"]
    return [c - j * blk for j in range(1, (c + blk - 1) // blk) if c - j * blk > 0]
