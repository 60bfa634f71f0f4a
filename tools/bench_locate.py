#!/usr/bin/env python3
"""What does it cost to also ask WHICH chunk of an inconsistent stripe is
wrong? (locate_batch vs verify_batch)

reed_sol_van RS(8,3), 1 MiB chunks, S = 1024, device-resident stripes filled
with fill_random and encoded on the device. The cases are alternated within
one process, each timed with a host clock around call + sync() and with the
call's own device events (last_kernel_ms, first launch to last):

  A   verify_batch, full mask, clean batch: the comparison point
  B   locate_batch on the same buffer: what a scrub pays on the batches it
      almost always sees. B - A = two memsets instead of one, the list
      kernel, k near-empty candidate launches and the finish kernel
  C   locate_batch, one byte changed in 1 % of the stripes. It runs on A's
      own buffer (the bytes are changed before each timed call and put back
      after it, outside the timed window), because the same kernel on
      another allocation of the same size differs by more than the work
      added (profiles/verify_summary.md)
  D   locate_batch, chunk 0 of every stripe overwritten with random bytes:
      every stripe flagged, every candidate reads the whole batch; the
      recorded worst case

Before timing, the words are checked: B bad 0 and culprit the full mask; C
flagged exactly on the changed stripes, each with the changed chunk as its
only culprit; D every stripe flagged with culprit chunk 0; and one changed
stripe of C against the CPU oracle (the reference of tests/locate_cases.py).
Not wired into bench.py; prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import ceph_amd  # noqa: E402

K, M, TECH = 8, 3, "reed_sol_van"
N = K + M
FULL = (1 << N) - 1


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4),
            "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4),
            "reps": len(ms)}


def oracle_words(oracle, ctx, d, s, C):
    """Stripe s of batch d under the full mask: (bad, culprit) from oracle
    rebuilds alone."""
    stored = np.empty((N, C), dtype=np.uint8)
    ctx.download(stored, ctypes.c_void_p(d.value + s * N * C))

    def word(mask):
        present = [i for i in range(N) if mask >> i & 1]
        chunks = [stored[i].copy() for i in range(N)]
        oracle.decode(TECH, K, M, chunks,
                      [int(i in present[:K]) for i in range(N)])
        return sum(1 << i for i in present[K:]
                   if not np.array_equal(chunks[i], stored[i]))

    return word(FULL), sum(1 << x for x in range(N)
                           if word(FULL & ~(1 << x)) == 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "bench_locate.json"))
    A = ap.parse_args()
    S, C = A.stripes, A.chunk
    if A.reps < 20:
        ap.error("--reps must be >= 20")
    if S < 100 or S > 65535 or C % 16:
        ap.error("--stripes must be 100..65535 and --chunk a multiple of 16")

    if ceph_amd.device_count() < 1:
        raise SystemExit("bench_locate: no GPU visible — this tool measures "
                         "on the device and has no fallback")
    import oracle  # the checker, never the measured path

    rng = random.Random(0xEC)
    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    total = S * N * C
    # two copies of one encoded batch: clean (A, B, C), chunk 0 random (D)
    bufs = {}
    for name in ("clean", "D"):
        bufs[name] = ctx.dbuf_alloc(total)
        ctx.fill_random(bufs[name], total, 0xEC)
        ctx.encode_batch(bufs[name], S, C)
    ctx.sync()
    # case C: one byte in each of 1 % of the stripes, anywhere in the stripe
    changed = sorted(rng.sample(range(S), max(1, S // 100)))
    flips, chunk_of = [], {}
    for s in changed:
        chunk_of[s] = rng.randrange(N)
        at = ctypes.c_void_p(bufs["clean"].value
                             + (s * N + chunk_of[s]) * C + rng.randrange(C))
        orig = np.zeros(1, dtype=np.uint8)
        ctx.download(orig, at)
        flips.append((at, orig, orig ^ np.uint8(1 << rng.randrange(8))))

    def damage():
        for at, _, bad in flips:
            ctx.upload(at, bad)

    def repair():
        for at, orig, _ in flips:
            ctx.upload(at, orig)

    for s in range(S):
        ctx.fill_random(ctypes.c_void_p(bufs["D"].value + s * N * C), C,
                        0xE000 + s)
    ctx.sync()
    d_bad = ctx.dbuf_alloc(8 * S)
    d_cul = ctx.dbuf_alloc(8 * S)

    def loc(buf):
        return lambda: ctx.locate_batch(bufs[buf], S, C, FULL, d_bad, d_cul)

    # ---- the words, before anything is timed ----
    if ctx.verify_batch(bufs["clean"], S, C, FULL, d_bad).any():
        raise SystemExit("bench_locate: case A: a clean batch was flagged")
    bad, cul = loc("clean")()
    if bad.any() or (cul != FULL).any():
        raise SystemExit("bench_locate: case B: a clean batch was flagged")
    damage()
    bad, cul = loc("clean")()
    if sorted(np.flatnonzero(bad)) != changed:
        raise SystemExit("bench_locate: case C flags other stripes than the "
                         "changed ones")
    for s in range(S):
        want = 1 << chunk_of[s] if s in chunk_of else FULL
        if int(cul[s]) != want:
            raise SystemExit(f"bench_locate: case C stripe {s}: culprit "
                             f"{int(cul[s]):#x}, expected {want:#x}")
    s = changed[len(changed) // 2]
    want = oracle_words(oracle, ctx, bufs["clean"], s, C)
    if (int(bad[s]), int(cul[s])) != want:
        raise SystemExit(f"bench_locate: case C stripe {s}: words "
                         f"{int(bad[s]):#x} {int(cul[s]):#x}, oracle {want}")
    repair()
    if ctx.verify_batch(bufs["clean"], S, C, FULL, d_bad).any():
        raise SystemExit("bench_locate: the changed bytes were not put back")
    bad, cul = loc("D")()
    if not bad.all() or (cul != 1).any():
        raise SystemExit("bench_locate: case D: not every stripe names "
                         "chunk 0")

    # time the calls themselves, as the C-ABI, without the wrappers'
    # download of the words
    lib, h = ceph_amd.lib(), ctx._h

    def raw_verify():
        r = lib.ecx_verify_batch(h, bufs["clean"], S, C, FULL, d_bad, 0)
        if r != 0:
            raise SystemExit(f"bench_locate: ecx_verify_batch = {r}")

    def raw_locate(buf):
        def call():
            r = lib.ecx_locate_batch(h, bufs[buf], S, C, FULL, d_bad, d_cul,
                                     0)
            if r != 0:
                raise SystemExit(f"bench_locate: ecx_locate_batch = {r}")
        return call

    timed = [("A", raw_verify), ("B", raw_locate("clean")),
             ("C", raw_locate("clean")), ("D", raw_locate("D"))]
    ms = {name: [] for name, _ in timed}
    dev_ms = {name: [] for name, _ in timed}
    for rep in range(A.warmup + A.reps):
        for name, fn in timed:  # alternate the cases within one process
            if name == "C":
                damage()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= A.warmup:
                ms[name].append(dt)
                dev_ms[name].append(ctx.last_kernel_ms())
            if name == "C":
                repair()

    # chunk reads: the verify passes, plus per flagged stripe and candidate
    # k sources + (n_checked - 1) stored chunks
    n_flag = {"A": 0, "B": 0, "C": len(changed), "D": S}
    res = {}
    for name, _ in timed:
        st = stats(ms[name])
        dv = stats(dev_ms[name])
        st["device_span_median_ms"] = dv["median_ms"]
        st["device_span_min_ms"] = dv["min_ms"]
        st["device_span_max_ms"] = dv["max_ms"]
        st["stripes_flagged"] = n_flag[name]
        st["bytes_read"] = (N * S + n_flag[name] * K * (K + M - 1)) * C
        st["GBps_at_median"] = round(st["bytes_read"] / st["median_ms"] / 1e6,
                                     1)
        res[name] = st
    res["C"]["buffer"] = "A's, bytes changed and restored around each call"

    for b in bufs.values():
        ctx.dbuf_free(b)
    ctx.dbuf_free(d_bad)
    ctx.dbuf_free(d_cul)
    ctx.close()

    med = {n: res[n]["median_ms"] for n in res}
    dmed = {n: res[n]["device_span_median_ms"] for n in res}
    out = {
        "metric": "locate_batch (name the corrupt chunk) vs verify_batch",
        "unit": "ms per call, host clock to sync(); device_span = the "
                "call's event pair",
        "config": {"technique": TECH, "k": K, "m": M, "chunk_bytes": C,
                   "n_stripes": S, "reps": A.reps, "warmup": A.warmup,
                   "seed": "0xec",
                   "timing": "cases alternated within one process"},
        "cases": res,
        "B_minus_A_ms": round(med["B"] - med["A"], 4),
        "B_minus_A_device_span_ms": round(dmed["B"] - dmed["A"], 4),
        "B_range_above_A_range": bool(res["B"]["min_ms"] > res["A"]["max_ms"]),
        "C_minus_B_ms": round(med["C"] - med["B"], 4),
        "D_over_A_time": round(med["D"] / med["A"], 4),
        "verified": "B bad 0 and culprit the full mask; C flagged exactly on "
                    "the changed stripes, each naming the changed chunk; D "
                    "every stripe naming chunk 0; one changed stripe of C "
                    "equal to the CPU oracle's words",
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
    with open(A.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
