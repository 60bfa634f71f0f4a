#!/usr/bin/env python3
"""What does a per-stripe erasure pattern cost? (decode_batch_multi)

reed_sol_van RS(8,3), 1 MiB chunks, S = 1024 device-resident stripes,
filled with fill_random and encoded on the device. Four cases, alternated
within one process, each timed with a host clock around work that ends in
sync():

  A  one uniform 3-erasure mask through decode_batch (existing code: the
     ceiling)
  B  the same uniform mask through decode_batch_multi (cost of the
     per-block record indirection alone, equal bytes)
  C  64 distinct random masks with 1-3 erasures, assigned round-robin so
     neighbouring stripes differ, through decode_batch_multi
  D  the work of C as the uniform API allows it: the same stripes laid out
     contiguous by pattern, one decode_batch per pattern (64 launches).
     D cannot serve C's interleaved layout at all; it is the best case of
     "sort by pattern first".

Bytes moved are counted per case from the masks (k survivor reads + one
write per erased chunk, per stripe that loses anything). Before timing, the
tool's own decode_batch_multi output is checked bit-exactly against the CPU
oracle on 2 sampled stripes. Not wired into bench.py; prints one JSON line
and writes it to --out."""
import argparse
import ctypes
import json
import os
import random
import sys
import time
from itertools import combinations

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import ceph_amd  # noqa: E402

K, M, TECH = 8, 3, "reed_sol_van"
N = K + M
FULL = (1 << N) - 1


def n_erased(mask):
    return N - bin(mask & FULL).count("1")


def bytes_moved(masks, chunk):
    return sum((K + n_erased(mk)) * chunk for mk in masks if n_erased(mk))


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4),
            "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4),
            "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--patterns", type=int, default=64)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "bench_decode_multi.json"))
    A = ap.parse_args()
    S, C, P = A.stripes, A.chunk, A.patterns
    if A.reps < 20:
        ap.error("--reps must be >= 20")
    if S % P:
        ap.error("--stripes must be a multiple of --patterns")

    rng = random.Random(0xEC)
    every = [FULL & ~sum(1 << c for c in er) for e in (1, 2, 3)
             for er in combinations(range(N), e)]
    pats = rng.sample(every, P)
    uniform = FULL & ~((1 << 1) | (1 << 6) | (1 << (K + 1)))  # 2 data + 1 parity
    masks_a = [uniform] * S
    masks_c = [pats[s % P] for s in range(S)]                # interleaved
    masks_d = [pats[s // (S // P)] for s in range(S)]        # sorted runs
    # refuses (EIO) here, on the CPU, if any pattern were undecodable
    launches_c = ceph_amd.decode_multi_plan_probe(TECH, K, M, masks_c)[0]
    launches_b = ceph_amd.decode_multi_plan_probe(TECH, K, M, masks_a)[0]

    if ceph_amd.device_count() < 1:
        raise SystemExit("bench_decode_multi: no GPU visible — this tool "
                         "measures on the device and has no fallback")
    import oracle  # the checker, never the measured path

    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    total = S * N * C
    d = ctx.dbuf_alloc(total)
    ctx.fill_random(d, total, 0xEC)
    ctx.encode_batch(d, S, C)
    ctx.sync()

    # ---- bit-exact check of the tool's own output on 2 sampled stripes ----
    mc = np.array(masks_c, dtype=np.uint64)
    ma = np.array(masks_a, dtype=np.uint64)
    for s in (rng.randrange(S), rng.randrange(S)):
        sp = ctypes.c_void_p(d.value + s * N * C)
        want = np.empty(N * C, dtype=np.uint8)
        ctx.download(want, sp)
        oracle.cpu_encode_batch(TECH, K, M, want, 1, C)  # parity from data
        poison = np.full(C, 0xA5, dtype=np.uint8)
        for c in range(N):
            if not (masks_c[s] >> c) & 1:
                ctx.upload(ctypes.c_void_p(sp.value + c * C), poison)
        ctx.decode_batch_multi(d, S, C, mc)
        ctx.sync()
        got = np.empty(N * C, dtype=np.uint8)
        ctx.download(got, sp)
        if not np.array_equal(got, want):
            raise SystemExit(f"bench_decode_multi: stripe {s} differs from "
                             "the oracle after decode_batch_multi")

    run_len = S // P

    def case_a():
        ctx.decode_batch(d, S, C, uniform)

    def case_b():
        ctx.decode_batch_multi(d, S, C, ma)

    def case_c():
        ctx.decode_batch_multi(d, S, C, mc)

    def case_d():
        for p in range(P):
            ctx.decode_batch(ctypes.c_void_p(d.value + p * run_len * N * C),
                             run_len, C, pats[p])

    cases = [("A", case_a), ("B", case_b), ("C", case_c), ("D", case_d)]
    for _ in range(A.warmup):
        for _, fn in cases:
            fn()
            ctx.sync()
    ms = {name: [] for name, _ in cases}
    dev_ms = {"B": [], "C": []}
    for _ in range(A.reps):
        for name, fn in cases:  # alternate the cases within one process
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if name in dev_ms:
                dev_ms[name].append(ctx.last_kernel_ms())

    nbytes = {"A": bytes_moved(masks_a, C), "B": bytes_moved(masks_a, C),
              "C": bytes_moved(masks_c, C), "D": bytes_moved(masks_d, C)}
    res = {}
    for name, _ in cases:
        st = stats(ms[name])
        st["bytes_moved"] = nbytes[name]
        st["GBps_at_median"] = round(nbytes[name] / st["median_ms"] / 1e6, 1)
        res[name] = st
    for name in dev_ms:
        res[name]["device_span_median_ms"] = round(
            float(np.median(dev_ms[name])), 4)
    res["B"]["launches"] = launches_b
    res["C"]["launches"] = launches_c
    res["D"]["launches"] = P
    med = {n: res[n]["median_ms"] for n in res}
    out = {
        "metric": "decode_batch_multi vs uniform decode_batch",
        "unit": "ms per call, host clock to sync()",
        "config": {"technique": TECH, "k": K, "m": M, "chunk_bytes": C,
                   "n_stripes": S, "patterns": P, "reps": A.reps,
                   "warmup": A.warmup, "seed": "0xec",
                   "timing": "cases alternated within one process"},
        "cases": res,
        "B_over_A_time": round(med["B"] / med["A"], 4),
        "C_GBps_over_A_GBps": round(res["C"]["GBps_at_median"] /
                                    res["A"]["GBps_at_median"], 4),
        "C_over_D_time": round(med["C"] / med["D"], 4),
        "verified": "2 sampled stripes bit-exact vs CPU oracle",
    }
    ctx.dbuf_free(d)
    ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
    with open(A.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
