#!/usr/bin/env python3
"""What does the per-shard CRC-32C of a device batch cost? (crc32c_batch)

reed_sol_van RS(8,3), 1 MiB chunks, S = 1024, device-resident stripes filled
with fill_random and encoded on the device. The cases are alternated within
one process, each timed with a host clock around call + sync() and with the
call's own device events (last_kernel_ms, first launch to last):

  A   crc32c_batch, all 11 chunks
  B   verify_batch, full mask, on the same buffer: it reads exactly the same
      bytes with a kernel this tool does not touch — the read-only yardstick
  C   crc32c_batch, the 8 data chunks only
  D   crc32c_batch, all chunks, chain mode (the batch as 1024 consecutive
      stripes of one object)
  E   for context only: crc32c_probe on the host over one stripe's worth of
      bytes (11 MiB), one thread, with the path it took named

Bytes are counted as (chunks hashed) * C * S. Before timing, A's words of
three sampled stripes are compared bit for bit with crc32c_probe over the
downloaded chunks, and D's rows 0..2 with the probe chained over the chunks
of stripes 0..2. Not wired into bench.py; prints one JSON line and writes it
to --out."""
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
DATA = (1 << K) - 1


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4),
            "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "bench_crc.json"))
    A = ap.parse_args()
    S, C = A.stripes, A.chunk
    if A.reps < 20:
        ap.error("--reps must be >= 20")
    if S < 3 or S > 65535 or C % 16:
        ap.error("--stripes must be 3..65535 and --chunk a multiple of 16")
    if ceph_amd.device_count() < 1:
        raise SystemExit("bench_crc: no GPU visible — this tool measures on "
                         "the device and has no fallback")

    rng = random.Random(0xC3C)
    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    total = S * N * C
    d = ctx.dbuf_alloc(total)
    ctx.fill_random(d, total, 0xEC)
    ctx.encode_batch(d, S, C)
    ctx.sync()
    d_crc = ctx.dbuf_alloc(4 * S * N)
    d_bad = ctx.dbuf_alloc(8 * S)

    # ---- the words, before anything is timed ----
    words = ctx.crc32c_batch(d, S, C, d_crc=d_crc)
    stripe = np.empty((N, C), dtype=np.uint8)
    for s in sorted(rng.sample(range(S), 3)):
        ctx.download(stripe, ctypes.c_void_p(d.value + s * N * C))
        for c in range(N):
            want = ceph_amd.crc32c_probe(0xFFFFFFFF, stripe[c])
            if int(words[s, c]) != want:
                raise SystemExit(f"bench_crc: stripe {s} chunk {c}: "
                                 f"{int(words[s, c]):#x}, host {want:#x}")
    chained = ctx.crc32c_batch(d, S, C, chain=True, d_crc=d_crc)
    run = [0xFFFFFFFF] * N
    for s in range(3):
        ctx.download(stripe, ctypes.c_void_p(d.value + s * N * C))
        run = [ceph_amd.crc32c_probe(run[c], stripe[c]) for c in range(N)]
        if [int(v) for v in chained[s]] != run:
            raise SystemExit(f"bench_crc: chain row {s} differs from the host")
    if ctx.verify_batch(d, S, C, FULL, d_bad).any():
        raise SystemExit("bench_crc: the encoded batch was flagged")

    lib, h = ceph_amd.lib(), ctx._h

    def crc(mask, chain):
        def call():
            r = lib.ecx_crc32c_batch(h, d, S, C, mask, None, chain, d_crc, 0)
            if r != 0:
                raise SystemExit(f"bench_crc: ecx_crc32c_batch = {r}")
        return call

    def verify():
        r = lib.ecx_verify_batch(h, d, S, C, FULL, d_bad, 0)
        if r != 0:
            raise SystemExit(f"bench_crc: ecx_verify_batch = {r}")

    timed = [("A", crc(FULL, 0), N), ("B", verify, N),
             ("C", crc(DATA, 0), K), ("D", crc(FULL, 1), N)]
    for _ in range(A.warmup):
        for _, fn, _ in timed:
            fn()
            ctx.sync()
    ms = {name: [] for name, _, _ in timed}
    dev_ms = {name: [] for name, _, _ in timed}
    for _ in range(A.reps):
        for name, fn, _ in timed:  # alternate the cases within one process
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dev_ms[name].append(ctx.last_kernel_ms())

    res = {}
    for name, _, chunks_read in timed:
        st = stats(ms[name])
        dv = stats(dev_ms[name])
        st["device_span_median_ms"] = dv["median_ms"]
        st["device_span_min_ms"] = dv["min_ms"]
        st["device_span_max_ms"] = dv["max_ms"]
        st["bytes_read"] = chunks_read * C * S
        st["GBps_at_median"] = round(st["bytes_read"] / st["median_ms"] / 1e6,
                                     1)
        st["GBps_at_device_median"] = round(
            st["bytes_read"] / dv["median_ms"] / 1e6, 1)
        res[name] = st

    # E: the host's own hash, one thread, one stripe's worth of bytes
    ctx.download(stripe, d)
    flat = stripe.reshape(-1)
    _, path = ceph_amd.crc32c_probe(0xFFFFFFFF, flat[:4096], with_path=True)
    host_ms = []
    for _ in range(max(5, A.reps // 4)):
        t0 = time.perf_counter()
        ceph_amd.crc32c_probe(0xFFFFFFFF, flat)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["E"] = stats(host_ms)
    res["E"]["bytes_read"] = int(flat.nbytes)
    res["E"]["path"] = path
    res["E"]["GBps_at_median"] = round(
        flat.nbytes / res["E"]["median_ms"] / 1e6, 2)

    plan = ceph_amd.crc32c_plan_probe(C, S, N)
    for p in (d, d_crc, d_bad):
        ctx.dbuf_free(p)
    ctx.close()

    dmed = {n: res[n]["device_span_median_ms"] for n in "ABCD"}
    out = {
        "metric": "crc32c_batch (per-shard CRC-32C) vs verify_batch reading "
                  "the same bytes",
        "unit": "ms per call, host clock to sync(); device_span = the "
                "call's event pair",
        "config": {"technique": TECH, "k": K, "m": M, "chunk_bytes": C,
                   "n_stripes": S, "reps": A.reps, "warmup": A.warmup,
                   "seed": "0xec", "plan": plan,
                   "timing": "cases alternated within one process"},
        "cases": res,
        "A_over_B_device_span": round(dmed["A"] / dmed["B"], 4),
        "A_over_B_time": round(res["A"]["median_ms"] / res["B"]["median_ms"],
                               4),
        "C_over_A_device_span": round(dmed["C"] / dmed["A"], 4),
        "D_over_A_device_span": round(dmed["D"] / dmed["A"], 4),
        "verified": "A equal to crc32c_probe on 3 sampled stripes (33 "
                    "chunks); chain rows 0..2 equal to the probe chained "
                    "over the same chunks; the batch clean under "
                    "verify_batch",
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
    with open(A.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
