#!/usr/bin/env python3
"""What does a small overwrite cost by parity delta? (update_batch)

reed_sol_van RS(8,3), device-resident stripes filled with fill_random and
encoded on the device. The cases are alternated within one process, each
timed with a host clock around work that ends in sync():

  A   update_batch, one random data chunk per stripe, 1 MiB chunks, S = 1024
  B   encode_batch alone on the same stripes: the alternative a caller has
      today, WITHOUT its copy of the new data into place — a lower bound on
      what re-encoding costs
  C1..C4  update_batch with the same c = 1, 2, 3, 4 chunks in every stripe:
      locates the measured break-even against B (from bytes: 2c < k - m)
  D   update_batch, 64 KiB chunks at S = 16384, c = 1: the OSD-sized write

Bytes moved are counted from the masks as (3c + 2m) * C per written stripe
(old and new data read, new data written, parity read and written); B moves
(k + m) * C per stripe. Repeating a call on the same buffers is the same
work: after the first call old == new, and nothing in the kernel depends on
the data. Before timing, the tool's own update_batch output is checked
bit-exactly against the CPU oracle on 2 sampled stripes.

Also times the host-pointer apply_delta of one delta into three parities
(what the plugin's apply_delta does per call) at 64 KiB and 1 MiB: the fused
ecx_apply_deltas_host against the loop over ecx_apply_delta_host that the
plugin made before. Not wired into bench.py; prints one JSON line and
writes it to --out."""
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


def popcount(mask):
    return bin(mask).count("1")


def update_bytes(masks, chunk):
    return sum((3 * popcount(mk) + 2 * M) * chunk for mk in masks if mk)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4),
            "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4),
            "reps": len(ms)}


def check_against_oracle(ctx, oracle, d, dn, S, C, masks, rng):
    """One update_batch call; 2 sampled stripes compared with the oracle's
    old_parity ^ G * (old ^ new)."""
    gen = oracle.matrix(TECH, K, M)
    base = ceph_amd.update_plan_probe(K, M, masks)[1]
    picks = [rng.randrange(S), rng.randrange(S)]
    before = {}
    for s in picks:
        old = np.empty((N, C), dtype=np.uint8)
        ctx.download(old, ctypes.c_void_p(d.value + s * N * C))
        new = np.empty((popcount(masks[s]), C), dtype=np.uint8)
        ctx.download(new, ctypes.c_void_p(dn.value + int(base[s]) * C))
        before[s] = (old, new)
    ctx.update_batch(d, S, C, dn, masks)
    ctx.sync()
    for s in picks:
        old, new = before[s]
        want = old.copy()
        ids = [j for j in range(K) if (masks[s] >> j) & 1]
        for t, j in enumerate(ids):
            delta = oracle.xor_region(old[j].copy(), new[t].copy())
            for r in range(M):
                oracle.region_mul_xor(int(gen[K + r, j]), delta, want[K + r])
            want[j] = new[t]
        got = np.empty((N, C), dtype=np.uint8)
        ctx.download(got, ctypes.c_void_p(d.value + s * N * C))
        if not np.array_equal(got, want):
            raise SystemExit(f"bench_update_batch: stripe {s} differs from "
                             "the oracle after update_batch")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--small-chunk", type=int, default=64 << 10)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "bench_update_batch.json"))
    A = ap.parse_args()
    S, C, C2 = A.stripes, A.chunk, A.small_chunk
    if A.reps < 20:
        ap.error("--reps must be >= 20")
    if C % C2 or S * (C // C2) > 65535:
        ap.error("--chunk must be a multiple of --small-chunk and the "
                 "small-chunk stripe count must stay within 65535")
    S2 = S * (C // C2)  # the same bytes as OSD-sized stripes

    rng = random.Random(0xEC)
    masks = {"A": [1 << rng.randrange(K) for _ in range(S)],
             "D": [1 << rng.randrange(K) for _ in range(S2)]}
    for c in (1, 2, 3, 4):
        masks[f"C{c}"] = [(1 << c) - 1] * S
    launches = ceph_amd.update_plan_probe(K, M, masks["A"])[0]

    if ceph_amd.device_count() < 1:
        raise SystemExit("bench_update_batch: no GPU visible — this tool "
                         "measures on the device and has no fallback")
    import oracle  # the checker, never the measured path

    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    total, total_new = S * N * C, 4 * S * C
    d, dn = ctx.dbuf_alloc(total), ctx.dbuf_alloc(total_new)
    ctx.fill_random(d, total, 0xEC)
    ctx.fill_random(dn, total_new, 0xED)
    ctx.encode_batch(d, S, C)
    ctx.sync()
    marr = {n: np.array(mk, dtype=np.uint64) for n, mk in masks.items()}

    check_against_oracle(ctx, oracle, d, dn, S, C, masks["A"], rng)
    check_against_oracle(ctx, oracle, d, dn, S2, C2, masks["D"], rng)

    def upd(name, s, c):
        return lambda: ctx.update_batch(d, s, c, dn, marr[name])

    cases = [("A", upd("A", S, C)),
             ("B", lambda: ctx.encode_batch(d, S, C))]
    cases += [(f"C{c}", upd(f"C{c}", S, C)) for c in (1, 2, 3, 4)]
    cases.append(("D", upd("D", S2, C2)))
    for _ in range(A.warmup):
        for _, fn in cases:
            fn()
            ctx.sync()
    ms = {name: [] for name, _ in cases}
    dev_ms = {name: [] for name, _ in cases}
    for _ in range(A.reps):
        for name, fn in cases:  # alternate the cases within one process
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dev_ms[name].append(ctx.last_kernel_ms())

    res = {}
    for name, _ in cases:
        st = stats(ms[name])
        st["bytes_moved"] = (N * C * S if name == "B" else update_bytes(
            masks[name], C2 if name == "D" else C))
        st["GBps_at_median"] = round(st["bytes_moved"] / st["median_ms"] / 1e6,
                                     1)
        st["device_span_median_ms"] = round(float(np.median(dev_ms[name])), 4)
        if name != "B":
            st["launches"] = launches
        res[name] = st
    med = {n: res[n]["median_ms"] for n in res}
    ctx.dbuf_free(d)
    ctx.dbuf_free(dn)

    # ---- host-pointer apply_delta: 1 delta into 3 parities ----
    host = {}
    nrng = np.random.default_rng(0xEC)
    for nbytes in (C2, C):
        delta = nrng.integers(0, 256, nbytes, dtype=np.uint8)
        par = {K + r: nrng.integers(0, 256, nbytes, dtype=np.uint8)
               for r in range(M)}
        loop_out = {c: p.copy() for c, p in par.items()}
        for c, p in loop_out.items():
            ctx.apply_delta(delta, 3, c, p)
        fused_out = ctx.apply_deltas({3: delta},
                                     {c: p.copy() for c, p in par.items()})
        if any(not np.array_equal(fused_out[c], loop_out[c]) for c in par):
            raise SystemExit("bench_update_batch: fused apply_deltas differs "
                             "from the pair loop")

        def fused():
            ctx.apply_deltas({3: delta}, par)

        def loop():
            for c, p in par.items():
                ctx.apply_delta(delta, 3, c, p)

        hc = [("fused", fused), ("pair_loop", loop)]
        for _ in range(A.warmup):
            for _, fn in hc:
                fn()
        hms = {n: [] for n, _ in hc}
        for _ in range(A.reps):
            for n, fn in hc:
                t0 = time.perf_counter()
                fn()
                hms[n].append((time.perf_counter() - t0) * 1e3)
        host[str(nbytes)] = {n: stats(v) for n, v in hms.items()}
        host[str(nbytes)]["fused_over_loop_time"] = round(
            host[str(nbytes)]["fused"]["median_ms"] /
            host[str(nbytes)]["pair_loop"]["median_ms"], 4)
    ctx.close()

    out = {
        "metric": "update_batch (parity delta) vs encode_batch (re-encode)",
        "unit": "ms per call, host clock to sync()",
        "config": {"technique": TECH, "k": K, "m": M, "chunk_bytes": C,
                   "n_stripes": S, "small_chunk_bytes": C2,
                   "small_n_stripes": S2, "reps": A.reps,
                   "warmup": A.warmup, "seed": "0xec",
                   "timing": "cases alternated within one process"},
        "cases": res,
        "A_over_B_time": round(med["A"] / med["B"], 4),
        "A_over_B_from_bytes": round((3 + 2 * M) / N, 4),
        "C_over_B_time": {f"c={c}": round(med[f"C{c}"] / med["B"], 4)
                          for c in (1, 2, 3, 4)},
        "break_even_from_bytes": "2c < k - m, c <= 2",
        "apply_delta_host_1_delta_3_parities": host,
        "verified": "2 sampled stripes per chunk size bit-exact vs CPU "
                    "oracle; fused host call equal to the pair loop",
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
    with open(A.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
