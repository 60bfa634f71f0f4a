#!/usr/bin/env python3
"""What does it cost to ask whether stored stripes are consistent?
(verify_batch)

reed_sol_van RS(8,3), 1 MiB chunks, S = 1024, device-resident stripes filled
with fill_random and encoded on the device. The cases are alternated within
one process, each timed with a host clock around call + sync() and with the
call's own device events (last_kernel_ms, first launch to last):

  A   verify_batch, full mask, clean batch
  B   encode_batch on the same stripes: the existing call that moves the same
      11 chunk transfers per stripe (8 reads + 3 writes where A has 11
      reads), and the comparison point
  C   verify_batch, one data chunk absent: 8 survivors, 2 checked
  D   verify_batch, full mask, one byte changed in 1 % of the stripes: what a
      realistic scrub pays for reporting. It runs on A's own buffer (the
      bytes are changed before each timed call and put back after it,
      outside the timed window), because the same kernel on another
      allocation of the same size differs by more than reporting costs
  E   verify_batch, full mask, chunk 0 of every stripe overwritten with
      random bytes: every wave reports, the atomic worst case

Bytes are counted as (k + n_checked) * C * S. Before timing, the words of
every verify case are checked: A and C all zero, D nonzero exactly on the
changed stripes, E nonzero everywhere, and one changed and one clean stripe of
D and one stripe of E against the CPU oracle's rebuild from the survivors.
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
ABSENT = 2  # case C: this data chunk is not held


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4),
            "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4),
            "reps": len(ms)}


def oracle_word(oracle, ctx, d, s, C, mask):
    """Stripe s of batch d: the word the oracle's rebuild from the survivors
    gives (the reference of tests/test_gpu_verify.py)."""
    stored = np.empty((N, C), dtype=np.uint8)
    ctx.download(stored, ctypes.c_void_p(d.value + s * N * C))
    present = [i for i in range(N) if mask >> i & 1]
    chunks = [stored[i].copy() for i in range(N)]
    oracle.decode(TECH, K, M, chunks,
                  [int(i in present[:K]) for i in range(N)])
    return sum(1 << i for i in present[K:]
               if not np.array_equal(chunks[i], stored[i]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "bench_verify.json"))
    A = ap.parse_args()
    S, C = A.stripes, A.chunk
    if A.reps < 20:
        ap.error("--reps must be >= 20")
    if S < 100 or S > 65535 or C % 16:
        ap.error("--stripes must be 100..65535 and --chunk a multiple of 16")

    if ceph_amd.device_count() < 1:
        raise SystemExit("bench_verify: no GPU visible — this tool measures "
                         "on the device and has no fallback")
    import oracle  # the checker, never the measured path

    rng = random.Random(0xEC)
    ctx = ceph_amd.EcContext(K, M, TECH, device=0)
    total = S * N * C
    # two copies of one encoded batch: clean (A, B, C, D), chunk 0 random (E)
    bufs = {}
    for name in ("clean", "E"):
        bufs[name] = ctx.dbuf_alloc(total)
        ctx.fill_random(bufs[name], total, 0xEC)
        ctx.encode_batch(bufs[name], S, C)
    ctx.sync()
    # case D: one byte in each of 1 % of the stripes, anywhere in the stripe
    changed = sorted(rng.sample(range(S), max(1, S // 100)))
    flips = []
    for s in changed:
        at = ctypes.c_void_p(bufs["clean"].value
                             + (s * N + rng.randrange(N)) * C
                             + rng.randrange(C))
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
        ctx.fill_random(ctypes.c_void_p(bufs["E"].value + s * N * C), C,
                        0xE000 + s)
    ctx.sync()
    d_bad = ctx.dbuf_alloc(8 * S)
    mask_c = FULL & ~(1 << ABSENT)

    def ver(buf, mask):
        return lambda: ctx.verify_batch(bufs[buf], S, C, mask, d_bad)

    cases = [("A", ver("clean", FULL), N),
             ("B", lambda: ctx.encode_batch(bufs["clean"], S, C), N),
             ("C", ver("clean", mask_c), K + 2),
             ("D", ver("clean", FULL), N),
             ("E", ver("E", FULL), N)]

    # ---- the words, before anything is timed ----
    words = {}
    for name, fn, _ in cases:
        if name == "D":
            damage()
        if name != "B":
            words[name] = fn()
        if name == "D":
            repair()
    if words["A"].any() or words["C"].any():
        raise SystemExit("bench_verify: a clean batch was flagged")
    if sorted(np.flatnonzero(words["D"])) != changed:
        raise SystemExit("bench_verify: case D flags other stripes than the "
                         "changed ones")
    if not words["E"].all():
        raise SystemExit("bench_verify: case E has an unflagged stripe")
    clean_s = next(s for s in range(S) if s not in changed)
    damage()
    for case, buf, s in (("D", "clean", changed[0]), ("D", "clean", clean_s),
                         ("E", "E", rng.randrange(S))):
        want = oracle_word(oracle, ctx, bufs[buf], s, C, FULL)
        if int(words[case][s]) != want:
            raise SystemExit(f"bench_verify: case {case} stripe {s}: word "
                             f"{int(words[case][s]):#x}, oracle {want:#x}")
    repair()
    if ctx.verify_batch(bufs["clean"], S, C, FULL, d_bad).any():
        raise SystemExit("bench_verify: the changed bytes were not put back")

    for _ in range(A.warmup):
        for name, fn, _ in cases:
            if name == "D":
                damage()
            fn()
            ctx.sync()
            if name == "D":
                repair()
    # time the calls themselves: verify_batch as the C-ABI, without the
    # wrapper's download of the words
    lib, h = ceph_amd.lib(), ctx._h

    def raw(buf, mask):
        def call():
            r = lib.ecx_verify_batch(h, bufs[buf], S, C, mask, d_bad, 0)
            if r != 0:
                raise SystemExit(f"bench_verify: ecx_verify_batch = {r}")
        return call

    timed = [("A", raw("clean", FULL)), ("B", cases[1][1]),
             ("C", raw("clean", mask_c)), ("D", raw("clean", FULL)),
             ("E", raw("E", FULL))]
    ms = {name: [] for name, _ in timed}
    dev_ms = {name: [] for name, _ in timed}
    for _ in range(A.reps):
        for name, fn in timed:  # alternate the cases within one process
            if name == "D":
                damage()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dev_ms[name].append(ctx.last_kernel_ms())
            if name == "D":
                repair()

    res = {}
    for name, _, chunks_moved in cases:
        st = stats(ms[name])
        dv = stats(dev_ms[name])
        st["device_span_median_ms"] = dv["median_ms"]
        st["device_span_min_ms"] = dv["min_ms"]
        st["device_span_max_ms"] = dv["max_ms"]
        st["bytes_moved"] = chunks_moved * C * S
        st["GBps_at_median"] = round(st["bytes_moved"] / st["median_ms"] / 1e6,
                                     1)
        st["GBps_at_device_median"] = round(
            st["bytes_moved"] / dv["median_ms"] / 1e6, 1)
        res[name] = st
    res["D"]["stripes_changed"] = len(changed)
    res["D"]["buffer"] = "A's, bytes changed and restored around each call"
    res["C"]["absent_chunk"] = ABSENT

    for b in bufs.values():
        ctx.dbuf_free(b)
    ctx.dbuf_free(d_bad)
    ctx.close()

    med = {n: res[n]["median_ms"] for n in res}
    dmed = {n: res[n]["device_span_median_ms"] for n in res}
    out = {
        "metric": "verify_batch (consistency check) vs encode_batch",
        "unit": "ms per call, host clock to sync(); device_span = the "
                "call's event pair",
        "config": {"technique": TECH, "k": K, "m": M, "chunk_bytes": C,
                   "n_stripes": S, "reps": A.reps, "warmup": A.warmup,
                   "seed": "0xec",
                   "timing": "cases alternated within one process"},
        "cases": res,
        "A_over_B_time": round(med["A"] / med["B"], 4),
        "A_over_B_device_span": round(dmed["A"] / dmed["B"], 4),
        "A_range_above_B_range": bool(res["A"]["min_ms"] > res["B"]["max_ms"]),
        "D_over_A_time": round(med["D"] / med["A"], 4),
        "E_over_A_time": round(med["E"] / med["A"], 4),
        "verified": "A and C all zero; D nonzero exactly on the changed "
                    "stripes; E nonzero everywhere; 3 sampled stripes equal "
                    "to the CPU oracle's rebuild from the survivors",
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
    with open(A.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
