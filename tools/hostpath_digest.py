#!/usr/bin/env python3
"""Digest of the host-pointer (plugin) path's outputs, for comparing two
builds of the core: one SHA-256 line per case, fixed seed. Run it on each
build and diff the output; equal lines mean byte-identical parity and
reconstructions.

Cases: every technique family (w=8 table, w=16, bitmatrix), encode and
decode, chunks of 64 KiB, 1 MiB and 4 MiB + 16 bytes (bitmatrix chunks are
whole multiples of w * packetsize = 16 KiB, so 4 MiB + 16 KiB there), an
encode with a zeros chunk, and the 64 KiB cases once more under
ECX_HOSTPIPE=0. Knobs are
read once per process, so that last set runs in a fresh child of this
script.

    python tools/hostpath_digest.py > digest.txt
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("reed_sol_van", "jerasure_reed_sol_van_w16", "cauchy_orig")
K, M, PKT = 4, 2, 2048
SIZES = (64 << 10, 1 << 20, (4 << 20) + 16)
SEED = 0xD16E57


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def run_cases(label, sizes):
    import ceph_amd
    for t, tech in enumerate(FAMILIES):
        ctx = ceph_amd.EcContext(K, M, tech, device=0, packetsize=PKT)
        for C in sizes:
            if tech == "cauchy_orig":
                C = -(-C // (8 * PKT)) * (8 * PKT)
            rng = np.random.default_rng(SEED + 131 * t + C)
            data = [rng.integers(0, 256, C, dtype=np.uint8) for _ in range(K)]
            par = ctx.encode_chunks(data)
            print(f"{digest(par)}  {label} {tech} C={C} encode")
            zdata = list(data)
            zdata[1] = None
            zpar = ctx.encode_chunks(zdata, chunk_bytes=C)
            print(f"{digest(zpar)}  {label} {tech} C={C} encode zeros[1]")
            for erase in ((0, K + 1), (2, 3)):
                chunks = [d.copy() for d in data] + [p.copy() for p in par]
                for e in erase:
                    chunks[e][:] = 0xA5
                ctx.decode_chunks(chunks,
                                  [i not in erase for i in range(K + M)])
                got = [chunks[e] for e in erase]
                print(f"{digest(got)}  {label} {tech} C={C} decode {erase}")
        ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--hostpipe0-child":
        run_cases("hostpipe=0", SIZES[:1])
        return
    run_cases("default", SIZES)
    sys.stdout.flush()
    env = dict(os.environ, ECX_HOSTPIPE="0")
    subprocess.run([sys.executable, os.path.abspath(__file__),
                    "--hostpipe0-child"], env=env, check=True, timeout=300)


if __name__ == "__main__":
    main()
