"""ec_gf_stream_kernel under the stripe-group width and XCD-mapping knobs of
its tile walk. ECX_STREAM_W and ECX_STREAM_XCD are read once per process,
so each setting is checked in a child process of its own (that is what this
test is about): one encode and one decode, bit-exact against the oracle, of
the batch of test_gpu_stream_knobs.py (3 tiles per chunk with the last one
partial, more tiles than resident blocks, a grid step that carries), and
one cauchy(10,4) batch for the 4-output instance. Run as a script, this
file is the child."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

C = 12272
# (technique, k, m, stripes, erased chunks, knobs)
RS = ("reed_sol_van", 4, 2, 800, (1, 4))
CASES = [
    RS + ({"ECX_STREAM_XCD": "1"},),
    RS + ({"ECX_STREAM_W": "3"},),  # does not divide 800
    RS + ({"ECX_STREAM_W": "16", "ECX_STREAM_XCD": "1",
           "ECX_STREAM_BPC": "3"},),
    RS + ({"ECX_STREAM_W": "16", "ECX_STREAM_XCD": "1",
           "ECX_STREAM_BPC": "0"},),
    ("cauchy", 10, 4, 40, (1, 4), {"ECX_STREAM_XCD": "1"}),
    # the mapping is on by default: blocks in hardware order, grid-striding
    RS + ({"ECX_STREAM_XCD": "0", "ECX_STREAM_BPC": "3"},),
]


def child(tech, k, m, S, erased):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import numpy as np

    import ceph_amd
    import oracle
    import test_gpu_stream_kernel as t

    n = k + m
    rows = oracle.matrix(tech, k, m)[k:]
    host = t.rand_batch(7, S, n, C)
    want = host.copy()
    t.ref_matmul(want, list(range(k)), list(range(k, n)), rows)
    ctx = ceph_amd.EcContext(k, m, tech, device=0)
    try:
        dev = t.Dev(ctx, host)
        ctx.encode_batch(dev.d, S, C)
        got = dev.get(host.shape)
        dev.free()
        assert np.array_equal(got, want), "encode mismatch"
        t.check_decode(ctx, want, erased, S, C)
    finally:
        ctx.close()
    print("WALK_OK")


def _id(case):
    tech, k, m, S, _, knobs = case
    return f"{tech}{k}+{m}x{S}," + ",".join(f"{a}={b}"
                                            for a, b in knobs.items())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_stream_walk_setting(case):
    tech, k, m, S, erased, knobs = case
    env = {a: b for a, b in os.environ.items()
           if not a.startswith("ECX_STREAM")}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    cmd += [os.path.abspath(__file__), tech, str(k), str(m), str(S),
            ",".join(map(str, erased))]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "WALK_OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    a = sys.argv[1:]
    child(a[0], int(a[1]), int(a[2]), int(a[3]),
          tuple(int(e) for e in a[4].split(",")))
