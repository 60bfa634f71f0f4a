"""ec_gf_stream_kernel under its grid and walk knobs. ECX_STREAM_BPC and
ECX_STREAM_ORDER are read once per process, so each setting is checked in
a child process of its own (that is what this test is about): one encode
and one decode of a batch with more tiles than blocks and 3 tiles per
chunk, bit-exact against the oracle. Run as a script, this file is the
child."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# 800 stripes x 3 tiles = 2400 tiles: more than a persistent grid (at most
# 8 x 256 = 2048 blocks) and more than 3 blocks per CU; in either walk order
# the grid step is no multiple of the inner dimension, so the walk carries.
K, M, S, C = 4, 2, 800, 12272

KNOBS = [
    {"ECX_STREAM_ORDER": "1"},
    {"ECX_STREAM_BPC": "0"},
    {"ECX_STREAM_BPC": "3", "ECX_STREAM_ORDER": "1"},
]


def child():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import numpy as np

    import ceph_amd
    import oracle
    import test_gpu_stream_kernel as t

    n = K + M
    rows = oracle.matrix(t.TECH, K, M)[K:]
    host = t.rand_batch(7, S, n, C)
    want = host.copy()
    t.ref_matmul(want, list(range(K)), list(range(K, n)), rows)
    ctx = ceph_amd.EcContext(K, M, t.TECH, device=0)
    try:
        dev = t.Dev(ctx, host)
        ctx.encode_batch(dev.d, S, C)
        got = dev.get(host.shape)
        dev.free()
        assert np.array_equal(got, want), "encode mismatch"
        t.check_decode(ctx, want, (1, 4), S, C)
    finally:
        ctx.close()
    print("KNOBS_OK")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS,
                         ids=lambda d: ",".join(f"{k}={v}"
                                                for k, v in d.items()))
def test_stream_knob_setting(knobs):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("ECX_STREAM")}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KNOBS_OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    child()
