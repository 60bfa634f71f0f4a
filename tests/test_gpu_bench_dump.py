"""bench.py --dump-outputs on the GPU: the dumped sample must be what the
timed path computed (bit-exact vs the oracle on the deterministic fill),
and a plain run's result line must carry consistent headline fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_plain_run_dumps_last_step_outputs(tmp_path):
    import bench
    k, m, S, C, steps, seed = 8, 3, 8, 64 * 1024, 3, 0xEC
    n = k + m
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps),
         "--warmup", "1", "--stripes", str(S), "--chunk-kib", str(C >> 10),
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "EC encode+decode GiB/s"
    assert line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None  # --full only
    # value and ms_per_step describe the same timed steps (both rounded:
    # value to 0.01, ms_per_step to 0.001)
    want = 2 * k * C * S / bench.GIB / (line["ms_per_step"] * 1e-3)
    tol = 0.0005 / line["ms_per_step"] + 0.005 / line["value"] + 1e-6
    assert abs(line["value"] - want) <= tol * want * 1.01

    parity = np.load(tmp_path / "parity.npy")
    decoded = np.load(tmp_path / "decoded.npy")
    erased = line["config"]["erasures"]
    assert parity.dtype == np.float32 and decoded.dtype == np.float32
    assert parity.nbytes + decoded.nbytes <= 64 * 1000 * 1000
    # at this size every stripe is sampled and each window is a whole chunk
    assert parity.shape == (S, m, 3, C)
    assert decoded.shape == (S, len(erased), 3, C)
    for s in range(S):
        fill = bench.expected_fill(s * n * C, k * C, seed)
        data = [fill[i * C:(i + 1) * C] for i in range(k)]
        full = data + oracle.encode("reed_sol_van", k, m, data)
        for w in range(3):
            for j in range(m):
                assert np.array_equal(parity[s, j, w], full[k + j]), (s, j)
            for j, e in enumerate(erased):
                assert np.array_equal(decoded[s, j, w], full[e]), (s, e)
