"""ec_plugin_diff on the CPU: the tool that tests/test_gpu_plugin_diff.py
relies on must itself pass where both sides are the same plugin and must
notice when they are not. Everything here runs the oracle fixture plugin on
both sides (directly, or as the sub-plugin of lrc and clay)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "ceph_amd", "harness")
STEPS = ("shape", "minimum", "encode", "encode_want", "encode_chunks",
         "decode", "decode_chunks", "delta", "repeat")


def run_diff(*args, env=None, timeout=120):
    tool = os.path.join(HARNESS, "ec_plugin_diff")
    assert os.path.exists(tool), "ec_plugin_diff not built (run `make harness`)"
    return subprocess.run([tool, "-d", HARNESS, *args], capture_output=True,
                          text=True, env=env, timeout=timeout)


def profile(**kv):
    args = []
    for k, v in kv.items():
        args += ["-P", f"{k}={v}"]
    return args


def steps_of(stdout):
    """{step: ("compared", N) or ("skipped", reason)} from the STEP lines."""
    out = {}
    for m in re.finditer(r"^STEP (\w+) (compared|skipped)=(.*)$", stdout, re.M):
        out[m.group(1)] = (m.group(2), m.group(3))
    return out


def assert_passed(r, allowed_skips=(), steps=STEPS):
    """Exit 0, DIFF_OK, every step compared something; a skip only where the
    caller allows it."""
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("DIFF_OK"), r.stdout
    got = steps_of(r.stdout)
    assert set(got) == set(steps), r.stdout
    for step, (kind, val) in got.items():
        if kind == "skipped":
            assert step in allowed_skips, f"unexpected skip: {step}: {val}"
        else:
            assert int(val) > 0, f"{step} compared nothing"


# widths: the smallest chunk, an odd width that pads the last chunk, and one
# larger stripe
@pytest.mark.parametrize("prof", [
    dict(technique="reed_sol_van", k=4, m=2),
    dict(technique="jerasure_reed_sol_van", w=16, k=4, m=3),
    dict(technique="cauchy_orig", k=4, m=2, packetsize=32),
], ids=["reed_sol_van", "w16", "cauchy_orig"])
def test_oracle_against_itself(prof):
    r = run_diff("--ref", "oracle", "--dut", "oracle", *profile(**prof),
                 "-s", "1", "-s", "4097", "-s", "65536")
    assert_passed(r)


def test_lrc_oracle_layers_against_itself():
    """lrc claims no parity delta: that skip, and no other."""
    r = run_diff("--ref", "lrc", "--dut", "lrc", *profile(k=4, m=2, l=3),
                 "-P", "lrc-default-plugin=oracle", "-s", "1", "-s", "4097")
    assert_passed(r, allowed_skips=("delta",))
    assert steps_of(r.stdout)["delta"][0] == "skipped"


def test_clay_oracle_mds_against_itself():
    r = run_diff("--ref", "clay", "--dut", "clay", *profile(k=4, m=2, d=5),
                 "-P", "scalar_mds=oracle", "-s", "1", "-s", "4097")
    assert_passed(r, allowed_skips=("delta",))
    assert steps_of(r.stdout)["delta"][0] == "skipped"


def diff_line(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("DIFF ")]
    assert len(lines) == 1, r.stdout + r.stderr
    assert "DIFF_OK" not in r.stdout
    return lines[0]


def test_detects_other_generator_in_encode():
    """reed_sol_van against cauchy: same data chunks, other parity. The
    first difference is in step encode, in a parity shard (id >= k)."""
    r = run_diff("--ref", "oracle", "--dut", "oracle", *profile(k=4, m=2),
                 "--ref-P", "technique=reed_sol_van",
                 "--dut-P", "technique=cauchy", "-s", "4096")
    assert r.returncode == 1, r.stdout + r.stderr
    line = diff_line(r)
    assert "step=encode " in line and "width=4096" in line, line
    m = re.search(r"shard=(\d+) offset=(\d+) ref=0x[0-9a-f]{2} "
                  r"dut=0x[0-9a-f]{2}$", line)
    assert m and int(m.group(1)) >= 4, line


def test_detects_other_generator_in_decode_alone():
    """--only decode leaves step encode out, so the tool makes REF's chunks
    itself; DUT then rebuilds other bytes from them."""
    r = run_diff("--ref", "oracle", "--dut", "oracle", *profile(k=4, m=2),
                 "--ref-P", "technique=reed_sol_van",
                 "--dut-P", "technique=cauchy", "-s", "4096",
                 "--only", "decode")
    assert r.returncode == 1, r.stdout + r.stderr
    line = diff_line(r)
    assert "step=decode " in line, line
    assert re.search(r"shard=\d+ offset=\d+ ref=0x", line), line


def test_detects_other_geometry_in_shape():
    r = run_diff("--ref", "oracle", "--dut", "oracle",
                 *profile(technique="reed_sol_van", m=2),
                 "--ref-P", "k=4", "--dut-P", "k=5", "-s", "4096")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "step=shape " in diff_line(r)


def test_usage_errors_are_not_differences():
    """A bad command line or a plugin that cannot be made exits 2, never 0
    or 1."""
    assert run_diff("--ref", "oracle", "--dut", "oracle").returncode == 2
    r = run_diff("--ref", "oracle", "--dut", "no_such_plugin", "-s", "64")
    assert r.returncode == 2, r.stdout + r.stderr
    r = run_diff("--ref", "oracle", "--dut", "oracle", "-s", "64",
                 "--only", "no_such_step")
    assert r.returncode == 2
