"""Every ErasureCodeInterface method of the GPU plugins against the CPU
oracle plugin, through ec_plugin_diff (ceph_amd/harness/ec_plugin_diff.cc):
the same bytes go to both plugins, and return code, key set and bytes of
every call must agree. This is the boundary Ceph calls; the C ABI under it
is covered by test_gpu_hostpath.py and the kernel files.

Each test is one process with one plugin instance per side, so encode,
decode, delta and their repeats share the instance's resident launch
params, decode-plan cache and captured graphs. The widths put the chunk
size C on the switch points of the host-pointer stagers; the tool prints
the C of every width and each test checks it is the C its comment claims.
tests/PLUGIN_DIFF_COVERAGE.md has the table of what reaches which stager."""
import os
import re

import pytest

from test_plugin_diff import STEPS, assert_passed, run_diff, steps_of

pytestmark = pytest.mark.gpu

# staging knobs are read once per process: strip them all, then set one
OWN = ("ECX_HOSTPIPE", "ECX_HPIPE_", "ECX_HGRAPH", "ECX_SPINWAIT",
       "ECX_STREAM", "ECX_NT", "ECX_PF")


def child_env(knob=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith(OWN)}
    env.update(knob or {})
    return env


def P(**kv):
    return [a for k, v in kv.items() for a in ("-P", f"{k}={v}")]


# Chunk sizes on the switch points of pipelined_matmul_host (w=8 table
# techniques): 32 = smallest chunk; 4128 = 257 16-byte vectors + a 32-byte
# tail; 131072 = last size replayed as a captured graph (ECX_HGRAPH_MAX,
# inclusive); 131104 = first size on the plain single-tile path.
ISA_K4 = {1: 32, 4 * 4128: 4128, 4 * 131072: 131072, 4 * 131072 + 1: 131104}
ISA_K5 = {1: 32, 5 * 4128: 4128, 5 * 131072: 131072, 5 * 131072 + 1: 131104}
# jerasure w=8: stripe padded to k*w*4 = 192, so C is a multiple of 32 too
JER_K6 = {1: 32, 6 * 4128: 4128, 6 * 131072: 131072, 6 * 131072 + 1: 131104}
# jerasure w=16: stripe padded to k*w*4 = 256, C a multiple of 64. One
# stager (single-shot pinned) at every size: smallest, odd multiple, 128 KiB
W16_K4 = {1: 64, 4 * 4160: 4160, 4 * 131072: 131072, 4 * 131072 + 1: 131136}
# bitmatrix at packetsize 32: C a multiple of w*packetsize*4 = 1024. Same
# single-shot stager; one, five and 128 superword groups, and one more
BIT_K4 = {1: 1024, 4 * 5120: 5120, 4 * 131072: 131072, 4 * 131072 + 1: 132096}
# clay 4+2 d=5: 8 sub-chunks of a multiple of 32, the sub-chunk is what the
# scalar codec sees: 32, 4128 and 16384 bytes
CLAY = {1: 256, 4 * 8 * 4128: 8 * 4128, 4 * 8 * 16384: 8 * 16384}

RS42 = P(technique="reed_sol_van", k=4, m=2)
RS46 = P(technique="reed_sol_van", k=4, m=6)
CORIG = P(technique="cauchy_orig", k=4, m=2, packetsize=32)

# id -> (ref plugin, dut plugin, tool args, {width: C}, allowed skips)
PROFILES = {
    "reed_sol_van_4_2": ("oracle", "mi355x", RS42, ISA_K4, ()),
    "cauchy_5_3": ("oracle", "mi355x", P(technique="cauchy", k=5, m=3),
                   ISA_K5, ()),
    # two output groups on every host call: two kernels in one captured
    # graph; decode of 5 and 6 erasures
    "reed_sol_van_4_6": ("oracle", "mi355x", RS46, ISA_K4, ()),
    "jerasure_6_2": ("oracle", "mi355x",
                     P(technique="jerasure_reed_sol_van", k=6, m=2),
                     JER_K6, ()),
    "jerasure_w16_4_3": ("oracle", "mi355x",
                         P(technique="jerasure_reed_sol_van", w=16, k=4, m=3),
                         W16_K4, ()),
    "reed_sol_r6_op_5_2": ("oracle", "mi355x",
                           P(technique="reed_sol_r6_op", k=5, m=2),
                           ISA_K5, ()),
    "cauchy_orig_4_2": ("oracle", "mi355x", CORIG, BIT_K4, ()),
    "cauchy_good_4_3": ("oracle", "mi355x",
                        P(technique="cauchy_good", k=4, m=3, packetsize=32),
                        BIT_K4, ()),
    # the layer logic is the same code on both sides; the sub-plugins differ.
    # lrc and clay claim no parity delta
    "lrc_4_2_3": ("lrc", "lrc",
                  P(k=4, m=2, l=3) + ["--ref-P", "lrc-default-plugin=oracle",
                                      "--dut-P", "lrc-default-plugin=mi355x"],
                  ISA_K4, ("delta",)),
    "clay_4_2_5": ("clay", "clay",
                   P(k=4, m=2, d=5) + ["--ref-P", "scalar_mds=oracle",
                                       "--dut-P", "scalar_mds=mi355x"],
                   CLAY, ("delta",)),
}

# C = 3 * 16384 + 32 under ECX_HPIPE_TILE=16384: four tiles, the last 32
# bytes, both pinned buffers reused, two groups per tile at m = 6
TILED = {4 * 49184: 49184}
# three widths of the default list: smallest, odd, graph/plain switch
SHORT_ISA = {w: ISA_K4[w] for w in (1, 4 * 4128, 4 * 131072)}
SHORT_BIT = {w: BIT_K4[w] for w in (1, 4 * 5120, 4 * 131072)}
# (k + m) * C = 6 * 175104 > ECX_HPIPE_MAX=1048576: per-chunk copies
OVER_MAX = {4 * 175104: 175104}

# id -> (profile args, {width: C}, knob)
KNOBS = {
    "tile-rs42": (RS42, TILED, {"ECX_HPIPE_TILE": "16384"}),
    "tile-rs46": (RS46, TILED, {"ECX_HPIPE_TILE": "16384"}),
    "nograph-rs42": (RS42, SHORT_ISA, {"ECX_HGRAPH": "0"}),
    "nograph-rs46": (RS46, SHORT_ISA, {"ECX_HGRAPH": "0"}),
    "nograph-corig": (CORIG, SHORT_BIT, {"ECX_HGRAPH": "0"}),
    "legacy-rs42": (RS42, SHORT_ISA, {"ECX_HOSTPIPE": "0"}),
    "legacy-rs46": (RS46, SHORT_ISA, {"ECX_HOSTPIPE": "0"}),
    "legacy-corig": (CORIG, SHORT_BIT, {"ECX_HOSTPIPE": "0"}),
    "pipemax-corig": (CORIG, OVER_MAX, {"ECX_HPIPE_MAX": "1048576"}),
    "nostream-rs42": (RS42, SHORT_ISA, {"ECX_STREAM": "0"}),
    "nostream-rs46": (RS46, SHORT_ISA, {"ECX_STREAM": "0"}),
    "nostream-corig": (CORIG, SHORT_BIT, {"ECX_STREAM": "0"}),
}


def width_args(chunks):
    return [a for w in chunks for a in ("-s", str(w))]


def check(r, chunks, allowed_skips=(), steps=STEPS):
    assert_passed(r, allowed_skips, steps)
    got = {int(w): int(c) for w, c in
           re.findall(r"^WIDTH (\d+) chunk=(\d+)$", r.stdout, re.M)}
    assert got == chunks, "the widths miss the chunk sizes they are there for"
    assert "refused" not in r.stderr, r.stderr


@pytest.mark.parametrize("case", sorted(PROFILES))
def test_plugin_matches_oracle(case):
    ref, dut, args, chunks, skips = PROFILES[case]
    r = run_diff("--ref", ref, "--dut", dut, *args, *width_args(chunks),
                 env=child_env())
    check(r, chunks, skips)
    for step in skips:
        assert steps_of(r.stdout)[step][0] == "skipped"


@pytest.mark.parametrize("case", sorted(KNOBS))
def test_plugin_matches_oracle_under_knob(case):
    args, chunks, knob = KNOBS[case]
    r = run_diff("--ref", "oracle", "--dut", "mi355x", *args,
                 *width_args(chunks), env=child_env(knob))
    check(r, chunks)


# largest chunk first, so that the pinned staging buffer never has to grow
# at the smaller ones (growing it drops every captured graph)
LARGE_FIRST = {4 * 131072: 131072, 4 * 4128: 4128, 1: 32}
# id -> (profile args, {width: C})
DECODE_FIRST = {"rs42": (RS42, LARGE_FIRST), "rs46": (RS46, LARGE_FIRST)}


@pytest.mark.parametrize("case", sorted(DECODE_FIRST))
def test_decode_first_on_a_fresh_instance(case):
    """--only decode, widths descending: at the two smaller chunk sizes the
    first host calls the GPU plugin sees are one-erasure decodes into a
    staging buffer that is already large enough, so each stream slot
    captures its graph for one output and the calls after it need more (2,
    then up to m). In the full run every slot meets the m-output encode
    first, and a graph captured for more outputs than a call needs still
    gives the right bytes; with ascending widths the staging buffer grows
    with the output count and takes the captured graphs with it. A graph
    cache that forgot the output count passes both, and fails here."""
    args, chunks = DECODE_FIRST[case]
    r = run_diff("--ref", "oracle", "--dut", "mi355x", *args,
                 *width_args(chunks), "--only", "decode", env=child_env())
    check(r, chunks, steps=("shape", "decode"))


def test_shec_delta_matches_its_own_reencode():
    """shec has no CPU twin at this boundary (its encode bytes are pinned
    by test_shec_encode_parity_vs_oracle): the delta-updated parity must
    equal shec's own encode_chunks of the new data."""
    chunks = {1: 32, 4 * 4128: 4128, 4 * 131072: 131072}
    r = run_diff("--ref", "shec", "--dut", "shec", *P(k=4, m=3, c=2),
                 *width_args(chunks), "--only", "delta",
                 "--delta-vs-reencode", env=child_env())
    check(r, chunks, steps=("shape", "delta"))
