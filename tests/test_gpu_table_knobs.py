"""The LDS-table kernels (ec_gf_matmul_kernel, ec_gf_slices_kernel and their
*_multi forms) under their knobs. ECX_STREAM=0 sends the non-accumulating
batch calls back to ec_gf_matmul_kernel; ECX_NT and ECX_PF pick its
instances. The knobs are read once per process, so each setting is checked
in a child process of its own (that is what this test is about), bit-exact
against the numpy reference of test_gpu_stream_kernel.py. Run as a script,
this file is the child."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

KNOBS = [
    {"ECX_STREAM": "0"},
    {"ECX_STREAM": "0", "ECX_NT": "0"},
    {"ECX_STREAM": "0", "ECX_PF": "1"},
    {"ECX_STREAM": "0", "ECX_PF": "0"},
]
OWN = ("ECX_STREAM", "ECX_NT", "ECX_PF", "ECX_TILE")

POISON = 0xA5


def child():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import numpy as np

    import ceph_amd
    import oracle
    import decode_multi_cases as cases
    import test_gpu_stream_kernel as t

    def encoded(tech, k, m, S, C, seed):
        full = t.rand_batch(seed, S, k + m, C)
        t.ref_matmul(full, list(range(k)), list(range(k, k + m)),
                     oracle.matrix(tech, k, m)[k:])
        return full

    def encode_decode(k, m, S, C, erased, seed):
        want = encoded(t.TECH, k, m, S, C, seed)
        host = want.copy()
        host[:, k:, :] = POISON  # parity region pre-dirtied
        ctx = ceph_amd.EcContext(k, m, t.TECH, device=0)
        try:
            dev = t.Dev(ctx, host)
            ctx.encode_batch(dev.d, S, C)
            got = dev.get(host.shape)
            dev.free()
            assert np.array_equal(got, want), ("encode", k, m, S, C)
            if erased:
                t.check_decode(ctx, want, erased, S, C)
        finally:
            ctx.close()

    # a single vector; 257 vectors = a partial second tile
    encode_decode(4, 2, 3, 16, (1, 4), seed=1)
    encode_decode(4, 2, 3, 4112, (1, 4), seed=2)
    # NOUT = 4 on both legs: where auto-prefetch switches on
    encode_decode(5, 4, 3, 4112, (0, 2, 5, 8), seed=3)
    # output groups of 4 and 2
    encode_decode(4, 6, 3, 4112, None, seed=4)
    # 2048 stripes keep grid x at 1 with two tiles per chunk: the
    # grid-stride loop takes a second trip, a one-vector tail
    encode_decode(4, 2, 2048, 4112, None, seed=5)

    # apply_delta: the ACCUM instance, parity ^= gen[coding][data] * delta
    k, m, C = 4, 2, 4112
    rng = np.random.default_rng(6)
    delta = rng.integers(0, 256, C, dtype=np.uint8)
    parity = rng.integers(0, 256, C, dtype=np.uint8)
    coef = int(oracle.matrix(t.TECH, k, m)[k + 1][2])
    want = parity ^ t.mul_table()[coef][delta]
    ctx = ceph_amd.EcContext(k, m, t.TECH, device=0)
    try:
        got = ctx.apply_delta(delta, 2, k + 1, parity.copy())
    finally:
        ctx.close()
    assert np.array_equal(got, want), "apply_delta"

    # encode_slices: three sizes, one NULL (= zeros) data chunk whose device
    # bytes are poison and must be neither read nor written
    n = k + m
    sizes = [16, 4112, 16400]
    null_slice, null_chunk = 1, 2
    parts = []
    for i, sz in enumerate(sizes):
        buf = t.rand_batch(10 + i, 1, n, sz)
        if i == null_slice:
            buf[0, null_chunk] = 0
        t.ref_matmul(buf, list(range(k)), list(range(k, n)),
                     oracle.matrix(t.TECH, k, m)[k:])
        if i == null_slice:
            buf[0, null_chunk] = POISON
        parts.append(buf.reshape(-1))
    want = np.concatenate(parts)
    host = want.copy()
    off = 0
    for sz in sizes:
        host[off + k * sz:off + n * sz] = POISON
        off += n * sz
    ctx = ceph_amd.EcContext(k, m, t.TECH, device=0)
    try:
        dev = t.Dev(ctx, host)
        ptrs, off = [], 0
        for sz in sizes:
            ptrs += [dev.d.value + off + c * sz for c in range(n)]
            off += n * sz
        ptrs[null_slice * n + null_chunk] = None
        ctx.encode_slices(ptrs, sizes)
        ctx.sync()
        got = dev.get(host.shape)
        dev.free()
    finally:
        ctx.close()
    assert np.array_equal(got, want), "encode_slices"

    # decode_batch_multi: every 1-3 erasure pattern of (4,3), and the (4,6)
    # set whose 5 and 6 erasures need a second <= 4-output pass
    for tech, k, m, masks in (("reed_sol_van", 4, 3, cases.all_patterns_43()),
                              ("cauchy", 4, 6, cases.extra_passes_46())):
        S, C = len(masks), 4112
        want = encoded(tech, k, m, S, C, seed=20 + m)
        host = want.copy()
        for s, mk in enumerate(masks):
            for c in cases.erased_of(k + m, mk):
                host[s, c, :] = POISON
        ctx = ceph_amd.EcContext(k, m, tech, device=0)
        try:
            dev = t.Dev(ctx, host)
            ctx.decode_batch_multi(dev.d, S, C, masks)
            ctx.sync()
            got = dev.get(host.shape)
            dev.free()
        finally:
            ctx.close()
        assert np.array_equal(got, want), ("decode_batch_multi", tech, k, m)

    # decode_slices and decode_slices_multi over scattered arenas
    # (slices_cases.py), whole arena against the reference-encoded one:
    # (4,6) with a second launch, a NULL survivor, sizes 16 / 4112 / 16400
    import slices_cases as sc
    ctx = ceph_amd.EcContext(4, 6, "cauchy", device=0)
    try:
        arena, truth, mask = sc.knob_decode_case()
        dev = t.Dev(ctx, sc.erase(arena, truth, [mask] * arena.n))
        ctx.decode_slices(arena.ptrs(dev.d.value), arena.sizes, mask)
        ctx.sync()
        got = dev.get(truth.shape)
        dev.free()
        assert np.array_equal(got, truth), "decode_slices, scattered"
        arena, truth, masks = sc.knob_multi_case()
        dev = t.Dev(ctx, sc.erase(arena, truth, masks))
        ctx.decode_slices_multi(arena.ptrs(dev.d.value), arena.sizes, masks)
        ctx.sync()
        got = dev.get(truth.shape)
        dev.free()
        assert np.array_equal(got, truth), "decode_slices_multi, scattered"
    finally:
        ctx.close()
    print("KNOBS_OK")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS,
                         ids=lambda d: ",".join(f"{k}={v}"
                                                for k, v in d.items()))
def test_table_kernel_knob_setting(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith(OWN)}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KNOBS_OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    child()
