"""The bitmatrix kernels under their knobs. In the launcher's bit_plan(),
ECX_BITREG, ECX_BITPIPE, ECX_BITT, ECX_BITW, ECX_BITQ and ECX_BITXCD (and, as
launch arguments, ECX_BITSTAGGER and ECX_NT) select kernels, template
instances and block mappings: the
register kernel's NR = 16/24/32 instances and the whole of
ec_bitmatrix_pipe_kernel are reached only through them. The knobs are read
once per process, so each setting is checked in a child process of its own
(that is what this test is about), bit-exact against bitmatrix_cases.ref_bit
in the guarded form of test_gpu_bitmatrix_kernel.py. Every child runs all of
bitmatrix_cases.KNOB_ENCODES / KNOB_DECODES / KNOB_DELTAS;
test_kernel_references.py derives which instance each setting reaches and
holds that derivation against the launcher's own plan. No
setting needs more than 64 KiB of dynamic LDS. Run as a script, this file is
the child."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
import bitmatrix_cases as cases  # noqa: E402

OWN = ("ECX_BIT", "ECX_NT")


def child():
    import ceph_amd
    import test_gpu_bitmatrix_kernel as t

    for tech, k, m, pkt, n_sw, S in cases.KNOB_ENCODES:
        ctx = ceph_amd.EcContext(k, m, tech, device=0, packetsize=pkt)
        try:
            t.check_encode(ctx, cases.encoded_bit(tech, k, m, pkt, n_sw, S),
                           k, ("encode", tech, k, m, pkt, n_sw, S))
        finally:
            ctx.close()
    for tech, k, m, pkt, n_sw, S, erased in cases.KNOB_DECODES:
        ctx = ceph_amd.EcContext(k, m, tech, device=0, packetsize=pkt)
        try:
            t.check_decode(ctx, cases.encoded_bit(tech, k, m, pkt, n_sw, S),
                           erased, ("decode", tech, k, m, pkt, n_sw, S))
        finally:
            ctx.close()
    k, m = 3, 3
    rows = cases.encode_rows(t.ORIG, k, m)
    for pkt, n_sw, data, coding in cases.KNOB_DELTAS:
        ctx = ceph_amd.EcContext(k, m, t.ORIG, device=0, packetsize=pkt)
        try:
            t.check_delta(ctx, rows, k, pkt, n_sw, data, coding,
                          seed=pkt + data + coding)
        finally:
            ctx.close()
    print("BITKNOBS_OK")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", cases.KNOBS,
                         ids=lambda d: ",".join(f"{k}={v}"
                                                for k, v in d.items()))
def test_bitmatrix_knob_setting(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith(OWN)}
    env.update(knobs)
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BITKNOBS_OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    child()
