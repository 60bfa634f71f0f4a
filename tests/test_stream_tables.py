"""The streaming batch kernel's 3/3/2 table builder (ecx_gf8_tabs332_probe)
against the oracle's GF(2^8) product. CPU only."""
import numpy as np

import ceph_amd
import oracle


def _lookup(tabs, x):
    """What the kernel's three v_perm lookups XOR together for byte x."""
    b = tabs.view(np.uint8)  # little-endian byte order, 20 bytes
    return int(b[x & 7]) ^ int(b[8 + ((x >> 3) & 7)]) ^ int(b[16 + (x >> 6)])


def test_tabs332_all_products():
    for c in range(256):
        tabs = ceph_amd.gf8_tabs332_probe(c)
        assert tabs.shape == (5,) and tabs.dtype == np.uint32
        for x in range(256):
            assert _lookup(tabs, x) == oracle.gf_mul(c, x), (c, x)


def test_tabs332_zero_coefficient():
    assert not ceph_amd.gf8_tabs332_probe(0).any()
