"""The device gunzip's cases (tests/gz_in_cases.py) on the CPU emulation of its kernels (capi.gunzip_probe, engine 0:
csrc/aqc_gunzip_ref.hpp deals the kernels' per-lane functions out with plain loops; no GPU).  Every case is ONE group and ONE
resolve with the budgets the kernels get: the text is zlib's, each section's CRC-32 is zlib.crc32's, the line feeds per 64 KiB
piece are numpy's count, the tail window is the last 32 KiB of window + text — and every section a case says must be found IS
found and chains to the next.  That last point is what test_gpu_gunzip.py leans on: it holds the kernels to this emulation
section by section, so no case may pass there by leaving a section to the host."""
import pytest

import gz_in_cases


@pytest.mark.parametrize("name", gz_in_cases.names())
def test_emulation_against_zlib(name):
    c = gz_in_cases.case(name)
    gz_in_cases.check(c, gz_in_cases.probe(c, 0))


def test_the_cases_cover_what_they_claim():
    """a case's own premises: the hand-made member that zlib must reject is the only invalid one, every other text is zlib's
    (checked when the case is made), and the section tables stay within one group of about 1 MB"""
    for name in gz_in_cases.names():
        c = gz_in_cases.case(name)
        assert c.valid == (name != "marker_into_the_void"), name
        assert len(c.text) <= 1300000 and len(c.image) <= 1300000, name
        assert c.nominal == sorted(c.nominal) and all(a <= b for a, b in zip(c.nominal, c.stop)), name
