"""-m gpu: the device gunzip's KERNELS (csrc/aqc_gunzip_dev.hpp) held to zlib and to their CPU emulation, case by case
(tests/gz_in_cases.py), through capi.gunzip_probe: one group and one resolve with DeviceInflate's own launch sequence, the
budgets the case names and no second attempt.

Whole files through aqc_gunzip_dev (test_gpu_pipe.py) come out right whatever the kernels do, because every block the device
fails goes back to the host.  Here nothing goes back: the text, every section's CRC-32, the line feeds per 64 KiB piece and the
tail window are compared with zlib's and numpy's, and found / start_bit / end_bit / n_sym of every section must EQUAL what the
emulation (engine 0) returns for the same call — a block the kernels fail but the plain loops decode is a shorter or a missing
section.  test_gunzip_cases_cpu.py checks, without a GPU, that the emulation finds every section a case says must be found."""
import pytest

import gz_in_cases
from afterqc_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", gz_in_cases.names())
def test_kernels_against_zlib_and_the_emulation(name):
    c = gz_in_cases.case(name)
    ref = gz_in_cases.probe(c, 0)
    try:
        got = gz_in_cases.probe(c, 1)
    except capi.AqcError as e:
        # (a HIP error, not a wrong answer: nothing more is started on a device that may have faulted)
        pytest.exit("the device gunzip failed on the GPU in case %s: %s" % (name, e), returncode=1)
    for key in ("found", "start_bit", "end_bit", "n_sym", "run", "status"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    gz_in_cases.check(c, got)
    for key in ("crc", "piece_nl", "text", "tail"):
        assert got[key] == ref[key], key
