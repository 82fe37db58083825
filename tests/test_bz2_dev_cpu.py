"""csrc/aqc_bunzip2_dev.hpp on the CPU (no GPU): the functions a lane of the device bunzip2 runs — block scan, entropy stage,
inverse BWT, RLE1 + CRC, chain — compiled with g++ and dealt out by plain loops (tests/native/bzb_selftest.cpp) through the
same stream walk that drives the kernels (csrc/aqc_bz2.hpp), over the inputs test_gpu_bunzip2.py gives the device.  Python's
bz2 module (fastq.py:25-26 upstream: bz2.BZ2File) is the oracle."""
import bz2
import os
import subprocess

import pytest

import bz2_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 30


def _build(tmp, flags):
    exe = os.path.join(tmp, "bzb_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "bzb_selftest.cpp"), "-ldl", "-o", exe])
    return exe


def _manifest(tmp):
    """every valid case with one window, the multi-block ones also in groups of 1 / 2 blocks, in windows that cut blocks short and
    with room for one block's text per group; the damaged ones"""
    lines = []

    def put(name, image, text, window, group, out_cap, want):
        p = os.path.join(tmp, "%s.%d.bz2" % (name, len(lines)))
        with open(p, "wb") as f:
            f.write(image)
        t = "-"
        if text is not None:
            t = p + ".txt"
            with open(t, "wb") as f:
                f.write(text)
        lines.append("%s %s %d %d %d %s" % (p, t, window, group, out_cap, want))
    for name, image, text in bz2_cases.valid_cases():
        assert bz2.decompress(image) == text, name
        put(name, image, text, BIG, 0, BIG, "exact")
    for name in ("fastq_level_1", "three_streams_and_an_empty_one"):
        _, image, text = bz2_cases.case(name)
        for group in (1, 2):
            put(name, image, text, BIG, group, BIG, "exact")
        put(name, image, text, 1 << 16, 3, BIG, "exact")        # (64 KiB windows: a level-1 block of FASTQ is ~25 KB — every window cuts one short)
        put(name, image, text, BIG, 4, 120_000, "exact")        # (text of one 100,000-byte block per group)
    for name, image in bz2_cases.damaged_cases():
        with pytest.raises((OSError, ValueError, EOFError)):
            bz2.decompress(image)
        put(name, image, None, BIG, 0, BIG, "error")
        put(name, image, None, 1 << 16, 1, BIG, "error")
    m = os.path.join(tmp, "manifest.txt")
    with open(m, "w") as f:
        f.write("\n".join(lines) + "\n")
    return m, len(lines)


def test_the_cases_cover_the_format_edges():
    """two to six Huffman tables, a full and a partial last selector group — read from the images themselves"""
    tables = {name: bz2_cases.first_block_tables(image) for name, image, text in bz2_cases.valid_cases() if text}
    assert {tables["letters_%d" % n] for n in (120, 420, 950, 1900, 6000)} == {2, 3, 4, 5, 6}, tables
    assert len(bz2_cases.block_starts(bz2_cases.case("fastq_level_9")[1])) == 1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_bunzip2_logic_on_the_cpu(tmp_path, flags):
    """byte-identical text with NO block handed back to libbz2 for every valid input (so the GPU test's cap of zero host blocks
    hides nothing), a negative status for every damaged one; once more as a stand-alone ASan / UBSan binary"""
    tmp = str(tmp_path)
    exe = _build(tmp, flags)
    manifest, n = _manifest(tmp)
    out = subprocess.run([exe, manifest], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all %d device-bunzip2 logic checks passed" % n in out.stdout, out.stdout[-3000:]
