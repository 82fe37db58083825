"""csrc/aqc_gzlz.hpp on the CPU (no GPU): the functions a lane of the level 6 - 9 gzip encoder runs — hash, insert, chain walk
with extension, token decision — compiled with g++ and dealt out by plain loops in the kernel's window order
(tests/native/gzlz_selftest.cpp) over the texts test_gpu_gzlz.py gives the device and a few raw ones.  For every text, member and
level the program checks every token (length 3 .. 258, distance 1 .. 32768 and inside the member, the copied bytes, the
tiling), encodes the members with aqcgz::build_codebook's code and has zlib inflate each one on its own."""
import os
import re
import subprocess
import zlib

import pytest

import gzlz_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "native", "gzlz_selftest.cpp"), os.path.join(ROOT, "afterqc_amd", "csrc", "aqc_deflate.cpp")]


def zlib_members(text, level):
    """bytes of the text as BGZF members of 0xff00 bytes made by zlib: raw deflate + 26 bytes each"""
    total = 0
    for o in range(0, len(text), gzlz_cases.MEMBER):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(text[o:o + gzlz_cases.MEMBER]) + c.flush()) + 26
    return total


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_lz_search_logic_on_the_cpu(tmp_path, flags):
    """every case at levels 6 - 9; once more as a stand-alone ASan / UBSan binary (every member in a heap block of exactly its
    size: a load past text + n is a report).  The deeper search is never worse by more than rounding on the real reads, and at
    depth 64 the members are smaller than zlib level 3's — the figure the GPU test asserts of the device."""
    tmp = str(tmp_path)
    exe = os.path.join(tmp, "gzlz_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-stringop-overflow"] + flags + SOURCES + ["-lz", "-pthread", "-o", exe])
    cases = gzlz_cases.cpu_cases()
    gzlz_cases.check_far_repeats(cases["far_repeats"])
    paths = []
    for name, text in cases.items():
        paths.append(os.path.join(tmp, name))
        with open(paths[-1], "wb") as f:
            f.write(text)
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    print(out.stdout[-8000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all %d gzlz logic checks passed" % len(cases) in out.stdout, out.stdout[-3000:]
    sizes = {}
    for line in out.stdout.splitlines():
        m = re.match(r"gzlz\| (\S+)\s+text\s+(\d+)\s+level 6\s+(\d+)\s+7\s+(\d+)\s+8\s+(\d+)\s+9\s+(\d+)", line)
        if m:
            sizes[os.path.basename(m.group(1))] = [int(x) for x in m.groups()[2:]]
    for name in ("real_R1", "real_R2", "far_repeats"):
        s = sizes[name]
        assert s[3] <= s[0], (name, s)
        assert s[3] <= zlib_members(cases[name], 3), (name, s, zlib_members(cases[name], 3))
    # the copy at distance 32768 is found, the one at 32769 must not be
    assert sizes["window_32768"][3] + 100 < sizes["window_32769"][3], (sizes["window_32768"], sizes["window_32769"])
