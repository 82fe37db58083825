"""csrc/aqc_keep.hpp, the keeper of the device decoders of .gz and .bz2 input, without a device: tests/native/keep_selftest.cpp as
a stand-alone program, plain and under ASan / UBSan (LeakSanitizer with it: what is kept is never freed, and is reachable)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_keeper_on_the_cpu(tmp_path, flags):
    """take / give / lend, every field of a gunzip decoder's key, the cap of 16, eight threads on four keys — and an atexit handler
    that runs after every static destructor finds no kept payload destroyed"""
    exe = os.path.join(str(tmp_path), "keep_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread"] + flags + [os.path.join(ROOT, "tests", "native", "keep_selftest.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k not in ("AQC_GZ_RESIDENT", "AQC_GZ_RATIO", "AQC_GZ_TOK_RATIO")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "FAIL" not in out.stdout and "FAIL" not in out.stderr, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all keeper checks passed" in out.stdout, out.stdout[-3000:]
    assert out.stdout.rstrip().endswith("at exit: no kept payload was destroyed"), out.stdout[-3000:]
    assert "LeakSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
