#!/usr/bin/env python3
"""device bunzip2 timing: python tools/gpu_bunzip2_dev.py [reads] [dir]

One config-3 style R1 file of `reads` reads (default 2 M), compressed once with the `bzip2` program (one stream), then
  A  aqc_bunzip2_dev on the file image, three times in one process (the first cold, the others warm): text rate and the
     per-stage microseconds from `stats`;
  B  the yardstick — libbz2 on one thread, the pipe's Bz2Source without a device decoder (the parent commit's path);
  C  the CLI's pass 2 (tools/e2e_bench.py --single --bz2), a fresh process per run, device (AQC_BZ2_DEVICE_IN=1) and host
     (AQC_BZ2_DEVICE_IN=0) interleaved, three times each."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["AQC_BZ2_DEBUG"] = "1"          # aqc_bunzip2_dev prints the BWT stage's parts (scatter / chase / sizes) on stderr
from afterqc_amd import capi  # noqa: E402

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/aqc_bz2"
bench = [sys.executable, os.path.join(ROOT, "tools", "e2e_bench.py"), "--single", "--bz2", "--pairs", str(reads), "--keep", "--dir", work]


def cli(tag, device, reuse=True):
    env = dict(os.environ, AQC_BZ2_DEVICE_IN="1" if device else "0")
    out = subprocess.run(bench + (["--reuse"] if reuse else []), env=env, capture_output=True, text=True)
    for ln in out.stdout.splitlines():
        if ln.startswith('{"mode"'):
            d = json.loads(ln)
            print("C  %-34s pass2 %.3f s = %.3f Mreads/s, wall %.3f s, cores busy %.1f, used_pipe %s" % (tag, d["pass2_s"], d["pass2_mreads_s"], d["wall_s"], d["pass2_cores_busy"], d["used_pipe"]), flush=True)
            return d
    print("C  %s: no result\n%s" % (tag, out.stderr[-2000:]), flush=True)
    return None


cli("host (makes the file: warm-up)", False, reuse=False)
path = os.path.join(work, "R1.fq.bz2")
image = open(path, "rb").read()
print("input: %d reads, %.1f MB of .bz2 (bzip2 program, one stream)" % (reads, len(image) / 1e6), flush=True)

# B: libbz2, one thread
t0 = time.perf_counter()
src = capi.NativeSource(path, 2, io_threads=4)
buf = bytearray(64 << 20)
total = 0
while True:
    k = src.readinto(buf)
    total += k
    if k < len(buf):
        break
src.close()
dt = time.perf_counter() - t0
print("B  libbz2, one thread (Bz2Source without a device): %.1f MB of text in %.2f s = %.1f MB/s" % (total / 1e6, dt, total / dt / 1e6), flush=True)

# A: the device
lib = capi.load_library()
arr = np.frombuffer(image, dtype=np.uint8)
out = np.zeros(total + 4096, dtype=np.uint8)
n_out = capi.C.c_uint64(0)
stats = np.zeros(8, dtype=np.uint64)
for rep in range(3):
    t0 = time.perf_counter()
    rc = lib.aqc_bunzip2_dev(0, arr.ctypes.data, len(image), out.ctypes.data, out.size, capi.C.byref(n_out), stats.ctypes.data, 1, 0)
    dt = time.perf_counter() - t0
    print("A  aqc_bunzip2_dev %s: rc %d, %d bytes (%s) in %.3f s = %.1f MB/s of text; blocks device %d host %d; ms: scan %.1f entropy %.1f BWT (its parts: the line above) %.1f expand + CRC %.1f copies %.1f" % (
        "cold" if rep == 0 else "warm", rc, n_out.value, "as many as libbz2" if n_out.value == total else "libbz2: %d" % total, dt, n_out.value / dt / 1e6, stats[0], stats[1],
        stats[3] / 1e3, stats[4] / 1e3, stats[5] / 1e3, stats[6] / 1e3, stats[7] / 1e3), flush=True)

for k in range(3):
    cli("device (AQC_BZ2_DEVICE_IN=1)", True)
    cli("host   (AQC_BZ2_DEVICE_IN=0)", False)
