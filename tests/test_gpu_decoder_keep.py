"""-m gpu: the device decoders of .gz and .bz2 input are kept for the life of the process (csrc/aqc_keep.hpp) and NOT destroyed
when it ends — no HIP call from a static destructor at exit() — and a kept decoder goes only to somebody who asks with the options
it was built with.  Each test is one fresh child process that decodes, then falls off the end of its script: a normal interpreter
shutdown with kept decoders alive.  The parent asserts a clean exit (status 0, no `tear-down:` line — what ~DeviceInflate prints
under AQC_GZ_DEBUG=1 — and no HIP error, terminate or abort text on stderr) and that the bytes are right."""
import bz2
import json
import os
import subprocess
import sys
import zlib

import pytest

import bz2_cases
from afterqc_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


def run_child(script, *args, env=None):
    """one fresh process: its last stdout line as JSON, its stderr; the clean-exit assertions every child is held to"""
    e = dict(os.environ)
    for k in ("AQC_GZ_RESIDENT", "AQC_GZ_RATIO", "AQC_GZ_TOK_RATIO", "AQC_GZ_GROUP", "AQC_GZ_DEVICE_MIN", "AQC_GZ_DEVICE_IN"):
        e.pop(k, None)
    e.update({"AQC_GZ_DEBUG": "1", "AQC_PIPE_DEBUG": "1"})
    e.update(env or {})
    out = subprocess.run([sys.executable, "-c", script, ROOT, TESTS] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=e)
    tail = out.stdout[-2000:] + out.stderr[-6000:]
    assert out.returncode == 0, tail
    assert "tear-down:" not in out.stderr, tail                  # a kept decoder is never destroyed
    for bad in ("HIP error", "hipError", "HSA_STATUS", "terminate", "Aborted", "Segmentation", "Traceback"):
        assert bad not in out.stderr, (bad, tail)
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


_HEAD = r"""
import hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from afterqc_amd import capi
"""

_GUNZIP = _HEAD + r"""
gz = open(sys.argv[3], "rb").read()
cap = int(sys.argv[4])
lib = capi.load_library()
src = np.frombuffer(gz, dtype=np.uint8)
res = []
for group in (1 << 20, 1 << 20, 512 << 10):
    out = np.zeros(cap, dtype=np.uint8)
    n_out = capi.C.c_uint64(0)
    stats = np.zeros(8, dtype=np.uint64)
    rc = lib.aqc_gunzip_dev(0, src.ctypes.data, len(gz), out.ctypes.data, out.size, capi.C.byref(n_out), stats.ctypes.data, 4, 64 << 10, group)
    res.append({"rc": rc, "error": (lib.aqc_last_error() or b"").decode() if rc else "", "n": int(n_out.value),
                "sha": hashlib.sha256(out[:n_out.value].tobytes()).hexdigest(), "stats": [int(x) for x in stats]})
print(json.dumps(res))
"""


def test_gunzip_seam_keeps_its_decoders_past_the_end_of_the_process(tmp_path):
    """aqc_gunzip_dev on the input of test_device_gunzip_sections_are_exact (level 6): twice with groups of 1 MiB, once with groups
    of 512 KiB — exact each time, the device supplying sections each time — and the process ends with its decoders alive"""
    d = synth.make_pairs(9000, 150, seed=46, dirty=True)
    buf, n = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    text = bytes(memoryview(buf)[:n])
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_DEFAULT_STRATEGY)
    p = str(tmp_path / "in.gz")
    with open(p, "wb") as f:
        f.write(c.compress(text) + c.flush())
    res, err = run_child(_GUNZIP, p, len(text) + 4096)
    import hashlib
    want = hashlib.sha256(text).hexdigest()
    assert len(res) == 3
    for r in res:
        assert r["rc"] == 0, r
        assert r["n"] == len(text) and r["sha"] == want, r
        assert r["stats"][0] >= 1, r


_BUNZIP2 = _HEAD + r"""
import bz2_cases
_, image, text = bz2_cases.case("fastq_level_1")
res = []
for _ in range(2):
    got, stats = capi.bunzip2_dev(image, len(text) + 4096)
    res.append({"sha": hashlib.sha256(got).hexdigest(), "n": len(got), "stats": [int(x) for x in stats]})
print(json.dumps(res))
"""


def test_bunzip2_seam_keeps_its_decoder_past_the_end_of_the_process():
    """capi.bunzip2_dev on fastq_level_1 twice: bz2.decompress's text both times, no block handed back, a clean exit"""
    import hashlib
    _, image, text = bz2_cases.case("fastq_level_1")
    assert bz2.decompress(image) == text
    res, err = run_child(_BUNZIP2)
    assert len(res) == 2
    for r in res:
        assert r["n"] == len(text) and r["sha"] == hashlib.sha256(text).hexdigest(), r
        assert r["stats"][0] >= 1 and r["stats"][1] == 0 and r["stats"][2] == 0, r


_PIPE = _HEAD + r"""
import gzip
from afterqc_amd import after, preprocesser
work, r1, r2 = sys.argv[3:6]

def run(tag, a, b):
    out = os.path.join(work, tag)
    argv = ["-1", a, "-2", b, "-f", "0", "-t", "0", "-g", os.path.join(out, "good"), "-b", os.path.join(out, "bad"), "-r", os.path.join(out, "QC")]
    options, _ = after.parseCommand(argv)
    after.finalize_options(options)
    options.barcode = False
    sys.stderr.write("RUN %s\n" % tag)
    sys.stderr.flush()
    flt = preprocesser.seqFilter(options, use_pipe=True, devices=[0])
    flt.run()
    files = {}
    for sub in ("good", "bad"):
        for fn in sorted(os.listdir(os.path.join(out, sub))):
            with (gzip.open if fn.endswith(".gz") else open)(os.path.join(out, sub, fn), "rb") as f:
                files[sub + "/" + (fn[:-3] if fn.endswith(".gz") else fn)] = hashlib.sha256(f.read()).hexdigest()
    return {"used_pipe": bool(flt.used_pipe), "files": files}

res = [run("plain", r1, r2), run("gz1", r1 + ".gz", r2 + ".gz"), run("gz2", r1 + ".gz", r2 + ".gz")]
os.environ["AQC_GZ_RESIDENT"] = "0"
res.append(run("gz3", r1 + ".gz", r2 + ".gz"))
print(json.dumps(res))
"""


def test_pipe_takes_a_kept_decoder_only_in_the_mode_it_asks_for(tmp_path):
    """two .gz mates (gzip level 6) through seqFilter(use_pipe=True) three times in one process, a pipe each: the first run makes a
    decoder per file, the second takes them warm from the keeper, the third — AQC_GZ_RESIDENT=0 set in between — asks for another
    mode and gets new ones, not the resident ones the keeper holds.  Outputs of all three: those of the plain files."""
    import gzip
    work = str(tmp_path)
    d = synth.make_pairs(20000, 150, seed=8822, dirty=True)
    r1, r2 = os.path.join(work, "R1.fq"), os.path.join(work, "R2.fq")
    synth.write_fastq_fixed(r1, d["seq1"], d["qual1"], 1)
    synth.write_fastq_fixed(r2, d["seq2"], d["qual2"], 2)
    for p in (r1, r2):
        with open(p, "rb") as f, gzip.open(p + ".gz", "wb", compresslevel=6) as g:
            g.write(f.read())
    res, err = run_child(_PIPE, work, r1, r2, env={"AQC_GZ_DEVICE_MIN": "0", "AQC_GZ_GROUP": "4194304"})
    plain, runs = res[0], res[1:]
    assert plain["used_pipe"] and len(plain["files"]) >= 4, plain
    for r in runs:
        assert r["used_pipe"]
        assert r["files"] == plain["files"]
    # the take lines of each run: "pipe: input <f> takes its gunzip decoder on device 0: new | warm from the keeper"
    takes = {}
    tag = None
    for line in err.splitlines():
        if line.startswith("RUN "):
            tag = line[4:].strip()
        elif "takes its gunzip decoder" in line:
            takes.setdefault(tag, {})[int(line.split("input")[1].split()[0])] = line.rsplit(":", 1)[1].strip().split()[0]
    print(takes)
    assert "plain" not in takes
    assert takes["gz1"] == {0: "new", 1: "new"}, takes
    assert takes["gz2"] == {0: "warm", 1: "warm"}, takes
    assert takes["gz3"] == {0: "new", 1: "new"}, takes
