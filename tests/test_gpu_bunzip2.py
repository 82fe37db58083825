"""-m gpu: .bz2 input decoded on the device, one bzip2 block at a time (csrc/aqc_bunzip2_dev.hpp through aqc_bunzip2_dev and
through the pipe's Bz2Source) — byte for byte what Python's bz2 module (fastq.py:25-26 upstream: bz2.BZ2File) makes of the same
file, with no block handed back to libbz2 for a valid input; damaged input is an error, never text and never a hang.  The
inputs are those libbz2's encoder writes (valid_cases, damaged_cases) and those it never does (crafted_cases)."""
import bz2
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bz2_cases
from afterqc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c[0] for c in bz2_cases.valid_cases()])
def test_device_bunzip2_is_exact(name):
    """every edge of the format (tests/bz2_cases.py): exactly bz2.decompress(data), zero blocks decoded on the host"""
    _, image, text = bz2_cases.case(name)
    assert bz2.decompress(image) == text
    got, stats = capi.bunzip2_dev(image, len(text) + 4096)
    assert len(got) == len(text) and got == text, (name, len(got), len(text))
    assert stats[1] == 0 and stats[2] == 0, stats
    if text:
        assert stats[0] >= 1, stats


@pytest.mark.parametrize("group_blocks", [0, 1, 2])
def test_four_blocks_at_unaligned_bits_in_groups(group_blocks):
    """350 KB of FASTQ at level 1 — four blocks, at bit positions that are no multiple of 8 — in one group and in groups of one
    and two blocks, whose text is stitched in stream order"""
    _, image, text = bz2_cases.case("fastq_level_1")
    starts = bz2_cases.block_starts(image)
    assert len(starts) == 4 and any(s % 8 for s in starts), starts
    got, stats = capi.bunzip2_dev(image, len(text) + 4096, group_blocks=group_blocks)
    assert got == text
    assert stats[0] == 4 and stats[1] == 0 and stats[2] == 0, stats


def test_output_that_does_not_fit_is_an_error():
    _, image, text = bz2_cases.case("fastq_level_9")
    with pytest.raises(capi.AqcError):
        capi.bunzip2_dev(image, len(text) - 1)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from afterqc_amd import capi
data = open(sys.argv[2], "rb").read()
try:
    text, stats = capi.bunzip2_dev(data, int(sys.argv[3]), group_blocks=int(sys.argv[4]) if len(sys.argv) > 4 else 0)
except capi.AqcError as e:
    print("ERROR %d" % e.code)
else:
    print("TEXT %d" % len(text))
"""


@pytest.mark.parametrize("name", [c[0] for c in bz2_cases.damaged_cases()])
def test_damaged_input_is_an_error_in_bounded_time(tmp_path, name):
    """a flipped bit in a block, the file cut at two thirds, a flipped bit in the trailer's CRC: a negative status within the
    time limit (every kernel loop is bounded by the block size or the window's bits), never text.  In a child process."""
    image = dict(bz2_cases.damaged_cases())[name]
    with pytest.raises((OSError, ValueError, EOFError)):
        bz2.decompress(image)
    p = str(tmp_path / "damaged.bz2")
    with open(p, "wb") as f:
        f.write(image)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, p, str(1 << 20)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().startswith("ERROR -"), out.stdout[-2000:] + out.stderr[-2000:]


def _crafted_runs():
    """(name, group_blocks): every crafted case in one group, those of several blocks also in groups of one block; the stream of
    65,537 blocks in groups of 256 (130 MB of group buffers at level 1, where the default group would take 1.7 GB)"""
    runs = []
    for name, image, cls in bz2_cases.crafted_cases():
        if name == "blocks_65537_one_byte_each":
            runs.append((name, 256))
            continue
        runs.append((name, 0))
        if len(bz2_cases.magic_hits(image, bz2_cases.BLOCK_MAGIC)) > 1 and name != "stream_then_70000_block_magics":
            runs.append((name, 1))
    return runs


@pytest.mark.parametrize("name,group_blocks", _crafted_runs())
def test_crafted_streams_as_libbz2_reads_them(tmp_path, name, group_blocks):
    """legal corners of the format that libbz2's encoder never writes, and a few illegal ones (tests/bz2_cases.py: crafted_cases,
    written with tests/bz2_writer.py; every one of them has passed the CPU emulation, plain and under ASan / UBSan, in
    test_bz2_dev_cpu.py).  Python's bz2 rules: where it raises, so does the device (in a child process, within the time limit);
    where it returns text, the device returns that text — with every block decoded on the device and none on the host (exact),
    or with libbz2 finishing the stream (handback)"""
    _, image, cls, dev_blocks = bz2_cases.crafted_case(name)
    try:
        text = bz2.decompress(image)
    except (OSError, ValueError, EOFError):
        text = None
    assert (text is None) == (cls == "error"), (name, cls)
    if text is None:
        p = str(tmp_path / "crafted.bz2")
        with open(p, "wb") as f:
            f.write(image)
        out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, p, str(1 << 20), str(group_blocks)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert out.stdout.strip().startswith("ERROR -"), out.stdout[-2000:] + out.stderr[-2000:]
        return
    t0 = time.perf_counter()
    got, stats = capi.bunzip2_dev(image, len(text) + 4096, group_blocks=group_blocks)
    print("%s, groups of %d: %.2f s, stats %s" % (name, group_blocks, time.perf_counter() - t0, [int(x) for x in stats[:3]]))
    assert len(got) == len(text) and got == text, (name, len(got), len(text))
    assert stats[0] == dev_blocks, (name, stats)
    if cls == "exact":
        assert stats[1] == 0 and stats[2] == 0, (name, stats)
    else:
        assert cls == "handback" and stats[1] >= 1, (name, stats)


_PIPE_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, sys.argv[1])
work = sys.argv[2]
from afterqc_amd import after, capi, preprocesser

def run(tag, r1, r2):
    out = os.path.join(work, tag)
    argv = ["-1", r1, "-2", r2, "-f", "0", "-t", "0", "-g", os.path.join(out, "good"), "-b", os.path.join(out, "bad"), "-r", os.path.join(out, "QC")]
    options, _ = after.parseCommand(argv)
    after.finalize_options(options)
    options.barcode = False
    before = capi.bz2_input_stats()
    flt = preprocesser.seqFilter(options, use_pipe=True, devices=[0])
    stat = json.loads(json.dumps(flt.run()))
    delta = [a - b for a, b in zip(capi.bz2_input_stats(), before)]
    files = {}
    for sub in ("good", "bad"):
        for fn in sorted(os.listdir(os.path.join(out, sub))):
            with open(os.path.join(out, sub, fn), "rb") as f:
                files[sub + "/" + fn.replace(".bz2", "")] = hashlib.sha256(f.read()).hexdigest()       # (R1.bz2.good.fq / R1.good.fq)
    stat.pop("command", None)
    return {"files": files, "stat": stat, "used_pipe": bool(flt.used_pipe), "bz2_stats": delta}

r1, r2 = os.path.join(work, "R1.fq"), os.path.join(work, "R2.fq")
res = {}
os.environ["AQC_BZ2_DEVICE_MIN"] = "0"
os.environ["AQC_BZ2_DEVICE_IN"] = "1"
res["device"] = run("device", r1 + ".bz2", r2 + ".bz2")
os.environ["AQC_BZ2_DEVICE_IN"] = "0"
res["host"] = run("host", r1 + ".bz2", r2 + ".bz2")
res["plain"] = run("plain", r1, r2)
print("RESULT " + json.dumps(res))
"""


def test_pipe_bz2_input_goes_through_the_device(tmp_path):
    """a paired R1.fq.bz2 / R2.fq.bz2 of 2,000 pairs through aqc_pipe_run with the one-stream branch forced onto the device
    (AQC_BZ2_DEVICE_IN=1, AQC_BZ2_DEVICE_MIN=0): output files and statistics equal those of the same run on libbz2
    (AQC_BZ2_DEVICE_IN=0) and of the plain-text input; the pipe was used; aqc_bz2_input_stats counts device blocks in the first
    run and none in the second.  In a child process (the switches are its environment's)."""
    import json
    from afterqc_amd import synth
    work = str(tmp_path)
    d = synth.make_pairs(2000, 150, seed=8850, dirty=True)
    for mate, name in ((1, "R1.fq"), (2, "R2.fq")):
        p = os.path.join(work, name)
        synth.write_fastq_fixed(p, d["seq%d" % mate], d["qual%d" % mate], mate)
        with open(p, "rb") as f, open(p + ".bz2", "wb") as g:
            g.write(bz2.compress(f.read(), 1))
    env = {k: v for k, v in os.environ.items() if not k.startswith("AQC_BZ2_")}
    out = subprocess.run([sys.executable, "-c", _PIPE_CHILD, ROOT, work], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    dev, host, plain = res["device"], res["host"], res["plain"]
    assert dev["used_pipe"] and host["used_pipe"] and plain["used_pipe"]
    assert len(dev["files"]) >= 4
    assert dev["files"] == host["files"] == plain["files"]
    assert dev["stat"] == host["stat"] == plain["stat"]
    assert dev["stat"]["afterqc_main_summary"]["total_reads"] >= 2000
    blocks, dev_blocks, text_bytes, dev_bytes = dev["bz2_stats"]
    assert dev_blocks > 0 and dev_blocks == blocks and dev_bytes == text_bytes > 0, dev["bz2_stats"]
    assert host["bz2_stats"][1] == 0 and host["bz2_stats"][3] == 0, host["bz2_stats"]
