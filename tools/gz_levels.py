#!/usr/bin/env python3
"""What `--compression 6 .. 9` costs and gains on the device (csrc/aqc_gzlz.hpp), measured; needs a GPU.

  python tools/gz_levels.py sizes                      # tests/golden/testdata: device bytes at levels 2, 6 - 9 beside zlib's members
  python tools/gz_levels.py digest                     # SHA-256 of the .gz bytes of five texts at levels 2, 6, 9 and at 2 with
                                                       # AQC_GZ_ENCODER=seg: the encoders are deterministic, so two builds that
                                                       # encode alike print the same lines
  python tools/gz_levels.py compress --pairs 131072    # aqc_compress per chunk (text resident in HBM) at levels 2, 6, 9
  python tools/gz_levels.py pipe --pairs 500000        # plain -> .gz through the pipe at levels 6 and 9: the device against the host
                                                       # codec at the same level (AQC_GZ_DEVICE=0), interleaved, a fresh process each

Every mode prints `gzlevels|` lines."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEMBER = 0xff00


def pad(data):
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def pass_all(capi, paired):
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.qc_kmer = 8
    return cfg


def zlib_members(text, level):
    total = 0
    for o in range(0, len(text), MEMBER):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(text[o:o + MEMBER]) + c.flush()) + 26
    return total


def formatted(eng, capi, text):
    """a single-end text whose records all pass, formatted in slot 0: stream 0 is the text itself"""
    eng.set_config(pass_all(capi, False))
    eng.set_circles([])
    eng.reset_stats()
    info = eng.frame(0, pad(text), len(text), True)
    eng.run(0)
    got = eng.format(0, int(info.n))
    assert got[0] == len(text), got


def sizes(args):
    from afterqc_amd import capi
    eng = capi.Engine(0, 1)
    try:
        for mate in (1, 2):
            with gzip.open(os.path.join(ROOT, "tests", "golden", "testdata", "R%d.fq.gz" % mate), "rb") as f:
                text = f.read()
            formatted(eng, capi, text)
            dev = {level: eng.compress(0, level)[0] for level in (2, 6, 7, 8, 9)}
            ref = {level: zlib_members(text, level) for level in (2, 3, 4, 6, 9)}
            print("gzlevels| sizes R%d text %d  device %s  zlib members of 0xff00 %s" % (mate, len(text), json.dumps(dev), json.dumps(ref)))
    finally:
        eng.close()


def digest(args):
    """tests/gzlz_cases.py's real reads and far_repeats, test_gpu_gzlz.py's stored_fallback text, one residue just above a member"""
    from afterqc_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gzlz_cases as cases
    seg = args.mode == "digest-seg"
    stored = cases.exact(np.random.default_rng(7950), 16 * MEMBER) + cases.noise_text(2 * MEMBER - 300)
    texts = [("real_R1", cases.real(1)), ("real_R2", cases.real(2)), ("far_repeats", cases.far_repeats()), ("stored_fallback", stored),
             ("residue_%d" % (MEMBER + 1), cases.exact(np.random.default_rng(7900 + (MEMBER + 1) % 89), MEMBER + 1))]
    eng = capi.Engine(0, 1)
    try:
        for name, text in texts:
            formatted(eng, capi, text)
            for level in ((2,) if seg else (2, 6, 9)):
                for q, zb in enumerate(eng.compress(0, level)):
                    if zb:
                        comp = np.zeros(zb + 64, dtype=np.uint8)
                        eng.fetch_gz(0, q // 3, q % 3, comp, comp.size)
                        print("gzlevels| digest %-16s level %d%s stream %d: text %8d  gz %8d  sha256 %s" % (
                            name, level, " seg" if seg else "", q, len(text), zb, hashlib.sha256(comp[:zb].tobytes()).hexdigest()))
    finally:
        eng.close()
    if seg:
        return 0
    sys.stdout.flush()
    # the seg encoder is chosen when the library first compresses: a fresh process
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "digest-seg"], env=dict(os.environ, AQC_GZ_ENCODER="seg"), timeout=300)
    return p.returncode


def compress(args):
    from afterqc_amd import capi, synth
    d = synth.make_pairs(args.pairs, 150, seed=1003, workers=8)
    t1, n1 = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    t2, n2 = synth.render_fastq_fixed(d["seq2"], d["qual2"], 2)
    eng = capi.Engine(0, 1)
    try:
        eng.set_config(pass_all(capi, True))
        eng.set_circles([])
        eng.reset_stats()
        info = eng.frame(0, t1, n1, True, t2, n2, True)
        eng.run(0)
        got = eng.format(0, int(info.n))
        text = sum(got)
        for level in (2, 6, 9, 2, 6, 9):          # (the first round of three warms buffers and code up)
            best, out = None, 0
            for _ in range(args.reps):
                t = time.perf_counter()
                out = sum(eng.compress(0, level))
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
            print("gzlevels| compress level %d: chunk of %d pairs, text %d bytes -> %d (ratio %.3f), best of %d: %.2f ms, %.2f GB/s of text" % (
                level, args.pairs, text, out, text / out, args.reps, best * 1e3, text / best / 1e9))
    finally:
        eng.close()


def pipe_child(args):
    from afterqc_amd import after, preprocesser
    out = os.path.join(args.dir, "out_%d_%s" % (args.level, os.environ.get("AQC_GZ_DEVICE", "1")))
    argv = ["-1", os.path.join(args.dir, "R1.fq"), "-2", os.path.join(args.dir, "R2.fq"), "-f", "0", "-t", "0", "-z", "--compression", str(args.level),
            "-g", os.path.join(out, "good"), "-b", os.path.join(out, "bad"), "-r", os.path.join(out, "QC")]
    options, _ = after.parseCommand(argv)
    after.finalize_options(options)
    options.barcode = False
    flt = preprocesser.seqFilter(options, use_pipe=True, devices=[0])
    t = time.perf_counter()
    flt.run()
    dt = time.perf_counter() - t
    size = sum(os.path.getsize(os.path.join(out, sub, f)) for sub in ("good", "bad") for f in os.listdir(os.path.join(out, sub)))
    print("gzlevels-child " + json.dumps({"level": args.level, "device": os.environ.get("AQC_GZ_DEVICE", "1") != "0", "seconds": round(dt, 3), "pipe_s": round(float(flt.timing.get("pipe_s", 0.0)), 3),
                                          "gz_bytes": size, "used_pipe": bool(flt.used_pipe)}))


def pipe(args):
    from afterqc_amd import synth
    os.makedirs(args.dir, exist_ok=True)
    d = synth.make_pairs(args.pairs, 150, seed=1003, workers=8)
    text = 0
    for mate in (1, 2):
        p = os.path.join(args.dir, "R%d.fq" % mate)
        synth.write_fastq_fixed(p, d["seq%d" % mate], d["qual%d" % mate], mate)
        text += os.path.getsize(p)
    del d
    for rep in range(args.reps):
        for level in (6, 9):
            for device in ("1", "0"):
                env = dict(os.environ, AQC_GZ_DEVICE=device)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "pipe-child", "--level", str(level), "--dir", args.dir], env=env,
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    # (a child that failed may have faulted the device: nothing more is started on it)
                    print("gzlevels| pipe child failed (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-2000:]))
                    return 1
                line = [l for l in p.stdout.splitlines() if l.startswith("gzlevels-child ")][0]
                r = json.loads(line[len("gzlevels-child "):])
                print("gzlevels| pipe rep %d level %d %s: %d pairs, text in %d bytes, .gz out %d, %.2f s whole run (pass 2 in the pipe %.2f s), %.2f GB/s of text, used_pipe %s" % (
                    rep, level, "device" if r["device"] else "host codec (AQC_GZ_DEVICE=0)", args.pairs, text, r["gz_bytes"], r["seconds"], r["pipe_s"],
                    text / r["seconds"] / 1e9, r["used_pipe"]))
                sys.stdout.flush()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sizes", "digest", "digest-seg", "compress", "pipe", "pipe-child"])
    ap.add_argument("--pairs", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--dir", default="/tmp/aqc_gz_levels")
    args = ap.parse_args()
    return {"sizes": sizes, "digest": digest, "digest-seg": digest, "compress": compress, "pipe": pipe, "pipe-child": pipe_child}[args.mode](args) or 0


if __name__ == "__main__":
    sys.exit(main())
