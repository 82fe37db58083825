#!/usr/bin/env python3
"""Measure the debubble pre-pass on the MI355X: the census kernel on config-3 text resident in HBM, and the command line
over a config-3 file pair.

    python tools/census_bench.py --reads 10000000 --out profiles/census

  kernel: 10 M reads (2 x 5 M, synth.make_census_text: names with lane / tile / x / y, 3 % polyX reads) framed into the
          slots of one context (chunks of --chunk reads, all resident), then aqc_poly_census on every slot --reps times; the
          kernel's time from HIP events (aqc_census_ms), its algorithmic bytes (the sequence lines + their offset / length
          words, the name lines, offsets and hit records of the polyX reads) over 8 TB/s
  trace:  the same kernel part again under rocprofv3 --kernel-trace --stats (in a child process, its own time limit)
  cli:    `python -m afterqc_amd.debubble -i DIR -o OUT -p 20 -d on` over the two files written as plain text
Writes <out>_kernel.json, <out>_rocprof_summary.txt, <out>_cli.txt."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def kernel_part(reads, chunk, reps, L=150, poly_frac=0.03):
    import numpy as np
    from afterqc_amd import capi, synth
    pieces = []
    for mate in (1, 2):
        for a in range(0, reads // 2, chunk):
            pieces.append((mate, a, min(chunk, reads // 2 - a)))
    eng = capi.Engine(0, len(pieces))
    n_tot = hits = name_bytes = 0
    for slot, (mate, a, m) in enumerate(pieces):
        t = synth.make_census_text(m, L, mate=mate, index0=a, poly_frac=poly_frac)
        info = eng.frame(slot, t, len(t), True)
        assert int(info.n) == m
        n_tot += m
        h = eng.fetch_census(slot, eng.poly_census(slot, 20))
        hits += len(h)
        name_bytes += int(h["name_len"].sum())
    ms = []
    for _ in range(reps):
        tot = 0.0
        for slot in range(len(pieces)):
            eng.poly_census(slot, 20)
            tot += eng.census_ms(slot)
        ms.append(tot)
    eng.close()
    best = min(ms)
    # sequence bytes + seq_off / seq_len words per read; name bytes + name_off / name_len words + a hit record per polyX read
    alg = n_tot * (L + 8) + name_bytes + hits * (8 + capi.CENSUS_HIT_DTYPE.itemsize)
    return dict(reads=n_tot, poly_frac=poly_frac, slots=len(pieces), polyx_reads=hits, kernel_ms_best=round(best, 3),
                kernel_ms_median=round(sorted(ms)[len(ms) // 2], 3), algorithmic_bytes=alg,
                hbm_fraction_of_8TBps=round(alg / (best * 1e-3) / PEAK, 3), gbps=round(alg / (best * 1e-3) / 1e9, 1),
                mreads_per_s=round(n_tot / (best * 1e-3) / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--chunk", type=int, default=1_250_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "census"))
    ap.add_argument("--kernel-only", action="store_true", help="the kernel part alone, result on stdout (the rocprofv3 child)")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: trace,cli")
    a = ap.parse_args()
    if a.kernel_only:
        print(json.dumps(kernel_part(a.reads, a.chunk, a.reps)))
        return
    skip = set(a.skip.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    k = kernel_part(a.reads, a.chunk, a.reps)
    k0 = kernel_part(a.reads, a.chunk, a.reps, poly_frac=0.0)        # the run test alone: no polyX read, no name walked
    print(json.dumps(k))
    print(json.dumps(k0))
    with open(a.out + "_kernel.json", "w") as f:
        json.dump({"config3_3pct_polyx": k, "config3_no_polyx": k0}, f, indent=1)
    if "trace" not in skip and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="aqc_census_prof_")
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "census",
               "--", sys.executable, os.path.abspath(__file__), "--kernel-only", "--reads", str(a.reads), "--chunk", str(a.chunk), "--reps", "3"]
        rc = subprocess.run(cmd, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        with open(a.out + "_rocprof_summary.txt", "w") as f:
            f.write("# rocprofv3 --kernel-trace --stats, tools/census_bench.py --kernel-only --reads %d --reps 3 (rc=%d)\n" % (a.reads, rc))
            for s in stats:
                f.write(open(s).read())
        print(open(a.out + "_rocprof_summary.txt").read())
        shutil.rmtree(d, ignore_errors=True)
        if rc != 0:
            sys.exit("rocprofv3 run failed: rc=%d" % rc)
    if "cli" not in skip:
        from afterqc_amd import synth
        d = tempfile.mkdtemp(prefix="aqc_census_cli_")
        try:
            t0 = time.time()
            for mate in (1, 2):
                synth.write_census_file(os.path.join(d, "C3_R%d.fq" % mate), a.reads // 2, mate=mate)
            t_gen = time.time() - t0
            size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            subprocess.run(["sync"])
            walls = {}
            for draw in ("off", "on"):                   # without the maps first: census + CSVs + detector alone
                t0 = time.time()
                p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-m", "afterqc_amd.debubble", "-i", d, "-o",
                                    os.path.join(d, "out_" + draw), "-p", "20", "-d", draw], cwd=ROOT, capture_output=True, text=True)
                walls[draw] = time.time() - t0
                if p.returncode != 0:
                    break
            wall = walls.get("on", 0.0)
            # the file reading alone, as the pass reads them (fastq.open_binary), for the bound
            from afterqc_amd import fastq
            import numpy as np
            t0 = time.time()
            buf = bytearray(64 << 20)
            got = 0
            for mate in (1, 2):
                src = fastq.open_binary(os.path.join(d, "C3_R%d.fq" % mate))
                while True:
                    m = src.readinto(buf)
                    if not m:
                        break
                    got += m
                src.close()
            t_read = time.time() - t0
            assert got == size, (got, size)
            lines = ["# python -m afterqc_amd.debubble -i DIR -o OUT -p 20 -d on over a config-3 pair (2 x %d reads, plain text, "
                     "%.2f GB; files written %.1f s before, page cache warm)" % (a.reads // 2, size / 1e9, t_gen),
                     "rc=%d wall_s=%.2f  (%.2f GB/s, %.1f Mreads/s)" % (p.returncode, wall, size / max(wall, 1e-9) / 1e9, a.reads / max(wall, 1e-9) / 1e6),
                     "the same with -d off (no image_by_camera maps): wall_s=%.2f" % walls.get("off", 0.0),
                     "read-only pass over the same files (fastq.open_binary readinto): %.2f s (%.2f GB/s)" % (t_read, size / t_read / 1e9),
                     "--- tail of the pass's output ---"] + p.stdout.strip().splitlines()[-6:] + p.stderr.strip().splitlines()[-5:]
            with open(a.out + "_cli.txt", "w") as f:
                f.write("\n".join(lines) + "\n")
            print("\n".join(lines))
            if p.returncode != 0:
                sys.exit("the pre-pass failed: rc=%d" % p.returncode)
        finally:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
