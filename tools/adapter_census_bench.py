#!/usr/bin/env python3
"""Measure the adapter census of pass 1 (--adapter_sequence auto) on the MI355X.

    python tools/adapter_census_bench.py kernels [--records N] [--reps R]
        1 M records resident in HBM, single-end 150 and paired 2 x 150 and 2 x 300 (the input of tools/adapter_bench.py: 30 % of
        the reads carry their adapter).  In one context, ALTERNATING per repetition: the census with the 4-row table (one
        aqc_adapter_census per mate, aqc_adapter_census_ms), an aqc_run with one adapter per mate (the adapter pass,
        aqc_adapter_ms) and aqc_qc_stat of the same records (HIP events around AQC_K_QC_STAT).  The census's rate over the bytes
        it must move — per mate the sequence bytes, a length word and an offset word — as a share of the 8000 GB/s peak.
    python tools/adapter_census_bench.py pass1 [--records N] [--reps R]
        the wall time of pass 1 (seqFilter.timing["pass1_s"]) of the default run (--qc_sample 200000) on a 2 x 150 file pair, with
        and without --adapter_sequence auto: fresh processes, interleaved
    python tools/adapter_census_bench.py once LOAD
        the census alone, for a profiler (LOAD: se150, pe150 or pe300)

Results: profiles/r20_adapter_census.txt."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import adapter_bench as ab
import viewpass_bench as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def moved_bytes(L, paired, n):
    return (2 if paired else 1) * (L + 8) * n


def set_probes(eng):
    from afterqc_amd import adapter_detect, capi
    for mate, which in enumerate((capi.QC_R1_PRE, capi.QC_R2_PRE)):
        eng.set_adapter_probes(which, adapter_detect.probes(mate))


def census(eng, n, paired):
    """the census of the slot's records, every mate -> its device time, the mates' launches added"""
    from afterqc_amd import capi
    ms = 0.0
    for mate in range(2 if paired else 1):
        eng.adapter_census(0, capi.QC_R2_PRE if mate else capi.QC_R1_PRE, mate, 0, n)
        eng.sync(0)
        ms += eng.adapter_census_ms(0)
    return ms


def kernels(a):
    import numpy as np
    from afterqc_amd import capi
    eng = capi.Engine(0, 1)
    print("# adapter_census_bench kernels on %s: %d records, %d warm-up + %d timed rounds of census / aqc_run / aqc_qc_stat in turn; census: the 4-row table, "
          "every mate; adapter pass: one adapter of 33 bases per mate, min overlap 4" % (eng.device_name(), a.records, a.warmup, a.reps), flush=True)
    print("# %-6s %10s %9s %9s %8s | %10s %9s %9s | %10s %9s | %s" % ("load", "census_ms", "min_ms", "max_ms", "of_peak", "adapter_ms", "min_ms", "max_ms", "qc_stat_ms",
                                                                       "min_ms", "census / adapter (medians)"))
    for load, (L, paired) in ab.LOADS.items():
        batch = ab.batch_of(ab.make_input(a.records, L), paired)
        eng.set_config(vb.base_config(paired))
        eng.set_adapter_trim(capi.AdapterConfig(ab.A1, ab.A2 if paired else b"", 4))
        eng.reset_stats()
        set_probes(eng)
        eng.upload(0, batch)
        t = {"census": [], "adapter": [], "qc": []}
        for k in range(a.warmup + a.reps):
            c = census(eng, batch.n, paired)
            eng.run(0)
            eng.sync(0)
            ad = eng.adapter_ms(0)
            q = 0.0
            for mate in range(2 if paired else 1):
                eng.qc_stat(0, capi.QC_R2_PRE if mate else capi.QC_R1_PRE, mate, 0, batch.n, 0)
                eng.sync(0)
                q += float(eng.kernel_ms(0)[capi.K_QC_STAT])
            if k >= a.warmup:
                t["census"].append(c); t["adapter"].append(ad); t["qc"].append(q)
        v = {k: np.array(x) for k, x in t.items()}
        counts = [eng.adapter_census_counts(w) // (a.warmup + a.reps) for w in (capi.QC_R1_PRE, capi.QC_R2_PRE)]
        print("  %-6s %10.4f %9.4f %9.4f %8.4f | %10.4f %9.4f %9.4f | %10.4f %9.4f | %.3f" % (
            load, float(np.median(v["census"])), float(v["census"].min()), float(v["census"].max()),
            vb.of_peak(moved_bytes(L, paired, batch.n), float(np.median(v["census"]))),
            float(np.median(v["adapter"])), float(v["adapter"].min()), float(v["adapter"].max()),
            float(np.median(v["qc"])), float(v["qc"].min()), float(np.median(v["census"]) / np.median(v["adapter"]))), flush=True)
        print("  %-6s reads looked at %d + %d, holding the rows' probes %s + %s" % (load, int(counts[0][0]), int(counts[1][0]), counts[0][1:5].tolist(), counts[1][1:5].tolist()), flush=True)
    eng.close()


def child(a):
    """one fresh process: the default run on the file pair, pass 1's wall time as a JSON line"""
    from afterqc_amd import after, preprocesser
    argv = ["-1", a.files[0], "-2", a.files[1], "-g", os.path.join(a.work, "good"), "--barcode", "off"] + (["--adapter_sequence", "auto"] if a.auto else [])
    options, _ = after.parseCommand(argv)
    after.finalize_options(options)
    options.barcode = False
    flt = preprocesser.seqFilter(options)
    stat = flt.run()
    det = stat.get("adapter_detect", {})
    print("CHILD " + json.dumps({"auto": bool(a.auto), "pass1_s": flt.timing["pass1_s"], "total_s": flt.timing["total_s"],
                                 "detected": [det.get(k, {}).get("detected") for k in ("read1", "read2")],
                                 "sampled": [det.get(k, {}).get("sampled") for k in ("read1", "read2")]}), flush=True)


def pass1(a):
    import numpy as np
    from afterqc_amd import synth
    with tempfile.TemporaryDirectory() as work:
        d = ab.make_input(a.records, 150)
        files = [os.path.join(work, "bench_R%d.fq" % (m + 1)) for m in range(2)]
        synth.write_fastq_fixed(files[0], d["seq1"], d["qual1"], 1)
        synth.write_fastq_fixed(files[1], d["seq2"], d["qual2"], 2)
        print("# adapter_census_bench pass1: %d pairs of 2 x 150 (%.1f MB per file), the default run (--qc_sample 200000), %d fresh processes per variant, interleaved"
              % (a.records, os.path.getsize(files[0]) / 1e6, a.reps), flush=True)
        t = {False: [], True: []}
        for k in range(a.reps + 1):                 # (the first pair warms the page cache and is left out)
            for auto in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "child", "--work", os.path.join(work, "out%d_%d" % (k, auto)), files[0], files[1]] + (["--auto"] if auto else [])
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("CHILD ")]
                if out.returncode != 0 or not line:
                    print(out.stdout[-2000:], out.stderr[-2000:])
                    raise SystemExit("the child process failed (exit status %d)" % out.returncode)
                r = json.loads(line[0][6:])
                if k:
                    t[auto].append(r["pass1_s"])
                print("  run %d %-5s pass1_s %.4f total_s %.4f detected %s sampled %s" % (k, "auto" if auto else "plain", r["pass1_s"], r["total_s"], r["detected"], r["sampled"]), flush=True)
        for auto in (False, True):
            v = np.array(t[auto])
            print("  %-5s pass1_s median %.4f min %.4f max %.4f" % ("auto" if auto else "plain", float(np.median(v)), float(v.min()), float(v.max())), flush=True)


def once(a):
    from afterqc_amd import capi
    L, paired = ab.LOADS[a.load]
    eng = capi.Engine(0, 1)
    eng.set_config(vb.base_config(paired))
    eng.reset_stats()
    set_probes(eng)
    batch = ab.batch_of(ab.make_input(a.records, L), paired)
    eng.upload(0, batch)
    for _ in range(a.reps):
        ms = census(eng, batch.n, paired)
    print("%s: %d censuses, census_ms of the last %.4f" % (a.load, a.reps, ms), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("kernels", "pass1", "once", "child"):
        p = sub.add_parser(name)
        if name == "child":
            p.add_argument("--work", required=True)
            p.add_argument("--auto", action="store_true")
            p.add_argument("files", nargs=2)
            continue
        p.add_argument("--records", type=int, default=1000000 if name != "pass1" else 250000)
        p.add_argument("--warmup", type=int, default=3)
        p.add_argument("--reps", type=int, default=10 if name != "pass1" else 5)
        if name == "once":
            p.add_argument("load", choices=sorted(ab.LOADS))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    {"kernels": kernels, "pass1": pass1, "once": once, "child": child}[a.cmd](a)


if __name__ == "__main__":
    main()
