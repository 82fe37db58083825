#!/usr/bin/env python3
"""The third stream's second writer pass on config 3 (5 M pairs of 2 x 150, resident in HBM): --store_overlap's overlap pass and
--store_merged's merged pass, side by side.

    python tools/merged_pass.py run [--pairs N] [--reps R]      frame -> run once, then R x aqc_format in mode 1 and R x in mode 2;
                                                                prints the stream sizes (run it under rocprofv3 --kernel-trace)
    python tools/merged_pass.py files DIR [--pairs N]           write the input as DIR/R1.fq, DIR/R2.fq (for CLI wall times)
    python tools/merged_pass.py summarize KERNEL_TRACE.csv OVERLAP_BYTES MERGED_BYTES
                                                                per format call of the trace: the kernels behind the main pass —
                                                                fmt_plan_kernel .. (overlap pass) or fmt_merged_kernel — in ms and
                                                                bytes written per ms
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(pairs):
    from afterqc_amd import synth
    return synth.make_pairs(pairs, 150, seed=1003, workers=min(16, os.cpu_count() or 1))


def run(args):
    d = make_input(args.pairs)
    from afterqc_amd import capi, synth
    n_rec = len(d["len1"])
    cfg = capi.Config()
    cfg.paired = 1
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    eng = capi.Engine(0, 2)
    eng.set_config(cfg)
    eng.reset_stats()
    w = synth.fixed_record_width(d["seq1"].shape[1])
    texts = []
    for mate in (1, 2):
        hb = eng.host_buffer(n_rec * w + 4096)
        _, nbytes = synth.render_fastq_fixed(d["seq%d" % mate], d["qual%d" % mate], mate, out=hb.array)
        texts.append((hb, nbytes))
    info = eng.frame(0, texts[0][0].array, texts[0][1], True, texts[1][0].array, texts[1][1], True)
    assert int(info.n) == n_rec
    eng.run(0)
    eng.sync(0)
    for mode, tag in ((capi.STORE_OVERLAP, "overlap"), (capi.STORE_MERGED, "merged")):
        for _ in range(args.reps):
            sizes = eng.format(0, n_rec, mode)
            eng.sync(0)
        print("%s: records %d third-stream bytes %d (file 0: %d, file 1: %d) good bytes %d" % (tag, n_rec, sizes[2] + sizes[5], sizes[2], sizes[5], sizes[0] + sizes[3]))
    eng.close()


def files(args):
    d = make_input(args.pairs)
    from afterqc_amd import synth
    import numpy as np
    os.makedirs(args.dir, exist_ok=True)
    w = synth.fixed_record_width(d["seq1"].shape[1])
    for mate in (1, 2):
        buf = np.empty(len(d["len1"]) * w + 4096, dtype=np.uint8)
        _, nbytes = synth.render_fastq_fixed(d["seq%d" % mate], d["qual%d" % mate], mate, out=buf)
        with open(os.path.join(args.dir, "R%d.fq" % mate), "wb") as f:
            f.write(buf[:nbytes].data)


def summarize(args):
    rows = list(csv.DictReader(open(args.csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "fmt_tile_sums_kernel" in name:
            cur = []
            calls.append(cur)
        if cur is not None and "fmt_" in name:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    for what, nbytes in (("overlap", args.overlap_bytes), ("merged", args.merged_bytes)):
        times = []
        for c in calls:
            names = [n for n, _ in c]
            if what == "merged" and any("fmt_merged_kernel" in n for n in names):
                times.append(sum(ms for n, ms in c if "fmt_merged_kernel" in n))
            elif what == "overlap" and any("fmt_plan_kernel" in n for n in names) and not any("fmt_merged_kernel" in n for n in names):
                k = next(i for i, n in enumerate(names) if "fmt_plan_kernel" in n)
                times.append(sum(ms for _, ms in c[k:]))
                detail = ", ".join("%s %.3f" % (n.split("(")[0].replace("aqc::", "").replace("void ", ""), ms) for n, ms in c[k:])
        if not times:
            print("%s pass: no such format call in the trace" % what)
            continue
        times.sort()
        med = times[len(times) // 2]
        print("%s pass: %d calls, ms min %.3f median %.3f max %.3f; %d bytes written -> %.1f MB per ms (median)%s"
              % (what, len(times), times[0], med, times[-1], nbytes, nbytes / med / 1e6, ("; last call: " + detail) if what == "overlap" else ""))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run"); a.add_argument("--pairs", type=int, default=5_000_000); a.add_argument("--reps", type=int, default=5)
    b = sub.add_parser("files"); b.add_argument("dir"); b.add_argument("--pairs", type=int, default=5_000_000)
    c = sub.add_parser("summarize"); c.add_argument("csv"); c.add_argument("overlap_bytes", type=int); c.add_argument("merged_bytes", type=int)
    args = ap.parse_args()
    {"run": run, "files": files, "summarize": summarize}[args.cmd](args)


if __name__ == "__main__":
    main()
