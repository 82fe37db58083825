#!/usr/bin/env python3
"""Measure the verdict kernel's 20-word tier (reads of 289 - 320 bases) against the general wave-per-record kernel of the same
build, on the MI355X:

    python tools/tier_bench.py [--pairs 1000000] [--workloads pe300,bc317,se320] [--label TEXT] >> profiles/<round>_tier20.txt

  workloads  pe300: synth.make_pairs(L=300) as a packed batch resident in HBM; bc317: the same plus the 17-base barcode / verify
             prefix on both mates, barcode mode; se320: read 1 of make_pairs(L=320), single-end
  contexts   two in one process: the second is created under AQC_FORCE_GENERIC=1 (the switch is read by aqc_create), so its
             aqc_run launches filter_overlap_kernel for every record
  timing     5 warm-up and 20 timed aqc_run per context, ALTERNATING between the two, each timed by the HIP events around
             AQC_K_FILTER_OVERLAP (aqc_timing_mean over one launch: the lane-per-pair kernel AND the list kernel behind it)
  reported   median and min of both, pairs/s, and the fraction of the HBM roofline by SURVEY 8d's algorithmic bytes,
             (4 L + 56) n / t / 8.0e12 for pairs ((2 L + 28) n for single reads), with L the sequenced length without the prefix;
             the deferred share; the spread (max / min) of each side's runs, which the gain has to exceed

AQC_LIB=<another build> selects the library (afterqc_amd/capi.py): a build with -DAQC_TIER20_WPBT=11 is how the 10- against
11-wave choice of the paired instances is repeated; --label names the build in the output."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def workload(name, n):
    import numpy as np
    from afterqc_amd import capi, synth
    cfg = capi.Config()
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    if name == "se320":
        d = synth.make_pairs(n, 320, seed=1003)
        cfg.paired = 0
        return capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"]), cfg, (2 * 320 + 28) * n
    d = synth.make_pairs(n, 300, seed=1003)
    cfg.paired = 1
    if name == "bc317":
        d = synth.add_barcodes(d, 1010)
        cfg.barcode = 1
    elif name != "pe300":
        raise SystemExit("unknown workload " + name)
    return capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"]), cfg, (4 * 300 + 56) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--workloads", default="pe300,bc317,se320")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import numpy as np
    from afterqc_amd import capi
    tier = capi.Engine(0, 1)
    os.environ["AQC_FORCE_GENERIC"] = "1"
    general = capi.Engine(0, 1)
    del os.environ["AQC_FORCE_GENERIC"]
    print("# tier_bench %s on %s: %d records, %d warm-up + %d timed aqc_run per context, alternating; library %s"
          % (a.label, tier.device_name(), a.pairs, a.warmup, a.reps, os.path.relpath(capi.LIB_PATH, ROOT)), flush=True)
    print("# %-6s %-8s %5s %9s %9s %7s %10s %9s %9s" % ("load", "kernel", "words", "median_ms", "min_ms", "max/min", "Mrec/s", "roofline", "deferred"))
    for name in a.workloads.split(","):
        batch, cfg, alg_bytes = workload(name, a.pairs)
        ms = {}
        engines = (("tier", tier), ("general", general))
        for _, eng in engines:
            eng.set_config(cfg)
            eng.reset_stats()
            eng.upload(0, batch)
        res = []
        for k in range(a.warmup + a.reps):
            for tag, eng in engines:
                eng.timing_reset(0)
                eng.run(0)
                t, cnt = eng.timing_mean(0)
                assert cnt[capi.K_FILTER_OVERLAP] == 1
                if k >= a.warmup:
                    ms.setdefault(tag, []).append(float(t[capi.K_FILTER_OVERLAP]))
        for tag, eng in engines:
            res.append(eng.fetch_results(0).tobytes())
            v = np.array(ms[tag])
            med, lo = float(np.median(v)), float(v.min())
            print("  %-6s %-8s %5d %9.4f %9.4f %7.3f %10.1f %9.4f %9.5f"
                  % (name, tag, eng.last_verdict_words(0), med, lo, float(v.max()) / lo, batch.n / (med * 1e-3) / 1e6,
                     alg_bytes / (med * 1e-3) / PEAK, eng.last_deferred(0) / batch.n), flush=True)
        assert res[0] == res[1], "the tier's results differ from the general kernel's"
        gain = float(np.median(ms["general"]) / np.median(ms["tier"]))
        print("  %-6s gain of the tier over the general kernel: %.2f x (medians), %.2f x (slowest tier run against the fastest general run); results identical"
              % (name, gain, min(ms["general"]) / max(ms["tier"])), flush=True)
    tier.close()
    general.close()


if __name__ == "__main__":
    main()
