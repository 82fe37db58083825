#!/usr/bin/env python3
"""Measure per-read quality cutting (--cut_front / --cut_tail / --cut_right) on the MI355X: 1 M pairs of 2 x 150 and 2 x 300 resident
in HBM, reads with decaying quality tails.

    python tools/qcut_bench.py kernels [--pairs N] [--reps R]
        two contexts in one process, both with a fixed trim (-f 2 -t 3), one with --cut_tail on, their aqc_run ALTERNATING:
        the cut pass's time (aqc_cut_ms) and its rate over the bytes it must move — both mates' quality bytes plus 8 bytes of
        views per pair — as a share of the 8000 GB/s peak; the verdict kernel's CUT instance against the plain instance of the
        same tier (HIP events around AQC_K_FILTER_OVERLAP), and the deferred share of each
    python tools/qcut_bench.py step [--tree DIR] [--cut_tail] [--pairs N] [--reps R]
        the device step on text resident in HBM: aqc_reframe -> aqc_run -> aqc_format, wall time per step with the slot synced.
        --tree: import afterqc_amd from another checkout (the parent's, built there) — a job script alternates processes of the
        two trees; the step uses only calls both have.  --cut_tail: with the cut on (this tree only)

Results: profiles/r16_qcut.txt."""
import argparse
import os
import sys
import time

import viewpass_bench as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(n, L):
    """synth.make_pairs with quality lines that are high up to a knee in the last 40 % of the read and decay behind it"""
    import numpy as np
    from afterqc_amd import synth
    d = synth.make_pairs(n, L, seed=1003, workers=min(16, os.cpu_count() or 1))
    rng = np.random.Generator(np.random.PCG64(1616 + L))
    j = np.arange(L, dtype=np.int32)[None, :]
    for k in ("qual1", "qual2"):
        knee = rng.integers((6 * L) // 10, L + 1, n).astype(np.int32)[:, None]
        noise = rng.integers(0, 6, (n, L)).astype(np.int32)
        q = np.where(j < knee, 40 - noise, np.maximum(2, 32 - (3 * (j - knee)) // 2 - noise))
        d[k] = (q + 33).astype(np.uint8)
    return d


def kernels(a):
    import numpy as np
    from afterqc_amd import capi
    plain, cut = capi.Engine(0, 1), capi.Engine(0, 1)
    print("# qcut_bench kernels on %s: %d pairs, %d warm-up + %d timed aqc_run per context, alternating; both contexts -f 2 -t 3, `cut` with --cut_tail on (window 4, quality 20)"
          % (plain.device_name(), a.pairs, a.warmup, a.reps), flush=True)
    print("# %-6s %-6s %5s %10s %9s %7s %9s | %9s %9s %8s" % ("load", "ctx", "words", "verdict_ms", "min_ms", "max/min", "deferred", "cut_ms", "min_ms", "of_peak"))
    for L in (150, 300):
        batch = vb.batch_of(make_input(a.pairs, L), True)
        engines = (("plain", plain), ("cut", cut))
        for tag, eng in engines:
            vb.prepare(eng, batch, True, lambda e: e.set_quality_cut(capi.CutConfig(0, 1, 0, 4, 20) if tag == "cut" else None), trim=(2, 3))
        ms, cms = vb.alternate(engines, a, "cut", lambda eng: eng.cut_ms(0))
        vb.verdict_rows(engines, ms, cms, "cut", "pe%d" % L, batch.n, (2 * L + 8) * batch.n, 6, 9)
        st = cut.cut_stats()
        print("  pe%-4d the CUT instance takes %.3f x the plain instance's time (medians); cut pass + CUT instance %.4f ms against %.4f ms; reads cut %d + %d of %d pairs, bases %d + %d"
              % (L, float(np.median(ms["cut"]) / np.median(ms["plain"])), float(np.median(ms["cut"]) + np.median(cms)), float(np.median(ms["plain"])),
                 int(st[0]) // (a.warmup + a.reps), int(st[2]) // (a.warmup + a.reps), batch.n, int(st[1]) // (a.warmup + a.reps), int(st[3]) // (a.warmup + a.reps)), flush=True)
    plain.close()
    cut.close()


def step(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    from afterqc_amd import capi
    eng = capi.Engine(0, 2)
    label = ("parent" if a.tree else "this") + (" cut_tail" if a.cut_tail else "")
    for L in (150, 300):
        d = make_input(a.pairs, L)
        eng.set_config(vb.base_config())
        if a.cut_tail:
            eng.set_quality_cut(capi.CutConfig(0, 1, 0, 4, 20))
        eng.reset_stats()
        v, sizes, n_rec = vb.device_step(eng, d, L, a)
        if a.detail:
            # where a step's time goes: each call synced on its own, and the verdict kernel by its HIP events
            parts = {"reframe": [], "run": [], "format": [], "verdict_kernel": []}
            for k in range(a.reps):
                for name, call in (("reframe", lambda: eng.reframe(0)), ("run", lambda: eng.run(0)), ("format", lambda: eng.format(0, n_rec, False))):
                    t0 = time.perf_counter()
                    call()
                    eng.sync(0)
                    parts[name].append(1000.0 * (time.perf_counter() - t0))
                parts["verdict_kernel"].append(float(eng.kernel_ms(0)[capi.K_FILTER_OVERLAP]))
            print("%-16s pe%-4d medians, each call synced: %s" % (label, L, "  ".join("%s %.4f" % (k, float(np.median(v))) for k, v in parts.items())), flush=True)
        print(vb.step_line(label, L, v, sizes), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("kernels", "step"):
        p = sub.add_parser(name)
        p.add_argument("--pairs", type=int, default=1000000)
        p.add_argument("--warmup", type=int, default=3)
        p.add_argument("--reps", type=int, default=10)
        if name == "step":
            p.add_argument("--tree", default="")
            p.add_argument("--cut_tail", action="store_true")
            p.add_argument("--detail", action="store_true", help="also time reframe / run / format synced one by one, and the verdict kernel's events")
    a = ap.parse_args()
    if a.cmd == "kernels":
        sys.path.insert(0, ROOT)
        kernels(a)
    else:
        step(a)


if __name__ == "__main__":
    main()
