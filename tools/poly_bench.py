#!/usr/bin/env python3
"""Measure cutting poly-G / poly-X tails (--trim_poly_g / --trim_poly_x) on the MI355X: 1 M records resident in HBM, single-end 150
and paired 2 x 150 and 2 x 300.  30 % of the reads end in a tail of 10 .. 60 bases of one letter (70 % of the tails G), one base
substituted in half of the tails of 24 bases or more.

    python tools/poly_bench.py passes [--sisters] [--tree DIR] [--records N] [--reps R] [--cache DIR]
        the view passes alone, each on a context of its own, -f 0 -t 0, their aqc_run ALTERNATING: the pass's time (aqc_poly_ms;
        --sisters: aqc_cut_ms with --cut_tail on and aqc_adapter_ms with both adapters) and its rate over the bytes it must move
        — per mate the sequence (the cut: quality) bytes, a length word, an offset word and 4 bytes of view — as a share of the
        8000 GB/s peak.  --tree: import afterqc_amd from another checkout (the parent's, built there; --sisters uses only calls
        the parent has) — a job script alternates processes of the two trees on the same batches.  --cache: keep the generated
        reads there (.npy), so that the processes of a job make them once.
    python tools/poly_bench.py step [--poly] [--records N] [--reps R]
        the device step on text resident in HBM: aqc_reframe -> aqc_run -> aqc_format, wall time per step with the slot synced;
        --poly: with --trim_poly_g on.  (Options off against the parent commit: tools/qcut_bench.py step [--tree DIR].)
    python tools/poly_bench.py once LOAD
        one aqc_run with poly-G on, for a profiler's kernel trace (LOAD: se150, pe150 or pe300)

Results: profiles/r19_polytail.txt."""
import argparse
import os
import sys

import viewpass_bench as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A1, A2, LOADS, batch_of, moved_bytes = vb.A1, vb.A2, vb.LOADS, vb.batch_of, vb.moved_bytes


def make_input(n, L, frac=0.3, cache=""):
    """synth.make_pairs with a tail of one letter written over the end of `frac` of the reads"""
    return vb.cached_input(cache, "poly_%d_%d_%d" % (n, L, round(100 * frac)), lambda: generate(n, L, frac))


def generate(n, L, frac):
    import numpy as np
    from afterqc_amd import synth
    d = synth.make_pairs(n, L, seed=1003, workers=min(16, os.cpu_count() or 1))
    rng = np.random.Generator(np.random.PCG64(1919 + L))
    j = np.arange(L, dtype=np.int32)[None, :]
    others = np.frombuffer(b"ACT", dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for key in ("seq1", "seq2"):
        has = rng.random(n) < frac
        t = rng.integers(10, 61, n).astype(np.int32)[:, None]
        letter = np.where(rng.random(n) < 0.7, np.uint8(ord("G")), others[rng.integers(0, 3, n)])[:, None]
        sub = np.where((t[:, 0] >= 24) & (rng.random(n) < 0.5), L - 1 - rng.integers(0, 23, n), -1).astype(np.int32)[:, None]
        seq = d[key]
        new = np.where(j >= L - t, letter, seq)
        new = np.where(j == sub, letters[(np.searchsorted(letters, np.minimum(new, 84)) + 1) % 4], new)
        d[key] = np.where(has[:, None], new, seq).astype(np.uint8)
    return d


def passes(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    from afterqc_amd import capi
    build = "parent" if a.tree else "this"
    if a.sisters:
        contexts = [("cut_tail", lambda e, paired: e.set_quality_cut(capi.CutConfig(0, 1, 0, 4, 20)), lambda e: e.cut_ms(0)),
                    ("adapter", lambda e, paired: e.set_adapter_trim(capi.AdapterConfig(A1, A2 if paired else b"", 4)), lambda e: e.adapter_ms(0))]
    else:
        contexts = [("poly_g", lambda e, paired: e.set_poly_trim(capi.PolyConfig(0, 0, 10, 0)), lambda e: e.poly_ms(0)),
                    ("poly_x", lambda e, paired: e.set_poly_trim(capi.PolyConfig(10, 10, 10, 10)), lambda e: e.poly_ms(0))]
    engines = [capi.Engine(0, 1) for _ in contexts]
    print("# poly_bench passes, %s build on %s: %d records, %d warm-up + %d timed aqc_run per context, alternating; -f 0 -t 0"
          % (build, engines[0].device_name(), a.records, a.warmup, a.reps), flush=True)
    print("# %-7s %-6s %-9s %9s %9s %9s %8s" % ("build", "load", "pass", "median_ms", "min_ms", "max_ms", "of_peak"))
    for load, (L, paired) in LOADS.items():
        batch = batch_of(make_input(a.records, L, cache=a.cache), paired)
        for (tag, setter, _), eng in zip(contexts, engines):
            vb.prepare(eng, batch, paired, lambda e: setter(e, paired))
        times = vb.pass_times([(eng, ms) for (_, _, ms), eng in zip(contexts, engines)], a)
        for (tag, _, _), eng, v in zip(contexts, engines, times):
            row = "  %-7s %-6s %-9s %9.4f %9.4f %9.4f %8.4f" % (build, load, tag, float(np.median(v)), float(v.min()), float(v.max()),
                                                              vb.of_peak(moved_bytes(L, paired, batch.n), float(np.median(v))))
            if not a.sisters:
                st = eng.poly_stats() // (a.warmup + a.reps)
                row += "  reads cut %d + %d of %d records, bases %d + %d" % (int(st[0]), int(st[2]), batch.n, int(st[1]), int(st[3]))
            print(row, flush=True)
    for eng in engines:
        eng.close()


def step(a):
    from afterqc_amd import capi
    vb.step(a, lambda L: make_input(a.records, L, cache=a.cache), "this poly_g" if a.poly else "this",
            lambda eng: eng.set_poly_trim(capi.PolyConfig(0, 0, 10, 0) if a.poly else None), "poly_ms")


def once(a):
    from afterqc_amd import capi
    L, paired = LOADS[a.load]
    vb.once(a, make_input(a.records, L, cache=a.cache), paired, lambda eng: eng.set_poly_trim(capi.PolyConfig(0, 0, 10, 0)), "poly_ms")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("passes", "step", "once"):
        p = sub.add_parser(name)
        p.add_argument("--records", type=int, default=1000000)
        p.add_argument("--warmup", type=int, default=3)
        p.add_argument("--reps", type=int, default=10)
        p.add_argument("--cache", default="")
        if name == "passes":
            p.add_argument("--sisters", action="store_true")
            p.add_argument("--tree", default="")
        if name == "step":
            p.add_argument("--poly", action="store_true")
        if name == "once":
            p.add_argument("load", choices=sorted(LOADS))
    a = ap.parse_args()
    if a.cmd != "passes":
        sys.path.insert(0, ROOT)
    {"passes": passes, "step": step, "once": once}[a.cmd](a)


if __name__ == "__main__":
    main()
