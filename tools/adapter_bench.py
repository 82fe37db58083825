#!/usr/bin/env python3
"""Measure trimming a given adapter (--adapter_sequence / --adapter_sequence_r2) on the MI355X: 1 M records resident in HBM,
single-end 150 and paired 2 x 150 and 2 x 300.  By default 30 % of the reads carry their adapter from a random place on (a third
of those only 4 .. 20 adapter bases at the very end), random bases behind it, one adapter base substituted in 30 % of them.

    python tools/adapter_bench.py kernels [--records N] [--reps R]
        two contexts in one process, -f 0 -t 0, one with the adapters set, their aqc_run ALTERNATING: the adapter pass's time
        (aqc_adapter_ms) and its rate over the bytes it must move — per mate the sequence bytes, a length word, an offset word and
        4 bytes of view — as a share of the 8000 GB/s peak; the verdict kernel's CUT instance against the plain instance of the
        same tier (HIP events around AQC_K_FILTER_OVERLAP)
    python tools/adapter_bench.py exit [--records N] [--reps R]
        the pass alone on 2 x 150 with the adapter in 0 %, 30 % and 100 % of the reads: what the early exits are worth
    python tools/adapter_bench.py step [--adapter] [--records N] [--reps R]
        the device step on text resident in HBM: aqc_reframe -> aqc_run -> aqc_format, wall time per step with the slot synced;
        --adapter: with the option on.  (Options off against the parent commit: tools/qcut_bench.py step [--tree DIR].)
    python tools/adapter_bench.py once LOAD
        one aqc_run with the adapters set, for a profiler's kernel trace (LOAD: se150, pe150 or pe300)

Results: profiles/r17_adapter.txt."""
import argparse
import os
import sys

import viewpass_bench as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A1, A2, LOADS, batch_of, moved_bytes = vb.A1, vb.A2, vb.LOADS, vb.batch_of, vb.moved_bytes


def make_input(n, L, frac=0.3):
    """synth.make_pairs with the mates' adapters written over the tail of `frac` of the reads"""
    import numpy as np
    from afterqc_amd import synth
    d = synth.make_pairs(n, L, seed=1003, workers=min(16, os.cpu_count() or 1))
    rng = np.random.Generator(np.random.PCG64(1717 + L))
    j = np.arange(L, dtype=np.int32)[None, :]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for key, A in (("seq1", A1), ("seq2", A2)):
        a = np.frombuffer(A, dtype=np.uint8)
        m = len(a)
        has = rng.random(n) < frac
        tail = rng.random(n) < 0.33
        p = np.where(tail, L - rng.integers(4, 21, n), rng.integers(20, L - 4, n)).astype(np.int32)[:, None]
        sub = np.where(rng.random(n) < 0.3, p[:, 0] + rng.integers(0, m, n), -1).astype(np.int32)[:, None]
        seq = d[key]
        body = a[np.clip(j - p, 0, m - 1)]
        behind = letters[rng.integers(0, 4, (n, L))]
        new = np.where(j < p, seq, np.where(j < p + m, body, behind))
        new = np.where((j == sub) & (j >= p) & (j < p + m), letters[(np.searchsorted(letters, np.minimum(new, 84)) + 1) % 4], new)
        d[key] = np.where(has[:, None], new, seq).astype(np.uint8)
    return d


def kernels(a):
    import numpy as np
    from afterqc_amd import capi
    plain, adp = capi.Engine(0, 1), capi.Engine(0, 1)
    print("# adapter_bench kernels on %s: %d records, %d warm-up + %d timed aqc_run per context, alternating; -f 0 -t 0, `adapter` with both adapters (33 bases, min overlap 4)"
          % (plain.device_name(), a.records, a.warmup, a.reps), flush=True)
    print("# %-6s %-8s %5s %10s %9s %7s %9s | %10s %9s %8s" % ("load", "ctx", "words", "verdict_ms", "min_ms", "max/min", "deferred", "adapter_ms", "min_ms", "of_peak"))
    for load, (L, paired) in LOADS.items():
        batch = batch_of(make_input(a.records, L), paired)
        engines = (("plain", plain), ("adapter", adp))
        for tag, eng in engines:
            vb.prepare(eng, batch, paired, lambda e: e.set_adapter_trim(capi.AdapterConfig(A1, A2 if paired else b"", 4) if tag == "adapter" else None))
        ms, ams = vb.alternate(engines, a, "adapter", lambda eng: eng.adapter_ms(0))
        vb.verdict_rows(engines, ms, ams, "adapter", load, batch.n, moved_bytes(L, paired, batch.n), 8, 10)
        st = adp.adapter_stats() // (a.warmup + a.reps)
        print("  %-6s the CUT instance takes %.3f x the plain instance's time (medians); adapter pass + CUT instance %.4f ms against %.4f ms; reads trimmed %d + %d of %d records, bases %d + %d"
              % (load, float(np.median(ms["adapter"]) / np.median(ms["plain"])), float(np.median(ms["adapter"]) + np.median(ams)), float(np.median(ms["plain"])),
                 int(st[0]), int(st[2]), batch.n, int(st[1]), int(st[3])), flush=True)
    plain.close()
    adp.close()


def early_exit(a):
    import numpy as np
    from afterqc_amd import capi
    eng = capi.Engine(0, 1)
    L, paired = LOADS["pe150"]
    print("# adapter_bench exit on %s: %d pairs of 2 x 150, the adapter pass (aqc_adapter_ms), %d warm-up + %d timed aqc_run" % (eng.device_name(), a.records, a.warmup, a.reps), flush=True)
    for frac in (0.0, 0.3, 1.0):
        batch = batch_of(make_input(a.records, L, frac), paired)
        vb.prepare(eng, batch, paired, lambda e: e.set_adapter_trim(capi.AdapterConfig(A1, A2, 4)))
        v, = vb.pass_times([(eng, lambda e: e.adapter_ms(0))], a)
        st = eng.adapter_stats() // (a.warmup + a.reps)
        print("  adapter in %3d %% of the reads: adapter_ms median %.4f min %.4f  of_peak %.4f  reads trimmed %d + %d"
              % (round(100 * frac), float(np.median(v)), float(v.min()), vb.of_peak(moved_bytes(L, paired, batch.n), float(np.median(v))), int(st[0]), int(st[2])), flush=True)
    eng.close()


def step(a):
    from afterqc_amd import capi
    vb.step(a, lambda L: make_input(a.records, L), "this adapter" if a.adapter else "this",
            lambda eng: eng.set_adapter_trim(capi.AdapterConfig(A1, A2, 4) if a.adapter else None), "adapter_ms")


def once(a):
    from afterqc_amd import capi
    L, paired = LOADS[a.load]
    vb.once(a, make_input(a.records, L), paired, lambda eng: eng.set_adapter_trim(capi.AdapterConfig(A1, A2 if paired else b"", 4)), "adapter_ms")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("kernels", "exit", "step", "once"):
        p = sub.add_parser(name)
        p.add_argument("--records", type=int, default=1000000)
        p.add_argument("--warmup", type=int, default=3)
        p.add_argument("--reps", type=int, default=10)
        if name == "step":
            p.add_argument("--adapter", action="store_true")
        if name == "once":
            p.add_argument("load", choices=sorted(LOADS))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    {"kernels": kernels, "exit": early_exit, "step": step, "once": once}[a.cmd](a)


if __name__ == "__main__":
    main()
