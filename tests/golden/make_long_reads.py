#!/usr/bin/env python3
"""Generate tests/golden/long_reads_cases.json.gz by running the REAL reference on the inputs of long_cases.py: mates of
289 - 320 bases, which no other fixture reaches (function_vectors stop at 160 bases, e2e_cases at 2 x 250).

Like make_golden.py it runs only where the reference is present, imports it under the same shim (make_golden.install_shim) and
refuses to run otherwise; what it writes is data: the reference's answers and output digests, and one digest per input set.

    python tests/golden/make_long_reads.py
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import long_cases
import make_golden


def function_vectors():
    make_golden.install_shim()
    import preprocesser
    import util
    out = {}
    pairs = long_cases.overlap_pairs()
    out["overlap_digest"] = long_cases.digest(pairs)
    out["overlap"] = [list(util.overlap(r1, r2)) for _, r1, r2 in pairs]
    poly = long_cases.polyx_vectors()
    out["polyx_digest"] = long_cases.digest(poly)
    out["polyx"] = [preprocesser.hasPolyX(s, mp, mm) for s, mp, mm in poly]
    cnt = long_cases.count_vectors()
    out["counts_digest"] = long_cases.digest(cnt)
    out["counts"] = [[preprocesser.lowQualityNum(["@n", s, "+", q], qv), preprocesser.nNumber(["@n", s, "+", q])] for s, q, qv in cnt]
    return out


def main():
    if not os.path.isdir(make_golden.REF):
        print("reference not present at %s: golden vectors can only be regenerated in the build container" % make_golden.REF)
        sys.exit(2)
    out = {"func": function_vectors(), "e2e": {}}
    print("function vectors:", {k: len(v) for k, v in out["func"].items() if not k.endswith("_digest")})
    for name, argv, sp in long_cases.CASES:
        rec = make_golden.run_case(name, argv, lambda work, sp=sp: long_cases.materialize(sp, work))
        rec.pop("report", None)
        out["e2e"][name] = rec
        s = rec["stat"]["afterqc_main_summary"]
        print(name, {k: s[k] for k in ("total_reads", "good_reads", "bad_reads")})
    path = os.path.join(HERE, "long_reads_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
