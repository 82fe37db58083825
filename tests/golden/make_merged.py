#!/usr/bin/env python3
"""tests/golden/merged_cases.json.gz: what --store_merged must write, derived from the REAL reference's own outputs.

Per case (tests/merged_rule.py: the cases of cases.py by name, and one with adapter read-through) the reference runs — in a
subprocess, through make_golden.py's --run-ref driver and shim — with `--store_overlap on` added to the case's argv; the merged
file is then put together from its good files and read 1's overlap file by merged_rule.merged_from_outputs.  Recorded: sha256 /
bytes / lines of the merged text, the number of merged pairs, of pairs left out as irregular, of merged pairs with p == 0 and
with mates of different lengths, and the argv and input spec the tests rebuild the inputs from.  Nothing of the reference is
copied; the script refuses to run where the reference is absent.

    python tests/golden/make_merged.py
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases            # noqa: E402
import make_golden      # noqa: E402
import merged_rule      # noqa: E402


def only_file(folder, marker):
    names = [fn for fn in sorted(os.listdir(folder)) if marker in fn]
    assert len(names) == 1, (folder, marker, names)
    return merged_rule.read_maybe_gz(os.path.join(folder, names[0])).decode("latin-1")


def run_case(name, argv, spec):
    work = tempfile.mkdtemp(prefix="aqc_merged_")
    try:
        cases.materialize(spec, work)
        p = subprocess.run([sys.executable, os.path.join(HERE, "make_golden.py"), "--run-ref"] + list(argv) + ["--store_overlap", "on"],
                           cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            print(p.stdout[-3000:])
            raise RuntimeError("reference failed on case " + name)
        r1 = merged_rule_main_name(argv[argv.index("-1") + 1])
        r2 = merged_rule_main_name(argv[argv.index("-2") + 1])
        good1 = only_file(os.path.join(work, "good"), r1 + ".good")
        good2 = only_file(os.path.join(work, "good"), r2 + ".good")
        ovl1 = only_file(os.path.join(work, "overlap"), r1 + ".overlap")
        text, counts = merged_rule.merged_from_outputs(good1, good2, ovl1)
        rec = merged_rule.digest_bytes(text.encode("latin-1"))
        rec.update(counts)
        rec.update({"argv": list(argv), "spec": spec, "overlap_records": len(merged_rule.records(ovl1))})
        return rec
    finally:
        shutil.rmtree(work, ignore_errors=True)


def merged_rule_main_name(fn):
    base = os.path.basename(fn)
    for ext in (".fastq", ".fq", ".gz"):
        base = base.replace(ext, "")
    return base


def main():
    if not os.path.isdir(make_golden.REF):
        print("reference not present at %s: the fixture can only be regenerated in the build container" % make_golden.REF)
        sys.exit(2)
    out = {}
    for name, (_, argv, spec, _) in merged_rule.case_table().items():
        rec = out[name] = run_case(name, argv, spec)
        print(name, {k: rec[k] for k in ("overlap_records", "merged", "irregular", "p0", "len_diff", "bytes")})
        # no case passes vacuously
        if name == "pe_nooverlap":
            assert rec["merged"] == 0 and rec["bytes"] == 0, rec
        else:
            assert rec["merged"] >= 50, (name, rec["merged"])
        if name == merged_rule.ADAPTER_CASE[0]:
            assert rec["p0"] >= 10, (name, rec["p0"])
        if name == "pe_ragged_short":
            assert rec["len_diff"] >= 10, (name, rec["len_diff"])
    assert set(out) == set(merged_rule.CASE_NAMES) | {merged_rule.ADAPTER_CASE[0]}
    with gzip.open(merged_rule.FIXTURE, "wt") as f:
        json.dump(out, f, sort_keys=True)


if __name__ == "__main__":
    main()
