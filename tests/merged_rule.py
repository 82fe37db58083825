"""The --store_merged rule, stated once for the fixture script (tests/golden/make_merged.py, which applies it to the REFERENCE's
good and overlap files) and for the tests (which apply it to inputs of their own): a pair that upstream writes to the overlap
files goes out once, as

    name line : read 1's, as written to good
    sequence  : s1 + reverseComplement(s2[0:p])      p = len(s2) - overlap_len
    plus line : read 1's
    quality   : q1 + reversed(q2[0:p])

with s, q the lines of the good files; a pair with a mate whose quality line is not as long as its sequence line is left out."""
import gzip
import hashlib
import json
import os

import cases

COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "a": "t", "t": "a", "c": "g", "g": "c", "N": "N"}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merged_cases.json.gz")

# the cases of the fixture: those of tests/golden/cases.py by name, and one of this file's — pairs with adapter read-through (40 % of
# the inserts are shorter than the read: read 2 ends inside read 1, p == 0)
CASE_NAMES = ["pe_store_overlap", "pe_default", "pe_trim_explicit", "pe_trim_pair_diff", "pe_barcode", "pe_barcode_tails", "pe_mask",
              "pe_nocorr", "pe_ragged", "pe_ragged_short", "pe_l250", "pe_lowercase", "pe_gz_out", "pe_nooverlap"]
ADAPTER_CASE = ("pe_adapter", cases.PE + cases.F0, cases.pe(1401, n=1500, short_frac=0.4), False)


def case_table():
    """name -> (name, argv, input spec, keep flag), as cases.CASES has them"""
    table = {c[0]: c for c in cases.CASES if c[0] in CASE_NAMES}
    table[ADAPTER_CASE[0]] = ADAPTER_CASE
    return table


def reverse_complement(s):
    return "".join(COMP.get(c, "N") for c in reversed(s))


def merged_record(name1, s1, plus1, q1, s2, q2, ovl):
    """the merged read of one pair (text lines without their newlines), or None for an irregular pair"""
    if len(q1) != len(s1) or len(q2) != len(s2):
        return None
    p = len(s2) - ovl
    assert p >= 0
    return "%s\n%s\n%s\n%s\n" % (name1, s1 + reverse_complement(s2[0:p]), plus1, q1 + q2[0:p][::-1])


def records(text):
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0, "not whole four-line records"
    return [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]


def merged_from_outputs(good1, good2, overlap1):
    """good1, good2: the text of the two good files; overlap1: the text of read 1's overlap file.  The overlap records are matched
    to the good pairs in order and by name line, overlap_len is the length of the overlap record's sequence.
    -> (text of the merged file, counts: merged / irregular (left out) / p == 0 / len(s2) != len(s1) among the merged)"""
    g1, g2, ov = records(good1), records(good2), records(overlap1)
    assert len(g1) == len(g2)
    out = []
    counts = {"merged": 0, "irregular": 0, "p0": 0, "len_diff": 0}
    k = 0
    for a, b in zip(g1, g2):
        if k == len(ov) or ov[k][0] != a[0]:
            continue
        ovl = len(ov[k][1])
        k += 1
        rec = merged_record(a[0], a[1], a[2], a[3], b[1], b[3], ovl)
        if rec is None:
            counts["irregular"] += 1
            continue
        out.append(rec)
        counts["merged"] += 1
        counts["p0"] += 1 if len(b[1]) == ovl else 0
        counts["len_diff"] += 1 if len(b[1]) != len(a[1]) else 0
    assert k == len(ov), "overlap records without a good pair of their name: %d of %d matched" % (k, len(ov))
    return "".join(out), counts


def digest_bytes(data):
    return {"sha256": hashlib.sha256(data).hexdigest(), "lines": data.count(b"\n"), "bytes": len(data)}


def read_maybe_gz(path):
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        return f.read()


def load_fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def child_main(argv):
    """`python tests/merged_rule.py WORKDIR KWARGS_JSON argv...`: the CLI's filter on the HIP engine in a process of its own (the
    tests that set AQC_SPANS / AQC_FUSED in the child's environment), seqFilter keywords from KWARGS_JSON -> prints used_pipe"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from afterqc_amd import after, preprocesser
    os.chdir(argv[0])
    kw = json.loads(argv[1])
    options, _ = after.parseCommand(list(argv[2:]))
    after.finalize_options(options)
    options.barcode = False
    flt = preprocesser.seqFilter(options, **kw)
    flt.run()
    print("used_pipe=%d" % (1 if flt.used_pipe else 0))


if __name__ == "__main__":
    import sys
    child_main(sys.argv[1:])
