#!/usr/bin/env python3
"""Golden vectors for the debubble pre-pass, produced by the REAL reference (/root/reference, under the py3 shim of
make_golden.py) — run in the build container only:

    python tests/golden/make_debubble.py        ->  tests/golden/debubble_cases.json.gz

Each case is a folder of generated FASTQ files (kept in the fixture as text; .gz / .bz2 files are compressed again by the
test) run through the reference's debubble.debubbleDir(folder, 20, out, draw) the way after.runDebubble calls it
(after.py:177-184, with main's `except Exception`).  The fixture keeps upstream's list of output files and folders, the CSV
texts, whether circles.csv exists, the exception type (None, or ZeroDivisionError on the CircleDetector path) and, per
PNG, its size and the sha256 of its decoded RGB pixels.  Files of a folder are listed in sorted order (os.listdir's
order depends on the file system, and the records of several files are joined in that order); the tests list them so too.  Names that would make upstream's census child raise (and the
parent hang in queue.get()) are kept out.  Nothing of the reference is copied."""
import gzip
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = make_golden.REF


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def poly(rng, L, base, run, at=None):
    s = list(rseq(rng, L))
    at = rng.randrange(0, L - run + 1) if at is None else at
    for i in range(at, at + run):
        s[i] = base
    # keep the run exactly `run` long
    if at > 0 and s[at - 1] == base:
        s[at - 1] = "C" if base != "C" else "A"
    if at + run < L and s[at + run] == base:
        s[at + run] = "C" if base != "C" else "A"
    return "".join(s)


def rec(name, seq):
    return "%s\n%s\n+\n%s\n" % (name, seq, "F" * len(seq))


def illumina(lane, tile, x, y, mate=1):
    return "@SIM:7:FCX:%d:%d:%d:%d %d:N:0:ACGT" % (lane, tile, x, y, mate)


def random_reads(rng, n, lanes=(1,), tiles=(1101, 1102, 1103), frac=0.06, L=100):
    out = []
    for i in range(n):
        name = illumina(rng.choice(lanes), rng.choice(tiles), rng.randrange(1000, 20000), rng.randrange(1000, 19000))
        if rng.random() < frac:
            seq = poly(rng, L, rng.choice("ATCG"), rng.randrange(20, min(60, L)))
        else:
            seq = rseq(rng, L)
        out.append(rec(name, seq))
    return out


def bubble_reads(rng, n, lane, tile, cx, cy, r=250, L=100):
    out = []
    for i in range(n):
        x = cx + rng.randrange(-r, r)
        y = cy + rng.randrange(-r, r)
        out.append(rec(illumina(lane, tile, x, y), poly(rng, L, "G", 40)))
    return out


def make_cases():
    rng = random.Random(20261016)
    cases = []
    cases.append(dict(name="no_bubble", draw=True, files={"S_R1.fq": "".join(random_reads(rng, 1500))}))
    body = random_reads(rng, 1500, tiles=(1101, 1102, 1103, 1104))
    body += bubble_reads(rng, 400, 1, 1102, 9000, 9000)
    rng.shuffle(body)
    cases.append(dict(name="bubble", draw=True, files={"S_R1.fq": "".join(body)}))
    cases.append(dict(name="lanes_surfaces", draw=True, files={
        "A_R1.fq": "".join(random_reads(rng, 900, lanes=(1, 2), tiles=(11101, 21101, 11102, 21102, 12101), frac=0.1, L=120)),
        "A_R2.fq": "".join(random_reads(rng, 500, lanes=(2, 3), tiles=(11101, 21101, 22103), frac=0.1, L=120))}))
    many = {}
    for fn in ("B_R1.fq.gz", "B_R2.fq.bz2", "B_I1.fastq", "Undetermined_R1.fq", "notes.txt"):
        many[fn] = "".join(random_reads(rng, 250, lanes=(1, 3), tiles=(1101, 1205, 2101), frac=0.1, L=rng.choice([50, 101])))
    cases.append(dict(name="many_files", draw=True, files=many))
    reads = random_reads(rng, 300, frac=0.2)
    cases.append(dict(name="blank_line", draw=False, files={"C_R1.fq": "".join(reads[:150]) + "\n" + "".join(reads[150:])}))
    # runs near the threshold, several bases, lowercase, N
    edge = []
    L = 90
    specials = [
        poly(rng, L, "A", 19), poly(rng, L, "A", 20), poly(rng, L, "T", 21), poly(rng, L, "G", 19) + "",
        "C" * 20 + rseq(rng, 10) + "A" * 20 + rseq(rng, 10),           # A wins over an earlier C
        "T" * 25 + "GATC" + "A" * 20 + "C",                              # A wins over an earlier T
        "T" * 19 + "G" + "T" * 22 + "CG",                                 # the second T run is the first of >= 20
        "a" * 30 + rseq(rng, 20), "N" * 40 + rseq(rng, 10), "G" * 120, "GGGGGGGGGG" + "g" * 10 + "GGGGGGGGGG",
        "A" * 20, "C" * 20 + "A" * 19 + "G" * 21, "T" * 200, "A" * 45 + "N" + "A" * 21,
    ]
    for i, s in enumerate(specials * 6):
        edge.append(rec(illumina(1 + i % 2, 1101 + (i % 3), 100 + 37 * i, 200 + 53 * i), s))
    cases.append(dict(name="runs", draw=True, files={"E_R1.fq": "".join(edge)}))
    names = []
    for i in range(60):
        s = poly(rng, 80, "G", 30 + i % 5)
        nm = [
            "@read_%d" % i,                                                    # not Illumina: skipped
            "@SIM:7:FCX:2:11101:%d:%d:9 1:N:0:ACGT" % (500 + i, 700 + i),     # an extra field behind y
            "@SIM:7:FCX:2:11101:%d:%d 1:N:0:AC:GT:TT" % (500 + i, 900 + i),   # colons in the comment
            "@SIM:7:FCX:1:2101:%d:%d" % (500 + i, 900 + i),
            "@SIM 7:FCX:3:1101:1:2:3",                                         # the match is in the comment
        ][i % 5]
        names.append(rec(nm, s))
    cases.append(dict(name="names", draw=True, files={"N_R1.fq": "".join(names)}))
    return cases


def write_inputs(folder, files):
    import bz2
    for fn, text in files.items():
        p = os.path.join(folder, fn)
        if fn.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(text.encode())
        elif fn.endswith(".bz2"):
            with bz2.open(p, "wb") as f:
                f.write(text.encode())
        else:
            with open(p, "w") as f:
                f.write(text)


def outputs(out):
    from PIL import Image
    res = dict(dirs=[], files={}, images={})
    if not os.path.exists(out):
        return res
    for root, dirs, files in os.walk(out):
        rel = os.path.relpath(root, out)
        for d in dirs:
            res["dirs"].append(os.path.normpath(os.path.join(rel, d)))
        for f in files:
            p = os.path.join(root, f)
            k = os.path.normpath(os.path.join(rel, f))
            if f.endswith(".png"):
                im = Image.open(p).convert("RGB")
                res["images"][k] = dict(size=list(im.size), sha256=hashlib.sha256(im.tobytes()).hexdigest())
            else:
                res["files"][k] = open(p).read()
    res["dirs"].sort()
    return res


RUNNER = r"""
import sys, json
sys.path.insert(0, %r)
import make_golden
make_golden.install_shim()
import os
_listdir = os.listdir
os.listdir = lambda p=".": sorted(_listdir(p))     # one listing order for the fixture (os.listdir's own depends on the file system)
import debubble
err = None
try:
    debubble.debubbleDir(sys.argv[1], 20, sys.argv[2], sys.argv[3] == "1")
except Exception as e:
    err = type(e).__name__
json.dump({"exception": err}, open(sys.argv[4], "w"))
"""


def run_case(case):
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "in")
        os.makedirs(folder)
        write_inputs(folder, case["files"])
        out = os.path.join(tmp, "debubble")
        res = os.path.join(tmp, "res.json")
        subprocess.run([sys.executable, "-c", RUNNER % HERE, folder, out, "1" if case["draw"] else "0", res], cwd=tmp,
                       check=True, timeout=600, stdout=subprocess.DEVNULL)
        got = outputs(out)
        got["exception"] = json.load(open(res))["exception"]
        got["circles"] = "circles.csv" in got["files"]
        return got


def main():
    if not os.path.isdir(REF):
        sys.exit("make_debubble.py needs the reference at %s" % REF)
    cases = make_cases()
    for c in cases:
        c["expect"] = run_case(c)
        print(c["name"], c["expect"]["exception"], sorted(c["expect"]["files"]), sorted(c["expect"]["images"]))
    with gzip.open(os.path.join(HERE, "debubble_cases.json.gz"), "wt") as f:
        json.dump(cases, f)


if __name__ == "__main__":
    main()
