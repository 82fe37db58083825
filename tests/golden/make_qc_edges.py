#!/usr/bin/env python3
"""Golden vectors for QualityControl.statRead and fastq.Reader at byte edges, produced by the REAL reference (/root/reference,
under the py3 shim of make_golden.py) — run in the build container only:

    python tests/golden/make_qc_edges.py        ->  tests/golden/qc_edges.json.gz

"stat": hand-built reads (the same list for every k in 1..8) whose lines end in a printable byte, so that line stripping stays
out of them:
  - quality bytes 0x00-0x20 (not '\\n') and 0x7f-0xff INSIDE the line: qualNum is ord(q) - 33 (util.py:39-40), negative for the
    low ones;
  - sequences with NUL runs of length >= k (a zero-filled block of a damaged file): the all-NUL k-mer is counted like any other;
  - IUPAC letters, '.', lowercase and high bytes in the sequence;
  - reads of length 5, k and k+1.
For every k the fixture keeps the accumulators statRead fills (trimmed to the longest read) and the k-mer dict in insertion order.

"reader": fastq.Reader.nextRead on two-record files whose sequence and quality lines end in one byte 0x00-0x20 (before the
'\\n'), read twice: as the shim runs the reference (text mode: str.rstrip, which also strips 0x1c-0x1f) and over a binary file
object (bytes.rstrip: space \\t \\n \\v \\f \\r, what the python 2 program does).  Kept: the lengths of the lines of each record.
tests/test_qc_edges.py pins the oracle to this fixture on the CPU; tests/test_gpu_qc_scale.py runs the reads on the device."""
import gzip
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

OUT = os.path.join(HERE, "qc_edges.json.gz")
SEED = 20261016


def edge_reads():
    """[(seq, qual)] as latin-1 strings (one char per byte)"""
    rng = random.Random(SEED)
    acgt = "ACGT"

    def bases(n):
        return "".join(rng.choice(acgt) for _ in range(n))

    def quals(n):
        return "".join(rng.choice("#+5?FIJ") for _ in range(n))

    reads = []
    # quality bytes below '!' (not '\n') and 0x7f-0xff inside the line, scattered and in runs
    low = [chr(b) for b in range(0x00, 0x21) if b != 0x0a]
    high = [chr(b) for b in range(0x7f, 0x100)]
    bad = low + high
    for i in range(0, len(bad), 8):
        L = 48
        q = list(quals(L))
        for p, c in zip(rng.sample(range(L - 1), 8), bad[i:i + 8]):
            q[p] = c                                # (never the last byte)
        reads.append((bases(L), "".join(q)))
    reads.append((bases(len(low) + 1), "".join(low) + "I"))       # every low byte in one run
    reads.append((bases(41), "!" * 10 + "\x20\x01\x1f\x00" * 5 + "!" * 10 + "J"))
    reads.append((bases(33), "\x7f\x80\xfe\xff" * 8 + "5"))
    # NUL runs of length >= k in the sequence
    for run in (1, 2, 4, 5, 8, 9, 12, 17):
        reads.append((bases(10) + "\x00" * run + bases(20), quals(30 + run)))
    reads.append(("\x00" * 30 + "A", quals(31)))
    reads.append(("\x00" * 8 + "C" + "\x00" * 8 + "G", quals(18)))
    # IUPAC letters, '.', lowercase, high bytes
    iupac = "NRYKMSWBDHVN.acgtnrykmswbdhv"
    for _ in range(6):
        s = list(bases(40))
        for _ in range(8):
            s[rng.randrange(0, 39)] = rng.choice(iupac)
        reads.append(("".join(s), quals(40)))
    reads.append(("".join(rng.choice(iupac) for _ in range(36)) + "T", quals(37)))
    reads.append(("\x80\xff\xc3\xa9ACGT\x90" * 4 + "G", quals(37)))
    reads.append(("NNNNNNNNNNNNNNNNNNNNNNNN", quals(24)))
    # short reads: 5, k and k + 1 for every k (statRead raises IndexError below 5 bases)
    for L in sorted({5, 6, 7, 8, 9}):
        reads.append((bases(L), quals(L)))
        reads.append(("N" * (L - 1) + "A", quals(L)))
        reads.append(("\x00" * (L - 1) + "G", quals(L)))
    return reads


def capture_stat(reads, k):
    import qualitycontrol
    qc = qualitycontrol.QualityControl(qc_sample=1 << 30, qc_kmer=k)
    for s, q in reads:
        qc.statRead(["@r", s, "+", q])
    n = max(len(s) for s, _ in reads)
    return {
        "total_num": qc.totalNum[:n],
        "total_qual": qc.totalQual[:n],
        "base_count": {b: qc.baseCounts[b][:n] for b in "ATCG"},
        "base_qual": {b: qc.baseTotalQual[b][:n] for b in "ATCG"},
        "discontinuity": [int(x) for x in qc.totalDiscontinuity[:n]],
        "gc_hist": qc.gcHistogram[:n + 1],
        "total_kmer": qc.totalKmer,
        "kmers": [[km, c] for km, c in qc.kmerCount.items()],       # dict insertion order
    }


def capture_reader():
    import fastq
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for b in range(0x00, 0x21):
            c = bytes([b])
            text = b"@r1\nACGTACGTAC" + c + b"\n+\nIIIIIIIIII" + c + b"\n@r2\nGATTACA\n+\nFFFFFFF\n"
            fn = os.path.join(tmp, "e%02x.fq" % b)
            with open(fn, "wb") as f:
                f.write(text)
            got = {"byte": b}
            for mode in ("text", "binary"):
                r = fastq.Reader(fn)
                if mode == "binary":
                    r._Reader__file.close()
                    r._Reader__file = open(fn, "rb")
                recs = []
                while True:
                    rec = r.nextRead()
                    if rec is None:
                        break
                    recs.append([len(x) for x in rec])
                del r
                got[mode] = recs
            out.append(got)
    return out


def main():
    if not os.path.isdir(make_golden.REF):
        sys.exit("the reference is not here: nothing to regenerate")
    make_golden.install_shim()
    reads = edge_reads()
    data = {"reads": [[s, q] for s, q in reads],
            "stat": {str(k): capture_stat(reads, k) for k in range(1, 9)},
            "reader": capture_reader()}
    raw = json.dumps(data, sort_keys=True).encode()
    with open(OUT, "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
            g.write(raw)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(reads), "reads")


if __name__ == "__main__":
    main()
