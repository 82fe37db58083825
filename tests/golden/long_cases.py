"""Inputs of the fixtures above 250 bases (tests/golden/long_reads_cases.json.gz): mates of 289 - 320 bases, the lengths
of the verdict kernel's 20-word tier, and one case a base over it.

Everything is rebuilt from seeds (numpy's PCG64 and afterqc_amd.synth), so make_long_reads.py (the reference's run) and the
tests (ours) see byte-identical inputs and the fixture holds results only, plus one digest per input set that the tests check
first.  The alphabet stays within what the reference survives: A C G T N and lower-case a c g t (util.py:27; no 'n').
"""
import hashlib
import os

import numpy as np

from afterqc_amd import synth

LO, HI = 289, 320          # the tier's lengths
_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "a": "t", "t": "a", "c": "g", "g": "c"}
_NEXT = {"A": "C", "C": "G", "G": "T", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def _seq(rng, n):
    return synth.BASES[rng.integers(0, 4, n, dtype=np.uint8)].tobytes().decode()


def _mutate(rng, s, k, to=None):
    """k distinct positions of s get another base (or `to`)"""
    s = list(s)
    for p in rng.choice(len(s), size=min(k, len(s)), replace=False):
        s[p] = to if to else "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4] if s[p] in "ACGT" else "A"
    return "".join(s)


def _pair(rng, L1, L2, ins):
    """mates of a fragment of `ins` bases; what lies past the fragment's end (adapter read-through) is random"""
    frag = _seq(rng, ins)
    return (frag + _seq(rng, L1))[:L1], (revcomp(frag) + _seq(rng, L2))[:L2]


def _flip(r1, cols, off):
    """substitutions in read 1 at the diagonal's columns `cols` (read 1 position off + column)"""
    r1 = list(r1)
    for c in cols:
        if 0 <= off + c < len(r1):
            r1[off + c] = _NEXT[r1[off + c]]
    return "".join(r1)


def overlap_pairs():
    """[(tag, r1, r2)] for util.overlap: about 2,000 pairs of 289 - 320 bases"""
    rng = np.random.Generator(np.random.PCG64(20261019))
    out = []
    ln = lambda: int(rng.integers(LO, HI + 1))
    # ---- general: every insert size, equal and unequal lengths, substitutions, N, lower case
    for _ in range(700):
        L1 = ln()
        L2 = L1 if rng.random() < 0.5 else ln()
        if rng.random() < 0.1:
            r1, r2 = _seq(rng, L1), _seq(rng, L2)
        else:
            r1, r2 = _pair(rng, L1, L2, int(rng.integers(40, L1 + L2 + 20)))
        r1 = _mutate(rng, r1, int(rng.choice([0, 0, 0, 1, 2, 3, 4, 6])))
        if rng.random() < 0.3:
            r2 = _mutate(rng, r2, int(rng.choice([1, 2, 3, 5])))
        if rng.random() < 0.2:
            r1 = _mutate(rng, r1, int(rng.integers(1, 7)), "N")
            r2 = _mutate(rng, r2, int(rng.integers(1, 7)), "N")
        if rng.random() < 0.08:
            k = int(rng.integers(1, L1)); r1 = r1[:k].lower().replace("n", "N") + r1[k:]
        if rng.random() < 0.08:
            k = int(rng.integers(1, L2)); r2 = r2[:k].lower().replace("n", "N") + r2[k:]
        out.append(("general", r1, r2))
    # ---- 320 / 289 and 289 / 320: read 2 inside read 1 (the tail-anchored walk of SURVEY App. B-6) and the other way round
    for (L1, L2) in ((320, 289), (289, 320)):
        for _ in range(120):
            off = int(rng.integers(0, 45))
            ins = max(L1, off + L2) if rng.random() < 0.7 else int(rng.integers(200, L1 + L2))
            frag = _seq(rng, max(ins, off + L2) + 40)
            r1 = frag[:L1]
            r2 = revcomp(frag[off:off + L2]) if rng.random() < 0.7 else (revcomp(frag[:ins]) + _seq(rng, L2))[:L2]
            r1 = _mutate(rng, r1, int(rng.choice([0, 1, 1, 2, 3])))
            r2 = _mutate(rng, r2, int(rng.choice([0, 0, 1, 2])))
            out.append(("unequal_%d_%d" % (L1, L2), r1, r2))
    # ---- full-length overlap at offset 0
    for _ in range(100):
        L = ln()
        r1, r2 = _pair(rng, L, L, L)
        out.append(("full", _mutate(rng, r1, int(rng.choice([0, 1, 2, 3, 5]))), r2))
    # ---- minimal overlap at the far end: 30 (too short) .. 34 bases, which lands in the scan's last word
    for _ in range(160):
        L1 = ln()
        L2 = L1 if rng.random() < 0.5 else ln()
        ov = int(rng.integers(30, 35))
        r1, r2 = _pair(rng, L1, L2, L1 + L2 - ov)
        cols = rng.choice(ov, size=int(rng.choice([0, 0, 1, 2, 3])), replace=False)
        out.append(("minimal_%d" % ov, _flip(r1, cols, L1 - ov), r2))
    # ---- inserts of 60 - 299 bases: adapter read-through, negative offsets, the second overlap call after the cut
    for _ in range(320):
        L1 = ln()
        L2 = L1 if rng.random() < 0.5 else ln()
        r1, r2 = _pair(rng, L1, L2, int(rng.integers(60, 300)))
        r1 = _mutate(rng, r1, int(rng.choice([0, 0, 1, 2, 3, 4])))
        if rng.random() < 0.3:
            r2 = _mutate(rng, r2, int(rng.choice([1, 2, 3])))
        if rng.random() < 0.1:
            r1 = _mutate(rng, r1, 2, "N")
        out.append(("readthrough", r1, r2))
    # ---- the third mismatch at exact columns of the accepted diagonal: 49 / 50 / 51 (complete_compare_require) and behind
    #      the 16-, 18- and 19-word marks
    third = (49, 50, 51, 255, 256, 257, 287, 288, 289, 303, 304, 305)
    firsts = ((0, 1), (10, 40), (47, 48), (3, 60), (100, 200), (254, 255), (48, 286))
    for (L, ov) in ((320, 320), (320, 310), (301, 301), (300, 296), (305, 305), (320, 306), (289, 289)):
        for t in third:
            for a, b in firsts:
                if not (a < b < t < ov):
                    continue
                r1, r2 = _pair(rng, L, L, 2 * L - ov)
                extra = (t + 1, t + 7) if rng.random() < 0.3 else ()
                out.append(("third_%d" % t, _flip(r1, (a, b, t) + tuple(c for c in extra if c < ov), L - ov), r2))
    # ... and the same columns on a reverse (negative) offset
    for t in third:
        for a, b in ((0, 1), (10, 40), (47, 48)):
            if not b < t:
                continue
            L = 320
            ins = int(rng.integers(max(t + 2, 120), L))          # the overlap is the insert: columns 0 .. ins - 1
            r1, r2 = _pair(rng, L, L, ins)
            out.append(("third_rev_%d" % t, _flip(r1, (a, b, t), 0), r2))
    return out


def polyx_vectors():
    """[(seq, maxPoly, mismatch)] for hasPolyX at 289 - 320 bases"""
    rng = np.random.Generator(np.random.PCG64(20261020))
    out = []
    params = ((35, 2), (20, 0), (10, 3), (50, 5), (31, 0), (40, 4))
    def run_at(L, end, k, ch, nmut=0):
        s = _seq(rng, L)
        s = s[:end - k] + ch * k + s[end:]
        if nmut:
            s = list(s)
            for p in rng.choice(np.arange(end - k + 1, end - 1), size=nmut, replace=False):
                s[p] = _NEXT[ch] if ch in _NEXT else "A"
            s = "".join(s)
        return s[:L]
    for mp, mm in params:
        need = mp - mm
        for L in (289, 300, 301, 304, 305, 317, 319, 320):
            for end in (304, 320, 303, 305, 319, 288, 289):
                if end > L:
                    continue
                for k in (need - 1, need, need + 1, mp, mp + 3):
                    # a run that ends exactly at base `end` (one base short, just enough, more)
                    out.append((run_at(L, end, k, "ACGTN"[int(rng.integers(0, 5))], 0), mp, mm))
                    if mm and k > mm + 2:
                        out.append((run_at(L, end, k, "ACGT"[int(rng.integers(0, 4))], mm), mp, mm))
            # a run inside word 18 or word 19 only (bases 288 .. 303 / 304 .. 319): too short for most settings, enough for (10, 3)
            for w0 in (288, 304):
                if w0 + 16 <= L:
                    for k in (7, 10, 16):
                        out.append((run_at(L, w0 + 16, min(k, 16), "ACGT"[int(rng.integers(0, 4))], 0), mp, mm))
    for _ in range(300):
        L = int(rng.integers(LO, HI + 1))
        s = _seq(rng, L)
        if rng.random() < 0.8:
            k = int(rng.integers(15, 90)); st = int(rng.integers(0, L - 10))
            s = (s[:st] + "ACGTNacgt"[int(rng.integers(0, 9))] * k + s[st:])[:L]
            s = _mutate(rng, s, int(rng.integers(0, 7))) if s.isupper() else s
        mp, mm = params[int(rng.integers(0, len(params)))]
        out.append((s, mp, mm))
    return out


def count_vectors():
    """[(seq, qual, qualified)] for lowQualityNum / nNumber at 289 - 320 bases, with more than 255 low-quality bases in some"""
    rng = np.random.Generator(np.random.PCG64(20261021))
    out = []
    for i in range(300):
        L = int(rng.integers(LO, HI + 1)) if i % 5 else (289, 304, 305, 320)[(i // 5) % 4]
        s = np.frombuffer(b"ACGTNN", dtype=np.uint8)[rng.integers(0, 6 if i % 3 == 0 else 5, L)].tobytes().decode()
        frac = (0.0, 0.3, 0.85, 0.97, 1.0)[i % 5]           # 0.85 and up: more than 255 of >= 300 bases
        q = np.where(rng.random(L) < frac, rng.integers(33, 48, L), rng.integers(48, 75, L)).astype(np.uint8).tobytes().decode()
        out.append((s, q, int(rng.choice([15, 15, 20, 0, 2, 30, 41]))))
    return out


def digest(vectors):
    h = hashlib.sha256()
    for v in vectors:
        h.update(repr(tuple(v)).encode())
    return h.hexdigest()


# ---- end-to-end cases: name, after.py argv, input spec ----------------------------------------------------------------------------------
PE = ["-1", "R1.fq", "-2", "R2.fq"]
BC = ["-1", "barcode_R1.fq", "-2", "barcode_R2.fq"]
F0 = ["-f", "0", "-t", "0"]


def spec(seed, n=600, L=301, **kw):
    d = dict(kind="pe", seed=seed, n=n, L=L, ragged=False, min_len=0, short_frac=0.03, barcode=False, r1="R1.fq", r2="R2.fq")
    d.update(kw)
    return d


CASES = [
    ("pe_l301", PE + F0, spec(3001)),
    ("pe_l301_default", PE, spec(3002)),
    # lengths 35 - 320: short and long records share chunks
    ("pe_l300_ragged", PE + F0 + ["-s", "20"], spec(3003, L=320, ragged=True, min_len=35)),
    ("pe_l300_adapters", PE + F0, spec(3004, L=300, short_frac=0.5)),
    ("pe_l300_mask", PE + F0 + ["--mask_mismatch"], spec(3005, L=300, short_frac=0.2)),
    # 2 x 300 plus the 12 + 5 base barcode / verify prefix: 317 bases, "barcode" in the file names (after.py:215-221)
    ("barcode_l317", BC + ["-t", "0"], spec(3006, L=300, barcode=True, r1="barcode_R1.fq", r2="barcode_R2.fq")),
    ("se_l320", ["-1", "R1.fq"] + F0, dict(kind="se", seed=3007, n=800, L=320)),
    # one base over the widest tier: stays on the general kernel
    ("pe_l321", PE + F0, spec(3008, n=400, L=321)),
]
CASE_TABLE = {c[0]: c for c in CASES}
MAX_LEN = {"pe_l301": 301, "pe_l301_default": 301, "pe_l300_ragged": 320, "pe_l300_adapters": 300, "pe_l300_mask": 300,
           "barcode_l317": 317, "se_l320": 320, "pe_l321": 321}


def pairs_of(sp):
    """the case's reads as synth matrices (the GPU tests upload them as packed batches too)"""
    if sp["kind"] == "se":
        return synth.make_single(sp["n"], sp["L"], sp["seed"])
    d = synth.make_pairs(sp["n"], sp["L"], sp["seed"], ragged=sp["ragged"], dirty=True, short_frac=sp["short_frac"])
    if sp["min_len"]:
        for m in ("len1", "len2"):
            d[m] = np.maximum(d[m], sp["min_len"]).astype(np.uint32)
    if sp["barcode"]:
        d = synth.add_barcodes(d, sp["seed"] + 7, tail_frac=0.1)
    return d


def materialize(sp, work):
    d = pairs_of(sp)
    lane, tile, x, y = d["meta"]
    if sp["kind"] == "se":
        synth.write_fastq(os.path.join(work, "R1.fq"), synth.render_names(lane, tile, x, y, 1), d["seq1"], d["qual1"], d["len1"])
        return
    for m, fn in ((1, sp["r1"]), (2, sp["r2"])):
        synth.write_fastq(os.path.join(work, fn), synth.render_names(lane, tile, x, y, m), d["seq%d" % m], d["qual%d" % m], d["len%d" % m])
