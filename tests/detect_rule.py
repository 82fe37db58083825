"""The specification of finding a mate's adapter in the pass-1 sample (--adapter_sequence auto / --adapter_sequence_r2 auto), as
plain python.  Upstream has no such step: this file is the rule.

A fixed table of candidates, column 1 searched in read 1's sample and column 2 in read 2's.  A candidate's probe is its first
PROBE_LEN bases.  A read HOLDS a probe when the 12 bytes stand somewhere in its raw sequence line (the line before -f / -t), byte for
byte: any place 0 .. n - 12, an N or a lower-case letter is no match, a read under 12 bases holds nothing, a read that holds a
probe twice counts once for it, a read may count for several probes.  The sample is the set of reads pass 1 hands to statRead for
that file, S their number.  Each mate decides alone: the candidate with the largest count, the earlier row on a tie, is detected
when count >= MIN_READS and count * 1000 >= S * MIN_PER_MILLE; its full sequence is then the mate's adapter, used exactly as if
it had been given on the command line (tests/adapter_rule.py).  Otherwise nothing is detected and the mate is not searched.

holds / census / decide are the model; the rest are the helpers the tests share (a brute-force restatement, seeded reads that hold
no probe, the named placements of the GPU test)."""
import random

PROBE_LEN = 12
MIN_READS = 10
MIN_PER_MILLE = 1
MAX_PROBES = 16

# name, read 1's adapter, read 2's adapter
CANDIDATES = [
    ("illumina_truseq", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"),
    ("nextera", b"CTGTCTCTTATACACATCT", b"CTGTCTCTTATACACATCT"),
    ("illumina_small_rna", b"TGGAATTCTCGGGTGCCAAGG", b"GATCGTCGGACTGTAGAACTCTGAAC"),
    ("bgi_mgi", b"AAGTCGGAGGCCAAGCGGTCTTAGGAAGACAA", b"AAGTCGGATCGTAGCCATGTCGTTCTGTGAGCCAAGGAGTTG"),
]


def column(mate):
    return [row[1 + mate] for row in CANDIDATES]


def probes(mate):
    return [a[:PROBE_LEN] for a in column(mate)]


def holds(s, probe):
    """does the read's raw sequence line s (bytes) hold the probe?"""
    return any(s[p:p + PROBE_LEN] == probe for p in range(0, len(s) - PROBE_LEN + 1))


def holds_brute(s, probe):
    """the same restated with explicit indices, from the back, without slices"""
    n = len(s)
    found = False
    p = n - 1
    while p >= 0:
        if p + len(probe) <= n:
            same = 0
            for j in range(len(probe)):
                if s[p + j] == probe[j]:
                    same += 1
            if same == len(probe):
                found = True
        p -= 1
    return found


def census(reads, probe_list):
    """aqc_get_adapter_census of the reads: [reads looked at, reads holding probe 0, probe 1, ...]"""
    out = [0] * (1 + len(probe_list))
    for s in reads:
        out[0] += 1
        for i, p in enumerate(probe_list):
            out[1 + i] += p in s                # (holds(s, p), by bytes' own search: the tests' batches are megabytes)
    return out


def decide(counts, sampled):
    """counts per candidate in table order, the sample's size -> the row detected, None: none"""
    if not counts:
        return None
    best = max(range(len(counts)), key=lambda i: (counts[i], -i))
    c = counts[best]
    return best if c >= MIN_READS and c * 1000 >= sampled * MIN_PER_MILLE else None


def decide_brute(counts, sampled):
    """the same from the back: the earliest row with the largest count is the last one noted"""
    best = None
    for i in range(len(counts) - 1, -1, -1):
        if best is None or counts[i] >= counts[best]:
            best = i
    if best is None or counts[best] < MIN_READS:
        return None
    return best if sampled <= 1000 * counts[best] // MIN_PER_MILLE else None


def detect(reads, mate):
    """what the statistics JSON says of one asked mate"""
    c = census(reads, probes(mate))
    row = decide(c[1:], c[0])
    return {"sampled": c[0], "candidates": [[CANDIDATES[i][0], c[1 + i]] for i in range(len(CANDIDATES))],
            "detected": None if row is None else CANDIDATES[row][0], "adapter": "" if row is None else column(mate)[row].decode()}


# ---- seeded inputs
def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def make_probes(rng, k, share=()):
    """k different probes; share: (i, j, nbytes) makes probe j start with the first nbytes bytes of probe i"""
    out = []
    while len(out) < k:
        p = bases(rng, PROBE_LEN)
        if p not in out:
            out.append(p)
    for i, j, nb in share:
        other = bytes(b for b in b"ACGT" if b != out[i][nb])            # (they share exactly nb bytes)
        out[j] = out[i][:nb] + bytes([rng.choice(other)]) + bases(rng, PROBE_LEN - nb - 1)
    assert len(set(out)) == k
    return out


def clean_read(rng, n, probe_list):
    """n random bases that hold none of the probes"""
    while True:
        s = bases(rng, n)
        if not any(holds(s, p) for p in probe_list):
            return s


def plant(s, p, what):
    """`what` written over s from place p on (cut at the read's end)"""
    return (s[:p] + what + s[p + len(what):])[:len(s)]


def spoil(s, p, byte):
    """the byte at place p made an N (byte "N") or lower case (byte "l")"""
    b = b"N" if byte == "N" else s[p:p + 1].lower()
    return s[:p] + b + s[p + 1:]


def placements(rng, n, probe_list):
    """(tag, read of n bytes) over the named places of the probes on a read that holds none by chance: every place mod 16, every
    lane border of the device pass (16 g - 11 .. 16 g + 1), the read's two ends and one place too far, spoiled bytes, a probe
    twice, two probes"""
    k = len(probe_list)
    pick = lambda i: probe_list[i % k]
    base = clean_read(rng, n, probe_list)
    yield "clean", base
    if n < PROBE_LEN:
        yield "prefix", pick(n)[:n]                                  # the whole read is the probe's start: holds nothing
        return
    last = n - PROBE_LEN
    places = set(range(0, min(last, 33) + 1)) | {last}
    for g in range(1, n // 16 + 1):
        places |= {p for p in range(16 * g - 11, 16 * g + 2) if 0 <= p <= last}
    for p in sorted(places):
        yield "at_%d" % p, plant(base, p, pick(p))
    yield "cut_%d" % (last + 1), plant(base, last + 1, pick(1))      # 11 of the 12 bytes at the tail: must not count
    for b in (0, 5, 11):
        p = min(last, 3 + b)
        yield "N_%d" % b, spoil(plant(base, p, pick(b)), p + b, "N")
        yield "lower_%d" % b, spoil(plant(base, p, pick(b)), p + b, "l")
    if n >= 2 * PROBE_LEN + 1:
        yield "twice", plant(plant(base, 0, pick(2)), last, pick(2))
        if k > 1:
            yield "two", plant(plant(base, 1, pick(0)), last, pick(1))
    if n >= PROBE_LEN + 4 and k > 1:
        yield "overlapping", plant(plant(base, 0, pick(0)), 4, pick(1))   # (the second overwrites the first's tail: one probe left)


PROBE_SETS = {1: (), 4: ((0, 1, 4), (2, 3, 8)), 16: ((0, 1, 4), (2, 3, 8), (4, 5, 11))}     # probes -> which of them share their first bytes


def seam_case(lengths, k, seed):
    """the batch of one case of the GPU seam test -> (probes, reads): k probes, every named placement at every length"""
    rng = random.Random(seed)
    probe_list = make_probes(rng, k, share=PROBE_SETS[k])
    return probe_list, [s for n in lengths for _, s in placements(rng, n, probe_list)]
