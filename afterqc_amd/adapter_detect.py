"""--adapter_sequence auto: which adapter a mate carries, from the census of its pass-1 sample.

The rule is stated in tests/detect_rule.py; this is the copy the run uses.  A fixed table of candidates, column 1 searched in
read 1's sample and column 2 in read 2's; a candidate's probe is its first PROBE_LEN bases; the device counts, per probe, the
sampled reads that hold it (aqc_adapter_census); the candidate with the largest count — the earlier row on a tie — is detected when
at least MIN_READS reads and MIN_PER_MILLE in a thousand of the sample hold it.  No GPU code here, and nothing of the engine."""

AUTO = "auto"
PROBE_LEN = 12
MIN_READS = 10
MIN_PER_MILLE = 1

# name, read 1's adapter, read 2's adapter
CANDIDATES = (
    ("illumina_truseq", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"),
    ("nextera", "CTGTCTCTTATACACATCT", "CTGTCTCTTATACACATCT"),
    ("illumina_small_rna", "TGGAATTCTCGGGTGCCAAGG", "GATCGTCGGACTGTAGAACTCTGAAC"),
    ("bgi_mgi", "AAGTCGGAGGCCAAGCGGTCTTAGGAAGACAA", "AAGTCGGATCGTAGCCATGTCGTTCTGTGAGCCAAGGAGTTG"),
)


def is_auto(value):
    """an option value that asks for detection (case-insensitive)"""
    return isinstance(value, str) and value.lower() == AUTO


def column(mate):
    """the candidates' adapters of read 1 (mate 0) / read 2 (mate 1), in table order"""
    return [row[1 + mate] for row in CANDIDATES]


def probes(mate):
    return [a[:PROBE_LEN].encode() for a in column(mate)]


def shortest(mate):
    """the length --adapter_min_overlap is held to while the mate's adapter is not known yet"""
    return min(len(a) for a in column(mate))


def decide(counts, sampled):
    """counts: reads holding each candidate's probe, in table order; sampled: the reads looked at -> the row detected, or None"""
    best = None
    for i, c in enumerate(counts):
        if best is None or c > counts[best]:
            best = i
    if best is None:
        return None
    c = int(counts[best])
    return best if c >= MIN_READS and c * 1000 >= int(sampled) * MIN_PER_MILLE else None


def report(mate, counts, sampled):
    """what the statistics JSON says of one asked mate ("adapter_detect": read1 / read2)"""
    row = decide(counts, sampled)
    return {
        "sampled": int(sampled),
        "candidates": [[CANDIDATES[i][0], int(c)] for i, c in enumerate(counts)],
        "detected": None if row is None else CANDIDATES[row][0],
        "adapter": "" if row is None else CANDIDATES[row][1 + mate],
    }
