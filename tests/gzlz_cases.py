"""FASTQ texts for the hash-chain gzip encoder of levels 6 - 9 (csrc/aqc_gzlz.hpp), shared by its CPU test (the search's
functions dealt out by loops, tests/native/gzlz_selftest.cpp) and its GPU test (aqc_compress).  Every text is made of whole
records, from a seed; MEMBER = 0xff00 is the text of one gzip member."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBER = 0xff00
PRINTABLE = np.arange(33, 127, dtype=np.uint8)             # '!' .. '~'
QUALS = np.frombuffer(b"EA/<6#", dtype=np.uint8)
QUAL_P = [0.64, 0.18, 0.09, 0.06, 0.02, 0.01]


def record(name, seq, qual):
    assert len(seq) == len(qual)
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def bases(rng, L, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), L)].tobytes()


def quals(rng, L):
    return QUALS[rng.choice(6, L, p=QUAL_P)].tobytes()


def noise(rng, L):
    """bytes drawn uniformly from '!' .. '~': as a name (never '@' first: a byte is put in front) or a quality line"""
    return PRINTABLE[rng.integers(0, len(PRINTABLE), L)].tobytes()


def sim_name(rng, i):
    return b"SIM:1:FC1:%d:%d:%d:%d 1:N:0:ACGT" % (1 + i % 4, 1101 + int(rng.integers(0, 1200)), 1000 + int(rng.integers(0, 24000)), 1000 + int(rng.integers(0, 19000)))


def ordinary(rng, nbytes, L=100):
    """ordinary low-entropy FASTQ records: at least nbytes of them"""
    out, n, i = [], 0, 0
    while n < nbytes:
        out.append(record(sim_name(rng, i), bases(rng, L), quals(rng, L)))
        n += len(out[-1])
        i += 1
    return out


def exact(rng, total):
    """ordinary FASTQ of exactly `total` bytes (>= 200): the last records' name lengths make up the size"""
    assert total >= 200
    out, n, i = [], 0, 0
    while True:
        r = record(sim_name(rng, i), bases(rng, 100), quals(rng, 100))
        if n + len(r) + 160 > total:
            break
        out.append(r)
        n += len(r)
        i += 1
    left = total - n                     # 160 .. ~420: one or two records with names of x's
    if left > 300:
        out.append(record(b"x" * 40, bases(rng, 50), quals(rng, 50)))
        left -= len(out[-1])
    L = 20
    out.append(record(b"t" * (left - 6 - 2 * L), bases(rng, L), quals(rng, L)))
    text = b"".join(out)
    assert len(text) == total, (len(text), total)
    return text


def real(mate):
    """the NextSeq reads of tests/golden/testdata: 250 records, one full member and a 23 KB tail"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "testdata", "R%d.fq.gz" % mate), "rb") as f:
        return f.read()


def far_repeats():
    """400 records of 100 bases: sequence and quality line of record i are those of record i - 37 (9 KB back), names are unique.
    Qualities are uniform over '!' .. '~': no runs.  What repeats is neither at distance 1 nor in the line four lines up."""
    rng = np.random.default_rng(7100)
    seqs, qs, out = [], [], []
    for i in range(400):
        seqs.append(seqs[i - 37] if i >= 37 else bases(rng, 100))
        qs.append(qs[i - 37] if i >= 37 else noise(rng, 100))
        out.append(record(b"far.%d.%d" % (i, int(rng.integers(0, 10 ** 9))), seqs[i], qs[i]))
    return b"".join(out)


def check_far_repeats(text):
    """from the text: record i repeats record i - 37, and neither old matcher can see it — no byte repeats twelve times in a row
    (distance 1), no line shares a stretch of 8 columns with the line four lines up"""
    lines = text.split(b"\n")[:-1]
    seqs, qs = lines[1::4], lines[3::4]
    assert len(seqs) == 400 and all(seqs[i] == seqs[i - 37] and qs[i] == qs[i - 37] for i in range(37, 400))
    assert len(set(lines[0::4])) == 400

    def longest_true(eq):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], eq.astype(np.int32), [0]))))
        return int((edges[1::2] - edges[0::2]).max()) if len(edges) else 0
    a = np.frombuffer(text, dtype=np.uint8)
    assert longest_true(a[1:] == a[:-1]) < 11
    for i in range(4, len(lines)):
        x, y = np.frombuffer(lines[i], dtype=np.uint8), np.frombuffer(lines[i - 4], dtype=np.uint8)
        n = min(len(x), len(y))
        assert longest_true(x[:n] == y[:n]) < 8, (i, lines[i], lines[i - 4])


def window_edge(dist):
    """a 300-byte record of noise at offset 0 and its copy at offset `dist`, ordinary FASTQ between and behind: one member"""
    rng = np.random.default_rng(7200)
    block = record(b"w" + noise(rng, 97), bases(rng, 98), noise(rng, 98))
    assert len(block) == 300
    text = block + exact(rng, dist - 300) + block + b"".join(ordinary(rng, 1500))
    assert text[dist:dist + 300] == block and len(text) < MEMBER
    return text


REPEAT_LENGTHS = (3, 4, 257, 258, 259, 260, 516, 1000)


def length_edges():
    """per length L: a string of L noise bytes inside a quality line, and again 6 KB or more later, between other neighbours
    both times (so the repeat is L long and no longer).  -> (text, [(first offset, second offset, L)])"""
    rng = np.random.default_rng(7300)
    out, n, marks = [], 0, []

    def put(r):
        nonlocal n
        out.append(r)
        n += len(r)

    for L in REPEAT_LENGTHS:
        if n // MEMBER != (n + 4 * L + 9000) // MEMBER:           # (keep both copies inside one member)
            while n % MEMBER > 500:
                put(record(sim_name(rng, len(out)), bases(rng, 100), quals(rng, 100)))
        rep = noise(rng, L).replace(b"a", b"e").replace(b"b", b"e").replace(b"c", b"e").replace(b"d", b"e")
        at = []
        for left, right in ((b"a", b"c"), (b"b", b"d")):
            pre, post = (b"", b"") if L == 1000 else (noise(rng, 5).replace(b"a", b"e").replace(b"b", b"e") + left, right + noise(rng, 5))
            q = pre + rep + post
            name = sim_name(rng, len(out))
            at.append(n + 1 + len(name) + 1 + len(q) + 3 + len(pre))
            put(record(name, bases(rng, len(q)), q))
            for r in ordinary(rng, 6000):
                put(r)
        marks.append((at[0], at[1], L))
    text = b"".join(out)
    for a, b, L in marks:
        assert text[a:a + L] == text[b:b + L] and b - a >= 6000 and b - a <= 32768
        if L < 1000:
            assert text[a - 1] != text[b - 1] and text[a + L] != text[b + L]
    return text, marks


def ends_on_last_byte():
    """exactly one member whose last record is a copy of an earlier one, 10 KB back: the repeat ends on the member's last byte"""
    rng = np.random.default_rng(7400)
    one = record(sim_name(rng, 0), bases(rng, 100), noise(rng, 100))
    body = exact(rng, MEMBER - 10000 - len(one))
    text = body + one + exact(rng, 10000 - len(one)) + one
    assert len(text) == MEMBER and text.endswith(one) and text.count(one) == 2
    return text


def source_in_previous_member():
    """two members: the second begins with copies of the records the first one ends with (3 KB back, across the border)"""
    rng = np.random.default_rng(7500)
    tail = b"".join(record(sim_name(rng, i), bases(rng, 100), noise(rng, 100)) for i in range(12))
    text = exact(rng, MEMBER - len(tail)) + tail + tail + b"".join(ordinary(rng, 3000))
    assert text[MEMBER - len(tail):MEMBER] == text[MEMBER:MEMBER + len(tail)] and MEMBER < len(text) < 2 * MEMBER
    return text


def long_chains(kind):
    """60 KB in records of 1000 bases: ACAC... with one quality character, or bases over {A, C} and qualities over {I, H}
    from a seed — thousands of positions share a hash"""
    rng = np.random.default_rng(7600)
    if kind == "acac":
        return b"".join(record(b"c%d" % i, b"AC" * 500, b"I" * 1000) for i in range(30))
    return b"".join(record(b"c%d" % i, bases(rng, 1000, b"AC"), bases(rng, 1000, b"IH")) for i in range(30))


def noise_text(nbytes):
    """records of noise names and noise qualities around ten bases: nothing to match, about 6.5 bits a byte"""
    rng = np.random.default_rng(7700)
    out, n = [], 0
    while n < nbytes:
        out.append(record(b"n" + noise(rng, 79), bases(rng, 10), noise(rng, 10)))
        n += len(out[-1])
    return b"".join(out)


def residues():
    return [MEMBER, MEMBER + 1, MEMBER + 2, MEMBER + 3, 2 * MEMBER + 4, 2 * MEMBER - 1]


def cpu_cases():
    """name -> text for the CPU program: the GPU test's texts, and a few that need no records (the search does not know FASTQ)"""
    rng = np.random.default_rng(7800)
    cases = {"real_R1": real(1), "real_R2": real(2), "far_repeats": far_repeats(), "window_32768": window_edge(32768),
             "window_32769": window_edge(32769), "length_edges": length_edges()[0], "ends_on_last_byte": ends_on_last_byte(),
             "source_in_previous_member": source_in_previous_member(), "chains_acac": long_chains("acac"),
             "chains_two_letters": long_chains("two"), "noise": noise_text(MEMBER + 5000)}
    for total in residues():
        cases["residue_%d" % total] = exact(np.random.default_rng(7900 + total % 89), total)
    for n in (0, 1, 2, 3, 4, 5):
        cases["tiny_%d" % n] = b"ACACA"[:n]
    cases["one_byte_run"] = b"A" * 70000
    cases["period_3"] = b"ACG" * 30000
    cases["two_letters_raw"] = bases(rng, 2 * MEMBER + 3, b"AC")
    cases["all_bytes"] = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    return cases
