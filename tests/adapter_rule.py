"""The specification of trimming a given adapter from each read (--adapter_sequence / --adapter_sequence_r2 /
--adapter_min_overlap), as plain python.  Upstream has no such stage: this file is the rule.

The stage stands inside the trim stage of preprocesser.py:455-466, behind upstream's fixed trim and behind the quality cut
(tests/cut_rule.py).  At a place p of the read the k = min(m, n - p) bases the read still has are compared with the adapter's
first k, byte for byte as they are; p matches when at most k >> 3 of them differ (one per full eight, integers only), and the
smallest matching p of 0 .. n - K wins: the read ends there.  adapter_find is the model; precut turns a record into the record a
run WITHOUT the options would have to be given to write the same reads; the rest are the helpers the tests share (a brute-force
restatement, the counts of aqc_get_adapter_stats, seeded inputs and the named placements)."""
import random

import cut_rule

VIEW_ALL = (0, 0xffff)
MIN_LEN, MAX_LEN = 4, 64


class AdapterConfig:
    """a1 / a2: the adapters of read 1 / read 2 as the stage uses them (bytes; b"": that mate is not searched); K: the fewest
    adapter bases a match at the tail needs; cut: the cut_rule.CutConfig of the run (its fixed trims count with every mode off)"""

    def __init__(self, a1=b"", a2=None, K=4, cut=None):
        self.a1 = bytes(a1)
        self.a2 = self.a1 if a2 is None else bytes(a2)
        self.K = int(K)
        self.cut = cut if cut is not None else cut_rule.CutConfig()

    @property
    def on(self):
        return bool(self.a1 or self.a2)

    def adapter(self, mate):
        return self.a2 if mate else self.a1


def adapter_find(s, A, K):
    """s: the bytes of one read behind trim() and the quality cut; -> the place the read ends at, None: no match"""
    n, m = len(s), len(A)
    for p in range(0, n - K + 1):
        k = min(m, n - p)
        mm = 0
        for x, y in zip(s[p:p + k], A[:k]):
            mm += x != y
            if mm > k >> 3:
                break                                   # (this place is lost: no need to count on)
        if mm <= k >> 3:
            return p
    return None


def adapter_find_brute(s, A, K):
    """the same rule restated with explicit loops and indices, from the back: the smallest place is the last one noted"""
    n = len(s)
    m = len(A)
    found = None
    p = n - K
    while p >= 0:
        left = n - p
        k = m if m < left else left
        allowed = k // 8
        wrong = 0
        j = 0
        while j < k:
            if s[p + j] != A[j]:
                wrong += 1
                if wrong > allowed:
                    break
            j += 1
        if wrong <= allowed:
            found = p
        p -= 1
    return found


def compose(view, s_trimmed, A, K):
    """(c0, c1) of a mate behind the quality cut and its trimmed SEQUENCE line -> the view behind the adapter stage"""
    c0, c1 = view
    p = adapter_find(s_trimmed[c0:c1], A, K) if A else None
    return (c0, c1) if p is None else (c0, c0 + p)


def mate_view(s, q, cfg, mate=0):
    """the view (c0, c1) of one mate behind the quality cut and the adapter stage, relative to its trimmed lines"""
    cut = cfg.cut
    tf, tt = (cut.trim_front, cut.trim_tail) if mate == 0 else (cut.trim_front2, cut.trim_tail2)
    s1, q1 = cut_rule.trim(s, tf, tt), cut_rule.trim(q, tf, tt)
    view = cut_rule.cut_window(q1, cut.window, cut.mean_quality, *cut.modes()) if cut.on else VIEW_ALL
    return compose(view, s1, cfg.adapter(mate), cfg.K)


def cut_lines(s, q, cfg, mate=0):
    """the sequence and quality line of one mate (bytes) as the trim stage leaves them: each sliced by its own length"""
    cut = cfg.cut
    tf, tt = (cut.trim_front, cut.trim_tail) if mate == 0 else (cut.trim_front2, cut.trim_tail2)
    c0, c1 = mate_view(s, q, cfg, mate)
    return cut_rule.trim(s, tf, tt)[c0:c1], cut_rule.trim(q, tf, tt)[c0:c1]


def precut(record, cfg, mate=0):
    name, s, strand, q = record
    s2, q2 = cut_lines(s, q, cfg, mate)
    return name, s2, strand, q2


def precut_pairs(pairs, cfg, paired):
    out = []
    for s1, q1, s2, q2 in pairs:
        k1 = cut_lines(s1, q1, cfg, 0)
        k2 = cut_lines(s2, q2, cfg, 1) if paired else (None, None)
        out.append((k1[0], k1[1], k2[0], k2[1]))
    return out


def adapter_counts(pairs, cfg, accum_limit=None):
    """aqc_get_adapter_stats of a run over `pairs` ((s1, q1, s2, q2) bytes; s2 None: single-end): reads of R1 the adapter made
    shorter, bases it removed from them — on the SEQUENCE line, beyond what trim and quality cut took — and the same for R2,
    counted only where read 1 leaves the stage with 5 bases or more"""
    off = AdapterConfig(b"", b"", cfg.K, cfg.cut)
    out = [0, 0, 0, 0]
    for i, (s1, q1, s2, q2) in enumerate(pairs):
        if accum_limit is not None and i >= accum_limit:
            break
        before, after = cut_lines(s1, q1, off, 0)[0], cut_lines(s1, q1, cfg, 0)[0]
        if len(after) < len(before):
            out[0] += 1
            out[1] += len(before) - len(after)
        if s2 is None or len(after) < 5:
            continue
        before, after = cut_lines(s2, q2, off, 1)[0], cut_lines(s2, q2, cfg, 1)[0]
        if len(after) < len(before):
            out[2] += 1
            out[3] += len(before) - len(after)
    return out


# ---- seeded inputs ------------------------------------------------------------------------------------------------
def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other_base(rng, b):
    return rng.choice([x for x in b"ACGT" if x != b])


def make_adapter(rng, m):
    """an adapter of m bases with no base repeated next to itself (so that it does not match itself shifted by one)"""
    out = bytearray()
    while len(out) < m:
        b = rng.choice(b"ACGT")
        if not out or out[-1] != b:
            out.append(b)
    return bytes(out)


def clean_read(rng, n, A):
    """n random bases over a two-letter alphabet the adapter's first base is not in: no place of it starts a match by chance,
    whatever K is (every comparison's first byte differs and nothing shorter than 8 bases forgives that; the longer ones are
    left to the model: the tests compare with it, they do not assume)"""
    letters = bytes(x for x in b"ACGT" if x != A[0])[:2]
    return bytes(rng.choice(letters) for _ in range(n))


def plant(read, p, A):
    """the read with the adapter written over it from place p on, as much of it as fits"""
    k = max(0, min(len(A), len(read) - p))
    return read[:p] + A[:k] + read[p + k:]


def substitute(rng, read, places):
    out = bytearray(read)
    for j in places:
        out[j] = other_base(rng, out[j])
    return bytes(out)


def placements(n, A, K, rng):
    """the named placements of the tests for a read of n bases: (tag, bytes).  What each must give is the model's to say."""
    m = len(A)
    out = [("clean", clean_read(rng, n, A)), ("random", bases(rng, n))]
    if n == 0:
        return out
    base = clean_read(rng, n, A)
    # the whole adapter (or what fits) at every early place and at the last place it fits whole
    for p in sorted(set(list(range(0, 34)) + [n - m])):
        if 0 <= p < n:
            out.append(("at_%d" % p, plant(base, p, A)))
    # the partial adapter at the tail: k = K .. m bases of it, and K - 1 bases, which must not match
    for k in range(max(K - 1, 1), m + 1):
        if k <= n:
            out.append(("tail_%d" % k, plant(base, n - k, A)))
    # exactly k >> 3 mismatches, and one more, in a comparison of k bases
    for k in (7, 8, 15, 16, 63, 64):
        if k > m or k > n or k < K:
            continue
        p = n - k if k < m else max(0, (n - k) // 2)
        r = plant(base, p, A)
        for extra in (0, 1):
            wrong = (k >> 3) + extra
            if wrong > k:
                continue
            places = rng.sample(range(p, p + k), wrong)
            out.append(("mm_%d_%d" % (k, wrong), substitute(rng, r, places)))
    # one mismatch in the first / the last compared byte and on either side of every dword edge of the adapter
    if n >= m:
        p = rng.randrange(0, n - m + 1)
        r = plant(base, p, A)
        for j in sorted(set([0, m - 1] + [e + d for e in range(4, m, 4) for d in (-1, 0)])):
            if 0 <= j < m:
                out.append(("edge_%d" % j, substitute(rng, r, [p + j])))
        # N and lower case inside the match
        for tag, f in (("N", lambda b: ord("N")), ("lower", lambda b: b | 0x20)):
            for j in (0, m // 2, m - 1):
                x = bytearray(r)
                x[p + j] = f(x[p + j])
                out.append(("%s_%d" % (tag, j), bytes(x)))
        # two places: the smaller wins
        if n >= 2 * m + 3:
            p1 = rng.randrange(0, n - 2 * m - 2)
            p2 = rng.randrange(p1 + m + 1, n - m + 1)
            out.append(("two", plant(plant(base, p2, A), p1, A)))
    return out


def with_adapters(rng, pairs, a1, a2, frac=0.3):
    """pairs (s1, q1, s2, q2) with the mate's adapter written over the tail of `frac` of the mates from a place of 20 or beyond
    (a third of them a partial adapter of 4 .. 20 bases at the very end, some adapter bases substituted), random bases behind it"""
    out = []
    for s1, q1, s2, q2 in pairs:
        mates = []
        for s, A in ((s1, a1), (s2, a2)):
            if s is not None and A and len(s) > 40 and rng.random() < frac:
                n = len(s)
                if rng.random() < 0.33:
                    p = n - rng.randint(4, min(20, len(A)))
                else:
                    p = rng.randint(20, n - 5)
                s = plant(s, p, A)
                s = s[:min(n, p + len(A))] + bases(rng, max(0, n - p - len(A)))
                if rng.random() < 0.3 and n - p >= 8:
                    s = substitute(rng, s, [p + rng.randrange(min(len(A), n - p))])
            mates.append(s)
        out.append((mates[0], q1, mates[1], q2))
    return out
