"""The specification of cutting poly-G / poly-X tails from each read (--trim_poly_g / --trim_poly_x / --poly_g_min_len /
--poly_x_min_len), as plain python.  Upstream has no such stage: this file is the rule.  Integers only.

The stage stands inside the trim stage of preprocesser.py:455-466, behind upstream's fixed trim, behind the quality cut
(tests/cut_rule.py) and behind the adapter stage (tests/adapter_rule.py).  For a letter X, a minimum length L and a line s of n
bytes:

  mm(u)    the number of bytes among the last u of s that are not exactly X (an N, a lower-case letter, any other byte: a mismatch)
  fail(u)  mm(u) > 5, or u >= L and mm(u) > (u >> 3)
  scanned  (the smallest u in 1 .. n with fail(u)) - 1; n where there is no such u
  t        scanned < L: X cuts nothing; else the largest u <= scanned with s[n - u] == X — the line ends at n - t

Every letter that is on is tried on the same line with its own L, the smallest end wins, once.  poly_end is the model; precut turns
a record into the record a run WITHOUT the options would have to be given to write the same reads; the rest are the helpers the
tests share (a brute-force restatement, the counts of aqc_get_poly_stats, seeded inputs and the named placements)."""
import adapter_rule
import cut_rule

VIEW_ALL = (0, 0xffff)
LETTERS = b"ACGT"
MAX_MISMATCH = 5
MAX_MIN_LEN = 1000


def poly_end(s, X, L):
    """s: the bytes of one line; X: the letter (an int); -> where the line ends (len(s): nothing is cut)"""
    n = len(s)
    scanned = n
    mm = 0
    for u in range(1, n + 1):
        mm += s[n - u] != X
        if mm > MAX_MISMATCH or (u >= L and mm > (u >> 3)):
            scanned = u - 1
            break
    if scanned < L:
        return n
    t = max((u for u in range(1, scanned + 1) if s[n - u] == X), default=0)
    return n - t


def poly_end_brute(s, X, L):
    """the sequential loop the rule was taken from, with its break: walk from the last byte, remember the leftmost X seen, stop
    where the mismatches are too many; cut if the walk got far enough"""
    rlen = len(s)
    mismatch = 0
    first_pos = rlen - 1
    i = 0
    while i < rlen:
        if s[rlen - i - 1] != X:
            mismatch += 1
        else:
            first_pos = rlen - i - 1
        allowed = (i + 1) // 8
        if mismatch > 5 or (mismatch > allowed and i >= L - 1):
            break
        i += 1
    if i >= L:
        return first_pos
    return rlen


class PolyConfig:
    """min_len: the minimum lengths of A, C, G, T (0: the letter is off); adapter: the adapter_rule.AdapterConfig of the run (its
    cut_rule.CutConfig and fixed trims count with no adapter given)"""

    def __init__(self, min_len=(0, 0, 0, 0), adapter=None):
        self.min_len = tuple(int(v) for v in min_len)
        self.adapter = adapter if adapter is not None else adapter_rule.AdapterConfig()

    @classmethod
    def from_options(cls, g=False, x=False, g_len=10, x_len=10, adapter=None):
        """--trim_poly_g / --trim_poly_x as the command line gives them: poly-X tries every letter, G takes the smaller length"""
        lx = x_len if x else 0
        lg = (min(g_len, x_len) if x else g_len) if g else lx
        return cls((lx, lx, lg, lx), adapter)

    @property
    def on(self):
        return any(self.min_len)


def line_end(s, min_len):
    """every letter that is on, each with its own L, on the same line: the smallest end"""
    end = len(s)
    for X, L in zip(LETTERS, min_len):
        if L:
            end = min(end, poly_end(s, X, L))
    return end


def compose(view, s_trimmed, min_len):
    """(c0, c1) of a mate behind the earlier stages and its trimmed SEQUENCE line -> the view behind this stage"""
    c0, c1 = view
    s = s_trimmed[c0:c1]
    end = line_end(s, min_len)
    return (c0, c1) if end >= len(s) else (c0, c0 + end)


def trims(cfg, mate):
    cut = cfg.adapter.cut
    return (cut.trim_front, cut.trim_tail) if mate == 0 else (cut.trim_front2, cut.trim_tail2)


def mate_view(s, q, cfg, mate=0):
    """the view (c0, c1) of one mate behind the quality cut, the adapter stage and this one, relative to its trimmed lines"""
    tf, tt = trims(cfg, mate)
    return compose(adapter_rule.mate_view(s, q, cfg.adapter, mate), cut_rule.trim(s, tf, tt), cfg.min_len)


def cut_lines(s, q, cfg, mate=0):
    """the sequence and quality line of one mate (bytes) as the trim stage leaves them: each sliced by its own length"""
    tf, tt = trims(cfg, mate)
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


def poly_counts(pairs, cfg, accum_limit=None):
    """aqc_get_poly_stats of a run over `pairs` ((s1, q1, s2, q2) bytes; s2 None: single-end): reads of R1 the stage made shorter,
    bases it removed from them — on the SEQUENCE line, beyond what trim, quality cut and adapter took — and the same for R2,
    counted only where read 1 leaves the stage with 5 bases or more"""
    off = PolyConfig((0, 0, 0, 0), cfg.adapter)
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
    return bytes(rng.choice(LETTERS) for _ in range(n))


def other_base(rng, b):
    return rng.choice([x for x in LETTERS if x != b])


def clean_read(rng, n, X):
    """n random bases over the three letters that are not X"""
    letters = bytes(x for x in LETTERS if x != X)
    return bytes(rng.choice(letters) for _ in range(n))


def with_tail(read, t, X):
    """the read with its last t bytes (as many as it has) written over with X"""
    t = max(0, min(t, len(read)))
    return read[:len(read) - t] + bytes([X]) * t


def substitute(rng, read, places):
    out = bytearray(read)
    for j in places:
        out[j] = other_base(rng, out[j])
    return bytes(out)


def placements(n, X, L, rng):
    """the named placements of the tests for a read of n bases: (tag, bytes).  What each must give is the model's to say."""
    out = [("clean", clean_read(rng, n, X)), ("random", bases(rng, n))]
    if n == 0:
        return out
    base = clean_read(rng, n, X)
    # a tail of t bases around L and around the edges of a lane's 16 bytes
    for t in sorted(set([L - 2, L - 1, L, L + 1, 15, 16, 17, 31, 32, 33, 47, 48, 49])):
        if 1 <= t <= n:
            out.append(("tail_%d" % t, with_tail(base, t, X)))
    out.append(("whole", bytes([X]) * n))
    # exactly u >> 3 mismatches, and one more, inside a tail of u bases (never its leftmost base, which stays X)
    for u in (8, 16, 48, 64):
        if u > n:
            continue
        r = with_tail(base, u, X)
        for extra in (0, 1):
            wrong = (u >> 3) + extra
            places = rng.sample(range(n - u + 1, n), wrong)
            out.append(("mm_%d_%d" % (u, wrong), substitute(rng, r, places)))
    # the cap: a tail of 100 with 5 mismatches, and with a 6th
    if n >= 100:
        r = with_tail(base, 100, X)
        for wrong in (5, 6):
            out.append(("cap_%d" % wrong, substitute(rng, r, rng.sample(range(n - 99, n), wrong))))
    # a mismatch as the read's very last byte
    for t in (L, L + 1, 24):
        if 2 <= t <= n:
            out.append(("last_%d" % t, substitute(rng, with_tail(base, t, X), [n - 1])))
    # N and lower case inside the tail
    t = min(n, max(L + 8, 20))
    r = with_tail(base, t, X)
    for tag, f in (("N", lambda b: ord("N")), ("lower", lambda b: b | 0x20)):
        for j in sorted(set([n - t, n - (t + 1) // 2, n - 1])):
            x = bytearray(r)
            x[j] = f(x[j])
            out.append(("%s_%d" % (tag, n - j), bytes(x)))
    # two letters' tails one behind the other: X in front of another letter, and behind it
    Y = other_base(rng, X)
    for t1, t2 in ((L + 3, L + 2), (20, 12), (12, 3)):
        if t1 + t2 <= n:
            out.append(("two_%d_%d" % (t1, t2), with_tail(with_tail(base, t1 + t2, X), t2, Y)))
            out.append(("two_%d_%d" % (t2, t1), with_tail(with_tail(base, t1 + t2, Y), t2, X)))
    return out


def with_tails(rng, pairs, frac=0.3):
    """pairs (s1, q1, s2, q2) with a tail of 10 .. 60 bases written over the end of `frac` of the mates: mostly G, the rest one of
    the other letters, one substitution inside half of the tails of 24 bases or more.  The tail's qualities are high, as a dark
    cycle's are (phred 37): a quality cut leaves it standing"""
    out = []
    for s1, q1, s2, q2 in pairs:
        mates = []
        for s, q in ((s1, q1), (s2, q2)):
            if s is not None and len(s) > 70 and rng.random() < frac:
                t = rng.randint(10, 60)
                X = ord("G") if rng.random() < 0.7 else rng.choice(b"ACT")
                s = with_tail(s, t, X)
                if t >= 24 and rng.random() < 0.5:
                    s = substitute(rng, s, [len(s) - 1 - rng.randrange(t - 1)])
                if len(q) == len(s):
                    q = q[:len(q) - t] + bytes([33 + 37]) * t
            mates.append((s, q))
        out.append((mates[0][0], mates[0][1], mates[1][0], mates[1][1]))
    return out
