"""Constructed records for the verdict kernel's per-read filters (csrc/aqc_fast.hpp, phase 2): polyX, the low-quality count, the N
count, trim / BADTRIM / length and the order of the flags, each at its threshold and at the borders of the kernel's words.  Not a
test module: test_verdict_filter_cases_cpu.py proves the table against oracle/pyloop.py and the C oracle, test_gpu_verdict_filters.py
runs it through aqc_run on every tier.

A case is (tag, seq1, qual1, seq2 | None, qual2 | None, cfg keywords, expected flag, may_defer: reason | None).  The flag is stated by
the builder, from how the record was made, never computed by an implementation of the filters.  What makes that possible:

  * the reads are seeded random permutations of the letters in blocks ("background"): every letter turns up once per block, so a
    window of W bases holds at most W / 4 + 2 copies of a letter (W / 3 + 2 in a background of three letters) — far below any
    `need` the polyX cases plant — and two backgrounds never overlap: the scan finds nothing;
  * a read with a planted poly-X window holds X nowhere else (its background is drawn from the other letters), so the count of X
    in any window is what the builder put there;
  * mates of a GOOD-side case keep final views of at least 16 bases, or both keep at most 30 (no diagonal of 31 columns exists):
    the scan's short16 deferral cannot fire, the lane-per-read kernel decides the pair itself.

The tag names family / config / length / mate / position class / kind, "/"-separated (a polyX row adds the poly and the foreign
base planted in each mate); the coverage asserts of the CPU test read it.
Position classes: first (base 0), last (the read's last base), w16 (a 16-base border of the tier's or the read's last two words),
w32 (a 32-base border, the low-quality plane's words); read 2's are counted from its end, as the kernel's reverse_r2 stream is.
With lead > 0 (the barcode instance: every mate gets `lead` bases in front) the borders are those of the raw read, prefix
included, and of the moved stream."""
import random
from collections import namedtuple

Case = namedtuple("Case", "tag seq1 qual1 seq2 qual2 cfg flag may_defer")

GOOD, BADBCD1, BADBCD2, BADTRIM1, BADTRIM2, BADLEN, BADPOL, BADLQC, BADNCT = 0, 1, 2, 3, 4, 6, 7, 8, 9

OFF = dict(trim_front=0, trim_tail=0, trim_front2=0, trim_tail2=0, seq_len_req=0, poly_size_limit=0, allow_mismatch_in_poly=0,
           qualified_quality_phred=15, unqualified_base_limit=0, n_base_limit=0)

POLY_WORD = [(35, 2), (31, 0), (36, 5), (50, 5)]
POLY_DOUBLING = [(20, 0), (20, 1), (30, 0), (10, 3), (36, 6)]
POLY_STEP_CAP = [(240, 6)]
POLY_ALL = [(5, 4), (10, 10), (3, 7), (35, -1)]
POLY_CONFIGS = POLY_WORD + POLY_DOUBLING + POLY_STEP_CAP + POLY_ALL
NEVER_FIRES = [(35, -1)]            # need = 36 copies in a window of 35: hasPolyX cannot return a base, whatever the read
LQ_LIMITS, LQ_PHREDS = (1, 60), (0, 2, 15, 41, 93, 94)
N_LIMITS = (1, 5)
TIER_FLOOR = {10: 0, 16: 160, 18: 256, 20: 288}
PREFIX = 17                         # 12-base barcode + CAGTA
TRIMS = dict(trim_front=3, trim_tail=2, trim_front2=2, trim_tail2=3)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def cfg_of(**kw):
    d = dict(OFF)
    d.update(kw)
    return d


def cfg_key(cfg):
    return tuple(sorted(cfg.items()))


def poly_screen(max_poly, mismatch):
    """which screen the kernel runs for a config, by its own formula (aqc_fast.hpp: run_req, poly_word) -> (regime, run_req)"""
    need = max_poly - mismatch
    run_req = (need + mismatch) // (mismatch + 1) if mismatch >= 0 else 0
    poly_word = mismatch >= 0 and need >= 31 and mismatch <= 5
    return ("all" if run_req < 2 else "word" if poly_word else "doubling"), run_req


def view_len(n, front, tail):
    """len(s[front:-tail]) / len(s[front:]) the python way (preprocesser.py:19-28)"""
    end = max(n - tail, 0) if tail > 0 else n
    return max(end - min(front, n), 0)


def lengths(NW, lead=0):
    """read lengths of a tier: raw (prefix included) 16 NW, 16 NW - 1, the tier's floor + 1, and 150"""
    raw = sorted(set([16 * NW, 16 * NW - 1, TIER_FLOOR[NW] + 1, 150]))
    return [r - lead for r in raw if r - lead >= 1 and r <= 16 * NW]


def background(rng, n, letters="ACGT"):
    out = []
    while len(out) < n:
        blk = list(letters)
        rng.shuffle(blk)
        out += blk
    return "".join(out[:n])


def positions(L, NW, lead=0, from_end=False):
    """-> [(class, p)]: a feature lies on both sides of the border in front of base p (p = 0: it starts the read, p = L: it ends it).
    from_end: p counts from the read's end — the caller builds the read in stream order and reverses it."""
    frames = [(L + (0 if from_end else lead), 0 if from_end else lead)]
    if lead and not from_end:
        frames.append((L, 0))                        # the stream after the barcode moved the view
    found = {}
    for R, shift in frames:
        top = 16 * NW
        w16 = [top - 32, top - 16, 16 * ((R - 1) // 16), 16 * ((R - 1) // 16) - 16]
        w32 = [32 * ((R - 1) // 32), 32 * ((R - 1) // 32) - 32]
        for cls, borders in (("w16", w16), ("w32", w32)):
            for B in borders:
                p = B - shift
                if 0 < p < L:
                    found.setdefault(p, set()).add(cls)
    return [("first", 0)] + [("+".join(sorted(found[p])), p) for p in sorted(found)] + [("last", L)]


def place(p, k, lo, hi, side=0):
    """start of a feature of k bases at border p inside [lo, hi): half on either side, the odd base on the side asked for"""
    return max(lo, min(p - (k + 1 - side) // 2, hi - k))


def put(s, start, piece):
    return s[:start] + piece + s[start + len(piece):]


def window(max_poly, nx, X, F):
    """max_poly bases with nx copies of X, the foreign ones spread evenly: the longest run is ceil(nx / (foreign + 1))"""
    f = max_poly - nx
    base, extra = divmod(nx, f + 1)
    sizes = [base + 1] * extra + [base] * (f + 1 - extra)
    if extra > 1:                                    # the longer groups at both ends
        sizes = [base + 1] + sizes[extra:] + [base + 1] * (extra - 1)
    w = F.join(X * g for g in sizes)
    assert len(w) == max_poly and w.count(X) == nx
    return w


def mate_len(L, cap):
    """an unrelated mate for a read of L bases: as long as the read, but 24 bases for a read under 16 (both at most 30: no scan)"""
    return min(L, cap) if L >= 16 else 24


def qual_high(n, thr):
    """qualified throughout: exactly thr and a comfortable value in turn"""
    a, b = chr(min(thr, 127)), chr(min(max(thr, 73), 127))
    return ((a + b) * (n // 2 + 1))[:n]


def qual_low(n, thr):
    """unqualified throughout — but for phred 0, where only chr(32) is unqualified: phred -1, and a line of nothing else has a
    negative sum in the one window of the CUT instance's quality cut, which would then cut the read away.  There every other base is
    chr(32) (upstream never counts read 2, whatever it holds)"""
    if thr - 1 >= 34:
        return chr(thr - 1) * n
    return (chr(thr - 1) + "I") * (n // 2) + chr(thr - 1) * (n % 2)


class Builder:
    def __init__(self, NW, paired, lead=0, seed=20261021):
        self.NW, self.paired, self.lead = NW, paired, lead
        self.cap = 16 * NW - lead
        self.rng = random.Random(seed * 64 + NW * 4 + (2 if paired else 0) + (1 if lead else 0))
        self.cases = []
        self.turn = 0

    def add(self, tag, s1, q1, s2, q2, cfg, flag, may_defer=None):
        assert len(s1) == len(q1) and len(s1) <= self.cap
        if self.paired:
            assert len(s2) == len(q2) and len(s2) <= self.cap
            self.cases.append(Case(tag, s1, q1, s2, q2, cfg, flag, may_defer))
        else:
            self.cases.append(Case(tag, s1, q1, None, None, cfg, flag, may_defer))

    def mates(self):
        return ("r1", "r2", "both") if self.paired else ("r1",)

    def plain(self, n, letters="ACGT"):
        return background(self.rng, n, letters)

    # ---- polyX -----------------------------------------------------------------------------------------------------------------------
    def letters_for(self):
        """the poly base and the foreign base of the next case: X from A C G T N in turn, the foreign base another letter or N
        (for X = G always N, which shares G's 2-bit code)"""
        self.turn += 1
        X = "ACGTN"[self.turn % 5]
        other = "A" if X == "N" else "ACGT"[("ACGT".index(X) + 1 + self.turn // 5) % 4]
        if other == X:
            other = "ACGT"[("ACGT".index(X) + 1) % 4]
        F = "N" if X == "G" or (X != "N" and (self.turn // 5) % 2) else other
        return X, F

    def poly_mate(self, L, p, win, X, from_end):
        """a read of L bases whose only copies of X are the window's, at border p"""
        s = self.plain(L, "".join(c for c in "ACGT" if c != X))
        s = put(s, L - len(win) if p == L else place(p, len(win), 0, L), win)
        return s[::-1] if from_end else s

    def poly_pair(self, tag, cfg, L, mate, make, flag):
        """make(X, F, from_end) -> the featured read; the other mate is background.  Both mates get the same letters, but for
        X = N in both: rc(N) = N, read 1's run would meet read 2's on a diagonal, so there read 1 holds a run of A and read 2 the
        run of N.  The tag's last field names what was planted, mate by mate."""
        X, F = self.letters_for()
        X1 = "A" if X == "N" and mate == "both" else X
        F1 = "C" if F == X1 else F
        planted = []
        if mate in ("r1", "both"):
            s1 = make(X1, F1, False)
            planted.append("r1:X%s-F%s" % (X1, F1))
        else:
            s1 = self.plain(mate_len(L, self.cap))
        if mate in ("r2", "both"):
            s2 = make(X, F, True)
            planted.append("r2:X%s-F%s" % (X, F))
        else:
            s2 = self.plain(mate_len(L, self.cap))
        self.add("%s/%s" % (tag, ",".join(planted)), s1, "I" * len(s1), s2, "I" * len(s2), cfg, flag)

    def polyx(self):
        for mp, mm in POLY_CONFIGS:
            if mp > self.cap:
                continue
            regime, _ = poly_screen(mp, mm)
            need = mp - mm
            cfg = cfg_of(poly_size_limit=mp, allow_mismatch_in_poly=mm)
            cfgt = cfg_of(poly_size_limit=mp, allow_mismatch_in_poly=mm, **TRIMS)
            name = "polyx/%d,%d" % (mp, mm)
            if regime == "all":
                self.polyx_all(name, mp, mm, cfg, cfgt)
                continue
            for L in lengths(self.NW, self.lead):
                if L < mp:
                    continue
                for mate in self.mates():
                    for cls, p in positions(L, self.NW, self.lead, mate == "r2"):
                        # exactly need copies in a window of exactly mp: fires; one fewer, X nowhere else: does not
                        self.poly_pair("%s/L%d/%s/%s/fire" % (name, L, mate, cls), cfg, L, mate,
                                       lambda X, F, e: self.poly_mate(L, p, window(mp, need, X, F), X, e), BADPOL)
                        self.poly_pair("%s/L%d/%s/%s/quiet" % (name, L, mate, cls), cfg, L, mate,
                                       lambda X, F, e: self.poly_mate(L, p, window(mp, need - 1, X, F), X, e), GOOD)
            # hasPolyX returns early for len < maxPoly: a pure run of maxPoly - 1 bases is no polyX, one of maxPoly is
            for mate in self.mates():
                for n, kind, flag in ((mp - 1, "quiet", GOOD), (mp, "fire", BADPOL)):
                    self.poly_pair("%s/L%d/%s/whole/%s" % (name, n, mate, kind), cfg, n, mate, lambda X, F, e: X * n, flag)
            # a firing window at the view's edge: the trim takes its outermost X (need - 1 left) or stops just short of it
            for L in lengths(self.NW, self.lead):
                if L < mp + 8:
                    continue
                for mate in self.mates()[:2]:
                    front, tail = (TRIMS["trim_front"], TRIMS["trim_tail"]) if mate == "r1" else (TRIMS["trim_front2"], TRIMS["trim_tail2"])
                    for end, t in (("front", front), ("tail", tail)):
                        for cut, kind, flag in ((t - 1, "quiet", GOOD), (t, "fire", BADPOL)):
                            def make(X, F, e, L=L, end=end, cut=cut):
                                s = self.plain(L, "".join(c for c in "ACGT" if c != X))
                                w = window(mp, need, X, F)
                                assert w[0] == X and w[-1] == X
                                return put(s, cut if end == "front" else L - cut - mp, w)
                            self.poly_pair("%s/L%d/%s/trim-%s/%s" % (name, L, mate, end, kind), cfgt, L, mate,
                                           lambda X, F, e: make(X, F, e), flag)

    def polyx_all(self, name, mp, mm, cfg, cfgt):
        """run_req < 2: every read of maxPoly bases or more is a suspect, and for need <= 1 every one of them fires (the first base
        alone reaches the count); (35, -1) needs 36 copies in a window of 35 and never fires"""
        never = (mp, mm) in NEVER_FIRES
        Ls = [L for L in lengths(self.NW, self.lead) if L >= mp]
        if never:
            for L in Ls:
                for mate in self.mates():
                    for cls, p in positions(L, self.NW, self.lead, mate == "r2"):
                        self.poly_pair("%s/L%d/%s/%s/quiet" % (name, L, mate, cls), cfg, L, mate,
                                       lambda X, F, e: self.poly_mate(L, p, X * (mp + 1), X, e), GOOD)
                    self.poly_pair("%s/L%d/%s/whole/quiet" % (name, L, mate), cfg, L, mate, lambda X, F, e: X * L, GOOD)
            for mate in self.mates():
                self.poly_pair("%s/L%d/%s/whole/quiet" % (name, mp - 1, mate), cfg, mp - 1, mate, lambda X, F, e: X * (mp - 1), GOOD)
            return
        for a in [mp - 1, mp] + Ls:
            for b in ([mp - 1, mp] + Ls[-1:] if self.paired else [0]):
                fires = a >= mp or b >= mp
                mate = "both" if a >= mp and b >= mp else "r1" if a >= mp else "r2" if b >= mp else "both"
                s1, s2 = self.plain(a), self.plain(b)
                self.add("%s/L%d-%d/%s/whole/%s" % (name, a, b, mate, "fire" if fires else "quiet"), s1, "I" * a, s2, "I" * b, cfg,
                         BADPOL if fires else GOOD)
        # the same through the trims: views of maxPoly - 1 and maxPoly bases
        for v1 in (mp - 1, mp):
            for v2 in ((mp - 1, mp) if self.paired else (0,)):
                if min(v1, v2 if self.paired else v1) < 5:
                    continue
                fires = v1 >= mp or v2 >= mp
                mate = "both" if v1 >= mp and v2 >= mp else "r1" if v1 >= mp else "r2" if v2 >= mp else "both"
                s1, s2 = self.plain(v1 + 5), self.plain(v2 + 5)
                self.add("%s/L%d-%d/%s/trim-both/%s" % (name, v1 + 5, v2 + 5, mate, "fire" if fires else "quiet"), s1, "I" * len(s1), s2,
                         "I" * len(s2), cfgt, BADPOL if fires else GOOD)

    # ---- low quality (read 1 only upstream) ----------------------------------------------------------------------------------------------
    def lq_case(self, tag, cfg, L, lows, flag):
        """read 1 qualified but for the bases `lows`, exactly one below the threshold; read 2 unqualified throughout"""
        thr = cfg["qualified_quality_phred"] + 33
        q = list(qual_high(L, thr))
        for i in lows:
            q[i] = chr(thr - 1)
        L2 = mate_len(L, self.cap)
        self.add(tag, self.plain(L), "".join(q), self.plain(L2), qual_low(L2, thr), cfg, flag)

    def lowq(self):
        for limit in LQ_LIMITS:
            for phred in LQ_PHREDS:
                for path, trim in (("summed", 0), ("plane", 1)):
                    cfg = cfg_of(unqualified_base_limit=limit, qualified_quality_phred=phred, trim_front=trim, trim_tail=trim,
                                 trim_front2=trim, trim_tail2=trim)
                    name = "lq/%d,q%d,%s" % (limit, phred, path)
                    for L in lengths(self.NW, self.lead):
                        lo, hi = trim, L - trim
                        if trim and hi - lo < 16:
                            continue
                        for cls, p in positions(L, self.NW, self.lead):
                            self.turn += 1                       # (the odd base of a feature: in front of the border and behind it in turn)
                            for count, kind, flag in ((limit, "quiet", GOOD), (limit + 1, "fire", BADLQC)):
                                if count > hi - lo:
                                    continue
                                st = hi - count if p == L else place(p, count, lo, hi, self.turn & 1)
                                self.lq_case("%s/L%d/r1/%s/%s" % (name, L, cls, kind), cfg, L, range(st, st + count), flag)
                    if phred == 94 and path == "summed":
                        # thr = 127: every printable byte is unqualified
                        for L in lengths(self.NW, self.lead):
                            L2 = mate_len(L, self.cap)
                            self.add("%s/L%d/r1/whole/%s" % (name, L, "fire" if L > limit else "quiet"), self.plain(L), "I" * L, self.plain(L2),
                                     "I" * L2, cfg, BADLQC if L > limit else GOOD)
            # surplus low bases that lie wholly in the trimmed-off front / tail do not count
            cfg = cfg_of(unqualified_base_limit=limit, trim_front=3, trim_tail=3, trim_front2=3, trim_tail2=3)
            for L in lengths(self.NW, self.lead):
                if L < limit + 24:
                    continue
                for cls, p in positions(L, self.NW, self.lead):
                    for count, kind, flag in ((limit, "quiet", GOOD), (limit + 1, "fire", BADLQC)):
                        st = L - 3 - count if p == L else place(p, count, 3, L - 3)
                        lows = list(range(st, st + count)) + [0, 1, 2, L - 3, L - 2, L - 1]
                        self.lq_case("lq/%d,q15,surplus/L%d/r1/%s/%s" % (limit, L, cls, kind), cfg, L, lows, flag)
        # phred 95: thr = 128 is no byte of a quality line — every base is unqualified, and the general kernel runs the batch
        cfg = cfg_of(unqualified_base_limit=60, qualified_quality_phred=95)
        for L, flag in ((60, GOOD), (61, BADLQC), (min(150, self.cap), BADLQC)):
            self.add("lq/60,q95,general/L%d/r1/whole/%s" % (L, "fire" if flag else "quiet"), self.plain(L), "~" * L, self.plain(L), "~" * L, cfg, flag)

    # ---- N count -----------------------------------------------------------------------------------------------------------------------
    def ncount(self):
        for limit in N_LIMITS:
            for path, trims in (("whole", {}), ("view", TRIMS)):
                cfg = cfg_of(n_base_limit=limit, **trims)
                name = "n/%d,%s" % (limit, path)
                for L in lengths(self.NW, self.lead):
                    if L < limit + 24:
                        continue
                    for mate in self.mates()[:2]:
                        # (stream order: read 2 is built from its end and reversed, so its trims swap sides)
                        f, t = (trims.get("trim_front", 0), trims.get("trim_tail", 0)) if mate == "r1" else (trims.get("trim_tail2", 0), trims.get("trim_front2", 0))
                        for cls, p in positions(L, self.NW, self.lead, mate == "r2"):
                            self.turn += 1
                            for count, kind, flag in ((limit, "quiet", GOOD), (limit + 1, "fire", BADNCT)):
                                st = L - t - count if p == L else place(p, count, f, L - t, self.turn & 1)
                                s = put(self.plain(L), st, "N" * count)
                                if trims and kind == "quiet":
                                    s = "N" * f + s[f:L - t] + "N" * t          # Ns in the trimmed-off part do not count
                                s = s[::-1] if mate == "r2" else s
                                o = self.plain(L)
                                s1, s2 = (s, o) if mate == "r1" else (o, s)
                                self.add("%s/L%d/%s/%s/%s" % (name, L, mate, cls, kind), s1, "I" * L, s2, "I" * L, cfg, flag)

    # ---- length and trim -----------------------------------------------------------------------------------------------------------------
    def bg_case(self, tag, cfg, l1, l2, flag, may_defer=None):
        self.add(tag, self.plain(l1), "I" * l1, self.plain(l2), "I" * l2, cfg, flag, may_defer)

    def length_trim(self):
        big = self.cap
        for L in sorted(set([150 - self.lead, big])):
            # read 1's view exactly seq_len_req / one short; a read 2 far shorter than seq_len_req is nobody's business
            for trims, cut in (({}, 0), (TRIMS, 5)):
                cfg = cfg_of(seq_len_req=L - 5, **trims)
                name = "len/req%d,%s" % (L - 5, "trim" if trims else "plain")
                self.bg_case("%s/L%d/r1/at/quiet" % (name, L - 5 + cut), cfg, L - 5 + cut, L, GOOD)
                self.bg_case("%s/L%d/r1/below/fire" % (name, L - 6 + cut), cfg, L - 6 + cut, L, BADLEN)
                self.bg_case("%s/L%d/r2/short-mate/quiet" % (name, L), cfg, L, 20 + cut, GOOD)
        # trims that swallow a mate whole: front >= len, tail >= len, front + tail >= len
        L = big
        for which, kw in (("front", dict(trim_front=400)), ("tail", dict(trim_tail=400)), ("both", dict(trim_front=200, trim_tail=200))):
            self.bg_case("trim/r1-%s-swallows/L%d/r1/whole/fire" % (which, L), cfg_of(**kw), L, L, BADTRIM1)
            self.bg_case("trim/r1-%s-swallows/L150/r1/whole/fire" % which, cfg_of(**kw), min(150, L), 20, BADTRIM1)
        if self.paired:
            for which, kw in (("front", dict(trim_front2=400)), ("tail", dict(trim_tail2=400)), ("both", dict(trim_front2=200, trim_tail2=200))):
                cfg = cfg_of(trim_front=1, **kw)
                self.bg_case("trim/r2-%s-swallows/L%d/r2/whole/fire" % (which, L), cfg, L, L, BADTRIM2)
                self.bg_case("trim/r2-%s-swallows/L150/r2/whole/fire" % which, cfg, 20, min(150, L), BADTRIM2)
        # final views of 4 and 5 bases (under BADTRIM1 the result's read 2 is the read as it came: the GPU test looks)
        cfg = cfg_of(**TRIMS)
        for l1, l2, flag in ((9, 9, BADTRIM1), (9, L, BADTRIM1), (10, 9, BADTRIM2), (L, 9, BADTRIM2), (10, 10, GOOD), (10, 30, GOOD), (30, 10, GOOD)):
            if not self.paired and flag == BADTRIM2:
                flag = GOOD                          # (there is no read 2: read 1's view of 5 bases or more is all there is)
            mate = "r1" if flag == BADTRIM1 or not self.paired else "r2" if flag == BADTRIM2 else "both"
            length = "L%d-%d" % (l1, l2) if self.paired else "L%d" % l1
            self.bg_case("trim/view45/%s/%s/whole/%s" % (length, mate, "fire" if flag else "quiet"), cfg, l1, l2, flag)
        # upstream's gate (preprocesser.py:455): read 2's trims alone trim nothing — an 8-base read 2 stays 8 bases, GOOD
        cfg = cfg_of(trim_front2=5, trim_tail2=7)
        for l1, l2 in ((L, L), (150 - self.lead, 150 - self.lead), (24, 8), (24, 12)):
            self.bg_case("trim/gate/L%d-%d/r2/whole/quiet" % (l1, l2), cfg, l1, l2, GOOD)

    # ---- several rules broken at once: upstream's order BADTRIM, BADLEN, BADPOL, BADLQC, BADNCT --------------------------------------------
    def order(self):
        cfg = cfg_of(seq_len_req=60, poly_size_limit=35, allow_mismatch_in_poly=2, unqualified_base_limit=10, n_base_limit=2, **TRIMS)
        L = min(150, self.cap)

        def dirty(n, poly=True, lowq=True, ns=True):
            """a read of n bases with a run of 40 A at base 4, three N behind it, and 20 unqualified bases, as asked"""
            s = self.plain(n, "CGT")
            if poly and n >= 50:
                s = put(s, 4, "A" * 40)
            if ns:
                s = put(s, min(46, n - 4), "NNN") if n >= 7 else "N" * n
            q = "I" * n
            if lowq:
                q = put(q, max(n - 24, 0), "#" * min(20, n))
            return s, q

        rows = [("badtrim1", dirty(8), dirty(L), BADTRIM1), ("badtrim2", dirty(L), dirty(9), BADTRIM2), ("badlen", dirty(60), dirty(L), BADLEN),
                ("badpol", dirty(L), dirty(L, poly=False), BADPOL), ("badpol-r2", dirty(L, poly=False, ns=False), dirty(L), BADPOL),
                ("badlqc", dirty(L, poly=False), dirty(L, poly=False), BADLQC), ("badnct", dirty(L, poly=False, lowq=False), dirty(L, False, True, False), BADNCT),
                ("badnct-r2", dirty(L, False, False, False), dirty(L, poly=False), BADNCT), ("good", dirty(L, False, False, False), dirty(L, False, True, False), GOOD)]
        for tag, (s1, q1), (s2, q2), flag in rows:
            if not self.paired and tag in ("badtrim2", "badpol-r2", "badnct-r2"):
                continue
            self.add("order/all/L%d/both/whole/%s" % (len(s1), tag), s1, q1, s2, q2, cfg, flag)

    # ---- rows the general kernel decides: the lane-per-read kernel packs A C G T N only, and no empty mate -------------------------------------
    def general(self):
        cfg = cfg_of(poly_size_limit=35, allow_mismatch_in_poly=2)
        L = min(150, self.cap)
        for cls, p in positions(L, self.NW, self.lead):
            # upstream counts 'a' apart from 'A': 35 of one fire, 20 + 20 of either do not
            st = L - 40 if p == L else place(p, 40, 0, L)
            self.add("general/lower/L%d/r1/%s/fire" % (L, cls), put(self.plain(L, "CGT"), st, "a" * 35), "I" * L, self.plain(L), "I" * L, cfg, BADPOL, "lower case")
            self.add("general/lower/L%d/r1/%s/quiet" % (L, cls), put(self.plain(L, "CGT"), st, "A" * 20 + "a" * 20), "I" * L, self.plain(L), "I" * L, cfg, GOOD, "lower case")
        # one byte outside A C G T N ends hasPolyX where it stands: in front of the run nothing fires, behind it the run has fired
        run = "A" * 40
        self.add("general/exotic/L%d/r1/first/quiet" % L, put(self.plain(L, "CGT"), 0, "R" + run), "I" * L, self.plain(L), "I" * L, cfg, GOOD, "exotic byte")
        self.add("general/exotic/L%d/r1/last/fire" % L, put(self.plain(L, "CGT"), L - 41, run + "R"), "I" * L, self.plain(L), "I" * L, cfg, BADPOL, "exotic byte")
        if self.paired:
            self.add("general/exotic/L%d/r2/last/quiet" % L, self.plain(L), "I" * L, put(self.plain(L, "CGT"), 0, "." + run), "I" * L, cfg, GOOD, "exotic byte")
            self.add("general/empty/L0-%d/r1/whole/quiet" % L, "", "", self.plain(L), "I" * L, cfg, GOOD, "empty mate")
            self.add("general/empty/L%d-0/r2/whole/quiet" % L, self.plain(L), "I" * L, "", "", cfg, GOOD, "empty mate")
            self.add("general/empty/L%d-0/r1/whole/fire" % L, put(self.plain(L, "CGT"), 9, run), "I" * L, "", "", cfg, BADPOL, "empty mate")
        else:
            self.add("general/empty/L0/r1/whole/quiet", "", "", None, None, cfg, GOOD, "empty mate")


_TABLES = {}


def cases(NW, paired, lead=0):
    """the table of a tier (NW in 10, 16, 18, 20); lead = PREFIX: every read 17 bases shorter, for the barcode instance"""
    key = (NW, bool(paired), lead)
    if key not in _TABLES:
        b = Builder(NW, bool(paired), lead)
        b.polyx()
        b.lowq()
        b.ncount()
        b.length_trim()
        b.order()
        b.general()
        _TABLES[key] = b.cases
    return list(_TABLES[key])


def background_flag(cfg, l1, l2, paired):
    """the flag of a pair of featureless background reads, qualified throughout (phred 95: nothing is), rule by rule"""
    v1, v2 = l1, l2
    if cfg["trim_front"] > 0 or cfg["trim_tail"] > 0:
        v1 = view_len(l1, cfg["trim_front"], cfg["trim_tail"])
        if v1 < 5:
            return BADTRIM1
        if paired:
            v2 = view_len(l2, cfg["trim_front2"], cfg["trim_tail2"])
            if v2 < 5:
                return BADTRIM2
    if v1 < cfg["seq_len_req"]:
        return BADLEN
    mp, need = cfg["poly_size_limit"], cfg["poly_size_limit"] - cfg["allow_mismatch_in_poly"]
    if mp > 0:
        assert need <= 1 or need >= 7           # a background window of W bases holds at most W / 4 + 2 copies of a letter
        if need <= 1 and (v1 >= mp or (paired and v2 >= mp)):
            return BADPOL
    if cfg["unqualified_base_limit"] > 0 and cfg["qualified_quality_phred"] + 33 > 127 and v1 > cfg["unqualified_base_limit"]:
        return BADLQC
    return GOOD


def with_tier(table, NW, lead=0):
    """the table plus, per config, one unrelated background record whose mates have 16 NW bases (NW = 0: 321), prefix included: it
    sets the batch's max_len, so the same table runs on any instance (choose_verdict_kernel, aqc_capi_run.hip)"""
    out = list(table)
    paired = table[0].seq2 is not None
    rng = random.Random(4177 + NW)
    L = (16 * NW if NW else 321) - lead
    for cfg, _ in by_config(table):
        q = qual_high(L, min(cfg["qualified_quality_phred"] + 33, 127))
        s1, s2 = background(rng, L), background(rng, L)
        out.append(Case("tier/%d/L%d/both/whole/record" % (NW, L), s1, q, s2 if paired else None, q if paired else None, cfg,
                        background_flag(cfg, L, L, paired), None))
    return out


def by_config(table):
    """-> [(cfg keywords, [cases])] in the order the configs first appear"""
    groups = {}
    for c in table:
        groups.setdefault(cfg_key(c.cfg), (c.cfg, []))[1].append(c)
    return list(groups.values())


def make_config(cfg, paired, **extra):
    """cfg keywords -> afterqc_amd.capi.Config (every filter the keywords leave out is off)"""
    from afterqc_amd import capi
    c = capi.Config()
    c.paired = 1 if paired else 0
    c.barcode_length = 12
    c.set_verify("CAGTA")
    c.qc_kmer = 8
    for k, v in list(cfg.items()) + list(extra.items()):
        setattr(c, k, v)
    return c


def pack(table, paired):
    from afterqc_amd import capi
    if paired:
        return capi.Batch.from_strings([c.seq1 for c in table], [c.qual1 for c in table], [c.seq2 for c in table], [c.qual2 for c in table])
    return capi.Batch.from_strings([c.seq1 for c in table], [c.qual1 for c in table])


# ---- the barcode instance: every mate gets a valid 12-base barcode + CAGTA in front (synth.add_barcodes shows the layout) ----------------
def barcode_for(other_mate):
    """a barcode whose reverse complement is twelve copies of a letter that is rare at the other mate's end and is not its last base:
    cleanBarcodeTail (barcodeprocesser.py:47-75) compares the other mate's last k bases with the tail of rc(barcode + verify) and wants an
    edit distance of at most k / 5 — here at least k minus the letter's count in those bases, so nothing is ever cut"""
    tail = other_mate[-PREFIX:]
    c = min((x for x in "ACGT" if not tail.endswith(x)), key=lambda x: (tail.count(x), x))
    return COMP[c] * 12


def with_barcodes(table):
    """-> (table with the prefix in front of every mate, expected flags): a mate of 18 bases or less, prefix included, has no barcode
    for detectBarcode (barcodeprocesser.py) — BADBCD1 / BADBCD2 for the rows with an empty mate"""
    out, flags = [], []
    for c in table:
        thr = c.cfg["qualified_quality_phred"] + 33
        pq = chr(min(max(thr - 1, 33), 126)) * PREFIX                   # unqualified where the config allows: the prefix is never counted
        if c.seq2 is None:
            out.append(c._replace(seq1="ACGTTGCAACGT" + "CAGTA" + c.seq1, qual1=pq + c.qual1))
            flags.append(BADBCD1 if len(c.seq1) <= 1 else c.flag)
        else:
            out.append(c._replace(seq1=barcode_for(c.seq2 or "A") + "CAGTA" + c.seq1, qual1=pq + c.qual1,
                                  seq2=barcode_for(c.seq1 or "A") + "CAGTA" + c.seq2, qual2=pq + c.qual2))
            flags.append(BADBCD1 if len(c.seq1) <= 1 else BADBCD2 if len(c.seq2) <= 1 else c.flag)
    return out, flags
