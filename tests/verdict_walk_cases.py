"""Constructed pairs for the verdict kernel's pair phase (csrc/aqc_fast.hpp from "overlap (util.py:158-212)" to the result store, and
its restatement in csrc/aqc_record.hpp): the diagonal scan, the accept rule, the adapter cut, the shifted diagonal and the three-step
correction walk, each at its threshold and at the borders of the kernel's words.  Not a test module: test_verdict_walk_cases_cpu.py
proves the table against the real reference's outputs (tests/golden/walk_cases.json.gz, made by tests/golden/make_walk.py),
oracle/pyloop.py and the C oracle; test_gpu_verdict_walk.py runs it through aqc_run on every tier.

A case is the filter table's tuple (tag, seq1, qual1, seq2, qual2, cfg keywords, flag, may_defer: reason | None) plus what the builder
states from how it made the pair:

  triple   (offset, overlap_len, distance) of the result record
  edits    [(o, kind, base, qual)] in walk order, n_edits their number
  counts   the pair's share of corrected / masked / skipped (in mismatches) / read_corrected / overlapped / adapter_base / adapter_read
  matrix   [(written, replaced)] error-matrix cells
  hists    (bin of overlap_hist, bin of distance_hist | None)
  final    the final lengths of both mates
  raises   upstream dies at this record (the trusted lower-case row): the row runs in a batch of its own

Nothing is computed by an implementation of the loop.  What makes that possible:

  * read 1 and reverse_r2 are seeded random A C G T, and reverse_r2 is a copy of the part of read 1 the geometry names: no other
    diagonal of 31 columns or more has fewer than three mismatches (chance ~4^-28 per diagonal), so util.overlap finds the planted
    diagonal or nothing;
  * mismatches are planted at stated columns with stated bases and qualities; every other quality is 'I' (phred 40);
  * whom the walk trusts is read off two lists, TRUST_HI and TRUST_LO — the byte values on the trusted side of q >= 30 and of
    q <= 14 among the values this table plants;
  * the accept rule (util.py:176-184: fewer than three mismatches, or the third at column 50 or later on a diagonal of 52 columns or
    more) is stated by `accepted`.

Tag: family / config / lengths / geometry / position class / kind.
  config          fix (the default), fix+mask, nocorr, nocorr+mask; rows about a filter add it (",req40", ",trims")
  geometry        fwd<d>, off0, rev<a> (the closed form), rev<a>-2nd (len1 < len2 + offset: "second scan"), shift<d>, short15 / short16
  position class  first, last, w16r1 / w16r2 (either side of a 16-base border of read 1's / reverse_r2's stream, "f" in front of the
                  border, "b" behind it), c49 c50 c51 c63 c64 c127 c128, tierlast (read 1's stream in the tier's last word), "+"-joined
                  where a column is several of them; the col/ cut/ view/ rows add "@column:whom the qualities trust"
  kind            per mismatch fixr2 / fixr1 / mask / skip, "+"-joined; none; reject, baddiff, badlen, badmismatch, raise"""
import hashlib
import random
from collections import namedtuple

from verdict_filter_cases import (PREFIX, TIER_FLOOR, TRIMS, by_config, cfg_of, make_config, pack, view_len,  # noqa: F401
                                  with_barcodes)
from verdict_filter_cases import with_tier as _filter_with_tier

Case = namedtuple("Case", "tag seq1 qual1 seq2 qual2 cfg flag may_defer triple edits n_edits counts matrix hists final raises")

GOOD, BADLEN, BADDIFF, BADMISMATCH = 0, 6, 10, 11
EDIT_FIX_R2, EDIT_FIX_R1, EDIT_MASK = 1, 2, 3
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
ALL_BASES = "ATCG"                                       # the order of the error matrix (qualitycontrol.py:24)

# quality bytes: phred 30 is byte 63, phred 14 is byte 47 (preprocesser.py:571,579)
TRUST_HI = (63, 64, 73, 126, 255)
TRUST_LO = (33, 35, 46, 47)
GRID_HI, GRID_LO = (62, 63, 64, 126, 255), (33, 46, 47, 48)
GRID_NEITHER = ((63, 63), (47, 47), (48, 62), (62, 48))
R2WRONG, R1WRONG, NEITHER = (73, 35), (35, 73), (73, 73)     # the everyday quality pairs (qa, qb)

CONFIGS = {"fix": dict(no_correction=0, mask_mismatch=0), "fix+mask": dict(no_correction=0, mask_mismatch=1),
           "nocorr": dict(no_correction=1, mask_mismatch=0), "nocorr+mask": dict(no_correction=1, mask_mismatch=1)}
COUNT_KEYS = ("corrected", "masked", "skipped", "read_corrected", "overlapped", "adapter_base", "adapter_read")
VIEWS = {"trims": dict(TRIMS), "trims-r1": dict(trim_front=3, trim_tail=2), "tail2": dict(trim_front=1, trim_tail2=3)}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def accepted(cols, n):
    """util.py:176-184 for a diagonal of n columns whose mismatches lie at `cols`"""
    cols = sorted(cols)
    return len(cols) < 3 or (cols[2] >= 50 and n >= 52)


def trusted(qa, qb):
    """-> "r2wrong" (read 1 is trusted), "r1wrong" or None"""
    if qa in TRUST_HI and qb in TRUST_LO:
        return "r2wrong"
    if qb in TRUST_HI and qa in TRUST_LO:
        return "r1wrong"
    assert not (qa >= 63 and qb <= 47) and not (qb >= 63 and qa <= 47), (qa, qb)       # (the lists cover what is planted)
    return None


Plant = namedtuple("Plant", "col b1 b2 qa qb")           # b1: read 1's base, b2: reverse_r2's base (None: whatever is there / another)


def plant(col, q=NEITHER, b1=None, b2=None):
    return Plant(col, b1, b2, q[0], q[1])


class Builder:
    def __init__(self, NW, lead=0, seed=20261022):
        self.NW, self.lead = NW, lead
        self.cap = 16 * NW - lead
        self.rng = random.Random(seed * 64 + NW * 2 + (1 if lead else 0))
        self.cases = []

    def rand(self, n):
        return "".join(self.rng.choice("ACGT") for _ in range(n))

    def other(self, b):
        return "ACGT"[("ACGT".index(b) + 1 + self.rng.randrange(3)) % 4] if b in "ACGT" else "A"

    # ---- one pair -----------------------------------------------------------------------------------------------------------------------
    def outcome(self, p, o, b1, b2, cfg, edits, counts, matrix):
        """one mismatch of the walk at column o: read 1 holds b1, reverse_r2 holds b2 -> its kind"""
        who = trusted(p.qa, p.qb)
        if who and b1 != "N" and b2 != "N" and b1 in COMP and b2 in COMP:
            # (written, replaced): read 2 := complement(b1) where it held complement(b2) / read 1 := b2 where it held b1
            matrix.append((COMP[b1], COMP[b2]) if who == "r2wrong" else (b2, b1))
        if who and not cfg["no_correction"]:
            if who == "r2wrong":
                edits.append((o, EDIT_FIX_R2, COMP[b1], p.qa))
            else:
                edits.append((o, EDIT_FIX_R1, b2, p.qb))
            counts["corrected"] += 1
            return "fix" + who[:2]
        if cfg["mask_mismatch"]:
            edits.append((o, EDIT_MASK, "\0", 33))
            counts["masked"] += 1
            return "mask"
        counts["skipped"] += 1
        return "skip"

    def pair(self, family, config, len1, len2, geo, plants, cls, extra=None, view=None, may_defer=None, walk=None, lower=None,
             raises=False, geo_name=None):
        """geo: ("fwd", d) — read 1 from d on against reverse_r2 from its start; ("rev", a) — read 1 from its start against reverse_r2
        from a on.  plants: the mismatches of that diagonal.  walk: for a shifted pair (len2 < len1 - d) the mismatches of the walk's
        own diagonal, read 1's last len2 bases against reverse_r2.  view: a key of VIEWS — both mates get the bases the trims take.
        lower: (column, case of read 1's base) — read 1 holds a lower-case letter where reverse_r2 holds the same letter in capitals."""
        cfg = cfg_of(**CONFIGS[config])
        cfg.update(extra or {})
        if view:
            cfg.update(VIEWS[view])
        how, d = geo
        r1 = list(self.rand(len1))
        rr2 = list(self.rand(len2))
        q1, q2r = [73] * len1, [73] * len2                  # q2r: read 2's qualities in reverse_r2's order
        if how == "fwd":
            n = min(len1 - d, len2)
            i0, j0 = d, 0
        else:
            n = min(len1, len2 - d)
            i0, j0 = 0, d
        # the diagonal is one util.overlap looks at: 31 columns or more before the shorter mate ends it
        assert n >= 1 and (len1 - d >= 31 if how == "fwd" else 0 < d and len2 - d >= 31), (len1, len2, geo)
        rr2[j0:j0 + n] = r1[i0:i0 + n]
        shifted = how == "fwd" and len2 < len1 - d
        if shifted and walk is not None:
            assert len1 >= d + 2 * len2                     # the walk's diagonal lies behind the accepted one: it can be planted freely
            r1[len1 - len2:] = rr2
        cols = sorted(p.col for p in plants)
        assert len(set(cols)) == len(cols) and all(0 <= c < n for c in cols)
        bases = {}
        for p in plants:
            if shifted:                                     # in read 1, so that reverse_r2 stays what the walk's diagonal copies
                r1[i0 + p.col] = self.other(rr2[j0 + p.col])
            else:
                if p.b1:
                    r1[i0 + p.col] = p.b1
                b1 = r1[i0 + p.col]
                rr2[j0 + p.col] = p.b2 if p.b2 else self.other(b1)
                assert rr2[j0 + p.col] != b1
                q1[i0 + p.col], q2r[j0 + p.col] = p.qa, p.qb
                bases[p.col] = (b1, rr2[j0 + p.col])
        if lower:
            p = plant(lower[0], lower[2] if len(lower) > 2 else NEITHER)
            r1[i0 + p.col], rr2[j0 + p.col] = lower[1].lower(), lower[1]
            q1[i0 + p.col], q2r[j0 + p.col] = p.qa, p.qb
            bases[p.col] = (lower[1].lower(), lower[1])
            plants = list(plants) + [p]
            cols = sorted(cols + [p.col])
        # ---- what upstream does with it, step by step (preprocesser.py:515-617)
        counts = dict((k, 0) for k in COUNT_KEYS)
        edits, matrix, kinds = [], [], []
        flag, f1, f2 = GOOD, len1, len2
        ok = accepted(cols, n)
        if not ok:
            triple, hists = (0, 0, 0), (0, 0)
            kinds = ["reject" if cols else "none"]
        else:
            off, dist = (d if how == "fwd" else -d), len(cols)
            hist0 = n
            second = None
            if off < 0 and n > 30:
                counts["adapter_base"], counts["adapter_read"] = 2 * d, 1
                f1 = f2 = n
                if len1 < len2 - d:
                    # the cut reads: read 1 whole, reverse_r2's last len1 bases — the planted diagonal is now the forward one at
                    # len2 - len1 - d, of len1 minus that many columns (the walk's rows keep 31 or more)
                    s = len2 - len1 - d
                    assert len1 - s >= 31 and not cols and may_defer == "second scan"
                    second = (s, len1 - s, 0)
                off = 0
            if off == 0 and how == "rev" and n > 30 and n < cfg["seq_len_req"]:
                flag, triple, hists = BADLEN, (0, 0, 0), (hist0, None)
                kinds = ["badlen"]
            else:
                triple = second or (off, n, dist)
                hists = (hist0, dist)
                if dist > 3:
                    flag = BADDIFF
                    kinds = ["baddiff"]
                elif triple[1] > 30:
                    counts["overlapped"] = 1
                    if dist and not shifted:
                        if raises:
                            kinds = ["raise"]               # upstream indexes its error matrix with the lower-case letter: KeyError
                        for p in ([] if raises else sorted(plants, key=lambda p: p.col)):
                            kinds.append(self.outcome(p, p.col, bases[p.col][0], bases[p.col][1], cfg, edits, counts, matrix))
                    elif dist:
                        # the walk's own diagonal: the first `dist` of its mismatches; fewer than that: BADMISMATCH with the edits
                        # made so far, no counter and no cell
                        assert walk is not None
                        for p in sorted(walk, key=lambda p: p.col):
                            x = len1 - len2 + p.col
                            r1[x] = p.b1 or self.other(rr2[p.col])
                            assert r1[x] != rr2[p.col]
                            q1[x], q2r[p.col] = p.qa, p.qb
                        for p in sorted(walk, key=lambda p: p.col)[:dist]:
                            kinds.append(self.outcome(p, p.col, r1[len1 - len2 + p.col], rr2[p.col], cfg, edits, counts, matrix))
                        if len(walk) < dist:
                            flag, matrix, kinds = BADMISMATCH, [], kinds + ["badmismatch"]
                            for k in ("corrected", "masked", "skipped"):
                                counts[k] = 0
                    else:
                        kinds = ["none"]
                else:
                    kinds = ["none" if not dist else "unwalked"]
        if counts["corrected"]:
            counts["read_corrected"] = 1
        # ---- the records as they are uploaded
        s1, s2 = "".join(r1), rc("".join(rr2))
        a1, a2 = "".join(chr(q) for q in q1), "".join(chr(q) for q in reversed(q2r))
        if view:
            # the bases the trims take: random ones, of a quality that is neither high nor low
            tf, tt = cfg["trim_front"], cfg["trim_tail"]
            tf2, tt2 = cfg["trim_front2"], cfg["trim_tail2"]
            s1, a1 = self.rand(tf) + s1 + self.rand(tt), "5" * tf + a1 + "5" * tt
            s2, a2 = self.rand(tf2) + s2 + self.rand(tt2), "5" * tf2 + a2 + "5" * tt2
        assert max(len(s1), len(s2)) <= self.cap, (family, len(s1), len(s2), self.cap)
        config += "".join(",%s%s" % (k[:7], v) for k, v in sorted((extra or {}).items())) + ("," + view if view else "")
        geo_name = geo_name or ("shift%d" % d if shifted else "rev%d" % d if how == "rev" else "fwd%d" % d if d else "off0")
        tag = "%s/%s/L%d-%d/%s/%s/%s" % (family, config, len(s1), len(s2), geo_name, cls, "+".join(kinds))
        self.cases.append(Case(tag, s1, a1, s2, a2, cfg, None if raises else flag, may_defer, None if raises else triple, None if raises else edits,
                               None if raises else len(edits), counts, matrix, hists, (f1, f2), raises))
        return self.cases[-1]

    # ---- the position classes of a geometry -------------------------------------------------------------------------------------------------
    def columns(self, len1, len2, geo):
        """-> [(class, o)] for one mismatch of the accepted diagonal, which is the walk's (no shifted pair here)"""
        how, d = geo
        n = min(len1 - d, len2) if how == "fwd" else min(len1, len2 - d)
        x1 = d if how == "fwd" else 0                        # read 1's stream position of column 0 (the cut pair's walk starts at base 0)
        x2 = 0 if how == "fwd" else d                        # reverse_r2's
        streams = [(x1, "w16r1"), (x2, "w16r2")] + ([(x1 + self.lead, "w16r1")] if self.lead else [])    # (the raw read, prefix included)
        found = {}

        def note(o, cls):
            if 0 <= o < n:
                found.setdefault(o, []).append(cls)
        note(0, "first")
        note(n - 1, "last")
        for x0, name in streams:
            first = (-x0) % 16 or 16                           # the first column whose stream position is a multiple of 16
            last = first + 16 * ((n - 1 - first) // 16) if n - 1 >= first else None
            for b in sorted(set([first] + ([last] if last else []))):
                note(b - 1, name + "f")
                note(b, name + "b")
        for c in (49, 50, 51, 63, 64, 127, 128):
            note(c, "c%d" % c)
        top = 16 * (self.NW - 1) - x1 - self.lead                         # the first column in the tier's last word of read 1's stream
        if 0 <= top < n:
            note(top, "tierlast")
        return [("+".join(sorted(set(found[o]))), o) for o in sorted(found)]

    # ---- families -----------------------------------------------------------------------------------------------------------------------
    def qual(self):
        """one mismatch at column 20 of a 40-base overlap, read 1 from base 7 on: the trust rule on the whole grid, every config"""
        for config in CONFIGS:
            grid = [(a, b) for a in GRID_HI for b in GRID_LO]
            for qa, qb in grid + [(b, a) for a, b in grid] + [q for q in GRID_NEITHER if q not in grid and q[::-1] not in grid]:
                self.pair("qual", config, 47, 44, ("fwd", 7), [plant(20, (qa, qb))], "q%d,%d" % (qa, qb))

    def matrix(self):
        for config in ("fix", "nocorr+mask"):
            for x in "ACGT":
                for y in "ACGT":
                    if x != y:
                        # read 1 holds x, reverse_r2 holds y: trusted from either side
                        self.pair("matrix", config, 50, 50, ("fwd", 9), [plant(17, R2WRONG, x, y)], "%s%s-r2wrong" % (x, y))
                        self.pair("matrix", config, 50, 50, ("fwd", 9), [plant(17, R1WRONG, x, y)], "%s%s-r1wrong" % (x, y))
            for x, y in (("N", "A"), ("N", "G"), ("C", "N"), ("T", "N")):
                for q, who in ((R2WRONG, "r2wrong"), (R1WRONG, "r1wrong"), (NEITHER, "neither")):
                    # (columns 17 and 31: the N plane's bit next to a 16-base border of reverse_r2's stream as well)
                    self.pair("matrix", config, 50, 50, ("fwd", 9), [plant(17, q, x, y)], "%s%s-%s" % (x, y, who))
                    self.pair("matrix", config, 50, 50, ("fwd", 1), [plant(31, q, x, y)], "%s%s-%s" % (x, y, who))
            # N against N is no mismatch
            c = self.pair("matrix", config, 50, 50, ("fwd", 9), [], "NN-none")
            s1, s2 = list(c.seq1), list(c.seq2)
            s1[9 + 17] = "N"
            s2[len(s2) - 1 - 17] = "N"
            self.cases[-1] = c._replace(seq1="".join(s1), seq2="".join(s2))

    def count(self):
        q3 = {"r2": R2WRONG, "r1": R1WRONG, "x": NEITHER}
        for config in CONFIGS:
            # distance 0 .. 3; all three in one 16-base word of both streams, and in three different words
            self.pair("count", config, 76, 76, ("fwd", 16), [], "d0")
            self.pair("count", config, 76, 76, ("fwd", 16), [plant(33, R2WRONG)], "d1")
            self.pair("count", config, 76, 76, ("fwd", 16), [plant(33, R2WRONG), plant(40, R1WRONG)], "d2")
            self.pair("count", config, 76, 76, ("fwd", 16), [plant(50, R2WRONG), plant(53, R1WRONG), plant(59, NEITHER)], "d3-oneword")
            self.pair("count", config, 76, 76, ("fwd", 16), [plant(10, R2WRONG), plant(30, R1WRONG), plant(55, NEITHER)], "d3-threewords")
        for config in ("fix", "fix+mask", "nocorr+mask"):
            # mixed outcomes in every order: with fix the third kind fills no edit slot, with fix+mask it fills one
            for order in (("r2", "r1", "x"), ("r2", "x", "r1"), ("r1", "r2", "x"), ("r1", "x", "r2"), ("x", "r2", "r1"), ("x", "r1", "r2"),
                          ("x", "x", "r2"), ("r1", "x", "x"), ("x", "r2", "x"), ("r2", "r2", "r2"), ("r1", "r1", "r1"), ("x", "x", "x")):
                self.pair("count", config, 70, 70, ("fwd", 3), [plant(c, q3[k]) for c, k in zip((14, 47, 58), order)], "d3-" + "-".join(order))
            for order in (("r2", "x"), ("x", "r2"), ("r1", "x"), ("x", "r1"), ("r1", "r2"), ("r2", "r1"), ("x", "x")):
                self.pair("count", config, 56, 49, ("fwd", 15), [plant(c, q3[k]) for c, k in zip((15, 16), order)], "d2-" + "-".join(order))

    def col_rows(self, family, config, len1, len2, geo, view=None, extra=None):
        for cls, o in self.columns(len1, len2, geo):
            for q in ((R2WRONG, R1WRONG, NEITHER) if cls in ("first", "last") or config != "fix" else (R2WRONG, R1WRONG)):
                # (the class names the column and whom the qualities trust: r2 = read 2 is wrong, r1, x = neither)
                who = {R2WRONG: "r2", R1WRONG: "r1", NEITHER: "x"}[q]
                self.pair(family, config, len1, len2, geo, [plant(o, q)], "%s@%d:%s" % (cls, o, who), view=view, extra=extra)

    def geometries(self):
        """(len1, len2, geo): forward with the scan's word shift 0, smallest and largest; offset 0; the tier's lengths"""
        out = [(56, 60, ("fwd", 16)), (57, 57, ("fwd", 1)), (72, 70, ("fwd", 15)), (75, 60, ("fwd", 17)), (61, 61, ("fwd", 0)), (40, 75, ("fwd", 0))]
        for raw in sorted(set([16 * self.NW, 16 * self.NW - 1, TIER_FLOOR[self.NW] + 1])):
            L = raw - self.lead
            if L >= 40:
                out += [(L, L, ("fwd", 1)), (L - 1, L, ("fwd", 0)), (L, L, ("fwd", min(31, L - 33)))]
        return out

    def col(self):
        for len1, len2, geo in self.geometries():
            self.col_rows("col", "fix", len1, len2, geo)
        self.col_rows("col", "fix+mask", 72, 70, ("fwd", 15))
        self.col_rows("col", "nocorr", 57, 57, ("fwd", 1))

    def gate(self):
        for config in ("fix", "fix+mask"):
            # the third mismatch at column 49, 50 or 51 of a diagonal of 51, 52 or 53 columns
            for n in (51, 52, 53):
                for third in (49, 50, 51):
                    if third < n:
                        self.pair("gate", config, n + 5, n + 2, ("fwd", 5), [plant(3, R2WRONG), plant(21, R1WRONG), plant(third, NEITHER)],
                                  "n%d-third-c%d" % (n, third))
            # distance 4: two in front of column 50, two behind; distance 40
            self.pair("gate", config, 75, 70, ("fwd", 5), [plant(c) for c in (12, 49, 50, 69)], "d4")
            self.pair("gate", config, 112, 100, ("fwd", 12), [plant(c) for c in [10, 30] + list(range(51, 89))], "d40")
            # overlap_len 30, 31, 32 with 0 and 2 mismatches: 30 columns are a diagonal only for a mate of 30 bases
            for n in (30, 31, 32):
                for k, pl in ((0, []), (2, [plant(4, R2WRONG), plant(n - 1, R1WRONG)])):
                    self.pair("gate", config, max(n, 31) + 20, n, ("fwd", 20), pl, "ovl%d-d%d" % (n, k))
                    if n > 30:
                        self.pair("gate", config, n + 2, n + 6, ("fwd", 2), pl, "ovl%d-d%d" % (n, k))
            # the scan's 16-base prefix filter at its bound: two mismatches in columns 0..15 that differ in both bits of the 2-bit code
            self.pair("gate", config, 60, 58, ("fwd", 6), [plant(2, R2WRONG, "A", "G"), plant(13, R1WRONG, "C", "T")], "prefix-AG-CT")
            self.pair("gate", config, 60, 58, ("fwd", 16), [plant(0, R1WRONG, "G", "A"), plant(15, R2WRONG, "T", "C")], "prefix-GA-TC")
            self.pair("gate", config, 59, 60, ("rev", 1), [plant(0, R1WRONG, "T", "C"), plant(15, R2WRONG, "A", "G")], "prefix-TC-AG")

    def cut(self):
        for config in ("fix", "fix+mask"):
            for a in (1, 16, 17):
                for n in (31, 60):
                    # the closed form: len1 >= len2 - a
                    self.pair("cut", config, n + 9, n + a, ("rev", a), [], "ovl%d" % n)
                    self.pair("cut", config, n, n + a, ("rev", a), [plant(5, R2WRONG), plant(n - 1, R1WRONG)], "ovl%d-len1" % n)
                    # seq_len_req at overlap_len and one above
                    self.pair("cut", config, n + 9, n + a, ("rev", a), [plant(7, R2WRONG)], "req-at", extra=dict(seq_len_req=n))
                    self.pair("cut", config, n + 9, n + a, ("rev", a), [plant(7, R2WRONG)], "req-above", extra=dict(seq_len_req=n + 1))
                # len1 < len2 - a: the cut pair is scanned again
                self.pair("cut", config, 50, 50 + a + 9, ("rev", a), [], "ovl50", may_defer="second scan", geo_name="rev%d-2nd" % a)
            # offset -1 with overlap_len 30: no cut
            self.pair("cut", config, 30, 34, ("rev", 3), [], "ovl30-nocut")
            self.pair("cut", config, 30, 32, ("rev", 1), [plant(3), plant(29)], "ovl30-nocut")
        for a in (1, 17):
            self.col_rows("cut", "fix", 70, 64 + a, ("rev", a))
        self.col_rows("cut", "fix+mask", 66, 80, ("rev", 16))
        L = 16 * self.NW - self.lead
        self.col_rows("cut", "fix", L, L, ("rev", 1))
        self.col_rows("cut", "fix", L - 1, L, ("rev", 17))

    def shift(self):
        for config in ("fix", "fix+mask", "nocorr"):
            for d, len2 in ((0, 33), (1, 31), (15, 40), (16, 36)):
                len1 = d + 2 * len2 + 5
                two = [plant(4), plant(len2 - 2)]
                # more mismatches on the walk's diagonal than `distance`, exactly as many, fewer, none
                self.pair("shift", config, len1, len2, ("fwd", d), two, "more", walk=[plant(0, R2WRONG), plant(16, R1WRONG), plant(len2 - 1, R2WRONG)])
                self.pair("shift", config, len1, len2, ("fwd", d), two, "exact", walk=[plant(15, R1WRONG), plant(len2 - 1, NEITHER)])
                self.pair("shift", config, len1, len2, ("fwd", d), two, "fewer", walk=[plant(len2 - 16, R2WRONG)])
                self.pair("shift", config, len1, len2, ("fwd", d), two[:1], "zero", walk=[])
                self.pair("shift", config, len1, len2, ("fwd", d), [], "d0", walk=[plant(3, R2WRONG)])
        # three mismatches: the accepted diagonal has its third behind column 50
        for d in (0, 17):
            three = [plant(7), plant(33), plant(52)]
            self.pair("shift", "fix", d + 2 * 60 + 3, 60, ("fwd", d), three, "more", walk=[plant(c, q) for c, q in ((0, R1WRONG), (31, R2WRONG), (32, NEITHER), (59, R2WRONG))])
            self.pair("shift", "fix+mask", d + 2 * 60 + 3, 60, ("fwd", d), three, "fewer", walk=[plant(47, NEITHER), plant(48, R1WRONG)])
        L = 16 * self.NW - self.lead
        len2 = (L - 1) // 2
        self.pair("shift", "fix", L, len2, ("fwd", 1), [plant(0), plant(len2 - 1)], "more", walk=[plant(len2 - 17, R1WRONG), plant(len2 - 2, R2WRONG), plant(len2 - 1, R2WRONG)])
        self.pair("shift", "fix", L, len2, ("fwd", 1), [plant(0), plant(len2 - 1)], "fewer", walk=[plant(len2 - 1, R2WRONG)])

    def view(self):
        for name in VIEWS:
            self.col_rows("view", "fix", 72, 70, ("fwd", 15), view=name)
            self.col_rows("view", "fix+mask", 57, 57, ("fwd", 1), view=name)
            self.col_rows("view", "fix", 66, 64 + 17, ("rev", 17), view=name)
            self.pair("view", "fix", 90, 35, ("fwd", 16), [plant(4), plant(30)], "more", view=name, walk=[plant(0, R2WRONG), plant(16, R1WRONG), plant(34, R2WRONG)])
            self.pair("view", "fix", 90, 35, ("fwd", 16), [plant(4), plant(30)], "fewer", view=name, walk=[plant(34, R1WRONG)])

    def general(self):
        for config in ("fix", "fix+mask"):
            # a mate of 15 bases against one of 31 or more: the lane-per-read kernel hands it on; 16 bases: it does not
            for short, name in ((15, "short15"), (16, "short16")):
                md = "short16" if short == 15 else None
                self.pair("general", config, 45, short, ("fwd", 5), [], "r2", may_defer=md, geo_name=name)
                self.pair("general", config, short, 45, ("rev", 3), [], "r1", may_defer=md, geo_name=name)
            for a in (1, 17):
                self.pair("general", config, 40, 40 + a + 6, ("rev", a), [], "ovl40", may_defer="second scan", geo_name="rev%d-2nd" % a)
            # a case-only difference is a mismatch to the scan and to the walk
            self.pair("general", config, 60, 60, ("fwd", 8), [], "lower-untrusted", may_defer="lower case", lower=(19, "A"))
            self.pair("general", config, 60, 60, ("fwd", 8), [plant(3, R2WRONG)], "lower-untrusted", may_defer="lower case", lower=(19, "G"))
        self.pair("general", "fix", 60, 60, ("fwd", 8), [], "lower-trusted", may_defer="lower case", lower=(19, "A", R2WRONG), raises=True)
        self.pair("general", "nocorr", 60, 60, ("fwd", 8), [], "lower-trusted", may_defer="lower case", lower=(19, "C", R1WRONG), raises=True)


_TABLES = {}


def cases(NW, lead=0):
    """the table of a tier (NW in 10, 16, 18, 20); lead = PREFIX: every read at most 16 NW - 17 bases, for the barcode instance"""
    key = (NW, lead)
    if key not in _TABLES:
        b = Builder(NW, lead)
        for family in (b.qual, b.matrix, b.count, b.col, b.gate, b.cut, b.shift, b.view, b.general):
            family()
        assert len(set(c.tag for c in b.cases)) == len(b.cases)
        _TABLES[key] = b.cases
    return list(_TABLES[key])


def with_tier(table, NW, lead=0):
    """the table plus, per config, the filter table's unrelated background record of 16 NW bases (NW = 0: 321), prefix included"""
    zero = dict((k, 0) for k in COUNT_KEYS)
    out = []
    for c in _filter_with_tier(table, NW, lead):
        if not isinstance(c, Case):
            gate = c.cfg["trim_front"] > 0 or c.cfg["trim_tail"] > 0
            v1 = view_len(len(c.seq1), c.cfg["trim_front"], c.cfg["trim_tail"]) if gate else len(c.seq1)
            v2 = view_len(len(c.seq2), c.cfg["trim_front2"], c.cfg["trim_tail2"]) if gate else len(c.seq2)
            c = Case(c.tag, c.seq1, c.qual1, c.seq2, c.qual2, c.cfg, c.flag, None, (0, 0, 0), [], 0, dict(zero), [], (0, 0), (v1, v2), False)
        out.append(c)
    return out


def digest(table):
    """of everything a run reads: the records and their configs, in order"""
    h = hashlib.sha256()
    for c in table:
        h.update(repr((c.tag, c.seq1, c.qual1, c.seq2, c.qual2, sorted(c.cfg.items()))).encode("latin-1"))
    return h.hexdigest()


def matrix_index(written, replaced):
    """the cell's place among the 16 error-matrix counters"""
    return ALL_BASES.index(written) * 4 + ALL_BASES.index(replaced)
