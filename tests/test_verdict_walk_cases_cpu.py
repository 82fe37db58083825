"""The case table of tests/verdict_walk_cases.py, before a kernel sees it: every value the builder states — flag, triple, edits, final
lengths, the pair's share of every counter, its error-matrix cells and histogram bins — is what the REAL reference did with the same
records (tests/golden/walk_cases.json.gz, made by tests/golden/make_walk.py), what oracle/pyloop.py's process_pair does and what the C
oracle writes into its result records and counters; and the table holds what it says it holds, read off its tags."""
import gzip
import json
import os

import numpy as np
import pytest

import verdict_walk_cases as vwc
from afterqc_amd import capi
from oracle import oracle, pyloop

TIERS = (10, 16, 18, 20)
HERE = os.path.dirname(os.path.abspath(__file__))
_FIXTURE = {}


def fixture(NW, lead):
    if not _FIXTURE:
        with gzip.open(os.path.join(HERE, "golden", "walk_cases.json.gz"), "rt") as f:
            for t in json.load(f)["tables"]:
                _FIXTURE[(t["NW"], t["lead"])] = t
    return _FIXTURE[(NW, lead)]


def parts(tag):
    """family, config, lengths, geometry, position class, kind"""
    return tag.split("/")[:6]


def starts(c):
    """where the final views begin (preprocesser.py:455-466: read 1's trims open the gate for both mates)"""
    gate = c.cfg["trim_front"] > 0 or c.cfg["trim_tail"] > 0
    return (c.cfg["trim_front"], c.cfg["trim_front2"]) if gate else (0, 0)


def stated_record(c):
    """the result record the builder's statements add up to"""
    r = np.zeros(1, dtype=capi.RESULT_DTYPE)[0]
    r["flag"], r["n_edits"] = c.flag, c.n_edits
    (r["start1"], r["start2"]), (r["len1"], r["len2"]) = starts(c), c.final
    r["offset"], r["overlap_len"], r["distance"] = c.triple
    for k, (o, kind, base, qual) in enumerate(c.edits):
        r["edits"][k] = (o, kind, ord(base), qual)
    return r


def reference_reads(c, row):
    """the reference's final reads of a row of the fixture: [seq1, qual1, seq2, qual2]"""
    _, st1, l1, st2, l2, patches = row
    out = [bytearray(c.seq1[st1:st1 + l1], "latin-1"), bytearray(c.qual1[st1:st1 + l1], "latin-1"),
           bytearray(c.seq2[st2:st2 + l2], "latin-1"), bytearray(c.qual2[st2:st2 + l2], "latin-1")]
    for mate, line, pos, byte in patches:
        out[2 * (mate - 1) + (line == 3)][pos] = byte
    return [bytes(x) for x in out]


def stated_totals(group):
    """the config's counters as the stats JSON names them, summed over the rows' shares"""
    rows = [c for c in group if not c.raises]
    tot = dict((k, sum(c.counts[k] for c in rows)) for k in vwc.COUNT_KEYS)
    matrix = np.zeros(16, dtype=np.int64)
    for c in rows:
        for w, r in c.matrix:
            matrix[vwc.matrix_index(w, r)] += 1
    ovl, dist = np.zeros(capi.AQC_QC_COLS, dtype=np.int64), np.zeros(capi.AQC_QC_COLS, dtype=np.int64)
    for c in rows:
        ovl[c.hists[0]] += 1
        if c.hists[1] is not None:
            dist[c.hists[1]] += 1
    flags = np.bincount([c.flag for c in rows], minlength=capi.N_FLAGS)
    return tot, matrix, ovl, dist, flags


def test_constants_are_the_abi_s():
    for name in ("GOOD", "BADLEN", "BADDIFF", "BADMISMATCH", "EDIT_FIX_R2", "EDIT_FIX_R1", "EDIT_MASK"):
        assert getattr(vwc, name) == getattr(capi, name) == getattr(pyloop, name), name
    assert vwc.ALL_BASES == "".join(pyloop.ALL_BASES)
    # phred 30 and 14 as bytes, and the lists on the right side of them
    assert min(vwc.TRUST_HI) == 30 + 33 and max(vwc.TRUST_LO) == 14 + 33
    assert 62 in vwc.GRID_HI and 63 in vwc.GRID_HI and 47 in vwc.GRID_LO and 48 in vwc.GRID_LO


@pytest.mark.parametrize("lead", [0, vwc.PREFIX])
@pytest.mark.parametrize("NW", TIERS)
def test_stated_values_are_the_reference_s(NW, lead):
    """the fixture: destination and flag, final lengths and starts, the final reads (the stated edits applied by oracle.final_read
    against the reference's bytes), and per config every counter, the matrix and both histograms"""
    table = vwc.with_tier(vwc.cases(NW, lead), NW, lead)
    fx = fixture(NW, lead)
    assert vwc.digest(table) == fx["digest"], "tests/golden/make_walk.py has to run again"
    groups = vwc.by_config(table)
    assert len(groups) == len(fx["configs"])
    bad, n_raise = [], 0
    for (cfg, group), ref in zip(groups, fx["configs"]):
        assert cfg == ref["cfg"]
        assert ref["index"] == [i for i, c in enumerate(group) if not c.raises]
        assert [i for i, _ in ref["raises"]] == [i for i, c in enumerate(group) if c.raises]
        n_raise += len(ref["raises"])
        for i, (flag, st1, l1, st2, l2, patches) in zip(ref["index"], ref["rows"]):
            c = group[i]
            if capi.FLAG_NAMES[c.flag] != flag or (l1, l2) != c.final or (st1, st2) != tuple(s if n else 0 for s, n in zip(starts(c), c.final)):
                bad.append((c.tag, "flag / lengths", capi.FLAG_NAMES[c.flag], c.final, starts(c), flag, (l1, l2), (st1, st2)))
                continue
            want = reference_reads(c, (flag, st1, l1, st2, l2, patches))
            r = stated_record(c)
            got = oracle.final_read(c.seq1.encode("latin-1"), c.qual1.encode("latin-1"), r, 1) + \
                oracle.final_read(c.seq2.encode("latin-1"), c.qual2.encode("latin-1"), r, 2)
            if want != list(got):
                bad.append((c.tag, "final reads", c.edits, patches))
        tot, matrix, ovl, dist, flags = stated_totals(group)
        o, s = ref["overlap"], ref["summary"]
        got = dict(corrected=o["corrected_bases"], read_corrected=o["corrected_reads"], skipped=o["skipped_correction_bases"],
                   masked=o["zero_qual_masked"], overlapped=o["overlapped_pairs"], adapter_base=o["trimmed_adapter_bases"],
                   adapter_read=o["trimmed_adapter_reads"])
        # (upstream counts a masked or skipped mismatch as two bases, preprocesser.py:608-610)
        assert got == dict(tot, skipped=2 * tot["skipped"], masked=2 * tot["masked"]), cfg
        assert [o["error_matrix"][w][r] for w in vwc.ALL_BASES for r in vwc.ALL_BASES if w != r] == \
            [int(matrix[vwc.matrix_index(w, r)]) for w in vwc.ALL_BASES for r in vwc.ALL_BASES if w != r], cfg
        assert not any(matrix[vwc.matrix_index(b, b)] for b in vwc.ALL_BASES)
        assert o["edit_distance_histogram"] == dist[:10].tolist(), cfg
        assert ref["overlap_hist"] == ovl[:len(ref["overlap_hist"])].tolist() and not ovl[len(ref["overlap_hist"]):].any(), cfg
        assert (o["bad_diff"], o["bad_mismatch_reads"], s["bad_reads_with_bad_read_length"]) == (flags[capi.BADDIFF], flags[capi.BADMISMATCH], flags[capi.BADLEN]), cfg
        assert (s["good_reads"], s["total_reads"]) == (flags[capi.GOOD], len(ref["index"])), cfg
    assert not bad, (len(bad), bad[:6])
    assert n_raise == 2


@pytest.mark.parametrize("lead", [0, vwc.PREFIX])
@pytest.mark.parametrize("NW", TIERS)
def test_stated_values_are_pyloop_s_and_the_oracle_s(NW, lead):
    """pyloop record by record, the C oracle batch by batch (one per config): whole result records, counters, matrix, histograms;
    for the widest table also with the 321-base records that send the batch to the general kernel"""
    table = vwc.with_tier(vwc.cases(NW, lead), NW, lead)
    if NW == 20:
        table += [c for c in vwc.with_tier(vwc.cases(NW, lead), 0, lead) if c.tag.startswith("tier/")]
    bad = []
    for cfg, group in vwc.by_config(table):
        rows = [c for c in group if not c.raises]
        for c in rows:
            r = pyloop.process_pair(c.seq1, c.qual1, c.seq2, c.qual2, dict(cfg, no_overlap=0))
            got = (r["flag"], (r["offset"], r["overlap_len"], r["distance"]), [(o, k, b, ord(q)) for o, k, b, q in r["edits"]], (len(r["seq1"]), len(r["seq2"])))
            if got != (c.flag, c.triple, c.edits, c.final):
                bad.append(("pyloop", c.tag, (c.flag, c.triple, c.edits, c.final), got))
        eng = oracle.OracleEngine()
        eng.set_config(vwc.make_config(cfg, True))
        eng.reset_stats()
        eng.upload(0, vwc.pack(rows, True))
        eng.run(0)
        res, cnt, (ovl_hist, dist_hist) = eng.fetch_results(0), eng.counters(), eng.histograms()
        for c, r in zip(rows, res):
            want = stated_record(c)
            if r.tobytes() != want.tobytes():
                bad.append(("oracle", c.tag, want, r))
        tot, matrix, ovl, dist, flags = stated_totals(group)
        got = dict(corrected=cnt[capi.C_BASE_CORRECTED], read_corrected=cnt[capi.C_READ_CORRECTED], skipped=cnt[capi.C_BASE_SKIPPED_CORRECTION],
                   masked=cnt[capi.C_BASE_ZERO_QUAL_MASKED], overlapped=cnt[capi.C_OVERLAPPED], adapter_base=cnt[capi.C_TRIMMED_ADAPTER_BASE],
                   adapter_read=cnt[capi.C_TRIMMED_ADAPTER_READ])
        assert got == dict(tot, skipped=2 * tot["skipped"], masked=2 * tot["masked"]), cfg
        assert cnt[capi.C_ERR_MATRIX0:capi.C_ERR_MATRIX0 + 16].tolist() == matrix.tolist(), cfg
        assert cnt[capi.C_FLAG0:capi.C_FLAG0 + capi.N_FLAGS].tolist()[1:] == flags.tolist()[1:] and cnt[capi.C_GOOD_READS] == flags[capi.GOOD], cfg
        assert cnt[capi.C_OVERLAP_LEN_SUM] == sum(c.triple[1] for c in rows if c.counts["overlapped"]), cfg
        assert cnt[capi.C_OVERLAP_BASE_ERR] == sum(c.triple[2] for c in rows if c.counts["overlapped"]), cfg
        assert ovl_hist.tolist() == ovl.tolist() and dist_hist.tolist() == dist.tolist(), cfg
        # upstream dies at a trusted lower-case mismatch, at its error matrix: so does the oracle, at that record
        for c in group:
            if c.raises:
                eng.upload(0, vwc.pack([rows[0], c], True))
                with pytest.raises(capi.AqcError) as e:
                    eng.run(0)
                assert e.value.code == capi.ERR_ALPHABET
        eng.close()
    assert not bad, (len(bad), bad[:6])


def handed_on(c):
    """the reason the lane-per-read kernel's own rules hand a pair to the general kernel, or None (aqc_fast.hpp: a byte outside
    A C G T N; an empty mate; a mate under 16 bases against a diagonal; overlap_len != len2 + offset after a cut)"""
    if not set(c.seq1 + c.seq2) <= set("ACGTN"):
        return "lower case"
    s1, s2 = starts(c)
    gate = c.cfg["trim_front"] > 0 or c.cfg["trim_tail"] > 0
    l1 = vwc.view_len(len(c.seq1), c.cfg["trim_front"], c.cfg["trim_tail"]) if gate else len(c.seq1)
    l2 = vwc.view_len(len(c.seq2), c.cfg["trim_front2"], c.cfg["trim_tail2"]) if gate else len(c.seq2)
    if not l1 or not l2:
        return "empty mate"
    if (l1 > 30 and l2 < 16) or (l2 > 30 and l1 < 16):
        return "short16"
    off, ovl, _ = oracle.overlap(c.seq1[s1:s1 + l1], c.seq2[s2:s2 + l2])
    if off < 0 and ovl > 30 and ovl != l2 + off:
        return "second scan"
    return None


@pytest.mark.parametrize("lead", [0, vwc.PREFIX])
@pytest.mark.parametrize("NW", TIERS)
def test_coverage(NW, lead):
    table = vwc.cases(NW, lead)
    tags = [parts(c.tag) for c in table]
    assert set(t[0] for t in tags) == set(["qual", "matrix", "count", "col", "gate", "cut", "shift", "view", "general"])

    def has(**kw):
        """a row whose tag has these fields: the position class and the kind as one of their "+"-joined parts"""
        def field(t, k):
            return dict(family=[t[0]], config=[t[1].split(",")[0]], geometry=[t[3]], cls=t[4].split("@")[0].split("+") + [t[4]], kind=t[5].split("+"))[k]
        return any(all(v in field(t, k) for k, v in kw.items()) for t in tags)
    # qual/: the whole grid, both ways round, and the four pairs that trust nobody, under all four configs
    grid = [(a, b) for a in vwc.GRID_HI for b in vwc.GRID_LO]
    for config in vwc.CONFIGS:
        for qa, qb in grid + [(b, a) for a, b in grid] + list(vwc.GRID_NEITHER):
            assert has(family="qual", config=config, cls="q%d,%d" % (qa, qb)), (config, qa, qb)
        kinds = set(t[5] for t in tags if t[0] == "qual" and t[1] == config)
        assert kinds == set({"fix": ["fixr1", "fixr2", "skip"], "fix+mask": ["fixr1", "fixr2", "mask"], "nocorr": ["skip"], "nocorr+mask": ["mask"]}[config])
    # matrix/: all 12 cells in both directions; N from either side
    cells = set((cell, p[5]) for c, p in zip(table, tags) if p[0] == "matrix" and p[1] == "fix" for cell in c.matrix)
    assert cells == set(((w, r), k) for w in "ACGT" for r in "ACGT" if w != r for k in ("fixr2", "fixr1"))
    n_rows = [c for c, p in zip(table, tags) if p[0] == "matrix" and "N" in p[4].split("-")[0]]
    assert not any(c.matrix for c in n_rows)
    assert set((chr(c.edits[0][1] + 48), c.edits[0][2] == "N") for c in n_rows if c.edits and c.edits[0][1] != vwc.EDIT_MASK) == \
        set([("1", True), ("1", False), ("2", True), ("2", False)])
    assert has(family="matrix", cls="NN-none", kind="none")
    # count/: distance 0 .. 3, one word and three words, every order of the edit slots
    for config in vwc.CONFIGS:
        for cls in ("d0", "d1", "d2", "d3-oneword", "d3-threewords"):
            assert has(family="count", config=config, cls=cls), (config, cls)
    for config in ("fix", "fix+mask", "nocorr+mask"):
        orders = set(tuple(t[4].split("-")[1:]) for t in tags if t[0] == "count" and t[1] == config and t[4].startswith("d3-") and "word" not in t[4])
        assert orders >= set([("r2", "r1", "x"), ("r2", "x", "r1"), ("r1", "r2", "x"), ("r1", "x", "r2"), ("x", "r2", "r1"), ("x", "r1", "r2")])
    assert set(c.n_edits for c, p in zip(table, tags) if p[0] == "count") == set([0, 1, 2, 3])
    # col/ cut/ view/: one mismatch at every position class, trusted from either side; every geometry
    classes = ["first", "last", "w16r1f", "w16r1b", "w16r2f", "w16r2b", "c49", "c50", "c51"]
    for family, more in (("col", ["c63", "c64", "c127", "c128", "tierlast"]), ("cut", ["c63", "c64", "c127", "c128", "tierlast"]), ("view", [])):
        for cls in classes + more:
            for kind in ("fixr2", "fixr1"):
                assert has(family=family, cls=cls, kind=kind), (family, cls, kind)
    for geometry in ("fwd16", "fwd1", "fwd15", "fwd17", "off0"):
        assert has(family="col", geometry=geometry), geometry
    for a in (1, 16, 17):
        assert has(family="cut", geometry="rev%d" % a) and has(family="cut", geometry="rev%d-2nd" % a), a
    for view in vwc.VIEWS:
        for geometry in ("fwd15", "fwd1", "rev17", "shift16"):
            assert any(t[0] == "view" and t[1].endswith("," + view) and t[3] == geometry for t in tags), (view, geometry)
    lens = set(int(x) + lead for t in tags if t[0] in ("col", "cut") for x in t[2][1:].split("-"))
    assert set(raw for raw in (16 * NW, 16 * NW - 1, vwc.TIER_FLOOR[NW] + 1) if raw > 1) <= lens      # (tier 10's floor is 0: no pair of 1 base)
    # gate/
    for cls in ["n%d-third-c%d" % (n, c) for n in (51, 52, 53) for c in (49, 50, 51) if c < n] + ["d4", "d40", "prefix-AG-CT", "prefix-GA-TC", "prefix-TC-AG"] + \
            ["ovl%d-d%d" % (n, k) for n in (30, 31, 32) for k in (0, 2)]:
        assert has(family="gate", cls=cls), cls
    gate = dict((p[4], c) for c, p in zip(table, tags) if p[0] == "gate" and p[1] == "fix")
    assert [gate["n%d-third-c%d" % k].triple[2] for k in ((51, 49), (51, 50), (52, 49), (52, 50), (52, 51), (53, 49), (53, 50), (53, 51))] == [0, 0, 0, 3, 3, 0, 3, 3]
    assert (gate["d4"].flag, gate["d4"].triple[2], gate["d40"].flag, gate["d40"].triple[2]) == (vwc.BADDIFF, 4, vwc.BADDIFF, 40)
    assert gate["ovl30-d2"].triple[1:] == (30, 2) and not gate["ovl30-d2"].counts["overlapped"] and not gate["ovl30-d2"].n_edits
    assert gate["prefix-AG-CT"].triple[2] == 2
    # cut/: the length rule on both sides, no cut at 30 columns, adapter counters
    assert has(family="cut", cls="req-at", kind="fixr2") and has(family="cut", cls="req-above", kind="badlen") and has(family="cut", cls="ovl30-nocut")
    for c, p in zip(table, tags):
        if p[0] == "cut" and p[3].startswith("rev") and "nocut" not in p[4]:
            assert c.counts["adapter_read"] == 1 and c.counts["adapter_base"] == 2 * int(p[3][3:].split("-")[0]), c.tag
        if p[5] == "badlen":
            assert c.triple == (0, 0, 0) and c.hists[0] > 30 and c.hists[1] is None, c.tag
        if "nocut" in p[4]:
            assert c.triple[0] < 0 and c.triple[1] == 30 and not c.counts["adapter_read"], c.tag
    # shift/: more, exactly as many, fewer, none
    for cls in ("more", "exact", "fewer", "zero", "d0"):
        assert has(family="shift", cls=cls), cls
    for c, p in zip(table, tags):
        if p[0] == "shift" and p[4] in ("fewer", "zero"):
            assert c.flag == vwc.BADMISMATCH and not c.matrix and not (c.counts["corrected"] or c.counts["masked"] or c.counts["skipped"]), c.tag
    assert any(c.flag == vwc.BADMISMATCH and c.n_edits for c in table) and any(c.flag == vwc.BADMISMATCH and not c.n_edits for c in table)
    # general/ and who is handed on
    assert set(c.may_defer for c in table if c.may_defer) == set(["second scan", "short16", "lower case"])
    for c in table:
        assert handed_on(c) == c.may_defer, (c.tag, handed_on(c))
    assert sum(1 for c in table if c.raises) == 2 and has(family="general", cls="lower-untrusted", kind="skip")
    assert has(family="general", geometry="short16") and has(family="general", geometry="short15")
    n_tier = len(vwc.by_config(table))
    print("cases: %d + %d tier records in %d configs, %d of them rows upstream dies at" % (len(table), n_tier, n_tier, sum(1 for c in table if c.raises)))


@pytest.mark.parametrize("NW", TIERS)
def test_barcoded_rows_keep_their_values(NW):
    """the barcode instance's records: the table made for 17 bases less, a barcode + CAGTA in front of every mate.  The oracle's results
    are the stated ones behind the prefix, no mate loses a base to cleanBarcodeTail, and the longest raw read is the tier's"""
    table = [c for c in vwc.with_tier(vwc.cases(NW, vwc.PREFIX), NW, vwc.PREFIX) if not c.raises]
    coded, flags = vwc.with_barcodes(table)
    assert flags == [c.flag for c in table]
    assert max(max(len(c.seq1), len(c.seq2)) for c in coded) == 16 * NW
    bad = []
    for cfg, group in vwc.by_config(coded):
        eng = oracle.OracleEngine()
        eng.set_config(vwc.make_config(cfg, True, barcode=1))
        eng.reset_stats()
        eng.upload(0, vwc.pack(group, True))
        eng.run(0)
        for c, r in zip(group, eng.fetch_results(0)):
            want = stated_record(c)
            want["start1"] += vwc.PREFIX
            want["start2"] += vwc.PREFIX
            want["barcode"] = r["barcode"]
            if r.tobytes() != want.tobytes():
                bad.append((c.tag, want, r))
        eng.close()
    assert not bad, (len(bad), bad[:6])
