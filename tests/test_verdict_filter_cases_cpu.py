"""The case table of tests/verdict_filter_cases.py, before a kernel sees it: every constructed flag is the flag of oracle/pyloop.py's
process_pair (the Python restatement of upstream's loop) and of the C oracle, for every tier's table, paired and single-end, with
and without the room the barcode instance needs; and the table holds what it says it holds — every polyX config firing and quiet,
the three screen regimes, every position class per mate and family, every low-quality path."""
import numpy as np
import pytest

import verdict_filter_cases as vfc
from afterqc_amd import capi
from oracle import oracle, pyloop

TIERS = (10, 16, 18, 20)


def parts(tag):
    """family, config, length, mate, position class, kind"""
    return tag.split("/")[:6]


def test_flag_values_are_the_abi_s():
    for name in ("GOOD", "BADBCD1", "BADBCD2", "BADTRIM1", "BADTRIM2", "BADLEN", "BADPOL", "BADLQC", "BADNCT"):
        assert getattr(vfc, name) == getattr(capi, name), name
    for name in ("GOOD", "BADTRIM1", "BADTRIM2", "BADLEN", "BADPOL", "BADLQC", "BADNCT"):
        assert getattr(vfc, name) == getattr(pyloop, name), name


@pytest.mark.parametrize("lead", [0, vfc.PREFIX])
@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("NW", TIERS)
def test_constructed_flags_are_the_reference_s(NW, paired, lead):
    """pyloop record by record, the C oracle batch by batch (one per config); the tier records of this tier and — for the widest
    table, which also runs on the general kernel — the 321-base ones"""
    table = vfc.with_tier(vfc.cases(NW, paired, lead), NW, lead)
    if NW == 20:
        table += [c for c in vfc.with_tier(vfc.cases(NW, paired, lead), 0, lead) if c.tag.startswith("tier/")]
    assert all((c.seq2 is not None) == paired for c in table)
    bad = []
    for cfg, group in vfc.by_config(table):
        opt = dict(cfg, no_overlap=0, no_correction=0, mask_mismatch=0)
        for c in group:
            got = pyloop.process_pair(c.seq1, c.qual1, c.seq2, c.qual2, opt)["flag"]
            if got != c.flag:
                bad.append(("pyloop", c.tag, cfg, c.flag, got))
        eng = oracle.OracleEngine()
        eng.set_config(vfc.make_config(cfg, paired))
        eng.reset_stats()
        eng.upload(0, vfc.pack(group, paired))
        eng.run(0)
        flags = eng.fetch_results(0)["flag"]
        eng.close()
        for c, got in zip(group, flags.tolist()):
            if got != c.flag:
                bad.append(("oracle", c.tag, cfg, c.flag, got))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("NW", TIERS)
def test_barcoded_flags_are_the_oracle_s(NW, paired):
    """the barcode instance's records — the table made for 17 bases less, a barcode + CAGTA in front of every mate — keep their
    flags (BADBCD1 / BADBCD2 where a mate is nothing but its prefix), no mate loses a base to cleanBarcodeTail, and the longest
    raw read is the tier's"""
    table = vfc.with_tier(vfc.cases(NW, paired, vfc.PREFIX), NW, vfc.PREFIX)
    coded, flags = vfc.with_barcodes(table)
    assert max(max(len(c.seq1), len(c.seq2 or "")) for c in coded) == 16 * NW
    bad = []
    flag_of = dict((id(c), f) for c, f in zip(coded, flags))
    for cfg, group in vfc.by_config(coded):
        want = [flag_of[id(c)] for c in group]
        eng = oracle.OracleEngine()
        eng.set_config(vfc.make_config(cfg, paired, barcode=1))
        eng.reset_stats()
        eng.upload(0, vfc.pack(group, paired))
        eng.run(0)
        res = eng.fetch_results(0)
        eng.close()
        for c, w, r in zip(group, want, res):
            if int(r["flag"]) != w:
                bad.append((c.tag, cfg, w, int(r["flag"])))
            elif w not in (vfc.BADBCD1, vfc.BADBCD2, vfc.BADTRIM1, vfc.BADTRIM2):
                # what is left of each mate is the case's read through the config's trims: nothing was cut from a tail
                gate = cfg["trim_front"] > 0 or cfg["trim_tail"] > 0
                v1 = vfc.view_len(len(c.seq1) - vfc.PREFIX, cfg["trim_front"], cfg["trim_tail"]) if gate else len(c.seq1) - vfc.PREFIX
                assert int(r["len1"]) == v1, c.tag
                if paired:
                    v2 = vfc.view_len(len(c.seq2) - vfc.PREFIX, cfg["trim_front2"], cfg["trim_tail2"]) if gate else len(c.seq2) - vfc.PREFIX
                    assert int(r["len2"]) == v2, c.tag
    assert not bad, (len(bad), bad[:8])


def test_screen_regimes():
    """run_req and poly_word recomputed by the kernel's formula: each list of configs lies in the regime it is named for"""
    assert [vfc.poly_screen(*c)[0] for c in vfc.POLY_WORD] == ["word"] * len(vfc.POLY_WORD)
    assert [vfc.poly_screen(*c)[0] for c in vfc.POLY_DOUBLING + vfc.POLY_STEP_CAP] == ["doubling"] * (len(vfc.POLY_DOUBLING) + 1)
    assert [vfc.poly_screen(*c)[0] for c in vfc.POLY_ALL] == ["all"] * len(vfc.POLY_ALL)
    # the step cap: covered doubles to 16 and has more than 15 to go
    assert vfc.poly_screen(240, 6)[1] == 34
    assert set(vfc.POLY_CONFIGS) == set([(35, 2), (31, 0), (36, 5), (50, 5), (20, 0), (20, 1), (30, 0), (10, 3), (36, 6), (240, 6), (5, 4), (10, 10),
                                         (3, 7), (35, -1)])


@pytest.mark.parametrize("lead", [0, vfc.PREFIX])
@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("NW", TIERS)
def test_coverage(NW, paired, lead):
    table = vfc.cases(NW, paired, lead)
    tags = [parts(c.tag) for c in table]
    mates = ("r1", "r2") if paired else ("r1",)
    # every polyX config fires and stays quiet on every tier it fits
    regimes = set()
    for mp, mm in vfc.POLY_CONFIGS:
        kinds = set(t[5] for t in tags if t[0] == "polyx" and t[1] == "%d,%d" % (mp, mm))
        if mp > 16 * NW - lead:                          # (240, 6): reads of 240 bases or more only
            assert (mp, mm) == (240, 6) and not kinds
            continue
        regimes.add(vfc.poly_screen(mp, mm)[0])
        assert kinds == (set(["quiet"]) if (mp, mm) in vfc.NEVER_FIRES else set(["fire", "quiet"])), (mp, mm, kinds)
    assert regimes == set(["all", "word", "doubling"])
    if NW >= 18 or (NW == 16 and not lead):
        assert any(t[1] == "240,6" for t in tags)
    # every position class, per mate, per family, on both sides of the threshold
    for fam, fam_mates in (("polyx", mates + (("both",) if paired else ())), ("lq", ("r1",)), ("n", mates)):
        for mate in fam_mates:
            for cls in ("first", "last", "w16", "w32"):
                for kind in ("fire", "quiet"):
                    assert any(t[0] == fam and t[3] == mate and cls in t[4].split("+") and t[5] == kind for t in tags), (fam, mate, cls, kind)
    # every poly base — N among them — in read 1 and in read 2 (its N plane is reversed and moved on by a bit), firing and quiet
    planted = [(c.tag.split("/")[6], c.tag.split("/")[5]) for c in table if c.tag.startswith("polyx/") and len(c.tag.split("/")) > 6]
    for mate in mates:
        for X in "ACGTN":
            for kind in ("fire", "quiet"):
                assert any(k == kind and ("%s:X%s-" % (mate, X)) in what for what, k in planted), (mate, X, kind)
    for end in ("trim-front", "trim-tail"):
        for mate in mates:
            for kind in ("fire", "quiet"):
                assert any(t[0] == "polyx" and t[3] == mate and t[4] == end and t[5] == kind for t in tags), (end, mate, kind)
    # both low-quality paths, the surplus rows and the general kernel's config; every limit and phred
    for path in ("summed", "plane", "surplus", "general"):
        for kind in ("fire", "quiet"):
            assert any(t[0] == "lq" and t[1].endswith(path) and t[5] == kind for t in tags), (path, kind)
    for limit in vfc.LQ_LIMITS:
        for phred in vfc.LQ_PHREDS:
            for path in ("summed", "plane"):
                assert any(t[1] == "%d,q%d,%s" % (limit, phred, path) for t in tags)
    for limit in vfc.N_LIMITS:
        for path in ("whole", "view"):
            assert any(t[1] == "%d,%s" % (limit, path) for t in tags)
    # the order rows, the trim rows, the general kernel's rows
    assert set(c.flag for c in table if c.tag.startswith("order/")) >= set(
        [vfc.BADTRIM1, vfc.BADLEN, vfc.BADPOL, vfc.BADLQC, vfc.BADNCT, vfc.GOOD] + ([vfc.BADTRIM2] if paired else []))
    for name in ("view45", "gate", "r1-front-swallows", "r1-tail-swallows", "r1-both-swallows") + (
            ("r2-front-swallows", "r2-tail-swallows", "r2-both-swallows") if paired else ()):
        assert any(t[0] == "trim" and t[1] == name for t in tags), name
    assert set(c.may_defer for c in table if c.may_defer) == set(["lower case", "exotic byte", "empty mate"])
    assert all(c.tag.startswith("general/") for c in table if c.may_defer)
    # mates of a GOOD-side pair: both views at least 16 bases, or both at most 30 (no diagonal to scan)
    if paired:
        for c in table:
            if c.flag == vfc.GOOD and not c.may_defer:
                gate = c.cfg["trim_front"] > 0 or c.cfg["trim_tail"] > 0
                v1 = vfc.view_len(len(c.seq1), c.cfg["trim_front"], c.cfg["trim_tail"]) if gate else len(c.seq1)
                v2 = vfc.view_len(len(c.seq2), c.cfg["trim_front2"], c.cfg["trim_tail2"]) if gate else len(c.seq2)
                assert min(v1, v2) >= 16 or max(v1, v2) <= 30, c.tag
    print("cases: %d in %d configs" % (len(table), len(vfc.by_config(table))))
