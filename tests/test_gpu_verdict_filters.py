"""GPU (-m gpu): the verdict kernel's per-read filters (csrc/aqc_fast.hpp, phase 2) on constructed records that sit exactly on every
threshold — the polyX screens and their exact check, both low-quality paths, the N count, trim / BADTRIM / length and the order of
the flags — on every tier (10, 16, 18 and 20 words, and the general kernel), paired and single-end, on the plain, the CUT and the
barcode instances.  tests/verdict_filter_cases.py builds the records and states each one's flag;
test_verdict_filter_cases_cpu.py proves those flags against oracle/pyloop.py and the C oracle.

Per config one upload + run against the oracle (results, counters and both histograms bit for bit), then: which kernel decided; every
flag is the constructed one; the lane-per-read kernel handed on nothing but the rows made for the general kernel (a deferred pair
would be decided there and hide the very bug this file is for); and, for pairs, --no_overlap changes no flag.

The CUT instance runs with a quality cut that cuts nothing (mode tail, one window per read, mean quality 0): its results are the plain
ones, byte for byte — but for the rows that rest on upstream's closed gate.  With a view pass on, the trim stage is open for both mates
whatever read 1's trims are, and a mate under 5 bases is BADTRIM (aqc_record.hpp, the project's own rule for its view passes: upstream
has none).  Read 2's trims without read 1's and untrimmed mates of fewer than 5 bases have no plain result to equal there: those rows
run in a batch of their own per config and must show the project's rule — both views trimmed, BADTRIM1 / BADTRIM2 below 5 bases."""
import numpy as np
import pytest

import verdict_filter_cases as vfc
from afterqc_amd import capi
from test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu

PLAIN = set("ACGTN")


def gate_open(cfg):
    return cfg["trim_front"] > 0 or cfg["trim_tail"] > 0


def in_cut_instance(c):
    """the cut that cuts nothing leaves this row's plain result as it is"""
    paired = c.seq2 is not None
    if gate_open(c.cfg):
        return True
    if paired and (c.cfg["trim_front2"] > 0 or c.cfg["trim_tail2"] > 0):
        return False
    return min(len(c.seq1), len(c.seq2) if paired else len(c.seq1)) >= 5


def check_open_gate_rows(eng, cfg, rows, tier, paired, NW):
    """the CUT instance's own rule on the rows in_cut_instance leaves out (plus the config's tier record, for the batch's max_len):
    the trim stage runs for both mates, a view under 5 bases is BADTRIM1 / BADTRIM2, under BADTRIM1 read 2 is the read as it came;
    every row here is background that no other filter of its config flags once both views have 5 bases"""
    rows = rows + ([tier] if tier not in rows else [])
    eng.set_config(vfc.make_config(cfg, paired))
    eng.reset_stats()
    eng.upload(0, vfc.pack(rows, paired))
    eng.run(0)
    assert eng.last_verdict_words(0) == NW
    res = eng.fetch_results(0)
    for c, r in zip(rows, res):
        v1 = vfc.view_len(len(c.seq1), cfg["trim_front"], cfg["trim_tail"])
        v2 = vfc.view_len(len(c.seq2), cfg["trim_front2"], cfg["trim_tail2"]) if paired else 5
        want = vfc.BADTRIM1 if v1 < 5 else vfc.BADTRIM2 if v2 < 5 else c.flag
        assert want != vfc.GOOD or c.flag == vfc.GOOD, c.tag
        assert int(r["flag"]) == want, (c.tag, cfg, want, int(r["flag"]))
        # (where a view begins matters only while it holds a base.  The cut's one window is the whole read 1: a 1-base read whose quality
        #  is chr(32), phred -1, is the one row whose window sum is below 0 — the cut takes that base, the flag stays BADTRIM1)
        if sum(ord(q) - 33 for q in c.qual1) < 0:
            assert len(c.seq1) == 1 and want == vfc.BADTRIM1 and int(r["len1"]) == 0, c.tag
        else:
            assert int(r["len1"]) == v1 and (v1 == 0 or int(r["start1"]) == cfg["trim_front"]), c.tag
        if paired and want == vfc.BADTRIM1:
            assert (int(r["start2"]), int(r["len2"])) == (0, len(c.seq2)), c.tag
        elif paired:
            assert int(r["len2"]) == v2 and (v2 == 0 or int(r["start2"]) == cfg["trim_front2"]), c.tag
    if NW:
        _, deferred = eng.last_deferred(0, want_indices=True)
        assert not [rows[i].tag for i in deferred if not rows[i].may_defer], cfg
    return len(rows)


@pytest.mark.parametrize("instance", ["plain", "cut", "barcode"])
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("NW", [10, 16, 18, 20, 0])
def test_filters_at_every_threshold(gpu_engine, NW, paired, instance):
    lead = vfc.PREFIX if instance == "barcode" else 0
    table = vfc.with_tier(vfc.cases(NW or 20, paired, lead), NW, lead)
    open_gate = [c for c in table if instance == "cut" and not in_cut_instance(c)]
    table = [c for c in table if c not in open_gate]
    flags = [c.flag for c in table]
    if instance == "barcode":
        table, flags = vfc.with_barcodes(table)
    flag_of = dict((id(c), f) for c, f in zip(table, flags))
    n_records = n_runs = 0
    gpu_engine.set_quality_cut(capi.CutConfig(0, 1, 0, capi.AQC_MAX_READ_LEN, 0) if instance == "cut" else None)
    try:
        for cfg, group in vfc.by_config(table):
            want = np.array([flag_of[id(c)] for c in group])
            tags = [c.tag for c in group]
            batch = vfc.pack(group, paired)
            assert batch.max_len() == (16 * NW if NW else 321)
            g, o = run_both(gpu_engine, vfc.make_config(cfg, paired, barcode=1 if lead else 0), batch, qc=False)
            words = gpu_engine.last_verdict_words(0)
            n_def, deferred = gpu_engine.last_deferred(0, want_indices=True) if words else (0, np.zeros(0, dtype=np.uint32))
            assert_same(g, o)
            # thr = 128 is outside the byte compare of the lane-per-read kernel: the general kernel runs the whole batch
            assert words == (0 if cfg["qualified_quality_phred"] + 33 > 127 else NW), (cfg, words)
            got = g["res"]["flag"]
            wrong = np.flatnonzero(got != want)
            assert not len(wrong), [(tags[i], cfg, int(want[i]), int(got[i])) for i in wrong[:8]]
            # under BADTRIM1 read 2 is the read as it came (behind its barcode): neither trimmed nor cut
            for i in np.flatnonzero(want == vfc.BADTRIM1):
                if paired:
                    assert (int(g["res"]["start2"][i]), int(g["res"]["len2"][i])) == (lead, len(group[i].seq2) - lead), tags[i]
            if words:
                assert n_def == len(deferred)
                unexpected = [tags[i] for i in deferred if not group[i].may_defer]
                assert not unexpected, (cfg, unexpected[:8])
                # (the rows that MUST be handed on are those whose uploaded mates really hold an exotic byte or are empty: in the
                #  barcode instance an "empty mate" is its 17-base prefix, BADBCD1 / BADBCD2 on the lane-per-read kernel itself)
                must = [i for i, c in enumerate(group) if c.may_defer in ("exotic byte", "empty mate") and (
                    not c.seq1 or (paired and not c.seq2) or not set(c.seq1 + (c.seq2 or "")) <= PLAIN)]
                missing = [tags[i] for i in must if i not in set(deferred.tolist())]
                assert not missing, (cfg, missing)
            if paired:
                gpu_engine.set_config(vfc.make_config(cfg, paired, barcode=1 if lead else 0, no_overlap=1))
                gpu_engine.reset_stats()
                gpu_engine.upload(0, batch)
                gpu_engine.run(0)
                assert gpu_engine.last_verdict_words(0) == words
                again = gpu_engine.fetch_results(0)["flag"]
                wrong = np.flatnonzero(again != want)
                assert not len(wrong), [("no_overlap", tags[i], cfg, int(want[i]), int(again[i])) for i in wrong[:8]]
            n_records += len(group)
            n_runs += 1
        tiers = dict((vfc.cfg_key(c.cfg), c) for c in vfc.with_tier(vfc.cases(NW or 20, paired, lead), NW, lead) if c.tag.startswith("tier/"))
        for cfg, rows in vfc.by_config(open_gate):
            n_records += check_open_gate_rows(gpu_engine, cfg, rows, tiers[vfc.cfg_key(cfg)], paired, NW)
        assert (instance == "cut") == bool(open_gate)
    finally:
        gpu_engine.set_quality_cut(None)
    print("%d records in %d configs" % (n_records, n_runs))
    assert n_runs >= 60 and n_records >= 1000
