"""GPU (-m gpu): the verdict kernel's pair phase (csrc/aqc_fast.hpp from "overlap (util.py:158-212)" to the result store; the general
kernel's restatement in csrc/aqc_record.hpp) on constructed pairs that sit on every threshold of the diagonal scan, the accept rule,
the adapter cut, the shifted diagonal and the three-step correction walk — on every tier (10, 16, 18 and 20 words, and the general
kernel), on the plain, the CUT and the barcode instances.  tests/verdict_walk_cases.py builds the pairs and states each one's flag,
triple, edits, counters and matrix cells; test_verdict_walk_cases_cpu.py proves those against the real reference's outputs
(tests/golden/walk_cases.json.gz), oracle/pyloop.py and the C oracle.

Per config one upload + run against the oracle (result records byte for byte — all 32 bytes, edits included — counters, matrix and both
histograms), then: which kernel decided; every record is the stated one; the final reads rebuilt from the kernel's record are the
reference's; the lane-per-read kernel handed on nothing but the rows its own rules hand on (a deferred pair would be decided by the
general kernel and hide the very bug this file is for) and every one of those.  The CUT instance runs with a quality cut that cuts
nothing: its results are the plain instance's bytes.  Tier 10's table also goes through the zero-copy text arena.  The trusted
lower-case rows run alone: upstream dies at its error matrix, the engine raises at that record."""
import numpy as np
import pytest

import verdict_walk_cases as vwc
from afterqc_amd import capi, fastq
from oracle import oracle
from test_gpu_parity import assert_same, run_both
from test_verdict_walk_cases_cpu import fixture, reference_reads, stated_record

pytestmark = pytest.mark.gpu

MUST_DEFER = ("short16", "second scan", "lower case")
NO_CUT = (0, 1, 0, capi.AQC_MAX_READ_LEN, 0)           # mode tail, one window per read, mean quality 0: cuts nothing


def write_fastq(path, seqs, quals, mate):
    with open(path, "wb") as f:
        for i, (s, q) in enumerate(zip(seqs, quals)):
            f.write(b"@WALK:1:FC:1:1101:%d:2000 %d:N:0:ACGT\n" % (1000 + i, mate) + s.encode("latin-1") + b"\n+\n" + q.encode("latin-1") + b"\n")


def run_alone(eng, cfg, batch):
    eng.set_config(cfg)
    eng.reset_stats()
    eng.upload(0, batch)
    eng.run(0)
    return eng.fetch_results(0)


@pytest.mark.parametrize("instance", ["plain", "cut", "barcode"])
@pytest.mark.parametrize("NW", [10, 16, 18, 20, 0])
def test_walk_at_every_threshold(gpu_engine, NW, instance, tmp_path):
    lead = vwc.PREFIX if instance == "barcode" else 0
    whole = vwc.with_tier(vwc.cases(NW or 20, lead), NW, lead)
    fx = fixture(NW or 20, lead)
    n_records = n_runs = n_reads = n_deferred = 0
    try:
        for k, (cfg, stated) in enumerate(vwc.by_config(whole)):
            ref = fx["configs"][k]
            assert ref["cfg"] == cfg
            ref_rows = dict(zip(ref["index"], ref["rows"]))
            keep = [i for i, c in enumerate(stated) if not c.raises]
            stated = [stated[i] for i in keep]
            group = vwc.with_barcodes(stated)[0] if lead else stated
            tags = [c.tag for c in stated]
            config = vwc.make_config(cfg, True, barcode=1 if lead else 0)
            batch = vwc.pack(group, True)
            assert batch.max_len() == (16 * NW if NW else 321)
            plain = None
            if instance == "cut":
                gpu_engine.set_quality_cut(None)
                plain = run_alone(gpu_engine, config, batch)
                gpu_engine.set_quality_cut(capi.CutConfig(*NO_CUT))
            g, o = run_both(gpu_engine, config, batch, qc=False)
            words = gpu_engine.last_verdict_words(0)
            n_def, deferred = gpu_engine.last_deferred(0, want_indices=True) if words else (0, np.zeros(0, dtype=np.uint32))
            assert_same(g, o)
            assert words == NW, (cfg, words)
            res = g["res"]
            wrong = []
            for i, (c, raw, r) in enumerate(zip(stated, group, res)):
                want = stated_record(c)
                want["start1"] += lead
                want["start2"] += lead
                want["barcode"] = r["barcode"]
                if r.tobytes() != want.tobytes():
                    wrong.append((c.tag, want, r))
                    continue
                if keep[i] in ref_rows and not (NW == 0 and c.tag.startswith("tier/")):
                    got = oracle.final_read(raw.seq1.encode("latin-1"), raw.qual1.encode("latin-1"), r, 1) + \
                        oracle.final_read(raw.seq2.encode("latin-1"), raw.qual2.encode("latin-1"), r, 2)
                    if list(got) != reference_reads(c, ref_rows[keep[i]]):
                        wrong.append((c.tag, "final reads", r))
                    n_reads += 1
            assert not wrong, (cfg, len(wrong), wrong[:4])
            if words:
                assert n_def == len(deferred)
                handed = set(deferred.tolist())
                unexpected = [tags[i] for i in sorted(handed) if not stated[i].may_defer]
                assert not unexpected, (cfg, unexpected[:8])
                missing = [tags[i] for i, c in enumerate(stated) if c.may_defer in MUST_DEFER and i not in handed]
                assert not missing, (cfg, missing)
                n_deferred += n_def
            if plain is not None:
                assert res.tobytes() == plain.tobytes(), cfg
            if NW == 10 and instance == "plain":
                # the same records as FASTQ text, addressed in place
                p1, p2 = str(tmp_path / ("w%d_R1.fq" % k)), str(tmp_path / ("w%d_R2.fq" % k))
                write_fastq(p1, [c.seq1 for c in group], [c.qual1 for c in group], 1)
                write_fastq(p2, [c.seq2 for c in group], [c.qual2 for c in group], 2)
                arena = capi.Batch.from_raw(fastq.Reader(p1).next_batch(10000), fastq.Reader(p2).next_batch(10000))
                assert arena.n == batch.n
                assert run_alone(gpu_engine, config, arena).tobytes() == res.tobytes(), cfg
            n_records += len(group)
            n_runs += 1
        # upstream dies at a trusted lower-case mismatch; the engine raises at that record, whichever kernel meets it
        n_raise = 0
        for cfg, stated in vwc.by_config(whole):
            for c in stated:
                if c.raises:
                    first = [x for x in stated if not x.raises][0]
                    rows = [first, c, first]
                    rows = vwc.with_barcodes(rows)[0] if lead else rows
                    gpu_engine.set_config(vwc.make_config(cfg, True, barcode=1 if lead else 0))
                    gpu_engine.reset_stats()
                    gpu_engine.upload(0, vwc.pack(rows, True))
                    with pytest.raises(capi.AqcError) as e:
                        gpu_engine.run(0)
                        gpu_engine.fetch_results(0)
                    assert e.value.code == capi.ERR_ALPHABET, e.value
                    assert gpu_engine.error_record(0) == 1
                    n_raise += 1
        assert n_raise == 2
    finally:
        gpu_engine.set_quality_cut(None)
        gpu_engine.reset_stats()
    print("%d records in %d configs, %d final reads checked against the reference, %d handed on" % (n_records, n_runs, n_reads, n_deferred))
    # (the smallest table, tier 10's plain one: 1253 rows + 18 tier records - 2 rows upstream dies at, in 18 configs; test_verdict_walk_cases_cpu
    #  prints it)
    assert n_runs >= 18 and n_records >= 1269 and n_reads >= 1269 - 18
