"""CPU: the oracle's statRead and record framing against the reference's own answers at byte edges (tests/golden/qc_edges.json.gz,
made by tests/golden/make_qc_edges.py): quality bytes below '!' and above '~' inside a line, NUL runs in the sequence, IUPAC /
lowercase / high bytes, reads of 5, k and k + 1 bases, for every k in 1..8; and lines that end in each byte 0x00-0x20."""
import numpy as np
import pytest

from afterqc_amd import capi, synth
from oracle import oracle

import qc_compare


@pytest.fixture(scope="module")
def edges():
    return qc_compare.load_edges()


@pytest.mark.parametrize("k", range(1, 9))
def test_oracle_stat_read_vs_reference(edges, k):
    st = edges["stat"][str(k)]
    qc = oracle.OracleQC(k)
    for s, q in edges["reads"]:
        qc.statRead(s, q)
    qc_compare.assert_acc_equal(qc.acc(), qc_compare.fixture_acc(st, len(edges["reads"])), "oracle k=%d" % k)
    got = [(km.decode("latin-1"), c) for km, c in qc.kmers()]
    qc_compare.assert_kmers_equal(got, [tuple(x) for x in st["kmers"]], k, "oracle")


def test_fixture_covers_the_edges(edges):
    """the cases the fixture exists for are really in it"""
    quals = "".join(q[:-1] for _, q in edges["reads"])
    assert {chr(b) for b in range(0x21) if b != 0x0a} <= set(quals)
    assert {chr(b) for b in range(0x7f, 0x100)} <= set(quals)
    assert all(q[-1] > " " and s[-1] > " " for s, q in edges["reads"])
    for k in range(1, 9):
        kms = dict(map(tuple, edges["stat"][str(k)]["kmers"]))
        assert kms.get("\x00" * k, 0) > 0                            # the all-NUL k-mer, whose device key is 0


def test_oracle_framing_vs_reference_reader(edges):
    """fastq.Reader.nextRead on lines ending in each byte 0x00-0x20.  The framing (oracle and device) strips what python 2's
    str.rstrip strips — space \\t \\n \\v \\f \\r — which is what the reference's Reader does over a byte stream.  Under the python 3
    shim (text mode) str.rstrip also strips 0x1c-0x1f: that, and nothing else, separates the two captures."""
    for case in edges["reader"]:
        b = case["byte"]
        c = bytes([b])
        text = b"@r1\nACGTACGTAC" + c + b"\n+\nIIIIIIIIII" + c + b"\n@r2\nGATTACA\n+\nFFFFFFF\n"
        records, avail, eof, _ = oracle.frame_text(np.frombuffer(text, dtype=np.uint8), True)
        got = [[ln for _, ln in rec] for rec in records[:avail]]
        assert got == case["binary"], (b, got, case["binary"])
        if 0x1c <= b <= 0x1f:
            assert case["text"] != case["binary"] and case["text"][0][1] == 10
        else:
            assert case["text"] == case["binary"], b


def test_batched_oracle_qc_equals_per_read_loop():
    """OracleEngine.qc_stat's C range loop (orc_qc_stat_range) == statRead read by read, pre and post, in pieces"""
    d = synth.make_pairs(1500, 150, seed=8181, dirty=True)
    batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
    cfg = capi.Config()
    cfg.paired = 1
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.qc_kmer = 6
    eng = oracle.OracleEngine()
    eng.set_config(cfg)
    eng.reset_stats()
    eng.upload(0, batch)
    eng.run(0)
    res = eng.fetch_results(0)
    assert (res["n_edits"] > 0).sum() > 10 and (res["flag"] == capi.GOOD).sum() > 500
    for first, count in ((0, 700), (700, 800), (100, 50)):        # (the last one goes back: a new epoch)
        for w, mate, post in ((0, 0, 0), (1, 1, 0), (2, 0, 1), (3, 1, 1)):
            eng.qc_stat(0, w, mate, first, count, post)
    refqc = [oracle.OracleQC(6) for _ in range(4)]
    epoch = 0
    for first, count in ((0, 700), (700, 800), (100, 50)):
        if first == 100:
            epoch = 1
        for w, mate, post in ((0, 0, 0), (1, 1, 0), (2, 0, 1), (3, 1, 1)):
            for i in range(first, first + count):
                seq, qual = batch.read2(i) if mate else batch.read1(i)
                if post:
                    if res[i]["flag"] != capi.GOOD:
                        continue
                    seq, qual = oracle.final_read(seq, qual, res[i], 2 if mate else 1)
                refqc[w].statRead(seq, qual, (epoch << 44) | (i << 10))
    for w in range(4):
        qc_compare.assert_acc_equal(eng.qc(w), refqc[w].acc(), "which=%d" % w)
        got = qc_compare.kmer_list(eng.kmers(w), 6)
        exp = [(km.decode("latin-1"), c) for km, c in refqc[w].kmers()]
        assert got == exp
