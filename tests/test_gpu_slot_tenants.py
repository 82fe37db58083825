"""One slot, five tenants in a row (-m gpu).  A slot keeps its buffers, tables and counts per input file from call to call, so
what one tenant leaves behind must never reach the next: a paired text with a record whose read-2 quality line is short, a packed
paired batch, a single-end text, a packed single-end batch, and the first text again.  Every tenant's verdict records and, where it
is formatted, every stream's bytes are the oracle's; the last tenant's streams are also those of the first, and those of the same
text on a slot that has held nothing else.

The C oracle frames regular records only, so the paired text goes to it in two parts around its one irregular record; that record's
verdict and text are oracle/pyloop.py's (the reference's own slicing of each string by its own length, tests/test_irregular_oracle.py)."""
import numpy as np
import pytest

from afterqc_amd import capi, synth

pytestmark = pytest.mark.gpu

N_TEXT, L_TEXT, IRR = 130, 40, 100      # two format tiles, five verdict batches of 32 (the last one partial); the irregular record
N_SMALL = 33


def make_cfg(paired):
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 20, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    return cfg


def short_pairs(n, L, seed):
    """pairs of L-base reads (synth.make_pairs starts at 61 bases) that overlap by 25 .. L bases, with the artefacts the filters look for"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    d = dict((k, np.zeros((n, L), dtype=np.uint8)) for k in ("seq1", "qual1", "seq2", "qual2"))
    for i in range(n):
        ov = int(rng.integers(34 if i % 10 in (8, 9) else 25, L + 1))      # (read 2 meets read 1 in its last ov bases)
        frag = rng.integers(0, 4, 2 * L - ov)
        c1, c2 = frag[:L].copy(), (3 - frag[::-1])[:L].copy()            # (3 - code: A <-> T, C <-> G)
        q1, q2 = rng.integers(63, 75, L).astype(np.uint8), rng.integers(63, 75, L).astype(np.uint8)
        if i % 10 in (8, 9):                                              # mismatches in the overlap: two to correct, five that hide it
            at = rng.choice(np.arange(L - 16, L - 1), 2 if i % 10 == 8 else 5, replace=False)
            c2[at] = (c2[at] + 1) & 3
            q2[at] = ord("#")
        d["seq1"][i], d["seq2"][i], d["qual1"][i], d["qual2"][i] = bases[c1], bases[c2], q1, q2
        if i % 10 == 3:
            d["seq1"][i, 5:12] = ord("N")
        if i % 10 == 6:
            d["qual1"][i, 4:30] = ord("#")
    d["len1"] = d["len2"] = np.full(n, L, dtype=np.uint32)
    return d


def records(d, mate):
    """[name, sequence, plus, quality] per record, as text"""
    out = []
    for i in range(len(d["len" + mate])):
        l = int(d["len" + mate][i])
        name = "@SIM:1:FC1:%d:%d:%d:%d %s:N:0:ACGT" % (1 + i % 3, 1101 + i % 7, 1000 + 7 * i, 2000 + 3 * i, mate)
        out.append([name, d["seq" + mate][i, :l].tobytes().decode("latin-1"), "+" if i % 5 else "+" + name[1:],
                    d["qual" + mate][i, :l].tobytes().decode("latin-1")])
    return out


def text_of(recs):
    return "".join("\n".join(r) + "\n" for r in recs).encode("latin-1")


def pad(data):
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def run_text(eng, slot, cfg, t1, t2, store):
    """aqc_frame -> aqc_run -> aqc_format of one whole text on `slot` -> (verdict records, the six streams)"""
    eng.set_config(cfg)
    if t2 is None:
        info = eng.frame(slot, pad(t1), len(t1), True)
    else:
        info = eng.frame(slot, pad(t1), len(t1), True, pad(t2), len(t2), True)
    n = int(info.n)
    eng.run(slot)
    res = eng.fetch_results(slot)[:n].copy()
    streams = []
    for q, nb in enumerate(eng.format(slot, n, store)):
        out = np.zeros(int(nb) + 64, dtype=np.uint8)
        if nb:
            eng.fetch_text(slot, q // 3, q % 3, out, int(nb))
        streams.append(out[:int(nb)].tobytes())
    return res, streams


def run_batch(eng, slot, cfg, batch):
    eng.set_config(cfg)
    eng.upload(slot, batch)
    eng.run(slot)
    return eng.fetch_results(slot)[:batch.n].copy()


@pytest.fixture(scope="module")
def tenants():
    """the inputs of the five tenants and what the oracle makes of each; computed once, read only"""
    from oracle import oracle, pyloop
    d = short_pairs(N_TEXT, L_TEXT, 1301)
    r1, r2 = records(d, "1"), records(d, "2")
    # the irregular record: a clean pair that overlaps over its whole length, read 2's quality line 3 bytes short
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    s1 = "".join("ACGT"[(7 * k + k // 5) % 4] for k in range(L_TEXT))
    r1[IRR][1], r1[IRR][3] = s1, "I" * L_TEXT
    r2[IRR][1], r2[IRR][3] = "".join(comp[b] for b in reversed(s1)), "H" * (L_TEXT - 3)
    cfg2, cfg1 = make_cfg(True), make_cfg(False)
    ora = oracle.OracleEngine()
    ora.set_circles([])
    # (a) / (e): the regular records before and behind the irregular one from the C oracle, the irregular one from pyloop
    res_a, st_a = run_text(ora, 0, cfg2, text_of(r1[:IRR]), text_of(r2[:IRR]), True)
    res_b, st_b = run_text(ora, 0, cfg2, text_of(r1[IRR + 1:]), text_of(r2[IRR + 1:]), True)
    p = pyloop.process_pair(r1[IRR][1], r1[IRR][3], r2[IRR][1], r2[IRR][3], pyloop.options_from_config(cfg2))
    assert p["flag"] == pyloop.GOOD and p["overlap_len"] > 30 and p["distance"] == 0
    irr = [b""] * 6
    for k, (rec, seq, qual) in enumerate(((r1[IRR], p["seq1"], p["qual1"]), (r2[IRR], p["seq2"], p["qual2"]))):
        ov = p["overlap_len"]
        irr[3 * k] = ("%s\n%s\n%s\n%s\n" % (rec[0], seq, rec[2], qual)).encode("latin-1")
        # (getOverlap, preprocesser.py:78-84: the last overlap_len characters of EACH string; a start below zero counts from the end)
        irr[3 * k + 2] = ("%s\n%s\n%s\n%s\n" % (rec[0], seq[len(seq) - ov:], rec[2], qual[len(qual) - ov:])).encode("latin-1")
    text = dict(t1=text_of(r1), t2=text_of(r2), res_before=res_a, res_behind=res_b, irr=p,
                streams=[st_a[q] + irr[q] + st_b[q] for q in range(6)])
    assert all(len(text["streams"][q]) > 0 for q in (0, 1, 2, 3, 4, 5))
    # (b) a packed paired batch, (d) a packed single-end one: longer, ragged reads
    db = synth.make_pairs(n=N_SMALL, L=75, seed=1302, dirty=True, ragged=True)
    pb = capi.Batch.from_matrices(db["seq1"], db["qual1"], db["len1"], db["seq2"], db["qual2"], db["len2"])
    dd = synth.make_pairs(n=N_SMALL, L=100, seed=1304, dirty=True, ragged=True)
    sb = capi.Batch.from_matrices(dd["seq1"], dd["qual1"], dd["len1"])
    # (c) a single-end text of regular records
    dc = synth.make_pairs(n=N_SMALL, L=70, seed=1303, dirty=True)
    tc = text_of(records(dc, "1"))
    res_c, st_c = run_text(ora, 0, cfg1, tc, None, False)
    return dict(cfg2=cfg2, cfg1=cfg1, text=text, pb=pb, res_pb=run_batch(ora, 0, cfg2, pb), sb=sb, res_sb=run_batch(ora, 0, cfg1, sb),
                tc=tc, res_c=res_c, st_c=st_c)


def check_text(got, want, what):
    res, streams = got
    assert len(res) == N_TEXT, what
    assert np.array_equal(res[:IRR].view(np.uint8), want["res_before"].view(np.uint8)), what
    assert np.array_equal(res[IRR + 1:].view(np.uint8), want["res_behind"].view(np.uint8)), what
    r, p = res[IRR], want["irr"]
    assert (int(r["flag"]), int(r["offset"]), int(r["overlap_len"]), int(r["distance"]), int(r["n_edits"])) == \
        (p["flag"], p["offset"], p["overlap_len"], p["distance"], len(p["edits"])), what
    for q in range(6):
        assert streams[q] == want["streams"][q], "%s: stream %d" % (what, q)


def test_a_slot_forgets_its_previous_tenants(tenants, monkeypatch):
    monkeypatch.delenv("AQC_FORCE_GENERIC", raising=False)
    t = tenants
    eng = capi.Engine(0, 2)
    try:
        eng.set_circles([])
        first = run_text(eng, 0, t["cfg2"], t["text"]["t1"], t["text"]["t2"], True)                    # (a)
        check_text(first, t["text"], "(a)")
        res = run_batch(eng, 0, t["cfg2"], t["pb"])                                                   # (b)
        assert np.array_equal(res.view(np.uint8), t["res_pb"].view(np.uint8)), "(b)"
        res, streams = run_text(eng, 0, t["cfg1"], t["tc"], None, False)                              # (c)
        assert len(res) == N_SMALL and np.array_equal(res.view(np.uint8), t["res_c"].view(np.uint8)), "(c)"
        for q in range(6):
            assert streams[q] == t["st_c"][q], "(c): stream %d" % q
        res = run_batch(eng, 0, t["cfg1"], t["sb"])                                                   # (d)
        assert np.array_equal(res.view(np.uint8), t["res_sb"].view(np.uint8)), "(d)"
        again = run_text(eng, 0, t["cfg2"], t["text"]["t1"], t["text"]["t2"], True)                    # (e)
        check_text(again, t["text"], "(e)")
        fresh = run_text(eng, 1, t["cfg2"], t["text"]["t1"], t["text"]["t2"], True)
        for q in range(6):
            assert again[1][q] == first[1][q], "(e) against (a): stream %d" % q
            assert again[1][q] == fresh[1][q], "(e) against a fresh slot: stream %d" % q
    finally:
        eng.close()
