"""GPU (-m gpu): the verdict kernel's 20-word tier, reads of 289 - 320 bases (aqc_capi_run.hip, choose_verdict_kernel).

The reference's answers above 250 bases (tests/golden/long_reads_cases.json.gz, pinned on the CPU by test_long_reads_golden.py)
through aqc_run and through the three end-to-end drivers; every length pair of the tier, a batch larger than the persistent grid
and the barcode / single-end instances against the oracle; and which kernel decided — aqc_last_verdict_words — for each of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import long_cases
from afterqc_amd import capi, synth
from test_gpu_parity import assert_same, default_cfg, run_both
from test_host_golden import check_case
from test_long_reads_golden import golden, run_long_case, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_NAMES = [c[0] for c in long_cases.CASES]


def words_for(max_len):
    return 20 if 288 < max_len <= 320 else 0


def packed(name):
    """a case's reads as a packed batch, and the config the CLI would run them with but for the trims"""
    sp = long_cases.CASE_TABLE[name][2]
    d = long_cases.pairs_of(sp)
    paired = sp["kind"] == "pe"
    if paired:
        batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
    else:
        batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"])
    argv = long_cases.CASE_TABLE[name][1]
    cfg = default_cfg(paired, barcode=1 if sp.get("barcode") else 0, mask_mismatch=1 if "--mask_mismatch" in argv else 0,
                      seq_len_req=20 if "-s" in argv else 35)
    return batch, cfg


# ---- which kernel decided ---------------------------------------------------------------------------------------------------------------
def test_last_verdict_words_call_sequence():
    """AQC_ERR_STATE before the first run and after a new upload; 0 for an empty batch"""
    eng = capi.Engine(0, 2)
    try:
        eng.set_config(default_cfg(True))
        with pytest.raises(capi.AqcError):
            eng.last_verdict_words(0)
        batch, _ = packed("pe_l301")
        eng.upload(0, batch)
        with pytest.raises(capi.AqcError):
            eng.last_verdict_words(0)
        eng.run(0)
        assert eng.last_verdict_words(0) == 20
        with pytest.raises(capi.AqcError):
            eng.last_verdict_words(1)                    # the other slot never ran
        eng.upload(0, batch)
        with pytest.raises(capi.AqcError):
            eng.last_verdict_words(0)
        empty = np.zeros((0, 300), dtype=np.uint8)
        lens = np.zeros(0, dtype=np.uint32)
        eng.upload(0, capi.Batch.from_matrices(empty, empty, lens, empty, empty, lens))
        eng.run(0)
        assert eng.last_verdict_words(0) == 0
    finally:
        eng.close()


@pytest.mark.parametrize("max_len,words", [(150, 10), (160, 10), (161, 16), (256, 16), (257, 18), (288, 18), (289, 20), (320, 20), (321, 0)])
def test_words_at_every_tier_edge(gpu_engine, max_len, words):
    """every tier reports its own width: nothing of 288 bases or less moved, 289 .. 320 is the new tier, 321 the general kernel"""
    d = synth.make_pairs(700, max_len, seed=8800 + max_len, dirty=True)
    batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
    assert batch.max_len() == max_len
    g, o = run_both(gpu_engine, default_cfg(True), batch, qc=False)
    assert gpu_engine.last_verdict_words(0) == words
    assert_same(g, o)
    single = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"])
    g, o = run_both(gpu_engine, default_cfg(False), single, qc=False)
    assert gpu_engine.last_verdict_words(0) == words
    assert_same(g, o)


# ---- the reference's function vectors through aqc_run -------------------------------------------------------------------------------------
def test_long_overlap_golden_through_the_production_kernel(gpu_engine):
    """The reference's util.overlap answers for mates of 289 - 320 bases through aqc_run, as test_gpu_parity's
    test_overlap_golden_through_the_production_kernel does for the vectors up to 160: every filter off, no trim; the result holds
    the golden triple, or after an adapter cut (offset < 0, overlap_len > 30) the second call's, checked against the oracle, which
    test_long_reads_golden.py pins to the same fixture.  The lane-per-pair kernel itself must decide more than 95 % of the pairs
    it is built for (the project's rule, tests/test_gpu_parity.py): the share comes from aqc_last_deferred."""
    from oracle import oracle
    vec, exp_all = vectors("overlap"), golden()["func"]["overlap"]
    b = capi.Batch.from_strings([v[1] for v in vec], None, [v[2] for v in vec], None)
    cfg = default_cfg(True, seq_len_req=0, poly_size_limit=0, unqualified_base_limit=0, n_base_limit=0, no_correction=1)
    gpu_engine.set_config(cfg)
    gpu_engine.reset_stats()
    gpu_engine.upload(0, b)
    gpu_engine.run(0)
    assert gpu_engine.last_verdict_words(0) == 20
    res = gpu_engine.fetch_results(0)
    n_def, deferred = gpu_engine.last_deferred(0, want_indices=True)
    bad = []
    for i, ((tag, r1, r2), exp) in enumerate(zip(vec, exp_all)):
        r = res[i]
        got = [int(r["offset"]), int(r["overlap_len"]), int(r["distance"])]
        if exp[0] < 0 and exp[1] > 30:
            want = list(oracle.overlap(r1[:exp[1]], r2[:exp[1]]))
            if got != want or int(r["len1"]) != exp[1] or int(r["len2"]) != exp[1]:
                bad.append((i, tag, exp, want, got))
        elif got != exp:
            bad.append((i, tag, exp, got))
    assert not bad, (len(bad), bad[:5])
    plain = set("ACGTN")
    eligible = np.array([set(v[1]) <= plain and set(v[2]) <= plain for v in vec])
    was_deferred = np.zeros(len(vec), dtype=bool)
    was_deferred[deferred] = True
    assert n_def == was_deferred.sum()
    share = was_deferred[eligible].mean()
    tags = sorted(set(vec[i][0] for i in np.flatnonzero(was_deferred & eligible)))
    print("deferred: %d of %d eligible pairs (%.4f), tags %s" % (was_deferred[eligible].sum(), eligible.sum(), share, tags))
    assert eligible.sum() > 1700
    assert share < 0.05, (share, tags)


def test_long_read_stats_golden(gpu_engine):
    """hasPolyX, lowQualityNum and nNumber of the reference at 289 - 320 bases through the device's function seam, and the
    same reads through aqc_run's own polyX screen, low-quality plane and N count on the 20-word instances (single-end)"""
    vec, exp = vectors("polyx"), golden()["func"]["polyx"]
    for mp, mm in sorted(set((v[1], v[2]) for v in vec)):
        idx = [i for i, v in enumerate(vec) if (v[1], v[2]) == (mp, mm)]
        b = capi.Batch.from_strings([vec[i][0] for i in idx])
        px, _, _ = gpu_engine.read_stats(b, mp, mm, 15)
        assert px.tolist() == [0 if exp[i] is None else ord(exp[i]) for i in idx], (mp, mm)
        # the production kernel: polyX the only filter.  Lower-case reads are the general kernel's (deferred); verdicts must agree
        bq = capi.Batch.from_strings([vec[i][0] for i in idx], ["I" * len(vec[i][0]) for i in idx])
        gpu_engine.set_config(default_cfg(False, seq_len_req=0, poly_size_limit=mp, allow_mismatch_in_poly=mm, unqualified_base_limit=0, n_base_limit=0))
        gpu_engine.reset_stats()
        gpu_engine.upload(0, bq)
        gpu_engine.run(0)
        assert gpu_engine.last_verdict_words(0) == 20
        flags = gpu_engine.fetch_results(0)["flag"]
        assert [f == capi.BADPOL for f in flags] == [exp[i] is not None for i in idx], (mp, mm)
    cv, cexp = vectors("counts"), golden()["func"]["counts"]
    for qv in sorted(set(v[2] for v in cv)):
        idx = [i for i, v in enumerate(cv) if v[2] == qv]
        b = capi.Batch.from_strings([cv[i][0] for i in idx], [cv[i][1] for i in idx])
        _, lq, nn = gpu_engine.read_stats(b, 35, 2, qv)
        assert lq.tolist() == [cexp[i][0] for i in idx]
        assert nn.tolist() == [cexp[i][1] for i in idx]
        # aqc_run: the low-quality filter alone at limits below, at and above 255; then the N filter alone
        for field, col, limits in (("unqualified_base_limit", 0, (60, 254, 255, 256, 300)), ("n_base_limit", 1, (5, 60, 100))):
            for lim in limits:
                kw = dict(seq_len_req=0, poly_size_limit=0, unqualified_base_limit=0, n_base_limit=0, qualified_quality_phred=qv)
                kw[field] = lim
                gpu_engine.set_config(default_cfg(False, **kw))
                gpu_engine.reset_stats()
                gpu_engine.upload(0, b)
                gpu_engine.run(0)
                assert gpu_engine.last_verdict_words(0) == 20
                flags = gpu_engine.fetch_results(0)["flag"]
                assert [f != capi.GOOD for f in flags] == [cexp[i][col] > lim for i in idx], (field, lim, qv)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["text", "pipe", "pipe_small_chunks"])
@pytest.mark.parametrize("name", E2E_NAMES)
def test_long_e2e_on_gpu(name, mode, tmp_path):
    """the reference's outputs and statistics, byte for byte, through the serial text loop, the pipe, and the pipe with
    257-record chunks; every slot that ran reports the 20-word tier (pe_l321: the general kernel)"""
    eng = capi.Engine(0, 3)                 # a context of its own: every slot's last run is this case's
    try:
        info = {}
        work, stat = run_long_case(name, tmp_path, eng, mode, info)
        check_case(name, work, stat, golden()["e2e"])
        assert info["text_path"] and info["used_pipe"] == (mode != "text")
        seen = set()
        for slot in range(eng.n_slots):
            try:
                seen.add(eng.last_verdict_words(slot))
            except capi.AqcError:
                pass
        assert seen == {words_for(long_cases.MAX_LEN[name])}, seen
    finally:
        eng.close()


_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/tests/golden"]
import numpy as np
import long_cases
from afterqc_amd import capi
from test_gpu_long_tier import packed
eng = capi.Engine(0, 2)
out = {}
for name in long_cases.CASE_TABLE:
    batch, cfg = packed(name)
    eng.set_config(cfg)
    eng.reset_stats()
    eng.upload(0, batch)
    eng.run(0)
    res = eng.fetch_results(0)
    out[name] = dict(words=eng.last_verdict_words(0), res=res.tobytes().hex(), counters=eng.counters().tolist(),
                     hist=[h.tolist() for h in eng.histograms()])
eng.close()
json.dump(out, open(sys.argv[2], "w"))
"""


def test_same_results_under_force_generic(gpu_engine, tmp_path):
    """every end-to-end case's reads as a packed batch: the tier's results, counters and histograms are those of the general
    kernel (AQC_FORCE_GENERIC=1 is read by aqc_create, so that run is a child process) and of the oracle"""
    out = str(tmp_path / "generic.json")
    env = dict(os.environ, AQC_FORCE_GENERIC="1")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, check=True, timeout=300)
    with open(out) as f:
        generic = json.load(f)
    for name in E2E_NAMES:
        batch, cfg = packed(name)
        g, o = run_both(gpu_engine, cfg, batch, qc=False)
        assert gpu_engine.last_verdict_words(0) == words_for(long_cases.MAX_LEN[name]), name
        assert_same(g, o)
        if words_for(long_cases.MAX_LEN[name]):
            assert gpu_engine.last_deferred(0) < 0.05 * batch.n, (name, gpu_engine.last_deferred(0))
        x = generic[name]
        assert x["words"] == 0, name
        assert x["res"] == g["res"].tobytes().hex(), name
        assert x["counters"] == g["counters"].tolist(), name
        assert x["hist"] == [h.tolist() for h in g["hist"]], name


# ---- every length pair of the tier ------------------------------------------------------------------------------------------------------
def test_every_long_length_pair_vs_oracle(gpu_engine):
    """Built like test_gpu_parity's test_every_length_pairs_vs_oracle, for l1 in 289 .. 320 and l2 in {289, 290, 303, 304, 305,
    319, 320, l1}: read 2 is packed in 16-byte chunks counted from its END, both mates are padded behind their last base — at
    320 bases there is no padding left in the row — with overlapping tails so that the scan, the verification and the correction
    walk see the ends of the streams; with and without trims."""
    rng = np.random.default_rng(20261022)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    seqs1, quals1, seqs2, quals2 = [], [], [], []
    qchars = list("#/" + "5?I" * 6)
    for l1 in range(289, 321):
        for l2 in (289, 290, 303, 304, 305, 319, 320, l1):
            # the insert: a full overlap, a long one, the far end's last words
            for tail in (7, int(rng.integers(0, 260)), l1 + l2 - int(rng.integers(31, 48)) - max(l1, l2)):
                ins = "".join(rng.choice(list("ACGT"), size=max(l1, l2) + tail))
                r1 = list(ins[:l1])
                r2 = [comp[c] for c in reversed(ins[len(ins) - l2:])]
                for r in (r1, r2):                           # a few mismatches / N
                    for k in rng.integers(0, len(r), size=int(rng.integers(0, 4))):
                        r[k] = "ACGTN"[rng.integers(0, 5)]
                seqs1.append("".join(r1)); seqs2.append("".join(r2))
                # (a tenth of the bases below the qualified quality: under the low-quality filter's 60, the walk still sees both kinds)
                quals1.append("".join(rng.choice(qchars, size=l1))); quals2.append("".join(rng.choice(qchars, size=l2)))
    batch = capi.Batch.from_strings(seqs1, quals1, seqs2, quals2)
    assert batch.n == 32 * 8 * 3
    for cfgkw in (dict(seq_len_req=1), dict(seq_len_req=1, trim_front=1, trim_tail=2, trim_front2=2, trim_tail2=1),
                  dict(seq_len_req=1, trim_front=17, trim_tail=33, trim_front2=31, trim_tail2=16)):
        g, o = run_both(gpu_engine, default_cfg(True, **cfgkw), batch, qc=False)
        assert gpu_engine.last_verdict_words(0) == 20
        assert_same(g, o)
        print("overlapped:", int((g["res"]["overlap_len"] > 30).sum()), "flags:", np.bincount(g["res"]["flag"], minlength=12).tolist())
        assert (g["res"]["overlap_len"] > 30).sum() > batch.n // 2
        assert gpu_engine.last_deferred(0) < 0.05 * batch.n


# ---- more pairs than the persistent grid holds ------------------------------------------------------------------------------------------
def test_batch_larger_than_the_grid_vs_oracle(gpu_engine):
    """100,000 pairs of 2 x 300: the grid of 256 CUs x 11 waves x 32 pairs holds 90,112 (81,920 in a 10-wave build), so waves
    draw a second batch from the ticket counter and the counter flush runs behind it.  Results, counters and histograms against the oracle."""
    d = synth.make_pairs(100000, 300, seed=77001, dirty=True)
    batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
    g, o = run_both(gpu_engine, default_cfg(True), batch, qc=False)
    assert gpu_engine.last_verdict_words(0) == 20
    assert_same(g, o)
    assert int(g["counters"][capi.C_TOTAL_READS]) == 100000
    assert gpu_engine.last_deferred(0) < 0.05 * batch.n


@pytest.mark.parametrize("paired", [True, False])
def test_barcode_l317_vs_oracle(gpu_engine, paired):
    """2 x 300 plus the 17-base prefix with QC, bubbles and barcode tails, ragged too: the barcode instances of the tier"""
    import cases
    for ragged in (False, True):
        d = synth.make_pairs(1500, 300, seed=7317 + ragged, dirty=True, ragged=ragged)
        d = synth.add_barcodes(d, 7318, tail_frac=0.25)
        if paired:
            batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])
        else:
            batch = capi.Batch.from_matrices(d["seq1"], d["qual1"], d["len1"])
        assert batch.max_len() == 317
        lane, tile, x, y = d["meta"]
        which = tile % len(cases.CIRCLES)
        batch.set_aux(np.array([c[3] for c in cases.CIRCLES])[which], np.array([c[4] for c in cases.CIRCLES])[which], x, y, (x % 7 != 0).astype(np.uint8))
        cfg = default_cfg(paired, barcode=1, debubble=1, seq_len_req=20 if ragged else 35, trim_tail=3 if ragged else 0, trim_tail2=2 if ragged else 0)
        g, o = run_both(gpu_engine, cfg, batch, circles=cases.CIRCLES, qc=not ragged)
        assert gpu_engine.last_verdict_words(0) == 20
        assert_same(g, o)
        flags = np.bincount(g["res"]["flag"], minlength=12)
        assert flags[capi.BADBCD1] > 0 and flags[capi.BADBBL] > 0 and flags[capi.GOOD] > 500
        assert gpu_engine.last_deferred(0) < 0.05 * batch.n
