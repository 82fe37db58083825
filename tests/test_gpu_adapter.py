"""Trimming a given adapter from each read on the GPU (-m gpu): --adapter_sequence / --adapter_sequence_r2 / --adapter_min_overlap
from the adapter pass (adapter_cut_kernel, csrc/aqc_adapter.hpp) through the verdict kernels to the CLI, against the model of
tests/adapter_rule.py.

  seam        aqc_adapter_views against the model, one batch per group size of the pass (8, 16, 32, 64 lanes per read): the lengths
              at which the pass changes shape, every named placement at every length, six adapter lengths, K of 1, 4 and m;
              irregular quality lines, fixed trims, an incoming view (NULL and given); a read that is too long.
  verdicts    a run with the adapter on against a run of the same build, options off, on precut(records): every tier of the
              lane-per-read kernel, paired and single-end, and the general kernel (reads of 321 bases; AQC_FORCE_GENERIC=1 in a
              child) — each once more with a quality cut on as well; different adapters for the mates; only read 2 searched.
  below 5     records the adapter leaves under 5 bases, against the model: BADTRIM1 with read 2 untouched, BADTRIM2, the bad files' text.
  counts      aqc_get_adapter_stats against the model, with an accum_limit, over two contexts, with a cut on; aqc_get_cut_stats of
              the same run equal to those of a run without the adapter.
  end to end  the CLI through the whole-input pipe and the serial text loop against a run on pre-cut files with the options off.
  off is off  aqc_set_adapter_trim(NULL) after an adapter run gives what a context that never had it gives."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):       # (the child process below runs this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adapter_rule
import cut_rule
import viewpass_cases as vc
from afterqc_amd import after, capi, preprocesser

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED, ERR_READ_TOO_LONG = vc.ERR_UNSUPPORTED, -3
GROUP_LENGTHS, GROUP_RANGE = vc.GROUP_LENGTHS, vc.GROUP_RANGE
SEAM_ADAPTER_LENGTHS = [4, 8, 9, 17, 33, 64]
A1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"          # 33 bases
A2 = b"CTGTCTCTTATACACATCT"                        # 19


def adcfg(a1=b"", a2=b"", K=4):
    return capi.AdapterConfig(a1, a2, K)


views, se, run_pairs = vc.views, vc.se, vc.run_pairs


# ---- the seam against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sorted(GROUP_LENGTHS))
@pytest.mark.parametrize("m", SEAM_ADAPTER_LENGTHS)
def test_seam_against_the_model(m, G, gpu_engine):
    """no incoming view, one batch per group size and K: adapter_cut_kernel<8>, <16>, <32> and <64> each against the model"""
    rng = random.Random(5200 + 7 * m + G)
    A = adapter_rule.make_adapter(rng, m)
    for K in sorted({1, 4, m}):
        reads = [s for n in GROUP_LENGTHS[G] for _, s in adapter_rule.placements(n, A, K, rng)]
        batch = vc.pack(reads, [b"I" * len(s) for s in reads])
        assert batch.qlen1 is None and GROUP_RANGE[G][0] <= batch.max_len() <= GROUP_RANGE[G][1]
        got = views(*gpu_engine.adapter_views(batch, adcfg(A, b"", K)))
        want = [adapter_rule.compose(adapter_rule.VIEW_ALL, s, A, K) for s in reads]
        bad = [i for i in range(len(reads)) if got[i] != want[i]]
        assert not bad, (m, G, K, len(bad), [(len(reads[i]), got[i], want[i]) for i in bad[:5]])
        assert sum(1 for w in want if w != adapter_rule.VIEW_ALL) > len(reads) // 3


@pytest.mark.parametrize("trim", [(0, 0), (3, 0), (0, 7), (200, 200)])
def test_seam_fixed_trim_irregular_lines_and_an_incoming_view(trim, gpu_engine):
    """150-base reads behind a fixed trim, a third of them with a quality line of its own length (their length words carry the
    mark of such a record, the batch takes adapter_cut_kernel<64>), then the same reads with regular lines (<16>); each without an
    incoming view and with one — views that end in front of the adapter, inside it, behind it, and that start beyond the
    sequence's end"""
    rng = random.Random(91 + trim[0])
    seqs, quals = [], []
    for i in range(600):
        s = adapter_rule.bases(rng, 150)
        if i % 4:
            s = adapter_rule.plant(s, rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 30, 100, 140, 143, 146]) + rng.randrange(3), A1)
        seqs.append(s)
        quals.append(b"I" * (150 if i % 3 else rng.choice([0, 1, 4, 17, 100, 149, 151, 170, 400, 1000])))
    vin = [(0, 0xffff) if i % 5 == 0 else (c0, rng.choice([0xffff, c0, c0 + rng.randrange(0, 160)]))
           for i, c0 in enumerate(rng.choice([0, 0, 1, 3, 9, 29, 100, 149, 150, 151, 400]) for _ in range(600))]
    arrays = (np.array([v[0] for v in vin]), np.array([v[1] for v in vin]))
    for irregular in (True, False):
        batch = vc.pack(seqs, quals if irregular else [b"I" * 150] * 600)
        assert (batch.qlen1 is not None) == irregular
        for K, a in ((4, A1), (1, A1[:9])):
            got = views(*gpu_engine.adapter_views(batch, adcfg(a, b"", K), trim[0], trim[1]))
            assert got == [adapter_rule.compose(adapter_rule.VIEW_ALL, cut_rule.trim(s, *trim), a, K) for s in seqs], (irregular, K)
            got = views(*gpu_engine.adapter_views(batch, adcfg(a, b"", K), trim[0], trim[1], view_in=arrays))
            assert got == [adapter_rule.compose(v, cut_rule.trim(s, *trim), a, K) for s, v in zip(seqs, vin)], (irregular, K)


def test_seam_refuses_bad_options_and_long_reads(gpu_engine):
    batch = vc.pack([b"ACGTACGTAC"], [b"IIIIIIIIII"])
    for a, K in ((b"ACG", 1), (b"A" * 65, 4), (b"ACGN", 4), (b"acgt", 4), (b"ACGT", 0), (b"ACGT", 5)):
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.adapter_views(batch, adcfg(a, b"", K))
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.set_adapter_trim(adcfg(a, b"", K))
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.set_adapter_trim(adcfg(b"ACGTACGT", a, K))
        assert e.value.code == capi.ERR_ARG
    gpu_engine.set_adapter_trim(adcfg(b"", b"", 0))             # no adapter: off, whatever the rest says
    gpu_engine.set_adapter_trim(None)
    long_read = adapter_rule.bases(random.Random(1), 1001)
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.adapter_views(vc.pack([b"ACGT", long_read], [b"IIII", b"I" * 1001]), adcfg(b"ACGT"))
    assert e.value.code == ERR_READ_TOO_LONG


# ---- verdicts: the adapter on against a run on the pre-cut records --------------------------------------------------------------
def adapter_pairs(n, L, seed, a1, a2, short=()):
    """vc.tailed_pairs with adapters written over 30 % of the mates (adapter_rule.with_adapters: from place 20 on, a third of
    them 4 .. 20 adapter bases at the very end, some bases substituted)"""
    return adapter_rule.with_adapters(random.Random(seed), vc.tailed_pairs(n, L, seed, short), a1, a2)


def model_of(a1, a2, K, modes=None, trim=(0, 0)):
    return vc.model_of(modes, trim, a1, a2, K)


def check_against_precut(eng, pairs, paired, trim, a1, a2, K, words):
    """the adapter on, without and with a quality cut, each against the same build on the model's pre-cut records, options off"""
    plain = None
    try:
        for modes in (None, (0, 1, 0)):
            model = model_of(a1, a2, K, modes, trim)
            pre = adapter_rule.precut_pairs(pairs, model, paired)
            assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
            A = run_pairs(eng, pairs, paired, vc.base_config(paired, trim), vc.cutcfg(modes) if modes else None, adcfg(a1, a2 if paired else b"", K))
            B = run_pairs(eng, pre, paired, vc.base_config(paired), None, None)
            assert A["words"] == words
            assert A["adapter_ms"] > 0 and B["adapter_ms"] == 0 and (A["cut_ms"] > 0) == bool(modes)
            vc.compare_runs(pairs, pre, A, B, paired)
            want = adapter_rule.adapter_counts(se(pairs, paired), model)
            assert A["adapter_stats"].tolist() == want and want[0] > len(pairs) // 8
            # the quality cut's own counts are what they are without the adapter
            assert A["cut_stats"].tolist() == (cut_rule.cut_counts(se(pairs, paired), model.cut) if modes else [0, 0, 0, 0])
            if modes is None:
                plain = pre
            else:
                assert pre != plain                                 # (the cut does take part)
    finally:
        vc.set_passes(eng)


VERDICT_CASES = [(150, 10, True, (2, 3)), (150, 10, False, (0, 0)), (250, 16, True, (0, 0)), (250, 16, False, (2, 3)),
                 (280, 18, True, (2, 3)), (280, 18, False, (0, 0)), (310, 20, True, (0, 0)), (310, 20, False, (2, 3)),
                 (321, 0, True, (2, 3)), (321, 0, False, (0, 0))]


@pytest.mark.parametrize("L,words,paired,trim", VERDICT_CASES)
def test_verdicts_equal_a_run_on_precut_records(L, words, paired, trim, gpu_engine):
    """every tier and the general kernel; the paired cases with a different adapter for each mate"""
    pairs = adapter_pairs(700, L, 1300 + L + int(paired), A1, A2 if paired else A1)
    check_against_precut(gpu_engine, pairs, paired, trim, A1, A2 if paired else b"", 4, words)


def test_only_read_2_is_searched(gpu_engine):
    pairs = adapter_pairs(700, 150, 77, A2, A2)                # (both mates carry it; read 1's stays)
    model = model_of(b"", A2, 5)
    pre = adapter_rule.precut_pairs(pairs, model, True)
    assert all(p[0] == q[0] for p, q in zip(pairs, pre)) and sum(1 for p, q in zip(pairs, pre) if p[2] != q[2]) > 100
    A = run_pairs(gpu_engine, pairs, True, vc.base_config(True), None, adcfg(b"", A2, 5))
    B = run_pairs(gpu_engine, pre, True, vc.base_config(True), None, None)
    vc.compare_runs(pairs, pre, A, B, True)
    want = adapter_rule.adapter_counts(pairs, model)
    assert A["adapter_stats"].tolist() == want and want[:2] == [0, 0] and want[2] > 100


# ---- records the adapter leaves under 5 bases ----------------------------------------------------------------------------------
def sub5_pairs(n=400, L=150, seed=5):
    """even records: read 1 has its adapter at place 0 .. 4 (0: a dimer); odd: read 2; every fifth: both"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = [adapter_rule.clean_read(rng, L, A1), adapter_rule.clean_read(rng, L, A2)]
        for k in {i % 2} | ({1} if i % 5 == 0 else set()):
            s[k] = adapter_rule.plant(s[k], rng.randint(0, 4), (A1, A2)[k])
        out.append((s[0], bytes(rng.randrange(33 + 25, 33 + 41) for _ in range(L)), s[1], bytes(rng.randrange(33 + 25, 33 + 41) for _ in range(L))))
    return out


def test_reads_trimmed_below_five_bases(gpu_engine):
    pairs = sub5_pairs()
    model = model_of(A1, A2, 4)
    A = run_pairs(gpu_engine, pairs, True, vc.base_config(True), None, adcfg(A1, A2, 4), accum_limit=300)
    gpu_engine.set_adapter_trim(None)
    vc.check_below_five(pairs, A["res"], adapter_rule, model)
    # records below accum_limit only, and read 2 is not counted where read 1 ended the record
    assert A["adapter_stats"].tolist() == adapter_rule.adapter_counts(pairs, model, accum_limit=300)
    assert int(A["counters"][capi.C_FLAG0 + capi.BADTRIM1]) + int(A["counters"][capi.C_FLAG0 + capi.BADTRIM2]) == 300


def test_bad_file_text_of_reads_trimmed_below_five_bases(gpu_engine):
    """text in, text out: every record goes to the bad streams as @BADTRIM1... / @BADTRIM2..., read 1 trimmed, read 2 only under BADTRIM2"""
    pairs = sub5_pairs(300, 150, 6)
    model = model_of(A1, A2, 4)
    gpu_engine.set_config(vc.base_config(True))
    vc.set_passes(gpu_engine, adapter=adcfg(A1, A2, 4))
    try:
        got = vc.bad_streams(gpu_engine, pairs)
    finally:
        vc.set_passes(gpu_engine)
    assert got == vc.badtrim_text(pairs, adapter_rule, model)


# ---- the counts ---------------------------------------------------------------------------------------------------------------
def test_adapter_stats_over_two_contexts_with_a_cut_on(gpu_engine):
    pairs = adapter_pairs(600, 150, 12, A1, A2)
    modes = (1, 1, 0)
    model = model_of(A1, A2, 4, modes)
    other = capi.Engine(0, 2)
    try:
        a = run_pairs(gpu_engine, pairs[:350], True, vc.base_config(True), vc.cutcfg(modes), adcfg(A1, A2, 4))
        b = run_pairs(other, pairs[350:], True, vc.base_config(True), vc.cutcfg(modes), adcfg(A1, A2, 4))
        both = capi.MergedEngines([gpu_engine, other])
        merged, merged_cut = both.adapter_stats().tolist(), both.cut_stats().tolist()
        assert merged == adapter_rule.adapter_counts(pairs, model) and merged[0] > 50 and merged[2] > 50
        assert (a["adapter_stats"] + b["adapter_stats"]).tolist() == merged
        # the quality cut's counts of the same run: those of a run without the adapter
        c = run_pairs(gpu_engine, pairs[:350], True, vc.base_config(True), vc.cutcfg(modes), None)
        d = run_pairs(other, pairs[350:], True, vc.base_config(True), vc.cutcfg(modes), None)
        assert merged_cut == (c["cut_stats"] + d["cut_stats"]).tolist() == cut_rule.cut_counts(pairs, model.cut)
        assert c["adapter_stats"].tolist() == [0, 0, 0, 0] and c["adapter_ms"] == 0
        # an accum_limit
        e = run_pairs(gpu_engine, pairs, True, vc.base_config(True), vc.cutcfg(modes), adcfg(A1, A2, 4), accum_limit=211)
        assert e["adapter_stats"].tolist() == adapter_rule.adapter_counts(pairs, model, accum_limit=211)
        gpu_engine.reset_stats()
        assert gpu_engine.adapter_stats().tolist() == [0, 0, 0, 0]
    finally:
        other.close()
        vc.set_passes(gpu_engine)


# ---- off is off -------------------------------------------------------------------------------------------------------------
def test_off_after_an_adapter_run_is_the_run_without_it(gpu_engine):
    pairs = adapter_pairs(1200, 150, 44, A1, A2)
    cfg = vc.base_config(True, (2, 3))
    fresh = capi.Engine(0, 2)
    try:
        want = run_pairs(fresh, pairs, True, cfg, None, None)          # a context that never had an adapter
    finally:
        fresh.close()
    on = run_pairs(gpu_engine, pairs, True, cfg, None, adcfg(A1, A2, 4))
    assert on["adapter_ms"] > 0 and on["res"].tobytes() != want["res"].tobytes()
    got = run_pairs(gpu_engine, pairs, True, cfg, None, None)          # the same slot, the adapter taken away again
    assert got["res"].tobytes() == want["res"].tobytes()
    assert np.array_equal(got["counters"], want["counters"]) and np.array_equal(got["ovl"], want["ovl"]) and np.array_equal(got["dist"], want["dist"])
    assert got["adapter_ms"] == 0 and got["cut_ms"] == 0 and got["words"] == want["words"] == 10
    assert got["adapter_stats"].tolist() == [0, 0, 0, 0]


def test_barcode_with_an_adapter_is_unsupported(gpu_engine):
    pairs = vc.tailed_pairs(64, 150, 3)
    cfg = vc.base_config(True)
    cfg.barcode = 1
    with pytest.raises(capi.AqcError) as e:
        run_pairs(gpu_engine, pairs, True, cfg, None, adcfg(A1, A2, 4))
    assert e.value.code == ERR_UNSUPPORTED
    gpu_engine.set_adapter_trim(None)


# ---- a child process: AQC_FORCE_GENERIC=1 -----------------------------------------------------------------------------------------
def child_generic():
    """the general kernel alone decides 150-base pairs with the adapter on, without and with a cut"""
    eng = capi.Engine(0, 2)
    pairs = adapter_pairs(600, 150, 71, A1, A2)
    check_against_precut(eng, pairs, True, (2, 3), A1, A2, 4, 0)
    print(json.dumps({"ok": True}))


def test_general_kernel_alone_in_a_child_process():
    assert vc.run_child(__file__, "generic", {"AQC_FORCE_GENERIC": "1"}) == {"ok": True}


# ---- end to end -------------------------------------------------------------------------------------------------------------
def e2e_pairs(n, L, seed, a1, a2):
    """adapter pairs with one record whose quality line is longer than its sequence line"""
    pairs = adapter_pairs(n, L, seed, a1, a2)
    s1, q1, s2, q2 = pairs[9]
    pairs[9] = (s1, q1 + bytes([33 + 30]) * 11, s2, q2)
    return pairs


E2E_CASES = {
    # name: (paired, input compression, argv with the adapter, argv of the pre-cut run, driver, index files)
    # (plain, .gz and .bz2 input, single-end and paired, through each of the two drivers: twelve cells, the first twelve cases)
    "pipe_se": (False, "", [], [], "pipe_small_chunks", False),
    "pipe_se_gz": (False, ".gz", [], [], "pipe_small_chunks", False),
    "pipe_se_bz2": (False, ".bz2", ["--adapter_min_overlap", "5"], [], "pipe_small_chunks", False),
    "pipe_pe": (True, "", [], [], "pipe_small_chunks", False),
    "text_se": (False, "", [], [], "text", False),
    "text_pe_gz": (True, ".gz", [], [], "text", False),
    "text_pe_bz2": (True, ".bz2", ["--adapter_sequence_r2", A2.decode()], [], "text", False),
    "pipe_pe_gz": (True, ".gz", ["--adapter_sequence_r2", A2.decode()], [], "pipe_small_chunks", False),
    "pipe_pe_bz2_no_overlap": (True, ".bz2", ["--no_overlap"], ["--no_overlap"], "pipe_small_chunks", False),
    "pipe_two_contexts_merged": (True, "", ["--store_merged", "on"], ["--store_merged", "on"], "pipe_two_contexts", False),
    "text_se_gz": (False, ".gz", ["--adapter_min_overlap", "6"], [], "text", False),
    "text_se_bz2_cut": (False, ".bz2", ["--cut_tail", "on"], [], "text", False),
    "text_pe": (True, "", ["--adapter_sequence_r2", A2.decode(), "--adapter_min_overlap", "3"], [], "text", False),
    "text_pe_index": (True, "", [], [], "text", True),
    "text_pe_debubble": (True, "", ["--debubble"], ["--debubble"], "text", False),
    "text_pe_qc_only": (True, "", ["--qc_only", "--qc_sample", "300"], ["--qc_only", "--qc_sample", "300"], "text", False),
}


@pytest.mark.parametrize("name", sorted(E2E_CASES))
def test_cli_equals_a_run_on_precut_files(name, tmp_path, gpu_engine):
    paired, gz, argv_on, argv_pre, driver, index = E2E_CASES[name]
    trim = (2, 3) if name in ("text_se_gz", "pipe_pe_gz") else (0, 0)
    a2 = A2 if "--adapter_sequence_r2" in argv_on else A1
    K = int(argv_on[argv_on.index("--adapter_min_overlap") + 1]) if "--adapter_min_overlap" in argv_on else 4
    model = model_of(A1, a2, K, (0, 1, 0) if "--cut_tail" in argv_on else None, trim)
    pairs = e2e_pairs(900, 150, 500 + len(name), A1, a2)
    pre = adapter_rule.precut_pairs(pairs, model, paired)
    assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
    assert any(len(p[0]) != len(p[1]) for p in pairs)
    kw = vc.driver_kw(driver)
    work = [os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")]
    fa = vc.write_inputs(work[0], "raw", pairs, paired, gz, index)
    fb = vc.write_inputs(work[1], "pre", [p if paired else (p[0], p[1], b"", b"") for p in pre], paired, gz, index)
    extra = []
    if "--debubble" in argv_on:
        with open(os.path.join(str(tmp_path), "circles.csv"), "w") as f:
            f.write("x,y,radius,lane,tile\n1100,2100,30,1,101\n")
        extra = ["--debubble_dir", str(tmp_path)]
    sa, pipe_a = vc.run_cli(work[0], fa, paired, ["-f", str(trim[0]), "-t", str(trim[1]), "--adapter_sequence", A1.decode().lower()] + argv_on + extra, kw, gpu_engine, index)
    sb, pipe_b = vc.run_cli(work[1], fb, paired, ["-f", "0", "-t", "0"] + argv_pre + extra, kw, gpu_engine, index)
    # the driver the case names is the driver that ran: no quiet fall-back to the serial loop with the adapter on
    assert pipe_a == pipe_b == name.startswith("pipe_"), (pipe_a, pipe_b)
    oa, ob = vc.read_outputs(work[0]), vc.read_outputs(work[1])
    assert sorted(oa) == sorted(ob)
    if "--qc_only" in argv_on:
        assert not oa
    else:
        assert any(k.startswith("good/") and oa[k] for k in oa) and any(k.startswith("bad/") for k in oa)
    if "--store_merged" in argv_on:
        assert any(k.startswith("merged/") and oa[k] for k in oa)
    if "--debubble" in argv_on:
        assert sa["afterqc_main_summary"]["bad_reads_with_reads_in_bubble"] >= 20          # (the bubble filter took part)
    for k in oa:
        assert oa[k] == ob[k], k
    # the statistics: every key the run without the options has, but what sees the raw reads — total_bases, the pre-filter QC
    # sections and readlen — the echo of the options, and the two objects of the trim stage's own options
    assert "adapter_trim" in sa and "adapter_trim" not in sb
    counted = sb["afterqc_main_summary"]["total_reads"] if "--qc_only" in argv_on else None
    assert counted is None or 300 <= counted < len(pairs)
    want = adapter_rule.adapter_counts(se(pairs, paired), model, accum_limit=counted)
    at = sa["adapter_trim"]
    assert [at["read1_trimmed_reads"], at["read1_trimmed_bases"], at["read2_trimmed_reads"], at["read2_trimmed_bases"]] == want
    assert want[0] > 50 and (not paired or want[2] > 50)
    assert (at["adapter_sequence"], at["adapter_sequence_r2"], at["adapter_min_overlap"]) == (A1.decode(), a2.decode() if paired else "", K)
    if "--cut_tail" in argv_on:
        # the same bytes as the same run without the adapter options
        sc, _ = vc.run_cli(os.path.join(str(tmp_path), "c"), fa, paired, ["-f", str(trim[0]), "-t", str(trim[1])] + argv_on, kw, gpu_engine, index)
        assert json.dumps(sa["quality_cut"], sort_keys=True) == json.dumps(sc["quality_cut"], sort_keys=True)
        assert sa["quality_cut"]["read1_cut_reads"] > 100
    assert sorted(k for k in sa if k not in ("adapter_trim", "quality_cut")) == sorted(sb)
    vc.compare_cli_stats(sa, sb)


def test_folder_mode_with_debubble(tmp_path):
    """`-d DIR --debubble` with an adapter: after.main pairs the folder's files, finds the circles of an earlier pre-pass and runs
    each pair on an engine of its own — against the same command on the folder of pre-cut files, options off"""
    model = model_of(A1, A1, 4)
    pairs = e2e_pairs(900, 150, 640, A1, A1)
    pre = adapter_rule.precut_pairs(pairs, model, True)
    assert min(len(p[0]) for p in pre) >= 5 and min(len(p[2]) for p in pre) >= 5
    bubbles = os.path.join(str(tmp_path), "bubbles")
    os.makedirs(bubbles)
    with open(os.path.join(bubbles, "circles.csv"), "w") as f:
        f.write("x,y,radius,lane,tile\n1100,2100,30,1,101\n")
    stats = []
    for tag, recs, extra in (("raw", pairs, ["--adapter_sequence", A1.decode()]), ("pre", pre, [])):
        work = os.path.join(str(tmp_path), tag)
        vc.write_inputs(os.path.join(work, "in"), tag, recs, True, "")
        after.main(["-d", os.path.join(work, "in"), "--debubble", "--debubble_dir", bubbles, "-f", "0", "-t", "0", "--qc_sample", "0", "--barcode", "off",
                    "-g", os.path.join(work, "good"), "-b", os.path.join(work, "bad"), "-r", os.path.join(work, "QC")] + extra)
        with open(os.path.join(work, "QC", "%s_R1.fq.json" % tag)) as f:
            stats.append(json.load(f))
    oa, ob = vc.read_outputs(os.path.join(str(tmp_path), "raw")), vc.read_outputs(os.path.join(str(tmp_path), "pre"))
    assert sorted(oa) == sorted(ob) and any(k.startswith("good/") and oa[k] for k in oa) and any(k.startswith("bad/") and oa[k] for k in oa)
    for k in oa:
        assert oa[k] == ob[k], k
    sa, sb = stats
    assert sa["afterqc_main_summary"]["bad_reads_with_reads_in_bubble"] == sb["afterqc_main_summary"]["bad_reads_with_reads_in_bubble"] >= 20
    at = sa["adapter_trim"]
    assert [at["read1_trimmed_reads"], at["read1_trimmed_bases"], at["read2_trimmed_reads"], at["read2_trimmed_bases"]] == adapter_rule.adapter_counts(pairs, model)
    assert "adapter_trim" not in sb
    assert {k: v for k, v in sa["afterqc_main_summary"].items() if k not in ("total_bases", "readlen")} == \
           {k: v for k, v in sb["afterqc_main_summary"].items() if k not in ("total_bases", "readlen")}


def test_cli_refuses_barcoded_input(tmp_path, gpu_engine):
    pairs = vc.tailed_pairs(64, 150, 3)
    files = vc.write_inputs(str(tmp_path), "raw", pairs, True, "")
    options, _ = after.parseCommand(["-1", files[0], "-2", files[1], "-g", os.path.join(str(tmp_path), "good"), "--adapter_sequence", A1.decode()])
    after.finalize_options(options)
    options.barcode = True
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(options, engine=gpu_engine).run()
    assert "barcode" in str(e.value) and "adapter" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "good"))


if __name__ == "__main__":
    {"generic": child_generic}[sys.argv[1]]()
