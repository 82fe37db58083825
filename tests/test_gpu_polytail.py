"""Cutting poly-G / poly-X tails from each read on the GPU (-m gpu): --trim_poly_g / --trim_poly_x / --poly_g_min_len /
--poly_x_min_len against the model of tests/poly_rule.py.

  seam        aqc_poly_views against the model, one batch per group size of the pass (8, 16, 32, 64 lanes per read): the lengths
              at which it changes shape, every named placement, G alone, X alone and both; fixed trims, quality lines of their
              own length, an incoming view; bad options and a read that is too long
  verdicts    a run with the option on against a run of the same build, options off, on the model's pre-cut records: every tier,
              the general kernel, single-end and paired, each once more with a quality cut and an adapter on as well
  below 5     whole-read poly-G: BADTRIM1 with read 2 untouched, BADTRIM2; the bad files' text byte for byte
  counts      aqc_get_poly_stats against the model, with an accum_limit, over two contexts; the cut's and the adapter's counts of
              the same run are those of a run without the poly options
  off is off  aqc_set_poly_trim(NULL) after a poly run gives what a context that never had it gives
  end to end  the CLI against the CLI on pre-cut files, options off."""
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
import poly_rule
import viewpass_cases as vc
from afterqc_amd import after, capi, preprocesser

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED, ERR_READ_TOO_LONG = vc.ERR_UNSUPPORTED, -3
GROUP_LENGTHS, GROUP_RANGE = vc.GROUP_LENGTHS, vc.GROUP_RANGE
A1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
G = ord("G")
# G alone, X alone, both with different lengths (G takes the smaller one)
LETTER_SETS = {"g": (0, 0, 10, 0), "x": (8, 8, 8, 8), "both": (17, 17, 2, 17), "g1": (0, 0, 1, 0), "g40": (0, 0, 40, 0)}


def pcfg(lens):
    return capi.PolyConfig(*lens)


views, se, run_pairs = vc.views, vc.se, vc.run_pairs


# ---- the seam against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grp", sorted(GROUP_LENGTHS))
@pytest.mark.parametrize("name", sorted(LETTER_SETS))
def test_seam_against_the_model(name, grp, gpu_engine):
    """no incoming view, one batch per group size and set of letters: poly_tail_kernel<8>, <16>, <32> and <64> each against the
    model, every named placement of every letter that is on at every length of the group"""
    lens = LETTER_SETS[name]
    rng = random.Random(6100 + grp + len(name))
    reads = []
    for X, L in zip(poly_rule.LETTERS, lens):
        if L:
            reads += [s for n in GROUP_LENGTHS[grp] for _, s in poly_rule.placements(n, X, L, rng)]
    batch = vc.pack(reads, [b"I" * len(s) for s in reads])
    assert batch.qlen1 is None and GROUP_RANGE[grp][0] <= batch.max_len() <= GROUP_RANGE[grp][1]
    got = views(*gpu_engine.poly_views(batch, pcfg(lens)))
    want = [poly_rule.compose(poly_rule.VIEW_ALL, s, lens) for s in reads]
    bad = [i for i in range(len(reads)) if got[i] != want[i]]
    assert not bad, (name, grp, len(bad), [(len(reads[i]), got[i], want[i]) for i in bad[:5]])
    n_cut = sum(1 for w in want if w != poly_rule.VIEW_ALL)
    # (L = 40 cuts no read under 40 bases: fewer in the batch of the short lengths)
    assert n_cut > len(reads) // 8 and len(reads) - n_cut > len(reads) // 20, (n_cut, len(reads))


@pytest.mark.parametrize("trim", [(0, 0), (3, 0), (0, 7), (200, 200)])
def test_seam_fixed_trim_irregular_lines_and_an_incoming_view(trim, gpu_engine):
    """150-base reads behind a fixed trim, a third of them with a quality line of its own length (their length words carry the
    mark of such a record, the batch takes poly_tail_kernel<64>), then the same reads with regular lines (<16>); each without an
    incoming view and with one — views that end in front of the tail, inside it, behind it, and that start beyond the line"""
    rng = random.Random(93 + trim[0])
    seqs, quals = [], []
    for i in range(600):
        s = poly_rule.bases(rng, 150)
        if i % 4:
            X = G if i % 3 else rng.choice(b"ACT")
            s = poly_rule.with_tail(s, rng.choice([8, 9, 10, 11, 16, 17, 20, 33, 60, 140, 150]) + rng.randrange(3), X)
            if i % 8 == 1:
                s = poly_rule.substitute(rng, s, [150 - 1 - rng.randrange(20)])
        seqs.append(s)
        quals.append(b"I" * (150 if i % 3 else rng.choice([0, 1, 4, 17, 100, 149, 151, 170, 400, 1000])))
    vin = [(0, 0xffff) if i % 5 == 0 else (c0, rng.choice([0xffff, c0, c0 + rng.randrange(0, 160)]))
           for i, c0 in enumerate(rng.choice([0, 0, 1, 3, 9, 29, 100, 149, 150, 151, 400]) for _ in range(600))]
    arrays = (np.array([v[0] for v in vin]), np.array([v[1] for v in vin]))
    for irregular in (True, False):
        batch = vc.pack(seqs, quals if irregular else [b"I" * 150] * 600)
        assert (batch.qlen1 is not None) == irregular
        for lens in ((0, 0, 10, 0), (12, 12, 5, 12)):
            got = views(*gpu_engine.poly_views(batch, pcfg(lens), trim[0], trim[1]))
            want = [poly_rule.compose(poly_rule.VIEW_ALL, cut_rule.trim(s, *trim), lens) for s in seqs]
            assert got == want, (irregular, lens)
            assert trim == (200, 200) or sum(1 for w in want if w != poly_rule.VIEW_ALL) > 150
            got = views(*gpu_engine.poly_views(batch, pcfg(lens), trim[0], trim[1], view_in=arrays))
            want = [poly_rule.compose(v, cut_rule.trim(s, *trim), lens) for s, v in zip(seqs, vin)]
            assert got == want, (irregular, lens)
            assert trim == (200, 200) or sum(1 for w, v in zip(want, vin) if w != v) > 60


def test_seam_refuses_bad_options_and_long_reads(gpu_engine):
    batch = vc.pack([b"ACGTACGTAC"], [b"IIIIIIIIII"])
    try:
        for lens in ((0, 0, -1, 0), (0, 0, 1001, 0), (1001, 10, 10, 10), (10, 10, 10, -5), (0, -2 ** 31, 0, 0)):
            with pytest.raises(capi.AqcError) as e:
                gpu_engine.poly_views(batch, pcfg(lens))
            assert e.value.code == capi.ERR_ARG
            with pytest.raises(capi.AqcError) as e:
                gpu_engine.set_poly_trim(pcfg(lens))
            assert e.value.code == capi.ERR_ARG and "aqc_set_poly_trim" in str(e.value)
        for trim in ((-1, 0), (0, -1)):
            with pytest.raises(capi.AqcError) as e:
                gpu_engine.poly_views(batch, pcfg((0, 0, 10, 0)), *trim)
            assert e.value.code == capi.ERR_ARG
        gpu_engine.set_poly_trim(pcfg((1, 1000, 1, 1000)))
        gpu_engine.set_poly_trim(pcfg((0, 0, 0, 0)))                # every letter off: off
        gpu_engine.set_poly_trim(None)
        long_read = poly_rule.bases(random.Random(1), 1001)
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.poly_views(vc.pack([b"ACGT", long_read], [b"IIII", b"I" * 1001]), pcfg((0, 0, 10, 0)))
        assert e.value.code == ERR_READ_TOO_LONG
    finally:
        gpu_engine.set_poly_trim(None)


# ---- verdicts: the option on against a run on the pre-cut records ------------------------------------------------------------------
def poly_pairs(n, L, seed, short=()):
    """vc.tailed_pairs with tails of 10 .. 60 bases written over 30 % of the mates (poly_rule.with_tails: mostly G, one
    substitution in half of the longer ones)"""
    return poly_rule.with_tails(random.Random(seed), vc.tailed_pairs(n, L, seed, short))


def model_of(lens, modes=None, trim=(0, 0), a1=b"", a2=b"", K=4):
    return vc.model_of(modes, trim, a1, a2, K, lens)


def check_against_precut(eng, pairs, paired, trim, words):
    """G alone and poly-X, then G with a quality cut and an adapter on as well, each against the same build on the model's pre-cut
    records, options off"""
    seen = []
    try:
        for lens, modes, a in (((0, 0, 10, 0), None, b""), ((10, 10, 10, 10), None, b""), ((0, 0, 10, 0), (0, 1, 0), A1)):
            model = model_of(lens, modes, trim, a, a if paired else b"")
            pre = poly_rule.precut_pairs(pairs, model, paired)
            assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
            A = run_pairs(eng, pairs, paired, vc.base_config(paired, trim), vc.cutcfg(modes) if modes else None,
                          capi.AdapterConfig(a, a if paired else b"", 4) if a else None, pcfg(lens))
            B = run_pairs(eng, pre, paired, vc.base_config(paired), None, None, None)
            assert A["words"] == words
            assert A["poly_ms"] > 0 and B["poly_ms"] == 0 and (A["cut_ms"] > 0) == bool(modes) and (A["adapter_ms"] > 0) == bool(a)
            vc.compare_runs(pairs, pre, A, B, paired)
            want = poly_rule.poly_counts(se(pairs, paired), model)
            assert A["poly_stats"].tolist() == want and want[0] > len(pairs) // 10, (want, A["poly_stats"].tolist())       # more than a tenth of read 1 is cut
            # the earlier passes' own counts are what they are without the poly options
            assert A["cut_stats"].tolist() == (cut_rule.cut_counts(se(pairs, paired), model.adapter.cut) if modes else [0, 0, 0, 0])
            assert A["adapter_stats"].tolist() == (adapter_rule.adapter_counts(se(pairs, paired), model.adapter) if a else [0, 0, 0, 0])
            assert pre not in seen                                  # (each set of options does take part)
            seen.append(pre)
    finally:
        vc.set_passes(eng)


VERDICT_CASES = [(150, 10, True, (2, 3)), (150, 10, False, (0, 0)), (250, 16, True, (0, 0)), (250, 16, False, (2, 3)),
                 (280, 18, True, (2, 3)), (280, 18, False, (0, 0)), (310, 20, True, (0, 0)), (310, 20, False, (2, 3)),
                 (321, 0, True, (2, 3)), (321, 0, False, (0, 0))]


@pytest.mark.parametrize("L,words,paired,trim", VERDICT_CASES)
def test_verdicts_equal_a_run_on_precut_records(L, words, paired, trim, gpu_engine):
    """every tier and the general kernel"""
    check_against_precut(gpu_engine, poly_pairs(700, L, 1900 + L + int(paired)), paired, trim, words)


# ---- records the pass leaves under 5 bases ---------------------------------------------------------------------------------------
def sub5_pairs(n=400, L=150, seed=5):
    """even records: read 1 is G from its first 0 .. 4 bases on; odd: read 2; every fifth: both"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = [poly_rule.clean_read(rng, L, G), poly_rule.clean_read(rng, L, G)]
        for k in {i % 2} | ({1} if i % 5 == 0 else set()):
            s[k] = poly_rule.with_tail(s[k], L - rng.randint(0, 4), G)
        out.append((s[0], bytes(rng.randrange(33 + 25, 33 + 41) for _ in range(L)), s[1], bytes(rng.randrange(33 + 25, 33 + 41) for _ in range(L))))
    return out


def test_reads_trimmed_below_five_bases(gpu_engine):
    pairs = sub5_pairs()
    model = model_of((0, 0, 10, 0))
    A = run_pairs(gpu_engine, pairs, True, vc.base_config(True), None, None, pcfg((0, 0, 10, 0)), accum_limit=300)
    vc.check_below_five(pairs, A["res"], poly_rule, model)
    # records below accum_limit only, and read 2 is not counted where read 1 ended the record
    assert A["poly_stats"].tolist() == poly_rule.poly_counts(pairs, model, accum_limit=300)
    assert int(A["counters"][capi.C_FLAG0 + capi.BADTRIM1]) + int(A["counters"][capi.C_FLAG0 + capi.BADTRIM2]) == 300


def test_bad_file_text_of_reads_trimmed_below_five_bases(gpu_engine):
    """text in, text out: every record goes to the bad streams as @BADTRIM1... / @BADTRIM2..., read 1 trimmed, read 2 only under BADTRIM2"""
    pairs = sub5_pairs(300, 150, 6)
    model = model_of((0, 0, 10, 0))
    gpu_engine.set_config(vc.base_config(True))
    vc.set_passes(gpu_engine, poly=pcfg((0, 0, 10, 0)))
    try:
        got = vc.bad_streams(gpu_engine, pairs)
    finally:
        vc.set_passes(gpu_engine)
    assert got == vc.badtrim_text(pairs, poly_rule, model)


# ---- the counts ---------------------------------------------------------------------------------------------------------------
def test_poly_stats_over_two_contexts_with_a_cut_and_an_adapter_on(gpu_engine):
    pairs = adapter_rule.with_adapters(random.Random(3), poly_pairs(600, 150, 12), A1, A1, frac=0.15)
    modes, lens = (1, 1, 0), (10, 10, 8, 10)
    model = model_of(lens, modes, (0, 0), A1, A1)
    cfg, cut, ad = vc.base_config(True), vc.cutcfg(modes), capi.AdapterConfig(A1, A1, 4)
    other = capi.Engine(0, 2)
    try:
        a = run_pairs(gpu_engine, pairs[:350], True, cfg, cut, ad, pcfg(lens))
        b = run_pairs(other, pairs[350:], True, cfg, cut, ad, pcfg(lens))
        both = capi.MergedEngines([gpu_engine, other])
        merged = both.poly_stats().tolist()
        assert merged == poly_rule.poly_counts(pairs, model) and merged[0] > 50 and merged[2] > 50
        assert (a["poly_stats"] + b["poly_stats"]).tolist() == merged
        # the cut's and the adapter's counts of the same run: those of a run without the poly options
        c = run_pairs(gpu_engine, pairs[:350], True, cfg, cut, ad, None)
        d = run_pairs(other, pairs[350:], True, cfg, cut, ad, None)
        assert (a["cut_stats"] + b["cut_stats"]).tolist() == (c["cut_stats"] + d["cut_stats"]).tolist() == cut_rule.cut_counts(pairs, model.adapter.cut)
        assert (a["adapter_stats"] + b["adapter_stats"]).tolist() == (c["adapter_stats"] + d["adapter_stats"]).tolist() == adapter_rule.adapter_counts(pairs, model.adapter)
        assert (c["adapter_stats"] + d["adapter_stats"])[0] > 20
        assert c["poly_stats"].tolist() == [0, 0, 0, 0] and c["poly_ms"] == 0
        # an accum_limit
        e = run_pairs(gpu_engine, pairs, True, cfg, cut, ad, pcfg(lens), accum_limit=211)
        assert e["poly_stats"].tolist() == poly_rule.poly_counts(pairs, model, accum_limit=211)
        gpu_engine.reset_stats()
        assert gpu_engine.poly_stats().tolist() == [0, 0, 0, 0]
    finally:
        other.close()
        vc.set_passes(gpu_engine)


# ---- off is off -------------------------------------------------------------------------------------------------------------
def test_off_after_a_poly_run_is_the_run_without_it(gpu_engine):
    pairs = poly_pairs(1200, 150, 44)
    cfg = vc.base_config(True, (2, 3))
    fresh = capi.Engine(0, 2)
    try:
        want = vc.run_pairs(fresh, pairs, True, cfg, None, None)       # a context that never had the pass
        assert fresh.poly_ms(0) == 0 and fresh.poly_stats().tolist() == [0, 0, 0, 0]
    finally:
        fresh.close()
    on = run_pairs(gpu_engine, pairs, True, cfg, None, None, pcfg((0, 0, 10, 0)))
    assert on["poly_ms"] > 0 and on["res"].tobytes() != want["res"].tobytes()
    gpu_engine.set_poly_trim(pcfg((0, 0, 10, 0)))
    gpu_engine.set_poly_trim(None)                                     # taken away again through NULL, the same slot
    got = vc.run_pairs(gpu_engine, pairs, True, cfg, None, None)
    assert got["res"].tobytes() == want["res"].tobytes()
    assert np.array_equal(got["counters"], want["counters"]) and np.array_equal(got["ovl"], want["ovl"]) and np.array_equal(got["dist"], want["dist"])
    assert gpu_engine.poly_ms(0) == 0 and got["adapter_ms"] == 0 and got["cut_ms"] == 0 and got["words"] == want["words"] == 10
    assert gpu_engine.poly_stats().tolist() == [0, 0, 0, 0]


def test_barcode_with_the_pass_on_is_unsupported(gpu_engine):
    pairs = vc.tailed_pairs(64, 150, 3)
    cfg = vc.base_config(True)
    cfg.barcode = 1
    with pytest.raises(capi.AqcError) as e:
        run_pairs(gpu_engine, pairs, True, cfg, None, None, pcfg((0, 0, 10, 0)))
    assert e.value.code == ERR_UNSUPPORTED


# ---- a child process: AQC_FORCE_GENERIC=1 -----------------------------------------------------------------------------------------
def child_generic():
    """the general kernel alone decides 150-base pairs with the pass on, without and with a cut and an adapter"""
    eng = capi.Engine(0, 2)
    check_against_precut(eng, poly_pairs(600, 150, 71), True, (2, 3), 0)
    print(json.dumps({"ok": True}))


def test_general_kernel_alone_in_a_child_process():
    assert vc.run_child(__file__, "generic", {"AQC_FORCE_GENERIC": "1"}) == {"ok": True}


# ---- end to end -------------------------------------------------------------------------------------------------------------
def e2e_pairs(n, L, seed):
    """poly pairs with one record whose quality line is longer than its sequence line"""
    pairs = poly_pairs(n, L, seed)
    s1, q1, s2, q2 = pairs[9]
    pairs[9] = (s1, q1 + bytes([33 + 30]) * 11, s2, q2)
    return pairs


G_ON, X_ON = ["--trim_poly_g", "on"], ["--trim_poly_x", "on"]
E2E_CASES = {
    # name: (paired, input compression, argv with the options, argv of the pre-cut run, driver, index files)
    # (plain, .gz and .bz2 input, single-end and paired, through each of the two drivers: the first twelve cases)
    "pipe_se": (False, "", G_ON, [], "pipe_small_chunks", False),
    "pipe_se_gz": (False, ".gz", X_ON, [], "pipe_small_chunks", False),
    "pipe_se_bz2": (False, ".bz2", G_ON + ["--poly_g_min_len", "15"], [], "pipe_small_chunks", False),
    "pipe_pe": (True, "", G_ON, [], "pipe_small_chunks", False),
    "pipe_pe_gz": (True, ".gz", G_ON + X_ON + ["--poly_g_min_len", "6", "--poly_x_min_len", "20"], [], "pipe_small_chunks", False),
    "pipe_pe_bz2_no_overlap": (True, ".bz2", G_ON + ["--no_overlap"], ["--no_overlap"], "pipe_small_chunks", False),
    "text_se": (False, "", G_ON, [], "text", False),
    "text_se_gz": (False, ".gz", G_ON + ["--poly_g_min_len", "12"], [], "text", False),
    "text_se_bz2": (False, ".bz2", X_ON + ["--poly_x_min_len", "12"], [], "text", False),
    "text_pe": (True, "", X_ON, [], "text", False),
    "text_pe_gz": (True, ".gz", G_ON, [], "text", False),
    "text_pe_bz2": (True, ".bz2", G_ON + X_ON + ["--poly_g_min_len", "30"], [], "text", False),
    "pipe_two_contexts_merged": (True, "", G_ON + ["--store_merged", "on"], ["--store_merged", "on"], "pipe_two_contexts", False),
    "text_pe_cut_adapter": (True, "", G_ON + ["--cut_tail", "on", "--adapter_sequence", A1.decode()], [], "text", False),
    "text_pe_index": (True, "", G_ON, [], "text", True),
    "text_pe_qc_only": (True, "", G_ON + ["--qc_only", "--qc_sample", "300"], ["--qc_only", "--qc_sample", "300"], "text", False),
}


def opt_of(argv, key, default):
    return argv[argv.index(key) + 1] if key in argv else default


@pytest.mark.parametrize("name", sorted(E2E_CASES))
def test_cli_equals_a_run_on_precut_files(name, tmp_path, gpu_engine):
    paired, gz, argv_on, argv_pre, driver, index = E2E_CASES[name]
    trim = (2, 3) if name in ("text_se_gz", "pipe_pe_gz") else (0, 0)
    on_g, on_x = "--trim_poly_g" in argv_on, "--trim_poly_x" in argv_on
    g_len, x_len = int(opt_of(argv_on, "--poly_g_min_len", 10)), int(opt_of(argv_on, "--poly_x_min_len", 10))
    with_cut = "--cut_tail" in argv_on
    a = A1 if with_cut else b""
    model = poly_rule.PolyConfig.from_options(on_g, on_x, g_len, x_len, model_of((0, 0, 0, 0), (0, 1, 0) if with_cut else None, trim, a, a).adapter)
    pairs = e2e_pairs(900, 150, 700 + len(name))
    if with_cut:
        pairs = adapter_rule.with_adapters(random.Random(8), pairs, A1, A1, frac=0.15)
    pre = poly_rule.precut_pairs(pairs, model, paired)
    assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
    assert any(len(p[0]) != len(p[1]) for p in pairs)
    kw = vc.driver_kw(driver)
    work = [os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")]
    fa = vc.write_inputs(work[0], "raw", pairs, paired, gz, index)
    fb = vc.write_inputs(work[1], "pre", [p if paired else (p[0], p[1], b"", b"") for p in pre], paired, gz, index)
    try:
        sa, pipe_a = vc.run_cli(work[0], fa, paired, ["-f", str(trim[0]), "-t", str(trim[1])] + argv_on, kw, gpu_engine, index)
        sb, pipe_b = vc.run_cli(work[1], fb, paired, ["-f", "0", "-t", "0"] + argv_pre, kw, gpu_engine, index)
        # the driver the case names is the driver that ran: no quiet fall-back to the serial loop with the option on
        assert pipe_a == pipe_b == name.startswith("pipe_"), (pipe_a, pipe_b)
        oa, ob = vc.read_outputs(work[0]), vc.read_outputs(work[1])
        assert sorted(oa) == sorted(ob)
        if "--qc_only" in argv_on:
            assert not oa
        else:
            assert any(k.startswith("good/") and oa[k] for k in oa) and any(k.startswith("bad/") for k in oa)
        if "--store_merged" in argv_on:
            assert any(k.startswith("merged/") and oa[k] for k in oa)
        for k in oa:
            assert oa[k] == ob[k], k
        # the statistics: every key the run without the options has, but what sees the raw reads — total_bases, the pre-filter QC
        # sections and readlen — the echo of the options, and the objects of the trim stage's own options
        assert "poly_trim" in sa and "poly_trim" not in sb
        counted = sb["afterqc_main_summary"]["total_reads"] if "--qc_only" in argv_on else None
        assert counted is None or 300 <= counted < len(pairs)
        want = poly_rule.poly_counts(se(pairs, paired), model, accum_limit=counted)
        pt = sa["poly_trim"]
        assert [pt["read1_trimmed_reads"], pt["read1_trimmed_bases"], pt["read2_trimmed_reads"], pt["read2_trimmed_bases"]] == want
        assert want[0] > (20 if counted else 50) and (not paired or want[2] > (20 if counted else 50))
        assert (pt["trim_poly_g"], pt["poly_g_min_len"], pt["trim_poly_x"], pt["poly_x_min_len"]) == (on_g, g_len, on_x, x_len)
        if with_cut:
            # the same bytes as the same run without the poly options
            assert argv_on[:2] == G_ON
            argv_c = argv_on[2:]
            sc, _ = vc.run_cli(os.path.join(str(tmp_path), "c"), fa, paired, ["-f", str(trim[0]), "-t", str(trim[1])] + argv_c, kw, gpu_engine, index)
            for key in ("quality_cut", "adapter_trim"):
                assert json.dumps(sa[key], sort_keys=True) == json.dumps(sc[key], sort_keys=True)
            assert sa["quality_cut"]["read1_cut_reads"] > 100 and sa["adapter_trim"]["read1_trimmed_reads"] > 20
            assert "poly_trim" not in sc
        assert sorted(k for k in sa if k not in ("poly_trim", "adapter_trim", "quality_cut")) == sorted(sb)
        vc.compare_cli_stats(sa, sb)
    finally:
        vc.set_passes(gpu_engine)


def test_cli_refuses_barcoded_input(tmp_path, gpu_engine):
    pairs = vc.tailed_pairs(64, 150, 3)
    files = vc.write_inputs(str(tmp_path), "raw", pairs, True, "")
    options, _ = after.parseCommand(["-1", files[0], "-2", files[1], "-g", os.path.join(str(tmp_path), "good"), "--trim_poly_x", "on"])
    after.finalize_options(options)
    options.barcode = True
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(options, engine=gpu_engine).run()
    assert "barcode" in str(e.value) and "trim_poly_x" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "good"))


if __name__ == "__main__":
    {"generic": child_generic}[sys.argv[1]]()
