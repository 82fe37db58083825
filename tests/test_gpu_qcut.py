"""Per-read sliding-window quality cutting on the GPU (-m gpu): --cut_front / --cut_tail / --cut_right from the cut pass
(quality_cut_kernel, csrc/aqc_qcut.hpp) through the verdict kernels to the CLI, against the model of tests/cut_rule.py.

  seam        aqc_quality_cut_views against cut_window(), one batch per group size of the pass (8, 16, 32, 64 lanes per read): the
              lengths at which the pass changes shape, six windows, three qualities, the seven mode combinations, the named quality
              patterns at every length; irregular quality lines and fixed trims.
  verdicts    a run with the cut on against a run of the same build, cut and trim off, on precut(records): every tier of the
              lane-per-read kernel, paired and single-end, and the general kernel (reads of 321 bases; AQC_FORCE_GENERIC=1 in a child).
  below 5     records the cut leaves under 5 bases, against the model: BADTRIM1 with read 2 untouched, BADTRIM2, the bad files' text.
  counts      aqc_get_cut_stats against the model, with an accum_limit and over two contexts.
  end to end  the CLI through the whole-input pipe and the serial text loop against a run on pre-cut files with the options off.
  off is off  aqc_set_quality_cut(NULL) after a cut run gives what a context that never had the cut gives."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):       # (the child processes below run this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cut_rule
import viewpass_cases as vc
from afterqc_amd import capi
from viewpass_cases import (ERR_UNSUPPORTED, GROUP_LENGTHS, GROUP_RANGE, base_config, bases, compare_runs, cutcfg, driver_kw, pack, read_outputs,
                            run_cli, run_pairs, se, tailed_pairs, views, write_inputs)

pytestmark = pytest.mark.gpu

WINDOWS = [1, 4, 16, 17, 33, 1000]
QUALITIES = [0, 20, 93]


# ---- the seam against the model ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_lines():
    """per window and group size: the quality lines of every length of the group and every named pattern (one good window at every
    start 0 .. 33 and at n - w, at every length), shared by the cases"""
    out = {}
    for W in WINDOWS:
        for G, lengths in GROUP_LENGTHS.items():
            rng = random.Random(4100 + 7 * W + G)
            out[W, G] = [line for n in lengths for _, line in cut_rule.pattern_lines(n, W, rng)]
    return out


@pytest.mark.parametrize("G", sorted(GROUP_LENGTHS))
@pytest.mark.parametrize("W", WINDOWS)
def test_seam_against_the_model(W, G, gpu_engine, seam_lines):
    """regular quality lines, one batch per group size: quality_cut_kernel<8>, <16>, <32> and <64> each against the model"""
    lines = seam_lines[W, G]
    rng = random.Random(W)
    batch = pack([bases(rng, len(x)) for x in lines], lines)
    assert batch.qlen1 is None and GROUP_RANGE[G][0] <= batch.max_len() <= GROUP_RANGE[G][1]
    for Q in QUALITIES:
        for modes in cut_rule.MODES:
            got = views(*gpu_engine.quality_cut_views(batch, cutcfg(modes, W, Q)))
            want = [cut_rule.cut_window(x, W, Q, *modes) for x in lines]
            bad = [i for i in range(len(lines)) if got[i] != want[i]]
            assert not bad, (W, G, Q, modes, len(bad), [(len(lines[i]), got[i], want[i]) for i in bad[:5]])


@pytest.mark.parametrize("trim", [(0, 0), (3, 0), (0, 7), (200, 200)])
def test_seam_fixed_trim_and_irregular_lines(trim, gpu_engine):
    """150-base reads behind a fixed trim; quality lines shorter and longer than their sequence lines (qlen1): the view is that of
    the trimmed QUALITY line.  (A batch with quality lines of their own length always takes quality_cut_kernel<64>; the same trims
    on regular lines, which take <16>, are the second half.)"""
    rng = random.Random(77 + trim[0])
    seqs, quals = [], []
    for i in range(600):
        n = 150
        ql = n if i % 3 else rng.choice([0, 1, 4, 17, 100, 149, 151, 170, 400, 1000])
        seqs.append(bases(rng, n))
        quals.append(cut_rule.decaying_quality(rng, ql) if i % 2 else bytes(rng.randrange(33, 75) for _ in range(ql)))
    batch = pack(seqs, quals)
    assert batch.qlen1 is not None
    for modes in cut_rule.MODES:
        for W, Q in ((4, 20), (17, 25)):
            want = [cut_rule.cut_window(cut_rule.trim(x, *trim), W, Q, *modes) for x in quals]
            assert views(*gpu_engine.quality_cut_views(batch, cutcfg(modes, W, Q), trim[0], trim[1])) == want, (modes, W, Q)
    regular = [x[:150] + bytes([33 + 30]) * (150 - len(x)) for x in quals]
    batch = pack(seqs, regular)
    assert batch.qlen1 is None
    for modes in cut_rule.MODES:
        got = views(*gpu_engine.quality_cut_views(batch, cutcfg(modes, 4, 20), trim[0], trim[1]))
        assert got == [cut_rule.cut_window(cut_rule.trim(x, *trim), 4, 20, *modes) for x in regular], modes


def test_seam_refuses_bad_options(gpu_engine):
    batch = pack([b"ACGT"], [b"IIII"])
    for W, Q in ((0, 20), (1001, 20), (4, -1), (4, 94)):
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.quality_cut_views(batch, cutcfg((1, 0, 0), W, Q))
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.set_quality_cut(cutcfg((1, 0, 0), W, Q))
        assert e.value.code == capi.ERR_ARG
    gpu_engine.set_quality_cut(cutcfg((0, 0, 0), 0, -5))       # no mode set: off, whatever the rest says
    gpu_engine.set_quality_cut(None)


# ---- verdicts: the cut on against a run on the pre-cut records ------------------------------------------------------------------
def precut_pairs(pairs, cut, paired):
    out = []
    for s1, q1, s2, q2 in pairs:
        k1 = cut_rule.cut_lines(s1, q1, cut, 0)
        k2 = cut_rule.cut_lines(s2, q2, cut, 1) if paired else (None, None)
        out.append((k1[0], k1[1], k2[0], k2[1]))
    return out


VERDICT_CASES = [(150, 10, True, (0, 1, 0), (2, 3)), (150, 10, False, (1, 1, 1), (0, 0)), (250, 16, True, (1, 1, 0), (0, 0)), (250, 16, False, (0, 1, 0), (2, 3)),
                 (280, 18, True, (0, 0, 1), (2, 3)), (280, 18, False, (0, 1, 1), (0, 0)), (310, 20, True, (1, 1, 1), (2, 3)), (310, 20, False, (0, 1, 0), (0, 0)),
                 (321, 0, True, (0, 1, 0), (2, 3)), (321, 0, False, (1, 1, 1), (0, 0))]


@pytest.mark.parametrize("L,words,paired,modes,trim", VERDICT_CASES)
def test_verdicts_equal_a_run_on_precut_records(L, words, paired, modes, trim, gpu_engine):
    n = 1500
    short = set(range(7, n, 97))
    pairs = tailed_pairs(n, L, 900 + L + int(paired), short)
    model = cut_rule.CutConfig(*modes, window=4, mean_quality=20, trim_front=trim[0], trim_tail=trim[1])
    pre = precut_pairs(pairs, model, paired)
    assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
    A = run_pairs(gpu_engine, pairs, paired, base_config(paired, trim), cutcfg(modes))
    B = run_pairs(gpu_engine, pre, paired, base_config(paired), None)
    assert A["words"] == words
    assert A["cut_ms"] > 0 and B["cut_ms"] == 0
    compare_runs(pairs, pre, A, B, paired)
    assert A["cut_stats"].tolist() == cut_rule.cut_counts(se(pairs, paired), model)
    if words:
        # the fast path is kept: only a mate the cut leaves under 16 bases sends its record to the general kernel
        under16 = sum(1 for p in pre if len(p[0]) < 16 or (paired and len(p[2]) < 16))
        assert under16 >= len(short) - 1
        assert A["deferred"] <= B["deferred"] + under16
        assert A["deferred"] < n // 4


def test_irregular_mates_take_the_views_too(gpu_engine):
    """quality lines of their own length (LEN_IRR: the general kernel's): sequence and quality are each sliced by their own lengths,
    the final quality view comes back through aqc_fetch_quality_views — against a run on the pre-cut records, irregular as well"""
    rng = random.Random(31)
    pairs = tailed_pairs(300, 150, 31)
    for i in range(0, 300, 7):
        s1, q1, s2, q2 = pairs[i]
        # (longer than the sequence line: a shorter one ends the run at the overlap walk, as upstream's IndexError does)
        if i % 2:
            q1 = q1 + cut_rule.decaying_quality(rng, rng.randint(1, 30), good=38, knee=0)
        else:
            q2 = q2 + cut_rule.decaying_quality(rng, rng.randint(1, 30), good=38, knee=0)
        pairs[i] = (s1, q1, s2, q2)
    for modes in ((0, 1, 0), (1, 0, 1)):
        model = cut_rule.CutConfig(*modes, window=4, mean_quality=20, trim_front=2, trim_tail=3)
        pre = precut_pairs(pairs, model, True)
        assert any(len(p[0]) != len(p[1]) for p in pre) and any(len(p[2]) != len(p[3]) for p in pre)
        A = run_pairs(gpu_engine, pairs, True, base_config(True, (2, 3)), cutcfg(modes))
        B = run_pairs(gpu_engine, pre, True, base_config(True), None)
        assert A["words"] == 10 and A["deferred"] >= 43
        compare_runs(pairs, pre, A, B, True)
        assert A["cut_stats"].tolist() == cut_rule.cut_counts(pairs, model)


# ---- records the cut leaves under 5 bases ------------------------------------------------------------------------------------
def sub5_pairs(n=400, L=150, seed=5):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        knees = [rng.randint((6 * L) // 10, L), rng.randint((6 * L) // 10, L)]
        low = {i % 2} | ({1} if i % 5 == 0 else set())          # even records: read 1 goes under 5; odd: read 2; every fifth: both
        q = [cut_rule.decaying_quality(rng, L, good=40, floor=2, knee=k) for k in knees]
        for k in low:
            hi = rng.randint(0, 2)                              # phred 40 for 0 .. 2 bases, 2 behind them: the cut leaves 0 or 4 bases
            q[k] = bytes([33 + 40] * hi + [33 + 2] * (L - hi))
        out.append((bases(rng, L), q[0], bases(rng, L), q[1]))
    return out


def test_reads_cut_below_five_bases(gpu_engine):
    pairs = sub5_pairs()
    trim = (2, 3)
    model = cut_rule.CutConfig(0, 1, 0, window=4, mean_quality=20, trim_front=trim[0], trim_tail=trim[1])
    A = run_pairs(gpu_engine, pairs, True, base_config(True, trim), cutcfg((0, 1, 0)), accum_limit=300)
    gpu_engine.set_quality_cut(None)
    vc.check_below_five(pairs, A["res"], cut_rule, model)
    # records below accum_limit only, and read 2 is not counted where it was left as it is
    assert A["cut_stats"].tolist() == cut_rule.cut_counts(pairs, model, accum_limit=300)
    assert int(A["counters"][capi.C_FLAG0 + capi.BADTRIM1]) + int(A["counters"][capi.C_FLAG0 + capi.BADTRIM2]) == 300


def test_bad_file_text_of_reads_cut_below_five_bases(gpu_engine):
    """text in, text out: every record goes to the bad streams as @BADTRIM1... / @BADTRIM2..., read 1 cut, read 2 cut only under BADTRIM2"""
    pairs = sub5_pairs(300, 150, 6)
    model = cut_rule.CutConfig(0, 1, 0, window=4, mean_quality=20)
    gpu_engine.set_config(base_config(True))
    vc.set_passes(gpu_engine, cut=cutcfg((0, 1, 0)))
    try:
        got = vc.bad_streams(gpu_engine, pairs)
    finally:
        vc.set_passes(gpu_engine)
    assert got == vc.badtrim_text(pairs, cut_rule, model)


# ---- the counts over two contexts ---------------------------------------------------------------------------------------------
def test_cut_stats_add_up_over_two_contexts(gpu_engine):
    pairs = tailed_pairs(600, 150, 12)
    model = cut_rule.CutConfig(1, 1, 0, window=4, mean_quality=20)
    other = capi.Engine(0, 2)
    try:
        a = run_pairs(gpu_engine, pairs[:350], True, base_config(True), cutcfg((1, 1, 0)))
        b = run_pairs(other, pairs[350:], True, base_config(True), cutcfg((1, 1, 0)))
        merged = capi.MergedEngines([gpu_engine, other]).cut_stats()
        assert merged.tolist() == cut_rule.cut_counts(pairs, model)
        assert (a["cut_stats"] + b["cut_stats"]).tolist() == merged.tolist()
        gpu_engine.reset_stats()
        assert gpu_engine.cut_stats().tolist() == [0, 0, 0, 0]
    finally:
        other.close()
        gpu_engine.set_quality_cut(None)


# ---- off is off -------------------------------------------------------------------------------------------------------------
def test_off_after_a_cut_run_is_the_run_without_it(gpu_engine):
    pairs = tailed_pairs(1200, 150, 44)
    cfg = base_config(True, (2, 3))
    fresh = capi.Engine(0, 2)
    try:
        want = run_pairs(fresh, pairs, True, cfg, None)            # a context that never had the cut
    finally:
        fresh.close()
    run_pairs(gpu_engine, pairs, True, cfg, cutcfg((1, 1, 1)))
    got = run_pairs(gpu_engine, pairs, True, cfg, None)            # the same slot, the cut taken away again
    assert got["res"].tobytes() == want["res"].tobytes()
    assert np.array_equal(got["counters"], want["counters"]) and np.array_equal(got["ovl"], want["ovl"]) and np.array_equal(got["dist"], want["dist"])
    assert got["cut_ms"] == 0 and got["words"] == want["words"] == 10
    assert got["cut_stats"].tolist() == [0, 0, 0, 0]


def test_barcode_with_the_cut_is_unsupported(gpu_engine):
    pairs = tailed_pairs(64, 150, 3)
    cfg = base_config(True)
    cfg.barcode = 1
    with pytest.raises(capi.AqcError) as e:
        run_pairs(gpu_engine, pairs, True, cfg, cutcfg((0, 1, 0)))
    assert e.value.code == ERR_UNSUPPORTED
    gpu_engine.set_quality_cut(None)


# ---- child processes: AQC_FORCE_GENERIC=1, AQC_FUSED=1 ----------------------------------------------------------------------------
def child_generic():
    """the general kernel alone decides 150-base pairs with the cut on: equal to its run on the pre-cut pairs"""
    eng = capi.Engine(0, 2)
    pairs = tailed_pairs(800, 150, 71, set(range(3, 800, 50)))
    model = cut_rule.CutConfig(1, 1, 0, window=4, mean_quality=20, trim_front=2, trim_tail=3)
    pre = precut_pairs(pairs, model, True)
    A = run_pairs(eng, pairs, True, base_config(True, (2, 3)), cutcfg((1, 1, 0)))
    B = run_pairs(eng, pre, True, base_config(True), None)
    compare_runs(pairs, pre, A, B, True)
    assert A["cut_stats"].tolist() == cut_rule.cut_counts(pairs, model)
    print(json.dumps({"words": A["words"], "cut_ms_on": A["cut_ms"] > 0}))


def child_fused():
    """AQC_FUSED=1: with the cut on the verdict kernel never places the records itself; with the cut off again it does"""
    eng = capi.Engine(0, 2)
    pairs = tailed_pairs(512, 150, 72)
    out = []
    for cut in (cutcfg((0, 1, 0)), None):
        eng.set_config(base_config(True))
        eng.set_quality_cut(cut)
        eng.reset_stats()
        n = vc.frame_text(eng, 0, pairs)
        eng.run(0)
        eng.format(0, n, False)
        out.append((eng.format_fused(0), eng.cut_ms(0) > 0))
    print(json.dumps({"fused": out}))


def test_general_kernel_alone_in_a_child_process():
    assert vc.run_child(__file__, "generic", {"AQC_FORCE_GENERIC": "1"}) == {"words": 0, "cut_ms_on": True}


def test_fused_placement_is_back_with_the_cut_off_in_a_child_process():
    assert vc.run_child(__file__, "fused", {"AQC_FUSED": "1"}) == {"fused": [[0, True], [1, False]]}


# ---- end to end -------------------------------------------------------------------------------------------------------------
def e2e_pairs(n, L, seed):
    """tailed pairs with one irregular-quality record and one record whose cut leaves fewer than 16 bases (none under 5)"""
    pairs = tailed_pairs(n, L, seed, short={5, n // 2})
    s1, q1, s2, q2 = pairs[9]
    pairs[9] = (s1, q1 + bytes([33 + 3]) * 11, s2, q2)          # (a quality line longer than its sequence line)
    return pairs


E2E_CASES = {
    # name: (paired, input compression, argv with the cut, argv of the pre-cut run, model, driver, index files)
    "pipe_pe": (True, "", ["--cut_tail", "on"], [], dict(tail=1), "pipe_small_chunks", False),
    "pipe_se_gz": (False, ".gz", ["--cut_front", "on", "--cut_tail", "on"], [], dict(front=1, tail=1), "pipe_small_chunks", False),
    "pipe_two_contexts_merged": (True, "", ["--cut_tail", "on", "--store_merged", "on"], ["--store_merged", "on"], dict(tail=1), "pipe_two_contexts", False),
    "text_pe_gz_overlap": (True, ".gz", ["--cut_right", "on", "--store_overlap", "on"], ["--store_overlap", "on"], dict(right=1), "text", False),
    "text_se_trim": (False, "", ["--cut_tail", "on", "--cut_window_size", "5", "--cut_mean_quality", "22"], [], dict(tail=1, window=5, mean_quality=22), "text", False),
    "text_pe_index": (True, "", ["--cut_front", "on", "--cut_tail", "on", "--cut_right", "on"], [], dict(front=1, tail=1, right=1), "text", True),
    "pipe_pe_bz2": (True, ".bz2", ["--cut_tail", "on", "--cut_right", "on"], [], dict(tail=1, right=1), "pipe_small_chunks", False),
    "text_pe_debubble": (True, "", ["--cut_tail", "on", "--debubble"], ["--debubble"], dict(tail=1), "text", False),
    "text_pe_qc_only": (True, "", ["--cut_front", "on", "--cut_tail", "on", "--qc_only", "--qc_sample", "300"], ["--qc_only", "--qc_sample", "300"], dict(front=1, tail=1), "text", False),
}


@pytest.mark.parametrize("name", sorted(E2E_CASES))
def test_cli_equals_a_run_on_precut_files(name, tmp_path, gpu_engine):
    paired, gz, argv_cut, argv_pre, model_kw, driver, index = E2E_CASES[name]
    trim = (2, 3) if name in ("text_se_trim", "pipe_pe") else (0, 0)
    model = cut_rule.CutConfig(trim_front=trim[0], trim_tail=trim[1], **model_kw)
    pairs = e2e_pairs(900, 150, 300 + len(name))
    pre = precut_pairs(pairs, model, paired)
    assert min(len(p[0]) for p in pre) >= 5 and (not paired or min(len(p[2]) for p in pre) >= 5)
    assert any(len(p[0]) < 16 for p in pre) and any(len(p[0]) != len(p[1]) for p in pairs)
    kw = driver_kw(driver)
    work = [os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")]
    fa = write_inputs(work[0], "raw", pairs, paired, gz, index)
    fb = write_inputs(work[1], "pre", [p if paired else (p[0], p[1], b"", b"") for p in pre], paired, gz, index)
    extra = []
    if "--debubble" in argv_cut:
        # a circle around record 100's place on the tile (the names' x = 1000 + i, y = 2000 + i, lane 1, tile field 1101: upstream
        # drops the field's first character, preprocesser.py:187-192)
        with open(os.path.join(str(tmp_path), "circles.csv"), "w") as f:
            f.write("x,y,radius,lane,tile\n1100,2100,30,1,101\n")
        extra = ["--debubble_dir", str(tmp_path)]
    sa, pipe_a = run_cli(work[0], fa, paired, ["-f", str(trim[0]), "-t", str(trim[1])] + argv_cut + extra, kw, gpu_engine, index)
    sb, pipe_b = run_cli(work[1], fb, paired, ["-f", "0", "-t", "0"] + argv_pre + extra, kw, gpu_engine, index)
    # the driver the case names is the driver that ran: no quiet fall-back to the serial loop with the cut on
    assert pipe_a == pipe_b == name.startswith("pipe_"), (pipe_a, pipe_b)
    oa, ob = read_outputs(work[0]), read_outputs(work[1])
    assert sorted(oa) == sorted(ob)
    if "--qc_only" in argv_cut:
        assert not oa
    else:
        assert any(k.startswith("good/") for k in oa) and any(k.startswith("bad/") for k in oa)
    if "--debubble" in argv_cut:
        assert sa["afterqc_main_summary"]["bad_reads_with_reads_in_bubble"] >= 20
    if "--store_merged" in argv_cut:
        assert any(k.startswith("merged/") and oa[k] for k in oa)
    if "--store_overlap" in argv_cut:
        assert any(k.startswith("overlap/") and oa[k] for k in oa)
    for k in oa:
        assert oa[k] == ob[k], k
    # the statistics: every key the run without the options has, but what sees the raw reads — total_bases, the pre-filter QC
    # sections and readlen (the pre-filter sample's read length) — and the echo of the options
    assert "quality_cut" in sa and "quality_cut" not in sb
    # (--qc_only ends upstream's loop once the sample is full, preprocesser.py:630-631: the records the run without the options
    #  counted are the records the cut's counts cover)
    counted = sb["afterqc_main_summary"]["total_reads"] if "--qc_only" in argv_cut else None
    assert counted is None or 300 <= counted < len(pairs)
    want = cut_rule.cut_counts(se(pairs, paired), model, accum_limit=counted)
    qc = sa["quality_cut"]
    assert [qc["read1_cut_reads"], qc["read1_cut_bases"], qc["read2_cut_reads"], qc["read2_cut_bases"]] == want
    assert (qc["cut_front"], qc["cut_tail"], qc["cut_right"]) == (model.front, model.tail, model.right)
    assert (qc["cut_window_size"], qc["cut_mean_quality"]) == (model.window, model.mean_quality)
    assert sorted(k for k in sa if k != "quality_cut") == sorted(sb)
    vc.compare_cli_stats(sa, sb)


if __name__ == "__main__":
    {"generic": child_generic, "fused": child_fused}[sys.argv[1]]()
