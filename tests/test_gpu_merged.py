"""--store_merged on the GPU (-m gpu): the device writer's merged-read pass (aqc_format in mode AQC_STORE_MERGED, fmt_merged_kernel).

Engine level: pairs made from a known insert F — r1 = F[:len1], r2 = revcomp(F[-len2:]), no errors — are framed, judged and
formatted; stream [0][2] must be the rule of tests/merged_rule.py applied to the device's own good streams and verdicts, the merged
sequence of such a pair must be F itself, and the number of merged pairs is the number built to merge.  Then the whole CLI on the
fixture cases (tests/golden/merged_cases.json.gz, derived from the reference's outputs): device writer, host writer and fixture agree;
the pipe with two contexts and small chunks; gzip output; the opt-in writers in child processes; index files."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import merged_rule
import test_host_golden as thg
from afterqc_amd import capi
from test_merged_host import MERGED_ON, TABLE, check_merged_file, merged_argv, merged_path, run_merged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_VALUES = [0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 119, 219]
N_VALUES = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def merged_fixture():
    return merged_rule.load_fixture()


def revcomp(s):
    return merged_rule.reverse_complement(s)


def quals(rng, n):
    """phred 20 .. 39, no two neighbours alike: a quality line that is misplaced or not reversed does not compare equal"""
    steps = rng.integers(1, 20, n)
    return "".join(chr(53 + int(x)) for x in np.cumsum(steps) % 20)


def make_pair(rng, len1, len2, p, inside=False, tail_mix=False):
    """-> (r1, r2, F): the mates of an insert F of len1 + p bases (read 2's last len2 - p ... bases overlap read 1); inside: read 2
    lies inside read 1 (p == 0, F == r1); tail_mix: lower case and N in the part of F that only read 2 covers"""
    bases = np.array(list("ACGT"))
    F = "".join(bases[rng.integers(0, 4, len1 + p)])
    if tail_mix and p >= 8:
        t = list(F[len1:])
        for k in range(0, len(t), 3):
            t[k] = t[k].lower()
        t[1] = "N"
        if p > 40:
            t[p // 2] = "N"
        F = F[:len1] + "".join(t)
    if inside:
        a = (len1 - len2) // 2
        return F[:len1], revcomp(F[a:a + len2]), F[:len1]
    assert len2 >= p
    return F[:len1], revcomp(F[-len2:]), F


def unrelated_pair(rng, len1, len2):
    bases = np.array(list("ACGT"))
    return "".join(bases[rng.integers(0, 4, len1)]), "".join(bases[rng.integers(0, 4, len2)])


class Pairs:
    """FASTQ text of both files, and per pair what it was built as"""

    def __init__(self):
        self.t1, self.t2, self.want_merged, self.insert = [], [], [], []

    def add(self, rng, r1, r2, merged, insert=None, q1=None, q2=None):
        i = len(self.t1)
        # name lines of 1 .. 17 bytes, the two files out of step: source and destination stand at every offset mod 16
        n1 = "@" + "abcdefghijklmnopq"[:i % 17]
        n2 = "@" + "ABCDEFGHIJKLMNOPQ"[:(i // 3) % 17]
        self.t1.append("%s\n%s\n+\n%s\n" % (n1, r1, q1 if q1 is not None else quals(rng, len(r1))))
        self.t2.append("%s\n%s\n+\n%s\n" % (n2, r2, q2 if q2 is not None else quals(rng, len(r2))))
        self.want_merged.append(merged)
        self.insert.append(insert)

    def __len__(self):
        return len(self.t1)


def base_config():
    cfg = capi.Config()
    cfg.paired = 1
    cfg.seq_len_req = 35
    cfg.poly_size_limit = 35
    cfg.allow_mismatch_in_poly = 2
    cfg.qualified_quality_phred = 15
    cfg.unqualified_base_limit = 60
    cfg.n_base_limit = 5
    cfg.qc_kmer = 8
    return cfg


def frame_and_run(eng, pairs, slot=0):
    text1, text2 = "".join(pairs.t1).encode(), "".join(pairs.t2).encode()
    eng.set_config(base_config())
    eng.reset_stats()
    pad = lambda b: np.frombuffer(b + b"\0" * 4096, dtype=np.uint8).copy()
    info = eng.frame(slot, pad(text1), len(text1), True, pad(text2), len(text2), True)
    assert int(info.n) == len(pairs)
    eng.run(slot)
    eng.sync(slot)
    return eng.fetch_results(slot)


def fetch(eng, slot, sizes, file, stream):
    nb = sizes[file * 3 + stream]
    buf = np.zeros(max(nb, 1), dtype=np.uint8)
    if nb:
        eng.fetch_text(slot, file, stream, buf, nb)
    return buf[:nb].tobytes().decode("latin-1")


def selected(res):
    """the pairs upstream writes to the overlap files (preprocesser.py:614): good, overlap_len > 30, every mismatch corrected"""
    out = []
    for r in res:
        corrected = sum(1 for k in range(int(r["n_edits"])) if int(r["edits"][k]["kind"]) in (capi.EDIT_FIX_R1, capi.EDIT_FIX_R2))
        out.append(int(r["flag"]) == capi.GOOD and int(r["overlap_len"]) > 30 and int(r["distance"]) in (0, corrected))
    return out


def expected_streams(res, n, good1, good2):
    """the rule on the device's good streams and verdicts of records [0, n) -> (merged text, overlap text 1, overlap text 2, merged flags per pair)"""
    g1, g2 = merged_rule.records(good1), merged_rule.records(good2)
    sel = selected(res[:n])
    merged, o1, o2, flags = [], [], [], []
    k = 0
    for i in range(n):
        if int(res[i]["flag"]) != capi.GOOD:
            flags.append(False)
            continue
        a, b = g1[k], g2[k]
        k += 1
        rec = None
        if sel[i]:
            ovl = int(res[i]["overlap_len"])
            rec = merged_rule.merged_record(a[0], a[1], a[2], a[3], b[1], b[3], ovl)
            # getOverlap (preprocesser.py:78-84): the last overlap_len characters of each line
            o1.append("%s\n%s\n%s\n%s\n" % (a[0], a[1][len(a[1]) - ovl:], a[2], a[3][len(a[3]) - ovl:]))
            o2.append("%s\n%s\n%s\n%s\n" % (b[0], b[1][len(b[1]) - ovl:], b[2], b[3][len(b[3]) - ovl:]))
        if rec is not None:
            merged.append(rec)
        flags.append(rec is not None)
    assert k == len(g1) == len(g2)
    return "".join(merged), "".join(o1), "".join(o2), flags


def check_format(eng, res, pairs, n, slot=0):
    sizes = eng.format(slot, n, capi.STORE_MERGED)
    assert sizes[5] == 0, "stream [1][2] is not empty"
    good1, good2 = fetch(eng, slot, sizes, 0, 0), fetch(eng, slot, sizes, 1, 0)
    got = fetch(eng, slot, sizes, 0, 2)
    want, _, _, flags = expected_streams(res, n, good1, good2)
    assert flags == pairs.want_merged[:n], [i for i in range(n) if flags[i] != pairs.want_merged[i]][:10]
    assert len(got) == len(want) and got == want, first_difference(got, want)
    # built from a known insert without errors: the merged sequence IS the insert
    recs = merged_rule.records(got)
    inserts = [pairs.insert[i] for i in range(n) if flags[i]]
    assert len(recs) == len(inserts)
    for rec, F in zip(recs, inserts):
        if F is not None:
            assert rec[1] == F, (rec[0], rec[1], F)
            assert len(rec[3]) == len(F)
    return sizes, got


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d: got %r, want %r" % (len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40])


def mixed_set(seed, n, length, p_values):
    """n pairs of `length` bases: two of three built to merge (p cycling through p_values), every third one unrelated (not merged: good,
    or bad for its N bases)"""
    rng = np.random.default_rng(seed)
    ps = Pairs()
    for i in range(n):
        if i % 3 == 2:
            r1, r2 = unrelated_pair(rng, length, length)
            if (i // 3) % 2:
                r1 = "N" * 10 + r1[10:]             # a bad pair (BADNCT) between the good ones
            ps.add(rng, r1, r2, False)
            continue
        p = p_values[(i // 3 * 2 + i % 3) % len(p_values)]
        assert length - p > 30, "the overlap must be long enough to merge"
        r1, r2, F = make_pair(rng, length, length, p, tail_mix=(i % 4 == 1))
        ps.add(rng, r1, r2, True, F)
    return ps


@pytest.fixture(scope="module")
def set150(gpu_engine):
    """2049 pairs of 2 x 150: every p up to 119 that leaves an overlap of more than 30, at every name-line length"""
    ps = mixed_set(11, 2049, 150, [p for p in P_VALUES if p <= 119])
    res = frame_and_run(gpu_engine, ps, slot=2)
    return ps, res


@pytest.mark.parametrize("n", N_VALUES)
def test_record_counts_and_tails(n, gpu_engine, set150):
    ps, res = set150
    sizes, got = check_format(gpu_engine, res, ps, n, slot=2)
    assert (sizes[2] > 0) == any(ps.want_merged[:n])


def test_every_p_is_present(set150):
    ps, res = set150
    seen = {len(F) - 150 for F, m in zip(ps.insert, ps.want_merged) if m}
    assert seen == {p for p in P_VALUES if p <= 119}


def test_overlap_modes_unchanged(gpu_engine, set150):
    """format(slot, n, True) and format(slot, n, 1): the overlap tails of both files, as before"""
    ps, res = set150
    n = 1025
    out = []
    for mode in (True, 1):
        sizes = gpu_engine.format(2, n, mode)
        good1, good2 = fetch(gpu_engine, 2, sizes, 0, 0), fetch(gpu_engine, 2, sizes, 1, 0)
        _, o1, o2, _ = expected_streams(res, n, good1, good2)
        got1, got2 = fetch(gpu_engine, 2, sizes, 0, 2), fetch(gpu_engine, 2, sizes, 1, 2)
        assert got1 == o1 and got2 == o2 and len(o1) > 0
        out.append((sizes, got1, got2))
    assert out[0] == out[1]
    sizes0 = gpu_engine.format(2, n, 0)
    assert sizes0[2] == 0 and sizes0[5] == 0 and sizes0[:2] == out[0][0][:2]


@pytest.mark.parametrize("length", [300, 330], ids=["2x300_tier20", "2x330_general"])
def test_long_pairs(length, gpu_engine):
    ps = mixed_set(length, 200, length, P_VALUES)
    assert {len(F) - length for F, m in zip(ps.insert, ps.want_merged) if m} >= {0, 16, 49, 119, 219}
    res = frame_and_run(gpu_engine, ps)
    check_format(gpu_engine, res, ps, len(ps))


def test_mates_of_different_lengths_and_read2_inside_read1(gpu_engine):
    rng = np.random.default_rng(5)
    ps = Pairs()
    for i in range(300):
        kind = i % 4
        if kind == 0:
            r1, r2, F = make_pair(rng, 150, 120, P_VALUES[i // 4 % 14])            # len2 < len1
        elif kind == 1:
            r1, r2, F = make_pair(rng, 110, 150, [0, 3, 17, 33, 64, 100][i // 4 % 6])      # len2 > len1
        elif kind == 2:
            r1, r2, F = make_pair(rng, 150, 60 + i % 50, 0, inside=True)            # read 2 inside read 1: p == 0
        else:
            r1, r2 = unrelated_pair(rng, 140, 90)
            ps.add(rng, r1, r2, False)
            continue
        ps.add(rng, r1, r2, True, F)
    res = frame_and_run(gpu_engine, ps)
    check_format(gpu_engine, res, ps, len(ps))


def test_all_merged_and_none_merged(gpu_engine):
    rng = np.random.default_rng(6)
    ps = Pairs()
    for i in range(200):
        r1, r2, F = make_pair(rng, 150, 150, P_VALUES[i % 15])
        ps.add(rng, r1, r2, True, F)
    res = frame_and_run(gpu_engine, ps)
    sizes, got = check_format(gpu_engine, res, ps, len(ps))
    assert got.count("\n") == 4 * 200
    ps = Pairs()
    for i in range(200):
        r1, r2 = unrelated_pair(rng, 150, 150)
        ps.add(rng, r1, r2, False)
    res = frame_and_run(gpu_engine, ps)
    sizes, got = check_format(gpu_engine, res, ps, len(ps))
    assert sizes[2] == 0 and sizes[5] == 0 and got == ""


def test_one_irregular_pair_is_left_out(gpu_engine):
    """a quality line two characters short in read 1 of one pair, in read 2 of another: no merged read for them, their neighbours intact"""
    rng = np.random.default_rng(8)
    ps = Pairs()
    for i in range(140):
        r1, r2, F = make_pair(rng, 150, 150, P_VALUES[i % 15])
        if i == 70:
            ps.add(rng, r1, r2, False, None, q1=quals(rng, 148))
        elif i == 100:
            ps.add(rng, r1, r2, False, None, q2=quals(rng, 148))
        else:
            ps.add(rng, r1, r2, True, F)
    res = frame_and_run(gpu_engine, ps)
    sel = selected(res)
    assert sel[70] and sel[100], "the irregular pairs are not among the overlap stream's pairs: the case is vacuous"
    sizes, got = check_format(gpu_engine, res, ps, len(ps))
    assert got.count("\n") == 4 * 138


# ---- the whole CLI on the fixture cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TABLE))
def test_three_way_agreement(name, tmp_path, merged_fixture, gpu_engine):
    """device writer (serial text loop), host writer, fixture"""
    (tmp_path / "text").mkdir()
    (tmp_path / "host").mkdir()
    info = {}
    work, _ = run_merged(name, tmp_path / "text", gpu_engine, "text", info)
    assert info["text_path"] and not info["used_pipe"]
    check_merged_file(name, work, merged_fixture)
    work2, _ = run_merged(name, tmp_path / "host", gpu_engine, "host", info)
    assert not info["text_path"]
    check_merged_file(name, work2, merged_fixture)
    assert merged_rule.read_maybe_gz(merged_path(work, name)) == merged_rule.read_maybe_gz(merged_path(work2, name))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_pipe_two_contexts_small_chunks(name, tmp_path, merged_fixture, e2e, gpu_engine):
    """aqc_pipe_run, two contexts on one device, chunks of 300 records: merged reads on both sides of every chunk border"""
    info = {}
    work, stat = run_merged(name, tmp_path, gpu_engine, "pipe_two_contexts", info)
    assert info["used_pipe"], info
    check_merged_file(name, work, merged_fixture)
    if name in e2e and "--store_overlap" not in TABLE[name][1]:
        thg.check_case(name, work, stat, e2e)          # good / bad files, statistics: as without the option


@pytest.mark.parametrize("level", [2, 9])
def test_pipe_gzip_output(level, tmp_path, merged_fixture, gpu_engine):
    name = "pe_store_overlap"
    info = {}
    work, _ = run_merged(name, tmp_path, gpu_engine, "pipe_small_chunks", info, argv=merged_argv(name) + ["-z", "--compression", str(level)])
    assert info["used_pipe"], info
    with gzip.open(os.path.join(work, "merged", "R1.merged.fq.gz"), "rb") as f:
        got = merged_rule.digest_bytes(f.read())
    assert got == {k: merged_fixture[name][k] for k in ("sha256", "lines", "bytes")}


@pytest.mark.parametrize("env", [{"AQC_SPANS": "1"}, {"AQC_FUSED": "1"}], ids=["spans", "fused"])
def test_opt_in_writers_in_a_child_process(env, tmp_path, merged_fixture):
    import cases
    name = "pe_store_overlap"
    work = str(tmp_path)
    cases.materialize(TABLE[name][2], work)
    kw = dict(use_text_path=True, use_pipe=True, chunk_records=211, pipe_slots=3)
    child_env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests", "golden")]), **env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "merged_rule.py"), work, json.dumps(kw)] + merged_argv(name),
                       env=child_env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "used_pipe=1" in p.stdout, p.stdout[-2000:]
    check_merged_file(name, work, merged_fixture)


def test_index_files_get_no_merged_stream(tmp_path, e2e, gpu_engine):
    """pe_index's input with the option on: the merged reads of the same run without index files, the index outputs unchanged"""
    name = "pe_index"
    _, argv, spec, _ = thg.CASE_TABLE[name]
    outs = {}
    for tag, av in (("with", list(argv) + MERGED_ON), ("without", [a for a in argv if a not in ("-7", "I1.fq", "-5", "I2.fq")] + MERGED_ON)):
        (tmp_path / tag).mkdir()
        key = "merged:" + name + tag
        thg.CASE_TABLE[key] = (key, av, spec, False)
        try:
            work, stat = thg.run_case(key, tmp_path / tag, gpu_engine, "text")
        finally:
            del thg.CASE_TABLE[key]
        assert os.listdir(os.path.join(work, "merged")) == ["R1.merged.fq"]
        with open(os.path.join(work, "merged", "R1.merged.fq"), "rb") as f:
            outs[tag] = f.read()
        if tag == "with":
            thg.check_case(name, work, stat, e2e)      # good / bad files of R1, R2, I1, I2 and the statistics
    assert outs["with"] == outs["without"] and outs["with"].count(b"\n") >= 4 * 50
