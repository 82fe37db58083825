"""--adapter_sequence auto on the GPU: the census kernel (adapter_census_kernel, csrc/aqc_adpcensus.hpp) at its function seam against
the model of tests/detect_rule.py, one batch per group size and probe set; the windows, accumulation, the two files' counts side by
side, the refusals and a too-long read; then the CLI through the whole-input pipe and the serial text loop, against the same build
with the sequences given on the command line, and a file that holds no adapter against a run with no option at all."""
import os
import random
import threading

import pytest

import detect_rule
import viewpass_cases as vc
from afterqc_amd import capi, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_READ_TOO_LONG, ERR_STATE = capi.ERR_ARG, -3, -5
R1, R2 = capi.QC_R1_PRE, capi.QC_R2_PRE
TRUSEQ1, TRUSEQ2 = detect_rule.CANDIDATES[0][1], detect_rule.CANDIDATES[0][2]
NEXTERA = detect_rule.CANDIDATES[1][1]
# the lengths of each group size's batch (viewpass_cases.GROUP_LENGTHS), and with the smallest group every read of 0 .. 13 bases
SEAM_LENGTHS = {G: sorted(set(L) | (set(range(0, 14)) if G == 8 else set())) for G, L in vc.GROUP_LENGTHS.items()}


def quals(reads):
    return [b"I" * len(s) for s in reads]


def census(eng, which, reads, probes, slot=0, windows=None):
    """probes set (the counts start at zero), the reads uploaded, the windows censused -> the counts"""
    eng.set_adapter_probes(which, probes)
    eng.upload(slot, vc.pack(reads, quals(reads)))
    for first, count in windows if windows is not None else [(0, len(reads))]:
        eng.adapter_census(slot, which, 0, first, count)
    eng.sync(slot)
    return eng.adapter_census_counts(which).tolist()


def padded(counts):
    return counts + [0] * (1 + capi.ADP_MAX_PROBES - len(counts))


# ---- the seam against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sorted(SEAM_LENGTHS))
@pytest.mark.parametrize("k", sorted(detect_rule.PROBE_SETS))
def test_seam_against_the_model(k, G, gpu_engine):
    """adapter_census_kernel<8>, <16>, <32> and <64>, each with 1, 4 and 16 probes (some sharing their first 4, 8 and 11 bytes):
    the probe at every place mod 16, across every lane border, at the read's ends and one place too far, N and lower case in
    it, twice, two in one read, reads of 0 .. 13 bases"""
    probes, reads = detect_rule.seam_case(SEAM_LENGTHS[G], k, 5300 + 7 * k + G)
    batch = vc.pack(reads, quals(reads))
    assert vc.GROUP_RANGE[G][0] <= batch.max_len() <= vc.GROUP_RANGE[G][1]
    want = detect_rule.census(reads, probes)
    assert all(0 < c < len(reads) for c in want[1:]), want                      # every probe is held somewhere, none everywhere
    assert census(gpu_engine, R1, reads, probes) == padded(want)
    assert gpu_engine.adapter_census_ms(0) > 0.0
    # read by read: which probe is wrong where, should the totals ever differ
    if k == 4:
        for i in range(0, len(reads), 97):
            assert census(gpu_engine, R1, reads, probes, windows=[(i, 1)]) == padded(detect_rule.census(reads[i:i + 1], probes)), (G, i, len(reads[i]))


def test_windows_accumulation_and_reset(gpu_engine):
    """first / count that cut the batch at group and workgroup borders (32 reads per workgroup and round with 8 lanes per read),
    calls that add up, and the two ways back to zero"""
    probes, reads = detect_rule.seam_case([40, 128, 64, 12, 100], 4, 77)
    reads = (reads * 8)[:1500]
    n = len(reads)
    assert n == 1500
    for first, count in [(0, n), (0, 0), (n, 0), (0, 1), (1, 31), (31, 2), (32, 32), (33, 64), (255, 257), (n - 1, 1), (5, n - 5), (7, 1024)]:
        assert census(gpu_engine, R1, reads, probes, windows=[(first, count)]) == padded(detect_rule.census(reads[first:first + count], probes)), (first, count)
    wins = [(0, 100), (50, 300), (1400, 100), (0, n)]
    want = [sum(v) for v in zip(*(detect_rule.census(reads[a:a + c], probes) for a, c in wins))]
    assert census(gpu_engine, R1, reads, probes, windows=wins) == padded(want) and want[0] == 2000
    gpu_engine.adapter_census(0, R1, 0, 0, 10)                                  # a further call, later: on top
    gpu_engine.sync(0)
    more = detect_rule.census(reads[:10], probes)
    assert gpu_engine.adapter_census_counts(R1).tolist() == padded([a + b for a, b in zip(want, more)])
    gpu_engine.reset_stats()
    assert gpu_engine.adapter_census_counts(R1).tolist() == [0] * (1 + capi.ADP_MAX_PROBES)
    gpu_engine.adapter_census(0, R1, 0, 0, 10)                                  # (the probes stay set)
    gpu_engine.sync(0)
    assert gpu_engine.adapter_census_counts(R1).tolist() == padded(more)
    gpu_engine.set_adapter_probes(R1, probes)
    assert gpu_engine.adapter_census_counts(R1).tolist() == [0] * (1 + capi.ADP_MAX_PROBES)


def test_both_files_side_by_side_and_read_2_of_a_pair(gpu_engine):
    """the counts are per file: slots 0 and 1 censused from two threads at once, as pass 1 samples a pair; and mate 1 of a paired slot"""
    pa, ra = detect_rule.seam_case([150, 33, 12], 4, 81)
    pb, rb = detect_rule.seam_case([250, 129], 16, 82)
    gpu_engine.set_adapter_probes(R1, pa)
    gpu_engine.set_adapter_probes(R2, pb)
    gpu_engine.upload(0, vc.pack(ra, quals(ra)))
    gpu_engine.upload(1, vc.pack(rb, quals(rb)))
    errors = []

    def side():
        try:
            for _ in range(5):
                gpu_engine.adapter_census(1, R2, 0, 0, len(rb))
                gpu_engine.sync(1)
        except BaseException as e:      # re-raised on the main thread
            errors.append(e)
    t = threading.Thread(target=side)
    t.start()
    for _ in range(5):
        gpu_engine.adapter_census(0, R1, 0, 0, len(ra))
        gpu_engine.sync(0)
    t.join()
    assert not errors, errors
    assert gpu_engine.adapter_census_counts(R1).tolist() == padded([5 * v for v in detect_rule.census(ra, pa)])
    assert gpu_engine.adapter_census_counts(R2).tolist() == padded([5 * v for v in detect_rule.census(rb, pb)])
    # a paired slot: read 2's lines into read 2's counts, read 1's untouched
    m = min(len(ra), len(rb))
    gpu_engine.set_adapter_probes(R1, pb)
    gpu_engine.set_adapter_probes(R2, pb)
    gpu_engine.upload(0, vc.pack(ra[:m], quals(ra[:m]), rb[:m], quals(rb[:m])))
    gpu_engine.adapter_census(0, R2, 1, 3, m - 3)
    gpu_engine.sync(0)
    assert gpu_engine.adapter_census_counts(R2).tolist() == padded(detect_rule.census(rb[3:m], pb))
    assert gpu_engine.adapter_census_counts(R1).tolist() == [0] * (1 + capi.ADP_MAX_PROBES)


def test_refusals_and_a_too_long_read(gpu_engine):
    rng = random.Random(3)
    ok = detect_rule.make_probes(rng, 17)
    for bad in ([], ok, [ok[0][:5] + b"N" + ok[0][6:]], [ok[0].lower()], ok[:15] + [ok[15][:11] + b"U"]):
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.set_adapter_probes(R1, bad)
        assert e.value.code == ERR_ARG
    for which in (capi.QC_R1_POST, capi.QC_R2_POST, -1, 4):
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.set_adapter_probes(which, ok[:4])
        assert e.value.code == ERR_ARG
    reads = [detect_rule.plant(detect_rule.bases(rng, 60), 20, ok[0]) for _ in range(8)]
    gpu_engine.upload(0, vc.pack(reads, quals(reads)))
    gpu_engine.set_adapter_probes(R1, None)                                     # off: a census is a call out of order
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.adapter_census(0, R1, 0, 0, 8)
    assert e.value.code == ERR_STATE
    gpu_engine.set_adapter_probes(R1, ok[:1])
    for args in ((0, capi.QC_R1_POST, 0, 0, 8), (0, R1, 2, 0, 8), (0, R1, 1, 0, 8), (0, R1, 0, 0, 9), (0, R1, 0, 9, 0), (0, R1, 0, 1, capi.UINT64_MAX)):
        with pytest.raises(capi.AqcError) as e:
            gpu_engine.adapter_census(*args)
        assert e.value.code == ERR_ARG, args
    assert gpu_engine.adapter_census_counts(R1).tolist() == [0] * (1 + capi.ADP_MAX_PROBES)
    # a line longer than AQC_MAX_READ_LEN: raised at the slot's next wait, as the view passes do; it is looked at and holds nothing
    long_read = detect_rule.plant(detect_rule.bases(rng, 1001), 500, ok[0])
    gpu_engine.upload(0, vc.pack(reads + [long_read], quals(reads + [long_read])))
    gpu_engine.adapter_census(0, R1, 0, 0, 9)
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.sync(0)
    assert e.value.code == ERR_READ_TOO_LONG
    assert gpu_engine.adapter_census_counts(R1).tolist() == padded([9, 8])


# ---- end to end -------------------------------------------------------------------------------------------------------------
def synth_pairs(n, L, seed, short_frac):
    d = synth.make_pairs(n, L, seed=seed, short_frac=short_frac)
    return [(d["seq1"][i].tobytes(), d["qual1"][i].tobytes(), d["seq2"][i].tobytes(), d["qual2"][i].tobytes()) for i in range(n)]


def cli(tmp_path, tag, files, paired, argv, driver, engine):
    work = os.path.join(str(tmp_path), tag)
    stat, used_pipe = vc.run_cli(work, files, paired, ["-f", "0", "-t", "0"] + argv, vc.driver_kw(driver), engine)
    assert used_pipe == driver.startswith("pipe")
    return stat, vc.read_outputs(work)


def same_but(sa, sb, *keys):
    """two runs' statistics but for the named objects and the echo of the output folder"""
    a, b = ({k: v for k, v in s.items() if k not in keys and k != "command"} for s in (sa, sb))
    ca, cb = ({k: v for k, v in s["command"].items() if k != "good_output_folder"} for s in (sa, sb))
    return a == b and ca == cb


@pytest.fixture
def cli_engine(gpu_engine):
    """the session's engine, left as a run without the options leaves it"""
    yield gpu_engine
    gpu_engine.set_adapter_trim(None)
    for which in (R1, R2):
        gpu_engine.set_adapter_probes(which, None)


E2E = [("pipe_small_chunks", False), ("pipe_small_chunks", True), ("text", False), ("text", True), ("pipe_two_contexts", True)]


@pytest.mark.parametrize("driver,paired", E2E)
def test_cli_auto_equals_the_sequences_given(driver, paired, tmp_path, cli_engine):
    """4 000 reads of the generator with its adapters (TruSeq read-through in a fifth of them): auto finds both mates' adapters
    in the sample and the run is the run with the two sequences on the command line"""
    pairs = synth_pairs(4000, 150, 640 + len(driver) + paired, 0.2)
    files = vc.write_inputs(os.path.join(str(tmp_path), "in"), "raw", pairs, paired, "")
    given = ["--adapter_sequence", TRUSEQ1.decode()] + (["--adapter_sequence_r2", TRUSEQ2.decode()] if paired else [])
    sa, oa = cli(tmp_path, "auto", files, paired, ["--adapter_sequence", "auto"], driver, cli_engine)
    sb, ob = cli(tmp_path, "given", files, paired, given, driver, cli_engine)
    assert sorted(oa) == sorted(ob) and any(k.startswith("good/") and oa[k] for k in oa) and any(k.startswith("bad/") for k in oa)
    for k in oa:
        assert oa[k] == ob[k], k
    assert sa["adapter_trim"] == sb["adapter_trim"] and sa["adapter_trim"]["read1_trimmed_reads"] > 400
    assert (sa["adapter_trim"]["adapter_sequence"], sa["adapter_trim"]["adapter_sequence_r2"]) == (TRUSEQ1.decode(), TRUSEQ2.decode() if paired else "")
    assert "adapter_detect" not in sb and same_but(sa, sb, "adapter_detect")
    det = sa["adapter_detect"]
    assert sorted(det) == ["min_per_mille", "min_reads", "probe_len"] + ["read1"] + (["read2"] if paired else [])
    for mate in range(2 if paired else 1):
        # (pass 1 skips the file's first 999 reads: 1000 or more follow them)
        assert det["read%d" % (mate + 1)] == detect_rule.detect([p[2 * mate] for p in pairs[999:]], mate)
        assert det["read%d" % (mate + 1)]["detected"] == "illumina_truseq" and det["read%d" % (mate + 1)]["sampled"] == 3001


def test_cli_finds_nextera_in_a_single_end_file(tmp_path, cli_engine):
    rng = random.Random(9)
    pairs = [(detect_rule.plant(s1, rng.randrange(40, 138), NEXTERA) if rng.random() < 0.05 else s1, q1, s2, q2)
             for s1, q1, s2, q2 in synth_pairs(4000, 150, 650, 0.0)]
    files = vc.write_inputs(os.path.join(str(tmp_path), "in"), "raw", pairs, False, "")
    sa, oa = cli(tmp_path, "auto", files, False, ["--adapter_sequence", "auto"], "pipe_small_chunks", cli_engine)
    sb, ob = cli(tmp_path, "given", files, False, ["--adapter_sequence", NEXTERA.decode()], "pipe_small_chunks", cli_engine)
    assert oa == ob and sa["adapter_trim"] == sb["adapter_trim"] and sa["adapter_trim"]["read1_trimmed_reads"] > 100
    assert same_but(sa, sb, "adapter_detect")
    assert sa["adapter_detect"]["read1"] == detect_rule.detect([p[0] for p in pairs[999:]], 0)
    assert sa["adapter_detect"]["read1"]["detected"] == "nextera" and sa["adapter_detect"]["read1"]["adapter"] == NEXTERA.decode()


@pytest.mark.parametrize("driver,paired", [("pipe_small_chunks", True), ("text", False)])
def test_cli_nothing_planted_is_a_run_without_the_option(driver, paired, tmp_path):
    """no adapter in the file: the bytes of a run with no option at all, no kernel of the adapter pass — and without auto no
    census either (an engine of this test's own: a slot remembers its last census)"""
    pairs = synth_pairs(4000, 150, 660 + paired, 0.0)
    files = vc.write_inputs(os.path.join(str(tmp_path), "in"), "raw", pairs, paired, "")
    eng = capi.Engine(0, 3)
    try:
        sb, ob = cli(tmp_path, "off", files, paired, [], driver, eng)
        assert [eng.adapter_census_ms(s) for s in range(3)] == [0.0] * 3        # off is off
        sa, oa = cli(tmp_path, "auto", files, paired, ["--adapter_sequence", "auto"], driver, eng)
        assert eng.adapter_census_ms(0) > 0.0 and (eng.adapter_census_ms(1) > 0.0) == paired
        assert [eng.adapter_ms(s) for s in range(3)] == [0.0] * 3               # nothing found: no adapter pass
    finally:
        eng.close()
    assert oa == ob and any(k.startswith("good/") and oa[k] for k in oa)
    assert "adapter_trim" not in sa and "adapter_detect" not in sb and same_but(sa, sb, "adapter_detect")
    for mate in range(2 if paired else 1):
        rep = sa["adapter_detect"]["read%d" % (mate + 1)]
        assert rep == detect_rule.detect([p[2 * mate] for p in pairs[999:]], mate)
        assert (rep["detected"], rep["adapter"], rep["sampled"]) == (None, "", 3001) and max(c for _, c in rep["candidates"]) < 10
