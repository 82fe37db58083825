"""Finding a mate's adapter in the pass-1 sample (--adapter_sequence auto) on the CPU: the model of tests/detect_rule.py against a
brute-force restatement and the decision at its edges; the candidate table; the CLI's options (auto in each option, mixed and
inherited, the --adapter_min_overlap bound, every refusal); the driver on an oracle engine that answers the census from the model
(nothing detected: the run of no option plus "adapter_detect"; TruSeq planted: the resolved adapter reaches set_adapter_trim; the
pass-1 window; an engine without the census); the new symbols; and the per-read functions of the device census
(csrc/aqc_adpcensus.hpp) as a stand-alone C++ program on vectors the model writes, plain and under ASan / UBSan
(tests/native/adpcensus_selftest.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import detect_rule
from afterqc_amd import adapter_detect, after, capi, preprocesser, synth
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUSEQ1, TRUSEQ2 = detect_rule.CANDIDATES[0][1], detect_rule.CANDIDATES[0][2]
NEXTERA = detect_rule.CANDIDATES[1][1]
LENGTHS = list(range(0, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 999, 1000]


# ---- the model -------------------------------------------------------------------------------------------------------
def test_model_against_brute_force():
    rng = random.Random(20171)
    probes = detect_rule.make_probes(rng, 16, share=((0, 1, 4), (2, 3, 8)))
    assert probes[0][:4] == probes[1][:4] and probes[0][4] != probes[1][4]
    assert probes[2][:8] == probes[3][:8] and probes[2][8] != probes[3][8]
    n_cases = n_held = 0
    tags = set()
    for n in LENGTHS:
        for j, (tag, s) in enumerate(detect_rule.placements(rng, n, probes)):
            if n > 300 and j % 9 and tag.startswith("at_"):
                continue                                                        # (a long read's hundreds of places: one in nine)
            for p in probes:
                want = detect_rule.holds_brute(s, p)
                assert detect_rule.holds(s, p) == want == (p in s), (tag, n, s, p)
                n_held += want
            n_cases += 1
            tags.add(re.sub(r"\d+", "", tag))
    assert n_cases > 1500 and n_held > n_cases // 2
    assert tags == {"clean", "prefix", "at_", "cut_", "N_", "lower_", "twice", "two", "overlapping"}


def test_named_placements_give_what_their_names_say():
    """on a read that holds no probe by chance the expected answer is known without the model"""
    rng = random.Random(6)
    probes = detect_rule.make_probes(rng, 4)
    P = probes[0]
    for n in (12, 13, 40, 129, 1000):
        base = detect_rule.clean_read(rng, n, probes)
        assert detect_rule.census([base], probes) == [1, 0, 0, 0, 0]
        for p in sorted({0, 1, 5, n - 13, n - 12} & set(range(0, n - 11))):
            assert detect_rule.holds(detect_rule.plant(base, p, P), P)
        assert not detect_rule.holds(detect_rule.plant(base, n - 11, P), P)                 # 11 of its 12 bytes at the tail
        for b in (0, 5, 11):
            r = detect_rule.plant(base, 0, P)
            assert not detect_rule.holds(detect_rule.spoil(r, b, "N"), P) and not detect_rule.holds(detect_rule.spoil(r, b, "l"), P)
    for n in range(0, 12):
        assert not detect_rule.holds(P[:n], P)                                              # a read under 12 bases holds nothing
    twice = detect_rule.plant(detect_rule.plant(detect_rule.clean_read(rng, 60, probes), 0, P), 30, P)
    both = detect_rule.plant(twice, 30, probes[1])
    assert detect_rule.census([twice, both], probes) == [2, 2, 1, 0, 0]                     # twice counts once; a read may count for two


def test_gpu_seam_batches_hold_every_probe_somewhere_and_nowhere_everywhere():
    """the batches of tests/test_gpu_adapter_census.py, checked here: a count of 0 or of the batch size could not tell a census
    that looks from one that does not"""
    import viewpass_cases as vc
    for G, lengths in vc.GROUP_LENGTHS.items():
        lengths = sorted(set(lengths) | (set(range(0, 14)) if G == 8 else set()))
        for k in detect_rule.PROBE_SETS:
            probes, reads = detect_rule.seam_case(lengths, k, 5300 + 7 * k + G)
            want = detect_rule.census(reads, probes)
            assert want[0] == len(reads) > 100 and all(0 < c < len(reads) for c in want[1:]), (G, k, want)
            assert vc.GROUP_RANGE[G][0] <= max(len(s) for s in reads) <= vc.GROUP_RANGE[G][1]


DECISIONS = [
    # counts, S -> row
    ([9, 0, 0, 0], 100, None), ([10, 0, 0, 0], 100, 0),                                     # 9 / 10 reads
    ([10, 0, 0, 0], 10000, 0), ([10, 0, 0, 0], 10001, None),                                # 10 * 1000 against S
    ([0, 0, 199, 0], 199000, 2), ([0, 0, 199, 0], 199001, None),
    ([12, 12, 0, 0], 100, 0), ([0, 12, 0, 12], 100, 1), ([3, 12, 12, 5], 100, 1),           # a tie goes to the earlier row
    ([11, 12, 0, 0], 100, 1),
    ([0, 0, 0, 0], 100, None), ([0, 0, 0, 0], 0, None), ([], 0, None),                      # nothing counted, nothing sampled
    ([10, 0, 0, 0], 10, 0),                                                                 # every sampled read holds it
]


@pytest.mark.parametrize("case", range(len(DECISIONS)))
def test_decision_edges(case):
    counts, sampled, want = DECISIONS[case]
    assert detect_rule.decide(counts, sampled) == want
    assert detect_rule.decide_brute(counts, sampled) == want
    assert adapter_detect.decide(counts, sampled) == want


def test_decision_against_brute_force():
    rng = random.Random(7)
    for _ in range(20000):
        counts = [rng.choice([0, 9, 10, 11, rng.randrange(0, 300)]) for _ in range(rng.randrange(1, 6))]
        sampled = rng.choice([0, 1, max(counts), 1000 * max(counts), 1000 * max(counts) + 1, rng.randrange(0, 400000)])
        want = detect_rule.decide_brute(counts, sampled)
        assert detect_rule.decide(counts, sampled) == want == adapter_detect.decide(counts, sampled)


# ---- the table -------------------------------------------------------------------------------------------------------
def test_candidate_table():
    assert (detect_rule.PROBE_LEN, detect_rule.MIN_READS, detect_rule.MIN_PER_MILLE) == (12, 10, 1)
    assert [r[0] for r in detect_rule.CANDIDATES] == ["illumina_truseq", "nextera", "illumina_small_rna", "bgi_mgi"]
    assert len(detect_rule.CANDIDATES) <= detect_rule.MAX_PROBES
    for mate in (0, 1):
        for a in detect_rule.column(mate):
            assert 12 <= len(a) <= 64 and not set(a) - set(b"ACGT")
        assert len(set(detect_rule.probes(mate))) == len(detect_rule.CANDIDATES)
    # the first two rows are the adapters the generator and the adapter tests plant
    assert TRUSEQ1 == synth.ADAPTER1.tobytes() and TRUSEQ2 == synth.ADAPTER2.tobytes()
    assert NEXTERA == b"CTGTCTCTTATACACATCT"
    # the run's copy says the same
    assert [(n, a.encode(), b.encode()) for n, a, b in adapter_detect.CANDIDATES] == detect_rule.CANDIDATES
    assert (adapter_detect.PROBE_LEN, adapter_detect.MIN_READS, adapter_detect.MIN_PER_MILLE) == (12, 10, 1)
    assert [adapter_detect.probes(m) for m in (0, 1)] == [detect_rule.probes(m) for m in (0, 1)]
    assert (capi.ADP_PROBE_LEN, capi.ADP_MAX_PROBES) == (detect_rule.PROBE_LEN, detect_rule.MAX_PROBES)


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def parse(argv):
    options, _ = after.parseCommand(["-1", "r_R1.fq"] + argv)
    return after.finalize_options(options)


def test_cli_auto_parses():
    opt = parse(["--adapter_sequence", "auto"])                                 # single-end: read 2 takes no part
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == ("auto", "auto")
    assert preprocesser.adapter_auto(opt) == (True, False) and preprocesser.adapter_config(opt) is None
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence", "AUTO"])                # read 2 inherits: its own detection
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == ("auto", "auto")
    assert preprocesser.adapter_auto(opt) == (True, True) and preprocesser.adapter_config(opt) is None
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence", "Auto", "--adapter_sequence_r2", "ttgca"])
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == ("auto", "TTGCA")
    assert preprocesser.adapter_auto(opt) == (True, False)
    assert preprocesser.adapter_config(opt).adapters() == (b"", b"TTGCA")       # until the sample is seen read 1 is not searched
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence", "ACGTACGT", "--adapter_sequence_r2", "auto"])
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == ("ACGTACGT", "auto")
    assert preprocesser.adapter_auto(opt) == (False, True)
    assert preprocesser.adapter_config(opt).adapters() == (b"ACGTACGT", b"")
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence_r2", "auto"])             # given alone: only read 2 is looked at
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == (None, "auto")
    assert preprocesser.adapter_auto(opt) == (False, True) and preprocesser.adapter_config(opt) is None
    # what was found takes the place of `auto`, and of nothing else
    assert preprocesser.adapter_config(opt, ("AAAA", "CCCC")).adapters() == (b"", b"CCCC")
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence", "auto", "--adapter_sequence_r2", "TTGCA"])
    assert preprocesser.adapter_config(opt, ("AAAA", "CCCC")).adapters() == (b"AAAA", b"TTGCA")
    # nothing else changes meaning
    assert parse([]).adapter_sequence is None
    assert parse(["--adapter_sequence", "acgta"]).adapter_sequence == "ACGTA"


def test_cli_min_overlap_bound_with_auto():
    shortest = min(len(a) for a in detect_rule.column(0))
    assert shortest == min(len(a) for a in detect_rule.column(1)) == 19
    assert parse(["--adapter_sequence", "auto", "--adapter_min_overlap", "19"]).adapter_min_overlap == 19
    assert parse(["-2", "r_R2.fq", "--adapter_sequence", "auto", "--adapter_min_overlap", "19"]).adapter_min_overlap == 19
    # an explicit mate keeps its own length
    assert parse(["-2", "r_R2.fq", "--adapter_sequence", "auto", "--adapter_sequence_r2", "ACGTACGT", "--adapter_min_overlap", "8"]).adapter_min_overlap == 8
    assert parse(["-2", "r_R2.fq", "--adapter_sequence", "A" * 30, "--adapter_sequence_r2", "auto", "--adapter_min_overlap", "19"]).adapter_min_overlap == 19
    # single-end: read 2's takes no part
    assert parse(["--adapter_sequence", "auto", "--adapter_sequence_r2", "ACGTA", "--adapter_min_overlap", "19"]).adapter_min_overlap == 19


@pytest.mark.parametrize("argv,word", [
    (["--adapter_sequence", "auto", "--adapter_min_overlap", "20"], "outside"),
    (["--adapter_sequence", "auto", "--adapter_min_overlap", "0"], "outside"),
    (["-2", "r_R2.fq", "--adapter_sequence_r2", "auto", "--adapter_min_overlap", "20"], "outside"),
    (["-2", "r_R2.fq", "--adapter_sequence", "auto", "--adapter_sequence_r2", "ACGTACGT", "--adapter_min_overlap", "9"], "outside"),
    (["-2", "r_R2.fq", "--adapter_sequence", "A" * 30, "--adapter_sequence_r2", "auto", "--adapter_min_overlap", "20"], "outside"),
    (["--adapter_sequence_r2", "auto"], "single-end"),                          # read 2's alone, and no read 2
    (["--adapter_sequence", "autos"], "letters"), (["--adapter_sequence", "aut"], "outside"),
])
def test_cli_refusals(argv, word):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert word in str(e.value) and "adapter" in str(e.value)


# ---- the driver on the CPU ---------------------------------------------------------------------------------------------
class CensusOracle(oracle.OracleEngine):
    """the oracle engine with the census answered from the model: what capi.Engine's four census calls do, on the slot's batch"""

    def __init__(self):
        self.census_probes = {}
        self.census_counts = {}
        self.census_calls = []
        super().__init__()

    def reset_stats(self):
        super().reset_stats()
        for which in self.census_counts:
            self.census_counts[which] = [0] * (1 + capi.ADP_MAX_PROBES)

    def set_adapter_probes(self, which, probes):
        self.census_probes[which] = None if probes is None else [bytes(p) for p in probes]
        self.census_counts[which] = [0] * (1 + capi.ADP_MAX_PROBES)

    def adapter_census(self, slot, which, mate, first, count):
        assert self.census_probes.get(which), "a census without probes"
        b = self.slots[slot]
        assert first + count <= b.n
        reads = [bytes((b.read2(i) if mate else b.read1(i))[0]) for i in range(first, first + count)]
        got = detect_rule.census(reads, self.census_probes[which])
        for k, v in enumerate(got):
            self.census_counts[which][k] += v
        self.census_calls.append((slot, which, mate, first, count))

    def adapter_census_counts(self, which):
        return np.array(self.census_counts[which], dtype=np.int64)


def write_fastq(path, reads):
    with open(path, "wb") as f:
        f.write(b"".join(b"@SIM:1:FC1:1:1101:%d:%d 1:N:0:ACGT\n%s\n+\n%s\n" % (1000 + i, 2000 + i, s, b"I" * len(s)) for i, s in enumerate(reads)))


def make_reads(n, L, seed, planted=0.0, adapter=TRUSEQ1):
    """n reads of L random bases that hold no probe of column 1; the adapter from a random place on in a fraction of them"""
    rng = random.Random(seed)
    probes = detect_rule.probes(0)
    out = []
    for i in range(n):
        s = detect_rule.clean_read(rng, L, probes)
        if rng.random() < planted:
            s = detect_rule.plant(s, rng.randrange(36, L - 12), adapter)
        out.append(s)
    return out


def job(work, reads, argv, barcode=False):
    os.makedirs(work, exist_ok=True)
    p = os.path.join(work, "s_R1.fq")
    write_fastq(p, reads)
    options, _ = after.parseCommand(["-1", p, "-f", "0", "-t", "0", "-g", os.path.join(work, "good")] + argv)
    after.finalize_options(options)
    options.barcode = barcode
    return options


def outputs(work):
    out = {}
    for folder in ("good", "bad"):
        for f in sorted(os.listdir(os.path.join(work, folder))):
            with open(os.path.join(work, folder, f), "rb") as fh:
                out[folder + "/" + f] = fh.read()
    return out


def test_nothing_detected_is_a_run_without_the_option(tmp_path, capsys):
    reads = make_reads(3000, 60, seed=11)
    runs = []
    for tag, argv in (("off", []), ("auto", ["--adapter_sequence", "auto"])):
        work = os.path.join(str(tmp_path), tag)
        opt = job(work, reads, ["--qc_sample", "1500"] + argv)
        eng = CensusOracle()
        flt = preprocesser.seqFilter(opt, engine=eng, use_text_path=False)
        stat = flt.run()
        runs.append((stat, outputs(work), eng, flt))
    (s_off, o_off, e_off, _), (s_auto, o_auto, e_auto, f_auto) = runs
    assert e_off.census_calls == [] and e_off.census_probes == {}               # off is off: nothing of the census is called
    assert o_auto == o_off and sum(len(v) for v in o_off.values()) > 3000 * 60
    det = s_auto.pop("adapter_detect")
    for s in (s_off, s_auto):                                                   # (the two runs' folders differ by name)
        for k in ("read1_file", "good_output_folder"):
            s["command"].pop(k)
    assert s_auto == s_off and "adapter_trim" not in s_auto
    assert f_auto.adapter is None
    # the window of pass 1: the reads behind the 999 skipped ones, qc_sample of them
    assert det == {"probe_len": 12, "min_reads": 10, "min_per_mille": 1,
                   "read1": {"sampled": 1500, "candidates": [[r[0], 0] for r in detect_rule.CANDIDATES], "detected": None, "adapter": ""}}
    assert [c[3:] for c in e_auto.census_calls] == [(999, 1500)] and e_auto.census_probes[capi.QC_R1_PRE] == detect_rule.probes(0)
    assert e_auto.census_probes[capi.QC_R2_PRE] is None
    assert "read 1 adapter not detected in 1500 sampled reads" in capsys.readouterr().out


def test_truseq_planted_reaches_the_adapter_pass(tmp_path, capsys):
    """5 % of the reads carry TruSeq: the census finds it, and pass 2 is configured with the table's sequence — which the
    oracle engine cannot run: the error it has always given for an adapter"""
    reads = make_reads(3000, 80, seed=12, planted=0.05)
    # (--qc_sample 0 has no upper end, but pass 1 still skips the file's first 999 reads when 1000 or more follow them)
    want = detect_rule.detect(reads[999:], 0)
    assert want["detected"] == "illumina_truseq" and 60 < want["candidates"][0][1] < 140
    opt = job(str(tmp_path), reads, ["--qc_sample", "0", "--adapter_sequence", "auto", "--adapter_min_overlap", "6"])
    flt = preprocesser.seqFilter(opt, engine=CensusOracle(), use_text_path=False)
    with pytest.raises(RuntimeError) as e:
        flt.run()
    assert "set_adapter_trim" in str(e.value)
    assert (flt.adapter.adapters(), flt.adapter.min_overlap) == ((TRUSEQ1, b""), 6)
    assert flt.adapter_detect["read1"] == want and want["sampled"] == 2001 and want["adapter"] == TRUSEQ1.decode()
    assert "read 1 adapter illumina_truseq %s" % TRUSEQ1.decode() in capsys.readouterr().out


def test_engine_without_the_census_is_an_error(tmp_path):
    opt = job(str(tmp_path), make_reads(64, 60, seed=13), ["--qc_sample", "0", "--adapter_sequence", "auto"])
    with pytest.raises(RuntimeError) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "adapter_census" in str(e.value)


def test_skipped_reads_are_sampled_too(tmp_path):
    """fewer than 1000 reads follow the 999 skipped ones: pass 1 stats those as well, and so does the census"""
    reads = make_reads(1500, 60, seed=14, planted=0.02, adapter=NEXTERA)
    opt = job(str(tmp_path), reads, ["--adapter_sequence", "auto"])
    eng = CensusOracle()
    flt = preprocesser.seqFilter(opt, engine=eng, use_text_path=False)
    with pytest.raises(RuntimeError):
        flt.run()                                                               # (Nextera found: the oracle cannot trim it)
    assert flt.adapter_detect["read1"] == detect_rule.detect(reads, 0)
    assert flt.adapter_detect["read1"]["sampled"] == 1500 and flt.adapter_detect["read1"]["detected"] == "nextera"
    assert [c[3:] for c in eng.census_calls] == [(999, 501), (0, 999)]


def test_barcode_with_auto_is_refused(tmp_path):
    opt = job(str(tmp_path), make_reads(64, 60, seed=15), ["--qc_sample", "0", "--adapter_sequence", "auto"], barcode=True)
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=CensusOracle(), use_text_path=False).run()
    assert "barcode" in str(e.value) and "adapter" in str(e.value)


def test_read_2_auto_alone_on_a_single_end_file_is_refused(tmp_path):
    """the folder mode pairs the files after the options are parsed: the run itself refuses, before anything is created"""
    opt = job(str(tmp_path), make_reads(64, 60, seed=16), ["--qc_sample", "0"])
    opt.adapter_sequence_r2 = "auto"
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=CensusOracle(), use_text_path=False).run()
    assert "adapter_sequence_r2" in str(e.value) and "single-end" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "good"))


# ---- the symbols -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["aqc_set_adapter_probes", "aqc_adapter_census", "aqc_get_adapter_census", "aqc_adapter_census_ms"]


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "afterqc_hip.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(aqc_ctx\*" % s, hdr), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
        assert getattr(capi.load_library(), s).restype is ctypes.c_int
    assert "#define AQC_ADP_PROBE_LEN 12" in hdr and "#define AQC_ADP_MAX_PROBES 16" in hdr
    assert "typedef struct aqc_adapter_probes { int32_t n; uint8_t seq[16][12]; } aqc_adapter_probes;" in hdr
    assert ctypes.sizeof(capi.AdapterProbes) == 4 + 16 * 12
    p = capi.AdapterProbes(["AGATCGGAAGAG", b"CTGTCTCTTATA"])
    assert (p.n, p.probes()) == (2, [b"AGATCGGAAGAG", b"CTGTCTCTTATA"])
    for name in ("set_adapter_probes", "adapter_census", "adapter_census_counts", "adapter_census_ms"):
        assert callable(getattr(capi.Engine, name))
    assert lib.aqc_abi_version() == 3                           # (new symbols only: no struct changed)


# ---- the device census's per-read functions, on the CPU --------------------------------------------------------------------
VECTOR_LENGTHS = [0, 1, 3, 11, 12, 13, 15, 16, 17, 27, 28, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 320, 321, 511, 512, 513, 999, 1000]


def write_vectors(path):
    rng = random.Random(979)
    n_sets = n_reads = n_held = 0
    with open(path, "w") as f:
        sets = [detect_rule.make_probes(rng, 1), detect_rule.make_probes(rng, 4, share=((0, 1, 4), (2, 3, 8))),
                detect_rule.make_probes(rng, 16, share=((0, 1, 4), (2, 3, 8), (4, 5, 11))), detect_rule.probes(0), detect_rule.probes(1)]
        for probes in sets:
            f.write("P %d %s\n" % (len(probes), " ".join(p.decode() for p in probes)))
            n_sets += 1
            for n in VECTOR_LENGTHS:
                for tag, s in detect_rule.placements(rng, n, probes):
                    mask = sum(1 << i for i, p in enumerate(probes) if detect_rule.holds(s, p))
                    f.write("R %d %s %d\n" % (n, s.hex() or "-", mask))
                    n_reads += 1
                    n_held += mask != 0
            # bytes that have a letter's code bits but are no letter: an N for a G, '@' and 'a' for an A, a 0x80 bit set
            for look, real in ((b"N", b"G"), (b"@", b"A"), (b"a", b"A"), (b"B", b"C"), (b"\xc3", b"C"), (b"t", b"T")):
                for i, p in enumerate(probes):
                    if real not in p:
                        continue
                    at = p.index(real)
                    s = detect_rule.plant(detect_rule.clean_read(rng, 40, probes), 7, p[:at] + look + p[at + 1:])
                    assert not detect_rule.holds(s, p)
                    f.write("R 40 %s %d\n" % (s.hex(), sum(1 << j for j, q in enumerate(probes) if detect_rule.holds(s, q))))
                    n_reads += 1
        ok = detect_rule.make_probes(rng, 17)
        bad = [[], ok, ok[:3] + [ok[3][:5] + b"N" + ok[3][6:]], [ok[0].lower()], ok[:15] + [ok[15][:11] + b"U"]]
        for probes in bad:
            f.write("B %d %s\n" % (len(probes), " ".join(p.decode() for p in probes)))
    return n_sets, n_reads, n_held, len(bad)


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the vector file, written once for both builds of the self-test"""
    path = str(tmp_path_factory.mktemp("census_vectors") / "vectors.txt")
    return (path,) + write_vectors(path)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_functions_on_the_cpu(tmp_path, flags, vectors):
    """csrc/aqc_adpcensus.hpp without HIP: groups of 8, 16, 32 and 64 lanes dealt out by loops over every length at which the
    pass changes its shape, every named placement and bytes that only look like letters to the code compare, against the model;
    once more as a stand-alone ASan / UBSan binary (each read is allocated with exactly the 15 bytes a lane's 16-byte load may
    take behind it, each row with exactly the kernel's words)"""
    exe = os.path.join(str(tmp_path), "adpcensus_selftest")
    vec, n_sets, n_reads, n_held, n_bad = vectors
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "adpcensus_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all census checks passed" in out.stdout, out.stdout[-3000:]
    assert "%d probe sets, %d reads," % (n_sets, n_reads) in out.stdout and "%d refusals checked" % n_bad in out.stdout
    assert n_reads > 5000 and n_held > n_reads // 2
