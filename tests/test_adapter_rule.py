"""Trimming a given adapter from each read on the CPU: the model of tests/adapter_rule.py against a brute-force restatement over
the named placements and a list of edges worked out by hand; the CLI's options (defaults, read 2 inheriting, every refusal, an
engine that cannot trim adapters, the statistics JSON without the options); the new symbols; and the per-read functions of the
device pass (csrc/aqc_adapter.hpp) as a stand-alone C++ program on vectors the model writes, plain and under ASan / UBSan
(tests/native/adapter_selftest.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import adapter_rule
import cut_rule
from afterqc_amd import after, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = list(range(0, 71)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 999, 1000]
ADAPTER_LENGTHS = [4, 5, 8, 9, 16, 17, 33, 63, 64]


def ks_of(m):
    return sorted({1, 4, m})


# ---- the model -------------------------------------------------------------------------------------------------------
def model_cases(lengths=LENGTHS, adapter_lengths=ADAPTER_LENGTHS, seed=20170):
    """(read, adapter, K) over every read length, adapter length, K and named placement"""
    rng = random.Random(seed)
    for m in adapter_lengths:
        A = adapter_rule.make_adapter(rng, m)
        for K in ks_of(m):
            for n in lengths:
                for tag, s in adapter_rule.placements(n, A, K, rng):
                    yield tag, s, A, K


def test_model_against_brute_force():
    n_cases = n_hit = 0
    tags = set()
    for tag, s, A, K in model_cases():
        want = adapter_rule.adapter_find_brute(s, A, K)
        assert adapter_rule.adapter_find(s, A, K) == want, (tag, s, A, K)
        n_cases += 1
        n_hit += want is not None
        tags.add(re.sub(r"\d+", "", tag))
    assert n_cases > 100000 and n_hit > n_cases // 3 and n_cases - n_hit > n_cases // 20
    assert tags == {"clean", "random", "at_", "tail_", "mm__", "edge_", "N_", "lower_", "two"}


def test_named_placements_give_what_their_names_say():
    """the placements on a read that cannot match by chance: here the expected place is known without the model"""
    rng = random.Random(5)
    for m in ADAPTER_LENGTHS:
        A = adapter_rule.make_adapter(rng, m)
        for K in ks_of(m):
            for n in (70, 129, 1000):
                base = adapter_rule.clean_read(rng, n, A)
                assert adapter_rule.adapter_find(base, A, K) is None
                for p in list(range(0, 34)) + [n - m]:
                    # (behind n - K fewer than K bases of the adapter lie on the read: no match)
                    assert adapter_rule.adapter_find(adapter_rule.plant(base, p, A), A, K) == (p if p <= n - K else None)
                for k in range(K, m + 1):                       # the partial adapter at the tail
                    assert adapter_rule.adapter_find(adapter_rule.plant(base, n - k, A), A, K) == n - k
                if K > 1:                                       # one base fewer than K: no match
                    assert adapter_rule.adapter_find(adapter_rule.plant(base, n - K + 1, A), A, K) is None
                for k in (7, 8, 15, 16, 63, 64):                # k >> 3 mismatches pass, one more does not
                    if k > m or k < K:
                        continue
                    p = n - k if k < m else min(20, n - k)
                    r = adapter_rule.plant(base, p, A)
                    # (substituted from the comparison's end, its first byte stays: a place further on starts with a base of
                    #  the read's alphabet, which the adapter's first base is not in — and nothing under 8 bases forgives it)
                    ok = adapter_rule.substitute(rng, r, range(p + k - (k >> 3), p + k))
                    bad = adapter_rule.substitute(rng, r, range(p + k - (k >> 3) - 1, p + k))
                    assert adapter_rule.adapter_find(ok, A, K) == p, (m, K, n, k)
                    got = adapter_rule.adapter_find(bad, A, K)
                    assert got is None or got > p, (m, K, n, k)
                if n >= 2 * m + 3:
                    assert adapter_rule.adapter_find(adapter_rule.plant(adapter_rule.plant(base, n - m, A), 3, A), A, K) == 3


EDGES = [
    # read, adapter, K -> place
    (b"", b"ACGT", 1, None),                                    # an empty read
    (b"ACG", b"ACGT", 4, None),                                 # shorter than K
    (b"ACG", b"ACGT", 3, 0),                                    # ... K bases of the adapter are the whole read: a dimer's end
    (b"ACGT", b"ACGT", 4, 0),
    (b"TTACGT", b"ACGT", 4, 2),
    (b"TTACGA", b"ACGT", 4, None),                              # 4 compared bases forgive nothing
    (b"TTACGTAC", b"ACGTACGT", 4, 2),                           # 6 of 8 adapter bases at the tail
    (b"TTACGTACGA", b"ACGTACGT", 4, 2),                         # 8 compared: one mismatch allowed, in the last byte
    (b"TTTCGTACGT", b"ACGTACGT", 4, 2),                         # ... in the first byte
    (b"TTTCGTACGA", b"ACGTACGT", 4, None),                      # two are one too many
    (b"TTACGTACG", b"ACGTACGT", 4, 2),                          # 7 compared at the tail: none allowed
    (b"TTACGTACC", b"ACGTACGT", 4, None),
    (b"TTACNTACGT", b"ACGTACGT", 4, 2),                         # N is a mismatch like any other
    (b"TTACgTACGT", b"ACGTACGT", 4, 2),                         # so is a lower-case base ...
    (b"TTAcgTACGA", b"ACGTACGT", 4, None),                      # ... each of them
    (b"ACGTTTACGT", b"ACGT", 4, 0),                             # two places: the smaller
    (b"TTTTTTTTA", b"ACGT", 1, 8),                              # K = 1: the adapter's first base at the last place
    (b"TTTTTTTTA", b"ACGT", 2, None),
    (b"AAAAAAAAAA", b"ACGT", 1, 9),                             # only the last place compares a single base
]


@pytest.mark.parametrize("case", range(len(EDGES)))
def test_edges(case):
    s, A, K, want = EDGES[case]
    assert adapter_rule.adapter_find(s, A, K) == want
    assert adapter_rule.adapter_find_brute(s, A, K) == want


def q(*phreds):
    return bytes(33 + p for p in phreds)


def test_composition_with_an_incoming_view():
    A = b"ACGT"
    # no cut: everything, a match ends it
    assert adapter_rule.compose(adapter_rule.VIEW_ALL, b"TTTTTTACGTTT", A, 4) == (0, 6)
    assert adapter_rule.compose(adapter_rule.VIEW_ALL, b"TTTTTTTTTTTT", A, 4) == adapter_rule.VIEW_ALL
    # the search sees [c0:c1) only: the adapter lies behind c1 -> the view stays; inside -> (c0, c0 + p)
    assert adapter_rule.compose((2, 6), b"TTTTTTACGTTT", A, 4) == (2, 6)
    assert adapter_rule.compose((2, 9), b"TTTTTTACGTTT", A, 4) == (2, 9)          # three adapter bases in view, K = 4
    assert adapter_rule.compose((2, 9), b"TTTTTTACGTTT", A, 3) == (2, 6)
    assert adapter_rule.compose((2, 11), b"TTTTTTACGTTT", A, 4) == (2, 6)
    assert adapter_rule.compose((7, 12), b"ACGTTTTACGTT", A, 4) == (7, 7)         # a match at the view's start: nothing is kept
    # c0 beyond the sequence's end (a quality line longer than the sequence line): nothing to search, the view stays
    assert adapter_rule.compose((20, 30), b"TTTTTTACGTTT", A, 4) == (20, 30)
    # through the whole stage: fixed trim, the quality cut's view from the QUALITY line, each line sliced by its own length
    cut = cut_rule.CutConfig(front=1, tail=1, window=2, mean_quality=30, trim_front=1, trim_tail=1)
    cfg = adapter_rule.AdapterConfig(A, K=4, cut=cut)
    rec = (b"@r", b"GTTCCACGTCA", b"+", q(2, 2, 2, 40, 40, 40, 40, 40, 40, 40, 40, 40, 2, 2))
    # trim: s' = TTCCACGTC, q' = 2 2 40 x9 2; windows of 2 against 60: good at 2 .. 9 -> (2, 11); s'[2:11] = CCACGTC -> p = 2
    assert adapter_rule.mate_view(rec[1], rec[3], cfg) == (2, 4)
    assert adapter_rule.precut(rec, cfg) == (b"@r", b"CC", b"+", q(40, 40))
    assert adapter_rule.adapter_counts([(rec[1], rec[3], None, None)], cfg) == [1, 5, 0, 0]
    # read 2 is counted only where read 1 leaves the stage with 5 bases or more
    plain = adapter_rule.AdapterConfig(A, K=4)
    s_long, s_short = b"TTTTTTTTACGTTT", b"TTACGTTTTTTTTT"
    qq = b"I" * 14
    assert adapter_rule.adapter_counts([(s_long, qq, s_long, qq), (s_short, qq, s_long, qq)], plain) == [2, 6 + 12, 1, 6]
    assert adapter_rule.adapter_counts([(s_long, qq, s_long, qq), (s_short, qq, s_long, qq)], plain, accum_limit=1) == [1, 6, 1, 6]
    only2 = adapter_rule.AdapterConfig(b"", A, K=4)
    assert adapter_rule.adapter_counts([(s_long, qq, s_long, qq)], only2) == [0, 0, 1, 6]


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def parse(argv):
    options, _ = after.parseCommand(["-1", "r_R1.fq"] + argv)
    return after.finalize_options(options)


def test_cli_option_table():
    table = {long_: kw for _, long_, kw in after.OPTIONS}
    assert table["--adapter_sequence"]["default"] is None and table["--adapter_sequence_r2"]["default"] is None
    assert table["--adapter_min_overlap"]["default"] == 4 and table["--adapter_min_overlap"]["type"] == "int"


def test_cli_defaults_and_inheriting():
    from afterqc_amd import preprocesser
    opt = parse([])
    assert (opt.adapter_sequence, opt.adapter_sequence_r2, opt.adapter_min_overlap) == (None, None, 4)
    assert preprocesser.adapter_config(opt) is None
    opt = parse(["--adapter_sequence", "agatcggaagagc", "--adapter_min_overlap", "6"])
    assert (opt.adapter_sequence, opt.adapter_sequence_r2, opt.adapter_min_overlap) == ("AGATCGGAAGAGC", "AGATCGGAAGAGC", 6)
    c = preprocesser.adapter_config(opt)                        # single-end: no read 2 to search
    assert (c.adapters(), c.min_overlap) == ((b"AGATCGGAAGAGC", b""), 6)
    opt.read2_file = "r_R2.fq"
    assert preprocesser.adapter_config(opt).adapters() == (b"AGATCGGAAGAGC", b"AGATCGGAAGAGC")
    opt = parse(["--adapter_sequence", "ACGTACGT", "--adapter_sequence_r2", "ttgca"])
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == ("ACGTACGT", "TTGCA")
    opt = parse(["-2", "r_R2.fq", "--adapter_sequence_r2", "TTGCA"])            # given alone: only read 2 is searched
    assert (opt.adapter_sequence, opt.adapter_sequence_r2) == (None, "TTGCA")
    assert preprocesser.adapter_config(opt).adapters() == (b"", b"TTGCA")
    # a single-end run never uses read 2's adapter: K is held to read 1's alone
    assert parse(["--adapter_sequence", "ACGTACGT", "--adapter_sequence_r2", "ACGTA", "--adapter_min_overlap", "6"]).adapter_min_overlap == 6
    assert parse(["--adapter_sequence", "ACGT"]).adapter_min_overlap == 4
    assert parse(["--adapter_sequence", "A" * 64, "--adapter_min_overlap", "64"]).adapter_min_overlap == 64


@pytest.mark.parametrize("argv,word", [
    (["--adapter_sequence", "ACGNT"], "letters"), (["--adapter_sequence", "ACG-T"], "letters"), (["--adapter_sequence_r2", "ACGU"], "letters"),
    (["--adapter_sequence", "ACG"], "outside"), (["--adapter_sequence", "A" * 65], "outside"),
    (["--adapter_sequence", "ACGTACGT", "--adapter_sequence_r2", "ACG"], "outside"), (["--adapter_sequence_r2", "C" * 65], "outside"),
    (["--adapter_sequence", "ACGTACGT", "--adapter_min_overlap", "0"], "outside"),
    (["--adapter_sequence", "ACGTACGT", "--adapter_min_overlap", "9"], "outside"),
    (["-2", "r_R2.fq", "--adapter_sequence", "ACGTACGT", "--adapter_sequence_r2", "ACGTA", "--adapter_min_overlap", "6"], "outside"),
    (["-2", "r_R2.fq", "--adapter_sequence_r2", "ACGTA", "--adapter_min_overlap", "6"], "outside"),
    (["--adapter_sequence_r2", "ACGTA"], "single-end"),                         # read 2's adapter alone, and no read 2
])
def test_cli_refusals(argv, word):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert word in str(e.value) and "adapter" in str(e.value)


def small_job(tmp_path, argv, barcode=False):
    from afterqc_amd import synth
    d = synth.make_pairs(64, 60, seed=5)
    t1, n1 = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    p = os.path.join(str(tmp_path), "s_R1.fq")
    with open(p, "wb") as f:
        f.write(bytes(t1[:n1]))
    options, _ = after.parseCommand(["-1", p, "-f", "0", "-t", "0", "-g", os.path.join(str(tmp_path), "good"), "--qc_sample", "0"] + argv)
    after.finalize_options(options)
    options.barcode = barcode
    return options


def test_barcode_with_an_adapter_is_refused(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, ["--adapter_sequence", "AGATCGGAAGAGC"], barcode=True)
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "barcode" in str(e.value) and "adapter" in str(e.value)


def test_read_2_adapter_alone_on_a_single_end_file_is_refused(tmp_path):
    """the folder mode pairs the files after the options are parsed: the run itself refuses, before anything is created"""
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, [])
    opt.adapter_sequence_r2 = "TTGCA"
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "adapter_sequence_r2" in str(e.value) and "single-end" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "good"))


def test_engine_without_the_adapter_pass_is_an_error(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, ["--adapter_sequence", "AGATCGGAAGAGC"])
    with pytest.raises(RuntimeError) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "set_adapter_trim" in str(e.value)


def test_options_without_the_attributes_count_as_off(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, [])
    for k in ("adapter_sequence", "adapter_sequence_r2", "adapter_min_overlap"):
        delattr(opt, k)
    assert preprocesser.adapter_config(opt) is None
    stat = preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "adapter_trim" not in stat
    assert not any(k.startswith("adapter") for k in stat["command"])


# ---- the symbols -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["aqc_set_adapter_trim", "aqc_get_adapter_stats", "aqc_adapter_ms", "aqc_adapter_views"]


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "afterqc_hip.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(aqc_ctx\*" % s, hdr), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "typedef struct aqc_adapter_config { int32_t len1, len2, min_overlap; uint8_t seq1[64], seq2[64]; } aqc_adapter_config;" in hdr
    assert ctypes.sizeof(capi.AdapterConfig) == 3 * 4 + 2 * 64
    c = capi.AdapterConfig("ACGTA", b"TTGCAT", 5)
    assert (c.len1, c.len2, c.min_overlap, c.adapters(), c.on) == (5, 6, 5, (b"ACGTA", b"TTGCAT"), True)
    assert not capi.AdapterConfig().on
    for name in ("set_adapter_trim", "adapter_stats", "adapter_ms", "adapter_views"):
        assert callable(getattr(capi.Engine, name))
    assert callable(capi.MergedEngines.adapter_stats)
    assert lib.aqc_abi_version() == 3                           # (new symbols only: no struct changed)


# ---- the device pass's per-read functions, on the CPU -----------------------------------------------------------------------
def write_vectors(path):
    rng = random.Random(978)
    n_a = n_v = n_m = 0
    lengths = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 320, 321, 511, 512, 513, 999, 1000]
    with open(path, "w") as f:
        for m in ADAPTER_LENGTHS:
            A = adapter_rule.make_adapter(rng, m)
            for K in ks_of(m):
                for n in lengths:
                    for tag, s in adapter_rule.placements(n, A, K, rng):
                        p = adapter_rule.adapter_find(s, A, K)
                        f.write("A %d %s %d %s %d\n" % (K, A.decode(), n, s.hex() or "-", -1 if p is None else p))
                        n_a += 1
        for _ in range(3000):
            c0 = rng.randrange(0, 1001)
            s = adapter_rule.bases(rng, rng.randrange(0, 40))
            A = b"ACGT"
            if rng.random() < 0.6 and len(s) >= 4:
                s = adapter_rule.plant(s, rng.randrange(0, len(s) - 3), A)
            line = b"G" * c0 + s + b"G" * 7
            c1 = rng.choice([0xffff, c0 + rng.randrange(0, len(s) + 8)])
            p = adapter_rule.adapter_find(line[c0:c1], A, 4)
            o = adapter_rule.compose((c0, c1), line, A, 4)
            f.write("V %d %d %d %d %d\n" % (c0, c1, -1 if p is None else p, o[0], o[1]))
            n_v += 1
        for _ in range(4000):
            x = bytes(rng.choice([0, 0, rng.randrange(256), 0x80, 0x01, 0xff]) for _ in range(4))
            left = rng.randrange(-3, 9)
            f.write("M %08x %d %d\n" % (int.from_bytes(x, "little"), left, sum(1 for b in x[:max(left, 0)] if b)))
            n_m += 1
    return n_a, n_v, n_m


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the vector file, written once for both builds of the self-test"""
    path = str(tmp_path_factory.mktemp("adapter_vectors") / "vectors.txt")
    return (path,) + write_vectors(path)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_functions_on_the_cpu(tmp_path, flags, vectors):
    """csrc/aqc_adapter.hpp without HIP: groups of 8, 16, 32 and 64 lanes dealt out by loops over every length at which the pass
    changes its shape, every named placement, against the model; once more as a stand-alone ASan / UBSan binary (each read is
    allocated with exactly the 15 bytes a lane's 16-byte load may take behind it)"""
    exe = os.path.join(str(tmp_path), "adapter_selftest")
    vec, n_a, n_v, n_m = vectors
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "adapter_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all adapter checks passed" in out.stdout, out.stdout[-3000:]
    assert "%d views, %d words checked" % (n_v, n_m) in out.stdout
    assert n_a > 20000
