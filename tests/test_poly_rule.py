"""Cutting poly-G / poly-X tails from each read on the CPU: the model of tests/poly_rule.py against a brute-force restatement (the
sequential loop with its break) over the named placements and the edges worked out by hand; the CLI's options (defaults, both
options on, every refusal, barcoded input, an engine that has no such pass, options objects without the attributes, the
statistics JSON without the options); the new symbols; and the per-read functions of the device pass (csrc/aqc_polytail.hpp) as a
stand-alone C++ program on vectors the model writes, plain and under ASan / UBSan (tests/native/polytail_selftest.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import adapter_rule
import cut_rule
import poly_rule
from afterqc_amd import after, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = list(range(0, 71)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 999, 1000]
MIN_LENGTHS = [1, 2, 8, 10, 17, 40]
G = ord("G")


# ---- the model -------------------------------------------------------------------------------------------------------
def model_cases(lengths=LENGTHS, min_lengths=MIN_LENGTHS, seed=20190):
    """(tag, read, letter, L) over every read length, minimum length, letter and named placement"""
    rng = random.Random(seed)
    for X in poly_rule.LETTERS:
        for L in min_lengths:
            for n in lengths:
                for tag, s in poly_rule.placements(n, X, L, rng):
                    yield tag, s, X, L


def test_model_against_brute_force():
    n_cases = n_cut = 0
    tags = set()
    for tag, s, X, L in model_cases():
        want = poly_rule.poly_end_brute(s, X, L)
        assert poly_rule.poly_end(s, X, L) == want, (tag, s, X, L)
        n_cases += 1
        n_cut += want < len(s)
        tags.add(re.sub(r"\d+", "", tag))
    assert n_cases > 50000 and n_cut > n_cases // 3 and n_cases - n_cut > n_cases // 20, (n_cases, n_cut)
    assert tags == {"clean", "random", "tail_", "whole", "mm__", "cap_", "last_", "N_", "lower_", "two__"}


def test_model_against_brute_force_on_seeded_lines():
    """lines of 0 .. 150 bytes with a tail of any letter, 0 .. 3 substitutions and N inside it"""
    rng = random.Random(77)
    for _ in range(20000):
        n = rng.randrange(0, 151)
        X = rng.choice(poly_rule.LETTERS)
        s = bytearray(poly_rule.with_tail(poly_rule.bases(rng, n), rng.randrange(0, 70), X))
        for _ in range(rng.randrange(0, 4)):
            if n:
                s[n - 1 - rng.randrange(min(n, 70))] = rng.choice(b"ACGTN")
        L = rng.randrange(1, 41)
        assert poly_rule.poly_end(bytes(s), X, L) == poly_rule.poly_end_brute(bytes(s), X, L), (bytes(s), X, L)


EDGES = [
    # line, letter, L -> end
    (b"", b"G", 1, 0),                                                  # an empty line
    (b"ACTACTACTACT" + b"G" * 8, b"G", 10, 20),                         # a tail of 8: mm(10) = 2 > 1, scanned = 9
    (b"ACTACTACTACT" + b"G" * 9, b"G", 10, 12),                         # a tail of 9: mm(10) = 1, fail(11), scanned = 10 -> cut by 9
    (b"ACTACTACTACT" + b"G" * 10, b"G", 10, 12),
    (b"G" * 30, b"G", 10, 0),                                           # a whole read of G: nothing is kept
    (b"G" * 9, b"G", 10, 9),                                            # ... shorter than L: left alone
    (b"ACTACT" + b"G" * 12 + b"A", b"G", 10, 6),                        # a mismatch as the very last byte: the tail in front of it goes
    (b"ACTACT" + b"G" * 12 + b"A", b"G", 1, 19),                        # L = 1: fail(1), nothing
    (b"ACTACT" + b"G", b"G", 1, 6),
    (b"ACTACTACTACT" + b"GGGGGNGGGGGG", b"G", 10, 12),                  # N is a mismatch like any other
    (b"ACTACTACTACT" + b"GGGGGgGGGGGG", b"G", 10, 12),                  # so is a lower-case letter
    (b"ACTACTACTACT" + b"GGGGNgGGGG", b"G", 10, 22),                    # two of them in ten are one too many
    (b"ACT" * 10 + b"A" * 12 + b"G" * 12, b"A", 10, 54),                # the tail of another letter lies behind it: A sees 12 mismatches
    (b"ACT" * 10 + b"A" * 12 + b"G" * 12, b"G", 10, 42),
]


@pytest.mark.parametrize("case", range(len(EDGES)))
def test_edges(case):
    s, X, L, want = EDGES[case]
    assert poly_rule.poly_end(s, X[0], L) == want
    assert poly_rule.poly_end_brute(s, X[0], L) == want


def test_cap_of_five_mismatches():
    front = b"ACT" * 20
    tail = bytearray(b"G" * 100)
    for j in (10, 25, 40, 60, 80):                                      # u = 90, 75, 60, 40, 20: never more than u >> 3
        tail[j] = ord("A")
    s = front + bytes(tail)
    assert poly_rule.poly_end(s, G, 10) == poly_rule.poly_end_brute(s, G, 10) == 60
    tail[5] = ord("A")                                                  # a 6th at u = 95: the scan ends there, the tail behind it goes
    s = front + bytes(tail)
    assert poly_rule.poly_end(s, G, 10) == poly_rule.poly_end_brute(s, G, 10) == 66


def q(*phreds):
    return bytes(33 + p for p in phreds)


def test_smallest_end_and_composition():
    s = b"ACT" * 10 + b"A" * 12 + b"G" * 12
    assert poly_rule.line_end(s, (0, 0, 10, 0)) == 42
    assert poly_rule.line_end(s, (10, 10, 10, 10)) == 42               # one application: the A tail behind the cut is not looked at
    assert poly_rule.line_end(s, (10, 10, 20, 10)) == 54               # G needs 20: nothing cuts
    assert poly_rule.line_end(s[:42], (10, 10, 10, 10)) == 30
    assert poly_rule.PolyConfig.from_options(g=True, x=True, g_len=12, x_len=7).min_len == (7, 7, 7, 7)
    assert poly_rule.PolyConfig.from_options(g=True, x=True, g_len=5, x_len=7).min_len == (7, 7, 5, 7)
    assert poly_rule.PolyConfig.from_options(g=True, g_len=12).min_len == (0, 0, 12, 0)
    assert poly_rule.PolyConfig.from_options(x=True, x_len=9).min_len == (9, 9, 9, 9)
    assert not poly_rule.PolyConfig.from_options().on
    # an incoming view: the stage sees [c0:c1) only
    line = b"ACTACTACTACT" + b"G" * 12 + b"ACTACT"
    assert poly_rule.compose(poly_rule.VIEW_ALL, line, (0, 0, 10, 0)) == poly_rule.VIEW_ALL
    assert poly_rule.compose((0, 24), line, (0, 0, 10, 0)) == (0, 12)              # the view ends behind the tail
    assert poly_rule.compose((2, 20), line, (0, 0, 10, 0)) == (2, 20)              # ... inside it: 8 of G are too few
    assert poly_rule.compose((2, 22), line, (0, 0, 10, 0)) == (2, 12)
    assert poly_rule.compose((2, 12), line, (0, 0, 10, 0)) == (2, 12)              # ... in front of it
    assert poly_rule.compose((14, 24), line, (0, 0, 10, 0)) == (14, 14)            # nothing but tail: nothing is kept
    assert poly_rule.compose((40, 50), line, (0, 0, 10, 0)) == (40, 50)            # beyond the line: the view stays
    # through the whole stage: fixed trim, the quality cut's view from the QUALITY line, each line sliced by its own length
    cut = cut_rule.CutConfig(tail=1, window=2, mean_quality=30, trim_front=1, trim_tail=1)
    cfg = poly_rule.PolyConfig((0, 0, 4, 0), adapter_rule.AdapterConfig(cut=cut))
    rec = (b"@r", b"TACTAGGGGGCA", b"+", q(40, 40, 40, 40, 40, 40, 40, 40, 40, 2, 2, 2))
    # trim: s' = ACTAGGGGGC, q' = 40 x8 2 2 (10); the last good window of 2 starts at 6 -> (0, 8); s'[0:8] = ACTAGGGG -> end 4
    assert poly_rule.mate_view(rec[1], rec[3], cfg) == (0, 4)
    assert poly_rule.precut(rec, cfg) == (b"@r", b"ACTA", b"+", q(40, 40, 40, 40))
    assert poly_rule.poly_counts([(rec[1], rec[3], None, None)], cfg) == [1, 4, 0, 0]
    # read 2 is counted only where read 1 leaves the stage with 5 bases or more
    plain = poly_rule.PolyConfig((0, 0, 6, 0))
    s_long, s_short = b"ACTACTAC" + b"G" * 6, b"AC" + b"G" * 12
    qq = b"I" * 14
    assert poly_rule.poly_counts([(s_long, qq, s_long, qq), (s_short, qq, s_long, qq)], plain) == [2, 6 + 12, 1, 6]
    assert poly_rule.poly_counts([(s_long, qq, s_long, qq), (s_short, qq, s_long, qq)], plain, accum_limit=1) == [1, 6, 1, 6]


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def parse(argv):
    options, _ = after.parseCommand(["-1", "r_R1.fq"] + argv)
    return after.finalize_options(options)


def test_cli_option_table():
    table = {long_: kw for _, long_, kw in after.OPTIONS}
    assert table["--trim_poly_g"]["default"] == "off" and table["--trim_poly_x"]["default"] == "off"
    for k in ("--poly_g_min_len", "--poly_x_min_len"):
        assert table[k]["default"] == 10 and table[k]["type"] == "int"
    shorts = {short: long_ for short, long_, _ in after.OPTIONS if short}
    assert shorts["-g"] == "--good_output_folder" and "-x" not in shorts


def test_cli_defaults_and_both_options():
    from afterqc_amd import preprocesser
    opt = parse([])
    assert (opt.trim_poly_g, opt.poly_g_min_len, opt.trim_poly_x, opt.poly_x_min_len) == (False, 10, False, 10)
    assert preprocesser.poly_config(opt) is None
    assert preprocesser.poly_config(parse(["--trim_poly_g", "off", "--poly_g_min_len", "7"])) is None
    assert preprocesser.poly_config(parse(["--trim_poly_g", "on"])).lengths() == (0, 0, 10, 0)
    assert preprocesser.poly_config(parse(["--trim_poly_g", "on", "--poly_g_min_len", "1000", "--poly_x_min_len", "3"])).lengths() == (0, 0, 1000, 0)
    assert preprocesser.poly_config(parse(["--trim_poly_x", "on"])).lengths() == (10, 10, 10, 10)
    assert preprocesser.poly_config(parse(["--trim_poly_x", "on", "--poly_x_min_len", "1", "--poly_g_min_len", "5"])).lengths() == (1, 1, 1, 1)
    # both on: G takes the smaller of the two lengths
    assert preprocesser.poly_config(parse(["--trim_poly_g", "on", "--trim_poly_x", "on", "--poly_g_min_len", "6", "--poly_x_min_len", "15"])).lengths() == (15, 15, 6, 15)
    assert preprocesser.poly_config(parse(["--trim_poly_g", "on", "--trim_poly_x", "on", "--poly_g_min_len", "20", "--poly_x_min_len", "15"])).lengths() == (15, 15, 15, 15)
    for argv in (["--trim_poly_g", "on", "--trim_poly_x", "on", "--poly_g_min_len", "6", "--poly_x_min_len", "15"], ["--trim_poly_x", "on"], ["--trim_poly_g", "on"]):
        o = parse(argv)
        assert preprocesser.poly_config(o).lengths() == poly_rule.PolyConfig.from_options(o.trim_poly_g, o.trim_poly_x, o.poly_g_min_len, o.poly_x_min_len).min_len


@pytest.mark.parametrize("argv,word", [
    (["--poly_g_min_len", "0"], "poly_g_min_len"), (["--poly_g_min_len", "1001"], "poly_g_min_len"), (["--trim_poly_g", "on", "--poly_g_min_len", "-3"], "poly_g_min_len"),
    (["--poly_x_min_len", "0"], "poly_x_min_len"), (["--trim_poly_x", "on", "--poly_x_min_len", "1001"], "poly_x_min_len"),
])
def test_cli_refusals(argv, word):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert "--" + word in str(e.value) and "outside 1 .. 1000" in str(e.value)


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


@pytest.mark.parametrize("argv", [["--trim_poly_g", "on"], ["--trim_poly_x", "on"]], ids=["g", "x"])
def test_barcode_with_a_poly_option_is_refused(tmp_path, argv):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, argv, barcode=True)
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "barcode" in str(e.value) and "trim_poly_g" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "good"))


def test_engine_without_the_poly_pass_is_an_error(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    assert preprocesser.VIEW_PASSES[2][0] == "set_poly_trim" and len(preprocesser.VIEW_PASSES) == 3
    opt = small_job(tmp_path, ["--trim_poly_g", "on"])
    with pytest.raises(RuntimeError) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "set_poly_trim" in str(e.value)


def test_options_without_the_attributes_count_as_off(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, [])
    for k in ("trim_poly_g", "poly_g_min_len", "trim_poly_x", "poly_x_min_len"):
        delattr(opt, k)
    assert preprocesser.poly_config(opt) is None
    stat = preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "poly_trim" not in stat
    assert not any("poly_g" in k or "poly_x" in k for k in stat["command"])


def test_statistics_without_the_options_have_no_key(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    stat = preprocesser.seqFilter(small_job(tmp_path, []), engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "poly_trim" not in stat and "adapter_trim" not in stat and "quality_cut" not in stat
    assert not any("poly_g" in k or "poly_x" in k for k in stat["command"])


# ---- the symbols -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["aqc_set_poly_trim", "aqc_get_poly_stats", "aqc_poly_ms", "aqc_poly_views"]


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "afterqc_hip.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(aqc_ctx\*" % s, hdr), s
        assert hasattr(lib, s) and s in capi.EXPORTED_SYMBOLS
    assert "typedef struct aqc_poly_config { int32_t min_len[4]; } aqc_poly_config;" in hdr
    assert ctypes.sizeof(capi.PolyConfig) == 4 * 4
    c = capi.PolyConfig(0, 0, 10, 0)
    assert (c.lengths(), c.on) == ((0, 0, 10, 0), True)
    assert capi.PolyConfig(a=3, t=4).lengths() == (3, 0, 0, 4)
    assert not capi.PolyConfig().on
    for name in ("set_poly_trim", "poly_stats", "poly_ms", "poly_views"):
        assert callable(getattr(capi.Engine, name))
    assert callable(capi.MergedEngines.poly_stats)
    assert lib.aqc_abi_version() == 3                           # (new symbols only: no struct changed)


# ---- the device pass's per-read functions, on the CPU -----------------------------------------------------------------------
def write_vectors(path):
    rng = random.Random(979)
    n_p = n_v = n_m = 0
    lengths = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 320, 321, 511, 512, 513, 999, 1000]
    with open(path, "w") as f:
        for X in poly_rule.LETTERS:
            for L in MIN_LENGTHS:
                # the letter alone; with every other letter on at another length; G at a length of its own beside poly-X
                x = poly_rule.LETTERS.index(X)
                alone = tuple(L if j == x else 0 for j in range(4))
                others = tuple(L if j == x else 12 for j in range(4))
                for n in lengths:
                    for tag, s in poly_rule.placements(n, X, L, rng):
                        for lens in (alone, others) if tag.startswith(("two", "tail", "random")) else (alone,):
                            f.write("P %d %d %d %d %d %s %d\n" % (lens + (n, s.hex() or "-", poly_rule.line_end(s, lens))))
                            n_p += 1
        for _ in range(3000):
            c0 = rng.randrange(0, 1001)
            s = poly_rule.with_tail(poly_rule.bases(rng, rng.randrange(0, 40)), rng.randrange(0, 20), G)
            line = b"A" * c0 + s + b"G" * 7
            c1 = rng.choice([0xffff, c0 + rng.randrange(0, len(s) + 8)])
            part = line[c0:c1]
            o = poly_rule.compose((c0, c1), line, (0, 0, 5, 0))
            f.write("V %d %d %d %d %d %d\n" % (c0, c1, len(part), poly_rule.line_end(part, (0, 0, 5, 0)), o[0], o[1]))
            n_v += 1
        for _ in range(4000):
            X = rng.choice(poly_rule.LETTERS)
            b = bytes(rng.choice([X, X, X, rng.randrange(256), X | 0x20, X ^ 0x80, X + 1, 0, 0xff]) & 0xff for _ in range(16))
            nvalid = rng.randrange(0, 17)
            f.write("M %s %c %d %x\n" % (b.hex(), X, nvalid, sum(1 << j for j in range(nvalid) if b[j] != X)))
            n_m += 1
    return n_p, n_v, n_m


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the vector file, written once for both builds of the self-test"""
    path = str(tmp_path_factory.mktemp("poly_vectors") / "vectors.txt")
    return (path,) + write_vectors(path)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_functions_on_the_cpu(tmp_path, flags, vectors):
    """csrc/aqc_polytail.hpp without HIP: groups of 8, 16, 32 and 64 lanes dealt out by loops over every length at which the pass
    changes its shape, every named placement, against the model; once more as a stand-alone ASan / UBSan binary (each read is
    allocated with exactly the 15 bytes a lane's 16-byte load may take behind it)"""
    exe = os.path.join(str(tmp_path), "polytail_selftest")
    vec, n_p, n_v, n_m = vectors
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "polytail_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all poly-tail checks passed" in out.stdout, out.stdout[-3000:]
    assert "%d views, %d masks checked" % (n_v, n_m) in out.stdout
    assert n_p > 20000
