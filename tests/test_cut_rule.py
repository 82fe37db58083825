"""Per-read sliding-window quality cutting on the CPU: the model of tests/cut_rule.py against a brute-force restatement and a
list of edges worked out by hand; the CLI's options (defaults, range refusals, the barcode refusal, an engine that cannot cut,
the statistics JSON without the options); and the per-read functions of the device pass (csrc/aqc_qcut.hpp) as a stand-alone C++
program on vectors the model writes, plain and under ASan / UBSan (tests/native/qcut_selftest.cpp)."""
import os
import random
import subprocess

import pytest

import cut_rule
from afterqc_amd import after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def q(*phreds):
    return bytes(33 + p for p in phreds)


def test_model_against_brute_force():
    rng = random.Random(20161)
    n_cases = 0
    for _ in range(3000):
        n = rng.choice([0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 32, 33, 60])
        kind = rng.randrange(4)
        if kind == 0:
            line = bytes(rng.randrange(0, 256) for _ in range(n))
        elif kind == 1:
            line = bytes(rng.choice([35, 73]) for _ in range(n))
        elif kind == 2:
            line = cut_rule.decaying_quality(rng, n)
        else:
            line = bytes(rng.randrange(33 + 15, 33 + 26) for _ in range(n))
        W, Q = rng.choice([1, 2, 4, 5, 16, 17, 33, 1000]), rng.choice([0, 2, 15, 20, 21, 40, 93])
        for modes in cut_rule.MODES:
            assert cut_rule.cut_window(line, W, Q, *modes) == cut_rule.cut_window_brute(line, W, Q, *modes), (line, W, Q, modes)
            n_cases += 1
    assert n_cases == 21000


EDGES = [
    # line, W, Q, (front, tail, right) -> (c0, c1)
    (b"", 4, 20, (1, 1, 1), (0, 0)),                                        # an empty line
    (q(40), 4, 20, (1, 0, 0), (0, 1)),                                      # shorter than the window: one window
    (q(2), 4, 20, (1, 0, 0), (0, 0)),                                       # ... and it is bad: nothing kept
    (q(2), 4, 20, (0, 0, 1), (0, 0)),                                       # right alone: the first bad window starts at 0
    (q(20, 20, 20, 20), 4, 20, (1, 1, 1), (0, 4)),                          # exactly the threshold is good
    (q(20, 20, 20, 19), 4, 20, (1, 1, 1), (0, 0)),                          # one below: bad
    # 2 2 40 40 40 40 2 2 in windows of 4: sums 84, 122, 160, 122, 84
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 20, (1, 0, 0), (0, 8)),              # against 80 every window is good
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 30, (1, 0, 0), (1, 8)),              # against 120 the windows at 1, 2, 3 are
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 30, (0, 1, 0), (0, 7)),              # tail: the last good window ends at 3 + 4
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 30, (1, 1, 0), (1, 7)),
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 30, (0, 0, 1), (0, 0)),              # right from 0: window 0 is bad
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 30, (1, 0, 1), (1, 4)),              # right from c0 = 1: window 4 is the first bad one
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 40, (1, 1, 0), (2, 6)),              # against 160 only the window at 2: it alone is kept
    (q(2, 2, 40, 40, 40, 40, 2, 2), 4, 40, (1, 1, 1), (2, 3)),              # ... and right ends it where the bad window at 3 starts
    (q(40, 40, 40, 40, 40, 2, 2, 2), 4, 30, (0, 0, 1), (0, 3)),             # sums 160, 160, 122, 84, 46: the window at 3 is bad
    (q(40, 40, 40, 40, 40, 40), 4, 30, (0, 0, 1), (0, 6)),                  # no bad window: the whole line
    (q(40, 40, 40, 40, 40, 40), 1000, 30, (1, 1, 1), (0, 6)),               # window longer than the line
    (q(40, 2, 40), 1, 20, (1, 1, 1), (0, 1)),                               # W = 1: per-base
    (q(40, 2, 40), 1, 20, (1, 1, 0), (0, 3)),
    (bytes([0x20, 0x09, 33 + 40, 33 + 40]), 2, 10, (1, 0, 0), (2, 4)),      # bytes below '!' count negative: sums -25, 16, 80 against 20
    (bytes([0xff, 0xff]), 2, 93, (1, 1, 1), (0, 2)),                        # bytes >= 0x80 count 222
    (q(2, 2, 2, 2), 4, 0, (1, 1, 1), (0, 4)),                               # Q = 0: every window of non-negative sum is good
]


@pytest.mark.parametrize("case", range(len(EDGES)))
def test_edges(case):
    line, W, Q, modes, want = EDGES[case]
    assert cut_rule.cut_window(line, W, Q, *modes) == want
    assert cut_rule.cut_window_brute(line, W, Q, *modes) == want


def test_precut_slices_each_line_by_its_own_length():
    cfg = cut_rule.CutConfig(front=1, tail=1, window=2, mean_quality=30, trim_front=1, trim_tail=1)
    # quality line longer than the sequence line: the view comes from the quality line, the sequence takes what it has of it
    rec = (b"@r", b"ACGTAC", b"+", q(2, 2, 2, 40, 40, 40, 40, 40, 2, 2))
    # trim: s' = CGTA, q' = 2 2 40 40 40 40 40 2; windows of 2 against 60: good at 2 .. 5 -> c0 = 2, c1 = 7
    assert cut_rule.precut(rec, cfg) == (b"@r", b"TA", b"+", q(40, 40, 40, 40, 40))
    off = cut_rule.CutConfig(trim_front=1, trim_tail=1)
    assert cut_rule.precut(rec, off) == (b"@r", b"CGTA", b"+", q(2, 2, 40, 40, 40, 40, 40, 2))
    assert cut_rule.cut_counts([(rec[1], rec[3], None, None)], cfg) == [1, 2, 0, 0]


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def parse(argv):
    options, _ = after.parseCommand(["-1", "r_R1.fq"] + argv)
    return after.finalize_options(options)


def test_cli_defaults():
    opt = parse([])
    assert (opt.cut_front, opt.cut_tail, opt.cut_right, opt.cut_window_size, opt.cut_mean_quality) == (False, False, False, 4, 20)
    from afterqc_amd import preprocesser
    assert preprocesser.cut_config(opt) is None
    opt = parse(["--cut_tail", "on", "--cut_window_size", "7", "--cut_mean_quality", "25"])
    c = preprocesser.cut_config(opt)
    assert (c.front, c.tail, c.right, c.window, c.mean_quality) == (0, 1, 0, 7, 25)


@pytest.mark.parametrize("argv", [["--cut_window_size", "0"], ["--cut_window_size", "1001"], ["--cut_mean_quality", "-1"], ["--cut_mean_quality", "94"]])
def test_cli_refuses_out_of_range(argv):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert "outside" in str(e.value)


def test_cli_range_ends_are_taken():
    assert parse(["--cut_window_size", "1000", "--cut_mean_quality", "93"]).cut_window_size == 1000
    assert parse(["--cut_window_size", "1", "--cut_mean_quality", "0"]).cut_mean_quality == 0


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


def test_barcode_with_cut_is_refused(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, ["--cut_right", "on"], barcode=True)
    with pytest.raises(SystemExit) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "barcode" in str(e.value)


def test_engine_without_the_cut_is_an_error(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, ["--cut_front", "on"])
    with pytest.raises(RuntimeError) as e:
        preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "set_quality_cut" in str(e.value)


def test_no_quality_cut_key_when_off(tmp_path):
    from afterqc_amd import preprocesser
    from oracle import oracle
    opt = small_job(tmp_path, [])
    stat = preprocesser.seqFilter(opt, engine=oracle.OracleEngine(), use_text_path=False).run()
    assert "quality_cut" not in stat
    assert not any(k.startswith("cut_") for k in stat["command"])


# ---- the device pass's per-read functions, on the CPU -----------------------------------------------------------------------
def write_vectors(path):
    rng = random.Random(977)
    n_w = n_s = 0
    with open(path, "w") as f:
        for n in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 159, 160, 161, 256, 257, 320, 321, 512, 513, 999, 1000):
            for W in (1, 4, 16, 17, 33, 1000):
                for tag, line in cut_rule.pattern_lines(n, W, rng):
                    if n > 161 and tag.startswith("one_good_") and tag not in ("one_good_0", "one_good_33", "one_good_%d" % (n - min(W, n))):
                        continue
                    for Q in (0, 20, 93):
                        modes = cut_rule.MODES[rng.randrange(7)] if n > 33 else None
                        for m in ([modes] if modes else cut_rule.MODES):
                            c0, c1 = cut_rule.cut_window(line, W, Q, *m)
                            f.write("W %d %d %d %d %d %d %s %d %d\n" % (W, Q, m[0], m[1], m[2], n, line.hex() or "-", c0, c1))
                            n_w += 1
        for _ in range(4000):
            ln, tf, tt = rng.randrange(0, 40), rng.randrange(0, 12), rng.randrange(0, 12)
            c0 = rng.randrange(0, 45)
            c1 = rng.randrange(c0, 50)
            s = cut_rule.trim(bytes(range(ln)), tf, tt)[c0:c1]
            f.write("S %d %d %d %d %d %d %d\n" % (ln, tf, tt, c0, c1, s[0] if s else 0, len(s)))
            n_s += 1
    return n_w, n_s


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_functions_on_the_cpu(tmp_path, flags):
    """csrc/aqc_qcut.hpp without HIP: groups of 8, 16, 32 and 64 lanes dealt out by loops over every length at which the pass
    changes its shape, every pattern of the seam test, against the model; once more as a stand-alone ASan / UBSan binary (the line
    is allocated with exactly the 15 bytes a lane's 16-byte load may take behind it)"""
    exe = os.path.join(str(tmp_path), "qcut_selftest")
    vec = os.path.join(str(tmp_path), "vectors.txt")
    n_w, n_s = write_vectors(vec)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "qcut_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all quality cut checks passed" in out.stdout, out.stdout[-3000:]
    assert "%d slices checked" % n_s in out.stdout
    assert n_w > 20000
