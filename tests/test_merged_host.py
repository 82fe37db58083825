"""--store_merged on the CPU: the CLI's host driver with the ORACLE engine injected, through the host-side writer
(use_text_path=False — seqFilter._write builds the merged reads from the verdicts), against tests/golden/merged_cases.json.gz, which
tests/golden/make_merged.py derived from the REAL reference's good and overlap files by the rule of tests/merged_rule.py.
Also: the option changes no other output, is refused together with --store_overlap on, does nothing for single-end input; and
the per-window functions of the device's reversed copy (csrc/aqc_revcopy.hpp) and the window and plan rules of its forward copies
(csrc/aqc_fmtwin.hpp) as stand-alone C++ programs, plain and under ASan / UBSan (tests/native/revcopy_selftest.cpp, fmtcopy_selftest.cpp)."""
import json
import os
import subprocess
import sys

import pytest

import merged_rule
import test_host_golden as thg
from afterqc_amd import after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = merged_rule.case_table()
MERGED_ON = ["--store_merged", "on"]


@pytest.fixture(scope="module")
def merged_fixture():
    return merged_rule.load_fixture()


def merged_argv(name):
    """the case's argv with the option on; --store_overlap (pe_store_overlap has it) excludes it and is taken out"""
    argv = list(TABLE[name][1])
    if "--store_overlap" in argv:
        k = argv.index("--store_overlap")
        del argv[k:k + 2]
    return argv + MERGED_ON


def run_merged(name, tmp_path, engine, mode="host", info=None, argv=None):
    """test_host_golden.run_case on a case of this module's table (its own name in the table run_case reads)"""
    key = "merged:" + name
    thg.CASE_TABLE[key] = (key, argv if argv is not None else merged_argv(name), TABLE[name][2], False)
    try:
        return thg.run_case(key, tmp_path, engine, mode, info)
    finally:
        del thg.CASE_TABLE[key]


def merged_path(work, name):
    argv = TABLE[name][1]
    main = after_main_name(argv[argv.index("-1") + 1])
    gz = ".gz" if "-z" in argv else ""
    return os.path.join(work, "merged", main + ".merged.fq" + gz)


def after_main_name(fn):
    from afterqc_amd import preprocesser
    return preprocesser.getMainName(fn)


def check_merged_file(name, work, fixture):
    path = merged_path(work, name)
    assert os.path.exists(path), "no merged file " + path
    got = merged_rule.digest_bytes(merged_rule.read_maybe_gz(path))
    exp = {k: fixture[name][k] for k in ("sha256", "lines", "bytes")}
    assert got == exp, (name, got, exp)
    assert sorted(os.listdir(os.path.join(work, "merged"))) == [os.path.basename(path)]


def test_fixture_is_not_vacuous(merged_fixture):
    """what make_merged.py asserted when it wrote the fixture, and that the fixture's inputs are the ones this module rebuilds"""
    assert set(merged_fixture) == set(TABLE)
    for name, rec in merged_fixture.items():
        assert rec["argv"] == list(TABLE[name][1]) and rec["spec"] == TABLE[name][2], name
        if name == "pe_nooverlap":
            assert rec["merged"] == 0 and rec["bytes"] == 0
        else:
            assert rec["merged"] >= 50 and rec["lines"] == 4 * rec["merged"]
    assert merged_fixture["pe_adapter"]["p0"] >= 10
    assert merged_fixture["pe_ragged_short"]["len_diff"] >= 10
    assert merged_fixture["pe_store_overlap"]["overlap_records"] == 788


@pytest.mark.parametrize("name", sorted(TABLE))
def test_host_writer_merged_file(name, tmp_path, merged_fixture, e2e):
    """every fixture case through the host-side writer: the merged file is the fixture's; good / bad files and the stat JSON are
    what the reference wrote without the option (e2e_cases.json.gz; the adapter case has no record there)"""
    from oracle import oracle
    info = {}
    work, stat = run_merged(name, tmp_path, oracle.OracleEngine(), "host", info)
    assert not info["text_path"]
    check_merged_file(name, work, merged_fixture)
    if name in e2e:
        rec = dict(e2e[name])
        rec["files"] = {rel: d for rel, d in rec["files"].items() if not rel.startswith("overlap/")}
        assert not os.path.isdir(os.path.join(work, "overlap"))
        if "--store_overlap" in TABLE[name][1]:
            # (pe_store_overlap runs here without the option that --store_merged excludes: the echo of the command line says so)
            rec["stat"] = json.loads(json.dumps(rec["stat"]))
            rec["stat"]["command"]["store_overlap"] = False
        thg.check_case(name, work, stat, {name: rec})


def test_oracle_engine_takes_the_host_writer(tmp_path, merged_fixture):
    """an engine whose format() knows no merged reads is not asked for them: the default (text) mode falls to the host writer"""
    from oracle import oracle
    info = {}
    work, _ = run_merged("pe_trim_explicit", tmp_path, oracle.OracleEngine(), "text", info)
    assert not info["text_path"]
    check_merged_file("pe_trim_explicit", work, merged_fixture)


def test_merged_output_folder(tmp_path, merged_fixture):
    from oracle import oracle
    name = "pe_nocorr"
    work, _ = run_merged(name, tmp_path, oracle.OracleEngine(), "host", argv=merged_argv(name) + ["--merged_output_folder", "mout"])
    assert not os.path.isdir(os.path.join(work, "merged"))
    got = merged_rule.digest_bytes(merged_rule.read_maybe_gz(os.path.join(work, "mout", "R1.merged.fq")))
    assert got == {k: merged_fixture[name][k] for k in ("sha256", "lines", "bytes")}


def test_refused_with_store_overlap():
    for argv in (["-1", "R1.fq", "-2", "R2.fq", "--store_merged", "on", "--store_overlap", "on"],
                 ["-1", "R1.fq", "--store_overlap", "yes", "--store_merged", "true"]):
        options, _ = after.parseCommand(list(argv))
        with pytest.raises(SystemExit) as e:
            after.finalize_options(options)
        assert e.value.code not in (0, None)
        assert "--store_merged" in str(e.value.code) and "--store_overlap" in str(e.value.code)
    # either alone is fine, and the default is off
    options, _ = after.parseCommand(["-1", "R1.fq", "-2", "R2.fq", "--store_merged", "on"])
    assert after.finalize_options(options).store_merged is True
    options, _ = after.parseCommand(["-1", "R1.fq", "-2", "R2.fq"])
    assert after.finalize_options(options).store_merged is False and options.merged_output_folder is None


def test_refusal_is_the_cli_exit_status(tmp_path):
    """the whole CLI: the message on stderr, a non-zero status, nothing opened"""
    p = subprocess.run([sys.executable, "-m", "afterqc_amd.after", "-1", "R1.fq", "-2", "R2.fq", "--store_merged", "on", "--store_overlap", "on"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "--store_merged" in p.stderr and "--store_overlap" in p.stderr, p.stderr[-2000:]
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("mode", ["host", "text"])
def test_single_end_does_nothing(mode, tmp_path, e2e):
    from oracle import oracle
    name = "se_default"
    _, argv, spec, _ = thg.CASE_TABLE[name]
    key = "merged:" + name
    thg.CASE_TABLE[key] = (key, list(argv) + MERGED_ON, spec, False)
    try:
        work, stat = thg.run_case(key, tmp_path, oracle.OracleEngine(), mode)
    finally:
        del thg.CASE_TABLE[key]
    assert not os.path.exists(os.path.join(work, "merged"))
    thg.check_case(name, work, stat, e2e)


def test_qc_only_writes_nothing(tmp_path):
    from oracle import oracle
    name = "pe_nocorr"
    work, _ = run_merged(name, tmp_path, oracle.OracleEngine(), "host", argv=merged_argv(name) + ["--qc_only"])
    assert not os.path.exists(os.path.join(work, "merged"))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_reversed_copy_windows_on_the_cpu(tmp_path, flags):
    """csrc/aqc_revcopy.hpp without HIP: every (source offset mod 16, destination offset mod 16, p) for p = 0 .. 49, plain and
    complemented, against a byte loop; once more as a stand-alone ASan / UBSan binary"""
    exe = os.path.join(str(tmp_path), "revcopy_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "revcopy_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all revcopy window checks passed" in out.stdout, out.stdout[-3000:]
    assert "25600 pieces" in out.stdout


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_forward_copy_windows_and_plans_on_the_cpu(tmp_path, flags):
    """csrc/aqc_fmtwin.hpp without HIP — the text of the rules the copy kernels expand: the whole-record windows for every length 16 .. 512
    and the general kernel's for every piece length 16 .. 1100, at all 16 source alignments (inside, complete, on the grid, at most 32 /
    piece_items of them), and packed plans decoded per work item against a linear search; once more as a stand-alone ASan / UBSan
    binary, every copy into a heap block that ends with the record"""
    exe = os.path.join(str(tmp_path), "fmtcopy_selftest")
    # (the plan's bytes are read as 16- and 32-bit words, as the kernel reads them from LDS)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fno-strict-aliasing"] + flags + [os.path.join(ROOT, "tests", "native", "fmtcopy_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all fmtcopy window and plan checks passed" in out.stdout, out.stdout[-3000:]
    assert "whole records: 7952 (length, alignment) pairs" in out.stdout            # (512 - 16 + 1) x 16
    assert "general pieces: 17360 (length, alignment) pairs" in out.stdout          # (1100 - 16 + 1) x 16
    # (the plan cases are random: the program itself checks that every kind of them occurred)
