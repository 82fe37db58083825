"""Pin the oracle above 250 bases (CPU): tests/golden/long_reads_cases.json.gz holds what the REAL reference answered for the
inputs of tests/golden/long_cases.py — mates of 289 - 320 bases, the lengths of the verdict kernel's 20-word tier.  The function
vectors go through the oracle's util.overlap / hasPolyX / lowQualityNum / nNumber, the end-to-end cases through the host driver
with the oracle engine injected, as tests/test_host_golden.py does for the shorter cases.  tests/test_gpu_long_tier.py (-m gpu)
runs the same inputs on the device."""
import gzip
import json
import os

import pytest

import long_cases
from afterqc_amd import after
from test_host_golden import MODES, PIPE_MODES, check_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_reads_cases.json.gz")
_cache = {}


def golden():
    if "g" not in _cache:
        with gzip.open(GOLDEN, "rt") as f:
            _cache["g"] = json.load(f)
    return _cache["g"]


def vectors(kind):
    """the inputs of one function-vector set, rebuilt from their seed and checked against the digest taken when the reference ran"""
    if kind not in _cache:
        v = {"overlap": long_cases.overlap_pairs, "polyx": long_cases.polyx_vectors, "counts": long_cases.count_vectors}[kind]()
        assert long_cases.digest(v) == golden()["func"][kind + "_digest"], "the seeded inputs are not the ones the reference saw"
        assert len(v) == len(golden()["func"][kind])
        _cache[kind] = v
    return _cache[kind]


def run_long_case(name, tmp_path, engine, mode="text", info=None):
    """one end-to-end case of long_cases.CASES through afterqc_amd's driver (what test_host_golden.run_case does for cases.CASES)"""
    from afterqc_amd import preprocesser
    _, argv, sp = long_cases.CASE_TABLE[name]
    work = str(tmp_path)
    long_cases.materialize(sp, work)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        (options, args) = after.parseCommand(list(argv))
        after.finalize_options(options)
        if options.barcode_flag in options.read1_file and after.parseBool(options.barcode):
            options.barcode = True
            options.trim_front = 0
            options.trim_front2 = 0
        else:
            options.barcode = False
        kw = dict(MODES[mode] if mode in MODES else PIPE_MODES[mode])
        flt = preprocesser.seqFilter(options, engine=engine, **kw)
        stat = flt.run()
        if info is not None:
            info["text_path"] = flt.text_path
            info["used_pipe"] = flt.used_pipe
    finally:
        os.chdir(cwd)
    return work, stat


# ---- function vectors -------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_is_for():
    """the seeded inputs hold the cases the fixture exists for, and the reference's answers show them"""
    pairs, exp = vectors("overlap"), golden()["func"]["overlap"]
    assert 1900 <= len(pairs) <= 2100
    assert all(long_cases.LO <= len(r1) <= long_cases.HI and long_cases.LO <= len(r2) <= long_cases.HI for _, r1, r2 in pairs)
    tags = [t for t, _, _ in pairs]
    by = lambda pred: [e for t, e in zip(tags, exp) if pred(t)]
    assert {(len(r1), len(r2)) for _, r1, r2 in pairs} >= {(320, 289), (289, 320), (320, 320), (289, 289)}
    assert sum(e[0] == 0 and e[1] >= 289 for e in by(lambda t: t == "full")) > 50                 # full length at offset 0
    assert sum(31 <= e[1] <= 34 and e[0] > 250 for e in by(lambda t: t.startswith("minimal"))) > 80
    assert all(e == [0, 0, 0] for e in by(lambda t: t == "minimal_30"))
    assert sum(e[0] < 0 and e[1] > 30 for e in by(lambda t: t == "readthrough")) > 200            # negative offsets, the cut
    for t in (49, 50, 51, 255, 256, 257, 287, 288, 289, 303, 304, 305):
        got = by(lambda tag: tag == "third_%d" % t)
        assert len(got) >= 3, t
        # a third mismatch before column 50 ends the diagonal (util.py:180-183: i < complete_compare_require); from column 50 on
        # the loop runs to the diagonal's end and the pair is accepted with diff >= 3
        assert any(e[2] >= 3 for e in got) == (t >= 50), (t, got[:4])
    assert sum(any(c.islower() for c in r1 + r2) for _, r1, r2 in pairs) > 50
    assert sum("N" in r1 + r2 for _, r1, r2 in pairs) > 100


def test_overlap_vs_reference_289_to_320():
    from oracle import oracle
    bad = [(i, t, exp, oracle.overlap(r1, r2)) for i, ((t, r1, r2), exp) in enumerate(zip(vectors("overlap"), golden()["func"]["overlap"]))
           if list(oracle.overlap(r1, r2)) != exp]
    assert not bad, bad[:5]


def test_polyx_vs_reference_289_to_320():
    from oracle import oracle
    vec, exp = vectors("polyx"), golden()["func"]["polyx"]
    assert all(long_cases.LO <= len(s) <= long_cases.HI for s, _, _ in vec)
    bad = [(i, s, mp, mm, e, oracle.hasPolyX(s, mp, mm)) for i, ((s, mp, mm), e) in enumerate(zip(vec, exp)) if oracle.hasPolyX(s, mp, mm) != e]
    assert not bad, bad[:3]
    assert sum(e is not None for e in exp) > 300 and sum(e is None for e in exp) > 300


def test_counts_vs_reference_289_to_320():
    from oracle import oracle
    vec, exp = vectors("counts"), golden()["func"]["counts"]
    for (s, q, qv), (lq, nn) in zip(vec, exp):
        assert oracle.lowQualityNum(["@", s, "+", q], qv) == lq
        assert oracle.nNumber(["@", s, "+", q]) == nn
    assert sum(lq > 255 for lq, _ in exp) > 50          # counts that do not fit a byte


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["text", "host"])
@pytest.mark.parametrize("name", [c[0] for c in long_cases.CASES])
def test_long_cases_with_oracle_engine(name, mode, tmp_path):
    from oracle import oracle
    work, stat = run_long_case(name, tmp_path, oracle.OracleEngine(), mode)
    check_case(name, work, stat, golden()["e2e"])
