"""The debubble pre-pass on the CPU: census_host and the host stages against the reference's outputs
(tests/golden/debubble_cases.json.gz, make_debubble.py), the `python -m afterqc_amd.debubble` command line, and the
deviation where upstream would hang (a polyX read whose name int() rejects)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import debubble_golden as dg
from afterqc_amd import after, debubble, fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dg.load_cases()


def count_poly(seq, k):
    """bubbleprocesser.py:385-397 as written"""
    for p in "ATCG":
        if p * k in seq:
            pos = seq.find(p * k)
            count = k
            for c in seq[pos + k:]:
                if c != p:
                    break
                count += 1
            return p, count
    return None, 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_host_engine(case, tmp_path):
    got, err = dg.run_case(case, tmp_path, "host")
    dg.check(got, case["expect"], err)


@pytest.mark.parametrize("name", ["no_bubble", "bubble", "runs"])      # one input file each: no listing order involved
def test_cli_module(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    folder = str(tmp_path / "in")
    dg.write_inputs(folder, case["files"])
    out = str(tmp_path / "bubble_out")
    env = dict(os.environ, AQC_DEBUBBLE_ENGINE="host", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "afterqc_amd.debubble", "-i", folder, "-o", out, "-p", "20",
                        "-d", "on" if case["draw"] else "off"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    # debubble.py's own command line does not catch the detector's exception (debubble.py:37-45): it ends with it
    assert (p.returncode != 0) == (case["expect"]["exception"] is not None), p.stderr
    if case["expect"]["exception"]:
        assert case["expect"]["exception"] in p.stderr
    dg.check(dg.outputs(out), case["expect"], case["expect"]["exception"])


def test_count_poly_matches_upstream_on_random_reads():
    rng = random.Random(5)
    seqs = []
    for i in range(3000):
        L = rng.randrange(1, 160)
        s = [rng.choice("ACGTNacgt") for _ in range(L)]
        for _ in range(rng.randrange(0, 3)):
            b = rng.choice("ACGTa")
            r = rng.randrange(1, 26)
            a = rng.randrange(0, L)
            s[a:a + r] = [b] * r
        seqs.append("".join(s)[:L] or "A")
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, "F" * len(s)) for i, s in enumerate(seqs)).encode()
    rb = fastq.Reader.__new__(fastq.Reader)
    starts, lens, nrec, _, _ = fastq.Reader._frame(rb, text, True)
    buf = np.frombuffer(text + b"\0" * 64, np.uint8)
    for k in (1, 3, 5, 20):
        c = debubble.census_host(buf, starts[:, 1], lens[:, 1], starts[:, 0], lens[:, 0], k)
        got = {int(i): (chr(b), int(n)) for i, b, n in zip(c["index"], c["base"], c["count"])}
        want = {i: count_poly(s, k) for i, s in enumerate(seqs) if count_poly(s, k)[0]}
        assert got == want, k


def test_name_fields():
    st, f, t = debubble.parse_name(b"@A:1:FC:2:11101:100:200 1:N:0:ACGT")
    assert st == debubble.STATUS_OK and f == [2, 1, 1, 1, 1, 100, 200] and t == 11101
    assert debubble.parse_name(b"@read_7")[0] == debubble.STATUS_NO_NAME
    assert debubble.parse_name(b"@A:1:FC:2:110:100:200")[0] == debubble.STATUS_RAISE        # tile_no[3:] == ''
    assert debubble.parse_name(b"a:b:1:c:1:2:3:4")[0] == debubble.STATUS_RAISE              # int('c')
    st, f, t = debubble.parse_name(b"@A:1:FC:2:1101:123456789012345678901234:5")
    assert st == debubble.STATUS_OK and f[5] == 123456789012345678901234


def _raise_folder(tmp_path):
    folder = tmp_path / "in"
    folder.mkdir()
    reads = "".join("@S:1:FC:1:1101:%d:%d\n%s\n+\n%s\n" % (100 + i, 200 + i, "ACGT" * 10, "F" * 40) for i in range(50))
    reads += "@S:1:FC:1:110:7:8\n%s\n+\n%s\n" % ("G" * 30, "F" * 30)            # polyG, tile_no too short: int('') upstream
    (folder / "X_R1.fq").write_text(reads)
    return str(folder)


def test_raise_path_writes_nothing(tmp_path):
    folder = _raise_folder(tmp_path)
    out = str(tmp_path / "debubble")
    with pytest.raises(ValueError):
        debubble.debubbleDir(folder, 20, out, True, engine="host")
    assert not os.path.exists(out)


def test_after_main_prints_upstreams_message(tmp_path, monkeypatch, capsys):
    folder = _raise_folder(tmp_path)
    out = str(tmp_path / "debubble")
    seen = []
    monkeypatch.setenv("AQC_DEBUBBLE_ENGINE", "host")
    monkeypatch.setattr(after, "processDir", lambda folder, options: seen.append(folder))
    after.main(["-d", folder, "--debubble", "--debubble_dir", out, "-g", str(tmp_path / "good")])
    assert debubble.SKIP_MESSAGE in capsys.readouterr().out
    assert seen == [folder]                  # the filter pass runs all the same
    assert not os.path.exists(out)
