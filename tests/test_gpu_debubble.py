"""The debubble pre-pass on the MI355X: the census kernel (aqc_poly_census) against census_host on fuzzed records, every
golden case through the HIP engine, the `after -d DIR --debubble` wiring, two contexts on one GPU, and a 10 M-read
config-3 file pair."""
import os
import random

import numpy as np
import pytest

import debubble_golden as dg
from afterqc_amd import after, capi, debubble, fastq, synth

pytestmark = pytest.mark.gpu
CASES = dg.load_cases()


def _fuzz_text(n, seed):
    rng = random.Random(seed)
    alpha = "0123456789abcdefghijklmnopqrstuvwxyz: \t/#@"
    out = []
    for i in range(n):
        if rng.random() < 0.5:
            name = "@" + "".join(rng.choice(alpha) for _ in range(rng.randrange(1, 60)))
        else:
            f = [rng.choice(["SIM", "x:y", "7"]), str(rng.randrange(0, 9)), rng.choice(["FC", "F:C", "1"]),
                 rng.choice(["1", "12", "+3", "-4", "a", ""]), rng.choice(["1101", "11101", "110", "1a01", "0", "123456789012345678901"]),
                 rng.choice([str(rng.randrange(0, 30000)), "-5", "1" * 25, ""]), str(rng.randrange(0, 30000))]
            name = "@" + ":".join(f) + rng.choice(["", " 1:N:0:ACGT", ":9", "\t2:Y"])
        L = rng.randrange(1, 301)
        s = [rng.choice("ACGTNacgt") for _ in range(L)]
        for _ in range(rng.randrange(0, 4)):
            b = rng.choice("ACGTag")
            r = rng.randrange(15, 26)
            a = rng.randrange(0, L)
            s[a:a + r] = [b] * r
        s = "".join(s)[:L] or "G"
        out.append("%s\n%s\n+\n%s\n" % (name, s, "F" * len(s)))
    return "".join(out).encode()


def _device_hits(eng, text, k, chunk):
    """frame `text` in chunks of about `chunk` bytes and census each; hits as {index: tuple}"""
    got = {}
    pos, total = 0, 0
    buf = np.zeros(chunk + (1 << 16), dtype=np.uint8)
    while True:
        part = text[pos:pos + chunk]
        final = pos + len(part) >= len(text)
        buf[:len(part)] = np.frombuffer(part, np.uint8)
        info = eng.frame(0, buf, len(part), final, first_index=total)
        n = int(info.n)
        h = eng.fetch_census(0, eng.poly_census(0, k)) if n else []
        for r in h:
            st = int(r["status"])
            f = None
            if st == 0:
                f = (int(r["lane"]), int(r["surface"]), int(r["swath"]), int(r["camera"]), int(r["tile"]), int(r["x"]),
                     int(r["y"]), int(r["tile_no"])) if not r["wide"] else "wide"
            assert int(r["index"]) not in got
            got[int(r["index"])] = (st, chr(r["base"]), int(r["count"]), f)
        total += n
        if (info.eof1 or final) and int(info.avail1) == n:
            return got
        pos += int(info.consumed1)


def _host_hits(text, k):
    rd = fastq.Reader.__new__(fastq.Reader)
    starts, lens, nrec, _, _ = fastq.Reader._frame(rd, text, True)
    buf = np.frombuffer(text + b"\0" * 64, np.uint8)
    c = debubble.census_host(buf, starts[:, 1], lens[:, 1], starts[:, 0], lens[:, 0], k)
    want = {}
    for j, i in enumerate(c["index"]):
        st = int(c["status"][j])
        f = None
        if st == 0:
            fields, t = c["names"](j)
            f = tuple(fields) + (t,)
            if any(abs(v) >= 10 ** 18 for v in f):
                f = "wide"
        want[int(i)] = (st, chr(c["base"][j]), int(c["count"][j]), f)
    return want


@pytest.mark.parametrize("k", [20, 5, 3])
def test_census_kernel_fuzz(gpu_engine, k):
    text = _fuzz_text(200_000 if k == 20 else 40_000, seed=11 + k)
    got = _device_hits(gpu_engine, text, k, chunk=3 << 20)
    want = _host_hits(text, k)
    assert len(want) > 1000
    assert got == want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_hip_engine(case, tmp_path):
    got, err = dg.run_case(case, tmp_path, None)
    dg.check(got, case["expect"], err)


def _files(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                out[os.path.relpath(os.path.join(root, f), d)] = fh.read()
    return out


def test_after_main_debubble(tmp_path):
    case = next(c for c in CASES if c["name"] == "no_bubble")
    folder = str(tmp_path / "in")
    dg.write_inputs(folder, case["files"])
    deb = str(tmp_path / "deb")
    after.main(["-d", folder, "--debubble", "--debubble_dir", deb, "-g", str(tmp_path / "g1"), "-b", str(tmp_path / "b1"),
                "-r", str(tmp_path / "r1"), "--qc_sample", "1000"])
    dg.check(dg.outputs(deb), case["expect"], None)
    after.main(["-d", folder, "-g", str(tmp_path / "g2"), "-b", str(tmp_path / "b2"), "-r", str(tmp_path / "r2"), "--qc_sample", "1000"])
    for a, b in (("g1", "g2"), ("b1", "b2")):
        fa, fb = _files(str(tmp_path / a)), _files(str(tmp_path / b))
        assert fa == fb and fa
    # an existing circles.csv: the pass is skipped, the file stays as it is
    deb2 = tmp_path / "deb2"
    deb2.mkdir()
    (deb2 / "circles.csv").write_text("x,y,radius,lane,tile\n")
    st = os.stat(str(deb2 / "circles.csv"))
    after.main(["-d", folder, "--debubble", "--debubble_dir", str(deb2), "-g", str(tmp_path / "g3"), "-b", str(tmp_path / "b3"),
                "-r", str(tmp_path / "r3"), "--qc_sample", "1000"])
    st2 = os.stat(str(deb2 / "circles.csv"))
    assert (deb2 / "circles.csv").read_text() == "x,y,radius,lane,tile\n" and st2.st_mtime_ns == st.st_mtime_ns
    assert sorted(os.listdir(str(deb2))) == ["circles.csv"]


def test_two_workers_on_one_gpu(tmp_path, monkeypatch):
    case = next(c for c in CASES if c["name"] == "many_files")
    monkeypatch.setenv("AQC_DEVICES", "0")
    one, err1 = dg.run_case(case, tmp_path / "a", None)
    monkeypatch.setenv("AQC_DEVICES", "0,0")
    two, err2 = dg.run_case(case, tmp_path / "b", None)
    assert one == two and err1 == err2
    dg.check(two, case["expect"], err2)


def test_config3_10m_reads(tmp_path):
    """a config-3 file pair of 2 x 5 M reads: the device census (the pre-pass's own file loop) vs census_host"""
    for mate in (1, 2):
        p = str(tmp_path / ("C3_R%d.fq" % mate))
        synth.write_census_file(p, 5_000_000, mate=mate)
        eng = capi.Engine(0, 1)
        try:
            dev = debubble.stat_file_device(eng, p, 20)
        finally:
            eng.close()
        host = debubble.stat_file_host(p, 20)
        assert len(host) > 100_000
        assert dev == host
        os.remove(p)
