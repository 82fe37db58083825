#!/usr/bin/env python3
"""What the REAL reference (/root/reference, under the py3 shim of make_golden.py) does with the constructed pairs of
tests/verdict_walk_cases.py — run in the build container only:

    python tests/golden/make_walk.py        ->  tests/golden/walk_cases.json.gz

Per tier's table (NW in 10, 16, 18, 20; lead 0 and the barcode instance's 17 — the latter as the plain reads, the prefix adds
nothing the pair phase sees) and per config of it, the rows go in as one FASTQ pair, the row's index in the read name, and the
reference's outputs are reduced to data: per row where it went (good, or bad and under which flag), the final lengths, where the
final read starts in the input and the bytes that differ from it (mate, line, position, byte); per config the counters of the
stats JSON, its error matrix and edit-distance histogram, and the overlap-length histogram of the HTML report (the only place it
is written to).  A row on which the reference raises runs alone and is recorded as such.  The table's digest is stored with it.

The reference's command line sets read 2's trims to read 1's (after.py:200-201); the loop itself reads trim_front2 / trim_tail2 as
options of their own (preprocesser.py:455-466), so this driver replays after.py's main like make_golden's and then sets the four
trims from the config.  Files are read and written as latin-1, so that a quality byte of 255 passes through python 3's text mode
as the byte it is."""
import builtins
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402

TIERS = (10, 16, 18, 20)
OUT = os.path.join(HERE, "walk_cases.json.gz")


def run_ref_main(argv):
    """in a work dir: argv[0] is a JSON object with the four trims, the rest goes to the reference's parser"""
    trims = json.loads(argv[0])
    _open = builtins.open

    def latin_open(file, mode="r", *a, **k):
        if "b" not in mode and "encoding" not in k and len(a) < 2:
            k["encoding"] = "latin-1"
        return _open(file, mode, *a, **k)
    builtins.open = latin_open
    make_golden.install_shim()
    import after
    import qualitycontrol
    sys.argv = ["after.py"] + argv[1:]
    (options, args) = after.parseCommand()
    options.version = after.AFTERQC_VERSION
    options.trim_pair_same = after.parseBool(options.trim_pair_same)
    options.draw = after.parseBool(options.draw)
    options.store_overlap = after.parseBool(options.store_overlap)
    options.barcode = False
    for k, v in trims.items():
        setattr(options, k, v)
    qualitycontrol.len = lambda x: make_golden.Py2Int(builtins.len(x))
    after.processOptions(options)


def argv_of(cfg):
    trims = dict((k, cfg[k]) for k in ("trim_front", "trim_tail", "trim_front2", "trim_tail2"))
    argv = [json.dumps(trims), "-1", "R1.fq", "-2", "R2.fq", "-f", str(cfg["trim_front"]), "-t", str(cfg["trim_tail"]), "-s", str(cfg["seq_len_req"]),
            "-p", str(cfg["poly_size_limit"]), "-a", str(cfg["allow_mismatch_in_poly"]), "-q", str(cfg["qualified_quality_phred"]),
            "-u", str(cfg["unqualified_base_limit"]), "-n", str(cfg["n_base_limit"])]
    return argv + (["--no_correction"] if cfg["no_correction"] else []) + (["--mask_mismatch"] if cfg["mask_mismatch"] else [])


def name_of(i, mate):
    return "@WALK:1:FC:1:1101:%d:2000 %d:N:0:ACGT" % (1000 + i, mate)


def parse(text):
    """-> {row index: (flag name, seq, qual)}"""
    out = {}
    lines = text.split("\n")
    for k in range(0, len(lines) - 3, 4):
        name = lines[k]
        out[int(name.split(":")[5]) - 1000] = (name[1:name.index("WALK")], lines[k + 1], lines[k + 3])
    return out


def reduce_read(inp_seq, inp_qual, seq, qual):
    """-> (start, length, patches [[line, position, byte]]): where the final read lies in the input (the place with the fewest
    differing bases) and what differs there"""
    n = len(seq)
    assert len(qual) == n and n <= len(inp_seq)
    start = min(range(len(inp_seq) - n + 1), key=lambda s: sum(1 for a, b in zip(inp_seq[s:s + n], seq) if a != b))
    patches = [[1, p, ord(seq[p])] for p in range(n) if seq[p] != inp_seq[start + p]]
    patches += [[3, p, ord(qual[p])] for p in range(n) if qual[p] != inp_qual[start + p]]
    return start, n, patches


def run_rows(rows, cfg, indices):
    work = tempfile.mkdtemp(prefix="aqc_walk_")
    try:
        with open(os.path.join(work, "R1.fq"), "w", encoding="latin-1") as f:
            f.write("".join("%s\n%s\n+\n%s\n" % (name_of(i, 1), c.seq1, c.qual1) for i, c in zip(indices, rows)))
        with open(os.path.join(work, "R2.fq"), "w", encoding="latin-1") as f:
            f.write("".join("%s\n%s\n+\n%s\n" % (name_of(i, 2), c.seq2, c.qual2) for i, c in zip(indices, rows)))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run-ref"] + argv_of(cfg), cwd=work, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            tail = p.stdout.strip().splitlines()
            return {"raised": tail[-1] if tail else "?"}
        got = {}
        for dest, sub in (("good", "good"), ("bad", "bad")):
            per_mate = []
            for mate in (1, 2):
                with open(os.path.join(work, sub, "R%d.%s.fq" % (mate, sub)), encoding="latin-1") as f:
                    per_mate.append(parse(f.read()))
            for i in per_mate[0]:
                got[i] = (dest, per_mate[0][i], per_mate[1][i])
        out_rows = []
        for i, c in zip(indices, rows):
            dest, (flag, s1, q1), (flag2, s2, q2) = got[i]
            assert flag == flag2
            a = reduce_read(c.seq1, c.qual1, s1, q1)
            b = reduce_read(c.seq2, c.qual2, s2, q2)
            out_rows.append([flag if dest == "bad" else "GOOD", a[0], a[1], b[0], b[1], [[1] + x for x in a[2]] + [[2] + x for x in b[2]]])
        qc = os.path.join(work, "QC")
        stat = report = None
        for fn in sorted(os.listdir(qc)):
            if fn.endswith(".json"):
                with open(os.path.join(qc, fn)) as f:
                    stat = json.load(f)
            elif fn.endswith(".html"):
                with open(os.path.join(qc, fn), encoding="latin-1") as f:
                    report = make_golden.parse_report(f.read())
        return {"rows": out_rows, "summary": stat["afterqc_main_summary"], "overlap": stat["afterqc_overlap"],
                "overlap_hist": report["figures"]["overlap_stat"]["data"][0]["y"]}
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    import verdict_walk_cases as vwc
    out = {"what": __doc__.split("\n")[0] + " " + __doc__.split("\n")[1], "tables": []}
    for NW in TIERS:
        for lead in (0, vwc.PREFIX):
            table = vwc.with_tier(vwc.cases(NW, lead), NW, lead)
            rec = {"NW": NW, "lead": lead, "digest": vwc.digest(table), "configs": []}
            for cfg, group in vwc.by_config(table):
                plain = [(i, c) for i, c in enumerate(group) if not c.raises]
                got = run_rows([c for _, c in plain], cfg, [i for i, _ in plain])
                assert "raised" not in got, (cfg, got)
                got["cfg"] = cfg
                got["index"] = [i for i, _ in plain]
                got["raises"] = []
                for i, c in enumerate(group):
                    if c.raises:
                        alone = run_rows([c], cfg, [i])
                        assert "raised" in alone, c.tag
                        got["raises"].append([i, alone["raised"]])
                rec["configs"].append(got)
            out["tables"].append(rec)
            print(NW, lead, len(table), "rows in", len(rec["configs"]), "configs")
    # (mtime 0 and no file name in the gzip header: the same table gives the same file, bit for bit)
    with open(OUT, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode("ascii"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run-ref":
        run_ref_main(sys.argv[2:])
    else:
        main()
