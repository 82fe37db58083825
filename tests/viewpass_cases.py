"""What test_gpu_qcut.py, test_gpu_adapter.py and test_gpu_polytail.py share: the view passes in front of the verdict kernel
(csrc/aqc_viewpass.hpp) are tested the same way — byte strings packed into a batch, a run with the options on against a run of the
same build on the model's pre-cut records, the records a pass leaves under 5 bases, the CLI on files against the CLI on pre-cut
files.  Not a test module."""
import bz2
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np

import adapter_rule
import cut_rule
import poly_rule
import test_host_golden as thg
from afterqc_amd import after, capi, preprocesser, synth

ERR_UNSUPPORTED = -7
# lanes per read of a view pass (quality_cut_kernel<G>, adapter_cut_kernel<G>) -> the lengths of its batch: the host picks G by the batch's longest read (<= 128, <= 256,
# <= 512, anything up to AQC_MAX_READ_LEN), so every group size gets a batch of its own whose longest read is its range's
GROUP_LENGTHS = {8: [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128], 16: [129, 159, 160, 161, 255, 256],
                 32: [257, 288, 289, 320, 321, 511, 512], 64: [513, 999, 1000]}
GROUP_RANGE = {8: (0, 128), 16: (129, 256), 32: (257, 512), 64: (513, 1000)}


def cutcfg(modes, window=4, mean_quality=20):
    return capi.CutConfig(int(modes[0]), int(modes[1]), int(modes[2]), window, mean_quality)


def pack_mate(seqs, quals):
    """-> (seq arena, qual arena, seq offsets, qual offsets, lengths, quality lengths): arenas of their own, so that a quality
    line may have any length"""
    sl = np.array([len(s) for s in seqs], dtype=np.uint32)
    ql = np.array([len(x) for x in quals], dtype=np.uint32)
    so, st = capi.Batch._offsets(sl)
    qo, qt = capi.Batch._offsets(ql)
    sa, qa = np.zeros(st, dtype=np.uint8), np.zeros(qt, dtype=np.uint8)
    for i, (s, x) in enumerate(zip(seqs, quals)):
        sa[int(so[i]):int(so[i]) + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        qa[int(qo[i]):int(qo[i]) + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
    return sa, qa, so, qo, sl, ql


def pack(seqs1, quals1, seqs2=None, quals2=None):
    """a capi.Batch of byte strings; quality lines that are not as long as their sequence lines travel as qlen1 / qlen2"""
    b = capi.Batch(len(seqs1))
    b.seq1, b.qual1, b.off1, b.qoff1, b.len1, ql1 = pack_mate(seqs1, quals1)
    irregular = not np.array_equal(b.len1, ql1)
    ql2 = None
    if seqs2 is not None:
        b.seq2, b.qual2, b.off2, b.qoff2, b.len2, ql2 = pack_mate(seqs2, quals2)
        irregular = irregular or not np.array_equal(b.len2, ql2)
    if irregular:
        b.qlen1, b.qlen2 = ql1, ql2
    return b


def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def views(c0, c1):
    return list(zip(c0.tolist(), c1.tolist()))


def se(pairs, paired):
    return [p if paired else (p[0], p[1], None, None) for p in pairs]


def model_of(modes=None, trim=(0, 0), a1=b"", a2=b"", K=4, lens=None):
    """the models of the passes, each around that of the pass in front of it: the cut's (the fixed trim is its), the adapter's and —
    lens given — the poly-tail pass's"""
    cut = cut_rule.CutConfig(*(modes or (0, 0, 0)), window=4, mean_quality=20, trim_front=trim[0], trim_tail=trim[1])
    adapter = adapter_rule.AdapterConfig(a1, a2, K, cut)
    return adapter if lens is None else poly_rule.PolyConfig(lens, adapter)


def set_passes(eng, cut=None, adapter=None, poly=None):
    """the three passes as given; None: off"""
    eng.set_quality_cut(cut)
    eng.set_adapter_trim(adapter)
    eng.set_poly_trim(poly)


# ---- a run with the options on against a run on the pre-cut records
def base_config(paired, trim=(0, 0)):
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.seq_len_req = 35
    cfg.poly_size_limit = 35
    cfg.allow_mismatch_in_poly = 2
    cfg.qualified_quality_phred = 15
    cfg.unqualified_base_limit = 60
    cfg.n_base_limit = 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    cfg.trim_front = cfg.trim_front2 = trim[0]
    cfg.trim_tail = cfg.trim_tail2 = trim[1]
    return cfg


def tailed_pairs(n, L, seed, short=()):
    """synth.make_pairs (planted overlaps, adapter read-through, mismatches, N) with quality lines of this test's own: high up
    to a knee in the read's last 40 %, single low bases sprinkled in front of it (never two in a window of four), decaying
    behind it — no window of four in front of the knee is bad, no mate is cut below 5 bases.  short: records whose read 1 is high
    for its first 9 .. 13 bases and phred 2 behind them: whatever the modes and a front trim of 2, the cut leaves 5 .. 15 bases."""
    d = synth.make_pairs(n, L, seed=seed, short_frac=0.5, dirty=True)
    rng = random.Random(seed)
    out = []
    for i in range(n):
        mates = []
        for k, (sq, ql) in enumerate((("seq1", "qual1"), ("seq2", "qual2"))):
            if i in short and k == 0:
                knee = rng.randint(9, 13)
                line = bytearray([33 + 40] * knee + [33 + 2] * (L - knee))
            else:
                knee = rng.randint((6 * L) // 10, L)
                line = bytearray(cut_rule.decaying_quality(rng, L, good=40, knee=knee))
                for p in range(rng.randrange(5), knee - 1, 9):
                    line[p] = 33 + 2
            mates.append((d[sq][i].tobytes(), bytes(line)))
        out.append((mates[0][0], mates[0][1], mates[1][0], mates[1][1]))
    return out


def run_pairs(eng, pairs, paired, cfg, cut, adapter=None, poly=None, slot=0, accum_limit=capi.UINT64_MAX):
    """one upload + run with the quality cut, the adapters and the poly-tail pass as given (None: off) -> what the comparison looks
    at.  The cut and the adapters stay as given, the poly-tail pass is off again when this returns."""
    batch = pack([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs] if paired else None, [p[3] for p in pairs] if paired else None)
    eng.set_config(cfg)
    set_passes(eng, cut, adapter, poly)
    try:
        eng.reset_stats()
        eng.upload(slot, batch)
        eng.run(slot, accum_limit)
        res = eng.fetch_results(slot)
        qv = [eng.fetch_quality_views(slot, m) for m in ((0, 1) if paired else (0,))]
        ovl, dist = eng.histograms()
        return dict(res=res, qv=qv, counters=eng.counters(), ovl=ovl, dist=dist, words=eng.last_verdict_words(slot), deferred=eng.last_deferred(slot),
                    cut_ms=eng.cut_ms(slot), cut_stats=eng.cut_stats(), adapter_ms=eng.adapter_ms(slot), adapter_stats=eng.adapter_stats(),
                    poly_ms=eng.poly_ms(slot), poly_stats=eng.poly_stats())
    finally:
        eng.set_poly_trim(None)


def view_bytes(pairs, run, paired):
    """the bytes each result keeps of every line: start / len of the result record, the quality views for the quality lines"""
    out = []
    for i, (p, r) in enumerate(zip(pairs, run["res"])):
        row = []
        for m in ((0, 1) if paired else (0,)):
            a, l = int(r["start%d" % (m + 1)]), int(r["len%d" % (m + 1)])
            qa, ql = int(run["qv"][m][0][i]), int(run["qv"][m][1][i])
            row += [p[2 * m][a:a + l], p[2 * m + 1][qa:qa + ql]]
        out.append(row)
    return out


def compare_runs(pairs, pre, A, B, paired):
    for f in ("flag", "n_edits", "offset", "overlap_len", "distance", "len1") + (("len2",) if paired else ()):
        assert np.array_equal(A["res"][f], B["res"][f]), f
    assert A["res"]["edits"].tobytes() == B["res"]["edits"].tobytes()
    assert view_bytes(pairs, A, paired) == view_bytes(pre, B, paired)
    keep = np.ones(len(A["counters"]), dtype=bool)
    keep[capi.C_TOTAL_BASES] = False
    assert np.array_equal(A["counters"][keep], B["counters"][keep])
    assert np.array_equal(A["ovl"], B["ovl"]) and np.array_equal(A["dist"], B["dist"])


# ---- records a pass leaves under 5 bases.  rule: cut_rule, adapter_rule or poly_rule, whose cut_lines(seq, qual, model, mate) is the model
def check_below_five(pairs, res, rule, model):
    """every record has a mate under 5 bases: BADTRIM1 with read 2 as it came — neither trimmed nor cut —, else BADTRIM2"""
    n1 = n2 = 0
    for p, r in zip(pairs, res):
        k1, k2 = rule.cut_lines(p[0], p[1], model, 0), rule.cut_lines(p[2], p[3], model, 1)
        assert len(k1[0]) < 5 or len(k2[0]) < 5
        a1, l1, a2, l2 = int(r["start1"]), int(r["len1"]), int(r["start2"]), int(r["len2"])
        assert p[0][a1:a1 + l1] == k1[0]
        if len(k1[0]) < 5:
            assert int(r["flag"]) == capi.BADTRIM1
            assert (a2, l2) == (0, len(p[2]))
            n1 += 1
        else:
            assert int(r["flag"]) == capi.BADTRIM2
            assert p[2][a2:a2 + l2] == k2[0]
            n2 += 1
    assert n1 >= 200 and n2 >= 100


def fastq_text(pairs, mate):
    return b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, mate + 1, p[2 * mate], p[2 * mate + 1]) for i, p in enumerate(pairs))


def frame_text(eng, slot, pairs):
    """both mates' text framed into the slot -> the records it holds"""
    t = [fastq_text(pairs, 0), fastq_text(pairs, 1)]
    pad = lambda b: np.frombuffer(b + b"\0" * 4096, dtype=np.uint8).copy()
    return int(eng.frame(slot, pad(t[0]), len(t[0]), True, pad(t[1]), len(t[1]), True).n)


def bad_streams(eng, pairs):
    """text in, text out with the passes as the engine has them: both texts framed into slot 1, run, formatted -> the two bad
    streams; nothing is good"""
    eng.reset_stats()
    assert frame_text(eng, 1, pairs) == len(pairs)
    eng.run(1)
    sizes = eng.format(1, len(pairs), False)
    out = []
    for file in (0, 1):
        assert sizes[file * 3] == 0
        nb = sizes[file * 3 + 1]
        buf = np.zeros(nb + 64, dtype=np.uint8)
        eng.fetch_text(1, file, 1, buf, buf.size)
        out.append(buf[:nb].tobytes())
    return out


def badtrim_text(pairs, rule, model):
    """... and what they hold: every record as @BADTRIM1... / @BADTRIM2..., read 1 as the pass leaves it, read 2 only under BADTRIM2"""
    want = [[], []]
    for i, p in enumerate(pairs):
        k1, k2 = rule.cut_lines(p[0], p[1], model, 0), rule.cut_lines(p[2], p[3], model, 1)
        flag = b"BADTRIM1" if len(k1[0]) < 5 else b"BADTRIM2"
        if flag == b"BADTRIM1":
            k2 = (p[2], p[3])
        want[0].append(b"@%sr%d/1\n%s\n+\n%s\n" % (flag, i, k1[0], k1[1]))
        want[1].append(b"@%sr%d/2\n%s\n+\n%s\n" % (flag, i, k2[0], k2[1]))
    return [b"".join(w) for w in want]


# ---- a child process: a test module run as a script, with a role and an environment of its own
def run_child(script, role, env):
    """-> the JSON object on the last line the child wrote"""
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(script), role], capture_output=True, text=True, timeout=300, env=e, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


# ---- the CLI on files


def write_inputs(work, tag, pairs, paired, gz, index=False):
    os.makedirs(work, exist_ok=True)
    names = []
    for mate in range(2 if paired else 1):
        text = b"".join(b"@SIM:1:FC1:1:1101:%d:%d %d:N:0:ACGT\n%s\n+\n%s\n" % (1000 + i, 2000 + i, mate + 1, p[2 * mate], p[2 * mate + 1]) for i, p in enumerate(pairs))
        path = os.path.join(work, "%s_R%d.fq%s" % (tag, mate + 1, gz))
        with (gzip.open(path, "wb", compresslevel=1) if gz == ".gz" else bz2.open(path, "wb") if gz == ".bz2" else open(path, "wb")) as f:
            f.write(text)
        names.append(path)
    if index:
        for k in (1, 2):
            path = os.path.join(work, "%s_I%d.fq" % (tag, k))
            with open(path, "wb") as f:
                f.write(b"".join(b"@SIM:1:FC1:1:1101:%d:%d %d:N:0:ACGT\nACGTACGT\n+\nIIIIIIII\n" % (1000 + i, 2000 + i, k) for i in range(len(pairs))))
            names.append(path)
    return names


def run_cli(work, files, paired, argv, kw, engine, index=False):
    args = ["-1", files[0]] + (["-2", files[1]] if paired else []) + ["-g", os.path.join(work, "good"), "--qc_sample", "0", "--barcode", "off"] + argv
    if index:
        args += ["-7", files[-2], "-5", files[-1]]
    options, _ = after.parseCommand(args)
    after.finalize_options(options)
    options.barcode = False
    kw = dict(kw)
    if kw.pop("own_engines", False):
        engine = None
    flt = preprocesser.seqFilter(options, engine=engine, **kw)
    stat = flt.run()
    return stat, flt.used_pipe


def read_outputs(work):
    out = {}
    for folder in ("good", "bad", "overlap", "merged"):
        d = os.path.join(work, folder)
        if not os.path.isdir(d):
            continue
        for f in sorted(os.listdir(d)):
            p = os.path.join(d, f)
            with (gzip.open(p, "rb") if f.endswith(".gz") else open(p, "rb")) as fh:
                # the two runs' inputs are named "raw_*" and "pre_*"
                out[folder + "/" + f[4:]] = fh.read()
    return out


def compare_cli_stats(sa, sb):
    """the statistics of the run with the options (sa), key by key of the run without them: equal but for what sees the raw reads —
    total_bases, readlen (the pre-filter sample's read length) and the pre-filter QC sections — and the command line"""
    for k in sb:
        if k == "command":
            continue
        if k == "afterqc_main_summary":
            skip = ("total_bases", "readlen")
            assert {x: v for x, v in sa[k].items() if x not in skip} == {x: v for x, v in sb[k].items() if x not in skip}
        elif isinstance(sb[k], dict) and any("prefilter" in x for x in sb[k]):
            assert {x: v for x, v in sa[k].items() if "prefilter" not in x} == {x: v for x, v in sb[k].items() if "prefilter" not in x}, k
        else:
            assert sa[k] == sb[k], k


def driver_kw(driver):
    """the seqFilter keywords of a driver the host golden tests name (the serial text loop, the whole-input pipe's variants)"""
    return thg.MODES[driver] if driver in thg.MODES else thg.PIPE_MODES[driver]
