"""-m gpu: the hash-chain gzip encoder of `--compression 6 .. 9` (csrc/aqc_gzlz.hpp behind aqc_compress).  As in
test_gpu_gzdev.py every case frames a FASTQ text, lets every record pass whole and holds each compressed stream against zlib
alone (tests/gz_walk.py): the stream inflates to exactly what aqc_fetch_text hands out, MEMBER BY MEMBER — a match that
reached before its member's first byte, or further back than 32768, would fail there — and no member is larger than a stored
block of its text.  Sizes are asserted against zlib level 3 (its greedy parser with chains of 32) on the same 0xff00-byte
pieces, raw deflate + 26 bytes each, with no margin.

Each case prints a `gzlz|` line per stream and level: bytes of text, of the device's gzip, of zlib 3's members."""
import ctypes as C
import gzip
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gz_walk  # noqa: E402
import gzlz_cases as cases  # noqa: E402
from afterqc_amd import capi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

M_LZ = cases.MEMBER
SEG = os.environ.get("AQC_GZ_ENCODER", "")[:1] == "s"
LZ_ON = os.environ.get("AQC_GZ_LZ", "")[:1] != "0"


def member_text(level):
    """text bytes per member: 0xff00 at levels 6 - 9, the default encoder's 64 x 255 below"""
    return M_LZ if (level >= 6 and LZ_ON) or SEG else 64 * 255


def pass_all(paired=False):
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.qc_kmer = 8
    return cfg


def pad(data):
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def zlib_members(text, level, piece=M_LZ):
    """per piece: bytes of a BGZF member made by zlib at this level (raw deflate + 26)"""
    out = []
    for o in range(0, len(text), piece):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(len(c.compress(text[o:o + piece]) + c.flush()) + 26)
    return out


def frame_and_format(engine, slot, text1, text2=None, store_overlap=False, cfg=None):
    engine.set_config(cfg if cfg is not None else pass_all(text2 is not None))
    engine.set_circles([])
    engine.reset_stats()
    if text2 is None:
        info = engine.frame(slot, pad(text1), len(text1), True)
    else:
        info = engine.frame(slot, pad(text1), len(text1), True, pad(text2), len(text2), True)
    engine.run(slot)
    return engine.format(slot, int(info.n), store_overlap)


def compress_and_check(engine, slot, sizes, level, tag=""):
    """aqc_compress on a formatted slot; every non-empty stream checked against zlib and its own text.
    -> {q: dict(text, gz, members = walk()'s)}"""
    gz_sizes = engine.compress(slot, level)
    bufs = [np.zeros(zb + 64, dtype=np.uint8) for zb in gz_sizes]
    ptrs = (C.c_void_p * 6)(*[b.ctypes.data for b in bufs])
    caps = (C.c_uint64 * 6)(*[b.size for b in bufs])
    engine._check(engine.lib.aqc_fetch_streams(engine.h, slot, 1, C.byref(ptrs), C.byref(caps)))
    out = {}
    for q, (nb, zb) in enumerate(zip(sizes, gz_sizes)):
        assert (nb == 0) == (zb == 0), (q, nb, zb)
        if not nb:
            continue
        text = np.zeros(nb + 64, dtype=np.uint8)
        engine.fetch_text(slot, q // 3, q % 3, text, text.size)
        text = text[:nb].tobytes()
        comp = np.full(zb + 64, 0xA5, dtype=np.uint8)
        engine.fetch_gz(slot, q // 3, q % 3, comp, comp.size)
        assert comp[zb:].tobytes() == b"\xa5" * 64, "aqc_fetch_gz wrote past the stream's %d bytes" % zb
        gz = comp[:zb].tobytes()
        assert bufs[q][:zb].tobytes() == gz, "stream %d: aqc_fetch_streams(gz) and aqc_fetch_gz hand out different bytes" % q
        members = gz_walk.check_stream(gz, text, member_text(level))
        for k, m in enumerate(members):
            assert m["btype"] in (gz_walk.STORED, gz_walk.DYNAMIC), "stream %d member %d: block type %d" % (q, k, m["btype"])
        out[q] = {"text": text, "gz": gz, "members": members}
        print("gzlz| %-30s level %d stream %d: text %8d  gz %8d  zlib-3 members %8d  members %3d  stored %3d" % (
            tag, level, q, nb, zb, sum(zlib_members(text, 3)), len(members), sum(1 for m in members if m["btype"] == gz_walk.STORED)))
    return out


def single(engine, slot, text, tag, levels=(9,)):
    """a single-end text whose records all pass: stream 0 is the text itself.  -> {level: stream 0's dict}"""
    sizes = frame_and_format(engine, slot, text)
    assert sizes == [len(text), 0, 0, 0, 0, 0], "the case's records did not pass whole: %r for %d bytes" % (sizes, len(text))
    res = {}
    for level in levels:
        res[level] = compress_and_check(engine, slot, sizes, level, tag)[0]
        assert res[level]["text"] == text
    return res


def per_member(s):
    return [m["size"] for m in s["members"]]


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mate", [1, 2])
def test_real_reads(gpu_engine, mate):
    """tests/golden/testdata: one full member and a 23 KB tail of NextSeq reads.  size(9) <= size(6) < size(2), and level 9 is no
    larger than zlib level 3 on the same pieces"""
    text = cases.real(mate)
    assert M_LZ < len(text) < 2 * M_LZ
    r = single(gpu_engine, 0, text, "real_R%d" % mate, levels=(2, 6, 7, 8, 9))
    size = {level: len(r[level]["gz"]) for level in r}
    assert size[9] <= size[6] < size[2], size
    assert size[9] <= sum(zlib_members(text, 3)), (size, zlib_members(text, 3))


def test_far_repeats(gpu_engine):
    """sequence and quality of record i repeat record i - 37's, 9 KB back: out of reach of a run and of the line four lines up"""
    text = cases.far_repeats()
    cases.check_far_repeats(text)
    r = single(gpu_engine, 0, text, "far_repeats", levels=(2, 9))
    assert len(r[9]["gz"]) < len(r[2]["gz"])
    z3 = zlib_members(text, 3)
    assert len(z3) == len(r[9]["members"]) == 2
    for k, (got, ref) in enumerate(zip(per_member(r[9]), z3)):
        assert got <= ref, "member %d: %d bytes, zlib level 3 %d" % (k, got, ref)


def test_window_edges(gpu_engine):
    """a 300-byte record at member offset 0 and its copy at distance exactly 32768 (the furthest a match may reach) and 32769
    (one too far): both inflate, the first is smaller by most of the copy"""
    near = single(gpu_engine, 0, cases.window_edge(32768), "window_32768")[9]
    far = single(gpu_engine, 0, cases.window_edge(32769), "window_32769")[9]
    assert len(near["members"]) == len(far["members"]) == 1
    assert len(near["gz"]) < len(far["gz"]), (len(near["gz"]), len(far["gz"]))


def test_length_edges(gpu_engine):
    """far repeats of exactly 3, 4, 257, 258, 259, 260, 516 and 1000 bytes (a match is at most 258: the longer ones take two to
    four tokens)"""
    text, marks = cases.length_edges()
    assert [L for _, _, L in marks] == list(cases.REPEAT_LENGTHS)
    assert all(a // M_LZ == (b + L - 1) // M_LZ for a, b, L in marks), "both copies of a repeat lie inside one member"
    single(gpu_engine, 0, text, "length_edges", levels=(6, 9))


def test_repeat_ends_on_the_members_last_byte(gpu_engine):
    r = single(gpu_engine, 0, cases.ends_on_last_byte(), "ends_on_last_byte")[9]
    assert len(r["members"]) == 1 and r["members"][0]["isize"] == M_LZ


def test_source_in_the_previous_member_is_not_used(gpu_engine):
    """the second member begins with copies of what the first ends with: every member inflates on its own (gz_walk), so no match
    crossed the border"""
    r = single(gpu_engine, 0, cases.source_in_previous_member(), "source_in_previous_member")[9]
    assert len(r["members"]) == 2


@pytest.mark.parametrize("total", cases.residues())
def test_member_size_residues(gpu_engine, total):
    """streams of k x 0xff00 + 0, 1, 2, 3, 4 and 0xff00 - 1 bytes: last members of 1, 2 and 3 bytes have no position with a
    three-byte hash, every full member has two"""
    text = cases.exact(np.random.default_rng(7900 + total % 89), total)
    r = single(gpu_engine, 0, text, "residue_%d" % total, levels=(6, 9))
    assert r[9]["members"][-1]["isize"] == (total % M_LZ or M_LZ)


@pytest.mark.parametrize("kind", ["acac", "two_letters"])
def test_long_chains(gpu_engine, kind):
    """60 KB of ACAC... and of two letters from a seed: thousands of positions share each hash; the depth cap holds (the case
    returns) and the member inflates exactly"""
    text = cases.long_chains(kind)
    assert len(text) > 60000 and set(b"".join(text.split(b"\n")[1::2])) <= set(b"ACIH+")
    r = single(gpu_engine, 0, text, "chains_" + kind, levels=(6, 9))
    assert len(r[9]["gz"]) < len(text) // 4


def test_stored_fallback(gpu_engine):
    """16 pieces of ordinary FASTQ — all that the sampling pass sees of 18 — then two of noise: names and qualities uniform over
    '!' .. '~', bytes the shared code gives 12 bits and more.  Those members come out stored, text + 31 bytes at the most
    (check_stream asserts the bound for every member of every case)"""
    rng = np.random.default_rng(7950)
    head = cases.exact(rng, 16 * M_LZ)
    text = head + cases.noise_text(2 * M_LZ - 300)
    r = single(gpu_engine, 0, text, "stored_fallback")[9]
    kinds = [m["btype"] == gz_walk.STORED for m in r["members"]]
    assert len(kinds) == 18 and not any(kinds[:16]) and any(kinds[16:]), kinds
    for m in r["members"]:
        assert m["size"] <= m["isize"] + 31


def test_all_six_streams_and_empty_ones(gpu_engine):
    """paired input with --store_overlap: six streams in one launch; then nothing good and everything bad: streams 0 and 3 empty
    between the others"""
    d = synth.make_pairs(3000, 150, seed=4700, dirty=True)
    t1, n1 = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    t2, n2 = synth.render_fastq_fixed(d["seq2"], d["qual2"], 2)
    t1, t2 = bytes(memoryview(t1)[:n1]), bytes(memoryview(t2)[:n2])
    cfg = capi.Config()
    cfg.paired = 1
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    sizes = frame_and_format(gpu_engine, 0, t1, t2, store_overlap=True, cfg=cfg)
    assert all(sizes), sizes
    assert sorted(compress_and_check(gpu_engine, 0, sizes, 9, "six_streams")) == list(range(6))
    cfg = pass_all(True)
    cfg.seq_len_req = 500
    sizes = frame_and_format(gpu_engine, 0, t1, t2, cfg=cfg)
    assert sizes[0] == 0 and sizes[3] == 0 and sizes[1] > len(t1) and sizes[4] > len(t2), sizes
    assert sorted(compress_and_check(gpu_engine, 0, sizes, 9, "good_streams_empty")) == [1, 4]


def test_geometry_reuse(gpu_engine):
    """one slot at level 9 (members of 0xff00 in slots of 65536), level 2 (16320 in 16896), level 9 again: a 1.2 MB text, then
    the smallest text there is (one record of one base — a stream cannot be a single byte) and a stream with a one-byte tail
    member; and the reverse order.  The staging buffers keep the larger geometry's bytes: every result inflates exactly"""
    rng = np.random.default_rng(7960)
    big = cases.exact(rng, 1_200_000)
    tiny = cases.record(b"r", b"A", b"I")
    tail1 = cases.exact(rng, M_LZ + 1)
    first = {}
    for order in ((big, tiny, tail1), (tail1, tiny, big)):
        for text in order:
            sizes = frame_and_format(gpu_engine, 1, text)
            assert sizes == [len(text), 0, 0, 0, 0, 0]
            for level in (9, 2, 9):
                s = compress_and_check(gpu_engine, 1, sizes, level, "reuse_%d" % len(text))[0]
                assert s["text"] == text
                assert first.setdefault((len(text), level), s["gz"]) == s["gz"], "the same text and level gave other bytes on reuse"


def test_levels_1_to_5_are_unchanged(gpu_engine):
    """levels 1 and 5 give byte for byte level 2's streams"""
    text = cases.real(1)
    r = single(gpu_engine, 0, text, "unchanged_levels", levels=(2, 1, 5))
    assert r[1]["gz"] == r[2]["gz"] == r[5]["gz"]
    assert len(r[2]["members"]) == -(-len(text) // member_text(2))


def test_level_10_is_refused(gpu_engine):
    text = cases.exact(np.random.default_rng(7970), 3000)
    sizes = frame_and_format(gpu_engine, 0, text)
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.compress(0, 10)
    assert e.value.code == -2                              # AQC_ERR_ARG
    assert compress_and_check(gpu_engine, 0, sizes, 9, "after_level_10")[0]["text"] == text


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _run_filter(argv, **kw):
    from afterqc_amd import after, preprocesser
    options, _ = after.parseCommand(list(argv))
    after.finalize_options(options)
    options.barcode = False                                # (after.py:215-221: on only for file names that carry the barcode flag)
    flt = preprocesser.seqFilter(options, **kw)
    stat = json.loads(json.dumps(flt.run()))
    for k in ("good_output_folder", "bad_output_folder", "report_output_folder", "overlap_output_folder", "read1_file", "read2_file", "gzip", "compression"):
        stat["command"].pop(k, None)
    return stat, flt


def test_cli_compression_9_against_2(tmp_path):
    """after.py's options on 2000 pairs of real reads (the 250 of tests/golden/testdata eight times over: 88 KB apart, out of a
    match's reach) with -z --compression 9 and --compression 2, through the pipe: the same text and statistics, good files no
    larger at 9"""
    work = str(tmp_path)
    r1, r2 = os.path.join(work, "R1.fq"), os.path.join(work, "R2.fq")
    for path, mate in ((r1, 1), (r2, 2)):
        with open(path, "wb") as f:
            f.write(cases.real(mate) * 8)
    res = {}
    for level in (9, 2):
        out = os.path.join(work, "level%d" % level)
        stat, flt = _run_filter(["-1", r1, "-2", r2, "-z", "--compression", str(level), "-g", os.path.join(out, "good"), "-b", os.path.join(out, "bad"),
                                 "-r", os.path.join(out, "QC")], use_pipe=True, devices=[0])
        assert flt.used_pipe
        files = {}
        for sub in ("good", "bad"):
            for m in (1, 2):
                p = os.path.join(out, sub, "R%d.%s.fq.gz" % (m, sub))
                with gzip.open(p, "rb") as f:
                    files[(sub, m)] = (os.path.getsize(p), f.read())
        res[level] = (stat, files)
        print("gzlz| cli level %d: %s" % (level, {"%s%d" % k: v[0] for k, v in files.items()}))
    assert res[9][0] == res[2][0]
    for key in res[2][1]:
        assert res[9][1][key][1] == res[2][1][key][1], key
    for m in (1, 2):
        assert len(res[2][1][("good", m)][1]) > 100_000
        assert res[9][1][("good", m)][0] <= res[2][1][("good", m)][0], (m, res[9][1][("good", m)][0], res[2][1][("good", m)][0])
