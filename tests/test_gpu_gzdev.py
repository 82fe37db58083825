"""-m gpu: the device gzip encoders (csrc/aqc_gzdev.hpp behind aqc_compress) at member, line and code edges.  Every case frames
a FASTQ text made here from a seed, lets every record pass whole, and holds each compressed stream against zlib alone
(tests/gz_walk.py): the stream inflates to exactly what aqc_fetch_text hands out, member by member, and no member is larger
than a stored block of its text.  Every case asserts from its text or from the members that it reached the branch it is named
for.  The default encoder (gz_encode_wave_kernel, members of 16320 bytes) runs in this process; gz_encode_kernel (members of
65280 bytes) is chosen by AQC_GZ_ENCODER=seg, which the library reads once per process: one test runs this file's seg cases in
a fresh child process and asserts on the JSON line it prints.

Each case prints a `gzdev|` line per stream: bytes of text, of the device's gzip, of zlib level 1, the members, how many of
them stored.  Sizes are not asserted beyond the stored-block bound: the encoders are not designed for these shapes."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gz_walk  # noqa: E402
from afterqc_amd import capi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

M_WAVE, M_SEG = 64 * 255, 256 * 255           # GZW_TEXT, GZ_TEXT
PIECE = M_SEG                                  # what the sampling pass cuts a stream into, whatever the encoder
SEG = os.environ.get("AQC_GZ_ENCODER", "")[:1] == "s"
M = M_SEG if SEG else M_WAVE
ENCODER = "seg" if SEG else "wave"
TIMES = {}                                     # seconds of the default-encoder cases the seg child also runs


# ---- the helper -----------------------------------------------------------------------------------------------------------------
def pass_all(paired=False):
    """no trimming, no filter: every record is good and goes out as its own bytes"""
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.qc_kmer = 8
    return cfg


def pad(data):
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def roundtrip(engine, slot, text1, text2=None, store_overlap=False, level=2, cfg=None, tag=""):
    """frame -> run -> format -> compress; every non-empty stream checked against zlib and its own text.
    -> (sizes from format(), {q: dict(text, gz_bytes, zlib1_bytes, members = [(stored, bytes, text bytes)])})"""
    engine.set_config(cfg if cfg is not None else pass_all(text2 is not None))
    engine.set_circles([])
    engine.reset_stats()
    if text2 is None:
        info = engine.frame(slot, pad(text1), len(text1), True)
    else:
        info = engine.frame(slot, pad(text1), len(text1), True, pad(text2), len(text2), True)
    engine.run(slot)
    sizes = engine.format(slot, int(info.n), store_overlap)
    gz_sizes = engine.compress(slot, level)
    # the pipe's way out: all six streams with one call
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
        members = gz_walk.check_stream(gz, text, M)
        for k, m in enumerate(members):
            assert m["btype"] in (gz_walk.STORED, gz_walk.DYNAMIC), "stream %d member %d: block type %d" % (q, k, m["btype"])
        z1 = len(zlib.compress(text, 1))
        out[q] = {"text": text, "gz_bytes": zb, "zlib1_bytes": z1,
                  "members": [(m["btype"] == gz_walk.STORED, m["size"], m["isize"]) for m in members]}
        print("gzdev| %-28s %-4s stream %d: text %8d  gz %8d  zlib-1 %8d  gz/zlib-1 %5.2f  members %4d  stored %4d" % (
            tag, ENCODER, q, nb, zb, z1, zb / z1, len(members), sum(1 for m in out[q]["members"] if m[0])))
    return sizes, out


def single(engine, slot, text, tag, **kw):
    """a single-end text whose records all pass: stream 0 is the text itself"""
    sizes, out = roundtrip(engine, slot, text, tag=tag, **kw)
    assert sizes == [len(text), 0, 0, 0, 0, 0], "the case's records did not pass whole: %r for %d bytes" % (sizes, len(text))
    assert out[0]["text"] == text
    return out[0]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
QUALS = np.frombuffer(b"EA/<6#", dtype=np.uint8)
QUAL_P = [0.64, 0.18, 0.09, 0.06, 0.02, 0.01]


def record(name, seq, qual):
    assert len(seq) == len(qual)
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def bases(rng, L):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()


def quals(rng, L):
    return QUALS[rng.choice(6, L, p=QUAL_P)].tobytes()


def sim_name(rng, i):
    return b"SIM:1:FC1:%d:%d:%d:%d 1:N:0:ACGT" % (1 + i % 4, 1101 + int(rng.integers(0, 1200)), 1000 + int(rng.integers(0, 24000)), 1000 + int(rng.integers(0, 19000)))


def ordinary(rng, nbytes, L=150):
    """ordinary low-entropy FASTQ: at least nbytes of it"""
    out, n, i = [], 0, 0
    while n < nbytes:
        out.append(record(sim_name(rng, i), bases(rng, L), quals(rng, L)))
        n += len(out[-1])
        i += 1
    return out


def filler(rng, size):
    """one record of exactly `size` bytes (>= 40)"""
    assert size >= 40
    nl = 10 + size % 2
    L = (size - 6 - nl) // 2
    r = record(b"f" * nl, bases(rng, L), quals(rng, L))
    assert len(r) == size
    return r


def sized(seed, total):
    """ordinary FASTQ of exactly `total` bytes: the last record's name length makes up the size"""
    rng = np.random.default_rng(seed)
    out, n, i = [], 0, 0
    while True:
        r = record(sim_name(rng, i), bases(rng, 100), quals(rng, 100))
        if n + len(r) + 40 + 27 > total:
            break
        out.append(r)
        n += len(r)
        i += 1
    left = total - n                     # 67 .. ~310
    if left > 160:
        out.append(filler(rng, left - 100))
        left = 100
    out.append(record(b"t" * (left - 26), bases(rng, 10), quals(rng, 10)))
    text = b"".join(out)
    assert len(text) == total
    return text


def residue_sizes(m):
    """less than a member; exactly one; one plus 1, 2, 3 bytes; two plus 4; a byte short of three; exactly two; three plus 1"""
    return [1000, m, m + 1, m + 2, m + 3, 2 * m + 4, 3 * m - 1, 2 * m, 3 * m + 1]


def lines_per_piece(text, piece):
    return [text[o:o + piece].count(b"\n") for o in range(0, len(text), piece)]


def short_lines_text(kind):
    rng = np.random.default_rng(4100 + len(kind))
    if kind == "reads_of_20":
        # 20 bases, names of about 20 bytes: 66 bytes and 4 lines a record, ~990 lines in 16320 bytes
        return b"".join(record(b"SIM:1:FC1:2:%04d:%05d" % (1101 + i % 7, 10000 + 13 * i), bases(rng, 20), quals(rng, 20)) for i in range(2 * M // 66 + 40))
    if kind == "turns_short":
        # every member begins with 150-base records and turns to 5-base records: the line limit is crossed inside the member
        out, n = [], 0
        while n < 2 * M + 3000:
            at = n % M
            r = record(sim_name(rng, len(out)), bases(rng, 150), quals(rng, 150)) if at < M // 3 else record(b"s%d" % (len(out) % 10), bases(rng, 5), quals(rng, 5))
            out.append(r)
            n += len(r)
        return b"".join(out)
    if kind == "reads_of_5":
        # 5 bases, 2-byte names: 18 bytes and 4 lines a record, 14.5 K lines in 65280 bytes — the sampling pass's limit of 4096
        return b"".join(record(b"%c%c" % (97 + i % 26, 48 + i % 10), bases(rng, 5), quals(rng, 5)) for i in range(PIECE // 19 + 300))
    raise KeyError(kind)


def long_runs_text(L, n_bases=False):
    rng = np.random.default_rng(4200 + L)
    n = max(3, -(-(2 * M + 2000) // (2 * L + 40)))
    return b"".join(record(sim_name(rng, i), b"N" * L if n_bases else bases(rng, L), b"I" * L) for i in range(n))


def run_starts(text, at_least=258):
    """offsets at which a run of one byte at least that long begins"""
    a = np.frombuffer(text, dtype=np.uint8)
    change = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1], [True])))
    return [int(s) for s, e in zip(change[:-1], change[1:]) if e - s >= at_least]


ALIGNED = [(64, 63), (64, 62), (64, 0), (255, 254), (255, 253), (255, 0)]


def aligned_runs_text():
    """quality runs of 600 that begin at the last byte of a 64-byte window / at byte 254 of a 255-byte segment (and one byte
    before, where the run's first MATCHED byte is that byte; and at byte 0), all inside full members"""
    rng = np.random.default_rng(4300)
    out, n = [], 0
    for k, (mod, want) in enumerate(ALIGNED * 2):
        name = sim_name(rng, k)
        start = n + len(name) + 2 + 600 + 1 + 2              # where the quality line would begin
        shift = (want - start) % mod
        f = filler(rng, 40 + (shift - 40) % mod)
        out.append(f)
        n += len(f)
        out.append(record(name, bases(rng, 600), b"I" * 600))
        n += len(out[-1])
    out += ordinary(rng, 2 * M_SEG + 500 - n)
    return b"".join(out)


def columns_text(kind):
    rng = np.random.default_rng(4400 + len(kind))
    if kind == "counters":
        return b"".join(record(b"read.%d/1" % i, bases(rng, 30), quals(rng, 30)) for i in range(1200))
    if kind == "alternating":
        return b"".join(record(sim_name(rng, i), bases(rng, L), quals(rng, L)) for i in range(300) for L in ((30, 150, 31, 149)[i % 4],))
    if kind == "identical":
        out = ordinary(rng, 3000)
        one = record(sim_name(rng, 7), bases(rng, 150), quals(rng, 150))
        return b"".join(out + [one] * 10 + ordinary(rng, M) + [one] * 10 + ordinary(rng, 2000))
    if kind == "name_lengths":
        # a name longer than the one four lines up, then shorter, by 1 .. 40 bytes; the shared prefix is the column match
        return b"".join(record(b"SIM:1:FC1:3:1101:2000:3000" + b":x" * ((i * 5) % 21 if i % 2 else 0) + b" 1:N:0:ACGT", bases(rng, 50), quals(rng, 50)) for i in range(400))
    raise KeyError(kind)


def literals_text(kind):
    """names: carry space, tab, 0x7f, 0x80 and 0xff (none of them first or last in the name: whole lines are kept as they are);
    bases: lowercase acgtn; qualities: every byte of '!' .. '~'"""
    rng = np.random.default_rng(4500 + len(kind))
    if kind == "names":
        odd = [b" ", b"\t", b"\x7f", b"\x80", b"\xff", b"\x80\xff\x7f", b" \t "]
        return b"".join(record(b"SIM:1:FC1" + odd[i % 7] + b"%d" % (1101 + i % 5) + odd[(i // 7) % 7] + b"x:%d" % (2000 + 3 * i), bases(rng, 100), quals(rng, 100)) for i in range(200))
    if kind == "lowercase":
        return b"".join(record(sim_name(rng, i), bases(rng, 100).lower() if i % 3 else b"n" * 7 + bases(rng, 93).lower(), quals(rng, 100)) for i in range(200))
    if kind == "qualities":
        return b"".join(record(sim_name(rng, i), bases(rng, 94), (np.arange(94, dtype=np.uint8) + 33)[rng.permutation(94)].tobytes()) for i in range(200))
    raise KeyError(kind)


SHORT_REC = record(b"q", b"ACGTA", b"IIIII")


def stored_text(pieces=18):
    """SHORT_REC (the filter sends it to the bad stream: a tiny second stream), then 16 pieces of 65280 bytes of ordinary FASTQ
    — all that the sampling pass sees of a stream of 17 .. 31 pieces — then records whose names and qualities are drawn
    uniformly from '!' .. '~': bytes the shared code has seen rarely or never"""
    rng = np.random.default_rng(4600)
    out = ordinary(rng, 16 * PIECE + 200)
    n = sum(len(r) for r in out)
    while n < pieces * PIECE - 300:
        r = record(rng.integers(33, 127, 80, dtype=np.uint8).tobytes(), bases(rng, 10), rng.integers(33, 127, 10, dtype=np.uint8).tobytes())
        out.append(r)
        n += len(r)
    return SHORT_REC + b"".join(out)


def stored_case(engine, slot, tag="stored_fallback"):
    text = stored_text()
    cfg = pass_all()
    cfg.seq_len_req = 8                                   # SHORT_REC's five bases: BADLEN
    sizes, out = roundtrip(engine, slot, text, cfg=cfg, tag=tag)
    good = text[len(SHORT_REC):]
    assert sizes[0] == len(good) and sizes[1] > len(SHORT_REC) and sizes[2:] == [0, 0, 0, 0], sizes
    assert out[0]["text"] == good and out[1]["text"].endswith(SHORT_REC[2:])
    assert 17 <= -(-len(good) // PIECE) <= 20
    kinds = [m[0] for m in out[0]["members"]]
    assert any(kinds) and not all(kinds), "stored members: %d of %d" % (sum(kinds), len(kinds))
    assert not any(kinds[:16 * PIECE // M]), "an ordinary member came out stored"
    assert len(out[1]["members"]) == 1
    return out


# ---- the default encoder's cases ---------------------------------------------------------------------------------------------------
def timed(name):
    class T:
        def __enter__(self):
            self.t0 = time.perf_counter()

        def __exit__(self, *exc):
            TIMES[name] = TIMES.get(name, 0.0) + time.perf_counter() - self.t0
    return T()


@pytest.mark.parametrize("total", residue_sizes(M_WAVE))
def test_member_size_residues(gpu_engine, total):
    """stream sizes 1, 2, 3, 4, member - 1, 0 and 1 past a multiple of the member: the last member takes the CRC path for fewer
    than four bytes, or is full (no padding in front of it)"""
    with timed("residues"):
        s = single(gpu_engine, 0, sized(5000 + total % 97, total), "residue_%d" % total)
    assert len(s["text"]) == total and s["members"][-1][2] == (total % M or M)


@pytest.mark.parametrize("kind", ["reads_of_20", "turns_short", "reads_of_5"])
def test_short_lines(gpu_engine, kind):
    """more than GZW_MAX_LINES = 512 lines in a member of 16320 bytes (column matches stop inside the member), more than
    GZ_MAX_LINES = 4096 in a piece of 65280 (the sampling pass decides for the whole piece)"""
    text = short_lines_text(kind)
    with timed("short_lines"):
        s = single(gpu_engine, 0, text, "short_lines_" + kind)
    per = lines_per_piece(text, M)
    assert len(per) >= 3 and min(per[:-1]) > 512, per
    if kind == "turns_short":
        # line 511 is reached well inside each full member, behind a stretch of long records that has column matches
        for o in range(0, len(text) - M, M):
            piece = text[o:o + M]
            assert piece[:M // 4].count(b"\n") < 120 and piece.count(b"\n") > 2000
    if kind == "reads_of_5":
        assert lines_per_piece(text, PIECE)[0] > 4096
    assert sum(m[2] for m in s["members"]) == len(text)


@pytest.mark.parametrize("L,n_bases", [(258, False), (259, False), (300, False), (515, False), (1000, False), (1000, True)])
def test_long_runs(gpu_engine, L, n_bases):
    """quality lines of one character: runs of 258 (one match of 257 behind the literal), 259 (the cap of 258), 300 and 515 (a
    second and a third token), 1000 (AQC_MAX_READ_LEN: longer than the five 64-byte windows of masks kept ahead); bases too"""
    text = long_runs_text(L, n_bases)
    s = single(gpu_engine, 0, text, "long_runs_%d%s" % (L, "_N" if n_bases else ""))
    runs = run_starts(text)
    assert len(runs) >= (2 if n_bases else 1) * text.count(b"\n+\n") and len(s["members"]) >= 3
    assert all(text[r:r + L] in (b"I" * L, b"N" * L) and text[r + L] == 10 for r in runs)


def test_runs_at_window_and_segment_borders(gpu_engine):
    text = aligned_runs_text()
    with timed("aligned_runs"):
        s = single(gpu_engine, 0, text, "aligned_runs")
    runs = [r for r in run_starts(text) if r + 600 <= (len(text) // M_SEG) * M_SEG]          # inside members that are full for either encoder
    for mod, want in ALIGNED:
        assert any(r % mod == want for r in runs), (mod, want, [r % mod for r in runs])
    assert len(s["members"]) == -(-len(text) // M)


@pytest.mark.parametrize("kind", ["counters", "alternating", "identical", "name_lengths"])
def test_column_matches_with_shifting_columns(gpu_engine, kind):
    """the line four up as the match source: name counters that grow a digit, neighbours of other lengths (the match is cut where
    the line four up ends), identical records (matches run through the line end), names longer / shorter than the one before"""
    text = columns_text(kind)
    s = single(gpu_engine, 0, text, "columns_" + kind)
    lines = text.split(b"\n")
    if kind == "counters":
        assert b"@read.9/1" in lines and b"@read.10/1" in lines and b"@read.99/1" in lines and b"@read.100/1" in lines and b"@read.1000/1" in lines
    elif kind == "alternating":
        assert [len(l) for l in lines[1:16:4]] == [30, 150, 31, 149]
    elif kind == "identical":
        recs = [b"\n".join(lines[i:i + 4]) for i in range(0, len(lines) - 1, 4)]
        assert sorted(sum(1 for _ in g) for _, g in itertools.groupby(recs))[-3:] == [1, 10, 10]
    else:
        names = [len(l) for l in lines[0:-1:4]]
        d = np.diff(names)
        assert d.max() >= 40 and d.min() <= -40
    assert len(s["members"]) >= 2


@pytest.mark.parametrize("kind", ["names", "lowercase", "qualities"])
def test_unusual_literals(gpu_engine, kind):
    """names with space, tab, 0x7f, 0x80, 0xff inside; lowercase bases; qualities over all of '!' .. '~': bytes the sampled
    counts may hold once or not at all still have a code"""
    text = literals_text(kind)
    s = single(gpu_engine, 0, text, "literals_" + kind)
    have = set(text)
    if kind == "names":
        assert {0x20, 0x09, 0x7f, 0x80, 0xff} <= have
    elif kind == "lowercase":
        assert set(b"acgtn") <= have and not set(b"ACGT") & set(b"".join(text.split(b"\n")[1::4]))
    else:
        assert set(range(33, 127)) <= have
    assert s["text"] == text


def test_stored_fallback(gpu_engine):
    """a stream of 18 pieces whose last two the sampling pass never saw: their members come out stored, the ordinary ones
    dynamic; a one-record stream next to it round-trips either way"""
    with timed("stored"):
        stored_case(gpu_engine, 0)


def test_all_six_streams(gpu_engine):
    """paired input, --store_overlap: good, bad and overlap streams of both files in one launch"""
    d = synth.make_pairs(3000, 150, seed=4700, dirty=True)
    t1, n1 = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    t2, n2 = synth.render_fastq_fixed(d["seq2"], d["qual2"], 2)
    cfg = capi.Config()
    cfg.paired = 1
    cfg.seq_len_req, cfg.poly_size_limit, cfg.allow_mismatch_in_poly = 35, 35, 2
    cfg.qualified_quality_phred, cfg.unqualified_base_limit, cfg.n_base_limit = 15, 60, 5
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    sizes, out = roundtrip(gpu_engine, 0, bytes(memoryview(t1)[:n1]), bytes(memoryview(t2)[:n2]), store_overlap=True, cfg=cfg, tag="six_streams")
    assert all(sizes) and sorted(out) == list(range(6)), sizes


def test_empty_stream_between_two_others(gpu_engine):
    """nothing good, everything bad (stream 0 empty, stream 1 not): and paired, streams 0 and 3 empty between 1 and 4"""
    rng = np.random.default_rng(4800)
    text = b"".join(ordinary(rng, 2 * M + 700, L=100))
    cfg = pass_all()
    cfg.seq_len_req = 500
    sizes, out = roundtrip(gpu_engine, 0, text, cfg=cfg, tag="good_stream_empty")
    assert sizes[0] == 0 and sizes[1] > len(text) and sizes[2:] == [0, 0, 0, 0], sizes
    text2 = b"".join(ordinary(rng, 3 * M, L=100)[:text.count(b"\n") // 4])
    cfg = pass_all(True)
    cfg.seq_len_req = 500
    sizes, out = roundtrip(gpu_engine, 0, text, text2, cfg=cfg, tag="good_streams_empty_paired")
    assert sizes[0] == 0 and sizes[3] == 0 and sizes[1] > len(text) and sizes[4] > len(text2), sizes
    assert sorted(out) == [1, 4]


def test_more_than_256_members(gpu_engine):
    """gz_offsets_kernel scans a stream's member sizes 256 at a time and carries the sum over"""
    d = synth.make_pairs(14000, 150, seed=4900, dirty=True)
    t1, n1 = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    s = single(gpu_engine, 0, bytes(memoryview(t1)[:n1]), "more_than_256_members")
    assert len(s["members"]) > 256 + 16


def test_slot_reuse(gpu_engine):
    """the staging buffer is not cleared between calls: a one-byte tail member where a large stream just was, and back; then the
    same small case on every slot"""
    small = sized(5100, M + 1)
    a = stored_case(gpu_engine, 1, "reuse_large")
    b = single(gpu_engine, 1, small, "reuse_small")
    c = stored_case(gpu_engine, 1, "reuse_large_again")
    assert [a[q]["members"] for q in (0, 1)] == [c[q]["members"] for q in (0, 1)]
    assert b["members"][-1][2] == 1
    for slot in (0, 1, 2):
        assert single(gpu_engine, slot, small, "reuse_slot_%d" % slot)["members"] == b["members"]


def test_level_0_is_refused(gpu_engine):
    """aqc_compress(level = 0): AQC_ERR_UNSUPPORTED, and nothing to fetch"""
    text = sized(5200, 3000)
    gpu_engine.set_config(pass_all())
    gpu_engine.reset_stats()
    info = gpu_engine.frame(0, pad(text), len(text), True)
    gpu_engine.run(0)
    assert gpu_engine.format(0, int(info.n)) == [len(text), 0, 0, 0, 0, 0]
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.compress(0, 0)
    assert e.value.code == -7
    buf = np.zeros(4096, dtype=np.uint8)
    with pytest.raises(capi.AqcError) as e:
        gpu_engine.fetch_gz(0, 0, 0, buf, buf.size)
    assert e.value.code == -5
    assert gpu_engine.compress(0, 1)[0] > 0              # (and the slot is none the worse for it)


# ---- gz_encode_kernel: the same cases at its member size, in a process of their own ---------------------------------------------------
def seg_cases(engine):
    """what the child runs (AQC_GZ_ENCODER=seg): -> {case: per-stream results}"""
    res = {}
    for total in residue_sizes(M_SEG):
        s = single(engine, 0, sized(5000 + total % 97, total), "residue_%d" % total)
        assert s["members"][-1][2] == (total % M_SEG or M_SEG)
        res["residue_%d" % total] = {"0": s["members"]}
    text = short_lines_text("reads_of_5")
    per = lines_per_piece(text, M_SEG)
    assert per[0] > 4096 and len(per) == 2
    res["short_lines_reads_of_5"] = {"0": single(engine, 0, text, "short_lines_reads_of_5")["members"]}
    text = aligned_runs_text()
    runs = [r for r in run_starts(text) if r + 600 <= (len(text) // M_SEG) * M_SEG]
    assert all(any(r % mod == want for r in runs) for mod, want in ALIGNED)
    res["aligned_runs"] = {"0": single(engine, 0, text, "aligned_runs")["members"]}
    out = stored_case(engine, 0)
    res["stored_fallback"] = {str(q): out[q]["members"] for q in out}
    return res


def child_main():
    assert SEG, "the child is for AQC_GZ_ENCODER=seg"
    eng = capi.Engine(0, 3)
    try:
        res = seg_cases(eng)
    finally:
        eng.close()
    print("gzdev-seg-json " + json.dumps(res))


def test_seg_encoder_in_a_child_process(gpu_engine):
    """AQC_GZ_ENCODER=seg is read once per process: one fresh child runs the residues at 65280, the 4096-line limit, runs across
    the 255-byte segment borders and the stored fallback through gz_encode_kernel, and prints its results as one JSON line"""
    if not all(k in TIMES for k in ("residues", "short_lines", "aligned_runs", "stored")):
        # (run alone: take the times of the default encoder's share of the same cases here)
        for total in residue_sizes(M_WAVE):
            with timed("residues"):
                single(gpu_engine, 0, sized(5000 + total % 97, total), "residue_%d" % total)
        with timed("short_lines"):
            single(gpu_engine, 0, short_lines_text("reads_of_5"), "short_lines_reads_of_5")
        with timed("aligned_runs"):
            single(gpu_engine, 0, aligned_runs_text(), "aligned_runs")
        with timed("stored"):
            stored_case(gpu_engine, 0)
    # a few times what the same cases took with the default encoder in this session, and the start of a process and a context
    limit = 5.0 * sum(TIMES[k] for k in ("residues", "short_lines", "aligned_runs", "stored")) + 30.0
    env = dict(os.environ, AQC_GZ_ENCODER="seg")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--seg-child"], env=env, capture_output=True, text=True, timeout=limit)
    sys.stdout.write("".join(l + "\n" for l in p.stdout.splitlines() if l.startswith("gzdev|")))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("gzdev-seg-json ")]
    assert len(line) == 1
    res = json.loads(line[0][len("gzdev-seg-json "):])
    for total in residue_sizes(M_SEG):
        members = res["residue_%d" % total]["0"]
        assert len(members) == -(-total // M_SEG) and members[-1][2] == (total % M_SEG or M_SEG)
        assert sum(m[2] for m in members) == total
    assert [m[2] for m in res["short_lines_reads_of_5"]["0"]][0] == M_SEG
    assert len(res["aligned_runs"]["0"]) == 3 and not any(m[0] for m in res["aligned_runs"]["0"][:2])
    kinds = [m[0] for m in res["stored_fallback"]["0"]]
    assert len(kinds) == 18 and any(kinds) and not any(kinds[:16]), kinds
    assert len(res["stored_fallback"]["1"]) == 1


if __name__ == "__main__":
    if sys.argv[1:] == ["--seg-child"]:
        child_main()
