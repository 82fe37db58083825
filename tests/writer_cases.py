"""Inputs that put the device's text writer (csrc/aqc_fmt.hpp, aqc_fmtcopy.hpp) at its window, piece, plan and list edges, and one
checker for them.  Plain Python and numpy; nothing here reads the reference.

A generator returns (cfg, text1, text2 or None, extra) and ASSERTS, from the text it made and (cover_*) from the ORACLE's results,
that the shapes it is there for are present — so the CPU suite (test_writer_cases_cpu.py) proves without a GPU that the inputs reach
them, and an edit of a generator cannot silently empty a case.  check() frames, runs and formats the texts on the device engine and on
oracle.OracleEngine() and compares verdict records first, then all six streams, byte for byte, in every mode asked for and for every
cut n.  Reference semantics: seqFilter.writeReads (preprocesser.py:206-232), moveBarcodeToName (barcodeprocesser.py:34-45)."""
import numpy as np

from afterqc_amd import capi

# the writer's constants the cases are built around (csrc/aqc_fmt.hpp, aqc_fmtcopy.hpp, aqc_textin.hpp)
FMT_TILE, FMT_SUPER, TXT_BLOCK, GEN_LISTS, FMT_MAXP, GRID_MIN = 128, 8, 256, 256, 10, 48
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LOWER = b"abcdefghijklmnopq"
UPPER = b"ABCDEFGHIJKLMNOPQ"


def pad(data):
    a = np.zeros(len(data) + 4096, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def rand_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def revcomp(s):
    return s.translate(COMP)[::-1]


def quals(rng, n):
    """phred 20 .. 39, no two neighbours alike (test_gpu_merged.quals): a misplaced quality byte does not compare equal"""
    return bytes(53 + int(x) for x in np.cumsum(rng.integers(1, 20, n)) % 20)


def record(name, seq, qual, ends=(b"\n", b"\n", b"\n", b"\n"), plus=b"+"):
    return name + ends[0] + seq + ends[1] + plus + ends[2] + qual + ends[3]


def base_cfg(paired, **kw):
    """every filter off (test_text_framing.passthrough_cfg), then the keywords"""
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.seq_len_req = 0
    cfg.poly_size_limit = cfg.unqualified_base_limit = cfg.n_base_limit = 0
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def record_spans(text):
    """(start, size) of every four-line record of a text whose lines all end in a newline"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert len(nl) % 4 == 0 and (len(text) == 0 or nl[-1] == len(text) - 1)
    ends = nl[3::4] + 1
    starts = np.concatenate([[0], ends[:-1]])
    return starts, ends - starts


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
def frame_run(eng, cfg, t1, t2, slot=0):
    eng.set_config(cfg)
    eng.set_circles([])
    eng.reset_stats()
    if t2 is not None:
        info = eng.frame(slot, pad(t1), len(t1), True, pad(t2), len(t2), True)
    else:
        info = eng.frame(slot, pad(t1), len(t1), True)
    n = int(info.n)
    assert n > 0
    eng.run(slot)
    return info, n, eng.fetch_results(slot)[:n].copy()


def fetch_streams(eng, slot, sizes):
    out = []
    for q, nb in enumerate(sizes):
        buf = np.zeros(nb + 1, dtype=np.uint8)
        if nb:
            eng.fetch_text(slot, q // 3, q % 3, buf, nb)
        out.append(buf[:nb].tobytes())
    return out


def first_difference(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d: got %r, want %r" % (len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40])


def assert_streams(got_sizes, got, want_sizes, want, what):
    for q in range(6):
        assert got[q] == want[q], (what, "stream %d" % q, first_difference(got[q], want[q]))
    assert list(got_sizes) == list(want_sizes), (what, got_sizes, want_sizes)


def merged_expected(res, n, good1, good2):
    """the rule of tests/merged_rule.py on good streams and verdicts: the merged reads of records [0, n) (preprocesser.py:614 selects)"""
    import merged_rule
    g1, g2 = merged_rule.records(good1.decode("latin-1")), merged_rule.records(good2.decode("latin-1"))
    out, k = [], 0
    for i in range(n):
        r = res[i]
        if int(r["flag"]) != capi.GOOD:
            continue
        a, b = g1[k], g2[k]
        k += 1
        corrected = sum(1 for e in range(int(r["n_edits"])) if int(r["edits"][e]["kind"]) in (capi.EDIT_FIX_R1, capi.EDIT_FIX_R2))
        if int(r["overlap_len"]) > 30 and int(r["distance"]) in (0, corrected):
            rec = merged_rule.merged_record(a[0], a[1], a[2], a[3], b[1], b[3], int(r["overlap_len"]))
            if rec is not None:
                out.append(rec)
    return "".join(out).encode("latin-1")


MODES = ("plain", "overlap", "spans", "merged")


def check(eng, cfg, t1, t2, modes, cuts=None):
    """device engine against the oracle engine: verdict records, then the six streams and their sizes, per mode and cut; -> the oracle's
    verdict records"""
    from oracle import oracle
    ora = oracle.OracleEngine()
    info, n, res = frame_run(eng, cfg, t1, t2)
    oinfo, on, ores = frame_run(ora, cfg, t1, t2)
    assert n == on
    # (first: a verdict that differs is not the writer's)
    assert res.tobytes() == ores.tobytes(), "verdict records differ: %s" % np.flatnonzero((res.view(np.uint8).reshape(n, -1) != ores.view(np.uint8).reshape(n, -1)).any(axis=1))[:10]
    paired = t2 is not None
    for cut in (cuts if cuts is not None else sorted({n, n - 1, min(129, n), 1}, reverse=True)):
        want_sizes = ora.format(0, cut, False)
        want = fetch_streams(ora, 0, want_sizes)
        for mode in modes:
            assert mode in MODES
            what = (mode, cut)
            if mode == "plain":
                sizes = eng.format(0, cut, False)
                assert_streams(sizes, fetch_streams(eng, 0, sizes), want_sizes, want, what)
            elif mode == "overlap":
                wo = ora.format(0, cut, True)
                want_o = fetch_streams(ora, 0, wo)
                sizes = eng.format(0, cut, True)
                assert_streams(sizes, fetch_streams(eng, 0, sizes), wo, want_o, what)
            elif mode == "spans":
                sizes, n_ev = eng.format_spans(0, cut, False)
                got = fetch_streams(eng, 0, sizes)
                end = eng.span_end(0, cut)
                for f, chunk in enumerate((t1, t2) if paired else (t1,)):
                    ev = eng.fetch_span_events(0, f, n_ev[f])
                    # the assembled good stream against the ORACLE's
                    good = capi.assemble_spans(chunk, end[f], ev, got[3 * f])
                    assert good == want[3 * f], (what, f, first_difference(good, want[3 * f]))
                    assert got[3 * f + 1] == want[3 * f + 1], (what, f, first_difference(got[3 * f + 1], want[3 * f + 1]))
                    assert sizes[3 * f + 1] == want_sizes[3 * f + 1] and sizes[3 * f + 2] == 0
            elif mode == "merged":
                assert paired
                sizes = eng.format(0, cut, capi.STORE_MERGED)
                got = fetch_streams(eng, 0, sizes)
                wm = list(want)
                wm[2], wm[5] = merged_expected(ores, cut, want[0], want[3]), b""
                assert_streams(sizes, got, [len(x) for x in wm], wm, what)
    ora.close()
    eng.reset_stats()          # (the shared engine's statistics are not left to the next test)
    return ores


def check_expected(eng, cfg, t1, t2, expected, n_want):
    """for the cases too big for the oracle's per-record loop: format(n) against streams built by construction"""
    info, n, res = frame_run(eng, cfg, t1, t2)
    assert n == n_want
    sizes = eng.format(0, n, False)
    got = fetch_streams(eng, 0, sizes)
    for q in range(6):
        assert len(got[q]) == len(expected[q]) and got[q] == expected[q], ("stream %d" % q, first_difference(got[q], expected[q]))
    eng.reset_stats()


def oracle_results(cfg, t1, t2):
    from oracle import oracle
    ora = oracle.OracleEngine()
    info, n, res = frame_run(ora, cfg, t1, t2)
    ora.close()
    return res


# ---- what a record is made of: fmt_build's piece list, restated -------------------------------------------------------------------------
def model_pieces(text, cfg, rr, mate):
    """the piece lists fmt_build makes for the main pass, per record of `text` (file `mate`, 0 or 1), from the framing
    (oracle.frame_text) and the verdict records rr: a list of [(source offset or None for a literal, length), ...]"""
    from oracle import oracle
    records = oracle.frame_text(text, True)[0]
    out = []
    for r, ((no, nl), (so, sl), (po, pl), (qo, ql)) in enumerate(records[:len(rr)]):
        v = rr[r]
        flag = int(v["flag"])
        st, ln = (int(v["start1"]), int(v["len1"])) if mate == 0 else (int(v["start2"]), int(v["len2"]))
        bad = flag != capi.GOOD
        moved = bool(cfg.barcode) and flag not in (capi.BADBCD1, capi.BADBCD2)
        ps = []
        if bad or moved:
            ps.append((None, 1 + (len(capi.FLAG_NAMES[flag]) if bad else 0)))
        if moved:
            code = (int(v["barcode"]) & 15) if mate == 0 else (int(v["barcode"]) >> 4)
            b = min(max(code - 2 + cfg.barcode_length if cfg.paired else cfg.barcode_length, 0), sl)
            c = text[no:no + nl].find(b":")
            c = nl - 1 if c < 0 else c
            ps += [(so, b), (no + c, nl - c)]
        elif bad:
            ps.append((no + 1, nl - 1))
        else:
            ps.append((no, nl))
        ps.append((no + nl, 1) if so == no + nl + 1 else (None, 1))
        ps.append((so + st, ln))
        ps.append((so + sl, 1) if po == so + sl + 1 else (None, 1))
        ps.append((po, pl))
        ps.append((po + pl, 1) if qo == po + pl + 1 else (None, 1))
        ps.append((qo + st, ln))
        ps.append((qo + ql, 1) if (st + ln == ql and text[qo + ql:qo + ql + 1] == b"\n") else (None, 1))
        merged = []
        for src, n in ps:
            if n <= 0:
                continue
            if merged and src is not None and merged[-1][0] is not None and merged[-1][0] + merged[-1][1] == src:
                merged[-1] = (merged[-1][0], merged[-1][1] + n)
            else:
                merged.append((src, n))
        out.append(merged)
    return out


def piece_items(n):
    return ((n + 15) >> 4) + (1 if n >= GRID_MIN else 0) if n >= 16 else (1 if n else 0)


def mate_patches(v, mate):
    """byte patches the walk's edits make in one mate's record: a FIX of that mate is two (base, quality), a MASK one"""
    fix = capi.EDIT_FIX_R1 if mate == 0 else capi.EDIT_FIX_R2
    kinds = [int(v["edits"][e]["kind"]) for e in range(int(v["n_edits"]))]
    return 2 * sum(k == fix for k in kinds) + sum(k == capi.EDIT_MASK for k in kinds)


# ---- 1. small_own: records of 8 .. 80 bytes that go out as their own bytes, at every source alignment ---------------------------------
SMALL_SIZES = range(8, 81)


def small_file(letters, seed):
    """records of every size in SMALL_SIZES starting at every offset mod 16; names of 1 .. 17 bytes: size = name + 2 x read + 5"""
    rng = np.random.default_rng(seed)
    need = {(s, a) for s in SMALL_SIZES for a in range(16)}
    recs, pos, turn = [], 0, seed
    while need:
        a = pos % 16
        here = [s for s in SMALL_SIZES if (s, a) in need]
        if not here:
            # a filler that moves on to an alignment something is still wanted at
            here = [s for s in SMALL_SIZES if any((t, (pos + s) % 16) in need for t in SMALL_SIZES)]
        s = here[turn % len(here)]
        turn += 1
        need.discard((s, a))
        nls = [k for k in range(1, 18) if (s - 5 - k) % 2 == 0 and s - 5 - k >= 2]
        nlen = nls[turn % len(nls)]
        L = (s - 5 - nlen) // 2
        recs.append(record(b"@" + letters[:nlen - 1], rand_seq(rng, L), quals(rng, L)))
        assert len(recs[-1]) == s
        pos += s
    return recs


def small_own(paired):
    f1 = small_file(LOWER, 3)
    f2 = small_file(UPPER, 8) if paired else None
    if paired:
        # the two files out of step: other sizes and alignments side by side; the shorter one is topped up
        assert [len(r) for r in f1[:50]] != [len(r) for r in f2[:50]]
        while len(f2) < len(f1):
            f2.append(f2[len(f2) % 97])
        while len(f1) < len(f2):
            f1.append(f1[len(f1) % 97])
    t1, t2 = b"".join(f1), (b"".join(f2) if paired else None)
    for t in (t1, t2) if paired else (t1,):
        starts, sizes = record_spans(t)
        assert {(int(s), int(a) % 16) for s, a in zip(sizes, starts)} >= {(s, a) for s in SMALL_SIZES for a in range(16)}
        assert {8, 14, 15, 16, 17, 31, 32, 33, 47, 48, 49, 80} <= set(sizes.tolist())
    return base_cfg(paired), t1, t2, dict(n=len(f1))


def cover_small_own(cfg, t1, t2, res):
    assert (res["flag"] == capi.GOOD).all() and (res["n_edits"] == 0).all()       # the expected output is the input itself


# ---- 2. patched_own: own-bytes records with 0 .. 6 byte patches -------------------------------------------------------------------------
R1, R2, MK = "fix_r1", "fix_r2", "mask"
PATTERNS = [[], [R1], [R2], [MK], [R1, R1], [R2, R2], [R1, R2], [R1, MK], [R1, R1, MK], [R2, R2, MK], [R1, R1, R1], [R2, R2, R2],
            [R1, R2, MK], [MK, MK, MK], [R1, R1, R2]]


def patched_own(mask_mismatch=0, no_correction=0, n=600):
    """pairs of 80 and 100 bases from one insert of the same length (the mates overlap fully), 0 .. 3 planted mismatches each: R1 low
    against R2 high (a FIX of read 1), the reverse, both middling (nothing, or a MASK); at overlap index 0, the last one, and where the
    quality byte lands in the record's last 16 bytes — of read 1 (high indices) and of read 2 (low ones)"""
    rng = np.random.default_rng(21)
    f1, f2 = [], []
    for i in range(n):
        L = (80, 100)[i % 2]
        pat = PATTERNS[(i // 2) % len(PATTERNS)]
        sets = [(0, L - 1, L // 2), (L - 1, L - 2, L - 15), (0, 1, 14), (L - 16, 15, L - 3), (7, L - 8, 40), (L - 1, 0, 3), (L - 14, L - 9, L - 2), (2, 13, 8)]
        at = sets[(i // (2 * len(PATTERNS))) % len(sets)][:len(pat)]
        F = bytearray(rand_seq(rng, L))
        r1, r2 = bytearray(F), bytearray(revcomp(bytes(F)))
        q1, q2 = bytearray(quals(rng, L)), bytearray(quals(rng, L))
        for kind, o in zip(pat, at):
            r2[L - 1 - o] = b"CGTA"[b"ACGT".index(r2[L - 1 - o])]
            lo, hi = ord("#"), ord("I")
            q1[o], q2[L - 1 - o] = {R1: (lo, hi), R2: (hi, lo), MK: (ord("5"), ord("5"))}[kind]
        f1.append(record(b"@" + LOWER[:i % 17], bytes(r1), bytes(q1)))
        f2.append(record(b"@" + UPPER[:(i // 3) % 17], bytes(r2), bytes(q2)))
    cfg = base_cfg(True, seq_len_req=35, poly_size_limit=35, allow_mismatch_in_poly=2, qualified_quality_phred=15, unqualified_base_limit=60,
                   n_base_limit=5, mask_mismatch=mask_mismatch, no_correction=no_correction)
    return cfg, b"".join(f1), b"".join(f2), dict(n=n)


def cover_patched_own(cfg, t1, t2, res):
    good = res["flag"] == capi.GOOD
    assert good.sum() >= 0.95 * len(res)
    assert {0, 1, 2, 3} <= set(res["n_edits"][good].tolist()) or cfg.no_correction and not cfg.mask_mismatch
    # (three mismatches close together near the overlap's start lose the overlap: such a pair is written as it stands)
    ov = res["overlap_len"][good]
    assert set(ov.tolist()) <= {0, 80, 100} and (ov >= 80).mean() >= 0.85 and set(res["distance"][good][ov >= 80].tolist()) == {0, 1, 2, 3}
    counts = {k: 0 for k in range(7)}
    late = 0
    spans = [record_spans(t1), record_spans(t2)]
    for i in np.flatnonzero(good):
        v = res[i]
        for mate in (0, 1):
            counts[mate_patches(v, mate)] += 1
            # the last patch: the quality byte of the edit nearest the read's end
            ln, ov = int(v["len1"] if mate == 0 else v["len2"]), int(v["overlap_len"])
            fix = capi.EDIT_FIX_R1 if mate == 0 else capi.EDIT_FIX_R2
            pp = [(ln - ov + int(e["o"])) if mate == 0 else (ln - 1 - int(e["o"])) for e in v["edits"][:int(v["n_edits"])] if int(e["kind"]) in (fix, capi.EDIT_MASK)]
            size = int(spans[mate][1][i])
            if pp and size % 16 and size - 1 - ln + max(pp) >= size - 16:
                late += 1
    if not cfg.no_correction:
        # four patches: the most a whole plan holds; five (2 FIX + 1 MASK) and six (3 FIX) take the overflow path
        assert counts[4] >= 16 and counts[6] >= 16, counts
        assert late >= 16
    if cfg.mask_mismatch:
        assert (counts[5] >= 16 or cfg.no_correction) and counts[1] >= 16 and counts[3] >= 16, counts
    if cfg.no_correction:
        kinds = {int(e["kind"]) for v in res for e in v["edits"][:int(v["n_edits"])]}
        assert not kinds & {capi.EDIT_FIX_R1, capi.EDIT_FIX_R2}
    return counts


# ---- 3. piece_lengths: trimmed records, the written read of every length around the window edges ----------------------------------------
WRITTEN = list(range(1, 18)) + list(range(30, 35)) + list(range(46, 51)) + list(range(62, 67))
TRIM_FRONT, TRIM_TAIL = 2, 3


def piece_lengths(paired, seq_len_req=0):
    """trim_front 2, trim_tail 3: every record is three pieces and more (the name and its newline, the bases, the rest).  The written
    read has every length of WRITTEN at every source alignment (mod 16) of its first base, in both files.  Every fourth pair (of the
    longest pairs every second) is made bad, so that literal pieces of 7, 8 and 12 bytes occur: a polyX run ('@BADPOL'), low qualities
    ('@BADLQC'), N bases ('@BADNCT'); pairs: five mismatches behind column 50 of the overlap ('@BADDIFF', distance > 3), and a
    periodic read 1 with one changed base whose shorter mate fits both the first diagonal, with that mismatch, and the reads' ends,
    without it — the walk then counts fewer mismatches than the search did ('@BADMISMATCH'); with seq_len_req, '@BADLEN'"""
    rng = np.random.default_rng(31 + (1 if paired else 0))
    f1, f2 = [], []
    pos, ones = [0, 0], [0, 0]
    i = 0
    for rep in range(2 if paired else 1):
        # (in a shuffled order: walking the alignments in steps makes the name lengths that reach them fall into step, too)
        order = [(w, a) for w in WRITTEN for a in range(16)]
        rng.shuffle(order)
        for w, a in order:
            L = w + TRIM_FRONT + TRIM_TAIL
            s1, s2 = bytearray(rand_seq(rng, L)), bytearray(rand_seq(rng, L))
            long_pair = paired and w >= 62
            if i % 4 == 3 or (long_pair and i % 2):
                kind = (i // 2) % 5 if long_pair else (i // 4) % 3
                tgt = s1 if (i // 16) % 2 == 0 or not paired else s2
                if kind == 0 and w >= 30:
                    tgt[TRIM_FRONT + 2:TRIM_FRONT + 27] = b"A" * 25
                elif kind == 2 and w >= 5:
                    tgt[TRIM_FRONT:TRIM_FRONT + 5] = b"N" * 5
                elif kind == 3:
                    s2 = bytearray(revcomp(bytes(s1)))
                    for col in range(51, 56):              # (columns of the diagonal that pairs the trimmed mates: read 1's base 3 + col)
                        s2[L - 1 - (3 + col)] = b"CGTA"[b"ACGT".index(s2[L - 1 - (3 + col)])]
                elif kind == 4:
                    t1_ = bytearray((b"ACGT" * 20)[:w])
                    t1_[1] = ord("T")
                    s1 = bytearray(b"GA" + bytes(t1_) + b"TCA")
                    s2 = bytearray(b"CT" + revcomp(bytes(t1_[8:])) + b"GAG")
            q1, q2 = bytearray(quals(rng, len(s1))), bytearray(quals(rng, len(s2)))
            if (i % 4 == 3 or (long_pair and i % 2)) and ((i // 2) % 5 if long_pair else (i // 4) % 3) == 1 and w >= 8:
                (q1 if (i // 16) % 2 == 0 or not paired else q2)[TRIM_FRONT:TRIM_FRONT + 7] = b"#" * 7
            for k, (fl, letters, sq, ql) in enumerate(((f1, LOWER, s1, q1), (f2, UPPER, s2, q2))):
                # the name's length puts the first written base at alignment a (file 1: five further on)
                want = (a + 5 * k) % 16
                nlen = (want - pos[k] - 1 - TRIM_FRONT) % 16
                nlen = nlen if nlen else 16
                if nlen == 1:
                    ones[k] += 1
                    nlen = 17 if ones[k] % 2 else 1
                fl.append(record(b"@" + letters[:nlen - 1], bytes(sq), bytes(ql)))
                assert (pos[k] + nlen + 1 + TRIM_FRONT) % 16 == want
                pos[k] += len(fl[-1])
            i += 1
    cfg = base_cfg(paired, trim_front=TRIM_FRONT, trim_tail=TRIM_TAIL, trim_front2=TRIM_FRONT, trim_tail2=TRIM_TAIL, seq_len_req=seq_len_req,
                   poly_size_limit=20, allow_mismatch_in_poly=0, qualified_quality_phred=15, unqualified_base_limit=5, n_base_limit=3)
    t1, t2 = b"".join(f1), (b"".join(f2) if paired else None)
    from oracle import oracle
    for t in (t1, t2) if paired else (t1,):
        recs = oracle.frame_text(t, True)[0]
        seen = {(sl - TRIM_FRONT - TRIM_TAIL, (so + TRIM_FRONT) % 16) for (_, (so, sl), _, _) in recs}
        assert seen >= {(w, a) for w in WRITTEN for a in range(16)}
        assert {nl for ((_, nl), _, _, _) in recs} == set(range(1, 18))
    return cfg, t1, t2, dict(n=len(f1))


def cover_piece_lengths(cfg, t1, t2, res):
    flags = res["flag"].tolist()
    want = [capi.BADPOL, capi.BADLQC, capi.BADNCT] + ([capi.BADDIFF, capi.BADMISMATCH] if t2 is not None else []) + ([capi.BADLEN] if cfg.seq_len_req else [])
    for f in want:
        assert flags.count(f) >= 8, (capi.FLAG_NAMES[f], flags.count(f))
    assert flags.count(capi.GOOD) >= len(flags) // 3
    # the written slices are the trimmed ones, and no record goes out as one piece
    assert (res["start1"] == TRIM_FRONT).all()
    pieces = [p for t, m in ((t1, 0), (t2, 1)) if t is not None for ps in model_pieces(t, cfg, res, m) for p in ps]
    # the flag literals: '@BADPOL' and its like 7 bytes, '@BADDIFF' 8, '@BADTRIM1' 9, '@BADMISMATCH' 12 (the pairs' flags)
    literals = {n for src, n in pieces if src is None}
    assert {7, 9} <= literals and (t2 is None or {8, 12} <= literals), sorted(literals)
    lens = {n for _, n in pieces}
    assert set(range(1, 16)) <= lens                    # short pieces of every length: stored as 8 + 4 + 2 + 1


# ---- 4. barcode_names: moveBarcodeToName on names of every shape ------------------------------------------------------------------------
def barcode_name_list():
    """(class, name) for the barcode writer: name[name.find(':'):] with the colon in each 16-byte step, at the last byte, nowhere"""
    fill = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_-./abcdefghij"
    out = []
    for n in range(1, 71):                              # every length, a colon at a place that moves with it
        nm = bytearray(b"@" + fill[:n - 1])
        if n > 1:
            nm[1 + (7 * n) % (n - 1)] = ord(":")
        out.append(("length", bytes(nm)))
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 50):        # no colon at all: find() == -1 slices the last character
        out.append(("no_colon", b"@" + fill[:n - 1]))
    for c in (1, 2, 14, 15, 16, 17, 30, 31, 32, 33):     # the first colon at index c, more name behind it
        nm = bytearray(b"@" + fill[:c + 9])
        nm[c] = ord(":")
        out.append(("first_colon", bytes(nm)))
    for n in (2, 16, 17, 32, 33, 48, 49, 64):            # ... and at the last byte
        out.append(("first_colon", b"@" + fill[:n - 2] + b":"))
    for nm in (b"@a:b:c", b"@::", b"@:", b"@M01:23:FC:1:1101:5:6 1:N:0:AC", b"@" + fill[:15] + b"::" + fill[:20] + b":x", b"@ab:" + fill[:28] + b":" + fill[:5],
               b"@" + fill[:16] + b":" + fill[:15] + b":", b"@x:::::::::::::::y", b"@" + fill[:31] + b"::" + fill[:30] + b":" + fill[:3]):
        out.append(("several_colons", nm))
    for tail in range(1, 18):                           # name[cpos:] of every length 1 .. 17
        out.append(("tail", b"@" + fill[:(3 * tail) % 19] + b":" + fill[:tail - 1]))
    return out


def barcode_names(paired):
    """reads = 12 random bases + CAGTA + at least 13 bases (pairs: the template of make_golden.py's move_barcode pairs); per name two
    good reads and one whose barcode is not found — no verify sequence, or a read of 17 or 18 bases — which keeps its name"""
    rng = np.random.default_rng(41 + (1 if paired else 0))
    verify = b"CAGTA"
    f1, f2, classes = [], [], []
    names = barcode_name_list()
    for rep in range(3):
        for j, (cls, nm) in enumerate(names):
            L = (30, 44, 61, 35)[(j + rep) % 4]
            b1, b2 = rand_seq(rng, 12), rand_seq(rng, 12)
            if paired:
                tpl = b1 + verify + rand_seq(rng, 20 + (j % 3) * 25) + revcomp(b2 + verify)
                r1 = (tpl + rand_seq(rng, 2 * L))[:L]
                r2 = (revcomp(tpl) + rand_seq(rng, 2 * L))[:L]
            else:
                r1, r2 = b1 + verify + rand_seq(rng, L - 17), b""
            if rep == 2:
                kind = j % 3
                if kind == 0:
                    r1 = r1[:12] + b"GTCAT" + r1[17:]
                elif not paired:
                    r1 = r1[:16 + kind]                  # 17 and 18 bases
                else:
                    r2 = r2[:12] + b"GTCAT" + r2[17:]
            n2 = nm[:1] + nm[1:].swapcase() if len(nm) > 1 else nm
            f1.append(record(nm, r1, quals(rng, len(r1))))
            f2.append(record(n2, r2, quals(rng, len(r2))))
            classes.append(cls)
    cfg = base_cfg(paired, barcode=1)
    t1, t2 = b"".join(f1), (b"".join(f2) if paired else None)
    # the shapes, from the text
    for cls, nm in names:
        assert nm.startswith(b"@") and b"\n" not in nm
    assert {len(nm) for _, nm in names} >= set(range(1, 71))
    assert {len(nm) for c, nm in names if c == "no_colon"} == {1, 2, 15, 16, 17, 31, 32, 33, 50} and all(b":" not in nm for c, nm in names if c == "no_colon")
    assert {nm.find(b":") for c, nm in names if c == "first_colon"} >= {1, 2, 14, 15, 16, 17, 30, 31, 32, 33}
    assert sum(nm.find(b":") == len(nm) - 1 for _, nm in names) >= 8
    assert {len(nm) - nm.find(b":") for _, nm in names if b":" in nm} >= set(range(1, 18))
    return cfg, t1, t2, dict(n=len(f1), classes=classes)


def cover_barcode_names(cfg, t1, t2, res, classes):
    flags = res["flag"]
    for cls in ("length", "no_colon", "first_colon", "several_colons", "tail"):
        mine = np.array([c == cls for c in classes])
        assert (flags[mine] == capi.GOOD).sum() >= 8, cls
        assert np.isin(flags[mine], (capi.BADBCD1, capi.BADBCD2)).sum() >= 8, cls
    assert np.isin(flags, (capi.GOOD, capi.BADBCD1, capi.BADBCD2)).all()


# ---- 5. stripped_line_ends: newlines that are not taken from the text ------------------------------------------------------------------
def stripped_line_ends(paired, barcode, last="complete"):
    """each of the 16 subsets of the four lines ends in '\\r' (and, second variant, ' \\t') before its newline — the writer's newline is a
    literal piece of its own there; good and bad (N bases) records, names renamed by flag and by barcode: up to FMT_MAXP = 10 pieces.
    last: the file's last record 'complete', 'no_newline' (no final newline) or 'blanks' (trailing blanks and no newline)"""
    rng = np.random.default_rng(51 + 2 * paired + barcode)
    f1, f2 = [], []
    i = 0
    for rep in range(3):
        for variant in (b"\r", b" \t"):
            for subset in range(16):
                for bad in (0, 1):
                    ends = tuple((variant if subset >> ln & 1 else b"") + b"\n" for ln in range(4))
                    L = 40 + (i * 7) % 31
                    b1, b2 = rand_seq(rng, 12), rand_seq(rng, 12)
                    tpl = b1 + b"CAGTA" + rand_seq(rng, 30) + revcomp(b2 + b"CAGTA")
                    r1 = bytearray((tpl + rand_seq(rng, 2 * L))[:L] if paired else b1 + b"CAGTA" + rand_seq(rng, L - 17))
                    r2 = bytearray((revcomp(tpl) + rand_seq(rng, 2 * L))[:L])
                    if bad:
                        r1[20:26] = b"NNNNNN"
                    f1.append(record(b"@r%d:%s" % (i, LOWER[:i % 9]), bytes(r1), quals(rng, L), ends))
                    f2.append(record(b"@R%d:%s" % (i, UPPER[:i % 5]), bytes(r2), quals(rng, L), ends[1:] + ends[:1]))
                    i += 1
    t1, t2 = b"".join(f1), b"".join(f2)
    tail = {"complete": lambda t: t, "no_newline": lambda t: t[:-1], "blanks": lambda t: t[:-1] + b" \t "}[last]
    cfg = base_cfg(paired, barcode=barcode, n_base_limit=3)
    return cfg, tail(t1), (tail(t2) if paired else None), dict(n=len(f1))


def cover_stripped_line_ends(cfg, t1, t2, res):
    flags = res["flag"].tolist()
    assert flags.count(capi.GOOD) >= 90 and flags.count(capi.BADNCT) >= 90 and flags.count(capi.GOOD) + flags.count(capi.BADNCT) == len(flags)
    np_seen = {}
    for t, m in ((t1, 0), (t2, 1)):
        if t is not None:
            for ps, f in zip(model_pieces(t, cfg, res, m), flags):
                np_seen.setdefault(len(ps), set()).add(f == capi.GOOD)
    # every stripped line is a literal newline piece; a renamed record has one piece more, two with a moved barcode
    assert max(np_seen) == (FMT_MAXP if cfg.barcode else 9) and {8, 9} <= set(np_seen), sorted(np_seen)
    assert max(np_seen) <= FMT_MAXP
    return np_seen


# ---- 6. long_records --------------------------------------------------------------------------------------------------------------------
def long_records(paired, trim_tail=0):
    """reads of 230, 255, 256, 300, 520 and 1000 bases (records over 512 bytes are listed for the general kernel; with trim_tail = 1 every
    record is), a 600-byte name with a 40-base read, and records of just under and just over 1 KiB: 64 against 65 work items, the most a
    plan holds"""
    rng = np.random.default_rng(61)
    f1, f2 = [], []
    shapes = [(5 + i % 13, L) for i, L in enumerate([230, 255, 256, 300, 520, 1000] * 6)] + [(600, 40)] * 4
    shapes += [(n, L) for L in range(464, 500, 3) for n in (3, 18, 30)]
    for j, (nlen, L) in enumerate(shapes):
        nm = (b"@" + (LOWER + UPPER) * 20)[:nlen]
        f1.append(record(nm, rand_seq(rng, L), quals(rng, L)))
        f2.append(record(nm.swapcase(), rand_seq(rng, L), quals(rng, L)))
    cfg = base_cfg(paired, trim_tail=trim_tail, trim_tail2=trim_tail)
    t1, t2 = b"".join(f1), (b"".join(f2) if paired else None)
    sizes = record_spans(t1)[1]
    assert sizes.max() > 2000 and sizes.min() < 700
    return cfg, t1, t2, dict(n=len(f1))


def cover_long_records(cfg, t1, t2, res):
    assert (res["flag"] == capi.GOOD).all()
    items = [sum(piece_items(n) for _, n in ps) for ps in model_pieces(t1, cfg, res, 0)]
    sizes = record_spans(t1)[1]
    if cfg.trim_tail:
        assert 64 in items and 65 in items and max(items) > 100, sorted(set(items))[-12:]
    else:
        # (one piece each: 64 work items up to 1008 bytes, 65 from 1009 on)
        assert (sizes > 512).sum() >= 30 and (sizes <= 512).sum() >= 4 and 64 in items and 65 in items and max(items) > 100, sorted(set(items))[-12:]


# ---- 7. index_records: aqc_format_plain ---------------------------------------------------------------------------------------------------
def index_records(n):
    """two index texts of n records: 8 .. 80 bytes at every alignment (small_file), then a few of 470 .. 540 bytes, then small ones again"""
    rng = np.random.default_rng(71)
    out = []
    for letters, seed in ((LOWER, 5), (UPPER, 6)):
        recs = small_file(letters, seed)
        n_small = len(recs)
        for j in range(24):
            L = 225 + 3 * j + (seed % 2)
            recs.append(record(b"@idx%d" % j, rand_seq(rng, L), quals(rng, L)))
        assert n >= len(recs), "the verdict run is too short for the index records: %d" % len(recs)
        recs += [recs[k % n_small] for k in range(n - len(recs))]
        text = b"".join(recs)
        starts, sizes = record_spans(text)
        assert {(int(s), int(a) % 16) for s, a in zip(sizes, starts)} >= {(s, a) for s in SMALL_SIZES for a in range(16)}
        big = set(sizes.tolist())
        assert any(470 <= s <= 496 for s in big) and any(496 < s <= 512 for s in big) and any(s > 512 for s in big)
        out.append(text)
    return out


def index_verdict_run(store):
    """the pair run whose verdicts route the index records: piece_lengths twice over (good and bad of every flag), or, for the overlap
    store, patched_own (pairs that overlap)"""
    if store:
        return patched_own(0, 0, n=1500)
    cfg, t1, t2, extra = piece_lengths(True)
    return cfg, t1 + t1, t2 + t2, dict(n=2 * extra["n"])


# ---- 8. many_tiles ----------------------------------------------------------------------------------------------------------------------
def many_tiles_a():
    """257 x 128 + 1 records, every one listed (trim_tail = 1): tile t and tile t + 256 append to the same general list, and tile 256 is
    the first to do so; sizes vary from record to record.  -> expected streams by construction"""
    n = (GEN_LISTS + 1) * FMT_TILE + 1
    rng = np.random.default_rng(81)
    seq = rand_seq(rng, 4096)
    ql = quals(rng, 4096)
    recs, good, bad = [], [], []
    for i in range(n):
        L, o = 2 + (i * 7) % 61, (i * 13) % 4000
        nm = b"%d" % i
        recs.append(record(b"@" + nm, seq[o:o + L], ql[o:o + L]))
        # (a read that the trim leaves fewer than five bases is BADTRIM1, preprocesser.py:455-466)
        if L - 1 < 5:
            bad.append(record(b"@BADTRIM1" + nm, seq[o:o + L - 1], ql[o:o + L - 1]))
        else:
            good.append(record(b"@" + nm, seq[o:o + L - 1], ql[o:o + L - 1]))
    assert len(bad) > 2 * GEN_LISTS
    return base_cfg(False, trim_tail=1), b"".join(recs), None, dict(n=n, expected=[b"".join(good), b"".join(bad), b"", b"", b"", b""])


MANY_B_LEN_REQ = 2


def many_tiles_b():
    """TXT_BLOCK x 8 x FMT_SUPER x FMT_TILE + 300 records = 256 x 8 super-tiles of 8 x 128 records and a little more: the scan of the
    super-tiles' sums (fmt_tile_bases_kernel) takes TXT_BLOCK x 8 entries per round, so this is the smallest chunk with a second round.
    Reads of 1 and 2 bases alternate in a fixed pattern on either side of seq_len_req = 2, so that the good and the bad stream both
    carry bytes across the round.  Records of 9 .. 11 bytes, lines of under 3 bytes on average: more lines than the line table is first
    sized for (bytes / 16 + 4096) — the chunk is on the re-index path of test_device_reindexes_a_chunk_of_very_short_lines.
    -> expected streams by construction (joins)"""
    n = TXT_BLOCK * 8 * FMT_SUPER * FMT_TILE + 300
    recs = [b"@%d\nAC\n+\nII\n" % d for d in range(10)] + [b"@%d\nG\n+\nI\n" % d for d in range(10)]
    outs = [b"@%d\nAC\n+\nII\n" % d for d in range(10)] + [b"@BADLEN%d\nG\n+\nI\n" % d for d in range(10)]
    # the pattern: period 7, three short reads in it (so tiles and super-tiles do not all hold the same mix)
    short = np.array([(i % 7) in (1, 4, 5) for i in range(n)])
    idx = (np.arange(n) % 10) + 10 * short
    text = b"".join([recs[k] for k in idx])
    good = b"".join([outs[k] for k in idx[~short]])
    bad = b"".join([outs[k] for k in idx[short]])
    assert len(text) / (4 * n) < 16 and len(good) > 0 and len(bad) > 0
    # both streams grow on both sides of the round's border
    border = TXT_BLOCK * 8 * FMT_SUPER * FMT_TILE
    assert short[:border].any() and (~short[:border]).any() and short[border:].any() and (~short[border:]).any()
    return base_cfg(False, seq_len_req=MANY_B_LEN_REQ), text, None, dict(n=n, expected=[good, bad, b"", b"", b"", b""])
