"""Texts that put the device's text-in stage (csrc/aqc_textin.hpp: text_index_kernel, frame_records_kernel, frame_finish_kernel,
parse_names_kernel) at every border of its hand-built geometry, and the census that proves they do.  Plain Python and numpy; nothing
here needs a GPU or reads the reference.  The CPU suite (test_text_border_cases_cpu.py) asserts the builders' preconditions, the
device suite (test_gpu_text_borders.py) frames the texts and compares with the oracle (oracle.frame_text, OracleEngine.frame).

Geometry of the index pass: a lane loads 16-byte PIECEs; one load of a wave is a 1 KiB ROW; 8 rows are an 8 KiB SUB-tile (the
prefetch step); 32 rows a WAVE's 32 KiB; 4 waves a 128 KiB TILE; the look-back walks HOP = 64 tiles at a time.  The class of a border
is the coarsest of these it belongs to.  "The byte before this newline is blank" (LINE_WS) crosses each class by another mechanism.

Events at a border at byte B (border_census):
  E1   '\\n' at B-1 (the line ends with the last byte before the border)
  E2   '\\n' at B, a non-blank byte at B-1
  E3s  '\\n' at B, one ' ' at B-1          E3r  the same with '\\r'   (the strip crosses the border)
  E4a  "\\t \\r" at B-2..B, '\\n' at B+1     E4b  "\\t \\r" at B-1..B+1, '\\n' at B+2   (a blank run straddles the border)
  E5   the pieces before and behind B hold 8 line ends each (one-base records "@\\nA\\n+\\nI\\n" laid over the border)

What chance gave before these cases: the census of test_text_framing.py::test_device_framing_large_random's text (6.62 MB, 51 tiles,
80000 line ends; printed by test_text_border_cases_cpu.py::test_census_of_the_large_random_text) counts, as (class: E1 E2 E3s E3r
E4a E4b E5) summed over the four lines — two line ends at the 150 wave borders, neither with a blank before it; one at the 50 tile
borders; no second look-back hop (that takes more than 64 tiles of which none has published its prefix):
  piece: 4919 2151  907  922  916  922  0
  row:     73   29   10   10    7   16  0
  sub:      8    6    1    2    3    2  0
  wave:     1    1    0    0    0    0  0
  tile:     0    0    0    0    1    0  0
Name parser: the names of name_cases() are printable ASCII plus blank and tab.  Bytes >= 0x80 and 0x1c-0x1f (which a str pattern's
\\S and int() treat as blanks) are out of scope."""
import random
import re

import numpy as np

from afterqc_amd import capi, fastq

PIECE, ROW, SUB, WAVE_BYTES, TILE, HOP = 16, 1024, 8192, 32768, 131072, 64
CLASSES = ("piece", "row", "sub", "wave", "tile")
EVENTS = ("E1", "E2", "E3s", "E3r", "E4a", "E4b")
TAILS = (b"", b"\r", b" ", b"\t \r")
# (event: bytes between the line and its '\n', where the '\n' lands relative to the border)
EVENT_SHAPE = {"E1": (b"", -1), "E2": (b"", 0), "E3s": (b" ", 0), "E3r": (b"\r", 0), "E4a": (b"\t \r", 1), "E4b": (b"\t \r", 2)}
ONE_BASE = b"@\nA\n+\nI\n"
MAX_FILLER = 160           # no filler or target record is longer (asserted where they are made)


def header_constants(path):
    """TXT_BLOCK, IDX_K, IDX_SUB as aqc_textin.hpp states them"""
    src = open(path).read()
    return {k: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % k, src).group(1)) for k in ("TXT_BLOCK", "IDX_K", "IDX_SUB")}


def border_class(b):
    """the coarsest border class byte offset b is a border of (None: not a border, or the start of the text)"""
    if b <= 0 or b % PIECE:
        return None
    for name, size in (("tile", TILE), ("wave", WAVE_BYTES), ("sub", SUB), ("row", ROW)):
        if b % size == 0:
            return name
    return "piece"


def border_events(text):
    """[(B, line of the record 0..3, event)] over every line end of `text`, and (B, None, "E5") per border with full pieces around it"""
    a = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    out = []
    blank = a < 0x21
    for i in np.flatnonzero((nl % PIECE == PIECE - 1) | (nl % PIECE <= 2)):
        p, line = int(nl[i]), int(i) % 4
        if p % PIECE == PIECE - 1:
            out.append((p + 1, line, "E1"))
        elif p % PIECE == 0 and p > 0:
            if not blank[p - 1]:
                out.append((p, line, "E2"))
            elif p > 1 and not blank[p - 2] and a[p - 1] in (32, 13):
                out.append((p, line, "E3s" if a[p - 1] == 32 else "E3r"))
        elif p >= 4 and p % PIECE and text[p - 3:p] == b"\t \r" and not blank[p - 4]:
            out.append((p - (p % PIECE), line, "E4a" if p % PIECE == 1 else "E4b"))
    # E5: both pieces at the border hold eight line ends
    per_piece = np.bincount(nl // PIECE, minlength=len(a) // PIECE + 2)
    full = np.flatnonzero(per_piece == 8)
    out += [((int(q) + 1) * PIECE, None, "E5") for q in full[np.isin(full + 1, full)]]
    return [e for e in out if border_class(e[0])]


def border_census(text):
    """{(class, line, event): count} and {(class, "E5"): count}: which cells of the matrix the line ends of `text` realise"""
    out = {}
    for b, line, ev in border_events(text):
        cell = (border_class(b), ev) if ev == "E5" else (border_class(b), line, ev)
        out[cell] = out.get(cell, 0) + 1
    return out


def matrix_cells():
    return [(c, line, ev) for c in CLASSES for line in range(4) for ev in EVENTS] + [(c, "E5") for c in CLASSES]


# ---- records ---------------------------------------------------------------------------------------------------------------------
def _seq(rng, n):
    return bytes(rng.choice(b"ACGTN") for _ in range(n))


def _qual(rng, n):
    return bytes(rng.randrange(40, 75) for _ in range(n))


def filler(rng, tag, stretch=0, plain=False, length=None):
    """an ordinary record: every line ends in nothing, '\\r', ' ' or "\\t \\r" before its '\\n' (stripping is live everywhere);
    `stretch` more bytes in the name"""
    n = length if length is not None else rng.randrange(20, 61)
    tails = [b""] * 4 if plain else [rng.choice(TAILS) for _ in range(4)]
    rec = (b"@f%d" % tag + b"x" * stretch + tails[0] + b"\n" + _seq(rng, n) + tails[1] + b"\n+" + tails[2] + b"\n" +
           _qual(rng, n) + tails[3] + b"\n")
    assert len(rec) - stretch <= MAX_FILLER or length is not None
    return rec


def _fill_to(rng, parts, pos, start, tag, plain=False, length=None, bound=MAX_FILLER):
    """ordinary records from `pos` on; the last one's name is stretched so that the next record starts at `start`"""
    assert start - pos >= bound, "targets too close: %d bytes for the fillers" % (start - pos)
    while True:
        f = filler(rng, tag + len(parts), 0, plain, length)
        if pos + len(f) + bound <= start:
            parts.append(f)
            pos += len(f)
            continue
        pad = start - pos - len(f)
        assert pad >= 0
        parts.append(f[:3] + b"x" * pad + f[3:])          # (behind "@f" and the tag's first digit: inside the name)
        return start


def place_targets(targets, size, seed):
    """a text of `size` bytes or a little more whose records are laid so that, for every (B, line, event) of `targets` (sorted by B),
    line `line` of some record realises `event` at border B; E5 targets are (B, None, "E5")"""
    rng = random.Random(seed)
    parts, pos = [], 0
    for t, (b, line, ev) in enumerate(targets):
        if ev == "E5":
            pos = _fill_to(rng, parts, pos, b - 32, 1000 * t)
            parts.append(ONE_BASE * 8)
            pos += 64
            continue
        tail, shift = EVENT_SHAPE[ev]
        n = rng.randrange(24, 40)
        tails = [rng.choice(TAILS) for _ in range(4)]
        tails[line] = tail
        lines = [b"@t%d" % t, _seq(rng, n), b"+", _qual(rng, n)]
        rec = b"".join(lines[k] + tails[k] + b"\n" for k in range(4))
        assert len(rec) <= MAX_FILLER
        nl_in_rec = sum(len(lines[k]) + len(tails[k]) + 1 for k in range(line + 1)) - 1
        pos = _fill_to(rng, parts, pos, b + shift - nl_in_rec, 1000 * t)
        parts.append(rec)
        pos += len(rec)
    if size > pos:
        pos = _fill_to(rng, parts, pos, size, 1000 * len(targets)) if size - pos >= MAX_FILLER else pos
    return b"".join(parts)


# ---- part 1: the matrix, packed into N_PLACED texts of four tiles and a little -----------------------------------------------------
N_PLACED = 7
PLACED_SIZE = 4 * TILE + 2048
# where a text offers borders of each class, the ones the issue names first: per 8 KiB block k the border at 8192 k (sub, wave or
# tile), a row border at 8192 k + 3072 and a piece border at 8192 k + 5648 — all more than 2 KiB apart
_SLOTS = {
    "tile": [TILE * k for k in (1, 2, 3, 4)],
    "wave": [WAVE_BYTES * w for w in (1, 3, 6, 9)],
    "sub": [SUB * s for s in (1, 2, 7, 21)],
    "row": [SUB * k + 3072 for k in (0, 17, 33, 50)],
    "piece": [SUB * k + 5648 for k in (0, 18, 34, 51)],
}


def placed_targets(t):
    """the targets of placed text t: cell i of a class goes to text i % N_PLACED, to that text's (i // N_PLACED)-th border of the class"""
    cells = [(line, ev) for line in range(4) for ev in EVENTS] + [(None, "E5")]
    out = []
    for c in CLASSES:
        assert all(border_class(b) == c for b in _SLOTS[c])
        for i, (line, ev) in enumerate(cells):
            if i % N_PLACED == t:
                out.append((_SLOTS[c][i // N_PLACED], line, ev))
    return sorted(out)


def placed_text(t):
    text = place_targets(placed_targets(t), PLACED_SIZE, 100 + t)
    assert 3 * TILE < len(text) < 600 * 1024
    return text


# ---- part 2: where the file ends ---------------------------------------------------------------------------------------------------
END_SIZES = ([k * TILE + d for k in (1, 2) for d in (-1, 0, 1)] + [w * WAVE_BYTES + d for w in (1, 3) for d in (-1, 0, 1)] +
             [16 * m + d for m in (100, 2100) for d in (1, 15)])
LAST_LINES = ("terminated", "unterminated", "blanks")


def sized_text(size, last, seed=0, plain=False, length=None):
    """exactly `size` bytes of records; the last line is terminated, unterminated, or unterminated with a trailing " \\r"; the last
    record's name is padded to hit the size"""
    rng = random.Random(seed * 7919 + size)
    bound = MAX_FILLER if length is None else 2 * length + 40
    n = length if length is not None else 30
    end = {"terminated": b"\n", "unterminated": b"", "blanks": b" \r"}[last]
    tail = b"\n" + _seq(rng, n) + b"\n+\n" + _qual(rng, n) + end
    parts = []
    if size >= 2 * bound + len(tail) + 8:
        _fill_to(rng, parts, 0, size - len(tail) - 8 - bound, 0, plain, length, bound)
    pos = sum(len(p) for p in parts)
    parts.append(b"@" + b"L" * (size - pos - len(tail) - 1) + tail)
    text = b"".join(parts)
    assert len(text) == size and text.endswith(end) and (last == "terminated") == text.endswith(b"\n")
    return text


# ---- part 4: record-index edges of the framing kernel ------------------------------------------------------------------------------
RECORD_COUNTS = (63, 64, 65, 255, 256, 257, 512)


def blank_positions(n):
    """(record, line) of the whitespace-only line of each variant of count n"""
    return [(r, k) for r, k in ((0, 0), (63, 1), (64, 2), (n - 1, 3)) if r < n]


def record_edge_text(n, blank=None):
    """n records: line 4 of records 63 and 255 ends in " \\r", the longest sequence is in the last record, whose quality line is
    unterminated; blank = (record, line): that line holds whitespace only"""
    rng = random.Random(n)
    parts = []
    for r in range(n):
        ln = 200 if r == n - 1 else rng.randrange(10, 31)
        tails = [rng.choice(TAILS) for _ in range(4)]
        if r in (63, 255):
            tails[3] = b" \r"
        lines = [b"@e%d" % r, _seq(rng, ln), b"+", _qual(rng, ln)]
        if blank and blank[0] == r:
            lines[blank[1]] = b" \t"
        rec = b"".join(lines[k] + tails[k] + b"\n" for k in range(4))
        if r == n - 1:
            rec = rec[:-1 - len(tails[3])]           # the virtual line end: nothing behind the last quality
        parts.append(rec)
    return b"".join(parts)


# ---- part 5: paired texts with different byte rates --------------------------------------------------------------------------------
def lockstep_pair(n=2000, blank=None, shorter=None, seed=5):
    """(text1, text2): ragged lengths, R2's names three times as long.  blank = (file, record): a blank line in front of that record's
    sequence line, in that file only; shorter = file: that file lacks the last 7 records"""
    rng = random.Random(seed)
    texts = [[], []]
    for r in range(n):
        for k in (0, 1):
            ln = rng.randrange(30, 151)
            name = b"@pair%06d/%d" % (r, k + 1)
            name = name * 3 if k else name
            eol = rng.choice((b"\n", b"\n", b"\r\n"))
            rec = name + eol + (b" \n" if blank == (k, r) else b"") + _seq(rng, ln) + eol + b"+" + eol + _qual(rng, ln) + eol
            if shorter == k and r >= n - 7:
                continue
            texts[k].append(rec)
    return b"".join(texts[0]), b"".join(texts[1])


def drive_lockstep(t1, t2, chunk, frame):
    """feed the two texts in chunks of `chunk` new bytes each, lock step with carry-over, exactly like run_text of
    test_gpu_text_fuzz.py (preprocesser._run_text); frame(bufs, finals) -> the nine fields; -> the fields of every call"""
    texts = [t1, t2]
    pos, left, done, calls = [0, 0], [b"", b""], [False, False], []
    while True:
        bufs, finals = [], []
        for k, t in enumerate(texts):
            new = b"" if done[k] else t[pos[k]:pos[k] + chunk]
            pos[k] += len(new)
            finals.append(done[k] or pos[k] >= len(t))
            bufs.append(left[k] + new)
        info = frame(bufs, finals)
        calls.append(info)
        assert len(calls) < 10000
        n = info["n"]
        done1 = (info["eof1"] or finals[0]) and info["avail1"] == n
        done2 = (info["eof2"] or finals[1]) and info["avail2"] == n
        if done1 or (done2 and info["avail1"] > n):
            return calls
        cons = [info["consumed1"], info["consumed2"]]
        for k in range(2):
            left[k] = bufs[k][cons[k]:]
            if (info["eof1"], info["eof2"])[k] or (k == 1 and done2):
                done[k], left[k] = True, b""


# ---- part 6: the line table at its edge --------------------------------------------------------------------------------------------
OVERFLOW_DELTAS = (-1, 0, 1, 5)


def table_cap(nbytes):
    """entries the line table of a fresh context takes for a chunk (size_line_table, aqc_capi_text.hip)"""
    return nbytes // 16 + 4096


def overflow_text(delta, virtual, records=1200):
    """one-base records and one long padding record in their middle, with exactly table_cap(len) + delta newlines; virtual: the last
    line is unterminated (one line more than there are newlines).  -> (text, number of records)"""
    newlines = 4 * (records + 1) - (1 if virtual else 0)
    nbytes = 16 * (newlines - delta - 4096) + 7
    body = b"\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n"
    padlen = nbytes - 8 * records + (1 if virtual else 0) - len(body) - 1
    assert padlen > 0
    half = records // 2
    text = ONE_BASE * half + b"@" + b"p" * padlen + body + ONE_BASE * (records - half)
    if virtual:
        text = text[:-1]
    assert len(text) == nbytes and text.count(b"\n") == table_cap(len(text)) + delta == newlines and 10000 < nbytes < 80000
    return text, records + 1


def ordinary_text(records, seed=3):
    rng = random.Random(seed)
    return b"".join(filler(rng, r) for r in range(records))


# ---- part 7: names for the name parser ---------------------------------------------------------------------------------------------
TOKENS = ("", "0", "7", "12", "007", "2147483647", "2147483648", "99999999999", "a", "a1", "1a", "+5", "-5", "1_0", "@x")
DIGIT_TOKENS = ("0", "7", "12", "007", "2147483647", "2147483648", "99999999999")
SMALL_TOKENS = ("0", "7", "12", "007")
CIRCLE_XY, CIRCLE_R = 7.0, 6.0        # x and y of {5, 7, 10, 12} against {0, -5, 2^31 - 1, ...}: each moves a name in and out
INT32_MAX = 0x7fffffff


def _group(rng):
    """1..12 tokens joined with ':' — mostly near the pattern \\S+:\\d+:\\S+:\\d+:\\d+:\\d+:\\d+, so that every field decides somewhere"""
    if rng.random() < 0.25:
        return ":".join(rng.choice(TOKENS) for _ in range(rng.randrange(1, 13)))
    pick = lambda pool, p: rng.choice(pool) if rng.random() < p else rng.choice(TOKENS)
    friendly = SMALL_TOKENS + ("+5", "-5", "1_0", "a1", "12")
    toks = [rng.choice(TOKENS) for _ in range(rng.randrange(1, 4))]               # first \S+ (with ':' inside when more than one)
    toks.append(pick(SMALL_TOKENS, 0.8))
    toks += [pick(friendly, 0.8) for _ in range(rng.randrange(1, 3))]             # second \S+: items[3] or items[4] when the first is long
    toks += [pick(SMALL_TOKENS, 0.85) for _ in range(4)]
    toks += [rng.choice(TOKENS) for _ in range(rng.randrange(0, 13 - len(toks)) if rng.random() < 0.2 else 0)]
    return ":".join(toks[:12])


def name_cases(n=20000, seed=7):
    """n names of the grammar: 1..12 tokens joined with ':', optionally a second blank- or tab-separated group before or after,
    optionally a leading '@'; never empty, never ending in a blank (the framer strips that before the parser sees the name)"""
    rng = random.Random(seed)
    names = []
    while len(names) < n:
        name = _group(rng)
        u = rng.random()
        if u < 0.2:
            name = _group(rng) + rng.choice(" \t") + name
        elif u < 0.4:
            name = name + rng.choice(" \t") + _group(rng)
        if rng.random() < 0.5:
            name = "@" + name
        if name.strip(" \t") and name == name.rstrip(" \t"):
            names.append(name)
    return names


def parse_name(name):
    """(ok, lane, tile, x, y) by the host's parser (Python's re and int()), or None where it raises ValueError"""
    try:
        return fastq.parse_illumina_name(name.encode("latin-1"))
    except ValueError:
        return None


def first_token_has_colon(name):
    """the match's first \\S+ itself contains ':' — the regex engine had to back off into it"""
    m = fastq._NAME_RE.search(name)
    return bool(m) and len(m.group().split(":")) > 7


def name_circles(parsed):
    """one circle per (lane, tile) the names parse to (values beyond int32 have none: no circle file can name them)"""
    pairs = sorted({(p[1], p[2]) for p in parsed if p and p[0] and abs(p[1]) <= INT32_MAX and abs(p[2]) <= INT32_MAX})
    return [(CIRCLE_XY, CIRCLE_XY, CIRCLE_R, lane, tile) for lane, tile in pairs]


def in_bubble(p, circles):
    """isInBubble (preprocesser.py:176-204) on a parsed name, by the oracle; values beyond int32 are clamped to it, which changes no
    verdict: such a lane or tile matches no circle and such a coordinate is outside every one of these"""
    from oracle import oracle
    if not p or not p[0]:
        return False
    lane, tile, x, y = (max(-INT32_MAX, min(INT32_MAX, v)) for v in p[1:])
    if (lane, tile) != (p[1], p[2]):
        return False
    return oracle.isInBubble(lane, tile, x, y, circles)


def names_text(names):
    return "".join("%s\nACGTACGTAC\n+\nIIIIIIIIII\n" % nm for nm in names).encode("latin-1")


# ---- what the device is compared on ------------------------------------------------------------------------------------------------
INFO_FIELDS = ("n", "avail1", "avail2", "consumed1", "consumed2", "eof1", "eof2", "max_len", "next_len1")


def info_dict(info):
    return {k: int(getattr(info, k)) for k in INFO_FIELDS}


def pad(data):
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    a[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return a


def passthrough_cfg(paired=False, debubble=0):
    """every filter off (test_text_framing.passthrough_cfg); pairs are not looked at for an overlap either: what goes in comes out"""
    cfg = capi.Config()
    cfg.paired = 1 if paired else 0
    cfg.no_overlap = 1 if paired else 0
    cfg.seq_len_req = 0
    cfg.poly_size_limit = cfg.unqualified_base_limit = cfg.n_base_limit = 0
    cfg.barcode_length = 12
    cfg.set_verify("CAGTA")
    cfg.qc_kmer = 8
    cfg.debubble = debubble
    return cfg


def oracle_expect(texts, finals, max_records=capi.UINT64_MAX):
    """(the nine FrameInfo fields by OracleEngine.frame, per file the n records' stripped lines joined by '\\n')"""
    from oracle import oracle
    eng = oracle.OracleEngine()
    args = [pad(texts[0]), len(texts[0]), finals[0]]
    if len(texts) == 2:
        args += [pad(texts[1]), len(texts[1]), finals[1]]
    info = info_dict(eng.frame(0, *args, max_records=max_records))
    outs = []
    for buf, records in eng._text[0]:
        outs.append(b"".join(buf[o:o + l] + b"\n" for r in range(info["n"]) for o, l in records[r]))
    return info, outs


def device_frame(eng, texts, finals, max_records=capi.UINT64_MAX, slot=0):
    args = [pad(texts[0]), len(texts[0]), finals[0]]
    if len(texts) == 2:
        args += [pad(texts[1]), len(texts[1]), finals[1]]
    return info_dict(eng.frame(slot, *args, max_records=max_records))


def device_output(eng, n, files, slot=0):
    """run + format + fetch_text of the n records just framed: per file the good stream (everything, in the pass-through configuration)"""
    if not n:
        return [b""] * files
    eng.run(slot)
    sizes = eng.format(slot, n)
    outs = []
    for k in range(files):
        assert sizes[3 * k + 1] == 0 and sizes[3 * k + 2] == 0, "the pass-through configuration flagged a record"
        out = np.zeros(sizes[3 * k] + 1, dtype=np.uint8)
        eng.fetch_text(slot, k, 0, out, sizes[3 * k])
        outs.append(out[:sizes[3 * k]].tobytes())
    return outs


def check(eng, texts, finals, max_records=capi.UINT64_MAX, expect=None):
    """frame on the device, compare the nine fields and every file's records with the oracle's; -> the oracle's info"""
    want_info, want_out = expect or oracle_expect(texts, finals, max_records)
    got = device_frame(eng, texts, finals, max_records)
    assert got == want_info
    outs = device_output(eng, got["n"], len(texts))
    for k in range(len(texts)):
        if outs[k] != want_out[k]:
            a, b = np.frombuffer(outs[k], dtype=np.uint8), np.frombuffer(want_out[k], dtype=np.uint8)
            m = min(len(a), len(b))
            d = int(np.flatnonzero(a[:m] != b[:m])[0]) if (a[:m] != b[:m]).any() else m
            raise AssertionError("file %d: output differs at byte %d (%d against %d bytes): %r against %r"
                                 % (k + 1, d, len(a), len(b), outs[k][max(0, d - 20):d + 20], want_out[k][max(0, d - 20):d + 20]))
    return want_info
