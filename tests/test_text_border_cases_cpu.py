"""The inputs of tests/text_border_cases.py on the CPU: the geometry they are built around is still the header's, the placed texts fill
the whole (border class x line x event) matrix, every builder's precondition holds, the name grammar reaches each branch of the name
parser — the proof, without a GPU, that test_gpu_text_borders.py cannot pass by missing its targets.  And the oracle frames every
built text the same way whole and in chunks, so the reference the device is held against is self-consistent on these inputs."""
import os

import numpy as np
import pytest

import text_border_cases as tc
from conftest import ROOT
from test_text_framing import oracle_frame, stream_frames


def test_geometry_is_the_header_s():
    """a retune of the index pass must break these cases loudly, not move the borders out from under them"""
    k = tc.header_constants(os.path.join(ROOT, "afterqc_amd", "csrc", "aqc_textin.hpp"))
    assert k == {"TXT_BLOCK": 256, "IDX_K": 8, "IDX_SUB": 4}
    wave = 64
    assert tc.PIECE == 16 and tc.ROW == wave * tc.PIECE and tc.SUB == k["IDX_K"] * tc.ROW
    assert tc.WAVE_BYTES == k["IDX_SUB"] * tc.SUB and tc.TILE == (k["TXT_BLOCK"] // wave) * tc.WAVE_BYTES and tc.HOP == wave


def test_census_on_hand_made_texts():
    def at(prefix_len, body):
        """`body` behind prefix_len bytes of one long name line (line 0 ends with the first '\\n' of body)"""
        return b"@" * prefix_len + body
    assert tc.border_events(at(15, b"\nAC\n")) == [(16, 0, "E1")]
    assert tc.border_events(at(1024, b"\nAC\n")) == [(1024, 0, "E2")]
    assert tc.border_events(at(8191, b" \nAC\n")) == [(8192, 0, "E3s")]
    assert tc.border_events(at(32767, b"\r\nAC\n")) == [(32768, 0, "E3r")]
    assert tc.border_events(at(131070, b"\t \r\nAC\n")) == [(131072, 0, "E4a")]
    assert tc.border_events(at(31, b"\t \r\nAC\n")) == [(32, 0, "E4b")]
    assert tc.border_events(at(30, b"  \nAC\n")) == []                       # two blanks are neither E3 nor E4
    assert tc.border_events(b"@\n" + b"A" * 14 + b"\n") == [(16, 1, "E2")]   # the line of the record
    ev = tc.border_events(b"@" * 991 + b"\n" + tc.ONE_BASE * 8)
    assert [e for e in ev if e[2] == "E5"] == [(1008, None, "E5"), (1024, None, "E5"), (1040, None, "E5")]
    assert [tc.border_class(b) for b in (0, 8, 16, 1024, 8192, 32768, 98304, 131072, 262144)] == \
        [None, None, "piece", "row", "sub", "wave", "wave", "tile", "tile"]


def test_placed_texts_fill_the_matrix():
    seen, events = {}, set()
    for t in range(tc.N_PLACED):
        text = tc.placed_text(t)
        ev = set(tc.border_events(text))
        for target in tc.placed_targets(t):
            assert target in ev, (t, target)                  # every target landed where it was asked to
        events |= ev
        for cell, n in tc.border_census(text).items():
            seen[cell] = seen.get(cell, 0) + n
        # everything else is live too: lines that end in nothing, '\r', ' ' and "\t \r"
        tails = {line.rstrip(b"\n")[len(line.rstrip()):] for line in text.splitlines(True)[:400]}
        assert tails >= set(tc.TAILS)
    cells = tc.matrix_cells()
    assert len(cells) == 5 * 4 * 6 + 5
    assert [c for c in cells if not seen.get(c)] == []
    borders = {b for b, _, _ in events}
    assert {1 * tc.WAVE_BYTES, 3 * tc.WAVE_BYTES} <= borders              # wave borders inside a tile
    assert {1 * tc.TILE, 2 * tc.TILE} <= borders                          # the first and the second tile border
    assert any(tc.border_class(b) == "sub" for b in borders)              # a sub-tile border that is no wave border
    # the strip crosses a wave and a tile border with each blank
    for c in ("wave", "tile"):
        assert all(seen.get((c, line, e)) for line in range(4) for e in ("E3s", "E3r", "E4a", "E4b"))


def test_census_of_the_large_random_text(capsys):
    """printed, not asserted: what test_text_framing.py::test_device_framing_large_random's text reaches by chance (the counts in
    text_border_cases' docstring)"""
    rng = np.random.default_rng(5)
    parts = []
    for i in range(20000):
        L = int(rng.integers(1, 300))
        seq = "".join("ACGTN"[int(x)] for x in rng.integers(0, 5, L))
        tail = ["", "\r", " ", "\t \r"][int(rng.integers(0, 4))]
        parts.append("@read%d some text%s\n%s%s\n+%s\n%s\n" % (i, tail, seq, tail, tail, "F" * L))
    data = "".join(parts).encode()
    census = tc.border_census(data)
    with capsys.disabled():
        print("\nlarge random text: %d bytes, %.1f tiles" % (len(data), len(data) / tc.TILE))
        for c in tc.CLASSES:
            print("  %-6s" % (c + ":"), " ".join("%4d" % sum(census.get((c, line, e), 0) for line in range(4)) for e in tc.EVENTS),
                  "%2d" % census.get((c, "E5"), 0))


@pytest.mark.parametrize("last", tc.LAST_LINES)
def test_sized_texts(last):
    from oracle import oracle
    assert {tc.TILE - 1, tc.TILE, tc.TILE + 1, 2 * tc.TILE + 1, tc.WAVE_BYTES, 3 * tc.WAVE_BYTES - 1, 1601, 1615} <= set(tc.END_SIZES)
    for size in tc.END_SIZES:
        text = tc.sized_text(size, last)
        assert len(text) == size
        whole = oracle.frame_text(text, True)
        part = oracle.frame_text(text, False)
        assert whole[1] == len(whole[0]) and not whole[2]
        if last == "terminated":
            assert part[1] == whole[1]
        else:                                  # the partial line is not framed before the file ends, and nothing of its record is consumed
            assert part[1] == whole[1] - 1 and part[3][4 * part[1] - 1] < size - 60
        if last == "blanks":
            assert whole[0][-1][3][0] + whole[0][-1][3][1] == size - 2


@pytest.mark.parametrize("n", tc.RECORD_COUNTS)
def test_record_edge_texts(n):
    from oracle import oracle
    text = tc.record_edge_text(n)
    records, avail, eof, ends = oracle.frame_text(text, True)
    assert (avail, eof) == (n, False) and not text.endswith(b"\n") and text[-1] > 0x20
    assert records[n - 1][1][1] == 200 == max(r[1][1] for r in records) and all(r[1][1] == r[3][1] for r in records)
    for r in (63, 255):
        if r < n - 1:
            assert text[ends[4 * r + 3] - 3:ends[4 * r + 3]] == b" \r\n"
    assert oracle.frame_text(text, False)[1] == n - 1
    for rec, line in tc.blank_positions(n):
        _, avail, eof, _ = oracle.frame_text(tc.record_edge_text(n, (rec, line)), True)
        assert (avail, eof) == (rec, True)
    assert len(tc.blank_positions(n)) == (4 if n > 64 else 3 if n == 64 else 2)
    assert [k for _, k in tc.blank_positions(512)] == [0, 1, 2, 3]


def oracle_info(bufs, finals):
    return tc.oracle_expect(bufs, finals)[0]


@pytest.mark.parametrize("chunk", [3000, 40000])
def test_lockstep_pairs_drift_apart(chunk):
    t1, t2 = tc.lockstep_pair()
    assert len(t2) > 1.1 * len(t1)
    calls = tc.drive_lockstep(t1, t2, chunk, oracle_info)
    assert sum(c["n"] for c in calls) == 2000 and len(calls) >= (10 if chunk == 40000 else 100)
    assert sum(c["avail1"] != c["avail2"] for c in calls) > 0.8 * len(calls)
    assert any(c["next_len1"] for c in calls)
    # a blank line in one file only, a file that is 7 records short: the lock step ends where that file does
    calls = tc.drive_lockstep(*tc.lockstep_pair(blank=(1, 1234)), chunk, oracle_info)
    assert sum(c["n"] for c in calls) == 1234 and calls[-1]["eof2"] == 1 and not any(c["eof1"] for c in calls)
    # (file 1 runs ahead: its blank line comes into view while file 2 is still records behind, and the driver drops what it holds)
    calls = tc.drive_lockstep(*tc.lockstep_pair(blank=(0, 1234)), chunk, oracle_info)
    assert 0 < sum(c["n"] for c in calls) <= 1234 and any(c["eof1"] for c in calls) and not any(c["eof2"] for c in calls)
    for shorter in (0, 1):
        calls = tc.drive_lockstep(*tc.lockstep_pair(shorter=shorter), chunk, oracle_info)
        assert sum(c["n"] for c in calls) == 1993


@pytest.mark.parametrize("virtual", [False, True])
@pytest.mark.parametrize("delta", tc.OVERFLOW_DELTAS)
def test_overflow_texts(delta, virtual):
    from oracle import oracle
    text, n = tc.overflow_text(delta, virtual)                 # (asserts the number of newlines against the table's size itself)
    records, avail, eof, ends = oracle.frame_text(text, True)
    assert (avail, eof) == (n, False) and text.endswith(b"\n") != virtual
    assert (text.count(b"\n") > tc.table_cap(len(text))) == (delta > 0)


def test_name_grammar_reaches_every_branch():
    names = tc.name_cases()
    assert len(names) == 20000
    assert all(all(c == "\t" or 0x20 <= ord(c) < 0x7f for c in nm) and nm.strip(" \t") and nm == nm.rstrip(" \t") for nm in names)
    for nm in names[:2000]:
        for group in nm.lstrip("@").replace("\t", " ").split(" "):
            assert len(group.split(":")) <= 12 and all(t in tc.TOKENS or "@" + t in tc.TOKENS or t.lstrip("@") in tc.TOKENS
                                                       for t in group.split(":"))
    parsed = [tc.parse_name(nm) for nm in names]
    circles = tc.name_circles(parsed)
    inside = [tc.in_bubble(p, circles) for p in parsed]
    n = float(len(names))
    raising = sum(p is None for p in parsed)
    matched = sum(bool(p and p[0]) for p in parsed)
    backtracked = sum(bool(p and p[0]) and tc.first_token_has_colon(nm) for nm, p in zip(names, parsed))
    assert backtracked >= 0.10 * n          # the first \S+ holds a ':' — the regex engine backed off into it
    assert raising >= 0.05 * n              # int() raises
    assert sum(inside) >= 0.05 * n
    assert matched - sum(inside) >= 0.05 * n
    assert sum(p is not None and not p[0] for p in parsed) >= 0.05 * n          # no match at all
    # each parsed field decides the verdict for some names: take a circle's lane, tile, x or y away and some name leaves it
    ok = [p for p, i in zip(parsed, inside) if i]
    assert len({p[1] for p in ok}) >= 4 and len({p[2] for p in ok}) >= 3 and len({p[3] for p in ok}) >= 3 and len({p[4] for p in ok}) >= 3
    out = [p for p, i in zip(parsed, inside) if p and p[0] and not i and (tc.CIRCLE_XY, tc.CIRCLE_XY, tc.CIRCLE_R, p[1], p[2]) in circles]
    assert any(abs(p[3] - 7) <= 5 for p in out) and any(abs(p[4] - 7) <= 5 for p in out)          # x alone, y alone moves a name out
    # lanes and tiles that match only with the tile field's first character dropped
    undropped = 0
    for nm, p, i in zip(names, parsed, inside):
        if i:
            items = tc.fastq._NAME_RE.search(nm).group().split(":")
            undropped += items[4][:1].isdigit() and (p[1], int(items[4])) not in {(c[3], c[4]) for c in circles}
    assert undropped >= 50
    # int() takes more than digits: a sign, an underscore between digits — names that parse only because of it
    signed = [p for nm, p in zip(names, parsed) if p and p[0] and any(t in nm for t in ("+5", "-5", "1_0"))]
    assert any(p[1] == -5 or p[1] == 5 or p[1] == 10 for p in signed) and any(p[2] == 5 for p in signed)


def _texts():
    for t in range(tc.N_PLACED):
        yield "placed%d" % t, tc.placed_text(t)
    for last in tc.LAST_LINES:
        for size in tc.END_SIZES:
            yield "end%d%s" % (size, last), tc.sized_text(size, last)
    for n in tc.RECORD_COUNTS:
        yield "rec%d" % n, tc.record_edge_text(n)
        for b in tc.blank_positions(n):
            yield "rec%d%s" % (n, b), tc.record_edge_text(n, b)
    for delta in tc.OVERFLOW_DELTAS:
        for virtual in (False, True):
            yield "over%d%s" % (delta, virtual), tc.overflow_text(delta, virtual)[0]
    yield "names", tc.names_text(tc.name_cases()[:3000])
    for k, t in enumerate(tc.lockstep_pair()):
        yield "pair%d" % k, t


def test_oracle_frames_every_text_the_same_whole_and_chunked():
    for name, text in _texts():
        want = oracle_frame(text, True)[0]
        for chunk in (997, 40000, len(text) // 2 + 1):
            assert stream_frames(oracle_frame, text, chunk) == want, (name, chunk)


@pytest.mark.parametrize("tiles,extra", [(tc.HOP + 1, 0), (2 * tc.HOP + 1, 1)])
def test_oracle_frames_the_look_back_texts_the_same_whole_and_chunked(tiles, extra):
    text = tc.sized_text(tiles * tc.TILE + extra, "terminated", plain=True, length=150)
    assert -(-len(text) // tc.TILE) == tiles + extra          # 65 tiles: one hop of the look-back; 130: two
    want = oracle_frame(text, True)[0]
    assert len(want) > 27000 * (tiles // tc.HOP)
    for chunk in (100003, 1 << 20, len(text) // 2 + 1):
        assert stream_frames(oracle_frame, text, chunk) == want, chunk
