"""The text-in kernels (csrc/aqc_textin.hpp: text_index_kernel, frame_records_kernel, frame_finish_kernel, parse_names_kernel) at every
tile, wave, sub-tile, row and piece border, at the ends of a file, beyond one look-back hop, at the record-index edges of the framing
kernel, in lock step over two files, at the line table's edge and on adversarial names (-m gpu).  The texts come from
text_border_cases.py, whose preconditions test_text_border_cases_cpu.py proves without a GPU; the reference is the oracle
(OracleEngine.frame, the scalar restatement of fastq.Reader) and Python's own `re` and int() for the names.  Everything is integer and
byte work: every comparison is exact — all nine FrameInfo fields, and the records byte for byte through frame -> run -> format ->
fetch_text in the pass-through configuration."""
import random

import pytest

import text_border_cases as tc
from afterqc_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(gpu_engine):
    gpu_engine.set_config(tc.passthrough_cfg())
    gpu_engine.set_circles([])
    gpu_engine.reset_stats()
    return gpu_engine


# ---- 1. border placement, one file -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(tc.N_PLACED))
def test_placed_borders(eng, t):
    """every (border class x line x event) cell of the census, the whole text framed at once"""
    text = tc.placed_text(t)
    for final in (True, False):
        info = tc.check(eng, [text], [final])
        assert info["consumed1"] == len(text) and not info["eof1"]


# ---- 2. where the file ends --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tc.END_SIZES)
def test_file_ends(eng, size):
    """the last piece masked by `keep`, the wave that leaves the unchecked path, the virtual line end — at and around a tile's and a
    wave's end, and with a last piece of 1 and of 15 bytes"""
    for last in tc.LAST_LINES:
        text = tc.sized_text(size, last)
        whole = tc.check(eng, [text], [True])
        assert whole["consumed1"] == size
        part = tc.check(eng, [text], [False])
        assert part["n"] == whole["n"] - (last != "terminated") and (part["consumed1"] < size - 60 or last == "terminated")


# ---- 3. look-back beyond one hop ---------------------------------------------------------------------------------------------------
def plain_text(size):
    return tc.sized_text(size, "terminated", plain=True, length=150)


@pytest.mark.parametrize("tiles,extra", [(tc.HOP + 1, 0), (2 * tc.HOP + 1, 1)])
def test_look_back_hops(eng, tiles, extra):
    """65 tiles and 129 tiles + 1 byte: the smallest texts in which a tile's look-back can walk one and two whole hops"""
    text = plain_text(tiles * tc.TILE + extra)
    info = tc.check(eng, [text], [True])
    assert info["n"] > 27000 * (tiles // tc.HOP) and info["consumed1"] == len(text) and info["max_len"] == 150


@pytest.mark.parametrize("bytes1,bytes2", [(64 * tc.TILE, 66 * tc.TILE), (tc.TILE, tc.TILE + 1), (tc.TILE + 1, tc.TILE), (0, 300), (300, 0)])
def test_look_back_stops_at_the_second_file_s_first_tile(gpu_engine, bytes1, bytes2):
    """two files share the index launch: file 2's tiles look back no further than its own first one; an empty file is a legal chunk"""
    gpu_engine.set_config(tc.passthrough_cfg(paired=True))
    texts = [plain_text(b) if b > 1000 else tc.sized_text(b, "terminated") if b else b"" for b in (bytes1, bytes2)]
    assert [len(t) for t in texts] == [bytes1, bytes2]
    info = tc.check(gpu_engine, texts, [True, True])
    assert (info["n"] > 0) == (min(bytes1, bytes2) > 0)


# ---- 4. record-index edges of the framing kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.RECORD_COUNTS)
def test_record_index_edges(eng, n):
    """lane 0 takes the record's start from the line table (with its blank bit set), the virtual line end belongs to the last lane or
    the first of a wave or block, the longest sequence sits in the last record; then a whitespace-only line at ballot lanes 0 and 63"""
    info = tc.check(eng, [tc.record_edge_text(n)], [True])
    assert (info["n"], info["max_len"], info["eof1"]) == (n, 200, 0)
    assert tc.check(eng, [tc.record_edge_text(n)], [False])["n"] == n - 1
    for rec, line in tc.blank_positions(n):
        info = tc.check(eng, [tc.record_edge_text(n, (rec, line))], [True])
        assert (info["n"], info["avail1"], info["eof1"]) == (rec, rec, 1)


# ---- 5. lock-step bookkeeping, two files, field by field ---------------------------------------------------------------------------
def compare_each_call(eng):
    def frame(bufs, finals):
        want = tc.oracle_expect(bufs, finals)[0]
        assert tc.device_frame(eng, bufs, finals) == want
        return want
    return frame


@pytest.mark.parametrize("chunk", [3000, 40000])
@pytest.mark.parametrize("variant", ["plain", "blank_in_2", "blank_in_1", "short_2", "short_1"])
def test_lock_step_fields(gpu_engine, variant, chunk):
    """all nine FrameInfo fields at every call of a chunked, carried-over pair whose files run at different byte rates"""
    gpu_engine.set_config(tc.passthrough_cfg(paired=True))
    kw = {"plain": {}, "blank_in_2": {"blank": (1, 1234)}, "blank_in_1": {"blank": (0, 1234)}, "short_2": {"shorter": 1},
          "short_1": {"shorter": 0}}[variant]
    t1, t2 = tc.lockstep_pair(**kw)
    calls = tc.drive_lockstep(t1, t2, chunk, compare_each_call(gpu_engine))
    assert variant != "plain" or sum(c["avail1"] != c["avail2"] for c in calls) > 0.8 * len(calls)


def test_max_records(gpu_engine):
    """max_records below, at and above the records a whole-file call holds; next_len1 is R1's next sequence length, or 0"""
    t1, t2 = tc.lockstep_pair(n=300)
    for texts in ([t1, t2], [t1]):
        gpu_engine.set_config(tc.passthrough_cfg(paired=len(texts) == 2))
        for cap in (0, 1, 299, 300, 301):
            info = tc.check(gpu_engine, texts, [True] * len(texts), max_records=cap)
            assert info["n"] == min(cap, 300) and (info["next_len1"] > 0) == (cap < 300)


# ---- 6. the line table at its edge, single and paired ------------------------------------------------------------------------------
@pytest.mark.parametrize("virtual", [False, True], ids=["terminated", "virtual"])
@pytest.mark.parametrize("delta", tc.OVERFLOW_DELTAS)
def test_line_table_edge(delta, virtual):
    """cap - 1, cap, cap + 1 and cap + 5 line ends for a table of cap entries: counted by the first index pass, framed only up to the
    table, indexed again — alone, as file 2 beside an ordinary file 1, and the other way round; each on a fresh context, whose table has
    never been grown; then an ordinary chunk on the same context"""
    text, n = tc.overflow_text(delta, virtual)
    other = tc.ordinary_text(n)
    after = tc.ordinary_text(50, seed=9)
    for texts in ([text], [other, text], [text, other]):
        ctx = capi.Engine(0, 1)
        try:
            ctx.set_config(tc.passthrough_cfg(paired=len(texts) == 2))
            info = tc.check(ctx, texts, [True] * len(texts))
            assert info["n"] == n and info["max_len"] >= 20
            info = tc.check(ctx, [after] * len(texts), [True] * len(texts))
            assert info["n"] == 50
        finally:
            ctx.close()


# ---- 7. the name parser against Python's regex engine ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def names():
    names = tc.name_cases()
    parsed = [tc.parse_name(nm) for nm in names]
    return names, parsed, tc.name_circles(parsed)


def test_names_against_re(gpu_engine, names):
    """every name for which the host's parser (re.search, str.split, int) returns: the bubble verdict decides on each parsed field"""
    names, parsed, circles = names
    keep = [nm for nm, p in zip(names, parsed) if p is not None]
    want = [tc.in_bubble(p, circles) for p in parsed if p is not None]
    gpu_engine.set_config(tc.passthrough_cfg(debubble=1))
    gpu_engine.set_circles(circles)
    gpu_engine.reset_stats()
    try:
        text = tc.names_text(keep)
        info = gpu_engine.frame(0, tc.pad(text), len(text), True)
        assert int(info.n) == len(keep)
        gpu_engine.run(0)
        got = [int(f) == capi.BADBBL for f in gpu_engine.fetch_results(0)["flag"]]
        bad = [(nm, g, w) for nm, g, w in zip(keep, got, want) if g != w]
        assert not bad, (len(bad), bad[:8])
    finally:
        gpu_engine.set_circles([])


def test_names_that_raise(gpu_engine, names):
    """names for which int() raises upstream (ValueError): each fails its batch, alone in it"""
    names, parsed, circles = names
    raising = [nm for nm, p in zip(names, parsed) if p is None]
    sample = random.Random(3).sample(raising, 200)
    gpu_engine.set_config(tc.passthrough_cfg(debubble=1))
    gpu_engine.set_circles(circles)
    quiet = []
    try:
        for nm in sample:
            text = tc.names_text([nm])
            gpu_engine.frame(0, tc.pad(text), len(text), True)
            try:
                gpu_engine.run(0)
                gpu_engine.fetch_results(0)
                quiet.append(nm)
            except capi.AqcError:
                pass
    finally:
        gpu_engine.set_circles([])
    assert not quiet, (len(quiet), quiet[:8])
