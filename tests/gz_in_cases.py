"""Deflate streams for the device gunzip's tests (test_gunzip_cases_cpu.py without a GPU, test_gpu_gunzip.py on one): the edges
of the format and of the kernels in csrc/aqc_gunzip_dev.hpp, each as ONE group of sections for capi.gunzip_probe.

Most streams are written token by token by the small deflate writer below (stored, fixed-Huffman and dynamic-Huffman blocks
from explicit tokens: a literal byte, or a (length, distance) pair), so that a block holds exactly the tokens a case is
about; some are zlib's own.  The expected text of a hand-made member is built by APPLYING its tokens in Python, never by
inflating; zlib.decompress must accept every member and return that very text (checked when a case is made: zlib is the
authority on what valid deflate is).

case(name) -> Case:
  image      the gzip member
  text       what it inflates to
  nominal / stop / exact   the section table (bit positions in image) of the one group
  window     the text in front of section 0 (<= 32 KiB)
  text_off   {bit: offset in text}: where in the text a section that starts at a known block begins
  budgets    (ratio_cap, tok_ratio, overlap_tokens) of the decoder
  all_found  every section must be found and chain to its successor; otherwise `found` is the expected mask, from the
             decoder's rules as the case's docstring states them
  end_bit / n_sym   (optional) what section 0 must end at / hold, where the case is about that
  status     what resolve() must return (0; -1 for the marker into the void)
  valid      False for the one member zlib must REJECT
"""
import functools
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
WINDOW = 32768
# the decoder's constants a case is built around (csrc/aqc_gunzip_dev.hpp)
PLAIN_BITS, TILE, TILE_CAND, SEC_BLOCKS = 8192, 4096, 16, 4096
DEFAULT_BUDGETS = (6, 1, 512)


def len_symbol(length):
    """(symbol - 257, extra bits' value) of a match length; 258 is symbol 285"""
    if length == 258:
        return 28, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    assert length < LEN_BASE[i] + (1 << LEN_EXTRA[i])
    return i, length - LEN_BASE[i]


def dist_symbol(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    assert 1 <= dist < DIST_BASE[i] + (1 << DIST_EXTRA[i])
    return i, dist - DIST_BASE[i]


class BitWriter:
    def __init__(self, head=b""):
        self.out = bytearray(head)
        self.acc = 0
        self.n = 0

    def bit_pos(self):
        return len(self.out) * 8 + self.n

    def bits(self, value, count):
        """`count` bits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        self.bits(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def limited_lengths(freq, limit):
    """code lengths of a Huffman code for freq (0: unused), no length above `limit`; always a COMPLETE code of >= 2 symbols
    (a lone symbol gets a neighbour: deflate's code-length and literal/length codes must be complete)"""
    import heapq
    freq = list(freq)
    used = [s for s, f in enumerate(freq) if f]
    if len(used) < 2:
        extra = next(s for s in range(len(freq)) if s not in used)
        freq[extra] = 1
        used = sorted(used + [extra])
    heap = [(freq[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    count = [0] * (max(max(depth.values()), limit) + 1)
    for s in used:
        count[depth[s]] += 1
    for length in range(len(count) - 1, limit, -1):      # fold what is too long into the limit ...
        count[limit] += count[length]
        count[length] = 0
    total = sum(c << (limit - length) for length, c in enumerate(count) if length)
    while total > 1 << limit:                            # ... and pay for it: one code of the limit becomes the sibling of a shorter one, moved down
        count[limit] -= 1
        for length in range(limit - 1, 0, -1):
            if count[length]:
                count[length] -= 1
                count[length + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (-freq[s], s))    # the most frequent symbols take the shortest codes
    lens = [0] * len(freq)
    i = 0
    for length in range(1, limit + 1):
        for _ in range(count[length]):
            lens[order[i]] = length
            i += 1
    assert i == len(used)
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2: the code of every symbol from the code lengths"""
    count = [0] * 16
    for length in lens:
        count[length] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, length in enumerate(lens):
        if length:
            codes[s] = nxt[length]
            nxt[length] += 1
    return codes


def rle_lengths(seq, repeats=True):
    """the code-length sequence as symbols of the code-length code: [(symbol, extra value, index of its first length)]"""
    ops, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if not repeats:
            ops.append((v, 0, i))
            i += 1
        elif v == 0 and run >= 3:
            take = min(run, 138)
            ops.append((17, take - 3, i) if take <= 10 else (18, take - 11, i))
            i += take
        elif v != 0 and run >= 4:
            ops.append((v, 0, i))
            i += 1
            left = run - 1
            while left >= 3:
                take = min(left, 6)
                ops.append((16, take - 3, i))
                i += take
                left -= take
        else:
            ops.append((v, 0, i))
            i += 1
    return ops


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class Member:
    """one gzip member, block by block; .text is built by applying the tokens, .blocks lists (first bit, text offset, kind)"""

    def __init__(self):
        self.w = BitWriter(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff")
        self.text = bytearray()
        self.blocks = []
        self.headers = []           # per dynamic block: the code-length symbols written (rle_lengths' triples), hlit, hdist, first data bit

    def _apply(self, tokens):
        t = self.text
        for tok in tokens:
            if isinstance(tok, int):
                t.append(tok)
            else:
                length, dist = tok
                assert 3 <= length <= 258 and 1 <= dist <= 32768
                for _ in range(length):
                    t.append(t[-dist] if dist <= len(t) else 0)      # (before the member's start: only the member zlib must reject gets there)

    def _tokens(self, tokens, ll_lens, d_lens):
        w = self.w
        ll, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
        lit = [(int(format(ll[s], "0%db" % ll_lens[s])[::-1], 2), ll_lens[s]) if ll_lens[s] else None for s in range(256)]
        for tok in tokens:
            if isinstance(tok, int):
                w.bits(*lit[tok])
            else:
                ls, lx = len_symbol(tok[0])
                ds, dx = dist_symbol(tok[1])
                assert ll_lens[257 + ls] and d_lens[ds], tok
                w.code(ll[257 + ls], ll_lens[257 + ls])
                w.bits(lx, LEN_EXTRA[ls])
                w.code(dc[ds], d_lens[ds])
                w.bits(dx, DIST_EXTRA[ds])
        w.code(ll[256], ll_lens[256])

    def _begin(self, kind, final):
        self.blocks.append((self.w.bit_pos(), len(self.text), kind))
        self.w.bits(1 if final else 0, 1)

    def stored(self, data, final=False):
        assert len(data) <= 65535
        self._begin("stored", final)
        self.w.bits(0, 2)
        self.w.align()
        self.w.out += struct.pack("<HH", len(data), len(data) ^ 0xffff) + bytes(data)
        self.text += data

    def fixed(self, tokens, final=False):
        self._begin("fixed", final)
        self.w.bits(1, 2)
        self._tokens(tokens, FIXED_LL, FIXED_D)
        self._apply(tokens)

    def dynamic(self, tokens, final=False, ll_lens=None, d_lens=None, hlit=None, hdist=None, repeats=True):
        """code lengths given (286 / 30 of them) or computed from the tokens' frequencies, limited to 15 bits"""
        if ll_lens is None:
            f = [0] * 286
            f[256] = 1
            for tok in tokens:
                f[tok if isinstance(tok, int) else 257 + len_symbol(tok[0])[0]] += 1
            ll_lens = limited_lengths(f, 15)
        if d_lens is None:
            f = [0] * 30
            for tok in tokens:
                if not isinstance(tok, int):
                    f[dist_symbol(tok[1])[0]] += 1
            used = [s for s in range(30) if f[s]]
            d_lens = [0] * 30 if not used else ([int(s == used[0]) for s in range(30)] if len(used) == 1 else limited_lengths(f, 15))
        hlit = hlit or max(257, max(s for s in range(286) if ll_lens[s]) + 1)
        hdist = hdist or max([1] + [s + 1 for s in range(30) if d_lens[s]])
        ops = rle_lengths(list(ll_lens[:hlit]) + list(d_lens[:hdist]), repeats)
        f = [0] * 19
        for sym, _, _ in ops:
            f[sym] += 1
        cl_lens = limited_lengths(f, 7)
        cl = canonical_codes(cl_lens)
        hclen = max(4, max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1)
        w = self.w
        self._begin("dynamic", final)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        for sym, extra, _ in ops:
            w.code(cl[sym], cl_lens[sym])
            if sym >= 16:
                w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
        self.headers.append({"ops": ops, "hlit": hlit, "hdist": hdist, "data_bit": w.bit_pos(), "ll_lens": list(ll_lens), "d_lens": list(d_lens)})
        self._tokens(tokens, ll_lens, d_lens)
        self._apply(tokens)

    def finish(self):
        """an empty final stored block (no candidate: every chain ends in front of it), the trailer; -> image"""
        self.stored(b"", final=True)
        self.w.out += struct.pack("<II", zlib.crc32(bytes(self.text)) & 0xffffffff, len(self.text) & 0xffffffff)
        return bytes(self.w.out)


class Case:
    def __init__(self, doc, image, text, nominal, stop, exact, window=b"", text_off=None, budgets=DEFAULT_BUDGETS, all_found=True, found=None,
                 end_bit=None, n_sym=None, status=0, valid=True):
        self.doc, self.image, self.text = doc, bytes(image), bytes(text)
        self.nominal, self.stop, self.exact = list(nominal), list(stop), list(exact)
        self.window, self.text_off, self.budgets = bytes(window), dict(text_off or {}), tuple(budgets)
        self.all_found, self.found, self.end_bit, self.n_sym, self.status, self.valid = all_found, found, end_bit, n_sym, status, valid
        assert len(self.nominal) == len(self.stop) == len(self.exact) and len(self.window) <= WINDOW
        if all_found:
            assert found is None
            self.found = [True] * len(self.nominal)
        if valid:
            d = zlib.decompressobj(31)
            got = d.decompress(self.image) + d.flush()
            assert d.eof and not d.unused_data and got == self.text, doc
        else:
            try:
                zlib.decompress(self.image, 31)
            except zlib.error:
                pass
            else:
                raise AssertionError("zlib accepts the member it must reject: " + doc)


def _lit(i):
    """the i-th filler literal: upper-case letters and a line feed now and then, neighbours differ"""
    return 10 if i % 23 == 22 else 65 + (i * 7) % 26


def _lits(n, start=0):
    return [_lit(start + i) for i in range(n)]


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _one_section(m, first_block, doc, window_from_text=True, **kw):
    """the member m, finished; ONE section from block `first_block` (exact) up to the final block, the text before it as its window"""
    image = m.finish()
    bit, off, kind = m.blocks[first_block]
    assert kind == "dynamic"
    window = bytes(m.text[max(0, off - WINDOW):off]) if window_from_text else b""
    return Case(doc, image, m.text, [bit], [m.blocks[-1][0]], [1], window=window, text_off={bit: off}, **kw)


def _is_plain(m, image, block, header):
    """does ONE lane read this block when it is the window's only candidate?  (gzb_plan_lanes: the block is taken to reach the window's end)"""
    return len(image) * 8 - m.headers[header]["data_bit"] < PLAIN_BITS


def _history(m, seed=1):
    """a tiny dynamic block and 40,000 stored bytes of noise: the 32 KiB in front of what follows hold distinct bytes"""
    m.dynamic(_lits(10))
    m.stored(_noise(40000, seed))


# ---- the 64-token step of gzb_expand_kernel: hand-made blocks that one plain lane reads -----------------------------------------
def _plain_block(tokens, doc, **kw):
    m = Member()
    m.dynamic(tokens, **kw)
    c = _one_section(m, 0, doc)
    assert _is_plain(m, c.image, 0, 0), doc
    return c


def _case_lits(n):
    """n literal tokens, then the end-of-block code, which is token n % 64 of its step of 64: on lane 0, on lane 63.  No distance
    code.  A second block of five literals follows: a section without a symbol counts as not found, and with n = 0 the first
    block has none."""
    m = Member()
    m.dynamic(_lits(n))
    m.dynamic(_lits(5, 900))
    c = _one_section(m, 0, "n = %d: " % n + _case_lits.__doc__)
    assert _is_plain(m, c.image, 0, 0)
    return c


def _case_step_first_match():
    """every step's first token is a match whose source lies wholly before the step — the one way a self-overlapping match
    (distance < length) joins the batch of independent matches: distances 1, 2, 3, 7, 257, 258 with length 258, distance == length"""
    toks = _lits(64 + 200)             # steps 0 .. 3 and the first 8 tokens of step 4: 264 bytes of history
    toks += _lits(56, 300)
    for i, (length, dist) in enumerate([(258, 1), (258, 2), (258, 3), (258, 7), (258, 257), (258, 258), (100, 100), (3, 3)]):
        assert len(toks) % 64 == 0
        toks += [(length, dist)] + _lits(63, 1000 + 70 * i)
    return _plain_block(toks, _case_step_first_match.__doc__)


def _case_ordered_matches():
    """matches in the middle of a step whose source the SAME step wrote (the ordered copies, `j % distance`): distances 1, 2, 3, 7
    with length 258 behind fresh literals; distances 257 and 258, whose source straddles the step's first output position;
    distance == length"""
    toks = _lits(64)
    for i, (length, dist) in enumerate([(258, 1), (258, 2), (258, 3), (258, 7), (258, 257), (258, 258), (100, 100), (3, 3), (4, 3)]):
        while len(toks) % 64:
            toks += _lits(1, 5000 + len(toks))
        toks += _lits(9, 2000 + 50 * i) + [(length, dist)] + _lits(3, 3000 + 50 * i)
    return _plain_block(toks, _case_ordered_matches.__doc__)


def _case_chain_in_step():
    """a chain inside one step: a literal, then (distance, length) (1, 3), (4, 8), (12, 24), (36, 72) — each match's source was
    written by the one before it"""
    return _plain_block([88, (3, 1), (8, 4), (24, 12), (72, 36)] + _lits(5), _case_chain_in_step.__doc__)


def _case_straddle():
    """a match whose source straddles its step's first output position: 64 literals (step 0), 10 literals, then length 30 at
    distance 20 (ten bytes of step 0's, ten of step 1's, then its own), and length 40 at distance 45"""
    return _plain_block(_lits(64) + _lits(10, 100) + [(30, 20), (40, 45)] + _lits(4, 200), _case_straddle.__doc__)


# ---- markers and distances ---------------------------------------------------------------------------------------------------------
def _markers(from_history):
    """blocks of matches at offset 0 that reach back before their block, behind 40,000 bytes of stored noise: distance 32768 with
    length 258 and with length 3, distance 1, and the bases of the two largest distance symbols with and without their extra bits
    all ones (16385, 24576, 24577, 32768).  `window`: the section starts at the first of them, every marker is resolved from the
    window (gzb_resolve_kernel).  `rebase`: it starts at the tiny block in front of the noise, so gzb_gather_kernel's gzb_rebase
    finds every marker's byte inside the section."""
    m = Member()
    _history(m)
    m.dynamic([(258, 32768)] + _lits(5))
    m.dynamic([(3, 32768)] + _lits(5, 10))
    m.dynamic([(10, 1)] + _lits(5, 20))
    m.dynamic([(258, 16385), (258, 24576), (258, 24577), (258, 32768), (3, 32768), (7, 24577)] + _lits(5, 30))
    return _one_section(m, 0 if from_history else 2, _markers.__doc__, budgets=(64, 8, 512))


# ---- codes ------------------------------------------------------------------------------------------------------------------------
_LADDER = list(range(1, 15)) + [15, 15]


def _case_long_codes():
    """literal/length code lengths 1, 2, ..., 14, 15, 15 (the end-of-block code and length symbol 285 take the two of 15 bits) and
    a distance code built the same way over symbols 0 .. 15: longer than the 11- and 10-bit root tables, gzb_slow runs for both"""
    ll_syms = list(range(65, 77)) + [257, 270, 256, 285]
    ll_lens, d_lens = [0] * 286, [0] * 30
    for s, length in zip(ll_syms, _LADDER):
        ll_lens[s] = length
    for s in range(16):
        d_lens[s] = _LADDER[s]
    toks = [65 + i % 12 for i in range(300)]
    for s in range(16):
        toks += [(3, DIST_BASE[s]), 65 + s % 12, (LEN_BASE[13] + s % 4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1), (258, DIST_BASE[s])]
    return _plain_block(toks, _case_long_codes.__doc__, ll_lens=ll_lens, d_lens=d_lens)


def _case_hlit286_hdist30():
    """HLIT = 286 with symbol 285 used (length 258) and HDIST = 30 with distance symbol 29 used, behind 40,000 bytes of noise"""
    m = Member()
    _history(m)
    m.dynamic(_lits(20) + [(258, 32768), (258, 24577), (17, 5)] + _lits(3), hlit=286, hdist=30)
    assert m.headers[-1]["hlit"] == 286 and m.headers[-1]["hdist"] == 30
    return _one_section(m, 2, _case_hlit286_hdist30.__doc__, budgets=(64, 8, 512))


def _case_single_dist():
    """a single distance code of one bit (an incomplete code that inflate accepts)"""
    c = _plain_block(_lits(40) + [(10, 5), (20, 6), (258, 5)] + _lits(3), _case_single_dist.__doc__)
    return c


def _case_repeat_codes():
    """all three repeat codes in the header: 18 and 17 for runs of zeros, 16 for runs of 7s, and a 16 that carries the length 3
    across the border between the literal/length lengths (260 of them) and the distance lengths"""
    ll_lens, d_lens = [0] * 286, [0] * 30
    for s in list(range(32, 64)) + list(range(69, 101)):
        ll_lens[s] = 7
    for s in (256, 257, 258, 259):
        ll_lens[s] = 3
    for s in range(8):
        d_lens[s] = 3
    toks = [32 + i % 32 for i in range(40)] + [69 + i % 32 for i in range(40)] + [(3, 1), (4, 9), (5, 12)]
    m = Member()
    m.dynamic(toks, ll_lens=ll_lens, d_lens=d_lens)
    h = m.headers[0]
    syms = {op[0] for op in h["ops"]}
    assert {16, 17, 18} <= syms and h["hlit"] == 260
    assert any(sym == 16 and at < 260 < at + 3 + extra for sym, extra, at in h["ops"]), "no 16 across the border"
    c = _one_section(m, 0, _case_repeat_codes.__doc__)
    assert _is_plain(m, c.image, 0, 0)
    return c


# ---- the stream window of a decoding lane (GzbInLds) ---------------------------------------------------------------------------
def _tok48_codes():
    # literal/length: twelve literals with 1 .. 12 bits, end of block 13, length symbol 257 14, length symbols 281 and 284 15 bits
    ll_lens, d_lens = [0] * 286, [0] * 30
    for s, length in zip(list(range(65, 77)) + [256, 257, 281, 284], _LADDER):
        ll_lens[s] = length
    # distance: symbols 0 .. 13 with 1 .. 14 bits, symbols 28 and 29 with 15
    for s, length in zip(list(range(14)) + [28, 29], _LADDER):
        d_lens[s] = length
    return ll_lens, d_lens


def _case_tok48(n_tokens, lanes32):
    """every token 48 bits wide: a 15-bit code for length symbol 281 or 284 with 5 extra bits, a 15-bit code for distance symbol
    28 or 29 with 13 extra bits — the most stream a lane can consume between two sync() calls of its 32-word window (8 tokens: 12
    words).  Behind 40,000 bytes of noise; it expands about 30 x, so the case carries its own ratio_cap."""
    ll_lens, d_lens = _tok48_codes()
    m = Member()
    _history(m, seed=7)
    rng = np.random.default_rng(48)
    toks = []
    for i in range(n_tokens):
        ls = (281, 284)[int(rng.integers(0, 2))] - 257
        ds = 28 + int(rng.integers(0, 2))
        toks.append((LEN_BASE[ls] + int(rng.integers(0, 31 if ls == 27 else 32)), DIST_BASE[ds] + int(rng.integers(0, 8192))))
    m.dynamic(toks, ll_lens=ll_lens, d_lens=d_lens)
    bits = m.w.bit_pos() - m.headers[-1]["data_bit"]
    assert bits == 48 * n_tokens + 13
    c = _one_section(m, 2, _case_tok48.__doc__, budgets=(64, 8, 512))
    assert (len(c.image) * 8 - m.headers[-1]["data_bit"] >= PLAIN_BITS) == lanes32
    return c


# ---- scan and compaction ------------------------------------------------------------------------------------------------------------
def _case_header_at(bit_in_byte, start_byte):
    """a dynamic block's header at a chosen bit of a chosen byte: behind a stored block of zeros (no bit of it looks like a
    header) and a few fixed-Huffman blocks — empty ones take 10 bits, one with a single 9-bit literal takes 19, which is how
    odd offsets come about.  ONE section that is searched from the member's first block on (exact = 0): the block under test is
    the first candidate there is, at a lane's last byte (the 64 bits the quick test reads come from two lanes' loads), at a
    4,096-byte tile's last byte, or inside a lane."""
    # bits of fixed blocks in front: a * 10 + b * 19 = 8 * whole bytes + bit_in_byte
    a, b = next((a, b) for b in range(2) for a in range(8) if (10 * a + 19 * b) % 8 == bit_in_byte)
    pad_bytes = (10 * a + 19 * b) // 8
    stored_len = start_byte - pad_bytes - 10 - 5
    assert stored_len >= 0
    m = Member()
    m.stored(bytes(stored_len))
    for _ in range(a):
        m.fixed([])
    for _ in range(b):
        m.fixed([200])
    m.dynamic(_lits(30) + [(5, 3), (9, 20)] + _lits(4))
    bit, off, _ = m.blocks[-1]
    assert bit == start_byte * 8 + bit_in_byte, (bit, start_byte, bit_in_byte)
    image = m.finish()
    return Case(_case_header_at.__doc__, image, m.text, [80], [m.blocks[-1][0]], [0], text_off={bit: off})


def _two_blocks():
    m = Member()
    m.dynamic(_lits(50) + [(10, 7)])
    m.dynamic(_lits(30, 100) + [(10, 60)])
    return m


def _case_first_bit_miss():
    """the search starts ONE bit behind a block's header: the scan keeps candidates in [first_bit, last_bit), so that block is
    none, and the next one begins at the stop bit, where the search ends: nothing is found"""
    m = _two_blocks()
    image = m.finish()
    return Case(_case_first_bit_miss.__doc__, image, m.text, [m.blocks[0][0] + 1], [m.blocks[1][0]], [0], all_found=False, found=[False])


def _case_last_bit(inside):
    """two blocks, the section from the first: with the stop bit ONE behind the second block's header that header is the last
    candidate of the scan (at last_bit - 1) and the chain takes the block; with the stop bit AT it the chain ends in front"""
    m = _two_blocks()
    image = m.finish()
    b0, b1 = m.blocks[0][0], m.blocks[1][0]
    return Case(_case_last_bit.__doc__, image, m.text, [b0], [b1 + 1 if inside else b1], [1], text_off={b0: 0},
                end_bit=m.blocks[2][0] if inside else b1, n_sym=len(m.text) if inside else m.blocks[1][1])


def _case_tile_overflow():
    """40 small dynamic blocks, about 25 bytes each, all in the window's first 4,096-byte tile: the scan keeps the LOWEST 16 block
    starts of a tile.  Section 0 starts at block 0 and chains through 16 blocks; the 17th is no candidate, so it ends there.
    Section 1 must start at block 20 (exact), which the scan dropped: not found.  (Hand-made: zlib with Z_FULL_FLUSH every 64
    bytes of text writes fixed-Huffman blocks, which are no candidates at all.)"""
    m = Member()
    for i in range(40):
        m.dynamic(_lits(8, 10 * i) + [(4, 3)])
    image = m.finish()
    assert m.blocks[39][0] // 8 < TILE
    b = [x[0] for x in m.blocks]
    return Case(_case_tile_overflow.__doc__, image, m.text, [b[0], b[20]], [b[20], b[40]], [1, 1], text_off={b[0]: 0}, all_found=False,
                found=[True, False], end_bit=b[TILE_CAND], n_sym=m.blocks[TILE_CAND][1])


def _case_chain_capacity():
    """5,000 empty stored blocks between two dynamic blocks: a section's chain holds 4,096 entries (GZB_SEC_BLOCKS), so it ends
    behind the first block and 4,095 of the stored ones — found, but short.  (The first block is taken to reach up to the next
    candidate, 25 KB on, so 32 lanes read it and what follows it, stored blocks' zeros included, at two to four bits a token:
    the case gives them 16 token entries per compressed byte.)"""
    m = Member()
    m.dynamic(_lits(100))
    for _ in range(5000):
        m.stored(b"")
    m.dynamic(_lits(100, 500))
    image = m.finish()
    b = [x[0] for x in m.blocks]
    return Case(_case_chain_capacity.__doc__, image, m.text, [b[0]], [b[-1]], [1], text_off={b[0]: 0}, budgets=(6, 16, 4096), end_bit=b[SEC_BLOCKS], n_sym=100)


# ---- resolve, windows and CRC: sections of exact sizes, each ONE dynamic block of literals only (text-like bytes at six to seven
# bits each: from a few hundred symbols on, 32 lanes read the block).  Not many small blocks: a group's symbol and token space is
# budgeted for a block start per 16 KiB (+ 32), whatever the budgets.
def _sized(m, n, seed):
    m.dynamic(list(_fastq_like(n, seed)))


def _sized_sections(sizes, doc, seed, lead=0, budgets=DEFAULT_BUDGETS):
    m = Member()
    if lead:
        _sized(m, lead, seed + 1)
    starts = []
    for i, n in enumerate(sizes):
        starts.append(len(m.blocks))
        _sized(m, n, seed + 10 * i)
    image = m.finish()
    bits = [m.blocks[s][0] for s in starts] + [m.blocks[-1][0]]
    off0 = m.blocks[starts[0]][1]
    return Case(doc, image, m.text, bits[:-1], bits[1:], [1] * len(sizes), window=bytes(m.text[max(0, off0 - WINDOW):off0]), text_off={bits[0]: off0}, budgets=budgets)


def _fastq_like(n, seed):
    """n bytes that look like text: line feeds every 40 - 160 bytes (the resolve pass counts them per 64 KiB piece)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(33, 127, n, dtype=np.uint8)
    at = 0
    while at < n:
        at += int(rng.integers(40, 160))
        if at < n:
            t[at] = 10
    return t.tobytes()


def _case_window_len(wlen):
    """`wlen` bytes of the member in front of the section (valid0 = 32768 - wlen of the window do not exist), and the section's
    first token a match that reaches back exactly that far"""
    m = Member()
    if wlen:
        m.dynamic(_lits(1))
        if wlen > 1:
            m.stored(_noise(wlen - 1, 100 + wlen))
    first = len(m.blocks)
    m.dynamic(([(258, wlen)] if wlen else []) + _lits(40) + [(20, 33)])
    return _one_section(m, first, _case_window_len.__doc__, budgets=(64, 8, 512))


def _case_void():
    """the member begins 100 bytes before the section and the section's first token reaches 200 bytes back: invalid deflate (zlib
    rejects the member), a marker "into the void" — resolve() must return the data error, and nothing faults"""
    m = Member()
    m.dynamic(_lits(1))
    m.stored(_noise(99, 3))
    m.dynamic([(10, 200)] + _lits(20))
    return _one_section(m, 2, _case_void.__doc__, status=-1, valid=False)


# ---- zlib's own streams ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fastq_text():
    """3,500 reads of 150 bases, about 1.2 MB"""
    from afterqc_amd import synth
    d = synth.make_pairs(3500, 150, seed=4242, dirty=True)
    buf, n = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    return bytes(memoryview(buf)[:n])


def _deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    if not flush_every:
        return c.compress(text) + c.flush()
    out = b""
    for at in range(0, len(text), flush_every):
        out += c.compress(text[at:at + flush_every]) + c.flush(flush)
    return out + c.flush()


def _sections_every(image, text, section_bytes, doc, **kw):
    """sections of section_bytes compressed bytes over a zlib member whose first block, at bit 80, is a dynamic one: section 0
    starts AT it, the others are searched from their nominal bit on, each stops at the next one's nominal bit, the last one — of two to three
    times section_bytes, more than any block of zlib's, so that a block starts in it — just in front of the trailer (its chain
    ends where the final block begins)"""
    assert (image[10] & 7) == 4, "the member's first block is not a non-final dynamic one"
    nominal = [80] + [8 * at for at in range(section_bytes, len(image) - 2 * section_bytes, section_bytes)]
    stop = nominal[1:] + [8 * (len(image) - 8) - 1]
    return Case(doc, image, text, nominal, stop, [1] + [0] * (len(nominal) - 1), text_off={80: 0}, **kw)


def _case_fastq(level):
    return _sections_every(_deflate(fastq_text(), level), fastq_text(), 32 << 10,
                           "1.2 MB of FASTQ at zlib level %d in sections of 32 KiB: blocks far above GZB_PLAIN_BITS (32 entry points each, "
                           "stitched), sections that begin in the middle of the stream (markers)" % level, budgets=(12, 2, 512))


def _case_sync_flush():
    """60 KB of the FASTQ text with Z_SYNC_FLUSH every 2 KB: every block is below 8,192 bits (one plain lane reads it) and an
    empty stored block lies behind each, which the chain steps over.  ONE section and 60 KB, not all of the text, for two of
    the decoder's rules: the token space of a group is budgeted for a block start per 16 KiB (+ 32), and this stream has one
    every 600 bytes — the 30 blocks here fit, the 55th of a longer stream would be skipped; and a section ends AT the first block
    boundary behind its stop bit while the next one begins at the first dynamic block, so two sections never meet across the
    empty stored block between them (the host bridges those five bytes)."""
    text = fastq_text()[:60000]
    image = _deflate(text, 6, flush_every=2000)
    assert (image[10] & 7) == 4
    return Case(_case_sync_flush.__doc__, image, text, [80], [8 * (len(image) - 8) - 1], [1], text_off={80: 0}, budgets=(12, 2, 512))


def _case_strategy(strategy, what, budgets):
    text = fastq_text()[:300000]
    return _sections_every(_deflate(text, 6, strategy), text, 32 << 10, "300 KB of the FASTQ text with %s" % what, budgets=budgets)


_CASES = {}


def _add(name, fn, *args):
    _CASES[name] = (fn, args)


for _lv in (1, 6, 9):
    _add("fastq_level_%d" % _lv, _case_fastq, _lv)
_add("fastq_sync_flush_2k", _case_sync_flush)
_add("fastq_huffman_only", _case_strategy, zlib.Z_HUFFMAN_ONLY, "Z_HUFFMAN_ONLY: literals only, more than a token per compressed byte (tok_ratio 8)", (12, 8, 2048))
_add("fastq_rle", _case_strategy, zlib.Z_RLE, "Z_RLE: matches of distance 1 only (tok_ratio 8; the quality runs expand well: ratio_cap 24)", (24, 8, 2048))
for _n in (0, 1, 63, 64, 65, 127, 128):
    _add("literals_%d" % _n, _case_lits, _n)
_add("step_first_match", _case_step_first_match)
_add("ordered_matches", _case_ordered_matches)
_add("chain_in_step", _case_chain_in_step)
_add("source_straddles_step", _case_straddle)
_add("markers_window", _markers, False)
_add("markers_rebase", _markers, True)
_add("long_codes", _case_long_codes)
_add("hlit286_hdist30", _case_hlit286_hdist30)
_add("single_distance_code", _case_single_dist)
_add("repeat_codes", _case_repeat_codes)
_add("tokens_48bit_32_lanes", _case_tok48, 3000, True)
_add("tokens_48bit_plain_lane", _case_tok48, 165, False)
for _place, _byte in (("in_lane", 1029), ("lane_edge", 1039), ("tile_edge", 4095)):
    for _bit in range(8):
        _add("header_%s_bit%d" % (_place, _bit), _case_header_at, _bit, _byte)
_add("first_bit_miss", _case_first_bit_miss)
_add("last_bit_inside", _case_last_bit, True)
_add("last_bit_outside", _case_last_bit, False)
_add("tile_overflow", _case_tile_overflow)
_add("chain_capacity", _case_chain_capacity)
_add("sections_1_to_33", _sized_sections, (1, 15, 16, 17, 31, 32, 33), "a run of sections of 1, 15, 16, 17, 31, 32 and 33 symbols (the resolve pass: 16 symbols per thread, then a tail)", 11)
_add("sections_32k", _sized_sections, (32767, 32768, 32769), "a run of sections of 32,767, 32,768 and 32,769 symbols: one window's worth, one less, one more", 12, 0, (6, 2, 512))
_add("sections_64k", _sized_sections, (65535, 65536, 65537), "a run of sections of 65,535, 65,536 and 65,537 symbols: one CRC piece, one less, one more", 13, 0, (6, 2, 512))
_add("section_100_between", _sized_sections, (40000, 100, 40000, 50), "sections of 40,000, 100 and 40,000 symbols: the window behind the middle one is mostly its predecessor's "
     "(and one of 50 behind them: a window's last block is planned from its predecessor's size, and after one of 100 symbols that is one lane for 40,000 tokens)", 14, 20000, (6, 2, 512))
for _w in (0, 1, 32767, 32768):
    _add("window_%d" % _w, _case_window_len, _w)
_add("marker_into_the_void", _case_void)


def names():
    return list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    fn, args = _CASES[name]
    return fn(*args)


def probe(c, engine):
    from afterqc_amd import capi
    ratio_cap, tok_ratio, overlap_tokens = c.budgets
    return capi.gunzip_probe(c.image, c.nominal, c.stop, c.exact, window=c.window, ratio_cap=ratio_cap, tok_ratio=tok_ratio,
                             overlap_tokens=overlap_tokens, text_cap=len(c.text) + 4096, engine=engine)


def check(c, r):
    """what one probe returned against the case: zlib's text, zlib.crc32, a numpy count of line feeds, the tail window, and the
    sections the case says must be found — nothing here comes from the project's own code"""
    n = len(c.nominal)
    assert r["found"] == c.found, (r["found"], c.found)
    for k in range(n):
        if r["found"][k]:
            assert c.nominal[k] <= r["start_bit"][k] < r["end_bit"][k] and r["n_sym"][k] > 0, (k, r["start_bit"][k], r["end_bit"][k])
            if c.exact[k]:
                assert r["start_bit"][k] == c.nominal[k]
    if c.all_found:
        for k in range(n - 1):
            assert r["end_bit"][k] == r["start_bit"][k + 1], "sections %d and %d do not chain" % (k, k + 1)
            assert r["end_bit"][k] >= c.stop[k]
        assert r["run"] == (0, n), r["run"]
    if c.end_bit is not None:
        assert r["end_bit"][0] == c.end_bit, (r["end_bit"][0], c.end_bit)
    if c.n_sym is not None:
        assert r["n_sym"][0] == c.n_sym, (r["n_sym"][0], c.n_sym)
    first, count = r["run"]
    if not count:
        assert not any(r["found"])
        return
    assert r["status"] == c.status, r["status"]
    if c.status != 0:
        assert r["text"] == b"" and r["tail"] == b""
        return
    off = c.text_off[r["start_bit"][first]]
    sizes = r["n_sym"][first:first + count]
    total = sum(sizes)
    want = c.text[off:off + total]
    assert len(want) == total and len(r["text"]) == total
    assert r["text"] == want, "text differs from zlib's at byte %d" % next(i for i in range(total) if r["text"][i] != want[i])
    assert c.window == c.text[off - len(c.window):off]
    at, nl = 0, []
    for j, size in enumerate(sizes):
        piece = want[at:at + size]
        assert r["crc"][j] == zlib.crc32(piece) & 0xffffffff, "CRC-32 of the run's section %d" % j
        cuts = list(range(size, 0, -65536))[::-1]              # 64 KiB pieces, right-aligned: only the first one is short
        a = np.frombuffer(piece, dtype=np.uint8)
        nl += [int(np.count_nonzero(a[max(0, e - 65536):e] == 10)) for e in cuts]
        at += size
    assert r["piece_nl"] == nl, (r["piece_nl"], nl)
    assert r["tail"] == (c.window + want)[-WINDOW:]
