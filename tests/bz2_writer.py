"""A bzip2 stream writer for tests: the corners of the format that libbz2's encoder never writes.  Not a test module.

Two levels.  compress(text) goes the whole way — RLE1, BWT by sorted rotations (blocks of a few thousand bytes), MTF with
RUNA / RUNB, Huffman codes — and block(...) takes a block apart: any of the pre-BWT bytes, the last-column vector with any
origPtr, the symbol list, the code-length tables, the selector list, the randomised bit and the CRC can be given, whether or
not an encoder would ever write them.  stream(level, blocks) frames blocks into a .bz2 image.

Bits are kept as strings of "0" / "1" and joined once, so the cost is linear in the output: a block written once can be
repeated tens of thousands of times.  Codes are canonical in the order the decoders read them: by length, then by symbol
index."""
import collections
import heapq

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090
G_SIZE = 50

Block = collections.namedtuple("Block", "bits crc text nblock n_selectors n_tables max_len symbols")


def _crc_table():
    tab = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04c11db7) & 0xffffffff if c & 0x80000000 else (c << 1) & 0xffffffff
        tab.append(c)
    return tab


_CRC = _crc_table()


def crc32(data):
    """bzip2's CRC-32: polynomial 0x04c11db7, MSB first, initial value and final xor of all ones"""
    c = 0xffffffff
    tab = _CRC
    for b in data:
        c = ((c << 8) & 0xffffffff) ^ tab[(c >> 24) ^ b]
    return c ^ 0xffffffff


def combine(crcs):
    """the stream's CRC: rotate left by one, xor the block's"""
    c = 0
    for x in crcs:
        c = (((c << 1) | (c >> 31)) & 0xffffffff) ^ x
    return c


def bits(value, n):
    return format(value, "0%db" % n) if n else ""


# ---- RLE1 ----------------------------------------------------------------------------------------------------------------------
def rle1(text):
    """runs of 4 to 259 equal bytes become four of them and a count byte; a longer run starts again behind the count"""
    out = bytearray()
    i, n = 0, len(text)
    while i < n:
        c = text[i]
        r = 1
        while r < 259 and i + r < n and text[i + r] == c:
            r += 1
        if r >= 4:
            out += bytes([c]) * 4 + bytes([r - 4])
        else:
            out += bytes([c]) * r
        i += r
    return bytes(out)


def un_rle1(pre):
    """what a decoder makes of pre-BWT bytes (four equal bytes at the very end, with no count byte, expand to themselves)"""
    out = bytearray()
    run, last = 0, -1
    for c in pre:
        if run == 4:
            out += bytes([last]) * c
            run, last = 0, -1
            continue
        run = run + 1 if c == last else 1
        last = c
        out.append(c)
    return bytes(out)


# ---- BWT -----------------------------------------------------------------------------------------------------------------------
def bwt(pre):
    """(last column, origPtr) by sorting the rotations: quadratic memory, blocks of a few thousand bytes"""
    n = len(pre)
    twice = pre + pre
    order = sorted(range(n), key=lambda i: twice[i:i + n])
    return bytes(twice[i + n - 1] for i in order), order.index(0)


def inverse_bwt(last, orig_ptr):
    """the chase a decoder makes from origPtr for len(last) steps — `last` need not be a real BWT vector"""
    n = len(last)
    order = sorted(range(n), key=lambda i: last[i])        # (stable: row j of the sorted matrix is followed by row order[j])
    out = bytearray(n)
    t = orig_ptr
    for k in range(n):
        t = order[t]
        out[k] = last[t]
    return bytes(out)


# ---- MTF, RUNA / RUNB ----------------------------------------------------------------------------------------------------------
def mtf_encode(last, used):
    """the symbol list of `last` over the bytes in use: 0 / 1 = RUNA / RUNB, k + 1 = MTF position k, len(used) + 1 = end of block"""
    index = {b: i for i, b in enumerate(used)}
    mtf = list(range(len(used)))
    syms = []
    run = 0

    def flush():
        nonlocal run
        while run > 0:
            if run & 1:
                syms.append(0)
                run = (run - 1) >> 1
            else:
                syms.append(1)
                run = (run - 2) >> 1
    for b in last:
        j = mtf.index(index[b])
        if j == 0:
            run += 1
            continue
        flush()
        syms.append(j + 1)
        mtf.insert(0, mtf.pop(j))
    flush()
    syms.append(len(used) + 1)
    return syms


def mtf_decode(symbols, used):
    """the last-column vector a decoder gets from a symbol list (up to its end-of-block symbol)"""
    mtf = list(range(len(used)))
    out = bytearray()
    eob = len(used) + 1
    i = 0
    while symbols[i] != eob:
        s = symbols[i]
        if s < 2:
            es, n = 0, 1
            while symbols[i] < 2:
                es += n << symbols[i]
                n <<= 1
                i += 1
            out += bytes([used[mtf[0]]]) * es
            continue
        mtf.insert(0, mtf.pop(s - 1))
        out.append(used[mtf[0]])
        i += 1
    return bytes(out)


# ---- codes ---------------------------------------------------------------------------------------------------------------------
def huffman_lengths(freqs, max_len=17):
    """code lengths of a Huffman code in which every symbol has one; frequencies are flattened until none exceeds max_len"""
    freqs = [max(f, 1) for f in freqs]
    if len(freqs) == 1:
        return [1]
    while True:
        heap = [(f, i, (i,)) for i, f in enumerate(freqs)]
        heapq.heapify(heap)
        lengths = [0] * len(freqs)
        tie = len(freqs)
        while len(heap) > 1:
            fa, _, a = heapq.heappop(heap)
            fb, _, b = heapq.heappop(heap)
            for s in a + b:
                lengths[s] += 1
            heapq.heappush(heap, (fa + fb, tie, a + b))
            tie += 1
        if max(lengths) <= max_len:
            return lengths
        freqs = [(f >> 1) + 1 for f in freqs]


def canonical_codes(lengths):
    """code of every symbol: by length, then by symbol index.  Not checked: an incomplete code leaves values unused, an
    oversubscribed one gives some symbols a value that does not fit their length (code_bits refuses to write those)"""
    codes = [0] * len(lengths)
    vec = 0
    for ln in range(min(lengths), max(lengths) + 1):
        for i, li in enumerate(lengths):
            if li == ln:
                codes[i] = vec
                vec += 1
        vec <<= 1
    return codes


def _final(entry):
    return entry if isinstance(entry, int) else entry[-1]


def _length_table_bits(table):
    """5 bits of the first length, then per symbol: "10" = one up, "11" = one down, "0" = this is it.  An entry is a length, or a
    path of lengths that is walked in steps of one before the last of them is settled on"""
    first = table[0] if isinstance(table[0], int) else table[0][0]
    out = [bits(first, 5)]
    curr = first
    for entry in table:
        for target in ((entry,) if isinstance(entry, int) else entry):
            while curr < target:
                out.append("10")
                curr += 1
            while curr > target:
                out.append("11")
                curr -= 1
        out.append("0")
    return "".join(out)


# ---- a block -------------------------------------------------------------------------------------------------------------------
def block(text=None, pre=None, last=None, orig_ptr=None, symbols=None, used=None, lengths=None, n_tables=2, selectors=None,
          extra_selectors=0, randomised=False, crc=None):
    """One block, from the first of text / pre / last / symbols that is given:
      text      RLE1, BWT, MTF, Huffman — what an encoder does
      pre       the pre-BWT bytes as they stand (RLE1 is not run again)
      last      the last-column vector, with any orig_ptr (default 0) — it need not be a real BWT
      symbols   the symbol list, end-of-block symbol included, over the bytes `used` (orig_ptr default 0)
    used: the bytes marked in use (default: those that occur).  lengths: 2 to 6 tables of len(used) + 2 entries, each a length
    1..20 or a path of lengths (default: n_tables copies of a Huffman code).  selectors: a table per 50 symbols (default: all 0);
    extra_selectors more are written behind them.  crc: the header's CRC (default: that of the text a decoder gets — the writer's
    own inverse BWT and un-RLE1 of what it wrote, which for a randomised block is the text before libbz2 de-randomises it)."""
    if text is not None:
        pre = rle1(text)
    if pre is not None:
        last, real_orig = bwt(pre)
        if orig_ptr is None:
            orig_ptr = real_orig
    if orig_ptr is None:
        orig_ptr = 0
    if last is not None:
        if used is None:
            used = sorted(set(last))
        symbols = mtf_encode(last, used)
    else:
        last = mtf_decode(symbols, used)
    used = list(used)
    alpha = len(used) + 2
    decoded = None
    if crc is None:
        decoded = un_rle1(inverse_bwt(last, orig_ptr))
        crc = crc32(decoded)
    if lengths is None:
        freqs = [0] * alpha
        for s in symbols:
            freqs[s] += 1
        lengths = [huffman_lengths(freqs)] * n_tables
    assert 2 <= len(lengths) <= 6 and all(len(t) == alpha for t in lengths)
    needed = (len(symbols) + G_SIZE - 1) // G_SIZE
    if selectors is None:
        selectors = [0] * needed
    assert len(selectors) >= needed
    selectors = list(selectors) + [0] * extra_selectors
    assert len(selectors) < (1 << 15)

    out = [bits(BLOCK_MAGIC, 48), bits(crc, 32), "1" if randomised else "0", bits(orig_ptr, 24)]
    rows = [sum(1 << (15 - j) for j in range(16) if i * 16 + j in used) for i in range(16)]
    out.append(bits(sum(1 << (15 - i) for i in range(16) if rows[i]), 16))
    out += [bits(r, 16) for r in rows if r]
    out += [bits(len(lengths), 3), bits(len(selectors), 15)]
    order = list(range(len(lengths)))
    for s in selectors:
        j = order.index(s)
        out.append("1" * j + "0")
        order.insert(0, order.pop(j))
    final = []
    for table in lengths:
        out.append(_length_table_bits(table))
        final.append([_final(e) for e in table])
    code_bits = []
    for t in final:
        codes = canonical_codes(t)
        code_bits.append([bits(c, ln) if c < (1 << ln) else None for c, ln in zip(codes, t)])
    for k, s in enumerate(symbols):
        b = code_bits[selectors[k // G_SIZE]][s]
        if b is None:
            raise ValueError("symbol %d has no code of its length in table %d" % (s, selectors[k // G_SIZE]))
        out.append(b)
    return Block("".join(out), crc, decoded, len(last), len(selectors), len(lengths), max(max(t) for t in final), symbols)


def stream(level, blocks, combined=None):
    """a .bz2 image: "BZh" + level, the blocks, the end-of-stream magic, the combined CRC, padding to a whole byte"""
    if combined is None:
        combined = combine(b.crc for b in blocks)
    body = "".join([b.bits for b in blocks] + [bits(EOS_MAGIC, 48), bits(combined, 32)])
    body += "0" * (-len(body) % 8)
    return b"BZh" + bytes([0x30 + level]) + int(body, 2).to_bytes(len(body) // 8, "big")


def compress(text, level=9, block_bytes=2000):
    """text -> .bz2 the way an encoder goes, block_bytes of text to a block (the run state never crosses a block boundary)"""
    return stream(level, [block(text=text[o:o + block_bytes]) for o in range(0, len(text), block_bytes)])
