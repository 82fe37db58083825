"""The .bz2 inputs that test_bz2_dev_cpu.py (the device's functions on the CPU) and test_gpu_bunzip2.py (the kernels) both decode:
edges of the format chosen small — Python's bz2 module writes them and is the oracle.  Not a test module."""
import bz2
import functools
import random

from afterqc_amd import synth

BLOCK_MAGIC = 0x314159265359


def fastq_text(n_pairs, seed):
    d = synth.make_pairs(n_pairs, 150, seed=seed, dirty=True)
    buf, n = synth.render_fastq_fixed(d["seq1"], d["qual1"], 1)
    return bytes(memoryview(buf)[:n])


def first_block_tables(bz):
    """nGroups of the first block of a .bz2 image: behind "BZhN", the 48-bit magic, CRC (32), randomised (1), origPtr (24) and
    the symbol map (16 bits + 16 for each that is set)"""
    bits = int.from_bytes(bz[4:4 + 64].ljust(64, b"\0"), "big")
    total = 64 * 8

    def take(pos, n):
        return (bits >> (total - pos - n)) & ((1 << n) - 1)
    assert take(0, 48) == BLOCK_MAGIC
    pos = 48 + 32 + 1 + 24
    used = take(pos, 16)
    pos += 16 + 16 * bin(used).count("1")
    return take(pos, 3)


@functools.lru_cache(maxsize=None)
def block_starts(bz):
    """bit positions of the block magic in a .bz2 image (a brute-force scan: small inputs only)"""
    v = int.from_bytes(bz, "big")
    n = len(bz) * 8
    return [p for p in range(n - 47) if (v >> (n - p - 48)) & ((1 << 48) - 1) == BLOCK_MAGIC]


def _letters(rng, n, alphabet=b"ACGTN#,-5:<AFJ"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _distinct(rng, k):
    """k distinct byte values in a seeded order: no byte repeats, so MTF gives no zero and the block has exactly k + 1 symbols
    (the end-of-block symbol included)"""
    v = list(range(256 - k, 256))
    rng.shuffle(v)
    return bytes(v)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, .bz2 image, text)]: every image is valid, Python's bz2 decodes it to text"""
    rng = random.Random(20260)
    out = []

    def add(name, text, level=9):
        out.append((name, bz2.compress(text, level), text))
    add("empty", b"")
    add("one_byte", b"x")
    for k in (3, 4, 5, 258, 259, 260, 1000):
        add("A_x_%d" % k, b"A" * k)
    add("run_of_4_ends_the_block", b"hello, world" + b"Z" * 4)
    add("run_of_7_ends_the_block", b"hello, world" + b"Z" * 7)
    add("run_of_259_ends_the_block", b"hello, world" + b"Z" * 259)
    add("all_256_values", bytes(range(256)) * 4)
    add("byte_0_alone", b"\x00" * 7)
    add("byte_255_alone", b"\xff" * 7)
    add("bytes_0_and_255", b"\x00\xff" * 100)
    # two .. six Huffman tables: fewer than 200 / 600 / 1,200 / 2,400 symbols, and more
    for n in (120, 420, 950, 1900, 6000):
        add("letters_%d" % n, _letters(rng, n))
    # 200 symbols (four full selector groups) and 201 (a partial last group); 100 and 250 likewise
    for k in (99, 199, 200, 249):
        add("distinct_%d" % k, _distinct(rng, k))
    add("ACGT_x_50000", b"ACGT" * 50000)
    add("zeros_1MB", b"\x00" * 1_000_000)
    fq = fastq_text(1100, 5150)[:350_000]
    add("fastq_level_1", fq, 1)
    add("fastq_level_9", fq, 9)
    third = len(fq) // 3
    out.append(("three_streams_and_an_empty_one",
                bz2.compress(fq[:third], 1) + bz2.compress(b"") + bz2.compress(fq[third:2 * third], 9) + bz2.compress(b"") + bz2.compress(fq[2 * third:], 5), fq))
    out.append(("stream_then_garbage", bz2.compress(fq[:60_000], 1) + bytes(rng.randrange(256) for _ in range(100)), fq[:60_000]))
    add("random_64KB", bytes(rng.randrange(256) for _ in range(65536)))
    return out


def case(name):
    for c in valid_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """[(name, image)]: bz2.decompress raises for each"""
    _, good, _ = case("fastq_level_1")
    starts = block_starts(good)
    assert len(starts) == 4 and any(s % 8 for s in starts), starts          # four blocks, at unaligned bit positions
    mid = bytearray(good)
    mid[(starts[1] + starts[2]) // 16] ^= 0x10                              # the middle of the second block
    cut = good[:len(good) * 2 // 3]
    trailer = bytearray(good)
    trailer[-3] ^= 0x04                                                     # the combined CRC (the last 32 bits before the padding)
    return [("flipped_bit_in_a_block", bytes(mid)), ("cut_at_two_thirds", cut), ("flipped_bit_in_the_trailer_crc", bytes(trailer))]


# ---- crafted images (tests/bz2_writer.py): legal corners of the format that libbz2's encoder never writes ----------------------------
EOS_MAGIC = 0x177245385090


def magic_hits(bz, magic):
    """sorted bit positions of a 48-bit magic in an image of any size (linear: the image shifted by 0..7 bits, searched as bytes)"""
    v = int.from_bytes(bz, "big")
    pat = magic.to_bytes(6, "big")
    hits = []
    for s in range(8):
        shifted = (v >> s).to_bytes(len(bz), "big")          # its byte k holds the image's bits [8 k - s, 8 k - s + 8)
        k = shifted.find(pat)
        while k >= 0:
            hits.append(8 * k - s)
            k = shifted.find(pat, k + 1)
    return sorted(hits)


def block_header(bz, bit):
    """the header of the block whose magic stands at `bit`: the randomised bit, origPtr, bytes in use, nGroups, nSelectors and the
    longest code length of any of its tables"""
    chunk = bz[bit // 8:bit // 8 + 48_000]                     # (the longest header: 32,767 selectors x 6 bits, 6 x 258 x ~40 bits of lengths)
    v = int.from_bytes(chunk, "big")
    total = len(chunk) * 8
    pos = bit % 8

    def take(n):
        nonlocal pos
        pos += n
        return (v >> (total - pos)) & ((1 << n) - 1)
    assert take(48) == BLOCK_MAGIC
    h = {"crc": take(32), "randomised": take(1), "orig_ptr": take(24)}
    rows = take(16)
    h["in_use"] = sum(bin(take(16)).count("1") for i in range(16) if (rows >> (15 - i)) & 1)
    h["n_tables"] = take(3)
    h["n_selectors"] = take(15)
    for _ in range(h["n_selectors"]):
        while take(1):
            pass
    h["max_len"] = 0
    for _ in range(h["n_tables"]):
        curr = take(5)
        for _ in range(h["in_use"] + 2):
            while take(1):
                curr += -1 if take(1) else 1
                h["max_len"] = max(h["max_len"], curr)          # (lengths passed through on a path count: the decoder has to bear them)
            h["max_len"] = max(h["max_len"], curr)
    return h


MAGIC_SYMBOLS = {"block": [12, 20, 5, 25, 9, 37, 13, 25], "eos": [5, 55, 9, 5, 14, 5, 2, 16]}      # the two magics in groups of six bits


@functools.lru_cache(maxsize=None)
def _crafted():
    """[(name, image, class, device blocks)] — see crafted_cases()"""
    import bz2_writer as w
    rng = random.Random(20261)
    out = []

    def add(name, level, blocks, cls, dev_blocks=None, image=None):
        if image is None:
            image = w.stream(level, blocks)
        out.append((name, image, cls, len(blocks) if dev_blocks is None else dev_blocks))

    # code lengths up to 20 (BZB_MAX_LEN): libbz2's encoder stops at 17
    used19 = list(range(65, 84))                                            # 19 bytes in use: alpha = 21
    last = bytes(rng.choice(used19) for _ in range(300))
    syms = w.mtf_encode(last, used19)
    add("len20_both_tables", 9, [w.block(last=last, used=used19, lengths=[[20] * 21] * 2)], "exact")
    one_to_20 = [min(i + 1, 20) for i in range(21)]                        # 1, 2, .. 19, 20, 20: a complete code
    add("len_1_to_20", 9, [w.block(last=last, used=used19, lengths=[[20] * 21, one_to_20],
                                   selectors=[(k + 1) % 2 for k in range((len(syms) + 49) // 50)])], "exact")
    text = _letters(rng, 900)
    b = w.block(text=text)
    n_sel = (len(b.symbols) + 49) // 50
    assert len(b.symbols) < 1000
    add("six_tables_tiny_block", 9, [w.block(text=text, n_tables=6, selectors=[k % 6 for k in range(n_sel)])], "exact")
    # more selectors than the block needs (lbzip2 pads them; beyond 18,002 they are read and dropped)
    add("extra_selectors_7", 9, [w.block(text=text, extra_selectors=7)], "exact")
    add("selectors_over_18002", 9, [w.block(text=text, n_tables=3, extra_selectors=18010)], "exact")

    # origPtr
    real_last, _ = w.bwt(w.rle1(_letters(rng, 500)))
    add("orig_ptr_last", 9, [w.block(last=real_last, orig_ptr=len(real_last) - 1)], "exact")
    add("orig_ptr_equals_nblock", 9, [w.block(last=real_last, orig_ptr=len(real_last), crc=w.crc32(_letters(rng, 500)))], "error")
    add("not_a_bwt_vector", 9, [w.block(last=bytes(rng.randrange(256) for _ in range(5000)), orig_ptr=17)], "exact")

    # RLE1: the count byte's range, the run state behind a count byte and across a block boundary, a run with no count byte
    add("count_255", 9, [w.block(pre=b"ZZZZ\xff")], "exact")
    add("count_0_twice", 9, [w.block(pre=b"ZZZZ\0ZZZZ\0Z")], "exact")
    add("ends_on_three_then_same_byte", 9, [w.block(pre=b"helloZZZ"), w.block(pre=b"ZZ\x03world")], "exact")
    four = w.block(pre=b"helloZZZZ")
    assert four.text == b"helloZZZZ" and four.crc == w.crc32(b"helloZZZZ")
    add("ends_on_four_equal", 9, [four], "error")
    add("ends_on_four_equal_then_block", 9, [four, w.block(text=b"hello, world")], "error")

    # a block filled to the last byte of level x 100,000 (libbz2's encoder stops 19 short), and one byte beyond
    acgt = bytes(rng.choice(b"ACGT") for _ in range(100_001))
    add("nblock_100000_level_1", 1, [w.block(last=acgt[:100_000])], "exact")
    by_a_run = acgt[:99_997] + bytes([acgt[99_996] ^ 6]) * 3              # 99,998 bytes, then the last of them twice more: a run of 2
    b = w.block(last=by_a_run)
    assert len(by_a_run) == 100_000 and b.symbols[-2] == 1 and b.symbols[-3] > 1            # (... RUNB, end of block)
    add("nblock_100000_by_a_run", 1, [b], "exact")
    add("nblock_100001_level_1", 1, [w.block(last=acgt)], "error")

    # the two magics inside a block's symbol stream: 62 bytes in use, alpha 64, every code six bits long = the symbol's own value
    used62 = list(range(48, 110))
    normal = w.block(text=b"a normal block follows")
    for which, cls_blocks in (("block", 3), ("eos", 2)):
        head = [rng.randrange(2, 63) for _ in range(70)]
        tail = [rng.randrange(2, 63) for _ in range(70)]
        b = w.block(symbols=head + MAGIC_SYMBOLS[which] + tail + [63], used=used62, lengths=[[6] * 64] * 2)
        add("%s_magic_inside_a_block" % which, 9, [b, normal], "exact")

    # the randomised bit (bzip2 before 0.9.5): handed back to libbz2.  Its first toggle falls at byte 618 of the block
    fq = fastq_text(30, 5151)
    add("randomised_flag_bad_crc", 9, [w.block(text=fq[:1500], randomised=True)], "error")
    add("randomised_short_block_mid_stream", 9, [w.block(text=fq[:2000]), w.block(text=fq[2000:2400], randomised=True), w.block(text=fq[2400:4400])],
        "handback", dev_blocks=1)

    # more candidates than the device's list of 65,536 holds: the window shrinks to an eighth and slides / the host takes over
    add("blocks_65537_one_byte_each", 1, [w.block(text=b"x")] * 65537, "exact")
    tiny = bz2.compress(fastq_text(200, 5152)[:60_000], 1)
    add("stream_then_70000_block_magics", 1, [], "handback", dev_blocks=0, image=tiny + BLOCK_MAGIC.to_bytes(6, "big") * 70_000)

    # no prediction from the format: libbz2 rules.  What this project's decoder should make of them if libbz2 accepts them is
    # read from csrc/aqc_bunzip2_dev.hpp: an oversubscribed code decodes like any other (only its first values can occur), a
    # symbol with more than BZB_MAX_DELTAS = 64 length deltas is refused and handed back
    over = [[3] * 9, [3, 3, 3, 3, 3, 3, 3, 4, 4]]                          # table 0: nine symbols of length 3 (only the first eight can occur)
    group0 = [(2 + k % 6) if k % 7 else k % 2 for k in range(50)]
    b = w.block(symbols=group0 + [7, 3, 0, 1, 5, 8], used=list(range(65, 72)), lengths=over, selectors=[0, 1])
    add("oversubscribed_code", 9, [b], _oracle_class(w.stream(9, [b]), "exact"))
    zigzag = [[5, (5, 20, 5, 20, 5, 20, 5, 20, 5), 5, 5, 5]] * 2          # symbol 1: 8 x 15 = 120 deltas
    b = w.block(symbols=[2, 3, 0, 1, 2, 4], used=[65, 66, 67], lengths=zigzag)
    add("length_deltas_120", 9, [b], _oracle_class(w.stream(9, [b]), "handback"), dev_blocks=0)
    return out


def _oracle_class(image, accepted):
    try:
        bz2.decompress(image)
    except (OSError, ValueError, EOFError):
        return "error"
    return accepted


def crafted_cases():
    """[(name, .bz2 image, class)] built with tests/bz2_writer.py.  exact: the device decodes every block, none goes to the host;
    handback: the text is exact but libbz2 finished the stream; error: bz2.decompress raises, and so must the device"""
    return [c[:3] for c in _crafted()]


def crafted_case(name):
    """(name, image, class, blocks the device decodes)"""
    for c in _crafted():
        if c[0] == name:
            return c
    raise KeyError(name)
