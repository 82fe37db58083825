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
