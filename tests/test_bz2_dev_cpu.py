"""csrc/aqc_bunzip2_dev.hpp on the CPU (no GPU): the functions a lane of the device bunzip2 runs — block scan, entropy stage,
inverse BWT, RLE1 + CRC, chain — compiled with g++ and dealt out by plain loops (tests/native/bzb_selftest.cpp) through the
same stream walk that drives the kernels (csrc/aqc_bz2.hpp), over the inputs test_gpu_bunzip2.py gives the device.  Python's
bz2 module (fastq.py:25-26 upstream: bz2.BZ2File) is the oracle."""
import bz2
import os
import subprocess

import pytest

import bz2_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 30


def _build(tmp, flags):
    exe = os.path.join(tmp, "bzb_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "bzb_selftest.cpp"), "-ldl", "-o", exe])
    return exe


def _oracle(image):
    """the text Python's bz2 makes of an image, None where it raises"""
    try:
        return bz2.decompress(image)
    except (OSError, ValueError, EOFError):
        return None


def _manifest(tmp):
    """every valid case with one window, the multi-block ones also in groups of 1 / 2 blocks, in windows that cut blocks short and
    with room for one block's text per group; the damaged ones; the crafted ones"""
    lines = []

    def put(name, image, text, window, group, out_cap, want):
        p = os.path.join(tmp, "%s.%d.bz2" % (name, len(lines)))
        with open(p, "wb") as f:
            f.write(image)
        t = "-"
        if text is not None:
            t = p + ".txt"
            with open(t, "wb") as f:
                f.write(text)
        lines.append("%s %s %d %d %d %s" % (p, t, window, group, out_cap, want))
    for name, image, text in bz2_cases.valid_cases():
        assert bz2.decompress(image) == text, name
        put(name, image, text, BIG, 0, BIG, "exact")
    for name in ("fastq_level_1", "three_streams_and_an_empty_one"):
        _, image, text = bz2_cases.case(name)
        for group in (1, 2):
            put(name, image, text, BIG, group, BIG, "exact")
        put(name, image, text, 1 << 16, 3, BIG, "exact")        # (64 KiB windows: a level-1 block of FASTQ is ~25 KB — every window cuts one short)
        put(name, image, text, BIG, 4, 120_000, "exact")        # (text of one 100,000-byte block per group)
    for name, image in bz2_cases.damaged_cases():
        with pytest.raises((OSError, ValueError, EOFError)):
            bz2.decompress(image)
        put(name, image, None, BIG, 0, BIG, "error")
        put(name, image, None, 1 << 16, 1, BIG, "error")
    # the crafted images (tests/bz2_writer.py): Python's bz2 says what each is; one window, groups of one block, 64 KiB windows
    for name, image, cls in bz2_cases.crafted_cases():
        text = _oracle(image)
        assert (text is None) == (cls == "error"), name
        for window, group in ((BIG, 0), (BIG, 1), (1 << 16, 0)):
            want = cls
            if name == "stream_then_70000_block_magics" and window == 1 << 16:
                # (what hands this one back is the overflow of the candidate list, and a 64 KiB window holds at most
                #  65,536 x 8 / 48 = 10,922 magics: the stream's one block and its end are found in the first window)
                want = "exact"
            put(name, image, text, window, group, BIG, want)
    m = os.path.join(tmp, "manifest.txt")
    with open(m, "w") as f:
        f.write("\n".join(lines) + "\n")
    return m, len(lines)


def test_the_cases_cover_the_format_edges():
    """two to six Huffman tables, a full and a partial last selector group — read from the images themselves"""
    tables = {name: bz2_cases.first_block_tables(image) for name, image, text in bz2_cases.valid_cases() if text}
    assert {tables["letters_%d" % n] for n in (120, 420, 950, 1900, 6000)} == {2, 3, 4, 5, 6}, tables
    assert len(bz2_cases.block_starts(bz2_cases.case("fastq_level_9")[1])) == 1


def test_the_crafted_cases_are_what_they_claim():
    """the corners the crafted images are there for, read back from the images, and each case's class against Python's bz2"""
    cases = {name: (image, cls) for name, image, cls in bz2_cases.crafted_cases()}
    assert len(cases) == len(bz2_cases.crafted_cases()) == 24

    def first(name):
        return bz2_cases.block_header(cases[name][0], 32)
    classes = {}
    for name, (image, cls) in cases.items():
        assert len(image) <= 1_500_000, name
        text = _oracle(image)
        assert cls in ("exact", "handback", "error") and (text is None) == (cls == "error"), (name, cls)
        classes[cls] = classes.get(cls, 0) + 1
    assert classes == {"exact": 16, "handback": 3, "error": 5}, classes
    assert _oracle(cases["ends_on_three_then_same_byte"][0]) == b"helloZZZZZ\x03world"
    assert len(_oracle(cases["count_255"][0])) == 259 and _oracle(cases["count_0_twice"][0]) == b"Z" * 9
    # code lengths up to 20, in one table and in all; six tables on a block of under 1,000 symbols
    assert first("len20_both_tables")["max_len"] == 20 and first("len_1_to_20")["max_len"] == 20
    assert first("length_deltas_120")["max_len"] == 20
    assert first("six_tables_tiny_block")["n_tables"] == 6
    # selectors: 7 more than 50 symbols each need, and more than the 18,002 a decoder keeps
    base = first("six_tables_tiny_block")["n_selectors"]
    assert first("extra_selectors_7")["n_selectors"] == base + 7 and base <= 20
    assert first("selectors_over_18002")["n_selectors"] == base + 18010 > 18002
    # origPtr at the last row and one beyond it (the same vector of ~500 bytes in both)
    assert first("orig_ptr_equals_nblock")["orig_ptr"] == first("orig_ptr_last")["orig_ptr"] + 1 > 400
    assert len(cases["orig_ptr_equals_nblock"][0]) == len(cases["orig_ptr_last"][0])
    # a magic inside a block: more hits than blocks
    for name, n_blk, n_eos in (("block_magic_inside_a_block", 3, 1), ("eos_magic_inside_a_block", 2, 2)):
        image = cases[name][0]
        assert len(bz2_cases.magic_hits(image, bz2_cases.BLOCK_MAGIC)) == n_blk and bz2_cases.magic_hits(image, bz2_cases.BLOCK_MAGIC) == bz2_cases.block_starts(image), name
        assert len(bz2_cases.magic_hits(image, bz2_cases.EOS_MAGIC)) == n_eos, name
        assert bz2_cases.crafted_case(name)[3] == 2
        assert first(name)["in_use"] == 62 and first(name)["max_len"] == 6
    # the randomised bit: on the only block, and on the second of three
    assert first("randomised_flag_bad_crc")["randomised"] == 1
    image = cases["randomised_short_block_mid_stream"][0]
    starts = bz2_cases.block_starts(image)
    assert [bz2_cases.block_header(image, s)["randomised"] for s in starts] == [0, 1, 0]
    # more magics than the device's candidate list of 65,536 holds
    image = cases["blocks_65537_one_byte_each"][0]
    assert len(image) == 1_466_405 and len(bz2_cases.magic_hits(image, bz2_cases.BLOCK_MAGIC)) == 65537
    assert len(bz2_cases.magic_hits(image, bz2_cases.EOS_MAGIC)) == 1
    image = cases["stream_then_70000_block_magics"][0]
    assert len(bz2_cases.magic_hits(image, bz2_cases.BLOCK_MAGIC)) == 70001 and len(image) <= 1 << 20


def test_the_writer_round_trips_through_bz2():
    """tests/bz2_writer.py from text — RLE1, BWT, MTF, Huffman, CRCs — is a bzip2 encoder: Python's bz2 decodes what it writes"""
    import bz2_writer
    fq = bz2_cases.fastq_text(20, 5153)[:2048]
    assert len(fq) == 2048
    texts = [b"", b"x", bytes(range(256)), bytes(range(256)) * 3, fq, b"hello, world" + b"Z" * 4 + b"!"]
    texts += [b"A" * k for k in (3, 4, 5, 259, 260, 1000)] + [b"ab" + b"Z" * k + b"cd" for k in (3, 4, 5, 259, 260)]
    for text in texts:
        assert bz2.decompress(bz2_writer.compress(text)) == text, text[:40]
    # several blocks to a stream (the combined CRC), at every level
    for level in (1, 5, 9):
        image = bz2_writer.compress(fq, level, block_bytes=700)
        assert len(bz2_cases.block_starts(image)) == 3 and bz2.decompress(image) == fq
    assert bz2_writer.crc32(b"123456789") == 0xfc891918                   # (the check value of CRC-32/BZIP2)
    assert bz2_writer.rle1(b"A" * 260 + b"B" * 4) == b"AAAA\xffA" + b"BBBB\x00"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_device_bunzip2_logic_on_the_cpu(tmp_path, flags):
    """byte-identical text with NO block handed back to libbz2 for every valid input (so the GPU test's cap of zero host blocks
    hides nothing), a negative status for every damaged one; the crafted images as their classes say (exact / handback /
    error); once more as a stand-alone ASan / UBSan binary"""
    tmp = str(tmp_path)
    exe = _build(tmp, flags)
    manifest, n = _manifest(tmp)
    out = subprocess.run([exe, manifest], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all %d device-bunzip2 logic checks passed" % n in out.stdout, out.stdout[-3000:]
