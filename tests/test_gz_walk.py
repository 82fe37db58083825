"""tests/gz_walk.py proven on streams made with zlib alone, before it judges the device encoders (test_gpu_gzdev.py).  No GPU."""
import struct
import zlib

import pytest

import gz_walk


def bgzf_member(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    size = 18 + len(raw) + 8
    return gz_walk.BGZF_HEAD + bytes([0, 0, 0, 0, 0, 0xff]) + b"\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + raw + struct.pack("<II", zlib.crc32(data), len(data))


def two_members():
    text = b"".join(b"@r%d\nACGTTGCAAC%s\n+\nIIIIIHHHHH%s\n" % (i, b"ACGT"[i % 4:] * 9, b"F" * (36 - 9 * (i % 4))) for i in range(60))
    piece = 1000
    text = text[:piece + 300]
    return text, piece, bgzf_member(text[:piece], 0) + bgzf_member(text[piece:], 6)


def test_walker_reads_a_two_member_stream():
    text, piece, gz = two_members()
    assert gz_walk.inflate_all(gz) == text
    members = gz_walk.check_stream(gz, text, piece)
    assert [m["isize"] for m in members] == [piece, 300]
    assert [m["offset"] for m in members] == [0, members[0]["size"]] and sum(m["size"] for m in members) == len(gz)
    assert members[0]["btype"] == gz_walk.STORED and members[0]["size"] == piece + 5 + 26
    assert members[1]["btype"] in (gz_walk.FIXED, gz_walk.DYNAMIC) and members[1]["size"] < 300
    assert members[0]["text"] + members[1]["text"] == text


@pytest.mark.parametrize("damage", ["bsize_short", "bsize_long", "magic", "subfield", "crc", "isize", "tail_cut", "wrong_piece", "one_member_too_few", "oversize"])
def test_walker_refuses_what_is_wrong(damage):
    text, piece, gz = two_members()
    first = struct.unpack_from("<H", gz, 16)[0] + 1
    b = bytearray(gz)
    if damage == "bsize_short":
        struct.pack_into("<H", b, 16, first - 2)
    elif damage == "bsize_long":
        struct.pack_into("<H", b, 16, first)
    elif damage == "magic":
        b[first + 3] = 0
    elif damage == "subfield":
        b[first + 12] = ord("X")
    elif damage == "crc":
        b[first - 8] ^= 1
    elif damage == "isize":
        b[first - 4] ^= 1
    elif damage == "tail_cut":
        del b[-1:]
    elif damage == "wrong_piece":
        piece = 999                # the members are sound, only not cut where the caller says
    elif damage == "one_member_too_few":
        b = bytearray(bgzf_member(text, 6))
    elif damage == "oversize":
        # a sound member that takes more than a stored block would: an empty stored block in front of the stored text
        data = text[:piece]
        raw = b"\x00\x00\x00\xff\xff" + b"\x01" + struct.pack("<HH", piece, piece ^ 0xffff) + data
        size = 18 + len(raw) + 8
        b = bytearray(gz_walk.BGZF_HEAD + bytes([0, 0, 0, 0, 0, 0xff]) + b"\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + raw + struct.pack("<II", zlib.crc32(data), piece))
        b += gz[first:]
    with pytest.raises(AssertionError):
        gz_walk.check_stream(bytes(b), text, piece)
