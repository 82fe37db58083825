"""Shared by the gzip-output tests: a walker over BGZF-framed gzip streams (what aqc_compress and the pipe's .gz writer put
out) that trusts nothing but zlib.  walk() parses every member's 18-byte header and inflates the member on its own;
check_stream() holds a whole stream against the text it must carry and the member size it was cut by."""
import struct
import zlib

BGZF_HEAD = bytes([0x1f, 0x8b, 8, 4])          # magic, CM = deflate, FLG = FEXTRA
BGZF_EXTRA = b"\x06\x00BC\x02\x00"             # XLEN = 6, subfield 'B' 'C' of 2 bytes: BSIZE - 1
STORED, FIXED, DYNAMIC = 0, 1, 2


def walk(gz):
    """every member of a BGZF-framed stream, in order: dicts of offset, size (BSIZE), btype / bfinal of its first deflate block,
    isize and crc from its trailer, and text (the member inflated on its own).  Raises AssertionError when a header is not
    BGZF's, when walking by BSIZE does not land exactly on the end, or when a member does not inflate to what its trailer says."""
    gz = bytes(gz)
    out = []
    off = 0
    while off < len(gz):
        assert len(gz) - off >= 18 + 2 + 8, "member %d at %d: %d bytes left, less than the smallest member" % (len(out), off, len(gz) - off)
        head = gz[off:off + 18]
        assert head[:4] == BGZF_HEAD, "member %d at %d: header %s" % (len(out), off, head[:4].hex())
        assert head[10:16] == BGZF_EXTRA, "member %d at %d: extra field %s" % (len(out), off, head[10:16].hex())
        size = struct.unpack_from("<H", head, 16)[0] + 1
        assert off + size <= len(gz), "member %d at %d: BSIZE %d runs past the stream's end %d" % (len(out), off, size, len(gz))
        first = gz[off + 18]
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(gz[off + 18:off + size - 8])
        except zlib.error as e:
            raise AssertionError("member %d at %d: zlib: %s" % (len(out), off, e))
        assert d.eof and d.unused_data == b"", "member %d at %d: its deflate data does not end where BSIZE says" % (len(out), off)
        crc, isize = struct.unpack_from("<II", gz, off + size - 8)
        assert isize == len(text), "member %d at %d: ISIZE %d, %d bytes inflated" % (len(out), off, isize, len(text))
        assert crc == zlib.crc32(text), "member %d at %d: CRC-32 %08x, text has %08x" % (len(out), off, crc, zlib.crc32(text))
        out.append({"offset": off, "size": size, "bfinal": first & 1, "btype": (first >> 1) & 3, "isize": isize, "crc": crc, "text": text})
        off += size
    assert off == len(gz)
    return out


def inflate_all(gz):
    """the whole stream through zlib's own gzip reader, member after member (it checks every CRC-32 and ISIZE)"""
    gz = bytes(gz)
    out = []
    while gz:
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(gz))
        except zlib.error as e:
            raise AssertionError("member %d: zlib: %s" % (len(out), e))
        assert d.eof, "the stream ends inside a member"
        gz = d.unused_data
    return b"".join(out)


def check_stream(gz, text, member_text):
    """a stream that carries `text` cut into members of `member_text` bytes: zlib reads it back whole; there are
    ceil(len(text) / member_text) members; every one inflates on its own to its slice, says so in ISIZE, starts with a final
    block, and is no larger than its text + 5 (a stored block's header) + 26 (member header and trailer).  -> walk()'s members"""
    text = bytes(text)
    assert inflate_all(gz) == text, "the stream does not decompress to its text"
    members = walk(gz)
    n = -(-len(text) // member_text)
    assert len(members) == n, "%d members for %d bytes in pieces of %d: %d expected" % (len(members), len(text), member_text, n)
    for k, m in enumerate(members):
        piece = text[k * member_text:(k + 1) * member_text]
        assert m["isize"] == len(piece), "member %d: ISIZE %d, its piece has %d bytes" % (k, m["isize"], len(piece))
        assert m["text"] == piece, "member %d does not inflate to its own piece of the text" % k
        assert m["bfinal"] == 1, "member %d: its first block is not its last" % k
        assert m["size"] <= len(piece) + 5 + 26, "member %d: %d bytes for %d of text, more than a stored block takes" % (k, m["size"], len(piece))
    return members
