"""What a BGZF stream of leon_text_bgzf_device has to be, checked in pure Python against the text it holds: the members
are walked by BSIZE, every header byte is compared, each payload is inflated on its own with zlib and set against its slice of the text,
and the whole must be what gzip.decompress reads.  Never against the code under test."""
import gzip
import struct
import zlib

MEMBER_TEXT = 32768
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")      # the 16 bytes in front of BSIZE
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FRAME = 28                                                       # header 18, 03 00, CRC-32, ISIZE
STORED = 5 + FRAME                                               # what the stored form adds to its slice


def walk(out):
    """[(start, size)] of every member, the EOF marker included if it is there"""
    at, found = 0, []
    while at < len(out):
        assert len(out) - at >= FRAME, "a member of %d bytes at %d" % (len(out) - at, at)
        assert out[at:at + 16] == HEAD, "member at %d: header %s" % (at, out[at:at + 16].hex())
        size = struct.unpack_from("<H", out, at + 16)[0] + 1
        assert FRAME <= size <= len(out) - at, "member at %d: BSIZE + 1 = %d, %d bytes left" % (at, size, len(out) - at)
        found.append((at, size))
        at += size
    return found


def check(out, text, eof=True):
    """`out` is the BGZF of `text`: members of MEMBER_TEXT bytes of text (the last one what is left), then -- eof -- the EOF marker.
    Returns the data members' payload sizes (member bytes - 28)."""
    out, text = bytes(out), bytes(text)
    members = walk(out)
    if eof:
        assert out[-28:] == EOF, "the stream does not end with the EOF marker: " + out[-28:].hex()
        assert members and members[-1] == (len(out) - 28, 28)
        members = members[:-1]
    n = (len(text) + MEMBER_TEXT - 1) // MEMBER_TEXT
    assert len(members) == n, "%d data members for %d bytes of text" % (len(members), len(text))
    payloads = []
    for i, (at, size) in enumerate(members):
        part = text[i * MEMBER_TEXT:(i + 1) * MEMBER_TEXT]
        payload = out[at + 18:at + size - 8]
        d = zlib.decompressobj(-15)
        got = d.decompress(payload)
        assert d.eof and not d.unused_data and not d.unconsumed_tail, "member %d: the deflate stream does not end with the payload" % i
        assert got == part, "member %d inflates to other bytes than its slice of the text" % i
        crc, isize = struct.unpack_from("<II", out, at + size - 8)
        assert crc == zlib.crc32(part), "member %d: CRC32 %08x, the slice's is %08x" % (i, crc, zlib.crc32(part))
        assert isize == len(part) and (isize == MEMBER_TEXT or i == n - 1), "member %d: ISIZE %d" % (i, isize)
        # the kernel keeps the stored form when the dynamic one is not smaller: stored costs 5 + 28 bytes; 2 bytes of slack
        assert size <= len(part) + STORED + 2, "member %d: %d bytes for %d of text" % (i, size, len(part))
        payloads.append(size - FRAME)
    assert gzip.decompress(out) == text
    return payloads


def python_bgzf(text, level=6):
    """a stream of the same layout written by zlib: raw deflate of each slice closed by Z_SYNC_FLUSH's empty stored block"""
    out = []
    for a in range(0, len(text), MEMBER_TEXT):
        part = text[a:a + MEMBER_TEXT]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = c.compress(part) + c.flush(zlib.Z_SYNC_FLUSH)
        if len(payload) >= len(part) + 5:
            payload = b"\0" + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
        out.append(HEAD + struct.pack("<H", len(payload) + FRAME - 1) + payload + b"\x03\x00" + struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out) + EOF
