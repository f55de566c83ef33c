"""BGZF input for the tests of `leon -c -input-inflate`, built in pure Python: members written by zlib in every way it
has, members built token by token, damaged members, and a walk of the members that knows nothing of the code under test.  The oracle
for a member's text is zlib / gzip."""
import random
import struct
import zlib

import numpy as np

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZES = (0, 1, 15, 16, 17, 1023, 1024, 1025, 32767, 32768, 32769, 65280, 65536)   # where the flush, the ring's wrap or the gather can go wrong
WHOLE, PARTIAL, TRUNCATED, FOREIGN = 0, 1, 2, 3


# ---- text --------------------------------------------------------------------------------------------------------------------------

def fastq_text(n_bytes, seed, line_end=b"\n"):
    """n_bytes of FASTQ-like text (compressible: a BGZF member of 65 536 such bytes fits its 64 KiB)"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes + 400:
        L = int(rng.integers(30, 151))
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes()
        q = np.frombuffer(b"FFFFFF:,#J", dtype=np.uint8)[rng.integers(0, 10, size=L)].tobytes()
        rec = b"@read.%d %d/1" % (i, seed) + line_end + seq + line_end + b"+" + line_end + q + line_end
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


def match_text(seed):
    """text whose deflate holds matches at distance 1, at 2..63, at 64 and more, and far back"""
    rng = random.Random(seed)
    piece = bytes(rng.choice(b"ACGTN") for _ in range(5000))
    short = bytes(rng.choice(b"ACGT") for _ in range(100))
    parts = [b"I" * 700, b"AC" * 300, b"ACGTTGA" * 120, bytes(range(48, 111)) * 40, short * 30, piece, b"#" * 300, piece[:2500], short, piece,
             bytes(rng.choice(b"ACGT") for _ in range(20000)), piece, b"\r\n" * 99]
    return b"".join(parts)


# ---- members -----------------------------------------------------------------------------------------------------------------------

def deflate_raw(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=zlib.Z_FULL_FLUSH, zdict=None):
    if zdict is None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, zdict)
    if flush_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:flush_at]) + c.flush(flush) + c.compress(text[flush_at:]) + c.flush()


def frame(payload, crc, isize, extra=b"", bsize=None, xlen=None, after_bc=b""):
    """a BGZF member around a payload; extra: subfields in front of B C, after_bc: behind it; bsize / xlen: values that lie"""
    sub = extra + b"BC\x02\x00"
    real_xlen = len(sub) + 2 + len(after_bc)
    size = 12 + real_xlen + len(payload) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", real_xlen if xlen is None else xlen) + sub +
            struct.pack("<H", (size - 1 if bsize is None else bsize) & 0xFFFF) + after_bc + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def member(text=b"", payload=None, crc=None, isize=None, extra=b"", after_bc=b"", **how):
    """a member that holds `text`, written by zlib (how: deflate_raw's arguments) or around the payload given"""
    if payload is None:
        payload = deflate_raw(text, **how)
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) == text and d.eof and not d.unused_data
    m = frame(payload, zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize, extra=extra, after_bc=after_bc)
    assert len(m) <= 65536, "a member of %d bytes" % len(m)
    return m


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def bgzf(text, cuts=None, member_text=65280, eof=True, **how):
    """`text` as BGZF: members cut at the offsets `cuts` (default: every member_text bytes)"""
    if cuts is None:
        cuts = list(range(member_text, len(text), member_text))
    edges = [0] + sorted(cuts) + [len(text)]
    out = [member(text[a:b], **how) for a, b in zip(edges, edges[1:]) if b > a or len(text) == 0]
    return b"".join(out) + (EOF if eof else b"")


# ---- streams built token by token (the fixed Huffman code, RFC 1951 3.2.6) ---------------------------------------------------------

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class Bits:
    """deflate's bit order: fields from the least significant bit on, Huffman codes from their most significant bit on"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        for i in range(n - 1, -1, -1):
            self.put(v >> i & 1, 1)

    def symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):
        li = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
        self.symbol(257 + li)
        self.put(length - LEN_BASE[li], LEN_EXTRA[li])
        di = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(di, 5)
        self.put(dist - DIST_BASE[di], DIST_EXTRA[di])

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def fixed_stream(tokens, final=True):
    """one fixed-code block: tokens are bytes (literals) or (length, distance)"""
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            b.match(*t)
        else:
            for c in t:
                b.symbol(c)
    b.symbol(256)
    return b.done()


def token_member(tokens):
    """a member of one fixed-code block of the tokens; its text is what zlib makes of the stream"""
    payload = fixed_stream(tokens)
    d = zlib.decompressobj(-15)
    text = d.decompress(payload)
    assert d.eof and not d.unused_data
    return member(text, payload=payload), text


# ---- the walk, in Python -----------------------------------------------------------------------------------------------------------

def header_kind(p):
    """("member", size, pay0) | ("partial",) | ("foreign",) for the bytes p that begin a member"""
    magic = b"\x1f\x8b\x08\x04"
    if p[:4] != magic[:len(p[:4])]:
        return ("foreign",)
    if len(p) < 12:
        return ("partial",)
    xlen = p[10] | p[11] << 8
    head = 12 + xlen
    if head + 8 > 65536:
        return ("foreign",)
    if len(p) < head:
        return ("partial",)
    at, bsize = 12, None
    while at + 4 <= head:
        slen = p[at + 2] | p[at + 3] << 8
        if at + 4 + slen > head:
            return ("foreign",)
        if p[at:at + 2] == b"BC" and slen == 2:
            bsize = p[at + 4] | p[at + 5] << 8
            break
        at += 4 + slen
    if bsize is None or bsize + 1 < head + 8:
        return ("foreign",)
    if bsize + 1 > len(p):
        return ("partial",)
    return ("member", bsize + 1, head)


def walk(data, last):
    """what leon_host_bgzf_members has to report for data"""
    data = bytes(data)
    at, off, text, stop = 0, [], 0, WHOLE
    while at < len(data):
        k = header_kind(data[at:at + 65536])
        if k[0] == "partial":
            stop = TRUNCATED if last else PARTIAL
            break
        if k[0] == "foreign":
            stop = FOREIGN
            break
        isize = struct.unpack_from("<I", data, at + k[1] - 4)[0]
        if isize <= 65536:
            text += isize
        off.append(at)
        at += k[1]
    return {"member_off": off + [at], "n_members": len(off), "n_text": text, "consumed": at, "stop": stop}


def offsets_of(data):
    w = walk(data, True)
    assert w["stop"] == WHOLE, w
    return np.array(w["member_off"], dtype=np.uint64)
