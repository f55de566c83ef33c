"""What a record-aligned BGZF stream of leon_text_bgzf_records_device has to be, in pure Python and never against the code
under test: the cut rule restated in a dozen lines, the members walked by tests/bgzf_check.py, every payload inflated on its own with zlib
and set against its slice of the text, and a reader for the .gzi index."""
import bisect
import gzip
import struct
import zlib

import bgzf_check as B

W = B.MEMBER_TEXT


def cuts(rec_off, W=W, last=True):
    """[(begin, len)] of the members of a text whose records start at rec_off (first 0, last the text's size); without `last` members are
    cut from p only while more than W bytes lie behind p"""
    rec_off = [int(x) for x in rec_off]
    out, i = [], 0
    while i + 1 < len(rec_off) and (last or rec_off[-1] - rec_off[i] > W):
        p, nxt = rec_off[i], rec_off[i + 1]
        if nxt - p > W:                                           # oversized: members of its own
            out += [(a, min(W, nxt - a)) for a in range(p, nxt, W)]
            i += 1
            continue
        j = i + 1
        while j + 1 < len(rec_off) and rec_off[j + 1] <= p + W:   # the largest start <= p + W
            j += 1
        out.append((p, rec_off[j] - p))
        i = j
    return out


def bound(n_text, W=W):
    return 3 * (n_text // W) + 2


def cuts_call(rec_off, n_head, last, W=W):
    """one call of the rule: the members of n_head bytes of head (one record as far as the rule goes) and the body's records, and the
    bytes taken"""
    out = cuts(([0] if n_head else []) + [n_head + int(x) for x in rec_off], W, last)
    return out, (out[-1][0] + out[-1][1] if out else 0)


def offsets(lengths):
    """record lengths -> their start offsets, the text's size last"""
    out = [0]
    for n in lengths:
        out.append(out[-1] + int(n))
    return out


# record lengths, the smallest at which each branch of the rule and of its walkers can go wrong
SHAPES = {
    "no_text": [],
    "one_byte": [1],
    "one_member_of_exactly_W": [256] * 128,
    "one_byte_more_than_W": [256] * 127 + [257],
    "a_pair_that_fits_exactly_and_one_that_does_not": [16384, 16384, 16385, 16384],
    "a_record_of_exactly_W": [5, 32768, 5],
    "a_record_of_W_plus_1": [5, 32769, 5],
    "100000_between_small_records": [50] * 10 + [100000] + [50] * 10,
    "oversized_first_and_last": [70000, 10, 20, 65536],
    "two_oversized_in_a_row": [7, 40000, 32769, 7],
    "records_of_3_bytes": [3] * 200000,
    "records_of_1_byte": [1] * 70000,
}


def member_texts(out, eof=True):
    """[(start, size, text)] of the data members: each payload inflated on its own, its CRC-32, ISIZE and size checked"""
    out = bytes(out)
    members = B.walk(out)
    if eof:
        assert out[-28:] == B.EOF, "the stream does not end with the EOF marker: " + out[-28:].hex()
        assert members and members[-1] == (len(out) - 28, 28)
        members = members[:-1]
    found = []
    for i, (at, size) in enumerate(members):
        d = zlib.decompressobj(-15)
        got = d.decompress(out[at + 18:at + size - 8])
        assert d.eof and not d.unused_data and not d.unconsumed_tail, "member %d: the deflate stream does not end with the payload" % i
        crc, isize = struct.unpack_from("<II", out, at + size - 8)
        assert crc == zlib.crc32(got), "member %d: CRC32 %08x, its text's is %08x" % (i, crc, zlib.crc32(got))
        assert isize == len(got) and 1 <= isize <= W, "member %d: ISIZE %d for %d bytes" % (i, isize, len(got))
        assert size <= len(got) + B.STORED + 2, "member %d: %d bytes for %d of text" % (i, size, len(got))
        found.append((at, size, got))
    return found


def check_records(out, text, rec_off, eof=True, want=None):
    """`out` is the record-aligned BGZF of `text`, whose records start at rec_off: the members are those of cuts() (or `want`, for a call
    that is not the whole text).  Returns [(member start, text offset, ISIZE)]."""
    out, text = bytes(out), bytes(text)
    rec_off = [int(x) for x in rec_off]
    want = cuts(rec_off) if want is None else want
    found = member_texts(out, eof)
    assert len(found) == len(want), "%d data members, the rule gives %d" % (len(found), len(want))
    assert len(found) <= bound(len(text))
    starts, table, at_text = set(rec_off), [], 0
    for i, ((at, size, got), (a, m)) in enumerate(zip(found, want)):
        assert a == at_text and len(got) == m, "member %d holds text [%d, %d), the rule says [%d, %d)" % (i, at_text, at_text + len(got), a, a + m)
        assert got == text[a:a + m], "member %d inflates to other bytes than its slice of the text" % i
        if a not in starts:                                       # inside an oversized record, at a multiple of W from its start
            r = rec_off[bisect.bisect_right(rec_off, a) - 1]
            assert rec_off[bisect.bisect_right(rec_off, a)] - r > W and (a - r) % W == 0, "member %d begins at %d, inside the record at %d" % (i, a, r)
        table.append((at, a, m))
        at_text += m
    if eof:
        assert at_text == len(text)
        assert gzip.decompress(out) == text
    else:
        assert (gzip.decompress(out) if out else b"") == text[:at_text]
    return table


def gzi_bytes(table):
    """the .gzi of a file whose data members are `table` [(member start, text offset, ...)]: htslib's layout as recalled -- a little-endian
    uint64 count, then (compressed offset, uncompressed offset) per data member except the first"""
    rest = table[1:]
    return struct.pack("<Q", len(rest)) + b"".join(struct.pack("<QQ", t[0], t[1]) for t in rest)


def read_gzi(data):
    """[(compressed offset, uncompressed offset)] of a .gzi file, the implicit (0, 0) not included"""
    data = bytes(data)
    assert len(data) >= 8, "a .gzi of %d bytes" % len(data)
    n = struct.unpack_from("<Q", data)[0]
    assert len(data) == 8 + 16 * n, "a .gzi of %d bytes for %d entries" % (len(data), n)
    return [struct.unpack_from("<QQ", data, 8 + 16 * i) for i in range(n)]


def check_gzi(gzi, out, text):
    """every entry of the index (and the implicit first) names a member's first byte, and inflating that one member gives the text from
    the entry's offset on; the entries are all the data members but the first, in order"""
    out, text = bytes(out), bytes(text)
    entries = read_gzi(gzi)
    members = [m for m in B.walk(out) if m[1] != 28 or out[m[0]:m[0] + 28] != B.EOF]
    assert [e[0] for e in entries] == [at for at, _ in members[1:]], "the index does not list every data member but the first"
    for at, text_off in [(0, 0)] + entries:
        if not members:
            break
        size = struct.unpack_from("<H", out, at + 16)[0] + 1
        isize = struct.unpack_from("<I", out, at + size - 4)[0]
        got = zlib.decompressobj(-15).decompress(out[at + 18:at + size - 8])
        assert got == text[text_off:text_off + isize] and len(got) == isize, "the member at %d does not hold the text at %d" % (at, text_off)
    return entries
