"""Unaligned BAM, restated in Python from the format's description with struct -- not from the kernel.  The yardstick of
leon_records_bam_device, leon_host_records_bam, leon_bam_header and `leon -d -bam`; parity with htslib's reader is unpinned.

The uncompressed content of a file: "BAM\\1", l_text (int32), the text "@HD\\tVN:1.6\\tSO:unsorted\\n", n_ref = 0 (int32); then one record
per read, little-endian:
    block_size int32 (the bytes that follow)
    refID -1, pos -1, l_read_name uint8 (counting the NUL), mapq 0, bin uint16 4680, n_cigar_op uint16 0, flag uint16 4, l_seq uint32,
    next_refID -1, next_pos -1, tlen 0                                                                        -- 32 bytes
    the name and a NUL; (l_seq + 1) / 2 bytes of bases, two a byte, the first in the high nybble; l_seq quality bytes;
    'C' 'O' 'Z' the comment and a NUL when there is a comment
"""
import struct

HEADER_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
BASE_TABLE = b"=ACMGRSVTWYHKDBN"
MAX_NAME = 254
CORE = struct.Struct("<iiBBHHHIiii")                             # refID .. tlen
assert CORE.size == 32


class BamRefusal(Exception):
    """what the formatters refuse: .read is the read's index (counted from `first`), .text the words behind 'read N: '"""

    def __init__(self, read, text):
        Exception.__init__(self, "read %d: %s" % (read, text))
        self.read, self.text = read, text


def bam_header():
    return b"BAM\1" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT + struct.pack("<i", 0)


def name_and_comment(head):
    """the header line without its lead byte -> (name, comment or None)"""
    cut = min((i for i in (head.find(b" "), head.find(b"\t")) if i >= 0), default=-1)
    name, comment = (head, None) if cut < 0 else (head[:cut], head[cut + 1:])
    return name, comment if comment else None


def base_code(c):
    i = BASE_TABLE.find(bytes([c]).upper())
    return i if i >= 0 else 15


_CODE = bytes(base_code(c) for c in range(256))                  # bytes.translate tables: a 100 000-read file is restated in a second or two
_MINUS_33 = bytes((c - 33) & 0xFF for c in range(256))
_PLUS_33 = bytes((c + 33) & 0xFF for c in range(256))
_HEX_TO_BASE = str.maketrans("0123456789abcdef", BASE_TABLE.decode())


def bam_record(seq, head, qual, index):
    """one record; head None: the decimal read index is the name; qual None: 0xFF for every base"""
    name, comment = name_and_comment(head) if head is not None else (b"%d" % index, None)
    if len(name) > MAX_NAME:
        raise BamRefusal(index, "its name has %d bytes, BAM allows %d" % (len(name), MAX_NAME))
    name = name or b"*"
    codes = seq.translate(_CODE) + b"\0"                          # (a last odd low nybble is 0)
    packed = bytes(hi << 4 | lo for hi, lo in zip(codes[0:len(seq):2], codes[1::2]))
    if qual is None:
        q = b"\xff" * len(seq)
    else:
        assert len(qual) == len(seq)
        if qual and min(qual) < 33:
            raise BamRefusal(index, "a quality byte below 33")
        q = qual.translate(_MINUS_33)
    body = CORE.pack(-1, -1, len(name) + 1, 0, 4680, 0, 4, len(seq), -1, -1, 0) + name + b"\0" + packed + q
    if comment is not None:
        body += b"COZ" + comment + b"\0"
    return struct.pack("<i", len(body)) + body


def bam_records(reads, heads, quals, first=0):
    """(bytes, rec_off) of the reads' records; heads None: no header stream; quals None: no qualities.  A refusal names the smallest such
    read, and a name's comes before a quality's, as the formatters check them"""
    out, rec_off, at, refused = [], [0], 0, {}
    for r, seq in enumerate(reads):
        try:
            rec = bam_record(seq, heads[r] if heads is not None else None, quals[r] if quals is not None else None, first + r)
        except BamRefusal as e:
            refused.setdefault(e.text.startswith("its name"), e)
            if e.text.startswith("its name"):
                continue
            rec = bam_record(seq, heads[r] if heads is not None else None, None, first + r)      # (its name is still to be looked at)
        out.append(rec)
        at += len(rec)
        rec_off.append(at)
    for kind in (True, False):
        if kind in refused:
            raise refused[kind]
    return b"".join(out), rec_off


def parse_bam(data):
    """the uncompressed content of a file -> [(name, seq, qual or None, comment or None)]; seq in upper case, qual as FASTQ bytes (None
    when every byte is 0xFF).  Every field that -bam fixes is asserted."""
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", data, 4)
    assert data[8:8 + l_text] == HEADER_TEXT
    assert struct.unpack_from("<i", data, 8 + l_text) == (0,)
    at, out = 12 + l_text, []
    while at < len(data):
        (block_size,) = struct.unpack_from("<i", data, at)
        rec = data[at + 4:at + 4 + block_size]
        assert len(rec) == block_size >= 32
        ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = CORE.unpack_from(rec, 0)
        assert (ref, pos, mapq, bin_, n_cigar, flag, nref, npos, tlen) == (-1, -1, 0, 4680, 0, 4, -1, -1, 0)
        p = 32
        name = rec[p:p + l_name]
        assert l_name >= 2 and name[-1:] == b"\0" and b"\0" not in name[:-1]
        p += l_name
        packed = rec[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        assert len(packed) == (l_seq + 1) // 2
        seq = packed.hex()[:l_seq].translate(_HEX_TO_BASE).encode()             # (a hex digit is a nybble, the high one first)
        if l_seq & 1:
            assert packed[-1] & 15 == 0
        q = rec[p:p + l_seq]
        assert len(q) == l_seq
        p += l_seq
        qual = None if q == b"\xff" * l_seq and l_seq else q.translate(_PLUS_33)
        comment = None
        if p < len(rec):
            assert rec[p:p + 3] == b"COZ" and rec[-1:] == b"\0" and len(rec) - p > 4
            comment = rec[p + 3:-1]
        out.append((name[:-1], seq, qual, comment))
        at += 4 + block_size
    assert at == len(data)
    return out


def fold(seq):
    """what BAM keeps of a sequence: the table's letters in upper case, N for everything else"""
    return seq.translate(bytes(BASE_TABLE[c] for c in _CODE))
