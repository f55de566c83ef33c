"""The calls the BAM formatters are checked on (test_bam_records_cpu.py: leon_host_records_bam; test_gpu_bam_records.py:
leon_records_bam_device), each against tests/bam_records.py.  A case: (what, reads, heads | None, quals | None, fastq, first)."""
import random

import numpy as np

ALPHABET = b"ACGTN"


def _np(rng):
    return np.random.default_rng(rng.randrange(1 << 30))


def split(blob, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(blob[at:at + n])
        at += n
    return out


def reads_of(rng, lengths, alphabet=ALPHABET):
    return split(np.frombuffer(alphabet, dtype=np.uint8)[_np(rng).integers(0, len(alphabet), size=sum(lengths))].tobytes(), lengths)


def quals_for(reads, rng, lo=33, hi=126):
    lengths = [len(s) for s in reads]
    return split(_np(rng).integers(lo, hi + 1, size=sum(lengths)).astype(np.uint8).tobytes(), lengths)


def head_of(rng, n):
    """a header of n bytes, a name and (from 12 bytes on) a comment behind a space"""
    body = bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789.:_/") for _ in range(n))
    if n < 12:
        return body
    cut = rng.randrange(4, n - 4)
    return body[:cut] + b" " + body[cut + 1:]


EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 149, 150]        # the odd last nybble, the 16-byte lane edges

HEAD_KINDS = [
    b"plainname",                                                  # no separator
    b"name a comment",                                             # a space (the comment keeps its own)
    b"name\ta comment",                                            # a tab
    b"name two\tkinds",                                            # both: the first one wins
    b"name\ttwo kinds",
    b" comment alone",                                             # a separator as first byte: name "*"
    b"\tcomment alone",
    b"nocomment ",                                                 # a separator as last byte: no aux field
    b"nocomment\t",
    b" ",                                                          # "*" and nothing else
    b"",                                                           # an empty header
    b"N",                                                          # name lengths 1, 253, 254
    b"x" * 253,
    b"y" * 254,
    b"z" * 253 + b" with a comment",
    b"w" * 254 + b"\twith a comment",
    b"name  two spaces",                                           # the comment begins with the second
]


def cases():
    rng = random.Random(4190)
    out = []
    # every edge length with every header kind beside it
    lengths = EDGE_LENGTHS + [7] * (len(HEAD_KINDS) - len(EDGE_LENGTHS))
    reads = reads_of(rng, lengths)
    quals = quals_for(reads, rng)
    quals[9] = bytes([33, 126]) * 74 + b"!"                        # bytes 33 and 126
    out.append(("edge lengths, header kinds", reads, list(HEAD_KINDS), quals, True, 0))
    out.append(("edge lengths, reversed", reads[::-1], list(HEAD_KINDS), quals[::-1], True, 7))
    # a record that spans three tiles
    reads = reads_of(rng, [5, 10000, 0, 33])
    out.append(("one read of 10 000 bases", reads, [head_of(rng, 30) for _ in reads], quals_for(reads, rng), True, 0))
    # records starting at every offset modulo 16, several hundred tile edges
    n = 3000
    reads = reads_of(rng, [150] * n)
    out.append(("3 000 reads of 150", reads, [head_of(rng, rng.randrange(20, 61)) for _ in range(n)], quals_for(reads, rng), True, 1000))
    # the smallest record, 38 bytes
    out.append(("5 000 empty reads, empty headers", [b""] * 5000, [b""] * 5000, [b""] * 5000, True, 0))
    # no header stream: the index's digits change inside the call
    reads = reads_of(rng, [rng.choice((0, 1, 36, 101)) for _ in range(12)])
    quals = quals_for(reads, rng)
    out.append(("read index across 9 -> 10", reads, None, quals, True, 4))
    out.append(("read index across 99 999 -> 100 000", reads, None, quals, True, 99994))
    out.append(("read index, FASTA", reads, None, None, False, 0))
    # every byte value once: the table, the case folding, everything else N
    every = bytes(range(256))
    reads = [every, every[:255], every[::-1], b".-*=", b"=acmgrsvtwyhkdbn", b"=ACMGRSVTWYHKDBN"]
    out.append(("every byte value", reads, [b"r%d" % i for i in range(len(reads))], quals_for(reads, rng), True, 0))
    # -letters style: lower-case runs and IUPAC codes among the bases
    reads = reads_of(rng, [150, 149, 75, 1], alphabet=b"ACGTNacgtnRYKMSWBDHVrykmswbdhv")
    out.append(("lower case and IUPAC", reads, [head_of(rng, 25) for _ in reads], quals_for(reads, rng), True, 0))
    # no qualities: a FASTA container, and a call without d_quals
    reads = reads_of(rng, [0, 1, 17, 150, 33])
    heads = [head_of(rng, 20 + i) for i in range(len(reads))]
    out.append(("FASTA", reads, heads, None, False, 0))
    out.append(("fastq without qualities", reads, heads, None, True, 0))
    out.append(("no read", [], [], [], True, 0))
    out.append(("no read, no header stream", [], None, None, False, 3))
    return out


def name_refusals():
    """(what, reads, heads, quals, first, the read the message names, the name's bytes)"""
    rng = random.Random(255)
    reads = reads_of(rng, [20] * 12)
    quals = quals_for(reads, rng)
    heads = [head_of(rng, 30) for _ in reads]
    one, two = list(heads), list(heads)
    one[5] = b"n" * 255
    two[9] = b"m" * 300 + b" comment"
    two[3] = b"k" * 255 + b"\tcomment"
    two[11] = b"j" * 1000
    return [("a name of 255 bytes", reads, one, quals, 100, 105, 255), ("three offenders", reads, two, quals, 40, 43, 255)]


def quality_refusals():
    """(what, reads, heads, quals, first, the read the message names): a single byte 32 at the first, a middle and the last base of a call"""
    rng = random.Random(32)
    lengths = [150] * 40 + [0, 1]
    reads = reads_of(rng, lengths)
    heads = [head_of(rng, 30) for _ in reads]
    out = []
    for what, r, i in (("first base", 0, 0), ("a middle base", 20, 77), ("last base", 41, 0)):
        quals = quals_for(reads, rng)
        quals[r] = quals[r][:i] + b" " + quals[r][i + 1:]
        out.append((what, reads, heads, quals, 10, 10 + r))
    return out
