"""Directed header streams ("what a decoder accepts") for tests/test_header_streams_cpu.py and
tests/test_gpu_header_streams.py: streams the grammar admits and the encoder never writes, streams the device declines and the
host decodes, and one stream per refusal.  Every case states its headers, or that it is refused, literally; the tests first hold
the reader of tests/header_streams.py to that literal and then every decoding route to the reader."""
import functools
import random

import hdr_samples
import header_streams as S
import py_header

CAP = 4096                                    # capi.HEADER_TEXT_DEVICE_CAP (the tests check that it still is)
F = b"r1 x:12:007 ab"                         # fields: "r1 ", "x:", "12:", "007 ", "ab"
COLONS = b":" * 301                           # 301 fields of one separator each
LONGF = b"a" * 300 + b" q"
EM = S.end_match()
ALNUM = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def an(n):
    """n alphanumeric bytes that do not repeat at once (a run of one byte costs so little payload that a long header of it
    overruns the block's share of the symbol buffer before it reaches the cap)"""
    return (ALNUM * (n // len(ALNUM) + 1))[:n]


class Block:
    """one block: its symbols, its reads, and either its headers (want) or that it is refused"""

    def __init__(self, name, records, want=None, n_reads=None, declined=False, refused=None, host_only=False, payload=None):
        self.name, self.pairs, self.want, self.declined, self.refused, self.host_only = name, S.block(*records), want, declined, refused, host_only
        self.n_reads = n_reads if n_reads is not None else len(want)
        self._payload = payload

    @property
    def payload(self):
        if self._payload is None:
            self._payload = S.write(self.pairs)
        return self._payload

    def as_block(self, i=0):
        return (i, self.payload, self.n_reads)


def share(block):
    """the symbols k_hdr_decode_symbols may write for a block (hdr_kernels.hip, hdr_symbols_launch)"""
    return 24 * block.n_reads + 6 * len(block.payload) + 256


def _valid_F():
    V = []
    add = lambda name, records, want: V.append(Block(name, records, want))        # noqa: E731
    h = lambda mid: b"r1 x:" + mid + b":007 ab"                                     # noqa: E731  (field 2 replaced)
    # the byte count of a numeric: min(symbol, 8); 0 gives the value 0
    add("bc0", [S.numeric(2, 0, b":", bc=0), EM], [b"r1 x:0:007 ab"])
    add("bc8", [S.numeric(2, 2 ** 64 - 1, b":", bc=8), EM], [b"r1 x:18446744073709551615:007 ab"])
    add("bc9", [S.numeric(2, 5, b":", bc=9), EM], [b"r1 x:5:007 ab"])
    add("bc255", [S.numeric(2, 0x0807060504030201, b":", bc=255), EM], [b"r1 x:578437695752307201:007 ab"])
    add("nonminimal_5", [r for bc in range(1, 9) for r in (S.numeric(2, 5, b":", bc=bc), EM)], [b"r1 x:5:007 ab"] * 8)
    # count escapes: 255 and 256 on the zero model, and 3 written as 255 + a numeric that wraps
    add("zeros_254", [S.zero_only(3, 254, b" "), EM], [b"r1 x:12:" + b"0" * 254 + b" ab"])
    add("zeros_255", [S.zero_only(3, 255, b" "), EM], [b"r1 x:12:" + b"0" * 255 + b" ab"])
    add("zeros_256", [S.zero_only(3, 256, b" "), EM], [b"r1 x:12:" + b"0" * 256 + b" ab"])
    add("index_3_wrapped", [S.zero_only(S.count("idx", 3, escape=True, bc=8), 2, b" "), EM], [b"r1 x:12:00 ab"])
    add("index_3_wrapped_bc200", [S.numeric(S.count("idx", 3, escape=True, bc=200), 1, b"/"), EM], [b"r1 x:12:1/ab"])
    add("end_wrapped", [S.end(S.count("idx", 2, escape=True, bc=8))], [b"r1 x:"])
    # size at 254, 255, 256 (col: _valid_long)
    for n in (254, 255, 256):
        add("size_%d" % n, [S.ascii(4, 0, b"b" * n), EM], [b"r1 x:12:007 " + b"b" * n])
    # separators that are alphanumeric: the next header's fields are cut differently from the records that wrote this one
    add("numeric_sep_A", [S.numeric(2, 7, b"A"), EM, S.numeric(2, 9, b":"), EM], [b"r1 x:7A007 ab", b"r1 x:9:ab"])
    add("numeric_sep_0", [S.numeric(2, 7, b"0"), EM, S.delta(2, 1), EM], [b"r1 x:70007 ab", b"r1 x:70008 ab"])
    add("numeric_sep_z", [S.numeric(2, 7, b"z"), EM, S.ascii(2, 2, b"Q "), EM], [b"r1 x:7z007 ab", b"r1 x:7zQ ab"])
    add("zero_sep_A", [S.zero_only(3, 2, b"A"), EM, S.end(3)], [b"r1 x:12:00Aab", b"r1 x:12:"])
    add("zero_sep_0", [S.zero_only(3, 2, b"0"), EM, S.ascii(3, 0, b""), EM], [b"r1 x:12:000ab", b"r1 x:12:"])
    add("zero_sep_z", [S.zero_only(3, 2, b"z"), EM, S.ascii(3, 3, b"!"), EM], [b"r1 x:12:00zab", b"r1 x:12:00z!"])
    # (the field behind a previous header that does not end in a separator, and behind one that does)
    add("zeronum_sep_A", [S.zero_numeric(3, 1, 5, b"A"), EM, S.numeric(4, 3, 0), EM], [b"r1 x:12:05Aab", b"r1 x:12:05Aab3"])
    add("zeronum_sep_0", [S.zero_numeric(3, 1, 5, b"0"), EM, S.zero_only(3, 3, b":"), EM, S.numeric(4, 8, 0), EM],
        [b"r1 x:12:050ab", b"r1 x:12:000:", b"r1 x:12:000:8"])
    add("zeronum_sep_z", [S.zero_numeric(3, 1, 5, b"z"), EM, S.delta2(2, 2), EM], [b"r1 x:12:05zab", b"r1 x:10:05zab"])
    # ASCII bytes that hold separators: one record, three fields for the next header
    add("ascii_with_separators", [S.ascii(1, 0, b"ab:cd e"), EM, S.numeric(5, 4, 0), EM, S.ascii(6, 0, b"/x"), EM],
        [b"r1 ab:cd e12:007 ab", b"r1 ab:cd e12:007 4", b"r1 ab:cd e12:007 4/x"])
    add("ascii_size_0", [S.ascii(1, 0, b""), EM], [b"r1 12:007 ab"])
    add("ascii_col_full", [S.ascii(1, 2, b""), EM], [F])
    add("ascii_col_0_equal", [S.ascii(1, 0, b"x:"), EM], [F])
    add("ascii_col_below_prefix", [S.ascii(4, 0, b"ac"), EM], [b"r1 x:12:007 ac"])
    add("zero_only_z0", [S.zero_only(3, 0, b" "), EM], [b"r1 x:12: ab"])
    add("zero_only_z1", [S.zero_only(3, 1, b" "), EM], [b"r1 x:12:0 ab"])
    add("zeronum_z0", [S.zero_numeric(3, 0, 44, b" "), EM], [b"r1 x:12:44 ab"])
    add("numeric_big", [S.numeric(2, 10 ** 18, b":"), EM, S.numeric(2, 10 ** 19, b":"), EM, S.numeric(2, 2 ** 64 - 1, b":"), EM, S.numeric(2, 0, b":"), EM],
        [h(b"1000000000000000000"), h(b"10000000000000000000"), h(b"18446744073709551615"), h(b"0")])
    add("delta_to_19_digits", [S.numeric(2, 999999999999999999, b":"), EM, S.delta(2, 1), EM], [h(b"999999999999999999"), h(b"1000000000000000000")])
    add("delta_wraps", [S.numeric(2, 5, b":"), EM, S.delta(2, 2 ** 64 - 3), EM], [h(b"5"), h(b"2")])
    add("delta2_below_zero", [S.delta2(2, 13), EM], [h(b"18446744073709551615")])
    add("end_f_nothing_to_copy", [S.ascii(4, 1, b"c"), S.end(5)], [b"r1 x:12:007 ac"])
    add("end_f_first_field", [S.ascii(0, 0, b"k "), S.end(1)], [b"k "])
    add("end_0", [S.end(0), EM], [b"", b""])
    add("end_match", [EM, EM], [F, F])
    # the symbol window of k_hdr_text (256 symbols): a filler record of 5 + L symbols, then a record of 14 -- type, index escape, its
    # byte count and bytes, the value's byte count and bytes, separator -- each of which falls on symbol 255 | 256 for some L
    for L in range(236, 253):
        add("window_L%d" % L, [S.ascii(0, 0, b"f" * L + b" "), S.numeric(S.count("idx", 2, escape=True, bc=8), 300, b":"), EM], [b"f" * L + b" x:300:007 ab"])
    # a header of exactly the device's cap
    add("cap_zeros_number_sep", [S.zero_numeric(0, CAP - 3, 17, b":"), S.end(1)], [b"0" * (CAP - 3) + b"17:"])
    add("cap_col_size", [S.ascii(0, 0, an(3000) + b" "), S.end(1), S.ascii(0, 3000, an(CAP - 3000)), S.end(1)],
        [an(3000) + b" ", an(3000) + an(CAP - 3000)])
    add("cap_copied_record", [S.ascii(0, 0, an(4000) + b" "), S.end(1), S.ascii(1, 0, an(CAP - 4001)), EM],
        [an(4000) + b" ", an(4000) + b" " + an(CAP - 4001)])
    return V


def _valid_colons():
    return [Block("index_%d" % i, [S.ascii(i, 0, b"y:"), EM], [b":" * i + b"y:" + b":" * (300 - i)]) for i in (254, 255, 256, 300)]


def _valid_long():
    return [Block("col_%d" % c, [S.ascii(0, c, b"Z "), EM], [b"a" * c + b"Z q"]) for c in (254, 255, 256)]


def _valid_empty():
    return [Block("empty_first", [S.ascii(0, 0, b"hello 1"), EM, S.delta(1, 1), EM, EM], [b"hello 1", b"hello 2", b"hello 2"]),
            Block("empty_first_stays_empty", [EM, S.end(0)], [b"", b""])]


def _over_share():
    """more symbols than the block's share of the symbol buffer.  (Records of size 0 cannot do it: their indices must ascend within
    a header, so each costs its index in payload bits and the share grows with the payload faster than they add symbols.  A byte that
    repeats costs next to nothing: ten reads of 240 equal bytes are 2 460 symbols from under 200 bytes.)"""
    n = 10
    return Block("over_share", [r for _ in range(n) for r in (S.ascii(0, 0, b"a" * 240 + b" "), EM)], [b"a" * 240 + b" x:12:007 ab"] * n, declined=True)


def _declined_F():
    D = [Block("cap1_zeros_number_sep", [S.zero_numeric(0, CAP - 2, 17, b":"), S.end(1)], [b"0" * (CAP - 2) + b"17:"], declined=True),
         Block("plain_a", [S.delta(2, 1), EM, S.delta(2, 1), EM], [b"r1 x:13:007 ab", b"r1 x:14:007 ab"]),
         Block("cap1_col_size", [S.ascii(0, 0, an(3000) + b" "), S.end(1), S.ascii(0, 3000, an(CAP + 1 - 3000)), S.end(1)],
               [an(3000) + b" ", an(3000) + an(CAP + 1 - 3000)], declined=True),
         Block("cap1_copied_record", [S.ascii(0, 0, an(4000) + b" "), S.end(1), S.ascii(1, 0, an(CAP - 4000)), EM],
               [an(4000) + b" ", an(4000) + b" " + an(CAP - 4000)], declined=True),
         Block("zeros_100000", [S.zero_only(0, 100000, b" "), S.end(1)], [b"0" * 100000 + b" "], declined=True),
         _over_share(),
         Block("plain_b", [S.delta2(2, 2), EM], [b"r1 x:10:007 ab"])]
    return D


@functools.lru_cache(maxsize=None)
def valid_groups():
    """[(first header, [Block])]: the blocks of a group go to a route in ONE call (every block starts from the same first header)"""
    return [(F, _valid_F()), (COLONS, _valid_colons()), (LONGF, _valid_long()), (b"", _valid_empty()), (F, _declined_F())]


GOOD = [Block("good_a", [S.delta(2, 1), EM, S.delta(2, 1), EM], [b"r1 x:13:007 ab", b"r1 x:14:007 ab"]),
        Block("good_b", [S.ascii(4, 1, b"c"), EM], [b"r1 x:12:007 ac"])]


def _three_good():
    return [S.delta(2, 1), EM, S.delta(2, 1), EM, S.delta(2, 1), EM]


@functools.lru_cache(maxsize=None)
def refused():
    """[Block], first header F, one per way a decoder refuses (refused = the reader's kind)"""
    R = []
    add = lambda name, records, n_reads=1, kind="record", **kw: R.append(Block(name, records, n_reads=n_reads, refused=kind, **kw))   # noqa: E731
    add("index_below_placed", [S.numeric(2, 1, b":"), S.numeric(2, 2, b":"), EM])                       # idx < nf
    add("index_beyond_fields_plus_1", [S.numeric(6, 1, 0), EM])                                          # nf != idx
    add("end_below_placed", [S.numeric(2, 1, b":"), S.end(2)])                                           # f < nf
    add("end_beyond_fields", [S.end(6)])                                                                 # nf != f
    add("col_beyond_field", [S.ascii(1, 3, b""), EM])                                                    # col > p_len
    add("col_without_field", [S.ascii(5, 1, b""), EM])
    add("delta_without_field", [S.delta(5, 1), EM])
    add("delta_on_007", [S.delta(3, 1), EM])
    add("delta_on_text", [S.delta2(4, 1), EM])
    add("delta_on_19_digits", [S.numeric(2, 999999999999999999, b":"), EM, S.delta(2, 1), EM, S.delta(2, 1), EM], n_reads=3)
    add("delta_on_nul_separator", [S.ascii(2, 0, b"5\x00"), EM, S.delta(2, 1), EM], n_reads=2)
    add("type_0", [S.delta(2, 1), EM, [("type", 0)]], n_reads=2)
    add("type_0_first", [[("type", 0)]])
    add("ascii_size_2_40", [S.ascii(0, 0, b"abcdefghijkl", size=255 + 2 ** 40), EM], kind="size")
    add("zeros_2_31_plus_1", [S.zero_only(0, 2 ** 31 + 1, b" "), S.end(1)], kind="size", host_only=True)
    add("one_record_early", _three_good()[:-1], n_reads=3, kind=None)
    add("one_header_early", _three_good()[:-2], n_reads=3, kind=None)
    whole = S.write(S.block(S.numeric(2, 77, b":"), EM, S.delta(2, 1), EM))
    for n in range(8):
        R.append(Block("payload_%d_bytes" % n, [], n_reads=2, refused=None, payload=whole[:n]))
    return R


# ---- the end of the payload ---------------------------------------------------------------------------------------------------
# A decoder may take 16 bytes beyond the payload's end; that far out its code word is all zeros, and what it decodes then is
# each model's LAST symbol (code - low wraps).  A header can only END on such symbols where they spell a valid end: HEADER_END,
# count 255, byte count 255 (read as 8), eight bytes 255 = END 254 -- against a previous header of at least 254 fields.  So the
# blocks searched are SRA-style headers brought to 301 fields, then that END, then more of the same; they are cut short.
def _eop_block(seed):
    rnd = random.Random(seed)
    hs = [h.replace(b" ", b":" * 150, 1) + b":" * 143 for h in hdr_samples.sra(rnd.randint(1, 3), seed=seed)]
    first = hs[0]
    assert len(S.split(first)) >= 254
    end254 = S.end(S.count("idx", 254, escape=True, bc=255))
    pairs = []
    prev = first
    for h in hs:
        for r in py_header.records(h, prev):
            pairs += {py_header.DELTA: S.delta, py_header.DELTA_2: S.delta2, py_header.NUMERIC: S.numeric, py_header.ASCII: S.ascii,
                      py_header.END: S.end, py_header.END_MATCH: S.end_match}[r[0]](*r[1:])
        prev = h
    return first, len(hs), pairs + end254 * 4


@functools.lru_cache(maxsize=None)
def end_of_payload(seed=20240611, tries=40):
    """{15, 16, 17, "last": (first, payload, n_reads, the reader's answer)}: cuts of the blocks above at which the reader takes
    exactly 15 and 16 bytes beyond the end and gives headers, one it refuses for the 17th and for nothing else (one byte more of
    the payload and it reads), and one ("last") where the 17th byte is taken by the block's very last symbol"""
    found = {}
    rnd = random.Random(seed)
    for _ in range(tries):
        first, n, pairs = _eop_block(rnd.randrange(1 << 30))
        whole = S.write(pairs)
        for cut in range(len(whole) - 8, 0, -1):
            for n_reads in (n + 1, n + 2):
                r = S.read_full(whole[:cut], n_reads, first)
                if isinstance(r, S.Refused):
                    if r.kind == "end" and r.reason.startswith("byte 17 ") and (17 not in found or "last" not in found):
                        more = S.read_full(whole[:cut + 1], n_reads, first)
                        if not isinstance(more, S.Refused):
                            found.setdefault("last" if more[2] == r.n_symbols + 1 else 17, (first, whole[:cut], n_reads, r))
                elif r[1] in (15, 16) and r[1] not in found:
                    found[r[1]] = (first, whole[:cut], n_reads, r[:2])
            if len(found) == 4:
                return found
    return found
