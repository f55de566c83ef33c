"""The header stream at the level of its symbols, in pure Python: a WRITER that codes any list of
(model, symbol) pairs -- so a test can state streams the grammar admits and no encoder of ours emits, or streams it does not
admit at all -- and a READER that is the reference for every decoding route: a range decoder that is the inverse of
py_leon.RangeEncoder, and a record interpreter written from section 1.3's "what a decoder accepts", not from host_streams.cpp.
tests/py_header.py's encode_block goes through the same writer."""
import re
from bisect import bisect_right

from py_leon import M64, Model, RangeEncoder

END, END_MATCH, ASCII, NUMERIC, DELTA, DELTA_2, ZERO_ONLY, ZERO_AND_NUMERIC = 1, 2, 3, 4, 5, 6, 7, 8
MODELS = ("type", "idx", "col", "size", "ascii", "zero") + tuple("num%d" % i for i in range(9))
MAX_HEADER = 1 << 31          # the host decoder's limit on one header (an implementation's limit, not the format's)
BEYOND_MAX = 16               # bytes a decoder may take beyond the payload's end; the step that takes one more is refused


def _models():
    return {m: Model(9 if m == "type" else 256) for m in MODELS}


# ---- writer ----------------------------------------------------------------------------------------------------------------
def write(pairs):
    """[(model name, symbol)] -> payload bytes"""
    rc, M = RangeEncoder(), _models()
    for m, s in pairs:
        rc.encode(M[m], s)
    rc.flush()
    return bytes(rc.out)


def numeric_syms(v, bc=None):
    """encodeNumeric: the byte count on num0 (bc: what to write there, any of 0..255; min(bc, 8) bytes follow), then the bytes, low first"""
    if bc is None:
        bc = 1
        while bc < 8 and (v >> (8 * bc)):
            bc += 1
    return [("num0", bc)] + [("num%d" % (i + 1), (v >> (8 * i)) & 255) for i in range(min(bc, 8))]


def count(model, x, escape=False, bc=None):
    """a count on a 256-symbol model: itself below 255, else (or with escape=True) 255 and numeric(x - 255 modulo 2^64)"""
    if isinstance(x, list):                                       # already symbols
        return x
    if x < 255 and not escape:
        return [(model, x)]
    return [(model, 255)] + numeric_syms((x - 255) & M64, bc)


def _sep(s):
    if isinstance(s, (bytes, bytearray)):
        s = s[0] if s else 0
    return [("ascii", s)]


def ascii(idx, col, data, size=None):
    """size: the count to write when it is not len(data)"""
    return [("type", ASCII)] + count("idx", idx) + count("col", col) + count("size", len(data) if size is None else size) + [("ascii", b) for b in data]


def numeric(idx, v, sep, bc=None):
    return [("type", NUMERIC)] + count("idx", idx) + numeric_syms(v, bc) + _sep(sep)


def delta(idx, dv, bc=None):
    return [("type", DELTA)] + count("idx", idx) + numeric_syms(dv, bc)


def delta2(idx, dv, bc=None):
    return [("type", DELTA_2)] + count("idx", idx) + numeric_syms(dv, bc)


def zero_only(idx, z, sep):
    return [("type", ZERO_ONLY)] + count("idx", idx) + count("zero", z) + _sep(sep)


def zero_numeric(idx, z, v, sep, bc=None):
    return [("type", ZERO_AND_NUMERIC)] + count("idx", idx) + count("zero", z) + numeric_syms(v, bc) + _sep(sep)


def end(f):
    return [("type", END)] + count("idx", f)


def end_match():
    return [("type", END_MATCH)]


def block(*records):
    """records (lists of pairs) -> one list of pairs"""
    return [p for r in records for p in r]


# ---- reader ----------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    """kind: 'end' (the end-of-payload rule), 'record' (not a record sequence), 'size' (an implementation's size limit)"""

    def __init__(self, kind, reason):
        Exception.__init__(self, "%s: %s" % (kind, reason))
        self.kind, self.reason = kind, reason


class RangeDecoder:
    """the inverse of py_leon.RangeEncoder; bytes beyond the payload's end read as 0, the renormalisation step that takes the
    17th of them refuses the stream (the initial eight bytes count as taken)"""

    def __init__(self, payload):
        self.p, self.i = payload, 0
        self.low, self.range, self.code = 0, M64, 0
        self.n_symbols = 0
        for _ in range(8):
            self.code = (self.code << 8) | self._byte()

    def _byte(self):
        b = self.p[self.i] if self.i < len(self.p) else 0
        self.i += 1
        return b

    @property
    def beyond(self):
        return max(0, self.i - len(self.p))

    def decode(self, m):
        self.range //= m.r[m.n]
        if self.range == 0:
            raise Refused("end", "the range is exhausted")
        v = ((self.code - self.low) & M64) // self.range
        c = bisect_right(m.r, v, 0, m.n) - 1                     # the last symbol whose cumulative count is <= v
        self.low = (self.low + m.r[c] * self.range) & M64
        self.range = (self.range * (m.r[c + 1] - m.r[c])) & M64
        while True:
            if (self.low ^ ((self.low + self.range) & M64)) < RangeEncoder.TOP:
                pass
            elif self.range < RangeEncoder.BOTTOM:
                self.range = (-self.low) & (RangeEncoder.BOTTOM - 1)
            else:
                break
            self.code = ((self.code << 8) | self._byte()) & M64
            self.range = (self.range << 8) & M64
            self.low = (self.low << 8) & M64
            if self.beyond > BEYOND_MAX:
                raise Refused("end", "byte %d beyond the payload's end" % self.beyond)
        m.update(c)
        self.n_symbols += 1
        return c


_FIELD = re.compile(rb"[0-9A-Za-z]*(?:[^0-9A-Za-z]|$)", re.S)
_NUMERIC = re.compile(rb"(0|[1-9][0-9]{0,17})([^0-9A-Za-z\x00]?)", re.S)


def split(h):
    """a header's fields: an alphanumeric run and the one separator byte after it"""
    out, pos = [], 0
    while pos < len(h):
        m = _FIELD.match(h, pos)
        out.append(m.group(0))
        pos = m.end()
    return out


def interpret(sym, n_reads, first, max_header=MAX_HEADER):
    """sym(model name) -> the next symbol.  The headers of one block."""
    def numeric_():
        bc = min(sym("num0"), 8)
        return sum(sym("num%d" % (i + 1)) << (8 * i) for i in range(bc))

    def count_(m):
        x = sym(m)
        return x if x < 255 else (255 + numeric_()) & M64

    def sep_():
        s = sym("ascii")
        return bytes([s]) if s else b""

    out, prev = [], first
    for r in range(n_reads):
        pf, cur, size = split(prev), [], 0                        # cur: the fields placed, one entry each

        def place(piece):
            nonlocal size
            size += len(piece)
            if size > max_header:
                raise Refused("size", "header %d is longer than %d bytes" % (r, max_header))
            cur.append(piece)

        def copy_to(limit):
            while len(cur) < limit and len(cur) < len(pf):
                place(pf[len(cur)])

        while True:
            t = sym("type")
            if t == END_MATCH:
                copy_to(len(pf))
                break
            if t == 0:
                raise Refused("record", "type 0")
            idx = count_("idx")
            if idx < len(cur):
                raise Refused("record", "index %d, %d fields placed" % (idx, len(cur)))
            copy_to(idx)
            if len(cur) != idx:
                raise Refused("record", "index %d, the previous header has %d fields" % (idx, len(pf)))
            if t == END:
                break
            p = pf[idx] if idx < len(pf) else None
            if t == ASCII:
                col, sz = count_("col"), count_("size")
                if col > (len(p) if p is not None else 0):
                    raise Refused("record", "column %d beyond the previous field" % col)
                if sz > max_header or size + col + sz > max_header:
                    raise Refused("size", "ASCII record of %d bytes" % sz)
                place((p[:col] if col else b"") + bytes(sym("ascii") for _ in range(sz)))
            elif t in (DELTA, DELTA_2):
                dv = numeric_()
                m = _NUMERIC.fullmatch(p) if p is not None else None
                if not m:
                    raise Refused("record", "a delta on %r" % (p,))
                v = int(m.group(1))
                place(b"%d" % ((v + dv if t == DELTA else v - dv) & M64) + m.group(2))
            else:
                z = count_("zero") if t != NUMERIC else 0
                if z > max_header:
                    raise Refused("size", "%d zeros" % z)
                v = numeric_() if t != ZERO_ONLY else None
                place(b"0" * z + (b"%d" % v if v is not None else b"") + sep_())
        out.append(b"".join(cur))
        prev = out[-1]
    return out


def read_full(payload, n_reads, first, max_header=MAX_HEADER):
    """-> (headers, bytes taken beyond the end, symbols), or the Refused"""
    d, M = RangeDecoder(payload), _models()
    try:
        hs = interpret(lambda m: d.decode(M[m]), n_reads, first, max_header)
    except Refused as e:
        e.n_symbols = d.n_symbols                                 # (the symbols decoded before the one that was refused)
        return e
    return hs, d.beyond, d.n_symbols


def read(payload, n_reads, first, max_header=MAX_HEADER):
    """-> (headers, bytes taken beyond the payload's end), or Refused(reason)"""
    r = read_full(payload, n_reads, first, max_header)
    return r if isinstance(r, Refused) else r[:2]
