"""RFC 1951 streams built symbol by symbol, and a scanner that says what a stream is made of -- pure Python, no project code.

The writer (Stream) chains stored, fixed and dynamic blocks in one bit stream.  A dynamic block takes its code lengths, the items of its
header's code-length alphabet (so that the case decides where the repeats fall), the code-length code and HCLEN as given; the codes
are the canonical ones of RFC 1951 3.2.2.  Nothing here decides whether a stream is valid: zlib does (inflate()).

The scanner (scan) walks every header and symbol of a valid stream with a decoder of its own and reports, block by block, what the
tests then require of a case: the lengths of the codes declared and used, the symbols and their extra bits, the repeats of the header
and whether one crossed from the literal/length lengths into the distance lengths, the stored LENs, the alignment of every block.
"""
import zlib

from bgzf_input import Bits, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, member

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)                    # RFC 1951, 3.2.7
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---- code lengths ------------------------------------------------------------------------------------------------------------------

def kraft(lengths):
    """the share of the code space the lengths take, in units of 2^-15: 32 768 is a complete set"""
    return sum(1 << (15 - l) for l in lengths if l)


def complete_lengths(n, maxlen):
    """n code lengths of a complete set whose longest code has exactly maxlen bits (n > maxlen), sorted"""
    assert n > maxlen >= 1
    ls = list(range(1, maxlen)) + [maxlen, maxlen]
    while len(ls) < n:
        l = min(ls)
        assert l < maxlen, "no complete set of %d codes of at most %d bits" % (n, maxlen)
        ls.remove(l)
        ls += [l + 1, l + 1]
    assert kraft(ls) == 32768 and max(ls) == maxlen
    return sorted(ls)


def balanced(symbols):
    """{symbol: length}: a complete set over the symbols whose lengths differ by at most one bit"""
    symbols = list(symbols)
    n = len(symbols)
    assert n >= 2
    k = n.bit_length() - 1
    longer = 2 * (n - (1 << k))
    out = {s: (k + 1 if i < longer else k) for i, s in enumerate(symbols)}
    assert kraft(out.values()) == 32768
    return out


def table(d, n):
    if not isinstance(d, dict):
        d = dict(enumerate(d))
    out = [0] * max(n, max(d, default=-1) + 1)
    for s, l in d.items():
        out[s] = l
    return out


def canonical(lengths):
    """[(code, length) or None] by RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append((nxt[l], l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


# ---- the header's items ------------------------------------------------------------------------------------------------------------

def auto_items(lengths):
    """the lengths as items: every length for itself, runs of 3 .. 138 zeros as one item -- no 16, nothing the case did not ask for"""
    items, i = [], 0
    while i < len(lengths):
        if lengths[i] == 0:
            j = i
            while j < len(lengths) and lengths[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 3:
                items.append(("zeros", j - i))
                i = j
                continue
        items.append(("len", lengths[i]))
        i += 1
    return items


def expand(items):
    """the lengths the items stand for (a ("rep", n) with nothing in front of it repeats 0 here; zlib refuses it)"""
    out = []
    for kind, v in items:
        if kind == "len":
            out.append(v)
        elif kind == "rep":
            out += [out[-1] if out else 0] * v
        else:
            out += [0] * v
    return out


def item_symbol(item):
    """(code-length symbol, extra value, extra bits)"""
    kind, v = item
    if kind == "len":
        assert 0 <= v <= 15
        return v, 0, 0
    if kind == "rep":
        assert 3 <= v <= 6
        return 16, v - 3, 2
    assert kind == "zeros" and 3 <= v <= 138
    return (17, v - 3, 3) if v <= 10 else (18, v - 11, 7)


# ---- the writer --------------------------------------------------------------------------------------------------------------------

def length_symbol(length):
    li = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
    return 257 + li, length - LEN_BASE[li]


def distance_symbol(dist):
    di = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return di, dist - DIST_BASE[di]


class Stream:
    """Blocks of every kind in one bit stream.  Tokens: bytes (literals), (length, distance), ("m", length symbol, extra, distance
    symbol, extra) -- the symbols and extra bits as given, which is how 258 becomes 284 + 31 --, ("l", length symbol, extra) for the
    length half alone and ("bits", value, n) for bits as they are."""

    def __init__(self):
        self.b = Bits()

    def bits(self):
        return 8 * len(self.b.out) + self.b.n

    def done(self):
        return self.b.done()

    def _header(self, final, kind):
        self.b.put(1 if final else 0, 1)
        self.b.put(kind, 2)

    def more(self, tokens, eob=True):
        """further tokens of the block written last with eob=False, in its codes"""
        self._tokens(tokens, *self.codes, eob)
        return self

    def _tokens(self, tokens, ll, dd, eob):
        b = self.b
        self.codes = (ll, dd)

        def sym(codes, s):
            assert codes[s] is not None, "symbol %d has no code" % s
            b.code(*codes[s])

        for t in tokens:
            if isinstance(t, (bytes, bytearray)):
                for c in t:
                    sym(ll, c)
                continue
            if t[0] == "bits":
                b.put(t[1], t[2])
                continue
            if t[0] == "m":
                ls, le, ds, de = t[1:]
            elif t[0] == "l":
                ls, le, ds, de = t[1], t[2], None, 0
            else:
                (ls, le), (ds, de) = length_symbol(t[0]), distance_symbol(t[1])
            sym(ll, ls)
            assert 0 <= le < 1 << LEN_EXTRA[ls - 257]
            b.put(le, LEN_EXTRA[ls - 257])
            if ds is not None:
                sym(dd, ds)
                assert 0 <= de < 1 << DIST_EXTRA[ds]
                b.put(de, DIST_EXTRA[ds])
        if eob:
            sym(ll, 256)

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self._header(final, 0)
        if self.b.n:
            self.b.put(0, 8 - self.b.n)
        self.b.put(len(data), 16)
        self.b.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.b.out += data                                        # (byte-aligned here)
        return self

    def fixed(self, tokens, final=False, eob=True):
        self._header(final, 1)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def dynamic(self, ll, dl, tokens=(), final=False, items=None, cl=None, hclen=None, hlit=None, hdist=None, eob=True, check=True):
        """ll, dl: {symbol: length} (or lists) of the two alphabets; hlit / hdist: the NUMBER of lengths declared (default: up to the
        last one in use); items: the header's code-length items for the hlit + hdist lengths (default: auto_items of either array for
        itself); cl: {code-length symbol: length} (default: a balanced set over the symbols the items use); hclen: the number of
        code-length code lengths written (default: the fewest).  check=False writes what it is given, for the streams to be refused."""
        ll, dl = table(ll, 0), table(dl, 0)
        hlit = max(257, len(ll) - next((i for i, l in enumerate(reversed(ll)) if l), len(ll))) if hlit is None else hlit
        hdist = max(1, len(dl) - next((i for i, l in enumerate(reversed(dl)) if l), len(dl))) if hdist is None else hdist
        ll, dl = table(ll, hlit), table(dl, hdist)
        if items is None:
            items = auto_items(ll[:hlit]) + auto_items(dl[:hdist])
        syms = [item_symbol(it) for it in items]
        if cl is None:
            used = sorted({s for s, _, _ in syms})
            if len(used) == 1:
                used.append(next(s for s in (0, 1) if s not in used))      # (a code-length code of one code is incomplete)
            cl = balanced(used)
        cl = table(cl, 19)
        if hclen is None:
            hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
        if check:
            assert expand(items) == ll[:hlit] + dl[:hdist], "the items are not the lengths"
            assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and 4 <= hclen <= 19 and max(cl) <= 7
            assert kraft(cl) == 32768 and not any(cl[CL_ORDER[i]] for i in range(hclen, 19))
        self._header(final, 2)
        self.b.put(hlit - 257, 5)
        self.b.put(hdist - 1, 5)
        self.b.put(hclen - 4, 4)
        for i in range(hclen):
            self.b.put(cl[CL_ORDER[i]], 3)
        codes = canonical(cl)
        for s, extra, n in syms:
            assert codes[s] is not None, "code-length symbol %d has no code" % s
            self.b.code(*codes[s])
            self.b.put(extra, n)
        self._tokens(tokens, canonical(ll), canonical(dl), eob)
        return self


# ---- what zlib makes of a stream, and the two framings -----------------------------------------------------------------------------------

def inflate(raw):
    """the text of a raw deflate stream by zlib, which has to end with the stream's last byte"""
    d = zlib.decompressobj(-15)
    text = d.decompress(raw)
    assert d.eof and not d.unused_data, "not a whole stream"
    return text


def refusal(raw):
    """why zlib refuses the raw stream: its message, "" for a stream that merely ends early, None where it does not refuse"""
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
    except zlib.error as e:
        return str(e)
    return None if d.eof else ""


def as_zlib(raw, text):
    return b"\x78\x9c" + raw + zlib.adler32(text).to_bytes(4, "big")


def as_member(raw, text):
    return member(text, payload=raw)


# ---- the scanner -------------------------------------------------------------------------------------------------------------------

class _Reader:
    def __init__(self, data):
        self.d, self.p, self.end = bytes(data) + bytes(4), 0, 8 * len(data)

    def peek(self, n):                                            # n <= 24
        at = self.p >> 3
        return (int.from_bytes(self.d[at:at + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.p += n
        if self.p > self.end:
            raise EOFError("the stream ends inside a field")
        return v


class _Code:
    """a canonical code by its counts per length and its symbols in (length, symbol) order"""

    def __init__(self, lengths):
        self.lengths = list(lengths)
        self.count = [0] * 16
        for l in lengths:
            self.count[l] += 1
        self.count[0] = 0
        self.symbols = [s for _, s in sorted((l, s) for s, l in enumerate(lengths) if l)]

    def next(self, r):
        """(symbol, the length of its code)"""
        v = r.peek(15)
        code = first = index = 0
        for L in range(1, 16):
            code |= v & 1
            v >>= 1
            c = self.count[L]
            if code - c < first:
                r.get(L)
                return self.symbols[index + code - first], L
            index += c
            first = (first + c) << 1
            code <<= 1
        raise ValueError("bits that are no code at bit %d" % r.p)


def _crossed(start, count, hlit):
    """a repeat of `count` lengths from index `start` on lies on both sides of the literal/length lengths' end"""
    return start < hlit < start + count


def _symbols(r, ll, dd, text, rep):
    """the symbols of one block up to its end-of-block"""
    lit_lens, len_lens, d_lens, route, switches = set(), set(), set(), None, 0
    n = 0
    while True:
        s, L = ll.next(r)
        n += 1
        if route is not None and route != (L > 10):
            switches += 1
        route = L > 10
        if s < 256:
            lit_lens.add(L)
            text.append(s)
            continue
        if s == 256:
            rep["eob_len"] = L
            break
        assert s <= 285, "literal/length symbol %d" % s
        len_lens.add(L)
        e = r.get(LEN_EXTRA[s - 257])
        rep["len_syms"].setdefault(s, set()).add(e)
        length = LEN_BASE[s - 257] + e
        ds, DL = dd.next(r)
        assert ds <= 29, "distance symbol %d" % ds
        d_lens.add(DL)
        de = r.get(DIST_EXTRA[ds])
        rep["dist_syms"].setdefault(ds, set()).add(de)
        dist = DIST_BASE[ds] + de
        assert dist <= len(text), "a distance of %d after %d bytes" % (dist, len(text))
        rep["matches"].append((len(text), length, dist))
        for _ in range(length):
            text.append(text[-dist])
    rep.update(n_symbols=n, lit_used_lens=lit_lens, len_used_lens=len_lens, ll_used_lens=lit_lens | len_lens | {rep["eob_len"]},
               d_used_lens=d_lens, route_switches=switches)
    rep["ll_used"] = max(rep["ll_used_lens"])
    rep["d_used"] = max(d_lens, default=0)


def scan(raw):
    """{"blocks": [a report per block], "bits": the bits the stream takes, "text": its text} of a VALID raw deflate stream.
    Every report: kind, final, bit_at (of its first header bit), align (bit_at mod 8), out_at (the text in front of it);
    stored: len;  fixed and dynamic: the symbol side (ll_used, d_used, *_used_lens, eob_len, len_syms / dist_syms = {symbol: the extra
    values seen}, matches = [(text in front, length, distance)], route_switches = how often a literal/length code of more than 10 bits
    followed one of at most 10 or the reverse, n_symbols);  dynamic: hlit, hdist, hclen (the numbers, not the fields), cl_declared /
    cl_used, ll_declared, d_declared (the longest code of either kind), reps = [(16 | 17 | 18, count, the index it starts at, the
    length it repeats, the symbol in front of it)], crossed = the repeat symbols that ran across the HLIT boundary."""
    r, text, blocks = _Reader(raw), bytearray(), []
    final = 0
    while not final:
        rep = {"bit_at": r.p, "align": r.p & 7, "out_at": len(text)}
        final = r.get(1)
        kind = r.get(2)
        rep["final"] = bool(final)
        assert kind != 3, "block type 3"
        if kind == 0:
            r.get(-r.p & 7)
            n, nn = r.get(16), r.get(16)
            assert n ^ 0xFFFF == nn, "LEN and NLEN"
            at = r.p >> 3
            assert at + n <= len(raw), "a stored block longer than the stream"
            text += raw[at:at + n]
            r.p += 8 * n
            rep.update(kind="stored", len=n)
            blocks.append(rep)
            continue
        rep.update(len_syms={}, dist_syms={}, matches=[])
        if kind == 1:
            rep["kind"] = "fixed"
            ll, dd = _Code(FIXED_LL), _Code(FIXED_D)
        else:
            hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
            assert hlit <= 286 and hdist <= 30
            cl = [0] * 19
            for i in range(hclen):
                cl[CL_ORDER[i]] = r.get(3)
            assert kraft(cl) == 32768, "the code-length code is not complete"
            cc = _Code(cl)
            lens, reps, crossed, cl_used, before = [], [], set(), 0, None
            while len(lens) < hlit + hdist:
                s, L = cc.next(r)
                cl_used = max(cl_used, L)
                if s < 16:
                    lens.append(s)
                else:
                    assert s != 16 or lens, "a 16 with nothing in front of it"
                    v = lens[-1] if s == 16 else 0
                    count = 3 + r.get(2) if s == 16 else 3 + r.get(3) if s == 17 else 11 + r.get(7)
                    assert len(lens) + count <= hlit + hdist, "a repeat past the lengths"
                    reps.append((s, count, len(lens), v, before))
                    if _crossed(len(lens), count, hlit):
                        crossed.add(s)
                    lens += [v] * count
                before = s
            assert lens[256], "no end-of-block code"
            for name, part in (("literal/length", lens[:hlit]), ("distance", lens[hlit:])):
                k = kraft(part)
                assert k == 32768 or (k in (0, 16384) and max(part) <= 1 and name == "distance") or (k == 16384 and max(part) == 1), "the %s set" % name
            ll, dd = _Code(lens[:hlit]), _Code(lens[hlit:])
            rep.update(kind="dynamic", hlit=hlit, hdist=hdist, hclen=hclen, cl_declared=max(cl), cl_used=cl_used, ll_declared=max(lens[:hlit]),
                       d_declared=max(lens[hlit:]), reps=reps, crossed=crossed, ll_lengths=lens[:hlit], d_lengths=lens[hlit:])
        _symbols(r, ll, dd, text, rep)
        blocks.append(rep)
    return {"blocks": blocks, "bits": r.p, "text": bytes(text)}


def extremes(syms, extra_bits, base):
    """the symbols of {symbol: extra values seen} that were seen with their extra bits all zero AND all one"""
    return {s for s, seen in syms.items() if 0 in seen and (1 << extra_bits[s - base]) - 1 in seen}
