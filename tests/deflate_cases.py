"""The dynamic-code streams of test_deflate_tokens_cpu.py and test_gpu_inflate_dynamic.py, built with deflate_tokens.Stream: streams
that are valid RFC 1951 but that zlib's encoder never writes, and streams zlib refuses.  Every valid case carries a check of the
scanner's report -- the property the case is named for -- so that an edit cannot make it degenerate unnoticed; every refusal carries
the words zlib refuses it with.  The text of a case is what zlib makes of its stream.  Every text ends in a newline, so that it is a
quality block of text.count(b"\\n") reads as well as a BGZF member."""
import random

from bgzf_input import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA
import deflate_tokens as T

ZLIB, RAW = "zlib", "raw"                                          # the quality blocks' path, the BGZF members' path


class Valid:
    def __init__(self, name, raw, check, paths=(ZLIB, RAW)):
        self.name, self.raw, self.check, self.paths = name, raw, check, paths
        self.text = T.inflate(raw)
        assert self.text.endswith(b"\n") and 0xA5 not in self.text, name
        assert RAW not in paths or len(self.text) <= 65536, name

    def block(self):
        """(payload, n_reads, n_bytes) of the quality path"""
        n = self.text.count(b"\n")
        return T.as_zlib(self.raw, self.text), n, len(self.text) - n

    def member(self):
        return T.as_member(self.raw, self.text)


class Refused:
    def __init__(self, name, raw, words, text=b"", paths=(ZLIB, RAW)):
        """words: what zlib's message has to hold ("" for a stream that only ends early); text: the text the tables claim"""
        self.name, self.raw, self.words, self.text, self.paths = name, raw, words, text, paths

    def block(self):
        n = self.text.count(b"\n")
        return (T.as_zlib(self.raw, self.text), n, len(self.text) - n) if self.text else (T.as_zlib(self.raw, b""), 1, 1)

    def member(self):
        import zlib
        from bgzf_input import frame
        return frame(self.raw, zlib.crc32(self.text), len(self.text) if self.text else 2)


def lines(rng, n, alphabet=b"ACGT", width=60):
    """n bytes of lines over the alphabet, the last byte a newline"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, width))) + b"\n"
    return bytes(out[:n - 1]) + b"\n"


def only(report):
    assert len(report["blocks"]) == 1
    return report["blocks"][0]


# ---- valid: the literal/length ladder ----------------------------------------------------------------------------------------------

LADDER_LL = {65: 1, 67: 2, 71: 3, 84: 4, 10: 5, 70: 6, 257: 7, 73: 8, 35: 10, 258: 10, 44: 11, 259: 11, 58: 12, 265: 12, 59: 13, 273: 13,
             60: 14, 284: 14, 61: 15, 62: 15, 285: 15, 256: 15}


def ll_ladder():
    rng = random.Random(1)
    s = T.Stream()
    short = [k for k, l in LADDER_LL.items() if l <= 10]
    long_ = [k for k, l in LADDER_LL.items() if l > 10 and k != 256]
    tokens = [bytes(k for k in LADDER_LL if k < 256)]
    for i in range(400):                                           # a code of at most 10 bits, then one of more, symbol by symbol
        for k in (rng.choice(short), long_[i % len(long_)] if i < 2 * len(long_) else rng.choice(long_)):
            if k < 256:
                tokens.append(bytes([k]))
            else:
                e = LEN_EXTRA[k - 257]
                tokens.append(("m", k, rng.choice((0, (1 << e) - 1, rng.randrange(1 << e))), rng.randrange(4), 0))
                tokens.append(bytes([rng.choice(short[:6])]))      # (a distance code sits between two literal/length codes)
    s.dynamic(LADDER_LL, {0: 2, 1: 2, 2: 2, 3: 2}, tokens, final=True, eob=False)
    pad = -(s.bits() + 5 + 15) % 8                                 # 'A' has a code of one bit: the end-of-block code ends the last byte
    s.more([b"A" * pad + b"\n"])
    assert s.b.n == 0
    raw = s.done()

    def check(rep):
        b = only(rep)
        assert rep["bits"] == 8 * len(raw) and b["eob_len"] == 15, "the 15-bit end-of-block code does not end on the last bit"
        assert b["ll_declared"] == 15 and {11, 12, 13, 14, 15} <= b["lit_used_lens"] and {11, 12, 13, 14, 15} <= b["len_used_lens"]
        assert {l for l in b["ll_used_lens"] if l <= 10} >= {1, 2, 3, 8, 10} and b["route_switches"] >= 700
        assert 31 in b["len_syms"][284] and 0 in b["len_syms"][285] and b["hclen"] == 19
    return Valid("literal/length ladder: 11..15-bit literals, lengths and end-of-block", raw, check)


# ---- valid: the distance ladder, every length and distance symbol at both ends of its extra bits ------------------------------------

def dist_ladder():
    rng = random.Random(2)
    ls = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 11, 12, 12, 12] + [13] * 6 + [14] * 6 + [15] * 4
    assert len(ls) == 30 and T.kraft(ls) == 32768
    dl = {s: ls[s * 7 % 30] for s in range(30)}
    lits = b"ACGT\nN#I"
    ll = T.balanced(list(lits) + [256] + list(range(257, 286)))
    lplan = [(s, e) for s in range(257, 286) for e in sorted({0, (1 << LEN_EXTRA[s - 257]) - 1})]
    dplan = sorted((DIST_BASE[s] + e, s, e) for s in range(30) for e in sorted({0, (1 << DIST_EXTRA[s]) - 1}))
    tokens, out, li = [lines(rng, 40, lits[:4])], 40, 0

    def match(ds, de):
        nonlocal out, li
        s, e = lplan[li % len(lplan)]
        li += 1
        tokens.append(("m", s, e, ds, de))
        tokens.append(bytes(rng.choice(lits) for _ in range(rng.randrange(0, 3))))
        out += LEN_BASE[s - 257] + e + len(tokens[-1])

    for dist, ds, de in dplan:
        while out < dist:
            _, fs, fe = rng.choice([p for p in dplan if p[0] <= out])
            match(fs, fe)
        match(ds, de)
    while li < len(lplan):
        match(*rng.choice(dplan)[1:])
    tokens.append(b"\n")
    raw = T.Stream().dynamic(ll, dl, tokens, final=True).done()

    def check(rep):
        b = only(rep)
        assert b["hlit"] == 286 and b["hdist"] == 30 and b["d_declared"] == 15
        assert b["d_used_lens"] == set(ls) and {10, 11, 12, 13, 14, 15} <= b["d_used_lens"]
        assert T.extremes(b["dist_syms"], DIST_EXTRA, 0) == set(range(30)), "a distance symbol misses an end of its extra bits"
        assert T.extremes(b["len_syms"], LEN_EXTRA, 257) == set(range(257, 286)), "a length symbol misses an end of its extra bits"
        assert 31 in b["len_syms"][284] and max(m[2] for m in b["matches"]) == 32768
    return Valid("distance ladder: 10..15-bit distance codes, every length and distance symbol at both ends", raw, check)


# ---- valid: the code-length alphabet -----------------------------------------------------------------------------------------------

def cl_seven_bits():
    ll = {65: 1, 67: 2, 71: 3, 84: 4, 10: 5, 256: 5}
    cl = {18: 1, 0: 2, 17: 3, 1: 4, 2: 5, 3: 6, 4: 7, 5: 7}
    raw = T.Stream().dynamic(ll, {}, [b"ACGTTGCA\nAAAC\n"], final=True, cl=cl).done()

    def check(rep):
        b = only(rep)
        assert b["cl_declared"] == 7 and b["cl_used"] == 7 and b["hclen"] == 18 and b["hdist"] == 1 and b["d_declared"] == 0 and not b["matches"]
    return Valid("code-length alphabet: a 7-bit code in use, HDIST = 1 of length 0, no match", raw, check)


def hclen_smallest():
    rng = random.Random(3)
    ll = {s: 8 for s in range(1, 257)}
    items = [("len", 0), ("len", 8)] + [("rep", 6)] * 42 + [("rep", 3), ("len", 0)]
    text = bytes(rng.randrange(32, 127) for _ in range(200)) + bytes([1, 255, 164, 166]) + b"\n"
    raw = T.Stream().dynamic(ll, {}, [text], final=True, items=items, cl={16: 1, 0: 2, 8: 2}).done()

    def check(rep):
        b = only(rep)
        assert b["hclen"] == 5 and b["hlit"] == 257 and [r[:2] for r in b["reps"]] == [(16, 6)] * 42 + [(16, 3)]
    return Valid("HCLEN = 5, the fewest a block with any code can have", raw, check)


def hclen_nineteen():
    syms = list(b"ACGTNacgtn#,:;\n") + [256]
    assert len(syms) == 16
    ll = dict(zip(syms, list(range(1, 15)) + [15, 15]))
    items = T.auto_items(T.table(ll, 257)) + [("len", 0)]
    used = sorted({T.item_symbol(it)[0] for it in items})
    cl = dict(zip(used, reversed(T.complete_lengths(len(used), 7))))       # 7 bits for the smallest symbols: the zeros' and the one-bit code's
    raw = T.Stream().dynamic(ll, {}, [bytes(syms[:15]) * 2 + b"\n"], final=True, items=items, cl=cl).done()

    def check(rep):
        b = only(rep)
        assert b["hclen"] == 19 and b["cl_used"] == 7 and b["ll_used"] == 15 and b["lit_used_lens"] == set(range(1, 16))
    return Valid("HCLEN = 19 with a 7-bit code-length code and a 1..15 literal ladder", raw, check)


# ---- valid: repeats across the boundary between the two length arrays ----------------------------------------------------------------

def rep16_crosses():
    ll = {65: 3, 10: 3, 256: 2, 257: 2, 258: 2}
    dl = {0: 2, 1: 2, 2: 2, 3: 2}
    items = T.auto_items(T.table(ll, 256)[:256]) + [("len", 2), ("rep", 6)]
    raw = T.Stream().dynamic(ll, dl, [b"AA\nA", (3, 1), (4, 2), (3, 3), (4, 4), b"\n"], final=True, items=items, hlit=259, hdist=4).done()

    def check(rep):
        b = only(rep)
        assert b["crossed"] == {16} and b["reps"][-1] == (16, 6, 257, 2, 2), b["reps"]
        assert b["reps"][-1][1] + b["reps"][-1][2] == b["hlit"] + b["hdist"], "the last repeat does not spend the last length"
        assert set(b["dist_syms"]) == {0, 1, 2, 3}
    return Valid("a 16 from the literal/length lengths into the distance lengths, the header's last item", raw, check)


def rep17_crosses():
    ll = {65: 2, 10: 2, 256: 2, 257: 2}
    dl = {8: 1, 9: 1}
    items = T.auto_items(T.table(ll, 256)[:256]) + [("len", 2), ("len", 2), ("zeros", 10), ("len", 1), ("len", 1)]
    tokens = [lines(random.Random(4), 40, b"A"), (3, 17), (3, 24), (3, 25), (3, 32), b"\n"]
    raw = T.Stream().dynamic(ll, dl, tokens, final=True, items=items, hlit=260, hdist=10).done()

    def check(rep):
        b = only(rep)
        assert b["crossed"] == {17} and (17, 10, 258, 0, 2) in b["reps"] and T.extremes(b["dist_syms"], DIST_EXTRA, 0) == {8, 9}
    return Valid("a 17 of 10 zeros from the literal/length lengths into the distance lengths", raw, check)


def rep18_crosses_to_one_far_code():
    ll = {65: 2, 10: 2, 256: 2, 257: 2}
    items = T.auto_items(T.table(ll, 256)[:256]) + [("len", 2), ("len", 2), ("zeros", 57), ("len", 1)]
    tokens = [lines(random.Random(5), 24577, b"A", 150), (3, 24577), b"\n"]
    raw = T.Stream().dynamic(ll, {29: 1}, tokens, final=True, items=items, hlit=286, hdist=30).done()

    def check(rep):
        b = only(rep)
        assert b["crossed"] == {18} and (18, 57, 258, 0, 2) in b["reps"] and b["matches"] == [(24577, 3, 24577)]
        assert b["d_lengths"] == [0] * 29 + [1]
    return Valid("an 18 of 57 zeros across the boundary, then distance symbol 29 alone with a code of one bit", raw, check)


def rep18_crosses_to_the_end():
    ll = {65: 2, 66: 2, 10: 2, 256: 2}
    items = T.auto_items(T.table(ll, 256)[:256]) + [("len", 2), ("zeros", 59)]
    raw = T.Stream().dynamic(ll, {}, [b"ABBA\n"], final=True, items=items, hlit=286, hdist=30).done()

    def check(rep):
        b = only(rep)
        assert b["crossed"] == {18} and b["reps"][-1] == (18, 59, 257, 0, 2) and b["hlit"] + b["hdist"] == 316 and b["d_declared"] == 0
    return Valid("an 18 of 59 zeros -- the most that can cross -- ends HLIT = 286 and all of HDIST = 30", raw, check)


def repeat_counts():
    ll = {10: 2, 65: 2, 66: 2, 256: 2}
    items = [("zeros", 10), ("len", 2), ("zeros", 51), ("rep", 3), ("len", 2), ("len", 2), ("zeros", 3), ("rep", 6), ("zeros", 138), ("zeros", 11),
             ("rep", 4), ("rep", 5), ("zeros", 22), ("len", 2), ("len", 0)]
    raw = T.Stream().dynamic(ll, {}, [b"ABBA\nB\n"], final=True, items=items).done()

    def check(rep):
        b = only(rep)
        assert [r[:2] for r in b["reps"]] == [(17, 10), (18, 51), (16, 3), (17, 3), (16, 6), (18, 138), (18, 11), (16, 4), (16, 5), (18, 22)]
        assert [r[3:] for r in b["reps"] if r[0] == 16] == [(0, 18), (0, 17), (0, 18), (0, 16)], "the 16s do not repeat a zero behind a 17 / 18"
        assert not b["crossed"]
    return Valid("a 16 behind a 17 and behind an 18, 16 at 3 4 5 6, 17 at 3 and 10, 18 at 11 and 138", raw, check)


# ---- valid: sparse sets ------------------------------------------------------------------------------------------------------------

def one_distance_code():
    raw = T.Stream().dynamic({65: 2, 10: 2, 256: 2, 257: 2}, {0: 1}, [b"A\n", (3, 1), b"A", (3, 1), b"\n"], final=True).done()

    def check(rep):
        b = only(rep)
        assert b["hlit"] == 258 and b["hdist"] == 1 and b["d_lengths"] == [1] and len(b["matches"]) == 2
    return Valid("one distance code of one bit (the incomplete set zlib allows)", raw, check)


def hlit_257():
    raw = T.Stream().dynamic({65: 1, 10: 2, 256: 2}, {}, [b"AAA\n\nA\n"], final=True).done()

    def check(rep):
        b = only(rep)
        assert b["hlit"] == 257 and b["hdist"] == 1 and b["d_lengths"] == [0] and not b["matches"] and b["hclen"] < 19
    return Valid("HLIT = 257, HDIST = 1 with length 0, no match", raw, check)


def hlit_286_hdist_30():
    raw = T.Stream().dynamic({65: 1, 10: 2, 256: 3, 285: 3}, {0: 1, 29: 1}, [b"A", ("m", 285, 0, 0, 0), b"\n"], final=True).done()

    def check(rep):
        b = only(rep)
        assert b["hlit"] == 286 and b["hdist"] == 30 and b["matches"] == [(1, 258, 1)] and b["d_lengths"][29] == 1
    return Valid("HLIT = 286 and HDIST = 30 in a block of three symbols", raw, check)


# ---- valid: chains of blocks -------------------------------------------------------------------------------------------------------

def chain():
    s = T.Stream()
    a = {65: 1, 67: 2, 10: 3, 256: 4, 257: 4}
    b_ = {84: 2, 10: 2, 258: 2, 256: 3, 71: 3}                       # other lengths for '\n' and the end-of-block: the tables are rebuilt
    c = T.balanced([65, 67, 71, 84, 10, 256, 257, 285])
    s.dynamic(a, {0: 1, 1: 1}, [b"ACCA\nAC", (3, 2)])
    s.fixed([b"GATTACA\n", (5, 8), (3, 15)])
    s.fixed([b"TT", (258, 1), b"\n"])
    s.dynamic(b_, {4: 1, 5: 1}, [b"GT\n", (4, 5), (4, 8), b"T"])
    s.stored(b"")
    s.fixed([b"\nCAT", (3, 4), (10, 300)])
    s.dynamic(c, {0: 2, 1: 2, 2: 2, 16: 2}, [b"G", (258, 1), (3, 3), (258, 257), (3, 384), b"\n"], final=True)
    raw = s.done()

    def check(rep):
        assert [b["kind"] for b in rep["blocks"]] == ["dynamic", "fixed", "fixed", "dynamic", "stored", "fixed", "dynamic"]
        assert rep["blocks"][4]["len"] == 0 and [b["final"] for b in rep["blocks"]] == [False] * 6 + [True]
        assert all(b["matches"] for b in rep["blocks"] if b["kind"] != "stored")
        assert any(m[2] > m[0] - b["out_at"] for b in rep["blocks"][1:] if b["kind"] != "stored" for m in b["matches"]), "no match reaches into an earlier block"
    return Valid("dynamic, fixed, fixed, dynamic, stored of LEN 0, fixed, dynamic in one stream", raw, check)


def stored_alignments():
    s = T.Stream()
    s.dynamic({65: 1, 10: 2, 256: 2}, {}, [b"AA\n"])
    for a in range(8):
        k = next(k for k in range(8) if (s.bits() + 10 + 9 * k) % 8 == a)       # a literal above 143 has 9 bits in the fixed code
        s.fixed([bytes([200]) * k])
        assert s.bits() % 8 == a
        s.stored(b"<%d>\n" % a)
    s.fixed([(5, 5), b"\n"], final=True)
    raw = s.done()

    def check(rep):
        stored = [b for b in rep["blocks"] if b["kind"] == "stored"]
        assert [b["align"] for b in stored] == list(range(8)) and all(b["len"] == 4 for b in stored)
    return Valid("a stored block entered at each of the 8 bit alignments", raw, check)


def stored_65535():
    rng = random.Random(6)
    s = T.Stream()
    s.dynamic({65: 1, 10: 2, 256: 2}, {}, [b"A\n"])
    s.stored(lines(rng, 65535, b"ACGTN#"))
    s.dynamic({10: 1, 256: 2, 285: 3, 257: 3}, {0: 1, 29: 1}, [("m", 285, 0, 29, 8191), ("m", 257, 0, 29, 0), (258, 1), b"\n"], final=True)
    raw = s.done()

    def check(rep):
        assert [b["kind"] for b in rep["blocks"]] == ["dynamic", "stored", "dynamic"] and rep["blocks"][1]["len"] == 65535
        assert rep["blocks"][1]["align"] != 0 and rep["blocks"][2]["matches"][0] == (65537, 258, 32768)
    return Valid("a stored block of LEN 65 535 between two dynamic ones", raw, check, paths=(ZLIB,))


def empty_dynamic():
    s = T.Stream()
    s.dynamic({65: 1, 256: 1}, {})
    s.dynamic({65: 2, 10: 2, 256: 2, 66: 2}, {}, [b"AB\n"], final=True)
    raw = s.done()

    def check(rep):
        first = rep["blocks"][0]
        assert first["kind"] == "dynamic" and not first["final"] and first["n_symbols"] == 1 and rep["blocks"][1]["out_at"] == 0
    return Valid("a dynamic block of a header and its end-of-block, not the last", raw, check)


# ---- valid: the copy routes --------------------------------------------------------------------------------------------------------

def copy_routes():
    rng = random.Random(7)
    ll = T.balanced(list(b"ACGT\n") + [256, 257, 285])
    dl = T.balanced([0, 1, 2, 11, 12])
    tokens = [lines(rng, 70)]
    for d in (1, 2, 3, 63, 64, 65):
        tokens += [(3, d), bytes([rng.choice(b"ACGT")]), (258, d), bytes([rng.choice(b"ACGT")])]
    tokens.append(b"\n")
    raw = T.Stream().dynamic(ll, dl, tokens, final=True).done()

    def check(rep):
        b = only(rep)
        assert {(m[1], m[2]) for m in b["matches"]} == {(n, d) for n in (3, 258) for d in (1, 2, 3, 63, 64, 65)}
    return Valid("distances 1, 2, 3, 63, 64, 65 with lengths 3 and 258", raw, check)


def flush_edges():
    rng = random.Random(8)
    ll = T.balanced(list(b"ACGT\n") + [256, 285])
    ll[256], ll[285] = ll[285], ll[256]
    want, tokens, out = [], [], 0
    for k, (d, delta) in enumerate((d, delta) for d in (1, 7, 100) for delta in (-1, 0, 1)):
        start = 1024 * (k + 1) + delta - 258
        tokens += [lines(rng, start - out), (258, d)]
        want.append((start, 258, d))
        out = start + 258
    tokens.append(b"\n")
    raw = T.Stream().dynamic(ll, {0: 1, 5: 2, 13: 2}, tokens, final=True).done()

    def check(rep):
        b = only(rep)
        assert b["matches"] == want and [(m[0] + 258) % 1024 for m in want] == [1023, 0, 1] * 3
    return Valid("258-byte matches that end one before, on and one past a multiple of 1 024, by each copy route", raw, check)


def ring_wraps():
    rng = random.Random(9)
    ll = T.balanced(list(b"ACGT#\n") + [256, 257, 285])
    tokens = [lines(rng, 32768, b"ACGT#"), (258, 32768)]
    out = 32768 + 258
    while out + 258 <= 131072:
        tokens.append((258, 32768))
        out += 258
    while out < 131072:
        tokens.append((3, 32768))
        out += 3
    assert out == 131072
    tokens += [(258, 32768), (3, 32767), (258, 1), (3, 32768), b"\n"]
    raw = T.Stream().dynamic(ll, {0: 1, 29: 1}, tokens, final=True).done()

    def check(rep):
        b = only(rep)
        assert b["matches"][0] == (32768, 258, 32768) and (131072, 258, 32768) in b["matches"] and b["matches"][-1][0] > 4 * 32768
        assert any(m[0] < 65536 < m[0] + m[1] for m in b["matches"]), "no match lies across the ring's end"
        assert {8190, 8191} <= b["dist_syms"][29]
    return Valid("distance 32 768 at 32 768 bytes and again at 131 072, the ring wrapped four times", raw, check, paths=(ZLIB,))


# ---- refused -----------------------------------------------------------------------------------------------------------------------

SMALL = {65: 2, 10: 2, 256: 2, 257: 2}
PAD = bytes(8)                                                     # bits behind the fault, so that no stream merely ends early


def refusals(ladder):
    out = []

    def add(name, stream, words, **kw):
        out.append(Refused(name, stream.done() + PAD, words, **kw))

    add("an over-subscribed literal/length set", T.Stream().dynamic({65: 1, 10: 1, 256: 1}, {}, [b"A\n"], final=True, check=False), "invalid literal/lengths set")
    add("an incomplete literal/length set of two 2-bit codes", T.Stream().dynamic({65: 2, 256: 2}, {}, [b"A"], final=True, check=False), "invalid literal/lengths set")
    add("an incomplete distance set of two codes", T.Stream().dynamic(SMALL, {0: 2, 1: 2}, [b"A\n", (3, 1)], final=True, check=False), "invalid distances set")
    add("a one-code distance set and a match that uses the bit pattern without a code",
        T.Stream().dynamic(SMALL, {0: 1}, [b"A\n", (3, 1), ("l", 257, 0), ("bits", 1, 1), b"\n"], final=True), "invalid distance code")
    add("a 16 as the first item", T.Stream().dynamic(SMALL, {}, [b"A\n"], final=True, check=False, cl={16: 2, 0: 2, 2: 2, 17: 3, 18: 3},
                                                  items=[("rep", 3), ("zeros", 7), ("len", 2)] + T.auto_items(T.table(SMALL, 258)[11:])), "invalid bit length repeat")
    add("a repeat that runs past the last length", T.Stream().dynamic(SMALL, {0: 1}, [b"A\n"], final=True, check=False, hlit=258, hdist=1,
                                                                     items=T.auto_items(T.table(SMALL, 258)[:257]) + [("len", 2), ("rep", 3)]), "invalid bit length repeat")
    for field in (30, 31):
        add("HLIT field %d" % field, T.Stream().dynamic(SMALL, {}, [b"A\n"], final=True, check=False, hlit=257 + field), "too many length or distance symbols")
        add("HDIST field %d" % field, T.Stream().dynamic(SMALL, {0: 1}, [b"A\n"], final=True, check=False, hdist=1 + field), "too many length or distance symbols")
    add("a match in a block that declared no distance code", T.Stream().dynamic(SMALL, {}, [b"A\n", ("l", 257, 0), ("bits", 0, 1), b"\n"], final=True),
        "invalid distance code")
    add("a distance one more than the bytes written", T.Stream().dynamic(SMALL, {2: 1, 5: 1}, [b"AA\n", (3, 3), (3, 7), b"\n"], final=True), "invalid distance too far back")
    add("an 18 of 138 zeros across the boundary, which takes the end-of-block code with it",
        T.Stream().dynamic({65: 1, 10: 1}, {28: 1, 29: 1}, [b"A\n"], final=True, check=False, eob=False, hlit=286, hdist=30,
                           items=T.auto_items(T.table({65: 1, 10: 1}, 176)[:176]) + [("zeros", 138), ("len", 1), ("len", 1)]), "missing end-of-block")
    out.append(Refused("the literal/length ladder without its last byte: the 15-bit end-of-block code is cut", ladder.raw[:-1], "", text=ladder.text))
    return out


# ---- all of them, built once -------------------------------------------------------------------------------------------------------

_CASES = None


def cases():
    """(the valid cases, the refused ones)"""
    global _CASES
    if _CASES is None:
        valid = [f() for f in (ll_ladder, dist_ladder, cl_seven_bits, hclen_smallest, hclen_nineteen, rep16_crosses, rep17_crosses, rep18_crosses_to_one_far_code,
                               rep18_crosses_to_the_end, repeat_counts, one_distance_code, hlit_257, hlit_286_hdist_30, chain, stored_alignments, stored_65535,
                               empty_dynamic, copy_routes, flush_edges, ring_wraps)]
        _CASES = (valid, refusals(valid[0]))
    return _CASES
