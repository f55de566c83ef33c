"""Read blocks that leave the conforming set ON PURPOSE (test support, no GPU): the inputs of tests/test_dna_bad_streams_cpu.py and
tests/test_gpu_dna_refusals.py.

tests/dna_streams.py writes what a conforming encoder may write.  Here one chosen read of one chosen block gets a field, a delta type,
a list's declared size or its entries replaced (dna_streams.Tamper), the block table or the payload's length is changed, or a
conforming call is made heavy enough in N to need the decoder's list pool.  Every case states what must happen, from what the writer
knows and never from a decoder: `code` 1..4 (k_decode_blocks' refusal, WORDS), ANY (refused, whatever the reason), or None (it
decodes, to `reads`).

The bad read sits in block 1 of dna_streams.base_input(k) (400 reads, 100 per block) in three places: as the block's first read (no
previous values), as its last (99 reads of state before it) and right behind a read coded without its anchor.  Blocks 0, 2 and 3 stay
the conforming ones."""
import functools
import random
from dataclasses import dataclass
from typing import Optional

import numpy as np

import dna_streams as S

WORDS = {1: "anchor address or position out of range", 2: "more or fewer bases than the block table says",
         3: "too many N / error positions in one read", 4: "the payload ends before its reads do"}
ANY = "any"
PLACES = ("first", "last", "behind-noanchor")
DC_LIST_CAP = 8192                                       # decode_kernels.hip: longer lists of one read come from the pool
FIRST_POOL_FLOOR = 1 << 20                               # words of the pool a call of fewer than 2^21 bases starts with


def message(block, code):
    return "block %d does not decode: %s" % (block, WORDS[code])


@dataclass
class Case:
    name: str
    k: int
    anchors: list                                        # the dictionary, python ints
    blocks: list                                         # [(block id, payload, n reads)]
    nbases: list
    code: object = None                                  # 1..4 | ANY | None (decodes)
    reads: Optional[list] = None                         # what it decodes to (normalised), where it does or may
    may_decode: bool = False                             # with code ANY: decoding is allowed too, and then gives `reads`
    oracle: bool = True                                  # False: a value near 2^64 or above 2^31 -- the oracle's checks are sums that wrap
    bad_block: int = 1
    bad_syms: Optional[tuple] = None                     # (symbols of the bad block, symbols of its conforming twin, index of the bad read's first)
    repeats_walked: int = 0                              # equal-neighbour cases: repeats with a real, walked list position behind them
    twin: Optional[list] = None                          # blocks of the same call without the entries behind the repeats (must decode differently)
    ri: int = 0                                          # index of the chosen read in its block


@functools.lru_cache(maxsize=None)
def good(k):
    """the conforming four-block call every case is a variation of: (input, blocks, bases per block)"""
    inp = S.base_input(k)
    blocks, nbases, _ = S.build_blocks(inp.reads, k, inp.rpb, inp.bloom, inp.anchors, random.Random(k), S.POLICIES["base"], inp.cache)
    return inp, blocks, nbases


def good_reads(k):
    return [S.norm(r) for r in S.base_input(k).reads]


@functools.lru_cache(maxsize=None)
def _index(k):
    index = {}
    for a, x in enumerate(S.base_input(k).anchors):
        index.setdefault(x, []).append(a)
    return index


def _cands(read, k):
    return S.candidates([S._CODE.get(c, 0) for c in read], k, _index(k))


ROOM = 22                                                # walked positions the chosen read has on either side of its anchor


@functools.lru_cache(maxsize=None)
def _chosen(k, b):
    """(index in the block, anchor choice) of the read of block b that is tampered with: no N, an anchor candidate with ROOM on both sides"""
    inp = S.base_input(k)
    for j, r in enumerate(inp.reads[b * inp.rpb:(b + 1) * inp.rpb]):
        if any(c not in S._CODE for c in r):
            continue
        for c in _cands(r, k):
            if c[0] >= ROOM and len(r) - c[0] - k >= ROOM:
                return j, c
    raise AssertionError("no read with room around an anchor")


def layout(k, b, place, edit=None, noanchor=False):
    """block b's reads with the chosen read R (edited by `edit(R, apos)`) at `place`: (reads, given, ri, R, choice, bases left at R)"""
    inp = S.base_input(k)
    part = list(inp.reads[b * inp.rpb:(b + 1) * inp.rpb])
    j, choice = _chosen(k, b)
    R = part.pop(j)
    if edit:
        R = edit(R, choice[0])
    ri = {"first": 0, "last": len(part), "behind-noanchor": 50}[place]
    given = []
    for r in part:
        c = _cands(r, k)
        given.append(c[0] if c else None)
    part.insert(ri, R)
    given.insert(ri, None if noanchor else choice)
    if place == "behind-noanchor":
        given[ri - 1] = None
    left = sum(len(r) for r in part[ri:])
    return part, given, ri, R, choice, left


def write(k, b, place, tamper=None, edit=None, noanchor=False):
    """(payload, reads, Tamper as filled in by the writer, R, choice, bases left at R)"""
    inp = S.base_input(k)
    reads, given, ri, R, choice, left = layout(k, b, place, edit, noanchor)
    t = S.Tamper(read=ri, **(tamper(len(R), choice[0], left) if tamper else {}))
    payload, _ = S.build_block(reads, k, inp.bloom, inp.anchors, random.Random(1), S.Policy(anchor="given", given=given), inp.cache, tamper=t)
    return payload, reads, t, R, choice, left


def _call(k, b, payload, reads):
    inp, blocks, nbases = good(k)
    blocks, nbases = list(blocks), list(nbases)
    blocks[b] = (b, payload, len(reads))
    nbases[b] = sum(len(r) for r in reads)
    return blocks, nbases


def _whole(k, b, reads):
    inp = S.base_input(k)
    return [S.norm(r) for r in inp.reads[:b * inp.rpb] + list(reads) + inp.reads[(b + 1) * inp.rpb:]]


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _abs(v, nbytes=None):
    return lambda value, prev: (0, v, nbytes)


def _wrap(value, prev):
    return (2, prev + 1, None)                           # type 2 is prev - delta: prev - (prev + 1) = 2^64 - 1


def _field_refusals(k):
    """(name, code, the oracle may see it, the read is coded without its anchor, tamper(len, apos, bases left at the read))"""
    na = len(S.base_input(k).anchors)
    F = "fields"
    return [
        ("addr=n_anchors", 1, True, False, lambda L, p, left: dict(fields={"addr": _abs(na)}, cut=F)),
        ("addr=2^63", 1, False, False, lambda L, p, left: dict(fields={"addr": _abs(1 << 63, 8)}, cut=F)),
        ("addr~2^64", 1, False, False, lambda L, p, left: dict(fields={"addr": _wrap}, cut=F)),
        ("apos=len-k+1", 1, True, False, lambda L, p, left: dict(fields={"pos": _abs(L - k + 1)}, cut=F)),
        ("apos~2^64", 1, False, False, lambda L, p, left: dict(fields={"pos": _wrap}, cut=F)),
        ("len=k-1,apos=0", 1, True, False, lambda L, p, left: dict(fields={"size": _abs(k - 1), "pos": _abs(0)}, cut=F)),
        ("len=0", 1, True, False, lambda L, p, left: dict(fields={"size": _abs(0)}, cut=F)),
        ("len=left+1", 2, True, False, lambda L, p, left: dict(fields={"size": _abs(left + 1)}, cut=F)),
        ("noanchor-len=left+1", 2, True, True, lambda L, p, left: dict(fields={"nasize": _abs(left + 1)}, cut="nasize")),
        ("len=2^31", 2, True, False, lambda L, p, left: dict(fields={"size": _abs(1 << 31)}, cut=F)),
        ("len=2^31-1", 2, True, False, lambda L, p, left: dict(fields={"size": _abs((1 << 31) - 1)}, cut=F)),   # len_fits' second clause
        ("len~2^64", 2, False, False, lambda L, p, left: dict(fields={"size": _wrap}, cut=F)),
        ("n_count=len+1", 3, True, False, lambda L, p, left: dict(count={"n": lambda n, L_: L_ + 1}, cut="n_count")),
        ("err_count=len+1", 3, True, False, lambda L, p, left: dict(count={"err": lambda n, L_: L_ + 1}, cut="err_count")),
        ("n_count=2^40", 3, False, False, lambda L, p, left: dict(count={"n": lambda n, L_: 1 << 40}, cut="n_count")),
    ]


K63_SUBSET = ("addr=n_anchors", "apos=len-k+1", "len=left+1", "len~2^64", "n_count=len+1", "cut-middle", "reads-1", "reads+1")


@functools.lru_cache(maxsize=None)
def refusal_cases(k):
    """every refusal case of the issue at k = 31; at k = 63 (two-word k-mers) K63_SUBSET with the bad read first in its block"""
    inp, blocks, nbases = good(k)
    out = []
    for place in PLACES if k == 31 else PLACES[:1]:
        for name, code, oracle, noanchor, tamper in _field_refusals(k):
            if k != 31 and name not in K63_SUBSET:
                continue
            payload, reads, t, R, choice, left = write(k, 1, place, tamper, noanchor=noanchor)
            twin = write(k, 1, place, None, noanchor=noanchor)[2]
            b, nb = _call(k, 1, payload, reads)
            out.append(Case("%s, %s" % (name, place), k, inp.anchors, b, nb, code=code, oracle=oracle,
                            bad_syms=(t.syms, twin.syms, t.bad_at), ri=t.read))
    # the block table against the payload
    p1, n1 = blocks[1][1], blocks[1][2]
    last_len = len(inp.reads[2 * inp.rpb - 1])

    def table(name, code, payload, n_reads, n_bases, **kw):
        if k != 31 and name not in K63_SUBSET:
            return
        b, nb = list(blocks), list(nbases)
        b[1], nb[1] = (1, payload, n_reads), n_bases
        out.append(Case(name, k, inp.anchors, b, nb, code=code, **kw))
    table("reads-1", 2, p1, n1 - 1, nbases[1])                               # w != wcap at the block's end
    table("bases-last-read", 2, p1, n1, nbases[1] - last_len)               # the last read does not fit
    table("reads+1", ANY, p1, n1 + 1, nbases[1])
    table("empty-payload-1-read", ANY, b"", 1, 150)
    # a conforming payload cut short: zero bytes are fed behind its end, so another guard may be reached first; a cut of the last byte
    # or two may leave every symbol decodable, and then the reads must be exactly right
    n = len(p1)
    for cut, may in ((0, False), (1, False), (7, False), (8, False), (n // 2, False), (n - 17, False), (n - 2, True), (n - 1, True)):
        table("cut-middle" if cut == n // 2 else "cut-%s" % (cut if cut < 9 else "end-%d" % (n - cut)), ANY, p1[:cut], n1, nbases[1],
              may_decode=may, reads=good_reads(k) if may else None, oracle=False)
    # no dictionary at all and an anchored read: blocks 0, 2, 3 hold no anchored read (written without a dictionary), block 1 is the good one
    if k == 31:
        free, fnb, _ = S.build_blocks(inp.reads, k, inp.rpb, inp.bloom, [], random.Random(5), S.POLICIES["base"], inp.cache)
        assert fnb == nbases
        b = [free[0], blocks[1], free[2], free[3]]
        out.append(Case("empty-dictionary", k, [], b, list(nbases), code=1))
    return out


@functools.lru_cache(maxsize=None)
def two_bad_blocks(k=31):
    """block 0 fails at its LAST read, after 99 good ones (code 1); block 3 at its first symbol's read (code 2): the call names block 0"""
    inp, blocks, nbases = good(k)
    na = len(inp.anchors)
    p0, r0, _, _, _, _ = write(k, 0, "last", lambda L, p, left: dict(fields={"addr": _abs(na)}, cut="fields"))
    p3, r3, _, _, _, _ = write(k, 3, "first", lambda L, p, left: dict(fields={"size": _abs(1 << 31)}, cut="fields"))
    b, nb = list(blocks), list(nbases)
    b[0], nb[0] = (0, p0, len(r0)), sum(len(r) for r in r0)
    b[3], nb[3] = (3, p3, len(r3)), sum(len(r) for r in r3)
    return Case("two bad blocks", k, inp.anchors, b, nb, code=1, bad_block=0)


# ---- outside the conforming set, and not refused ----------------------------------------------------------------------------------

def _spots(apos, k):
    """N and listed-error positions of the chosen read, three of each before and three behind the anchor"""
    return ([apos - 18, apos - 11, apos - 5], [apos + k + 4, apos + k + 10, apos + k + 17],
            [apos - 15, apos - 8, apos - 2], [apos + k + 2, apos + k + 7, apos + k + 13])


def _with_n(R, apos, k):
    nb, na, _, _ = _spots(apos, k)
    r = bytearray(R)
    for p in nb + na:
        r[p] = ord("N")
    return bytes(r)


def _dup(at):
    """the list with entry `at` (an index, or a function of the list giving indices) written twice"""
    def f(x):
        idx = at(x) if callable(at) else [at]
        out = []
        for i, v in enumerate(x):
            out.append(v)
            if i in [j % len(x) for j in idx]:
                out.append(v)
        return out
    return f


def _repeats_walked(written, L, apos, k):
    """repeats (an entry equal to the one before it) behind which, in the order of the walk that meets them, a further position of the
    list is walked: right of the anchor a larger entry below len, left of it a smaller one"""
    n = 0
    for i in range(1, len(written)):
        v = written[i]
        if v != written[i - 1] or v >= L:
            continue
        if v >= apos + k and any(v < x < L for x in written):
            n += 1
        if v < apos and any(x < v for x in written):
            n += 1
    return n


def _odd_lists(k):
    """(name, which list, entries(conforming list, len, apos), twin entries or None)"""
    def around(x, L, apos):                               # indices of the middle entry before and of the middle entry behind the anchor
        before = [i for i, v in enumerate(x) if v < apos]
        behind = [i for i, v in enumerate(x) if apos + k <= v < L]
        return [before[len(before) // 2], behind[len(behind) // 2]]

    def behind_repeats(x, L, apos):                       # the same list without what lies behind those two repeats, walk-wise
        i, j = around(x, L, apos)
        return [v for v in _dup(lambda y: [i, j])(x) if x[i] <= v <= x[j]]
    cases = []
    for which in ("n", "err"):
        cases += [
            ("%s-repeat-second" % which, which, lambda x, L, apos: _dup(0)(x), None),
            ("%s-repeat-middle" % which, which, lambda x, L, apos: _dup(len(x) // 2)(x), None),
            ("%s-repeat-last" % which, which, lambda x, L, apos: _dup(-1)(x), None),
            ("%s-repeat-both-sides" % which, which, lambda x, L, apos: _dup(lambda y: around(y, L, apos))(x), behind_repeats if which == "n" else None),
            ("%s-thrice" % which, which, lambda x, L, apos: _dup(lambda y: around(y, L, apos))(_dup(lambda y: around(y, L, apos))(x)), None),
            ("%s-beyond-len" % which, which, lambda x, L, apos: x + [L, L + 5, (1 << 32) - 1], None),
        ]
    cases += [
        ("err-inside-anchor", "err", lambda x, L, apos: sorted(x + [apos + 3]), None),
        ("err-on-an-N", "err", lambda x, L, apos: sorted(x + [_spots(apos, k)[0][1], _spots(apos, k)[1][1]]), None),
    ]
    return cases


K63_ODD = ("n-repeat-both-sides", "err-repeat-both-sides", "err-on-an-N")


@functools.lru_cache(maxsize=None)
def decode_cases(k):
    """lists no conforming writer writes and no decoder refuses: membership decides, so they decode to the reads as written"""
    inp, blocks, nbases = good(k)
    out = []
    for place in PLACES if k == 31 else PLACES[:1]:
        for name, which, entries, twin_entries in _odd_lists(k):
            if k != 31 and name not in K63_ODD:
                continue
            written = {}

            def tamper(L, apos, left, entries=entries):
                def f(x):
                    written["list"] = entries(list(x), L, apos)
                    return written["list"]
                return dict(entries={which: f}, err_at=_spots(apos, k)[2] + _spots(apos, k)[3])
            edit = lambda R, apos: _with_n(R, apos, k)
            payload, reads, t, R, choice, left = write(k, 1, place, tamper, edit=edit)
            b, nb = _call(k, 1, payload, reads)
            c = Case("%s, %s" % (name, place), k, inp.anchors, b, nb, reads=_whole(k, 1, reads), ri=t.read,
                     repeats_walked=_repeats_walked(written["list"], len(R), choice[0], k))
            if twin_entries:
                tw = lambda L, apos, left: dict(entries={which: lambda x: twin_entries(list(x), L, apos)}, err_at=_spots(apos, k)[2] + _spots(apos, k)[3])
                c.twin = _call(k, 1, write(k, 1, place, tw, edit=edit)[0], reads)[0]
            out.append(c)
    # a block of 0 reads and 0 bases with an empty payload, as the first, a middle and the last block of the call
    for at in (0, 2, 4):
        b, nb = list(blocks), list(nbases)
        b.insert(at, (0, b"", 0))
        nb.insert(at, 0)
        b = [(i, p, n) for i, (_, p, n) in enumerate(b)]
        out.append(Case("empty block at %d" % at, k, inp.anchors, b, nb, reads=good_reads(k)))
    return out


# ---- the list pool, conforming ----------------------------------------------------------------------------------------------------

def _gappy_read(rng, n_n, n_clean, k):
    """a scaffold: k + 9 clean bases (its anchor), then runs of N between clean stretches of 4 bases"""
    head = k + 9
    stretches = max((n_clean - head) // 4, 1)
    run = n_n // stretches
    r = bytearray(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=head))
    done = 0
    for s in range(stretches):
        m = run if s < stretches - 1 else n_n - done
        r += b"N" * m
        done += m
        r += bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=4))
    return bytes(r)


@functools.lru_cache(maxsize=None)
def pool_case(name):
    """conforming calls whose N lists need the pool (every list longer than DC_LIST_CAP), anchored by Policy(anchor="given") on a dictionary
    made from their clean heads; bloom and k of base_input(31).  The expected reads are the input's.
      many:   124 reads of about 9 000 bases, 8 500 of them N, 31 to a block.  The lists' total is above 2^20 words, the bases below 2^21:
              more than the pool the call starts with (its 2^20 floor), though no block ever holds more than 8 500 entries at a time.
      growing: 8 blocks of two reads with 70 000 and then 80 000 N.  A block's second list does not fit its first allocation and takes
              min(max(80 000, 2 * 70 000), bases left) >= 80 000 words more: 8 * 150 000 > 2^20, the first pool runs out whichever
              block comes last, and the call is decoded again with the pool no call can exhaust (2 words per base: DESIGN.md 4.5).
    No bound is left to stand at: a conforming call is refused for its lists only when the device has no memory for 8 bytes per base."""
    k = 31
    inp = S.base_input(k)
    rng = np.random.default_rng(17)
    if name == "many":
        reads, rpb = [_gappy_read(rng, 8500, 500, k) for _ in range(124)], 31
    else:
        reads, rpb = [_gappy_read(rng, n, 360, k) for _ in range(8) for n in (70000, 80000)], 2
    anchors = []
    for r in reads:
        x = 0
        for c in r[:k]:
            x = (x << 2) | S._CODE[c]
        anchors.append(x)
    assert len(set(anchors)) == len(anchors)
    given = [(0, i, 0) for i in range(len(reads))]
    blocks, nbases, facts = S.build_blocks(reads, k, rpb, inp.bloom, anchors, random.Random(9), S.Policy(anchor="given", given=given), {})
    assert facts["anchored"] == len(reads)
    c = Case("pool, %s" % name, k, anchors, blocks, nbases, reads=[S.norm(r) for r in reads], oracle=False)
    c.n_lists = [sum(ch == 78 for ch in r) for r in reads]
    c.rpb = rpb
    return c
