"""A policy-driven writer of DNA read blocks (test support, no GPU): streams a conforming encoder MAY write and ours never does.

The format leaves a writer several freedoms -- which dictionary k-mer anchors a read, which delta type
codes a value, how many bytes a numeric takes, which walked positions are listed as errors, whether a read is anchored at all --
and the project's encoders make one choice at each.  `build_block` makes the others, by `Policy`, as (model, symbol) pairs coded
with the oracle's raw range coder.  The walk is tests/py_leon.py's.  The writer never leaves the conforming set: both position
lists strictly ascending, every entry below the read's length, every error entry on a walked position, no position in both."""
import functools
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence

import numpy as np

import common
import oracle_lib as O
import synth

# model ids of leon_device.h
M_TYPE, M_NOANCHOR, M_BIF, M_BIN, M_SIZE_DT, M_POS_DT, M_ADDR_DT, M_REV = range(8)
G_ADDR, G_POS, G_NASIZE, G_SIZE, G_NPOS, G_ERRPOS, G_NUM, G_NERR = range(8)
SIZES = [2, 5, 5, 2, 3, 3, 3, 2] + [256] * 72
N_NUMERIC_MODELS = 72
_CODE = {65: 0, 67: 1, 84: 2, 71: 3}                     # A C T G; anything else is an N


def group_model(g, idx=0):
    return 8 + 9 * g + idx


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | ((x & 3) ^ 2)
        x >>= 2
    return r


def norm(read):
    """what a decoder gives back: any non-ACGT byte is an N in the format"""
    return bytes(c if c in b"ACGT" else 78 for c in read)


def words(anchors, k):
    """python-int k-mers -> the flat uint64 array decoders take (kwords(k) words each, low word first)"""
    if not anchors:
        return np.zeros(0, dtype=np.uint64)
    return np.concatenate([O.kmer_words(a, k) for a in anchors])


@dataclass
class Policy:
    anchor: str = "first"                                # first | last | random | over_n | given
    given: Optional[Sequence] = None                     # anchor == "given": per read (pos, address, rev) or None (no anchor)
    noanchor: float = 0.0                                # probability of coding a read without its anchor
    free_delta: bool = False                             # any delta type that reproduces the value
    pad: bool = False                                    # numerics of minimal..8 bytes
    extra_err: float = 0.0                               # probability of listing a walked position nothing forces
    err_at: Optional[Callable] = None                    # (len, apos, k) -> positions to list by design


@dataclass
class Tamper:
    """tests/dna_bad_streams.py's hook: what one chosen read of a block is written with INSTEAD of what the writer would write.  Every
    callable gets the conforming value(s) and returns what goes into the stream; nothing here is looked at when `tamper` is None."""
    read: int                                            # index of the read in the block
    fields: dict = field(default_factory=dict)           # "size" | "pos" | "addr" | "nasize" -> f(value, prev) = (delta type, coded number, bytes or None)
    entries: dict = field(default_factory=dict)          # "n" | "err" -> f(conforming list) = the entries as written (coded as differences)
    count: dict = field(default_factory=dict)            # "n" | "err" -> f(len of the written list, read length) = the declared size
    err_at: Sequence = ()                                # walked positions of this read to list as errors by design
    cut: Optional[str] = None                            # the symbol list ends behind: "fields" (size, pos, addr) | "nasize" | "n_count" | "err_count"
    syms: Optional[list] = None                          # out: the block's (model, symbol) list as coded ...
    bad_at: Optional[int] = None                         # ... and the index of the chosen read's first symbol


def _minimal_bytes(v):
    bc = 1
    while bc < 8 and (v >> (8 * bc)):
        bc += 1
    return bc


def delta_rule(value, prev):
    """SymSink::delta: the type the project's encoders pick"""
    if value > prev and value - prev < value:
        return 1
    if value <= prev and prev - value < value:
        return 2
    return 0


def new_facts():
    return dict(reads=0, anchored=0, noanchor=0, anchored_over_n=0, off_first=0, models=set(), models_most_in_a_block=0,
                longest_err_list=0, n_err=0, err_unique=0, err_dead=0, err_before_anchor=0, err_after_anchor=0, err_at_0=0,
                err_at_end=0, selfrc_flag0=0, selfrc_flag1=0, delta_off_rule=[0, 0, 0], len_eq_k=0)


def merge_facts(total, f):
    for key, v in f.items():
        if key == "models":
            total["models"] |= v
            total["models_most_in_a_block"] = max(total["models_most_in_a_block"], len(v))
        elif key == "models_most_in_a_block":
            pass
        elif key == "longest_err_list":
            total[key] = max(total[key], v)
        elif key == "delta_off_rule":
            total[key] = [a + b for a, b in zip(total[key], v)]
        else:
            total[key] += v
    return total


def candidates(seq, k, index):
    """every (pos, address, rev) whose dictionary k-mer, as it is (rev 0) or reverse-complemented (rev 1), is the read's k-mer at pos
    (N read as A), in ascending order; index: k-mer -> its addresses"""
    out = []
    L = len(seq)
    if L < k:
        return out
    mask = (1 << (2 * k)) - 1
    fw = rc = 0
    for i, c in enumerate(seq):
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((c ^ 2) << (2 * (k - 1)))
        if i + 1 >= k:
            pos = i + 1 - k
            for a in index.get(fw, ()):
                out.append((pos, a, 0))
            for a in index.get(rc, ()):
                out.append((pos, a, 1))
    return out


def build_block(reads, k, bloom, anchors, rnd, policy, probe_cache=None, tamper=None):
    """reads: list of bytes; bloom: oracle_lib.Bloom; anchors: python-int k-mers (the dictionary, any order); rnd: random.Random.
    Returns (payload, facts).  probe_cache: a dict shared between calls with the same bloom (its answers are a function of the k-mer).
    tamper: a Tamper, for streams that leave the conforming set on purpose (None: the payload is what it always was)."""
    index = {}
    for a, x in enumerate(anchors):
        index.setdefault(x, []).append(a)
    if probe_cache is None:
        probe_cache = {}
    mask = (1 << (2 * k)) - 1
    syms = []
    facts = new_facts()

    def contains4(km, right):
        key = (km << 1) | right
        r = probe_cache.get(key)
        if r is None:
            r = probe_cache[key] = bloom.contains4(km, right)
        return r

    def numeric(g, v, forced=None):
        bc = _minimal_bytes(v)
        if policy.pad:
            bc = rnd.randint(bc, 8)
        if forced is not None:
            bc = forced
        syms.append((group_model(g), bc))
        facts["models"].add(group_model(g))
        for i in range(bc):
            syms.append((group_model(g, 1 + i), (v >> (8 * i)) & 255))
            facts["models"].add(group_model(g, 1 + i))

    def delta(mt, g, value, prev, forced=None):
        if forced is not None:                               # (delta type, coded number, bytes)
            syms.append((mt, forced[0]))
            numeric(g, forced[1], forced[2])
            return
        rule = delta_rule(value, prev)
        t = rule
        if policy.free_delta:
            t = rnd.choice([0] + ([1] if value >= prev else []) + ([2] if value <= prev else []))
        if t != rule:
            facts["delta_off_rule"][t] += 1
        syms.append((mt, t))
        numeric(g, value if t == 0 else (value - prev if t == 1 else prev - value))

    prev_size = prev_pos = prev_addr = 0
    for ri, read in enumerate(reads):
        L = len(read)
        seq = [_CODE.get(c, 0) for c in read]
        npos = [i for i, c in enumerate(read) if c not in _CODE]
        nset = set(npos)
        facts["reads"] += 1
        tam = tamper if tamper is not None and tamper.read == ri else None
        if tam:
            tam.bad_at = len(syms)
        if policy.anchor == "given":
            choice = policy.given[ri]
            cands = [choice] if choice is not None else []
        else:
            cands = candidates(seq, k, index)
            choice = None
            if cands and not (policy.noanchor and rnd.random() < policy.noanchor):
                if policy.anchor == "first":
                    choice = cands[0]
                elif policy.anchor == "last":
                    choice = cands[-1]
                elif policy.anchor == "random":
                    choice = rnd.choice(cands)
                elif policy.anchor == "over_n":
                    over = [c for c in cands if any(c[0] <= p < c[0] + k for p in npos)]
                    choice = rnd.choice(over) if over else cands[0]
                else:
                    raise ValueError(policy.anchor)
        if choice is None:                                   # a read without an anchor: its letters, one by one
            facts["noanchor"] += 1
            syms.append((M_TYPE, 1))
            if tam and "nasize" in tam.fields:
                f = tam.fields["nasize"](L, 0)
                numeric(G_NASIZE, f[1], f[2])
            else:
                numeric(G_NASIZE, L)
            if tam and tam.cut == "nasize":
                break
            syms.extend((M_NOANCHOR, _CODE.get(c, 4)) for c in read)
            continue
        apos, addr, rev = choice
        facts["anchored"] += 1
        if choice != cands[0]:
            facts["off_first"] += 1
        if any(apos <= p < apos + k for p in npos):
            facts["anchored_over_n"] += 1
        if L == k:
            facts["len_eq_k"] += 1
        anchor = anchors[addr]
        if revcomp(anchor, k) == anchor:
            facts["selfrc_flag1" if rev else "selfrc_flag0"] += 1
        if rev:
            anchor = revcomp(anchor, k)
        here = 0
        for c in seq[apos:apos + k]:
            here = (here << 2) | c
        assert 0 <= apos <= L - k and here == anchor, "not an anchor of this read"
        syms.append((M_TYPE, 0))
        forced = {name: f(value, prev) for name, f in tam.fields.items() for value, prev in
                  [dict(size=(L, prev_size), pos=(apos, prev_pos), addr=(addr, prev_addr)).get(name, (0, 0))]} if tam else {}
        delta(M_SIZE_DT, G_SIZE, L, prev_size, forced.get("size")); prev_size = L
        delta(M_POS_DT, G_POS, apos, prev_pos, forced.get("pos")); prev_pos = apos
        delta(M_ADDR_DT, G_ADDR, addr, prev_addr, forced.get("addr")); prev_addr = addr
        if tam and tam.cut == "fields":
            break
        syms.append((M_REV, rev))
        wanted = set(policy.err_at(L, apos, k)) if policy.err_at else set()
        if tam:
            wanted |= set(tam.err_at)
        bifs, errs = [], []
        for right in (0, 1):
            km = anchor
            for pos in (range(apos + k, L) if right else range(apos - 1, -1, -1)):
                nt = follow = seq[pos]
                if pos not in nset:
                    res4 = contains4(km, right)
                    solid = [x for x in range(4) if res4 >> x & 1]
                    forced = bool(solid) and nt not in solid     # the format requires this one
                    if forced or pos in wanted or (policy.extra_err and rnd.random() < policy.extra_err):
                        errs.append(pos)
                        bifs.append((M_BIF, nt))
                        follow = solid[0] if solid else nt
                        facts["err_unique"] += solid == [nt]
                        facts["err_dead"] += not solid
                        facts["err_before_anchor"] += pos == apos - 1
                        facts["err_after_anchor"] += pos == apos + k
                        facts["err_at_0"] += pos == 0
                        facts["err_at_end"] += pos == L - 1
                    elif len(solid) == 2:
                        bifs.append((M_BIN, 0 if solid[0] == nt else 1))
                    elif len(solid) != 1:
                        bifs.append((M_BIF, nt))
                km = (((km << 2) | follow) & mask) if right else ((km >> 2) | (follow << (2 * (k - 1))))
        errs.sort()
        assert len(set(errs)) == len(errs) and not nset & set(errs), "left the conforming set"
        assert all(0 <= p < L and not apos <= p < apos + k for p in errs), "left the conforming set"
        facts["n_err"] += len(errs)
        facts["longest_err_list"] = max(facts["longest_err_list"], len(errs))
        n_written = tam.entries["n"](npos) if tam and "n" in tam.entries else npos
        numeric(G_NUM, tam.count["n"](len(n_written), L) if tam and "n" in tam.count else len(n_written))
        if tam and tam.cut == "n_count":
            break
        p = 0
        for x in n_written:
            numeric(G_NPOS, x - p); p = x
        e_written = tam.entries["err"](errs) if tam and "err" in tam.entries else errs
        numeric(G_NERR, tam.count["err"](len(e_written), L) if tam and "err" in tam.count else len(e_written))
        if tam and tam.cut == "err_count":
            break
        p = 0
        for x in e_written:
            numeric(G_ERRPOS, x - p); p = x
        syms.extend(bifs)
    if tamper is not None:
        tamper.syms = list(syms)
    a = np.array(syms, dtype=np.uint8).reshape(-1, 2)
    facts["models_most_in_a_block"] = len(facts["models"])
    return O.rc_encode_stream(a[:, 0], a[:, 1], SIZES), facts


def build_blocks(reads, k, rpb, bloom, anchors, rnd, policy, probe_cache=None):
    """all blocks of a read set: ([(block id, payload, n reads)], bases per block, facts over all blocks)"""
    blocks, nbases, facts = [], [], new_facts()
    for b, r0 in enumerate(range(0, len(reads), rpb)):
        part = reads[r0:r0 + rpb]
        pol = policy
        if policy.anchor == "given":
            pol = Policy(**{**policy.__dict__, "given": policy.given[r0:r0 + rpb]})
        payload, f = build_block(part, k, bloom, anchors, rnd, pol, probe_cache)
        blocks.append((b, payload, len(part)))
        nbases.append(sum(len(r) for r in part))
        merge_facts(facts, f)
    return blocks, nbases, facts


# ---- the policies and what each must actually hold ---------------------------------------------------------------------------

def _edges(L, apos, k):
    return (0, L - 1, apos - 1, apos + k)


POLICIES = {
    "base": Policy(),
    "last": Policy(anchor="last"),
    "free": Policy(anchor="random", free_delta=True),
    "pad": Policy(pad=True, noanchor=0.05),
    "over_n": Policy(anchor="over_n"),
    "extra": Policy(anchor="random", extra_err=0.1),
    "all_err": Policy(extra_err=1.0),
    "mixed": Policy(noanchor=0.3, pad=True, free_delta=True, extra_err=0.03, anchor="random"),
    "edges": Policy(err_at=_edges),
}


def check_facts(name, f):
    """the condition a policy's streams must meet for its test to stand on something (conditions on the inputs, not on a decoder)"""
    assert f["anchored"] > 0, f
    if name == "last":
        assert f["off_first"] > 0, f
    elif name == "free":
        assert all(x > 0 for x in f["delta_off_rule"]), f
    elif name == "pad":
        assert f["models_most_in_a_block"] == N_NUMERIC_MODELS, f       # 58 of them beyond the decoder's LDS slots
        assert f["noanchor"] > 0, f
    elif name == "over_n":
        assert f["anchored_over_n"] >= 20, f
    elif name == "extra":
        assert f["err_unique"] > 0 and f["err_dead"] > 0, f
    elif name == "all_err":
        assert f["longest_err_list"] > 64, f
    elif name == "edges":
        assert min(f["err_at_0"], f["err_at_end"], f["err_before_anchor"], f["err_after_anchor"]) > 0, f


# ---- inputs shared by the CPU and the GPU test ---------------------------------------------------------------------------------

def split_reads(bases, off):
    return [bytes(bases[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def make_dictionary(reads, k, encoder_anchors, seed):
    """the oracle encoder's anchors, shuffled; 50 random k-mers nothing uses; the reverse complements of 40 of the anchors under
    further addresses (the same k-mer reachable as flag 0 and as flag 1: not a canonical dictionary); for every read with an N the
    k-mer (N as A) that covers its first N"""
    rng = np.random.default_rng(seed)
    d = list(encoder_anchors)
    rng.shuffle(d)
    d = [int(x) for x in d]
    for _ in range(50):
        d.append(int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * k)) - 1))
    for i in rng.choice(len(encoder_anchors), size=min(40, len(encoder_anchors)), replace=False):
        d.append(revcomp(int(encoder_anchors[int(i)]), k))
    have = set(d)
    for r in reads:
        ns = [i for i, c in enumerate(r) if c not in _CODE]
        if ns and len(r) >= k:
            p = min(max(ns[0] - k // 2, 0), len(r) - k)
            x = 0
            for c in r[p:p + k]:
                x = (x << 2) | _CODE.get(c, 0)
            if x not in have:
                have.add(x)
                d.append(x)
    order = rng.permutation(len(d))
    return [d[int(i)] for i in order]


class Input:
    """reads, bloom, dictionary and the probe cache the writer shares between the policies of one input"""


@functools.lru_cache(maxsize=None)
def base_input(k, n_reads=400):
    kw = dict(bloom_n_hash=3, bloom_block_nbits=9) if k == 21 else {}
    bases, off = common.synthetic(n_reads, 150 if k < 32 else 230, 3000, seed=7 + k, err=0.02, n_rate=0.01, ragged=True)
    inp = Input()
    inp.k, inp.rpb, inp.bloom_kw = k, 100, kw
    inp.bloom, _, inp.tai = common.make_bloom(bases, off, k, n_hash=kw.get("bloom_n_hash", 7), block_nbits=kw.get("bloom_block_nbits", 12))
    inp.reads = split_reads(bases, off)
    ref = O.encode(bases, off, k, inp.rpb, inp.bloom, trace=False)
    inp.anchors = make_dictionary(inp.reads, k, O.kmers_to_ints(ref.anchor_kmers, k), seed=100 + k)
    inp.cache = {}
    return inp


def only_anchor_reads(inp, n=60):
    """the first reads of an input with five reads among them that are one dictionary k-mer and nothing else (len == k: no walk)"""
    lone = []
    for x in inp.anchors[:5]:
        lone.append(bytes(b"ACTG"[(x >> (2 * (inp.k - 1 - i))) & 3] for i in range(inp.k)))
    reads = list(inp.reads[:n])
    for i, r in enumerate(lone):
        reads.insert(7 + 9 * i, r)
    return reads


@functools.lru_cache(maxsize=None)
def long_list_input():
    """one 20 000-base read among 300 of 200 bases, bloom at abundance 2: with every walked position listed its error list
    (19 969 entries) leaves a block's own scratch (8 192) behind"""
    k = 31
    g = synth.make_genome(30000, seed=5)
    b1, _ = synth.make_reads(g, 1, 20000, seed=6, err=0.0)
    b2, off2 = synth.make_reads(g, 300, 200, seed=7, err=0.01)
    short = split_reads(b2, off2)
    inp = Input()
    inp.k, inp.bloom_kw, inp.cache = k, {}, {}
    inp.short, inp.long = short, b1.tobytes()
    bases, off = O.reads_to_arrays(short[:150] + [inp.long] + short[150:])
    inp.bloom, _, inp.tai = common.make_bloom(bases, off, k, min_abundance=2)
    ref = O.encode(bases, off, k, 1000, inp.bloom, trace=False)
    inp.anchors = O.kmers_to_ints(ref.anchor_kmers, k)
    return inp


def selfrc_input():
    """k = 32: reads built around s + revcomp(s), |s| = 16 -- a k-mer that is its own reverse complement, in the dictionary; each read
    is coded once with flag 0 and once with flag 1 (both name the same k-mer)"""
    k = 32
    rng = np.random.default_rng(11)
    comp = {65: 84, 84: 65, 67: 71, 71: 67}
    reads, kmers = [], []
    for i in range(6):
        s = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=16))
        pal = s + bytes(comp[c] for c in reversed(s))
        left = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(0, 40))))
        right = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(0, 40))))
        reads.append(left + pal + right)
        x = 0
        for c in pal:
            x = (x << 2) | _CODE[c]
        assert revcomp(x, k) == x
        kmers.append((len(left), x))
    reads = reads * 3                                             # thrice each: their k-mers are solid at abundance 3
    bases, off = O.reads_to_arrays(reads)
    inp = Input()
    inp.k, inp.bloom_kw, inp.cache = k, {}, {}
    inp.bloom, _, inp.tai = common.make_bloom(bases, off, k)
    inp.anchors = [x for _, x in kmers]
    inp.reads = reads + reads                                     # first half flag 0, second half flag 1
    n = len(reads)
    inp.given = [(kmers[i % 6][0], i % 6, 0) for i in range(n)] + [(kmers[i % 6][0], i % 6, 1) for i in range(n)]
    return inp
