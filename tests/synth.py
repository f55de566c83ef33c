"""Seeded synthetic read sets modelled on data/toy.fasta's generator fields (er0.01, indel0, rev0/1)."""
import functools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    _COMP[a] = b


def make_genome(length, seed=42):
    rng = np.random.default_rng(seed)
    return _ACGT[rng.integers(0, 4, size=length)]


def make_reads(genome, n_reads, read_len, seed=43, err=0.01, n_rate=0.0, ragged=False):
    """returns (bases uint8[total], offsets uint64[n+1]); reads from both strands with substitutions."""
    rng = np.random.default_rng(seed)
    G = len(genome)
    if ragged:
        lens = rng.integers(max(1, read_len // 4), read_len + 1, size=n_reads)
    else:
        lens = np.full(n_reads, read_len, dtype=np.int64)
    lens = np.minimum(lens, G)
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    starts = (rng.random(n_reads) * (G - lens + 1)).astype(np.int64)
    rid = np.repeat(np.arange(n_reads), lens)
    within = np.arange(total) - np.repeat(off[:-1].astype(np.int64), lens)
    strand = rng.integers(0, 2, size=n_reads).astype(bool)
    fwd_idx = starts[rid] + within
    rev_idx = starts[rid] + (lens[rid] - 1 - within)
    idx = np.where(strand[rid], rev_idx, fwd_idx)
    b = genome[idx]
    b = np.where(strand[rid], _COMP[b], b)
    if err > 0:
        m = rng.random(total) < err
        sub = _ACGT[rng.integers(0, 4, size=total)]
        sub = np.where(sub == b, _ACGT[(np.searchsorted(_ACGT, sub) + 1) % 4], sub)
        b = np.where(m, sub, b)
    if n_rate > 0:
        m = rng.random(total) < n_rate
        b = np.where(m, np.uint8(ord("N")), b)
    return np.ascontiguousarray(b, dtype=np.uint8), off


def read_fasta(path):
    reads = []
    with open(path) as f:
        for line in f:
            if not line.startswith(">"):
                reads.append(line.strip())
    return reads


# ---- inputs with the structure of real genomes and real files ----------------------------------------
# The sets above place reads uniformly at random over an i.i.d. genome, in random order: file-order dependency chains of the
# anchor dictionary are 3-6 reads long there.  Real files are not like that: reads sorted by position (samtools sort | fastq,
# amplicon tilings, many simulators) make EVERY read depend on the one before it; repeats pile many reads on one dictionary key;
# PCR duplicates propose the same anchor again and again.

def make_structured_genome(length, seed=42, dispersed=4, tandem=4):
    """an i.i.d. genome with `dispersed` families of copied segments (0.1-5 kbp, 2-6 copies each, some reverse-complemented)
    and `tandem` microsatellites (a 1-6 bp unit repeated over 40-400 bp) written into it"""
    rng = np.random.default_rng(seed)
    g = _ACGT[rng.integers(0, 4, size=length)].copy()
    for _ in range(dispersed):
        seg = int(min(max(100, length // 8), rng.integers(100, 5001)))
        if seg >= length:
            continue
        src = int(rng.integers(0, length - seg))
        piece = g[src:src + seg].copy()
        for _ in range(int(rng.integers(2, 7))):
            dst = int(rng.integers(0, length - seg))
            g[dst:dst + seg] = _COMP[piece[::-1]] if rng.random() < 0.5 else piece
    for _ in range(tandem):
        unit = _ACGT[rng.integers(0, 4, size=int(rng.integers(1, 7)))]
        span = int(min(max(8, length // 10), rng.integers(40, 401)))
        dst = int(rng.integers(0, max(1, length - span)))
        g[dst:dst + span] = np.tile(unit, span // len(unit) + 1)[:span]
    return g


ORDERS = ("random", "sorted", "pairs", "sorted-strands")


def make_structured_reads(genome, n_reads, read_len, seed=43, order="sorted", err=0.01, n_rate=0.0, ragged=False,
                          dup_rate=0.0, skew=0.0, stride=None):
    """returns (bases uint8[total], offsets uint64[n+1]).
    order: "random" | "sorted" (by start position: what a position-sorted BAM gives back) | "sorted-strands" (sorted, all reads
           forward: tiled amplicons) | "pairs" (mates interleaved: forward read at p, reverse read ~2.2 read lengths downstream).
    dup_rate: that share of the reads are copies of another read's placement (PCR duplicates; errors drawn independently).
    skew: 0 = uniform coverage; > 0 concentrates the starts (a share `skew` of the reads falls into a tenth of the genome).
    stride: reads start every `stride` bases instead of at random places (with order="sorted": a tiling)."""
    assert order in ORDERS
    rng = np.random.default_rng(seed)
    G = len(genome)
    lens = rng.integers(max(1, read_len // 4), read_len + 1, size=n_reads) if ragged else np.full(n_reads, read_len, dtype=np.int64)
    lens = np.minimum(lens, G).astype(np.int64)
    span = np.maximum(G - lens + 1, 1)
    if stride is not None:
        starts = (np.arange(n_reads, dtype=np.int64) * stride) % span
    else:
        u = rng.random(n_reads)
        if skew > 0:
            hot = rng.random(n_reads) < skew
            lo = rng.random() * 0.9
            u = np.where(hot, lo + 0.1 * u, u)
        starts = (u * span).astype(np.int64)
    strand = rng.integers(0, 2, size=n_reads).astype(bool)
    if order == "sorted-strands":
        strand[:] = False
    if order == "pairs":
        half = n_reads // 2
        gap = int(2.2 * read_len)
        starts[1:2 * half:2] = np.minimum(starts[0:2 * half:2] + gap, span[1:2 * half:2] - 1)
        strand[0:2 * half:2] = False
        strand[1:2 * half:2] = True
    if dup_rate > 0:
        dup = np.nonzero(rng.random(n_reads) < dup_rate)[0]
        src = rng.integers(0, n_reads, size=len(dup))
        starts[dup] = np.minimum(starts[src], span[dup] - 1)
        strand[dup] = strand[src]
    if order in ("sorted", "sorted-strands"):
        o = np.argsort(starts, kind="stable")
        starts, strand, lens = starts[o], strand[o], lens[o]
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    rid = np.repeat(np.arange(n_reads), lens)
    within = np.arange(total) - np.repeat(off[:-1].astype(np.int64), lens)
    idx = np.where(strand[rid], starts[rid] + (lens[rid] - 1 - within), starts[rid] + within)
    b = genome[idx]
    b = np.where(strand[rid], _COMP[b], b)
    if err > 0:
        m = rng.random(total) < err
        sub = _ACGT[rng.integers(0, 4, size=total)]
        sub = np.where(sub == b, _ACGT[(np.searchsorted(_ACGT, sub) + 1) % 4], sub)
        b = np.where(m, sub, b)
    if n_rate > 0:
        b = np.where(rng.random(total) < n_rate, np.uint8(ord("N")), b)
    return np.ascontiguousarray(b, dtype=np.uint8), off


# ---- window-scale inputs: millions of reads, any read range regenerated on its own -------------------------------------------------
# The generators above draw every base of the file from one stream: at 2.3 M x 150 bp they take half a minute and 15-20 GB.  window_reads
# draws what places a read (start, strand, length, duplicates, order) from one stream for the whole file -- a few integers per read -- and
# its bases' noise per chunk of WINDOW_CHUNK reads from a stream of that chunk's own, so that reads [r0, r1) come out without the rest and
# equal the same slice of the whole file, whatever the thread count.

WINDOW_CHUNK = 1 << 16
_SUB = np.zeros((256, 3), dtype=np.uint8)            # _SUB[b, r]: the r-th of the three bases other than b
for _b in b"ACGT":
    _SUB[_b] = [x for x in b"ACGT" if x != _b]


def window_genome(g):
    """g: {"kind": "iid" | "structured", "length", "seed"[, "dispersed", "tandem"]}"""
    if g["kind"] == "iid":
        return make_genome(g["length"], seed=g["seed"])
    assert g["kind"] == "structured", g
    return make_structured_genome(g["length"], seed=g["seed"], dispersed=g.get("dispersed", 4), tandem=g.get("tandem", 4))


def window_placement(spec, G):
    """(lens, starts, strand) of every read of the file (int64, int64, bool)"""
    n, L = spec["n_reads"], spec["read_len"]
    rng = np.random.default_rng(spec["seed"])
    lens = rng.integers(max(1, L // 4), L + 1, size=n) if spec.get("ragged") else np.full(n, L, dtype=np.int64)
    lens = np.minimum(lens, G).astype(np.int64)
    span = np.maximum(G - lens + 1, 1)
    u = rng.random(n)
    if spec.get("skew", 0) > 0:
        hot = rng.random(n) < spec["skew"]
        lo = rng.random() * 0.9
        u = np.where(hot, lo + 0.1 * u, u)
    starts = (u * span).astype(np.int64)
    strand = rng.integers(0, 2, size=n).astype(bool)
    order = spec.get("order", "random")
    assert order in ("random", "sorted", "pairs"), order
    if order == "pairs":
        half = n // 2
        gap = int(2.2 * L)
        starts[1:2 * half:2] = np.minimum(starts[0:2 * half:2] + gap, span[1:2 * half:2] - 1)
        strand[0:2 * half:2] = False
        strand[1:2 * half:2] = True
    if spec.get("dup_rate", 0) > 0:
        dup = np.nonzero(rng.random(n) < spec["dup_rate"])[0]
        src = rng.integers(0, n, size=len(dup))
        starts[dup] = np.minimum(starts[src], span[dup] - 1)
        strand[dup] = strand[src]
    if order == "sorted":
        o = np.argsort(starts, kind="stable")
        starts, strand, lens = starts[o], strand[o], lens[o]
    return lens, starts, strand


@functools.lru_cache(maxsize=2)
def _window_placed(spec_json):
    """genome and placement of a spec (as JSON): the read ranges of one file, asked for one by one, share them"""
    spec = json.loads(spec_json)
    genome = window_genome(spec["genome"])
    placed = (genome,) + window_placement(spec, len(genome))
    for a in placed:
        a.setflags(write=False)
    return placed


def _window_chunk(spec, genome, lens, starts, strand, c, out, at):
    """the bases of chunk c (reads [c * WINDOW_CHUNK, ...)) into out[at:]"""
    a, b = c * WINDOW_CHUNK, min(len(lens), (c + 1) * WINDOW_CHUNK)
    G = len(genome)
    w = at
    for s in range(a, b, 8192):                                   # the 2-D gather in slices: a few MB of indices at a time
        e = min(b, s + 8192)
        ln, rv = lens[s:e, None], strand[s:e]
        j = np.arange(int(ln.max()), dtype=np.int32)[None, :]
        # a reverse read walks its span backwards from its last base
        first = np.where(rv, starts[s:e] + lens[s:e] - 1, starts[s:e]).astype(np.int32)[:, None]
        idx = first + np.where(rv, -1, 1).astype(np.int32)[:, None] * j
        if spec.get("ragged"):
            np.clip(idx, 0, G - 1, out=idx)                       # (past a short read's end: cut away below)
        seg = genome[idx]
        seg[rv] = _COMP[seg[rv]]
        seg = seg[j < ln] if spec.get("ragged") else seg.reshape(-1)
        out[w:w + len(seg)] = seg
        w += len(seg)
    err, n_rate = float(spec.get("err", 0)), float(spec.get("n_rate", 0))
    if err > 0 or n_rate > 0:
        # one float32 uniform per base: below err a substitution (which of the three other bases: where in [0, err) it lies), from err to
        # err + n_rate an N
        u = np.random.default_rng([spec["seed"], c]).random(w - at, dtype=np.float32)
        seg = out[at:w]
        if err > 0:
            m = np.nonzero(u < err)[0]
            seg[m] = _SUB[seg[m], np.minimum((u[m] * np.float32(3.0 / err)).astype(np.int64), 2)]
        seg[(u >= err) & (u < err + n_rate)] = ord("N")


def window_reads(spec, r0=0, r1=None, threads=None):
    """reads [r0, r1) of the file `spec` describes: (bases uint8[total], offsets uint64[r1 - r0 + 1], offsets[0] = 0).
    spec: {"genome": {...} (window_genome), "n_reads", "read_len", "seed", "ragged", "order": "random" | "sorted" | "pairs", "err",
    "n_rate", "dup_rate", "skew"}; "pairs" interleaves mates (forward read at p, reverse read ~2.2 read lengths downstream)."""
    n = spec["n_reads"]
    r1 = n if r1 is None else r1
    assert 0 <= r0 <= r1 <= n
    genome, lens, starts, strand = _window_placed(json.dumps(spec, sort_keys=True))
    assert len(genome) < 1 << 31                                    # (int32 indices)
    c0, c1 = r0 // WINDOW_CHUNK, (r1 + WINDOW_CHUNK - 1) // WINDOW_CHUNK
    a, b = c0 * WINDOW_CHUNK, min(n, c1 * WINDOW_CHUNK)             # whole chunks, cut to [r0, r1) at the end
    off = np.zeros(b - a + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens[a:b])
    out = np.empty(int(off[-1]), dtype=np.uint8)
    if threads is None:
        threads = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
    threads = max(1, min(threads, c1 - c0))
    jobs = [(c, int(off[c * WINDOW_CHUNK - a])) for c in range(c0, c1)]
    if threads == 1:
        for c, at in jobs:
            _window_chunk(spec, genome, lens, starts, strand, c, out, at)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda j: _window_chunk(spec, genome, lens, starts, strand, j[0], out, j[1]), jobs))
    o0, o1 = int(off[r0 - a]), int(off[r1 - a])
    return out[o0:o1], (off[r0 - a:r1 - a + 1] - off[r0 - a]).astype(np.uint64)
