"""Inputs of the lossy quality smoothing's tests (test_qual_smooth_cpu.py, test_gpu_qual_smooth.py): a case is a k, a bloom geometry,
the canonical k-mers in the bloom, reads and quality lines.  The expected bytes are always oracle_lib.qual_smooth's over an
oracle_lib.Bloom -- never the library under test.  Where a case is DESIGNED, the k-mer positions that are solid are chosen here and the
positions with coverage >= 2 follow from them by counting (covered_twice); test_qual_smooth_cpu.py certifies, from the oracle alone, that
the bloom gives exactly those.

Coverage: a solid k-mer at position p covers the bases p .. p + k - 1; a quality becomes '@' where two or more solid
k-mers cover its base, or where it is above '@'; reads shorter than k stay as they are; N is read as A."""
import numpy as np

import oracle_lib as O

GEOMETRIES = [(7, 12), (7, 4), (7, 16), (1, 6), (3, 9), (10, 14)]       # (n_hash, block_nbits); the kernels are built for 7 hashes, any other count is a run-time loop
DESIGNED_K = [21, 31, 32, 33, 63]                                        # one-word k-mers, the last of them, the first two-word ones, the largest
DESIGNED_TAI = 200000
WAVE_GRID_READS = 4096 * 4                                               # hdr_kernels.hip wave_grid: 4 096 workgroups of 4 waves, a read per wave and trip
THREAD_GRID = 8192 * 256                                                 # k_iota, k_mpos_from_anchors: 8 192 workgroups of 256 threads

_CODE = np.zeros(256, dtype=np.uint8)                                    # A = 0, C = 1, T = 2, G = 3; N and everything else is read as A
for _c, _v in ((b"C", 1), (b"T", 2), (b"G", 3)):
    _CODE[_c[0]] = _v
_LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)


def canonical_kmers(read, k):
    """the canonical k-mer (python int) at every k-mer position of `read` (bytes), N read as A"""
    mask, top, x, r, out = (1 << (2 * k)) - 1, 2 * (k - 1), 0, 0, []
    for i, c in enumerate(_CODE[np.frombuffer(bytes(read), dtype=np.uint8)].tolist()):
        x = ((x << 2) | c) & mask
        r = (r >> 2) | ((c ^ 2) << top)
        if i + 1 >= k:
            out.append(min(x, r))
    return out


def kmer_words(ints, k):
    """python ints -> the flat uint64 array oracle_lib.Bloom.insert and DnaEncodeContext.bloom_insert take"""
    w = O.kwords(k)
    a = np.zeros((len(ints), w), dtype=np.uint64)
    for i, x in enumerate(ints):
        a[i, 0] = x & 0xFFFFFFFFFFFFFFFF
        if w == 2:
            a[i, 1] = x >> 64
    return a.reshape(-1)


def covered_twice(solid_positions, length, k):
    """the base positions that two or more of the solid k-mer positions cover"""
    cover = np.zeros(length + 1, dtype=np.int64)
    for p in solid_positions:
        cover[p] += 1
        cover[p + k] -= 1
    return np.flatnonzero(np.cumsum(cover)[:length] >= 2)


def random_read(rng, length):
    return _LETTERS[rng.integers(0, 4, length)].tobytes()


def revcomp(read):
    return bytes(b"TGCA"[b"ACGT".index(c)] if c in b"ACGT" else c for c in reversed(read))


def quality_lines(lengths, seed):
    """one line per read, four kinds in turn: all 256 byte values in rotation; only '?', '@', 'A' (the rule's `> '@'` is an unsigned
    compare, and these sit either side of it); '@' throughout (nothing left to do); printable values either side of '@'"""
    rng = np.random.default_rng(seed)
    edge = np.frombuffer(b"?@A", dtype=np.uint8)
    out = []
    for i, n in enumerate(lengths):
        kind = i % 4
        if kind == 0:
            q = ((np.arange(n) + 37 * i) % 256).astype(np.uint8)
        elif kind == 1:
            q = edge[rng.integers(0, 3, n)]
        elif kind == 2:
            q = np.full(n, ord("@"), dtype=np.uint8)
        else:
            q = rng.integers(33, 75, n).astype(np.uint8)
        out.append(q)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


class Case:
    """bases / quals: uint8 arrays, off: uint64[n + 1]; solid: the bloom's canonical k-mers (python ints); designed: None, or per read the
    positions its coverage is >= 2 by design; check: the reads the rule can touch (None = every read of length >= k)"""

    def __init__(self, name, k, geometry, tai, solid, bases, off, quals, designed=None, check=None):
        self.name, self.k, self.geometry, self.tai = name, k, geometry, int(tai)
        self.solid = sorted(set(solid))
        self.bases, self.off, self.quals = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64), quals
        self.designed, self.check = designed, check
        self.n = len(self.off) - 1
        assert len(self.bases) == len(self.quals) == int(self.off[-1]) and int(self.off[0]) == 0

    def lengths(self):
        return np.diff(self.off.astype(np.int64))

    def read(self, i):
        return self.bases[int(self.off[i]):int(self.off[i + 1])].tobytes()

    def touched(self):
        return np.flatnonzero(self.lengths() >= self.k) if self.check is None else np.asarray(self.check)

    def bloom(self):
        bl = O.Bloom(self.tai, self.k, *self.geometry)
        if self.solid:
            bl.insert(kmer_words(self.solid, self.k))
        return bl

    def with_reads(self, name, reads, seed):
        """other reads against the same bloom"""
        return from_reads(name, self.k, self.geometry, self.tai, self.solid, reads, seed)


def from_reads(name, k, geometry, tai, solid, reads, seed, design=False):
    bases, off = O.reads_to_arrays(reads)
    quals = quality_lines([len(r) for r in reads], seed)
    designed = None
    if design:                                                          # what follows from the k-mers put in: a position is solid iff its k-mer was inserted
        inside = set(solid)
        designed = [covered_twice([p for p, c in enumerate(canonical_kmers(r, k)) if c in inside], len(r), k) if len(r) >= k
                    else np.zeros(0, dtype=np.int64) for r in reads]
    return Case(name, k, geometry, tai if tai else max(12 * len(set(solid)), 1000), solid, np.frombuffer(bases, dtype=np.uint8), off, quals, designed)


_expected = {}


def expected(case):
    """the oracle's bytes for the case, computed once (the tests share it and leave it as it is)"""
    if case.name not in _expected:
        bl = case.bloom()
        want = case.quals.copy()
        for i in case.touched():
            s, e = int(case.off[i]), int(case.off[i + 1])
            want[s:e] = np.frombuffer(O.qual_smooth(bl, case.k, case.bases[s:e].tobytes(), case.quals[s:e].tobytes()), dtype=np.uint8)
        want.setflags(write=False)
        _expected[case.name] = want
    return _expected[case.name]


def oracle_coverage(bl, k, read):
    """positions with coverage >= 2 as the oracle sees them: qualities of '!' that came back '@'"""
    return np.flatnonzero(np.frombuffer(O.qual_smooth(bl, k, read, b"!" * len(read)), dtype=np.uint8) == ord("@"))


def first_difference(case, got, want):
    """(read, position, got byte, want byte) of the first byte that differs"""
    at = int(np.flatnonzero(np.asarray(got) != np.asarray(want))[0])
    i = int(np.searchsorted(case.off, at, side="right")) - 1
    return "read %d (length %d) position %d: got 0x%02x, the oracle 0x%02x" % (i, int(case.off[i + 1] - case.off[i]), at - int(case.off[i]),
                                                                                 int(got[at]), int(want[at]))


# ---- 1. designed flags ----
PAIR_STARTS = (30, 31, 62, 63, 64, 127)          # adjacent pairs (a, a + 1) either side of the flag words' joins (31/32, 63/64, 127/128) and the ballots' (63/64)


def read_lengths(k):
    return sorted(set([k, k + 1, k + 31, k + 32, k + 63, k + 64, k + 65, 2 * k, 127, 128, 129, 191 + k]))


def solid_sets(k, length, rng):
    """(what, solid k-mer positions) for a read of `length`"""
    nk = length - k + 1
    sets = [("none", []), ("one", [int(rng.integers(0, nk))]), ("all", list(range(nk)))]
    if nk >= 2:
        sets += [("pair 0", [0, 1]), ("pair last", [nk - 2, nk - 1])]
        sets += [("pair %d" % a, [a, a + 1]) for a in PAIR_STARTS if a + 1 < nk]
    if nk >= k:
        a = int(rng.integers(0, nk - k + 1))
        sets.append(("k - 1 apart", [a, a + k - 1]))                 # coverage 2 on exactly one base, a + k - 1
    if nk >= k + 1:
        a = int(rng.integers(0, nk - k))
        sets.append(("k apart", [a, a + k]))                         # they do not meet
    return sets


def _designed_reads(k, lean, seed):
    rng = np.random.default_rng(seed)
    reads, solid, what = [], [], []
    for length in read_lengths(k):
        for name, pos in solid_sets(k, length, rng):
            if lean and (name == "all" and length > k + 1 or length != 191 + k and name not in ("one", "pair 0", "pair last", "all")):
                continue
            r = random_read(rng, length)
            if rng.integers(0, 2):                                   # either strand's k-mer may be the canonical one: random reads have both
                r = revcomp(r)
            c = canonical_kmers(r, k)
            solid += [c[p] for p in pos]
            reads.append(r)
            what.append("%s, length %d" % (name, length))
    while len(reads) < 300:                                          # nothing of theirs is in the bloom; some shorter than k, some empty: enough reads for the ordered routes
        reads.append(random_read(rng, int(rng.integers(0, 200)) if len(reads) % 5 else 0))
        what.append("nothing inserted")
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], solid, [what[i] for i in order]


def _first_exact_draw(name, k, geometry, draw):
    """draw(attempt) -> (reads, solid, what): the first draw in which the oracle's coverage is the designed one (a chance hit of the bloom
    beside a designed k-mer makes a draw unusable).  test_qual_smooth_cpu.py checks the outcome independently."""
    for attempt in range(40):
        reads, solid, what = draw(attempt)
        case = from_reads(name, k, geometry, DESIGNED_TAI, solid, reads, seed=k + geometry[1], design=True)
        bl = case.bloom()
        if all(np.array_equal(oracle_coverage(bl, k, r), d) for r, d in zip(reads, case.designed) if len(r) >= k):
            case.what = what                                         # per read, what was put in for it
            return case
    raise AssertionError("no draw of %s has exactly its designed coverage" % name)


def designed_case(k, geometry):
    """With one hash function a bloom of 200 000 bits answers yes to a k-mer that was never put in once in a few thousand times, so that
    geometry gets fewer inserted k-mers (`lean`)."""
    n_hash, nbits = geometry
    return _first_exact_draw("designed-k%d-h%d-b%d" % (k, n_hash, nbits), k, geometry,
                             lambda attempt: _designed_reads(k, n_hash < 3, 1000 * k + 10 * nbits + n_hash + 100000 * attempt))


def _every_length(k, seed):
    rng = np.random.default_rng(seed)
    reads, solid, what = [], [], []
    for length in range(k, k + 66):
        nk = length - k + 1
        for name, pos in (("all", list(range(nk))), ("pair 0", [0, 1]), ("pair last", [nk - 2, nk - 1]), ("first and last", [0, nk - 1])):
            if nk == 1 and name != "all":
                continue
            r = random_read(rng, length)
            c = canonical_kmers(r, k)
            solid += [c[p] for p in pos]
            reads.append(r)
            what.append("%s, length %d" % (name, length))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], solid, [what[i] for i in order]


def lengths_case(k):
    """every read length from k to k + 65 -- 1 to 66 k-mer positions: a lane past the last k-mer, a second step of 64 with one or two
    positions in it -- with every k-mer solid, the first two, the last two, and the first and the last"""
    return _first_exact_draw("lengths-k%d-to-k+65" % k, k, (7, 12), lambda attempt: _every_length(k, 50 * k + 100000 * attempt))


# ---- 2. N handling ----
def n_case(k, poly_a):
    rng = np.random.default_rng(77 + k + poly_a)
    reads, solid = [], [0] if poly_a else []                         # the poly-A k-mer is 0, and canonical (its reverse complement is poly-T)
    for n_at in ([40], [k + 5, k + 6], [36, 37, 38], [35], [35 + k], [50, 60, 64]):    # a designed pair at (35, 36); the N lie in both k-mers, or in one, at its end
        r = bytearray(random_read(rng, 150))
        for p in n_at:
            r[p] = ord("N")
        reads.append(bytes(r))
        c = canonical_kmers(reads[-1], k)                            # with A in the N's place
        solid += [c[35], c[36]]
    reads += [b"N" * k, b"N" * (k + 1), b"N" * 100, b"N" * 200, b"N" * (k - 1)]
    if k == 32:                                                      # ACGT x 8 is its own reverse complement; every fourth k-mer of ACGT x n is that one
        reads += [b"ACGT" * 8, b"ACGT" * 16, b"ACGT" * 8 + random_read(rng, 70), random_read(rng, 33) + b"ACGT" * 9]
        solid += canonical_kmers(b"ACGT" * 8, k)
    while len(reads) < 280:
        r = bytearray(random_read(rng, int(rng.integers(k - 3, 180))))
        for p in rng.integers(0, len(r), int(rng.integers(0, 4))):
            r[p] = ord("N")
        reads.append(bytes(r))
    order = rng.permutation(len(reads))
    return from_reads("n-k%d-%s" % (k, "polyA" if poly_a else "plain"), k, (7, 12), DESIGNED_TAI, solid, [reads[i] for i in order], seed=5 + k, design=True)


# ---- 3. dense random cases ----
def small_k_case(k, geometry):
    """few distinct k-mers: chance hits are the rule, the coverage is whatever it is"""
    rng = np.random.default_rng(300 + k)
    reads = [random_read(rng, int(rng.integers(0, 90))) for _ in range(400)]
    seen = sorted(set(c for r in reads for c in canonical_kmers(r, k)))
    solid = [c for c in seen if rng.random() < 0.4]
    return from_reads("small-k%d-h%d-b%d" % (k, geometry[0], geometry[1]), k, geometry, 0, solid, reads, seed=k)


def _genome_solid(genome, k, rng, spots):
    """the genome's k-mers but those over `spots` random bases and a random tenth: stretches without coverage, and k-mers alone"""
    c = canonical_kmers(genome, k)
    keep = rng.random(len(c)) >= 0.1
    for s in rng.integers(0, len(genome), spots):
        keep[max(int(s) - k + 1, 0):int(s) + 1] = False
    return [x for x, y in zip(c, keep) if y]


def genome_case(k, length, geometry):
    """a genome of 3 000 bases read at every offset, on both strands: the minimizer falls on the first and the last k-mer position and on
    either strand, and many reads share one; reads shorter than k and empty ones in between"""
    rng = np.random.default_rng(500 + k)
    genome = random_read(rng, 3000)
    reads = []
    for at in range(len(genome) - length + 1):
        r = genome[at:at + length]
        reads += [r, revcomp(r)]
        if at % 97 == 0:
            reads += [b"", random_read(rng, k - 1), genome[at:at + k]]
    return from_reads("genome-k%d" % k, k, geometry, 0, _genome_solid(genome, k, rng, 25), reads, seed=k)


# ---- 5. counts ----
def _sampled_reads(genome, n, lo, hi, rng, err=0.02):
    out = []
    for _ in range(n):
        length = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, len(genome) - length + 1))
        r = bytearray(genome[at:at + length])
        for p in np.flatnonzero(rng.random(length) < err):
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        out.append(bytes(r) if rng.integers(0, 2) else revcomp(bytes(r)))
    return out


COUNTS = [1, 255, 256, 257, WAVE_GRID_READS + 5]                     # the ordered routes begin at 256 reads; read 16 385 is a wave's second trip


def count_case(n):
    k = 21
    rng = np.random.default_rng(900)
    genome = random_read(rng, 2000)
    solid = _genome_solid(genome, k, rng, 10)
    rng = np.random.default_rng(901 + n)
    return from_reads("count-%d" % n, k, (7, 12), 0, solid, _sampled_reads(genome, n, 30, 60, rng), seed=n)


HUGE_N = THREAD_GRID + 300
HUGE_FRONT = 150


def huge_case():
    """2^21 + 300 reads, all of 8 bases (shorter than k: the rule leaves them) but 150 at the front and 150 behind index 2^21 -- those are
    a thread's second trip in k_iota, and the 129th trip of a wave in k_read_minimizer and k_qual_rewrite.  Arrays throughout."""
    k, long_len = 31, 100
    rng = np.random.default_rng(2100)
    genome = random_read(rng, 2000)
    solid = _genome_solid(genome, k, rng, 10)
    lengths = np.full(HUGE_N, 8, dtype=np.uint64)
    long_ones = np.concatenate((np.arange(HUGE_FRONT), np.arange(HUGE_N - 150, HUGE_N)))
    lengths[long_ones] = long_len
    off = np.zeros(HUGE_N + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    bases = _LETTERS[rng.integers(0, 4, int(off[-1]))]
    for i, r in zip(long_ones, _sampled_reads(genome, len(long_ones), long_len, long_len, rng)):
        bases[int(off[i]):int(off[i + 1])] = np.frombuffer(r, dtype=np.uint8)
    quals = rng.integers(0, 256, int(off[-1])).astype(np.uint8)
    return Case("count-%d" % HUGE_N, k, (7, 12), max(12 * len(set(solid)), 1000), solid, bases, off, quals, check=long_ones)


# ---- 6. one long read ----
def long_read_case():
    k = 31
    rng = np.random.default_rng(7000)
    genome = random_read(rng, 70000)
    solid = canonical_kmers(genome, k)
    r = bytearray(genome)
    for p in np.flatnonzero(rng.random(len(r)) < 0.005):
        r[p] = b"ACGT"[int(rng.integers(0, 4))]
    for p in np.flatnonzero(rng.random(len(r)) < 0.001):
        r[p] = ord("N")
    reads = _sampled_reads(genome, 300, 80, 150, rng)
    reads.insert(123, bytes(r))
    return from_reads("long-read-70000", k, (7, 12), 0, solid, reads, seed=70)


# ---- stale anchors ----
def stale_pair():
    """A, B: as many reads, of other lengths, against the same bloom; B has reads shorter than k, reads with room for a k-mer or two only (so
    shorter than where A's reads of that index have their anchor), and fewer bases in all than A"""
    k = 31
    rng = np.random.default_rng(4100)
    genome = random_read(rng, 4000)
    solid = _genome_solid(genome, k, rng, 10)
    a = from_reads("stale-A", k, (7, 12), 0, solid, _sampled_reads(genome, 1200, 100, 100, rng, err=0.01), seed=41)
    reads = []
    for i in range(a.n):
        lo, hi = ((0, k - 1), (k, k + 2), (k + 3, 99), (60, 99))[i % 4]
        reads += _sampled_reads(genome, 1, lo, hi, rng)
    return a, a.with_reads("stale-B", reads, seed=42)


# ---- the list ----
_BUILDERS = {}
for _k in DESIGNED_K:
    for _g in GEOMETRIES:
        _BUILDERS["designed-k%d-h%d-b%d" % (_k, _g[0], _g[1])] = (designed_case, (_k, _g))
for _k in DESIGNED_K:
    _BUILDERS["lengths-k%d-to-k+65" % _k] = (lengths_case, (_k,))
for _k in (31, 32):
    for _p in (False, True):
        _BUILDERS["n-k%d-%s" % (_k, "polyA" if _p else "plain")] = (n_case, (_k, _p))
for _k, _g in ((3, (7, 12)), (5, (3, 9)), (11, (7, 4))):
    _BUILDERS["small-k%d-h%d-b%d" % (_k, _g[0], _g[1])] = (small_k_case, (_k, _g))
_BUILDERS["genome-k31"] = (genome_case, (31, 100, (7, 12)))
_BUILDERS["genome-k47"] = (genome_case, (47, 120, (10, 14)))
for _n in COUNTS:
    _BUILDERS["count-%d" % _n] = (count_case, (_n,))
_BUILDERS["long-read-70000"] = (long_read_case, ())
HUGE = "count-%d" % HUGE_N
_BUILDERS[HUGE] = (huge_case, ())

NAMES = list(_BUILDERS)
DESIGNED = [n for n in NAMES if n.startswith(("designed-", "lengths-", "n-"))]
RANDOM = [n for n in NAMES if n not in DESIGNED and n != HUGE]
_cases = {}


def case(name):
    """the case of that name, built once"""
    if name not in _cases:
        f, args = _BUILDERS[name]
        _cases[name] = f(*args)
        assert _cases[name].name == name
    return _cases[name]
