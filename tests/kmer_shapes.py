"""Inputs of the solid k-mer counter's tests (test_kmer_counter_cpu.py, test_gpu_kmer_counter.py) and their reference: a count in plain
Python that is neither the library nor the oracle.  Every input is seeded, so both tests see the same bytes; reads are a tuple of bytes."""
import functools

import numpy as np

CODE = {65: 0, 67: 1, 84: 2, 71: 3}                # A C T G, the product's code; the complement is ^ 2
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

PART_CHUNK = 1024                                  # kmer_kernels.hip PART_CHUNK: the slots a wave of k_part_kmers claims at a time
PACK_MAP = 4096                                    # dna_kernels.hip PACK_MAP: up to that many slots of 32 bases k_pack maps a workgroup's reads in LDS
THRESHOLDS = (1, 2, 3, 254, 255, 256, 257, 258, 700, 701)
EXACT_ABUNDANCES = (1, 2, 3, 254, 255, 256, 257, 700)
UNITS_PER_ABUNDANCE = 3
LONG_K = (15, 31, 32, 63)
EXACT_K = (21, 47)
TINY_K = (3, 4)


# ---- the reference ----
@functools.lru_cache(maxsize=None)
def ref_counts(reads, k):
    """{canonical k-mer as int (first base in the highest bits): occurrences}; a k-mer with a byte outside ACGT in it is none"""
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    counts = {}
    for r in reads:
        fwd = rc = valid = 0
        for b in r:
            c = CODE.get(b)
            if c is None:
                fwd = rc = valid = 0
                continue
            fwd = ((fwd << 2) | c) & mask
            rc = (rc >> 2) | ((c ^ 2) << top)
            valid += 1
            if valid >= k:
                m = fwd if fwd < rc else rc
                counts[m] = counts.get(m, 0) + 1
    return counts


def ref_hist(counts):
    """distinct k-mers by abundance, 256 bins, 255 and more in the last"""
    h = np.zeros(256, dtype=np.uint64)
    for c in counts.values():
        h[min(c, 255)] += 1
    return h


def ref_cutoff(hist):
    """the automatic threshold: the first a, 1 <= a < last non-empty bin, at which the spectrum stops falling (hist[a + 1] >= hist[a]);
    never below 2, and 2 when there is none"""
    last = max([a for a in range(1, 256) if hist[a]], default=0)
    for a in range(1, last):
        if hist[a + 1] >= hist[a]:
            return max(a, 2)
    return 2


# ---- k-mer sets as sorted (n, words) uint64 arrays, low word first: what the library and the oracle return, once sorted ----
def kwords(k):
    return 2 if k >= 32 else 1


def words_of(kmers, k):
    """python ints -> sorted rows"""
    s = sorted(kmers)
    a = np.zeros((len(s), kwords(k)), dtype=np.uint64)
    a[:, 0] = [x & 0xFFFFFFFFFFFFFFFF for x in s]
    if kwords(k) == 2:
        a[:, 1] = [x >> 64 for x in s]
    return a


def sorted_words(flat, k):
    """a flat result (kwords(k) words per k-mer, any order) -> sorted rows"""
    a = np.asarray(flat, dtype=np.uint64).reshape(-1, kwords(k))
    return a[np.lexsort((a[:, 0], a[:, -1]))]


def ref_solid(reads, k, min_abundance):
    return words_of([m for m, c in ref_counts(reads, k).items() if c >= min_abundance], k)


def arrays(reads):
    """(bases as bytes, offsets as uint64[n + 1])"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return b"".join(reads), off


def total_positions(reads, k):
    return sum(len(r) - k + 1 for r in reads if len(r) >= k)


def keys_per_pass(reads, k, parts):
    """the max_keys_per_pass at which the counter makes `parts` hash partitions of these reads (it takes ceil(positions / max_keys_per_pass))"""
    total = total_positions(reads, k)
    per = -(-total // parts)
    assert -(-total // per) == parts, (total, parts)
    return per


# ---- the inputs ----
def random_bases(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def revcomp(seq):
    return seq.translate(_COMP)[::-1]


@functools.lru_cache(maxsize=None)
def long_reads(k):
    """7 reads of 20 000 bases cut from one 40 000-base genome, so that k-mers repeat (three of them taken from the other strand); in each
    about 60 N -- at the edges of the 32-base mask words, three in a row, the rest anywhere -- and over all of them four bytes in lower
    case or 'R'; between them reads of exactly k, k - 1, 0 and 4 bases.  One wave of k_part_kmers walks each long read: 19 chunks and more
    of one partition.  Together they have more than PACK_MAP 32-base slots, so k_pack finds a slot's read by bisection."""
    rng = np.random.default_rng(4100 + k)
    genome = random_bases(rng, 40000)
    long = []
    for i, start in enumerate((0, 7001, 13337, 20000, 9999, 16384, 3500)):
        r = bytearray(genome[start:start + 20000])
        if i & 1:
            r = bytearray(revcomp(bytes(r)))
        at = [31, 32, 63, 64, 95, 96, 1023, 1024, 5000, 5001, 5002, 19999 - 7 * i] + [int(x) for x in rng.integers(0, 20000, 48)]
        for p in at:
            r[p] = ord("N")
        long.append(r)
    long[0][100] = ord("a")
    long[0][7000] = ord("g")
    long[2][12345] = ord("R")
    long[4][33] = ord("R")
    long = [bytes(r) for r in long]
    return (long[0], genome[100:100 + k], long[1], b"", long[2], genome[300:300 + k - 1], long[3], genome[500:504], long[4], long[5], long[6])


def _from_spectrum(spectrum, k, seed):
    """reads of exactly k bases: for every (abundance, units) that many random units, each its own read repeated abundance times, on
    either strand, all shuffled.  One read is one k-mer, so the spectrum is known by construction (random units of 21 bases and more do
    not meet; the CPU test checks it)."""
    rng = np.random.default_rng(seed)
    reads = []
    for abundance, units in spectrum:
        for _ in range(units):
            u = random_bases(rng, k)
            reads += [revcomp(u) if rng.integers(0, 2) else u for _ in range(abundance)]
    return tuple(reads[i] for i in rng.permutation(len(reads)))


EXACT_SPECTRUM = tuple((a, UNITS_PER_ABUNDANCE) for a in EXACT_ABUNDANCES)
VALLEY_SPECTRUM = tuple((a, 41 - a) for a in range(1, 41)) + ((41, 5), (60, 3), (300, 2))          # stops falling at 40
NO_VALLEY_SPECTRUM = tuple((a, 30 - a) for a in range(1, 30))                                       # falls all the way: 2


def spectrum_hist(spectrum):
    h = np.zeros(256, dtype=np.uint64)
    for abundance, units in spectrum:
        h[min(abundance, 255)] += units
    return h


@functools.lru_cache(maxsize=None)
def exact_abundances(k):
    """about 5 200 reads: three each in bins 1, 2, 3 and 254, twelve in bin 255"""
    return _from_spectrum(EXACT_SPECTRUM, k, 4200 + k)


@functools.lru_cache(maxsize=None)
def valley(k):
    """about 12 500 reads whose spectrum has its first local minimum at 40; the two units of abundance 300 are kept through a clipped count"""
    return _from_spectrum(VALLEY_SPECTRUM, k, 4300 + k)


@functools.lru_cache(maxsize=None)
def no_valley(k):
    return _from_spectrum(NO_VALLEY_SPECTRUM, k, 4400 + k)


@functools.lru_cache(maxsize=None)
def tiny_k(k):
    """4 000 reads of 100 random bases for k = 3 or 4: every one of the 32 or 136 canonical k-mers, about 12 000 times each at k = 3 and
    1 500 (the 16 palindromes, which have one strand) or 3 000 times at k = 4: all in bin 255, every run far into k_flag_runs' doubling
    search.  (400 reads would leave the palindromes of k = 4 near 150, below the clip.)"""
    rng = np.random.default_rng(4500 + k)
    return tuple(random_bases(rng, 100) for _ in range(4000))


def all_inputs():
    """(name, reads, k) of every input above"""
    for k in LONG_K:
        yield "long_reads(%d)" % k, long_reads(k), k
    for k in EXACT_K:
        yield "exact_abundances(%d)" % k, exact_abundances(k), k
        yield "valley(%d)" % k, valley(k), k
        yield "no_valley(%d)" % k, no_valley(k), k
    for k in TINY_K:
        yield "tiny_k(%d)" % k, tiny_k(k), k
