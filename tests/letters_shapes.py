"""Inputs of the letters tests (test_letters_cpu.py, test_gpu_letters.py, test_host_cli_letters.py) and the numpy model of DESIGN.md 4.12
they are checked against -- never the code under test.

For a buffer of bases b[0..n): a RUN is a maximal interval [begin, end) of bytes in 'a'..'z'; an ODD byte is one that, folded to upper
case when it is lower-case, is none of A C G T N (its record: the position and the ORIGINAL byte); the FOLDED buffer holds the upper-case
form where that is one of A C G T N and 'N' elsewhere; RESTORE sets bit 0x20 of every byte in 'A'..'Z' inside a run, then writes every
odd record's byte to its position."""
import numpy as np

TILE = 4096
MAX_GROUPS = 2048          # kernels.h LETTERS_MAX_GROUPS: above that many tiles a workgroup walks more than one
WAVE = 64 * 16             # bytes of a tile that one wave of 64 lanes loads
EDGE_LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097)
BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)
# what a sequence line may hold beside ACGTN: lower-case bases, IUPAC codes in both cases, gaps and stops
ALPHABET = np.frombuffer(b"ACGTNacgtnRYKMSWBDHVrykmswbdhv.-*", dtype=np.uint8)

# what both forms of apply refuse before they touch anything, on a buffer of 64 bytes: (what, the tables and counts, the words)
REFUSALS = [
    ("no runs", dict(runs=None, odd_pos=None, odd_byte=None, n_runs=2), "letters: null argument"),
    ("no positions", dict(runs=None, odd_pos=None, odd_byte=[82], n_odd=1), "letters: null argument"),
    ("no bytes of the positions", dict(runs=None, odd_pos=[3], odd_byte=None, n_odd=1), "letters: null argument"),
    ("empty run", dict(runs=[[4, 4]], odd_pos=None, odd_byte=None), "letters: a run is empty or runs backwards"),
    ("run backwards", dict(runs=[[9, 4]], odd_pos=None, odd_byte=None), "letters: a run is empty or runs backwards"),
    ("run behind the bytes", dict(runs=[[4, 9], [60, 65]], odd_pos=None, odd_byte=None), "letters: a run ends behind the bytes given"),
    ("runs overlap", dict(runs=[[4, 9], [8, 12]], odd_pos=None, odd_byte=None), "letters: the runs overlap or are not ascending"),
    ("runs not ascending", dict(runs=[[20, 24], [4, 9]], odd_pos=None, odd_byte=None), "letters: the runs overlap or are not ascending"),
    ("position behind the bytes", dict(runs=None, odd_pos=[3, 64], odd_byte=[82, 82]), "letters: a position lies behind the bytes given"),
    ("position twice", dict(runs=None, odd_pos=[3, 3], odd_byte=[82, 82]), "letters: the positions are not strictly ascending"),
    ("positions not ascending", dict(runs=None, odd_pos=[9, 3], odd_byte=[82, 82]), "letters: the positions are not strictly ascending"),
]


class Model:
    """the tables and the folded form of a uint8 array, by the rule above"""

    def __init__(self, data):
        b = np.ascontiguousarray(data, dtype=np.uint8)
        low = (b >= ord("a")) & (b <= ord("z"))
        up = np.where(low, b - 32, b).astype(np.uint8)
        base = np.isin(up, BASES)
        step = np.diff(np.concatenate(([0], low.astype(np.int8), [0])))
        self.runs = np.stack([np.flatnonzero(step == 1), np.flatnonzero(step == -1)], axis=1).astype(np.uint64)
        self.odd_pos = np.flatnonzero(~base).astype(np.uint64)
        self.odd_byte = b[~base]
        self.folded = np.where(base, up, ord("N")).astype(np.uint8)
        self.n_runs, self.n_odd = len(self.runs), len(self.odd_pos)


def restore(folded, runs, odd_pos, odd_byte):
    """RESTORE of the rule, on a copy"""
    out = np.array(folded, dtype=np.uint8)
    runs = np.asarray(runs, dtype=np.uint64).reshape(-1, 2)
    step = np.zeros(len(out) + 1, dtype=np.int64)
    np.add.at(step, runs[:, 0].astype(np.int64), 1)
    np.add.at(step, runs[:, 1].astype(np.int64), -1)
    inside = np.cumsum(step[:-1]) > 0
    out[inside & (out >= ord("A")) & (out <= ord("Z"))] |= 0x20
    out[np.asarray(odd_pos, dtype=np.int64)] = odd_byte
    return out


def plain(n, seed):
    return BASES[np.random.default_rng(seed).integers(0, 4, n)].copy()


def lower(data, a, b):
    data[a:b] |= 0x20
    return data


def mixed(n, seed, p_run=0.02, p_odd=0.02):
    """upper-case bases; every position begins or ends a stretch of lower case with probability p_run, and is a byte of ALPHABET's
    second half (IUPAC in the stretch's case, gaps) with probability p_odd"""
    rng = np.random.default_rng(seed)
    data = plain(n, seed)
    in_run = np.cumsum(rng.random(n) < p_run) % 2 == 1
    odd = rng.random(n) < p_odd
    data[odd] = ALPHABET[rng.integers(10, len(ALPHABET), int(odd.sum()))]
    letters = (data >= ord("A")) & (data <= ord("Z"))
    data[in_run & letters] |= 0x20
    data[~in_run & (data >= ord("a")) & (data <= ord("z"))] &= 0xDF
    return data


def all_bytes():
    """every byte value, twice, the second time between lower-case bases"""
    v = np.arange(256, dtype=np.uint8)
    return np.concatenate((v, np.frombuffer(b"acgt", dtype=np.uint8), v, np.frombuffer(b"tgca", dtype=np.uint8)))


def edges(n=3 * TILE + 100):
    """a run at byte 0, one that ends at the last byte; odd bytes in the first and last position and next to one another; lower-case odd
    bytes inside and at both edges of runs"""
    d = plain(n, 11)
    lower(d, 0, 7)
    lower(d, n - 9, n)
    d[0] = ord("r"); d[n - 1] = ord("y")
    d[100:104] = np.frombuffer(b"RY.-", dtype=np.uint8)
    lower(d, 200, 230)
    d[200] = ord("n"); d[215] = ord("r"); d[229] = ord("k"); d[230] = ord("R")
    d[300] = ord("n"); d[301] = ord("N")
    return d


def whole_lower(n=2 * TILE + 33):
    return lower(plain(n, 12), 0, n)


def alternating(n=2 * TILE + 35):
    d = plain(n, 13)
    d[0::2] |= 0x20
    return d


def boundaries(lead, n=6 * TILE + 50):
    """runs at the joins of tiles, waves and lanes.  Tiles are cut at aligned ADDRESSES: with `lead` = the buffer's address mod 16,
    tile i begins at position i * TILE - lead.  Up to MAX_GROUPS tiles every tile is a workgroup's whole range."""
    d = plain(n, 14)
    t = lambda i: i * TILE - lead
    lower(d, t(1) - 40, t(1))                    # ends exactly at a tile boundary
    lower(d, t(2), t(2) + 40)                    # begins exactly at one
    lower(d, t(2) + WAVE - 5, t(2) + WAVE + 5)   # across a wave boundary inside a tile
    lower(d, t(2) + 2 * WAVE + 16 - 3, t(2) + 2 * WAVE + 16 + 3)   # across a lane boundary
    lower(d, t(3) - 1, t(3) + 1)                 # across two workgroups' ranges, one byte either side
    lower(d, t(4) - 10, t(5) + 10)               # covers a whole workgroup's range
    d[t(4) - 1] = ord("r"); d[t(4)] = ord("y"); d[t(5) - 1] = ord("."); d[t(5)] = ord("k")
    lower(d, t(6) - 1, t(6))                     # the last byte of a tile alone
    lower(d, t(6) + 1, t(6) + 2)
    return d


def past_the_grid_cap(lead):
    """more than three times MAX_GROUPS tiles: every workgroup walks `per` consecutive tiles; runs and odd bytes across the joins between
    a workgroup's tiles, across the joins between workgroups, over a workgroup's whole range, and wherever the draw puts them"""
    n = 3 * MAX_GROUPS * TILE + 777
    n_tiles = (lead + n + 1 + TILE - 1) // TILE
    per = (n_tiles + MAX_GROUPS - 1) // MAX_GROUPS
    assert per >= 3
    d = plain(n, 15)
    rng = np.random.default_rng(16)
    t = lambda i: i * TILE - lead
    for g in rng.integers(1, n_tiles // per - 1, 300):
        g = int(g)
        for j in range(per + 1):                 # every join of the workgroup's tiles, the one with the next workgroup included
            at = t(g * per + j)
            lower(d, at - int(rng.integers(0, 30)), at + int(rng.integers(0, 30)))
            if rng.random() < 0.3:
                d[at - 1] = ord("r"); d[at] = ord("-")
    for g in (7, 8, 500):                        # whole ranges, two of them neighbours
        lower(d, t(g * per) - 3, t((g + 1) * per) + (3 if g != 7 else 0))
    for at in rng.integers(0, n - 50, 2000):
        at = int(at)
        lower(d, at, at + int(rng.integers(1, 50)))
    d[rng.integers(0, n, 3000)] = ALPHABET[rng.integers(10, len(ALPHABET), 3000)]
    lower(d, n - 5, n)
    return d, per


HUGE = (1 << 32) + 4097 + 11
HUGE_RUNS = [(5, 9), ((1 << 31) - 3, (1 << 31) + 3), ((1 << 32) - 100, (1 << 32) + 100), (HUGE - 2, HUGE)]
HUGE_ODD = [(0, ord("R")), ((1 << 32) - 50, ord("r")), ((1 << 32) + 150, ord("-")), ((1 << 32) + 151, ord("Y")), ((1 << 32) + 4000, ord("K")), (HUGE - 1, ord("m"))]


def huge():
    """just past 4 GiB of 'A': a run straddling 2^32 and odd bytes behind it: positions that do not fit 32 bits.  The tables and the
    folded form follow from how the buffer is made (the model over 4 GiB of numpy temporaries would not fit a test's seconds):
    (data, runs, odd_pos, odd_byte, the places that differ from 'A' as (position, original byte, folded byte))"""
    d = np.full(HUGE, ord("A"), dtype=np.uint8)
    places = {}
    for a, b in HUGE_RUNS:
        d[a:b] = ord("a")
        for p in range(a, b):
            places[p] = (ord("a"), ord("A"))
    for p, v in HUGE_ODD:
        d[p] = v
        places[p] = (v, ord("N"))
    runs = np.array(HUGE_RUNS, dtype=np.uint64)
    # ('r' and the 'm' at the last position are lower-case and odd: they stay inside their runs)
    pos = np.array([p for p, _ in HUGE_ODD], dtype=np.uint64)
    byte = np.array([v for _, v in HUGE_ODD], dtype=np.uint8)
    return d, runs, pos, byte, sorted((p, o, f) for p, (o, f) in places.items())


def small_shapes(lead=0):
    """(name, data) of everything but the grid-cap and 4 GiB buffers"""
    for n in EDGE_LENGTHS:
        yield "mixed %d" % n, mixed(n, 20 + n, 0.1, 0.1)
    yield "every byte value", all_bytes()
    yield "edges", edges()
    yield "whole buffer lower-case", whole_lower()
    yield "alternating", alternating()
    yield "boundaries", boundaries(lead)
    yield "plain", plain(5000, 17)


def random_draws(count=200, seed=99):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(1, 3 * TILE))
        yield mixed(n, 1000 + i, float(rng.random()) ** 2 if i % 7 else float(i % 2), float(rng.random()) ** 2 if i % 5 else float(i // 5 % 2))
