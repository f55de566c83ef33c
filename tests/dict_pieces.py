"""Shapes, reference bytes and directed k-mer lists for the anchor dictionary in independently coded pieces.
Pure numpy and the oracle, no GPU.

A piece is P anchors through a fresh 5-symbol model (M_NOANCHOR_READ's, k_anchor_symbols' model id) and a fresh coder with its flush, so
the reference of every piece is oracle_lib.rc_encode_stream on that model over the piece's k * P symbols, symbol j of an anchor being
(kmer >> 2 (k - 1 - j)) & 3.

Random k-mers reach none of the coder's rare paths, so two DIRECTED lists are built with tests/rc_edges.py's hug / strike idea, restricted to
the one model and the values 0..3 a k-mer can hold (_Coder1 is RangeEncoder::encode in python ints):
  resets   k = 3, P = 16.  From some fillers on, the value whose sub-interval holds the multiple X of 2^56 inside the interval is coded
           (the range shrinks, no byte leaves) until that sub-interval is narrower than 2^48: coding it is a range-below-BOTTOM reset.
  strikes  k = 31, P = 4400: pieces of 136 400 symbols.  A piece uses the values 0..2 alone for its first 2^17 and more symbols, X is hugged
           until the range is below total * 2^32, then value 3 (frequency 1 of a total above 2^17) is struck: a range of some 2^31, whose
           ends agree on four bytes -- a step that emits >= 4 bytes with no reset.
What each list holds (RESETS_AT, STRIKES_AT; rare_steps) is certified by the reference alone (oracle_lib.rc_profile_stream) in test_dict_pieces_cpu.py."""
import functools

import numpy as np

import many_blocks as MB
import oracle_lib as O

MODEL_SIZES = MB.MODEL_SIZES
MODEL = 1                                   # M_NOANCHOR_READ: alphabet 5
TOP, BOTTOM, M64 = 1 << 56, 1 << 48, (1 << 64) - 1

KS = (3, 31, 32, 63)
PS = (1, 3, 64, 1024)


def shapes():
    """(k, P, n) of the host twins' and the device calls' tests: n in {0, 1, P - 1, P, P + 1, 5 P + 2} for every k and P"""
    out = []
    for k in KS:
        for P in PS:
            for n in sorted({0, 1, P - 1, P, P + 1, 5 * P + 2}):
                out.append((k, P, n))
    return out


def random_syms(seed, n, k):
    return np.random.default_rng(seed).integers(0, 4, n * k).astype(np.uint8)


def kmers_from_syms(syms, k):
    """n * k symbols (first base first) -> flat uint64 words, kwords(k) per k-mer, low word first"""
    s = np.asarray(syms, dtype=np.uint64).reshape(-1, k)
    n = len(s)
    lo, hi = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for j in range(k):
        if k - 1 - j >= 32:
            hi = (hi << np.uint64(2)) | s[:, j]
        else:
            lo = (lo << np.uint64(2)) | s[:, j]
    if O.kwords(k) == 1:
        return lo
    return np.stack([lo, hi], axis=1).reshape(-1)


def syms_from_kmers(kmers, k):
    """the inverse: symbol j of an anchor is (kmer >> 2 (k - 1 - j)) & 3 (k_anchor_symbols)"""
    w = np.asarray(kmers, dtype=np.uint64).reshape(-1, O.kwords(k))
    cols = []
    for j in range(k):
        bit = 2 * (k - 1 - j)
        cols.append((w[:, bit >> 6] >> np.uint64(bit & 63)) & np.uint64(3))
    return np.stack(cols, axis=1).astype(np.uint8).reshape(-1) if len(w) else np.zeros(0, np.uint8)


def piece_bounds(n, P):
    return [(a, min(a + P, n)) for a in range(0, n, P)]


def ref_piece(syms):
    """the oracle's bytes for one piece's symbols"""
    syms = np.ascontiguousarray(syms, dtype=np.uint8)
    return O.rc_encode_stream(np.full(len(syms), MODEL, dtype=np.uint8), syms, MODEL_SIZES)


def ref_pieces(syms, n, k, P):
    return [ref_piece(syms[a * k:b * k]) for a, b in piece_bounds(n, P)]


def split(stream, piece_off):
    return [bytes(stream[int(piece_off[p]):int(piece_off[p + 1])]) for p in range(len(piece_off) - 1)]


def profile_piece(syms):
    syms = np.ascontiguousarray(syms, dtype=np.uint8)
    return O.rc_profile_stream(np.full(len(syms), MODEL, dtype=np.uint8), syms, MODEL_SIZES)


# ---- the directed lists ------------------------------------------------------------------------------------------------------------
def _renorm(low, rng):
    """RangeEncoder::encode's loop: (low, range, bytes that left, whether the reset fired)"""
    nb, reset = 0, 0
    while True:
        if (low ^ ((low + rng) & M64)) < TOP:
            pass
        elif rng < BOTTOM:
            rng = (-low) & (BOTTOM - 1)
            reset = 1
        else:
            return low, rng, nb, reset
        nb += 1
        rng = (rng << 8) & M64
        low = (low << 8) & M64


class _Coder1:
    """the reference coder on ONE 5-symbol model: low, range, the cumulative counts"""

    def __init__(self, low=0, rng=M64, counts=(1, 1, 1, 1, 1)):
        self.low, self.rng = low, rng
        self.cum = [0]
        for c in counts:
            self.cum.append(self.cum[-1] + int(c))

    def copy(self):
        c = _Coder1.__new__(_Coder1)
        c.low, c.rng, c.cum = self.low, self.rng, list(self.cum)
        return c

    def total(self):
        return self.cum[-1]

    def sub(self, v):
        q = self.rng // self.cum[-1]
        return (self.low + self.cum[v] * q) & M64, q * (self.cum[v + 1] - self.cum[v])

    def outcome(self, v):
        return _renorm(*self.sub(v))[2:]

    def step(self, v):
        self.low, self.rng, nb, reset = _renorm(*self.sub(v))
        for i in range(v + 1, 6):
            self.cum[i] += 1
        return nb, reset

    def straddled(self):
        X = ((self.low >> 56) + 1) << 56
        return X if self.low < X < self.low + self.rng else None

    def holder(self, X, values):
        """(v, width) of the value among `values` whose sub-interval holds X strictly inside, or None"""
        q = self.rng // self.cum[-1]
        for v in values:
            if self.low + self.cum[v] * q < X < self.low + self.cum[v + 1] * q:
                return v, q * (self.cum[v + 1] - self.cum[v])
        return None


def _rare(nb, reset):
    return nb >= 4 or bool(reset)


def _filler(c, rnd, values):
    while True:
        v = int(values[int(rnd.integers(len(values)))])
        if not _rare(*c.outcome(v)):
            c.step(v)
            return v


def _hug(c, values, below):
    """hug X with `values` until the range is below `below`: the values coded on c, or None where X is lost"""
    steps = []
    for _ in range(200):
        if c.rng < below:
            return steps
        X = c.straddled()
        h = c.holder(X, values) if X is not None else None
        if h is None or h[1] < BOTTOM:
            return None
        assert c.step(h[0]) == (0, 0)
        steps.append(h[0])
    return None


def _hug_to_reset(c):
    """hug X with the values 0..3 until the sub-interval that holds it is below 2^48 and code that one: the values, the last one a reset"""
    steps = []
    for _ in range(200):
        X = c.straddled()
        h = c.holder(X, (0, 1, 2, 3)) if X is not None else None
        if h is None:
            return None
        nb, reset = c.step(h[0])
        steps.append(h[0])
        if h[1] < BOTTOM:
            return steps if reset else None
        if nb or reset:
            return None
    return None


def _reset_piece(seed, n_syms, at):
    """one piece's symbols with a reset at step `at` and no other rare step"""
    rnd = np.random.default_rng(seed)
    for _ in range(20000):
        c, syms = _Coder1(), []
        for _ in range(int(rnd.integers(max(at - 40, 0), at + 1))):
            syms.append(_filler(c, rnd, (0, 1, 2, 3)))
        hs = _hug_to_reset(c)
        if hs is None or len(syms) + len(hs) - 1 != at:
            continue
        syms += hs
        while len(syms) < n_syms:
            syms.append(_filler(c, rnd, (0, 1, 2, 3)))
        return syms
    raise RuntimeError("no reset placed at step %d" % at)


def _plain_piece(seed, n_syms):
    rnd, c = np.random.default_rng(seed), _Coder1()
    return [_filler(c, rnd, (0, 1, 2, 3)) for _ in range(n_syms)]


RESETS_K, RESETS_P = 3, 16
RESETS_AT = {1: 30, 2: 30, 3: RESETS_K * RESETS_P - 1, 5: 20}      # piece -> the step of its reset (piece 3: its last step)


@functools.lru_cache(maxsize=1)
def resets():
    """(k, P, n_anchors, syms): 8 pieces of 48 symbols; the pieces of RESETS_AT hold one reset each, at that step"""
    n_syms = RESETS_K * RESETS_P
    syms = []
    for p in range(8):
        syms += _reset_piece(4800 + p, n_syms, RESETS_AT[p]) if p in RESETS_AT else _plain_piece(4800 + p, n_syms)
    a = np.array(syms, dtype=np.uint8)
    a.setflags(write=False)
    return RESETS_K, RESETS_P, 8 * RESETS_P, a


STRIKES_K, STRIKES_P = 31, 4400
STRIKES_AT = {1: 133000, 2: 133000, 3: 135000}                     # piece -> the step of its strike (total = 5 + step > 2^17)
STRIKES_TAIL = 100                                                 # anchors of the last, partial piece


def _strike_piece(seed, n_syms, at):
    for attempt in range(200):
        rnd = np.random.default_rng(seed + 1000 * attempt)
        head = rnd.integers(0, 3, at - 60).astype(np.uint8)          # the values 0..2 alone
        p = profile_piece(head)
        cnt = np.bincount(head, minlength=4)
        c = _Coder1(p.low, p.range, (1 + cnt[0], 1 + cnt[1], 1 + cnt[2], 1, 1))
        syms = head.tolist()
        while len(syms) <= at:
            trial = c.copy()
            hs = _hug(trial, (0, 1, 2), trial.total() << 32)
            if hs is not None and len(syms) + len(hs) == at:
                nb, reset = trial.outcome(3)
                if nb >= 4 and not reset:
                    syms += hs + [3]
                    trial.step(3)
                    while len(syms) < n_syms:
                        syms.append(_filler(trial, rnd, (0, 1, 2, 3)))
                    return syms
            syms.append(_filler(c, rnd, (0, 1, 2)))
    raise RuntimeError("no strike placed at step %d" % at)


@functools.lru_cache(maxsize=1)
def strikes():
    """(k, P, n_anchors, syms): 4 pieces of 136 400 symbols and one of 100 anchors; the pieces of STRIKES_AT hold one step of >= 4 bytes
    with no reset, at that step.  A few seconds: the heads run through the oracle, the rest in python ints."""
    n_syms = STRIKES_K * STRIKES_P
    parts = []
    for p in range(4):
        if p in STRIKES_AT:
            parts.append(np.array(_strike_piece(1700 + p, n_syms, STRIKES_AT[p]), dtype=np.uint8))
        else:
            parts.append(random_syms(1700 + p, STRIKES_P, STRIKES_K))
    parts.append(random_syms(1799, STRIKES_TAIL, STRIKES_K))
    a = np.concatenate(parts)
    a.setflags(write=False)
    return STRIKES_K, STRIKES_P, 4 * STRIKES_P + STRIKES_TAIL, a


DIRECTED = {"resets": resets, "strikes": strikes}


@functools.lru_cache(maxsize=None)
def rare_steps(name):
    """{piece: [(step, bytes, reset)]} of the list's rare steps (>= 4 bytes, or a reset), from the reference's per-step record"""
    k, P, n, syms = DIRECTED[name]()
    out = {}
    for p, (a, b) in enumerate(piece_bounds(n, P)):
        pr = profile_piece(syms[a * k:b * k])
        idx = np.nonzero((pr.n_bytes >= 4) | (pr.reset != 0))[0]
        if len(idx):
            out[p] = [(int(i), int(pr.n_bytes[i]), int(pr.reset[i])) for i in idx]
    return out


# ---- corrupted pieces: what the device's verdict is held to the host's on -----------------------------------------------------------
def corruptions(stream, off):
    """{name: (stream, piece_off)} of a stream of at least four pieces"""
    s = bytearray(stream)
    out = {}
    for p in (0, 2, len(off) - 2):
        f = bytearray(s)
        f[int(off[p]) + 1] ^= 0x5A
        out["flipped byte in piece %d" % p] = (bytes(f), off.copy())
    cut = off.copy()
    cut[2:] -= np.uint64(int(off[2] - off[1]) // 2)                                             # piece 1 loses its second half (the bytes too)
    out["piece 1 cut short"] = (bytes(s[:int(off[1]) + int(off[2] - off[1]) // 2] + s[int(off[2]):]), cut)
    sw = off.copy()
    sw[2] = off[1] + (off[3] - off[2])
    out["pieces 1 and 2 swapped"] = (bytes(s[:int(off[1])] + s[int(off[2]):int(off[3])] + s[int(off[1]):int(off[2])] + s[int(off[3]):]), sw)
    big = off.copy()
    big[2:] += np.uint64(1)                                                                    # piece 1's entry one too large: every later piece begins a byte late
    out["table entry one too large"] = (bytes(s) + b"\0", big)
    return out


def verdict(capi, fn, stream, off, n, k, P):
    """(code, message, out_kmers afterwards)"""
    out = np.full(max(n * O.kwords(k), 1), 0x5EED, dtype=np.uint64)
    try:
        fn(stream, off, n, k, P, out=out)
        return 0, "", out
    except capi.LeonDnaError as e:
        return e.code, str(e), out
