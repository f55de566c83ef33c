"""Seeded, directed (model, value) streams for DnaEncodeContext.rc_encode_streams that reach the range coder's rare paths on purpose:
steps that emit four bytes or more while no range-below-BOTTOM reset fires (k_rc_encode's `xh == 0` branch), resets on demand, model
totals of 2^17, 2^20 and just below 2^22 (the host chains' 22-bit records and reciprocal table), and pairs of streams whose rare steps
fall on the same and on different step indices.  Random symbols reach none of these (tests/many_blocks.py's 2.2 M symbols: no step of
four bytes without a reset, no total above 785).

The streams are built by driving a copy of the reference coder's state (_Coder: RangeEncoder::encode in python ints; the long pumps run
in the oracle, lo_rc_profile_stream, which hands back low and range):
  pump    one value repeated on one model takes its total to a target;
  hug     while a multiple X of 2^56 lies strictly inside the interval, code the (model, value) whose sub-interval still holds X and is
          the narrowest one of at least 2^48: the range shrinks and no byte leaves -- until the range is below a wanted bound;
  strike  then a rare value (frequency 1 of a total of 2^17 or more) of the pumped model: a range of some 2^31 away from X, whose ends
          agree on four bytes.  A sub-interval narrower than 2^48 that holds X is a reset instead.
Filler symbols before the hug place the strike: after every filler a COPY of the state is hugged and struck, and the first placement
that lands on the wanted index or tile lane with the wanted outcome is kept.  What a stream must hold is stated in CENSUS below and
certified by the reference alone in tests/test_rc_edges_cpu.py; tests/test_gpu_rc_edges.py runs the streams through the three coders.
Pure numpy and the oracle, no GPU."""
import bisect
import collections
import functools

import numpy as np

import many_blocks as MB
import oracle_lib as O

MODEL_SIZES = MB.MODEL_SIZES
N_SMALL = MB.N_SMALL
N_MODELS = len(MODEL_SIZES)
TOP, BOTTOM, M64 = 1 << 56, 1 << 48, (1 << 64) - 1

PACK22_HOST_LEN = (1 << 22) - 1025        # the longest stream leon_rc_encode_streams / rc_on_host still give to the host chains (rc_kernels.hip)
PACK22_DEVICE_LEN = PACK22_HOST_LEN + 1
LANES = (0, 1, 62, 63)                    # index % 64: a tile's first records, and the clamp of rc_coder_tile's two-ahead prefetch `jn`

NAMES = ("strike17", "strike20", "strike20_small", "resets", "resets5", "pack22_host", "pack22_device", "pair_a", "pair_b")
# every stream but the two pack22 ones stays at or below this (so the small model pumped to 2^20 has a stream of its own, strike20_small)
MAX_LEN = (1 << 20) + (1 << 15)

PM = 8 + 9 * 2 + 1                          # the pumped numeric model
PM_SMALL = 0                                # ... and the small one (size 2: its total is read from Lw[size])

# What the census (tests/test_rc_edges_cpu.py) holds every stream to.  "big" is a step that emits >= 4 bytes with no reset.
#   big / resets: at least so many such steps; big_total: the pumped model's total at those steps; lanes: one such step at each of these
#   index % 64; last: the stream's last step is one; reset5 / reset6: resets that emit 5 / 6 bytes; pm: the pumped model (PM where not given).
# The resets' byte counts, as reached: the hugging rule places resets at will (any sub-interval below 2^48 that holds X), but such a reset
# emits 1 byte and one more for every whole byte by which d = X - (the sub-interval's lower end) stays short of 2^48: 5 bytes take
# d < 2^16, 6 bytes d < 2^8.  A lower end is low + cumLow * floor(range / total) with a range of 2^48 or more and a total below 2^22, so the
# lower ends of all 80 models lie 2^26 and more apart: one state in some 2^18 has one within 2^16 of X, and the rule has no handle on it.
# The one place where d is small by construction is a stream's beginning: the first range is 2^64 - 1, so value v of a fresh 256-symbol
# model leaves low = v * 2^56 - v, d = v -- a 6-byte reset when the next sub-interval (2^48 - 1 wide) begins there; a step in between that
# emits one byte takes d to (v + u) * 256, a 5-byte reset (every 5- and 6-byte reset of the many_blocks streams is of this kind, among a
# stream's first steps).  After either reset the state is a clean multiple of 2^48 and the construction does not repeat.  So a stream
# holds ONE such reset: `resets` the 6-byte one (its second step), and a short stream of its own, `resets5`, the 5-byte one (its third step).
CENSUS = {
    "strike17": dict(big=32, big_total=1 << 17, lanes=LANES, last="big"),
    "strike20": dict(big=32, big_total=1 << 20),
    "strike20_small": dict(pm=PM_SMALL, big=4, big_total=1 << 20),
    "resets": dict(resets=64, reset6=1, reset_lanes=(0, 63), last="reset"),
    "resets5": dict(resets=8, reset5=1, last="reset"),
    "pack22_host": dict(big=8, big_total=(1 << 22) - 4096, length=PACK22_HOST_LEN, tail=2000),
    "pack22_device": dict(big=8, big_total=(1 << 22) - 4096, length=PACK22_DEVICE_LEN, tail=2001),
    "pair_a": dict(big=8, big_total=1 << 17),
    "pair_b": dict(big=8, big_total=1 << 17),
}
PAIR_SHARED = PAIR_ONLY = 4               # step indices where both of pair_a / pair_b have a rare step (>= 4 bytes, or a reset); where one alone has


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


class _Coder:
    """the reference coder's state: low, range, and every model's cumulative counts (Order0Model's _charRanges)"""

    def __init__(self):
        self.low, self.rng = 0, M64
        self.cum = [list(range(n + 1)) for n in MODEL_SIZES]

    def copy(self):
        c = _Coder.__new__(_Coder)
        c.low, c.rng = self.low, self.rng
        c.cum = [list(x) for x in self.cum]
        return c

    def total(self, m):
        return self.cum[m][-1]

    def sub(self, m, v):
        cu = self.cum[m]
        q = self.rng // cu[-1]
        return (self.low + cu[v] * q) & M64, q * (cu[v + 1] - cu[v])

    def outcome(self, m, v):
        """(bytes, reset) of coding v on m, the state left alone"""
        return _renorm(*self.sub(m, v))[2:]

    def step(self, m, v):
        self.low, self.rng, nb, reset = _renorm(*self.sub(m, v))
        cu = self.cum[m]
        for i in range(v + 1, len(cu)):
            cu[i] += 1
        return nb, reset

    def straddled(self):
        """the multiple of 2^56 strictly inside the interval, or None"""
        X = ((self.low >> 56) + 1) << 56
        return X if self.low < X < self.low + self.rng else None

    def holder(self, m, X):
        """(v, width): the value of model m whose sub-interval holds X strictly inside, or None"""
        cu = self.cum[m]
        q = self.rng // cu[-1]
        if q == 0:
            return None
        idx = (X - self.low) // q
        if idx >= cu[-1]:
            return None
        v = bisect.bisect_right(cu, idx) - 1
        if self.low + cu[v] * q < X < self.low + cu[v + 1] * q:
            return v, q * (cu[v + 1] - cu[v])
        return None


def _hug(c, models, below):
    """hug the straddled multiple of 2^56 until the range is below `below`: the steps taken on c, or None where the straddle is lost"""
    steps = []
    while True:
        X = c.straddled()
        if X is None:
            return None
        if c.rng < below:
            return steps
        best = None
        for m in models:
            h = c.holder(m, X)
            if h is not None and BOTTOM <= h[1] < c.rng and (best is None or h[1] < best[0]):
                best = (h[1], m, h[0])
        if best is None:
            return None
        nb, reset = c.step(best[1], best[2])
        assert nb == 0 and not reset
        steps.append((best[1], best[2]))


def _is_big(nb, reset):
    return nb >= 4 and not reset


def _is_reset(nb, reset):
    return bool(reset)


def _is_rare(nb, reset):
    return nb >= 4 or bool(reset)


class _Builder:
    def __init__(self, seed, pumped, steer=None):
        self.rnd = np.random.default_rng(seed)
        self.c = _Coder()
        self.chunks, self.tail = [], []
        self.n = 0
        self.pumped = list(pumped)
        self.steer = steer if steer is not None else [m for m in range(N_MODELS) if m not in self.pumped]
        self.events = []                                           # (index, bytes, reset) of the placed strikes and resets

    def _flush(self):
        if self.tail:
            a = np.array(self.tail, dtype=np.uint8).reshape(-1, 2)
            self.chunks.append((a[:, 0].copy(), a[:, 1].copy()))
            self.tail = []

    def arrays(self):
        self._flush()
        if not self.chunks:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        return np.concatenate([c[0] for c in self.chunks]), np.concatenate([c[1] for c in self.chunks])

    def pump(self, m, v, count):
        """count times v on m; the state is stale until sync()"""
        self._flush()
        self.chunks.append((np.full(count, m, dtype=np.uint8), np.full(count, v, dtype=np.uint8)))
        self.n += count

    def sync(self):
        """the state after everything so far, from the oracle"""
        m, v = self.arrays()
        p = O.rc_profile_stream(m, v, MODEL_SIZES)
        self.c.low, self.c.rng = p.low, p.range
        cnt = np.bincount(m.astype(np.int64) * 256 + v, minlength=N_MODELS * 256).reshape(N_MODELS, 256)
        for i, n in enumerate(MODEL_SIZES):
            self.c.cum[i] = [0] + np.cumsum(cnt[i, :n] + 1).tolist()

    def put(self, m, v):
        st = self.c.step(m, v)
        self.tail += [m, v]
        self.n += 1
        return st

    def filler(self):
        """one symbol of a steering model; not a rare step (another draw where it would be one)"""
        while True:
            m = int(self.steer[int(self.rnd.integers(len(self.steer)))])
            n = MODEL_SIZES[m]
            v = int(self.rnd.integers(n)) if len(self.steer) > 1 else (0, n - 1)[int(self.rnd.integers(2))]
            if not _is_rare(*self.c.outcome(m, v)):
                self.put(m, v)
                return

    def _strike_values(self, pm):
        if MODEL_SIZES[pm] == 2:
            return [(pm, 1)]
        v0 = int(self.rnd.integers(1, 255))
        return [(pm, 1 + (v0 + i) % 254) for i in range(0, 254, 5)]           # (never the last value: pack22's second pumped value)

    def _reset_values(self, trial, X, pm):
        out = []
        for m in ([pm] if pm is not None else []) + self.steer:
            h = trial.holder(m, X)
            if h is not None and h[1] < BOTTOM:
                out.append((m, h[0]))
        return out

    def place(self, pm, want, below, at=None, lane=None, gap=0, reset=False, limit=4000):
        """fillers until a hug and a strike (reset: a sub-interval that holds X) on pm land on index `at` / lane `lane` with outcome `want`;
        for an index, fillers that run past it are taken back and drawn again"""
        for _ in range(gap):
            self.filler()
        snap = (self.c.copy(), len(self.tail), self.n)
        for _ in range(limit):
            trial = self.c.copy()
            hs = _hug(trial, self.steer, below)
            if hs is not None:
                idx = self.n + len(hs)
                if (at is None or idx == at) and (lane is None or idx % 64 == lane):
                    cands = self._reset_values(trial, trial.straddled(), pm) if reset else self._strike_values(pm)
                    for m, v in cands:
                        if want(*trial.outcome(m, v)):
                            for s in hs:
                                self.put(*s)
                            nb, rs = self.put(m, v)
                            self.events.append((idx, nb, rs))
                            return idx
            if at is not None and self.n >= at:
                self.c, self.n = snap[0].copy(), snap[2]
                del self.tail[snap[1]:]
                continue
            self.filler()
        raise RuntimeError("no placement at index %r / lane %r" % (at, lane))


def _strike_stream(seed, pm, log2_total, n_free, lanes=()):
    b = _Builder(seed, [pm])
    b.pump(pm, 0, 1 << log2_total)
    b.sync()
    for ln in lanes:
        b.place(pm, _is_big, b.c.total(pm) << 32, lane=ln, gap=8)
    for _ in range(n_free):
        b.place(pm, _is_big, b.c.total(pm) << 32, gap=int(b.rnd.integers(4, 40)))
    return b                                                  # (the last strike is the stream's last symbol)


def _resets5_stream(seed):
    b = _Builder(seed, [])
    # low = 2 * (2^56 - 1); a sub-interval of 2^48 - 1 across a multiple of 2^48 (one byte leaves, low is 5 * 256 below a multiple of
    # 2^56); then a sub-interval of 2^48 - 1 that begins there: the reset emits 5 bytes.  Then a dozen resets as they come.
    b.put(N_SMALL + 1, 2)
    b.put(N_SMALL + 2, 3)
    assert b.put(N_SMALL + 3, 0) == (5, 1)
    for _ in range(12):
        b.place(None, _is_reset, TOP, gap=int(b.rnd.integers(4, 24)), reset=True)
    return b


def _resets_stream(seed):
    b = _Builder(seed, [PM])
    # the stream's first two steps: low = 3 * (2^56 - 1), range 2^56 - 1, then a sub-interval of 2^48 - 1 that begins 3 below 3 * 2^56
    b.put(N_SMALL + 1, 3)
    assert b.put(N_SMALL + 2, 0) == (6, 1)
    b.pump(PM, 0, 1 << 17)
    b.sync()
    for ln in (0, 63):
        b.place(PM, _is_reset, TOP, lane=ln, gap=8, reset=True)
    for _ in range(70):
        b.place(PM, _is_reset, TOP, gap=int(b.rnd.integers(4, 24)), reset=True)
    return b                                                  # (the last reset is the stream's last symbol)


def _pack22(seed):
    n = PACK22_HOST_LEN
    b = _Builder(seed, [PM], steer=[PM])                      # one model: the hug halves the range with value 0 or 255
    half = n // 2
    b.pump(PM, 0, half)
    b.pump(PM, 255, n - 2000 - half)
    b.sync()
    while b.n < n - 150:
        b.place(PM, _is_big, b.c.total(PM) << 32, gap=int(b.rnd.integers(4, 40)))
    while b.n < n:
        b.filler()
    return b


def _pair(seed_a, seed_b):
    base, gap = 1 << 17, 160
    at = [base + gap * (i + 1) for i in range(3 * 5)]
    want = {"a": at[0:5] + at[5:10], "b": at[0:5] + at[10:15]}
    out = []
    for seed, key in ((seed_a, "a"), (seed_b, "b")):
        b = _Builder(seed, [PM])
        b.pump(PM, 0, base)
        b.sync()
        for t in sorted(want[key]):
            while b.n < t - 100:
                b.filler()
            b.place(PM, _is_big, b.c.total(PM) << 32, at=t)
        while b.n < base + gap * 16:
            b.filler()
        out.append(b)
    return out


@functools.lru_cache(maxsize=1)
def streams():
    """{name: (models uint8[n], values uint8[n])}, read-only.  A few seconds: the pumps of 2^20 and more run through the oracle."""
    built = {"strike17": _strike_stream(1717, PM, 17, 40, lanes=LANES),
             "strike20": _strike_stream(2020, PM, 20, 36),
             "strike20_small": _strike_stream(2021, PM_SMALL, 20, 6),
             "resets": _resets_stream(4848),
             "resets5": _resets5_stream(4855),
             "pack22_host": _pack22(2222)}
    built["pair_a"], built["pair_b"] = _pair(101, 202)
    out = {}
    for name, b in built.items():
        out[name] = b.arrays()
    m, v = out["pack22_host"]
    out["pack22_device"] = (np.append(m, np.uint8(PM)), np.append(v, np.uint8(255)))
    for m, v in out.values():
        m.setflags(write=False)
        v.setflags(write=False)
    return {name: out[name] for name in NAMES}


@functools.lru_cache(maxsize=1)
def profiles():
    """{name: oracle_lib.RcProfile}: the reference's payload and per-step record of every stream"""
    return {name: O.rc_profile_stream(m, v, MODEL_SIZES) for name, (m, v) in streams().items()}


def want():
    """{name: the oracle's payload}"""
    return {name: p.payload for name, p in profiles().items()}


def census(name):
    """Counter of (bytes, reset) over the stream's steps"""
    p = profiles()[name]
    return collections.Counter(zip(p.n_bytes.tolist(), p.reset.tolist()))


def big_steps(name):
    """indices of the steps that emit >= 4 bytes with no reset"""
    p = profiles()[name]
    return np.nonzero((p.n_bytes >= 4) & (p.reset == 0))[0]


def reset_steps(name):
    return np.nonzero(profiles()[name].reset)[0]


def rare_steps(name):
    """the steps k_rc_encode leaves its branch-free path for: >= 4 bytes, or a reset"""
    p = profiles()[name]
    return np.nonzero((p.n_bytes >= 4) | (p.reset != 0))[0]


def pack(names, extra=()):
    """(syms, begin) for rc_encode_streams: the named streams in order, then the (models, values) pairs of extra"""
    S = streams()
    parts = [S[n] for n in names] + list(extra)
    syms = [np.stack([m, v], axis=1).reshape(-1) for m, v in parts]
    begin = np.zeros(len(parts) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum([len(m) for m, _ in parts])
    return (np.concatenate(syms) if syms else np.zeros(0, np.uint8)), begin
