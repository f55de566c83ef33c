"""Seeded inputs of N_BLOCKS = 4099 blocks: more than twice the grid cap of every kernel that gives a block to a wave or a
workgroup and walks the rest in `for (b = blockIdx.x; b < n_blocks; b += gridDim.x)`.  The same wave (workgroup slot s) then
sees blocks s, s + 2048, s + 4096, and what one block leaves behind in LDS or registers can reach the next.  The kinds of
blocks are laid out by kind() so that consecutive trips of one slot never see the same kind.  Pure numpy, no GPU:
tests/test_many_blocks_cpu.py checks that the inputs are what they claim to be, tests/test_gpu_many_blocks.py runs them."""
import functools

import numpy as np

import hdr_samples as H
import synth

# The grid caps, in blocks per trip of the kernel's block loop (the launchers carry a comment that points back here):
#   launch_rc_encode (rc_kernels.hip): 256 * (8 / G) workgroups of G blocks each = 2048 blocks for G = 1, 2, 4, 8
#   launch_decode_blocks, launch_hdr_decode_symbols, launch_hdr_text (decode_kernels.hip): 256 * 8 waves = 2048 blocks
#   launch_rc_records (rc_kernels.hip): 256 * 4 workgroups = 1024 blocks
CAP = 256 * 8
CAP_RC_RECORDS = 256 * 4
N_BLOCKS = 2 * CAP + 3            # two full trips and a third with three blocks: G = 2, 4, 8 end in a partial group (1 of 2, 3 of 4, 3 of 8)
assert N_BLOCKS > 2 * CAP and N_BLOCKS > 4 * CAP_RC_RECORDS

N_KINDS = 8


def kind(b):
    """the kind (0..7) of block b: slot s = b % CAP sees kind s % 8 on trip 0 and a kind 1..7 further on each later trip, the step
    changing every 8 slots -- every ordered pair of distinct kinds follows one another on some slot, and 8 consecutive blocks
    (one G = 8 group) hold all 8 kinds"""
    s, t = b % CAP, b // CAP
    return (s + t * (1 + (s // 8) % 7)) % N_KINDS


# ---- (a) symbol streams for DnaEncodeContext.rc_encode_streams ------------------------------------------------------------------
EMPTY, ONE, TILE, TILE1, NARROW, WIDE, LONG, SKEW = range(N_KINDS)
KIND_NAMES = ("EMPTY", "ONE", "TILE", "TILE1", "NARROW", "WIDE", "LONG", "SKEW")
N_SMALL = 8
MODEL_SIZES = [2, 5, 5, 2, 3, 3, 3, 2] + [256] * 72          # the DNA stream's model set: 8 small models, 8 numeric groups of 9
_SZ = np.array(MODEL_SIZES, dtype=np.int64)
# (symbols per stream of each kind: exact, or an inclusive range)
STREAM_LEN = {EMPTY: (0, 0), ONE: (1, 1), TILE: (64, 64), TILE1: (65, 65), NARROW: (130, 170), WIDE: (560, 640), LONG: (2800, 3200),
              SKEW: (470, 530)}


def _mix_probs():
    from test_gpu_parity import _model_probs                  # (LONG's mix is that test's: one definition)
    return _model_probs()


def _values(rng, m):
    """a value for every model of m: three in ten uniform over the model's alphabet, the rest geometric (small values frequent)"""
    sz = _SZ[m]
    uni = np.minimum((rng.random(len(m)) * sz).astype(np.int64), sz - 1)
    geo = np.minimum(rng.geometric(0.3, size=len(m)) - 1, sz - 1)
    return np.where(rng.random(len(m)) < 0.3, uni, geo).astype(np.uint8)


def _stream(rng, kd, probs):
    lo, hi = STREAM_LEN[kd]
    n = int(rng.integers(lo, hi + 1))
    if kd == EMPTY:
        m = np.zeros(0, dtype=np.int64)
    elif kd == ONE:
        m = rng.integers(0, N_SMALL, size=1)
    elif kd in (TILE, TILE1, LONG):
        m = rng.choice(80, size=n, p=probs)
    elif kd == NARROW:                                          # the small models and numeric models 8 and 9 only
        m = rng.integers(0, 10, size=n)
    elif kd == WIDE:                                            # all 72 numeric models inside the first two tiles, and ever after
        head = np.concatenate([np.arange(N_SMALL, 80), rng.integers(0, 80, size=128 - 72)])
        m = np.concatenate([rng.permutation(head), rng.integers(0, 80, size=n - 128)])
    else:                                                       # SKEW: one value on one 256-symbol model
        m = np.full(n, int(rng.integers(N_SMALL, 80)), dtype=np.int64)
        return m.astype(np.uint8), np.full(n, int(rng.integers(0, 256)), dtype=np.uint8)
    return m.astype(np.uint8), _values(rng, m)


@functools.lru_cache(maxsize=1)
def rc_streams():
    """(syms uint8[2 * n] of (model, value) pairs, begin uint64[N_BLOCKS + 1], MODEL_SIZES); stream b is of kind(b).  Read-only."""
    rng = np.random.default_rng(4099)
    probs = _mix_probs()
    ms, vs, begin = [], [], np.zeros(N_BLOCKS + 1, dtype=np.uint64)
    for b in range(N_BLOCKS):
        m, v = _stream(rng, kind(b), probs)
        ms.append(m)
        vs.append(v)
        begin[b + 1] = begin[b] + np.uint64(len(m))
    syms = np.stack([np.concatenate(ms), np.concatenate(vs)], axis=1).reshape(-1)
    syms.setflags(write=False)
    begin.setflags(write=False)
    return syms, begin, MODEL_SIZES


def rc_stream(b):
    """(models, values) of stream b"""
    syms, begin, _ = rc_streams()
    a, e = int(begin[b]), int(begin[b + 1])
    return syms[2 * a:2 * e:2], syms[2 * a + 1:2 * e:2]


# ---- (b) reads for encode_batch / decode_blocks at reads_per_block = DNA_RPB ----------------------------------------------------
DNA_RPB = 3
GENOME_LEN = 90000
LONG_READ_LEN = 70000


def dna_heavy(b):
    return kind(b) % 2 == 1


def _heavy_blocks():
    return [b for b in range(N_BLOCKS) if dna_heavy(b)]


def dna_junk_blocks():
    """every 16th heavy block: its first read is random bases, longer than 255 (no anchor)"""
    return _heavy_blocks()[::16]


def dna_long_read_blocks():
    """(b0, b1): the blocks whose middle read is a 70 000-base read with a fifth of its positions in error.  b0 is on trip 0 and the
    block its wave decodes next (b0 + CAP) is a light one; b1 is on trip 1 and the block its wave decoded before (b1 - CAP) is light."""
    junk = set(dna_junk_blocks())
    b0 = next(b for b in range(64, CAP) if dna_heavy(b) and not dna_heavy(b + CAP) and b not in junk)
    b1 = next(b for b in range(CAP + 1024, 2 * CAP) if dna_heavy(b) and not dna_heavy(b - CAP) and b not in junk and b - CAP != b0)
    return b0, b1


@functools.lru_cache(maxsize=1)
def dna_reads():
    """the reads (list of bytes, DNA_RPB per block) and the genome they come from is synth.make_genome(GENOME_LEN, seed=5).
    heavy blocks (dna_heavy): ragged reads of up to 600 bases with 5 % errors and 1 % N -- N, error and anchor positions beyond 255
    take the second byte of their numeric models; light blocks: clean 100-base reads."""
    g = synth.make_genome(GENOME_LEN, seed=5)
    heavy = _heavy_blocks()
    light = [b for b in range(N_BLOCKS) if not dna_heavy(b)]
    reads = [None] * (N_BLOCKS * DNA_RPB)
    for blocks, kw in ((heavy, dict(read_len=600, seed=11, err=0.05, n_rate=0.01, ragged=True)), (light, dict(read_len=100, seed=12, err=0.0))):
        bs, off = synth.make_reads(g, DNA_RPB * len(blocks), **kw)
        raw = bs.tobytes()
        for i, b in enumerate(blocks):
            for j in range(DNA_RPB):
                r = DNA_RPB * i + j
                reads[DNA_RPB * b + j] = raw[int(off[r]):int(off[r + 1])]
    rng = np.random.default_rng(13)
    for b in dna_junk_blocks():
        reads[DNA_RPB * b] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(260, 400)))].tobytes()
    for seed, b in zip((6, 16), dna_long_read_blocks()):
        reads[DNA_RPB * b + 1] = synth.make_reads(g, 1, LONG_READ_LEN, seed=seed, err=0.2, n_rate=0.15)[0].tobytes()
    return tuple(reads)


def dna_normalised(reads):
    """what the format gives back: every byte that is not A, C, G or T is an N"""
    keep = np.zeros(256, dtype=bool)
    keep[list(b"ACGT")] = True
    out = []
    for r in reads:
        a = np.frombuffer(r, dtype=np.uint8)
        out.append(np.where(keep[a], a, np.uint8(ord("N"))).astype(np.uint8).tobytes())
    return out


# ---- (c) headers for header_encode_batch at reads_per_block = HDR_RPB -----------------------------------------------------------
HDR_RPB = 2
HDR_CAP = 4096                                                  # leon_amd.capi.HEADER_TEXT_DEVICE_CAP (the CPU test holds the two together)
HDR_LENGTHS = (700, 1500, 3000, HDR_CAP - 1)
FIRST_LEN = 3000


def hdr_heavy(b):
    return kind(b) % 2 == 1


def _template_fields(rng, n_bytes):
    """numeric fields of 1 to 6 digits (no leading zero), enough of them for n_bytes with their separators"""
    fields, size = [], 0
    while size < n_bytes:
        f = b"%d" % int(rng.integers(1, 10 ** int(rng.integers(1, 7))))
        fields.append(f)
        size += len(f) + 1
    return fields


def _bumped(rng, fields, length):
    """the template cut to `length` bytes, one or two of its numeric fields bumped (the digit count kept, so the length stays)"""
    fs = list(fields)
    for _ in range(int(rng.integers(1, 3))):
        i = int(rng.integers(0, len(fs)))
        v = int(fs[i])
        w = v + int(rng.choice([1, 1, 2, 7, -1]))
        if w >= 0 and len(b"%d" % w) == len(fs[i]):
            fs[i] = b"%d" % w
    h = b":".join(fs)
    assert len(h) >= length
    return h[:length]


def _headers(seed):
    rng = np.random.default_rng(seed)
    fields = _template_fields(rng, HDR_CAP + 64)
    first = b":".join(fields)[:FIRST_LEN]
    hs = []
    for b in range(N_BLOCKS):
        for j in range(HDR_RPB):
            if hdr_heavy(b):
                hs.append(_bumped(rng, fields, int(rng.choice(HDR_LENGTHS))))
            else:
                hs.append(b"SRR1.%d len=%d" % (HDR_RPB * b + j + 1, int(rng.integers(50, 300))))
    return hs, first, fields


@functools.lru_cache(maxsize=1)
def headers():
    """(hs, first): HDR_RPB headers per block; heavy blocks (hdr_heavy) are a ~3000-byte template of ':'-joined numeric fields (a
    separator in every 64-byte word) cut to a length of HDR_LENGTHS with a field or two bumped, light ones `SRR1.<n> len=<n>`.
    Every header is below the kernel's cap.  Read-only."""
    hs, first, _ = _headers(2053)
    return tuple(hs), first


def fallback_blocks():
    """the blocks headers_with_fallbacks replaces, every one on a workgroup slot of its own: the blocks of the same slot on the trip
    before and on the trip after, where there is one, are ordinary.  Even positions of the list get a header over the cap, odd ones
    a run of hdr_samples.nasty."""
    trip0 = [3 + 200 * i for i in range(9)]
    trip1 = [CAP + 100 + 200 * i for i in range(9)]
    out = sorted(trip0 + trip1 + [CAP + 1, 2 * CAP + 2])      # 2049 has a partner on both sides (1 and 4097), 4098 closes the last trip
    assert len(set(b % CAP for b in out)) == len(out) == 20
    return out


@functools.lru_cache(maxsize=1)
def headers_with_fallbacks():
    """(hs, first, replaced): headers() with the blocks of fallback_blocks() replaced by what the device kernel hands to the host
    decoder (a header of HDR_CAP + 1 bytes) or may hand to it (hdr_samples.nasty: empty, binary, hundreds of fields)"""
    hs, first, fields = _headers(2053)
    rng = np.random.default_rng(77)
    nasty = H.nasty(400, seed=21)
    replaced = fallback_blocks()
    for i, b in enumerate(replaced):
        if i % 2 == 0:
            hs[HDR_RPB * b] = _bumped(rng, fields, HDR_CAP + 1)
        else:
            at = int(rng.integers(0, len(nasty) - HDR_RPB))
            hs[HDR_RPB * b:HDR_RPB * (b + 1)] = nasty[at:at + HDR_RPB]
    return tuple(hs), first, tuple(replaced)
