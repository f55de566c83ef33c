"""Inputs of the CRC-32 tests (test_crc32_cpu.py, test_gpu_crc32.py): (name, bytes as a uint8 array, segment offsets) and the reference,
Python's zlib.crc32 over every segment -- never the code under test."""
import zlib

import numpy as np

EDGE_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097)
TILE = 4096
MAX_GROUPS = 4096          # kernels.h CRC32_MAX_GROUPS: above that many tiles a workgroup walks more than one

# what both forms refuse before they touch anything: (what, arguments beside the 64 bytes, the words)
REFUSALS = [
    ("no offsets", dict(seg_off=None, n_seg=2), "crc32 segments: null argument"),
    ("no result", dict(seg_off=[0, 4, 8], null_crc=True), "crc32 segments: null argument"),
    ("offsets run backwards", dict(seg_off=[0, 9, 8, 12]), "crc32 segments: segment offsets are not monotonic"),
    ("end behind the bytes", dict(seg_off=[0, 4, 65]), "crc32 segments: the segments end behind the bytes given"),
]


def reference(data, off):
    mv = memoryview(data)
    return np.array([zlib.crc32(mv[int(off[s]):int(off[s + 1])]) for s in range(len(off) - 1)], dtype=np.uint32)


def offsets(lengths, start=0):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[0] = start
    off[1:] = start + np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def edge_lengths_together():
    """every edge length as one segment, back to back, the first one 3 bytes into the buffer"""
    off = offsets(EDGE_LENGTHS, start=3)
    return random_bytes(int(off[-1]) + 9, 1), off


def one_segment(length, start, seed=2):
    """one segment of `length` bytes that begins `start` bytes into the buffer; bytes follow it"""
    return random_bytes(start + length + 21, seed + length), offsets([length], start=start)


def tiny_segments():
    """5 000 segments of 0-3 bytes, with runs of empty ones: hundreds of boundaries in one tile"""
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 4, 5000)
    for at in (0, 700, 701, 2500, 4990):
        lengths[at:at + int(rng.integers(3, 60))] = 0
    off = offsets(lengths[:5000], start=1)
    return random_bytes(int(off[-1]) + 5, 4), off


def one_long():
    return one_segment((1 << 20) + 5, 7)


def zero_segments():
    """all-zero bytes: only the length's term is non-zero, so a wrong power of x shows"""
    lengths = [0, 1, 2, 15, 16, 17, 255, 4096, 4097, 12345, 65536, (1 << 20) + 3, 3]
    off = offsets(lengths, start=11)
    return np.zeros(int(off[-1]) + 4, dtype=np.uint8), off


def past_the_grid_cap():
    """more than three times MAX_GROUPS tiles: every workgroup walks several consecutive tiles, some of them across the ends of segments
    (one of them empty) that fall wherever the draw puts them"""
    n = 3 * MAX_GROUPS * TILE + 777
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.integers(0, n, 8))
    bounds = np.concatenate(([0], cuts[:4], cuts[3:], [n])).astype(np.uint64) + np.uint64(13)     # cuts[3] twice: an empty segment
    return random_bytes(n + 13 + 6, 6), bounds


def huge():
    """one segment of 2^32 + 7 bytes, zeros but for a few places: the exponents do not fit 32 bits"""
    n = (1 << 32) + 7
    data = np.zeros(n + 9 + 3, dtype=np.uint8)
    for at, v in ((9, 0x31), (9 + 4095, 0x80), (9 + (1 << 31) + 17, 0x01), (9 + (1 << 32) - 1, 0xFE), (9 + n - 1, 0x7F)):
        data[at] = v
    return data, offsets([n], start=9)


def small_shapes():
    """(name, data, offsets) of everything but the one of 4 GiB"""
    yield ("edge lengths",) + edge_lengths_together()
    for L in EDGE_LENGTHS:
        for a in (0, 1, 15, 16):
            yield ("length %d at %d" % (L, a),) + one_segment(L, a)
    yield ("tiny segments",) + tiny_segments()
    yield ("one long",) + one_long()
    yield ("zeros",) + zero_segments()
    yield ("past the grid cap",) + past_the_grid_cap()
