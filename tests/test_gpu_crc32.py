"""-m gpu: leon_crc32_segments_device (k_crc32_tiles, k_crc32_final) against Python's zlib.crc32 -- never against the code under test.
The bytes lie in device memory between two canaries, at base + 5 (an odd address); the canaries come back unchanged, and a call gives
the same words whatever they hold."""
import ctypes as C

import numpy as np
import pytest

import crc_shapes as S
from crc_shapes import REFUSALS

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5


def device_crc(data, seg_off, fill=FILL, shift=SHIFT, **kw):
    """the call on `data` (uint8 array) uploaded between two canaries of `fill`, d_bytes = base + CANARY + shift"""
    from leon_amd import capi
    lib = capi.load_library()
    n = len(data)
    edge = np.full(CANARY + shift, fill, dtype=np.uint8)
    base = capi.device_alloc(CANARY + shift + n + CANARY)
    try:
        for at, a in ((0, edge), (CANARY + shift, data), (CANARY + shift + n, edge[:CANARY])):
            if len(a):
                a = np.ascontiguousarray(a)
                assert lib.leon_device_upload(0, C.c_void_p(base + at), C.c_void_p(a.ctypes.data), len(a)) == 0
        got = capi.crc32_segments_device(base + CANARY + shift, n, seg_off, **kw)
        assert capi.device_download(base, CANARY + shift) == edge.tobytes(), "bytes in front of d_bytes were written"
        assert capi.device_download(base + CANARY + shift + n, CANARY) == edge[:CANARY].tobytes(), "bytes behind d_bytes were written"
        return got
    finally:
        capi.device_free(base)


def check(data, off, **kw):
    got = device_crc(data, off, **kw)
    want = S.reference(data, off)
    assert np.array_equal(got, want), [(s, hex(int(g)), hex(int(w))) for s, (g, w) in enumerate(zip(got, want)) if g != w][:4]


def test_check_value():
    assert device_crc(np.frombuffer(b"123456789", dtype=np.uint8), [0, 9]).tolist() == [0xCBF43926]


def test_edge_lengths_back_to_back():
    check(*S.edge_lengths_together())


@pytest.mark.parametrize("length", S.EDGE_LENGTHS)
def test_every_start_alignment(length):
    """the segment's first byte at every address mod 16, through the offset and through the pointer"""
    for a in range(16):
        check(*S.one_segment(length, a))
        check(*S.one_segment(length, 2), shift=a)


def test_tiny_segments():
    check(*S.tiny_segments())


def test_one_long_segment():
    check(*S.one_long())


def test_zero_segments():
    check(*S.zero_segments())


def test_past_the_grid_cap():
    """the second and third tile of every workgroup: thread 0 carries a segment from tile to tile, and lets go of it where it ends"""
    data, off = S.past_the_grid_cap()
    assert (int(off[-1]) - int(off[0])) // S.TILE >= 3 * S.MAX_GROUPS
    check(data, off)


def test_past_4_gib():
    check(*S.huge())


def test_nothing_to_do():
    from leon_amd import capi
    assert len(capi.crc32_segments_device(0, 0, None, n_seg=0)) == 0
    assert capi.crc32_segments_device(0, 5, [5, 5, 5]).tolist() == [0, 0]
    assert device_crc(np.arange(40, dtype=np.uint8), [7, 7, 7, 7]).tolist() == [0, 0, 0]
    assert len(device_crc(np.arange(40, dtype=np.uint8), [3])) == 0


def test_canaries_of_other_values():
    """what lies around the segments -- in front of d_bytes, behind it, and inside it outside [seg_off[0], seg_off[n])) -- is not part
    of any word"""
    data, off = S.edge_lengths_together()
    want = S.reference(data, off)
    for fill in (0x00, 0xFF, 0x3C):
        other = data.copy()
        other[:int(off[0])] = fill
        other[int(off[-1]):] = fill
        assert np.array_equal(device_crc(other, off, fill=fill), want)


@pytest.mark.parametrize("what,kw,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, kw, words):
    from leon_amd import capi
    with pytest.raises(capi.LeonDnaError) as e:
        device_crc(np.zeros(64, dtype=np.uint8), **kw)
    assert e.value.code == -1 and str(e.value).endswith(": " + words)
    with pytest.raises(capi.LeonDnaError) as h:
        capi.host_crc32_segments(bytes(64), **kw)
    assert str(h.value) == str(e.value)


def test_refuses_segments_without_bytes():
    from leon_amd import capi
    with pytest.raises(capi.LeonDnaError) as e:
        capi.crc32_segments_device(0, 64, [0, 4])
    assert e.value.code == -1 and str(e.value).endswith(": crc32 segments: null argument")
