"""CPU tests of the block checksums' host side: leon_host_crc32_segments against Python's zlib.crc32 on the shapes the device form is
tested with (test_gpu_crc32.py), and what both forms refuse before they touch anything.  No GPU."""
import os

import numpy as np
import pytest

import crc_shapes as S
from crc_shapes import REFUSALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def capi():
    import leon_amd
    if not os.path.exists(leon_amd.lib_path()) or not os.path.exists(os.path.join(ROOT, "leon_amd", "lib", "leon")):
        leon_amd.build_library()
    leon_amd.load_library()
    from leon_amd import capi
    return capi


@pytest.fixture(scope="module")
def shapes():
    return [(name, data, off, S.reference(data, off)) for name, data, off in S.small_shapes()]


@pytest.fixture(scope="module")
def huge():
    data, off = S.huge()
    return data, off, S.reference(data, off)


def test_check_value(capi):
    assert capi.host_crc32_segments(b"123456789", [0, 9], n_threads=1).tolist() == [0xCBF43926]
    assert capi.host_crc32_segments(b"x123456789y", [1, 1, 10, 10], n_threads=3).tolist() == [0, 0xCBF43926, 0]


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_host_equals_zlib(capi, shapes, threads):
    for name, data, off, want in shapes:
        got = capi.host_crc32_segments(data, off, n_threads=threads)
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_host_equals_zlib_past_4_gib(capi, huge, threads):
    data, off, want = huge
    assert np.array_equal(capi.host_crc32_segments(data, off, n_threads=threads), want)


def test_nothing_to_do(capi):
    assert len(capi.host_crc32_segments(None, None, n_seg=0)) == 0
    assert len(capi.host_crc32_segments(b"abc", [1], n_threads=2)) == 0
    # all segments empty: no byte is needed, not even a buffer
    assert capi.host_crc32_segments(None, [5, 5, 5], n_bytes=5).tolist() == [0, 0]
    assert capi.host_crc32_segments(b"abcdef", [6, 6]).tolist() == [0]


@pytest.mark.parametrize("what,kw,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(capi, what, kw, words):
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_crc32_segments(bytes(64), **kw)
    assert e.value.code == -1 and str(e.value).endswith(": " + words)


def test_refuses_segments_without_bytes(capi):
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_crc32_segments(None, [0, 4], n_bytes=64)
    assert e.value.code == -1 and str(e.value).endswith(": crc32 segments: null argument")


def test_container_patch_helper(tmp_path):
    """the helper the checksum tests damage containers with (container_patch.py), on the file `leon -selftest-container` writes"""
    import subprocess
    import container_patch as P
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    path = str(tmp_path / "self.leon")
    r = subprocess.run([leon, "-selftest-container", path], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert P.h5_has(path, "leon/metadata/dna_blocksizes") and not P.h5_has(path, "leon/metadata/checksums")
    table, at = P.find_dataset(path, "leon/metadata/dna_blocksizes", np.uint64)
    assert table.tolist() == [1, 2, 3, 2 ** 64 - 1, 0]
    P.flip_bit(path, at + 8 * 2 + 1, bit=3)                       # word 2, bit 11
    assert P.h5_dataset(path, "leon/metadata/dna_blocksizes", np.uint64).tolist() == [1, 2, 3 ^ (1 << 11), 2 ** 64 - 1, 0]
    block, at = P.find_dataset(path, "leon/dna/block_0")
    assert len(block) == 100000
    P.patch(path, at + 99990, b"0123456789")
    after = P.h5_dataset(path, "leon/dna/block_0")
    assert after[99990:].tobytes() == b"0123456789" and np.array_equal(after[:99990], block[:99990])
    # the other datasets are where they were
    assert P.h5_dataset(path, "leon/header/block_0").tobytes() == block[:17].tobytes()
    with pytest.raises(AssertionError):
        P.find_bytes(path, b"these bytes are nowhere in the file")
    with pytest.raises(AssertionError):
        P.find_bytes(path, block[:17].tobytes())                  # twice: the header block is the DNA block's beginning
