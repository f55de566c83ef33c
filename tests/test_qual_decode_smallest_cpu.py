"""No GPU: leon_host_qual_decode_blocks names the SMALLEST block that fails (include/leon_dna.h), whichever of its threads fails first.
Many damaged blocks behind one good one, the early ones long and the late ones short, so that with several threads a later block's
failure is the first in time: the message must name block 1 on every run."""
import zlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def test_smallest_failing_block_is_named(built):
    from leon_amd import capi
    good = b"".join(b"IIIIFFFF" * 12 + b"\n" for _ in range(50))
    q = (33 + np.random.default_rng(1).integers(0, 41, size=(40000, 151))).astype(np.uint8)        # 6 MB that take zlib milliseconds to inflate
    q[:, 150] = 10
    long_text, long_lines = q.tobytes(), range(40000)
    damaged_long = bytearray(zlib.compress(long_text, 1))
    damaged_long[-1] ^= 0xFF                                      # the Adler-32: known only when the whole block is inflated
    blocks = [(0, zlib.compress(good), 50), (1, bytes(damaged_long), len(long_lines))]
    sizes = [len(good) - 50, len(long_text) - len(long_lines)]
    for b in range(2, 40):                                        # short streams that fail at their first byte
        blocks.append((b, b"\x00\x00\x00", 1))
        sizes.append(8)
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(damaged_long))
    for threads in (1, 2, 4, 8, 8, 8, 8, 8):
        with pytest.raises(capi.LeonDnaError) as e:
            capi.host_qual_decode_blocks(blocks, sizes, n_threads=threads)
        assert e.value.code == -1 and str(e.value).endswith("quality block 1 does not decode"), (threads, str(e.value))
