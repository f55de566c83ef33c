"""-m gpu: leon_text_bgzf_device (k_deflate_chunks, k_crc32_tiles, k_bgzf_sizes, k_bgzf_members) through capi.text_bgzf_device, judged by
tests/bgzf_check.py -- Python's zlib and gzip over every member -- never by the code under test.  The text lies in device memory
between two canaries, at base + 5 (an odd address); the canaries and the text come back unchanged."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import bgzf_check as B
import common
import hdr_samples as H

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5
M = B.MEMBER_TEXT
GRID_CAP = 4096                                                   # BGZF_MAX_GROUPS of deflate_kernels.hip


def bgzf(text, last=1, **kw):
    """the call on `text` uploaded between two canaries, d_text = base + CANARY + SHIFT: (output, n_taken, n_members)"""
    from leon_amd import capi
    lib = capi.load_library()
    data = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(data)
    edge = np.full(CANARY + SHIFT, FILL, dtype=np.uint8)
    base = capi.device_alloc(CANARY + SHIFT + n + CANARY)
    try:
        for at, a in ((0, edge), (CANARY + SHIFT, data), (CANARY + SHIFT + n, edge[:CANARY])):
            if len(a):
                a = np.ascontiguousarray(a)
                assert lib.leon_device_upload(0, C.c_void_p(base + at), C.c_void_p(a.ctypes.data), len(a)) == 0
        got = capi.text_bgzf_device(base + CANARY + SHIFT, n, last=last, **kw)
        back = np.frombuffer(capi.device_download(base, CANARY + SHIFT + n + CANARY), dtype=np.uint8)
        assert np.array_equal(back[:CANARY + SHIFT], edge), "bytes in front of d_text were written"
        assert np.array_equal(back[CANARY + SHIFT + n:], edge[:CANARY]), "bytes behind d_text were written"
        assert np.array_equal(back[CANARY + SHIFT:CANARY + SHIFT + n], data), "the text was written"
        return got
    finally:
        capi.device_free(base)


def fastq_text(n=2500, seed=41):
    bases, off = common.synthetic(n, 70, 6000, seed=seed, n_rate=0.002, err=0.02, ragged=True)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in zip(H.sra(n, seed=seed), reads, quals))


@pytest.fixture(scope="module")
def fastq():
    return fastq_text()


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, 32767, 32768, 32769, 65541])
def test_sizes(fastq, n):
    text = fastq[:n]
    out, taken, members = bgzf(text, last=1)
    assert taken == n and members == (n + M - 1) // M
    B.check(out, text)
    # without `last` only the whole members are taken, and no marker follows them
    sunk = []
    out, taken, members = bgzf(text, last=0, sink=lambda offset, size: sunk.append(size) or 0)
    assert taken == n - n % M and members == n // M
    B.check(out, text[:taken], eof=False)
    if n < M:
        assert out == b"" and sunk == []


def test_fastq_text_and_its_size(fastq):
    """the one measured bound: the payloads against zlib's Z_RLE over the same slices, DESIGN.md 4.8's 3 %, plus the 7 bytes per member
    (the empty stored block behind the chunk's block, and 03 00) that zlib's one stream does not have"""
    assert len(fastq) > 10 * M
    out, taken, members = bgzf(fastq)
    payloads = B.check(out, fastq)
    ref = 0
    for a in range(0, len(fastq), M):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        ref += len(c.compress(fastq[a:a + M]) + c.flush())
    got = sum(payloads) + 2 * len(payloads)                       # with each member's 03 00
    print("BGZF of %d bytes of FASTQ: %d members, payloads %d bytes, Z_RLE %d bytes, ratio %.4f, text / file %.3f"
          % (len(fastq), members, got, ref, got / ref, len(fastq) / len(out)))
    assert got <= 1.03 * ref + 7 * len(payloads), (got, ref)


def test_one_repeated_byte():
    text = b"A" * (3 * M + 1000)                                  # matches of 258 from end to end
    out, _, _ = bgzf(text)
    payloads = B.check(out, text)
    assert max(payloads) < 200, payloads


def test_random_bytes_are_stored():
    text = random_bytes(4 * M + 777, seed=7)
    out, _, _ = bgzf(text)
    payloads = B.check(out, text)
    assert payloads == [M + 5] * 4 + [777 + 5]                    # member size = slice + 33
    assert [size for _, size in B.walk(out)[:-1]] == [M + 33] * 4 + [777 + 33]


def test_alternating_members(fastq):
    parts = [fastq[i * M:(i + 1) * M] if i % 2 == 0 else random_bytes(M, seed=i) for i in range(7)] + [fastq[:999]]
    text = b"".join(parts)
    out, _, _ = bgzf(text)
    payloads = B.check(out, text)
    assert [p == M + 5 for p in payloads] == [False, True] * 3 + [False, False]


def by_calls(text, parts):
    """the text through one call per part, the caller carrying what a call did not take"""
    out, carry, pos = [], b"", 0
    for i, n in enumerate(parts):
        piece = carry + text[pos:pos + n]
        pos += n
        got, taken, _ = bgzf(piece, last=1 if i == len(parts) - 1 else 0)
        assert taken == (len(piece) if i == len(parts) - 1 else len(piece) - len(piece) % M)
        out.append(got)
        carry = piece[taken:]
    assert pos == len(text)
    return b"".join(out)


def test_split_into_calls(fastq):
    text = (fastq * 2)[:300000]
    whole, _, _ = bgzf(text)
    B.check(whole, text)
    assert by_calls(text, [40000, 1, 70000, 0, 300000 - 110001]) == whole


@pytest.mark.parametrize("slice_bytes", ["98304", "32768", "100000", "1"])
def test_slices(fastq, monkeypatch, slice_bytes):
    """three members per slice, one per slice, a value that is rounded down to three and one that is raised to one member: the bytes of
    the default's single slice"""
    text = (fastq * 2)[:10 * M + 4321]
    whole, _, members = bgzf(text)
    assert members == 11
    B.check(whole, text)
    monkeypatch.setenv("LEON_BGZF_SLICE", slice_bytes)
    assert bgzf(text)[0] == whole
    assert by_calls(text, [5 * M + 5, 4 * M, M + 4316]) == whole


def test_sink_contract(fastq):
    from leon_amd import capi
    seen = []
    out, _, _ = bgzf(fastq, sink=lambda offset, size: seen.append((offset, size)) or 0)
    seen.sort()
    assert seen[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(seen, seen[1:])) and sum(seen[-1]) == len(out)
    with pytest.raises(capi.LeonDnaError) as e:
        bgzf(fastq, sink=lambda offset, size: 1)
    assert e.value.code == -6 and "sink" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:                   # the marker's piece is refused like any other
        bgzf(b"", sink=lambda offset, size: 1)
    assert e.value.code == -6


def test_past_the_grid_cap():
    """4 099 members: k_bgzf_members' workgroups 0..2 frame a second member (and k_crc32_tiles walks several tiles per workgroup); every
    seventh member is random bytes (stored), the rest four letters; the output arrives in pieces from several threads"""
    n_members = GRID_CAP + 3
    n = (n_members - 1) * M + 1000
    rng = np.random.default_rng(99)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for m in range(0, n_members, 7):
        text[m * M:(m + 1) * M] = rng.integers(0, 256, len(text[m * M:(m + 1) * M]), dtype=np.uint8)
    seen = []
    out, taken, members = bgzf(text, sink=lambda offset, size: seen.append((offset, size)) or 0)
    assert taken == n and members == n_members == 4099
    assert len(out) > 2 * (16 << 20) and max(size for _, size in seen) <= 16 << 20 and sum(size for _, size in seen) == len(out)
    payloads = B.check(out, text.tobytes())
    assert all((p == min(M, n - i * M) + 5) == (i % 7 == 0) for i, p in enumerate(payloads))
    assert gzip.decompress(out) == text.tobytes()
