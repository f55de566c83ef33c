"""-m gpu: BGZF members inflated on the device (leon_bgzf_inflate_device: k_bgzf_inflate, the CRC-32 of the shares, k_bgzf_gather)
against gzip.decompress and leon_host_bgzf_inflate -- never against the code under test.  d_text sits at an odd address between two
canaries; a refusal has the host function's code and words, leaves the canaries alone and writes nothing behind the member it names."""
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

import bgzf_check
import bgzf_input as B

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5                                                        # (no text of these tests holds this byte)


def host_verdict(data, off):
    from leon_amd import capi
    try:
        return capi.host_bgzf_inflate(data, off, n_threads=4)
    except capi.LeonDnaError as e:
        return (e.code, str(e))


def device_verdict(data, off, per_launch=0, text_cap=None, pay_shift=1):
    """leon_bgzf_inflate_device between canaries: (the text, or (code, message)), and d_text's bytes as they are afterwards"""
    from leon_amd import capi
    off = np.asarray(off, dtype=np.uint64)
    raw = np.frombuffer(bytes(pay_shift) + bytes(data) + bytes(8), dtype=np.uint8)
    cap = 65536 * max(len(off) - 1, 0) if text_cap is None else text_cap
    d = capi.device_upload_bytes(bytes([FILL]) * (CANARY + SHIFT + cap + CANARY + 32))
    try:
        try:
            n_text, _ = capi.bgzf_inflate_device(raw[pay_shift:], off, d + CANARY + SHIFT, cap, max_members_per_launch=per_launch, n_bytes=len(data))
            verdict = None
        except capi.LeonDnaError as e:
            verdict = (e.code, str(e))
        got = capi.device_download(d, CANARY + SHIFT + cap + CANARY + 32)
    finally:
        capi.device_free(d)
    assert got[:CANARY + SHIFT] == bytes([FILL]) * (CANARY + SHIFT), "bytes in front of d_text were written"
    assert got[CANARY + SHIFT + cap:] == bytes([FILL]) * (CANARY + 32), "bytes behind d_text were written"
    body = got[CANARY + SHIFT:CANARY + SHIFT + cap]
    if verdict is not None:
        return verdict, body
    assert body[n_text:] == bytes([FILL]) * (cap - n_text), "bytes behind the text were written"
    return body[:n_text], body


def both_accept(data, **kw):
    off = B.offsets_of(data)
    want = gzip.decompress(data) if len(data) else b""
    assert host_verdict(data, off) == want
    got, _ = device_verdict(data, off, **kw)
    assert isinstance(got, bytes), got
    assert got == want
    return off


def both_refuse(members, bad, per_launch=0):
    """members: a list of members of which number `bad` does not decode; the device's verdict is the host's, word for word"""
    data = b"".join(members)
    off = np.zeros(len(members) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in members])
    want = host_verdict(data, off)
    assert isinstance(want, tuple) and want[0] == -1 and ("BGZF member %d (at byte %d) does not decode" % (bad, int(off[bad]))) in want[1], want
    got, body = device_verdict(data, off, per_launch=per_launch)
    assert got == want, (got, want)
    # the text in front of the later members' shares: ISIZE of every member that is one
    text0 = 0
    for m in members[:bad + 1]:
        isize = struct.unpack_from("<I", m, len(m) - 4)[0]
        text0 += isize if isize <= 65536 else 0
    assert body[text0:] == bytes([FILL]) * (len(body) - text0), "a later member's share was written"
    return got


WRITERS = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
           (6, zlib.Z_FIXED), (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)]


@pytest.mark.parametrize("level,strategy", WRITERS)
def test_every_size_by_every_writer(level, strategy):
    """every size of B.SIZES in one call, with small members between them so that text0 takes every residue mod 16"""
    sizes = [s for s in B.SIZES if level or s <= 65280]           # (65 536 stored bytes do not fit a member of 64 KiB)
    text = B.fastq_text(sum(sizes) + 2000, seed=level * 10 + strategy)
    members, at, residues = [], 0, set()
    for i, s in enumerate(sizes + list(range(1, 16)) + [3] * 3):
        residues.add(at % 16)
        members.append(B.member(text[at:at + s], level=level, strategy=strategy))
        at += s
    assert residues == set(range(16))
    both_accept(b"".join(members))


def test_matches_flushes_and_extra_fields():
    t = B.match_text(3)
    assert len(t) > 32768 + 2000
    far, far_text = B.token_member([t[:32768], (258, 32768), (258, 32768), b"xyz", (3, 1), (200, 32700), (258, 33), (17, 32768)])   # exactly 32 768, across the wrap
    assert far_text[32768:32768 + 516] == t[:516]
    members = [B.member(t[:60000], level=9), B.member(t[:60000], level=6, flush_at=20001), B.member(t[100:40000], level=1, flush_at=1, flush=zlib.Z_SYNC_FLUSH),
               far, B.EOF, B.member(b"I" * 65536, level=6), B.member(t[:5000], extra=B.subfield(b"XY", b"hello") + B.subfield(b"BC", b"abc")),
               B.member(t[:700], after_bc=B.subfield(b"ZZ", b"")), B.member((b"ACGT" * 20 + b"\n") * 780, level=9), B.EOF]
    both_accept(b"".join(members))
    for shift in (0, 2, 3):                                       # the bytes at every alignment
        both_accept(b"".join(members[2:5]), pay_shift=shift)


def test_members_written_as_minus_d_gz_writes_them():
    text = B.fastq_text(3 * 32768 + 1234, seed=8)
    data = bgzf_check.python_bgzf(text)
    bgzf_check.check(data, text)
    both_accept(data)


def test_launch_shapes():
    from leon_amd import capi
    rng = random.Random(4)
    text = B.fastq_text(40000, seed=5)
    # 1 300 tiny members in one call: more than the 1 024 chains that are resident at once
    members, at = [], 0
    for i in range(1300):
        n = rng.choice((0, 1, 7, 16, 31, 64))
        members.append(B.member(text[at:at + n], level=rng.choice((1, 6))))
        at += n
    both_accept(b"".join(members))
    # launches of 1, 2 and 3 members, an empty member on a launch's edge
    few = [B.member(text[:3000]), B.EOF, B.member(text[3000:3017]), B.member(text[3017:39000], level=9), B.EOF, B.EOF, B.member(text[39000:])]
    for per in (1, 2, 3):
        both_accept(b"".join(few), per_launch=per)
    # no members: nothing is touched, whatever the pointers
    assert capi.bgzf_inflate_device(None, None, 0, 0, n_members=0) == (0, 0)
    got, body = device_verdict(b"", np.zeros(1, dtype=np.uint64), text_cap=64)
    assert got == b"" and body == bytes([FILL]) * 64


def _good(seed, n=5000):
    return B.member(B.fastq_text(n, seed=seed))


def test_refusals_are_the_host_functions():
    text = B.fastq_text(9000, seed=6)
    pay = B.deflate_raw(text)
    crc = zlib.crc32(text)
    oversubscribed = B.Bits()
    oversubscribed.put(1, 1); oversubscribed.put(2, 2); oversubscribed.put(0, 5); oversubscribed.put(0, 5); oversubscribed.put(15, 4)   # noqa: E702
    for _ in range(19):
        oversubscribed.put(1, 3)                                  # nineteen code-length codes of one bit
    prev = B.fastq_text(4000, seed=7)
    with_dict = B.deflate_raw(prev[-1500:] + text[:500], zdict=prev)
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(with_dict)
    cases = {
        "a wrong CRC": B.frame(pay, crc ^ 0x10000, len(text)),
        "ISIZE one too large": B.frame(pay, crc, len(text) + 1),
        "ISIZE one too small": B.frame(pay, zlib.crc32(text[:-1]), len(text) - 1),
        "a slack byte in front of the trailer": B.frame(pay + b"\0", crc, len(text)),
        "a payload cut short": B.frame(pay[:-7], crc, len(text)),
        "a block of type 3": B.frame(b"\x07\x00", 0, 0),
        "an over-subscribed table": B.frame(oversubscribed.done() + bytes(8), 0, 0),
        "a match that reaches in front of the member": B.frame(with_dict, zlib.crc32(prev[-1500:] + text[:500]), 2000),
        "an ISIZE above 65 536": B.frame(pay, crc, 70000),
    }
    for name, damaged in cases.items():
        members = [_good(1), _good(2, 70), damaged, _good(3), _good(4, 16)]
        both_refuse(members, 2)
        both_refuse(members, 2, per_launch=2)                     # the launch in front of the member's has written its text
        both_refuse([damaged] + members, 0, per_launch=3)         # the smallest failing member is the one named
    # text_cap too small: the same code, the same words, the bytes needed, nothing written
    from leon_amd import capi
    data = b"".join([_good(1), _good(2)])
    off = B.offsets_of(data)
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_bgzf_inflate(data, off, text_cap=9999)
    got, body = device_verdict(data, off, text_cap=9999)
    assert e.value.code == -5 and e.value.n_text == 10000 and got == (e.value.code, str(e.value)) and "needs 10000 bytes" in got[1], (got, str(e.value))
    assert body == bytes([FILL]) * 9999


def test_pinned_buffers_of_the_reader():
    """leon_host_pinned_alloc / leon_host_pinned_free, as the reader of `-c -input-inflate device` uses them: a member's text downloaded
    into a pinned buffer in one direct copy, the buffer used twice, a buffer of 0 bytes, NULL freed"""
    import ctypes
    from leon_amd import capi
    text = B.fastq_text(50000, seed=12)
    data = B.member(text[:30000]) + B.member(text[30000:])
    d = capi.device_alloc(len(text) + 64)
    pinned = capi.host_pinned_alloc(len(text))
    try:
        assert pinned and pinned % 16 == 0
        for _ in range(2):
            ctypes.memset(pinned, FILL, len(text))
            n_text, _ = capi.bgzf_inflate_device(data, B.offsets_of(data), d, len(text))
            capi.device_download_to(pinned, d, n_text)
            assert n_text == len(text) and ctypes.string_at(pinned, n_text) == text
    finally:
        capi.host_pinned_free(pinned)
        capi.device_free(d)
    empty = capi.host_pinned_alloc(0)
    assert empty
    capi.host_pinned_free(empty)
    capi.host_pinned_free(None)
    lib = capi.load_library()
    assert lib.leon_host_pinned_alloc(0, 16, None) == -1 and b"null argument" in lib.leon_last_error(None)
