"""-m gpu: leon_text_bgzf_device_ex with LEON_BGZF_F_MATCHES (k_deflate_lz_chunks in front of the CRC kernels, k_bgzf_sizes and
k_bgzf_members) through capi.text_bgzf_device_ex, judged by tests/bgzf_check.py -- Python's zlib and gzip over every member -- and by
tests/deflate_lz.py: deflate_tokens.scan reads the tokens of every member that is not stored, and they have to be the restatement's
tokens of the member's text.  The text lies in device memory between two canaries at an odd address, as in test_gpu_bgzf.py.

A distance code past 15 bits -- df_code_lengths halving the distance frequencies -- can be built within 32 768 bytes and is the case
deep_distance_code of tests/deflate_lz_cases.py: 17 distance codes with Fibonacci counts, 4 180 matches of five bytes."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_check as B
import bgzf_records as R
import deflate_lz as Z
import deflate_lz_cases as K
import deflate_tokens as T

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5
M = B.MEMBER_TEXT
MATCHES = 1                                                       # LEON_BGZF_F_MATCHES
LZ_GROUPS = 256                                                   # DF_LZ_MAX_GROUPS of deflate_kernels.hip


def ex(text, flags=MATCHES, last=1, rec_off=None, n_head=0, call="ex", **kw):
    """leon_text_bgzf_device_ex on `text` uploaded between two canaries, d_text = base + CANARY + SHIFT; rec_off: the body's record
    starts (record mode), None: the fixed cuts.  call: 'ex', or 'records' / 'fixed' for the entries without flags.
    Returns (output, n_taken, n_members, the members' text offsets or None)."""
    from leon_amd import capi
    lib = capi.load_library()
    data = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(data)
    edge = np.full(CANARY + SHIFT, FILL, dtype=np.uint8)
    base = capi.device_alloc(CANARY + SHIFT + n + CANARY)
    off = None if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
    d_off = 0 if off is None else capi.device_alloc(8 * len(off))
    try:
        for at, a in ((0, edge), (CANARY + SHIFT, data), (CANARY + SHIFT + n, edge[:CANARY])):
            if len(a):
                a = np.ascontiguousarray(a)
                assert lib.leon_device_upload(0, C.c_void_p(base + at), C.c_void_p(a.ctypes.data), len(a)) == 0
        if d_off:
            assert lib.leon_device_upload(0, C.c_void_p(d_off), C.c_void_p(off.ctypes.data), 8 * len(off)) == 0
        d_text, n_rec = base + CANARY + SHIFT, 0 if off is None else len(off) - 1
        try:
            if call == "fixed":
                got = capi.text_bgzf_device(d_text, n, last=last, **kw) + (None,)
            elif call == "records":
                out, taken, members, _, m_text = capi.text_bgzf_records_device(d_text, n_head, n - n_head, d_off, n_rec, last=last, **kw)
                got = out, taken, members, m_text.tolist()
            else:
                out, taken, members, _, m_text = capi.text_bgzf_device_ex(d_text, n_head, n - n_head, d_off, n_rec, flags=flags, last=last, **kw)
                got = out, taken, members, m_text.tolist()
        finally:
            back = np.frombuffer(capi.device_download(base, CANARY + SHIFT + n + CANARY), dtype=np.uint8)
            assert np.array_equal(back[:CANARY + SHIFT], edge), "bytes in front of d_text were written"
            assert np.array_equal(back[CANARY + SHIFT + n:], edge[:CANARY]), "bytes behind d_text were written"
            assert np.array_equal(back[CANARY + SHIFT:CANARY + SHIFT + n], data), "the text was written"
        return got
    finally:
        capi.device_free(base)
        if d_off:
            capi.device_free(d_off)


def payload_tokens(payload):
    """the match tokens of a member's payload, None for the stored form; the layout around them is checked"""
    if payload[0] & 7 == 0:
        return None
    blocks = T.scan(payload)["blocks"]
    assert [b["kind"] for b in blocks] == ["dynamic", "stored", "fixed"] and blocks[1]["len"] == 0 and blocks[2]["n_symbols"] == 1
    assert [b["final"] for b in blocks] == [False, False, True] and blocks[1]["align"] <= 7
    return blocks[0]["matches"]


def check_tokens(out, text, begins=None, eof=True):
    """every member of `out` that is not stored holds the restatement's tokens of its text (the literals follow from the matches and
    the text, which the caller has checked); begins: the members' text offsets (default: the fixed cuts).  Returns which are stored."""
    members = B.walk(out)[:-1] if eof else B.walk(out)
    begins = list(range(0, len(text), M)) if begins is None else list(begins)
    assert len(begins) == len(members)
    stored = []
    for i, ((at, size), a) in enumerate(zip(members, begins)):
        b = begins[i + 1] if i + 1 < len(begins) else len(text)
        got = payload_tokens(out[at + 18:at + size - 8])
        stored.append(got is None)
        if got is not None:
            assert got == Z.matches(text[a:b]), "member %d: other tokens than the restatement's" % i
    return stored


def judged(text, **kw):
    """one call with `last` over the whole text, both judges; returns (output, payload sizes, which members are stored)"""
    out, taken, members, m_text = ex(text, **kw)
    assert taken == len(text) and members == (len(text) + M - 1) // M and m_text == list(range(0, len(text), M))
    payloads = B.check(out, text)
    return out, payloads, check_tokens(out, text)


@pytest.fixture(scope="module")
def fastq():
    return K.fastq_fixture()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 255, 256, 257, 32767, 32768, 32769, 65541])
def test_sizes(fastq, n):
    text = fastq[:n]
    _, _, stored = judged(text)
    assert not any(stored[:n // M]), "a whole member of FASTQ is compressible: its tokens were compared"
    out, taken, members, _ = ex(text, last=0)
    assert taken == n - n % M and members == n // M
    B.check(out, text[:taken], eof=False)
    check_tokens(out, text[:taken], eof=False)
    if n < M:
        assert out == b""


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case(name):
    """step and segment edges, collisions, the distance alphabet: what each case is meant to be is asserted in test_deflate_lz_cpu.py"""
    text = K.CASES[name]
    _, _, stored = judged(text)
    assert stored == [False], "the case is compressible: its tokens were compared"


def test_distance_code_cut_to_15_bits():
    """the frequencies of deep_distance_code want 16 bits (asserted in test_deflate_lz_cpu.py); the block declares a complete distance
    code of at most 15 and uses its longest codes"""
    text = K.CASES["deep_distance_code"]
    out, _, _, _ = ex(text)
    (at, size), = B.walk(out)[:-1]
    block = T.scan(out[at + 18:at + size - 8])["blocks"][0]
    lens = [l for l in block["d_lengths"] if l]
    assert len(lens) == 17 and T.kraft(lens) == 32768 and max(lens) <= 15
    assert block["d_used"] == block["d_declared"] == max(lens) and len(block["matches"]) == 4180


def test_one_repeated_byte_through_three_members():
    text = b"A" * (3 * M + 1000)
    _, payloads, stored = judged(text)
    assert stored == [False] * 4 and max(payloads) < 200, payloads


def test_random_bytes_are_stored(fastq):
    rnd = lambda n, seed: np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    text = rnd(4 * M + 777, 7)
    out, payloads, stored = judged(text)
    assert payloads == [M + 5] * 4 + [777 + 5] and stored == [True] * 5
    assert payloads == B.check(ex(text, call="fixed")[0], text)                    # the sizes k_deflate_chunks gives
    text = b"".join([fastq[i * M:(i + 1) * M] if i % 2 == 0 else rnd(M, i) for i in range(7)] + [fastq[:999]])
    out, payloads, stored = judged(text)
    assert stored == [False, True] * 3 + [False, False] and [p == M + 5 for p in payloads] == stored


def by_calls(text, parts, **kw):
    """the text through one call per part, the caller carrying what a call did not take"""
    out, carry, pos = [], b"", 0
    for i, n in enumerate(parts):
        piece = carry + text[pos:pos + n]
        pos += n
        got, taken, _, _ = ex(piece, last=1 if i == len(parts) - 1 else 0, **kw)
        assert taken == (len(piece) if i == len(parts) - 1 else len(piece) - len(piece) % M)
        out.append(got)
        carry = piece[taken:]
    assert pos == len(text)
    return b"".join(out)


def fastq_offsets(text):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    return [0] + (nl[3::4] + 1).tolist()


def test_members_do_not_depend_on_calls_slices_or_mode(fastq, monkeypatch):
    text = fastq[:5 * M + 4321]
    whole, _, _ = judged(text)
    assert by_calls(text, [40000, 1, 70000, 0, len(text) - 110001]) == whole
    for slice_bytes in ("32768", "98304"):                        # one member a slice, three members a slice
        monkeypatch.setenv("LEON_BGZF_SLICE", slice_bytes)
        assert ex(text)[0] == whole
    # record mode: other cuts, and every member still the restatement's tokens of its own text -- in one slice and in slices of one
    off = fastq_offsets(text + b"\n")[:-1] + [len(text)]
    outs = []
    for slice_bytes in ("32768", None):
        if slice_bytes is None:
            monkeypatch.delenv("LEON_BGZF_SLICE")
        out, taken, members, begins = ex(text, rec_off=off)
        assert taken == len(text) and begins != list(range(0, len(text), M))
        assert [a for _, a, _ in R.check_records(out, text, off)] == begins
        assert not any(check_tokens(out, text, begins))
        outs.append(out)
    assert outs[0] == outs[1]


def test_past_the_grid_cap():
    """2 * DF_LZ_MAX_GROUPS + 3 members: every workgroup walks its loop a second time, three a third time, with the distances of the
    member before still in its scratch; every seventh member is random bytes (stored), the rest four letters"""
    n_members = 2 * LZ_GROUPS + 3
    n = (n_members - 1) * M + 1000
    rng = np.random.default_rng(98)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for m in range(0, n_members, 7):
        text[m * M:(m + 1) * M] = rng.integers(0, 256, len(text[m * M:(m + 1) * M]), dtype=np.uint8)
    out, taken, members, _ = ex(text)
    assert taken == n and members == n_members
    payloads = B.check(out, text.tobytes())
    assert all((p == min(M, n - i * M) + 5) == (i % 7 == 0) for i, p in enumerate(payloads))


def test_flags_zero_is_the_old_encoder(fastq):
    text = fastq[:3 * M + 77]
    out, taken, members, begins = ex(text, flags=0)
    assert (out, taken, members) == ex(text, call="fixed")[:3]
    off = fastq_offsets(text + b"\n")[:-1] + [len(text)]
    assert ex(text, flags=0, rec_off=off) == ex(text, rec_off=off, call="records")
    assert ex(text, flags=0, rec_off=off)[0] != ex(text, rec_off=off)[0]


@pytest.mark.parametrize("flags", [2, 3, 0x80000000])
def test_unknown_flag_is_refused(fastq, flags):
    from leon_amd import capi
    sunk = []
    with pytest.raises(capi.LeonDnaError) as e:
        ex(fastq[:M + 5], flags=flags, sink=lambda offset, size: sunk.append(size) or 0)
    assert e.value.code == -1 and "flags" in str(e.value) and sunk == []


def test_size_on_the_fastq_fixture(fastq):
    """payloads plus 03 00 against zlib's Z_RLE and zlib level 1 over the same slices.  The cap of 0.85 of Z_RLE is the issue's
    condition (the CPU estimate is 0.69): a search that is silently off does not pass.  Against level 1: measured, not asserted."""
    out, payloads, stored = judged(fastq)
    assert not any(stored)
    rle = lvl1 = 0
    for a in range(0, len(fastq), M):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        rle += len(c.compress(fastq[a:a + M]) + c.flush())
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        lvl1 += len(c.compress(fastq[a:a + M]) + c.flush())
    got = sum(payloads) + 2 * len(payloads)
    print("BGZF with matches of %d bytes of FASTQ: %d members, payloads + 03 00 %d bytes; Z_RLE %d (ratio %.4f), zlib level 1 %d (ratio %.4f), "
          "text / file %.3f" % (len(fastq), len(payloads), got, rle, got / rle, lvl1, got / lvl1, len(fastq) / len(out)))
    assert got <= 0.85 * rle, (got, rle)
