"""No GPU: the host side of `leon -c -input-inflate`.  leon_host_bgzf_members against a walk written in Python,
leon_host_bgzf_inflate against gzip.decompress, both under AddressSanitizer / UBSan in a stand-alone program on damaged streams, the
three entry points declared, bound and exported, and the refusals of the option that need no device."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_check
import bgzf_input as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("leon_host_bgzf_members", "leon_host_bgzf_inflate", "leon_bgzf_inflate_device")


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


@pytest.fixture(scope="module")
def text():
    return B.fastq_text(200000, seed=1)


def same_walk(data, last):
    from leon_amd import capi
    want, got = B.walk(data, last), capi.host_bgzf_members(data, last=last)
    for key in ("n_members", "n_text", "consumed", "stop"):
        assert got[key] == want[key], (key, got, want)
    assert got["member_off"].tolist() == want["member_off"]
    assert (got["rc"] == 0) == (want["stop"] in (B.WHOLE, B.PARTIAL)), got
    if want["stop"] == B.TRUNCATED:
        assert got["rc"] == -1 and "BGZF member %d (at byte %d) is truncated" % (want["n_members"], want["consumed"]) in got["message"], got
    if want["stop"] == B.FOREIGN:
        assert got["rc"] == -1 and "no BGZF member at byte %d" % want["consumed"] in got["message"], got
    return want


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    raw = ctypes.CDLL(capi.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared"
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS, name + " is not bound"
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    for name in ("leon_host_pinned_alloc", "leon_host_pinned_free"):          # the reader's pinned buffers
        assert re.search(r"\b%s\s*\(" % name, src) and name in capi._EXPORTS and hasattr(raw, name), name
    assert callable(capi.host_pinned_alloc) and callable(capi.host_pinned_free)
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions


def test_walk_of_whole_files(built, text):
    data = B.bgzf(text)
    w = same_walk(data, True)
    assert w["stop"] == B.WHOLE and w["n_members"] == 5 and w["n_text"] == len(text) and w["consumed"] == len(data)
    extra = B.subfield(b"XY", b"some other field") + B.subfield(b"BC", b"xyz") + B.subfield(b"B\0", b"")       # XLEN > 6, a B C of another length
    members = [B.EOF, B.member(text[:70000 - 4720], extra=extra), B.EOF, B.EOF, B.member(text[:10], after_bc=B.subfield(b"QQ", b"12345")), B.member(b"")]
    for ms in (members, members[1:2], members[:3], members[1:] + [B.EOF]):                                      # EOF markers first, in the middle, last, absent
        data = b"".join(ms)
        for last in (False, True):
            w = same_walk(data, last)
            assert w["stop"] == B.WHOLE and w["n_members"] == len(ms)
    assert same_walk(b"", True)["n_members"] == 0
    assert same_walk(bgzf_check.python_bgzf(text[:100000]), True)["n_members"] == 5


def test_walk_of_ranges_that_end_inside_a_member(built, text):
    first = B.member(text[:30000], extra=B.subfield(b"AB", b"cd"))
    data = first + B.member(text[30000:50000]) + B.EOF
    head = 12 + 6 + 6                                             # the second member's header
    for cut in (len(first) + 1, len(first) + 3, len(first) + 11, len(first) + 13, len(first) + head - 1, len(first) + head, len(first) + head + 500,
                len(data) - len(B.EOF) - 8, len(data) - len(B.EOF) - 1, len(data) - 1, 2, 17):
        w = same_walk(data[:cut], False)                          # more of the file follows: not consumed
        assert w["stop"] == B.PARTIAL and w["consumed"] in (0, len(first), len(data) - len(B.EOF))
        w = same_walk(data[:cut], True)                           # the range ends the file: truncated
        assert w["stop"] == B.TRUNCATED
    from leon_amd import capi
    assert capi.host_bgzf_members(data, last=True, off_cap=3)["rc"] == -5       # the table has no room for the last entry
    assert capi.host_bgzf_members(data, last=True, off_cap=4)["rc"] == 0


def test_walk_meets_members_that_are_not_bgzf(built, text):
    plain = gzip.compress(text[:5000])
    good = B.member(text[:5000])
    no_bc = B.frame(B.deflate_raw(text[:100]), 0, 100)
    no_bc = no_bc[:12] + b"XC" + no_bc[14:]                       # FLG 4 and a subfield, but not B C
    small = B.frame(b"\x03\x00", 0, 0, bsize=24)                  # BSIZE + 1 = 25 bytes: less than its own header and trailer (26)
    flg = bytearray(good); flg[3] = 12                            # FLG 4 | FNAME
    subfield_overruns = B.frame(b"\x03\x00", 0, 0, extra=b"XY\xff\x00")
    for foreign in (plain, no_bc, small, bytes(flg), subfield_overruns, b"@read\nACGT\n+\nIIII\n", b"\x1f\x8b\x08"[:2] + b"\x07"):
        for front in ([], [good], [good, B.EOF, good]):
            data = b"".join(front) + foreign + good
            for last in (False, True):
                w = same_walk(data, last)
                assert w["stop"] == B.FOREIGN and w["n_members"] == len(front) and w["consumed"] == sum(len(m) for m in front), (foreign[:20], w)


def test_host_inflate_against_gzip(built, text):
    from leon_amd import capi
    t = B.match_text(2)
    members = [B.member(text[:s], level=l, strategy=st) for s, l, st in ((65536, 6, zlib.Z_DEFAULT_STRATEGY), (65280, 0, zlib.Z_DEFAULT_STRATEGY), (1, 9, zlib.Z_FIXED),
                                                                        (0, 6, zlib.Z_DEFAULT_STRATEGY), (32769, 1, zlib.Z_RLE), (1025, 6, zlib.Z_HUFFMAN_ONLY))]
    members += [B.EOF, B.member(t[:60000], level=9, flush_at=777), B.token_member([t[:32768], (258, 32768), (100, 1)])[0]]
    data = b"".join(members)
    for threads in (1, 3, 0):
        assert capi.host_bgzf_inflate(data, B.offsets_of(data), n_threads=threads) == gzip.decompress(data)
    assert capi.host_bgzf_inflate(None, None, n_members=0) == b""
    data = bgzf_check.python_bgzf(text)
    assert capi.host_bgzf_inflate(data, B.offsets_of(data)) == text


def test_host_inflate_refusals_name_the_smallest_member(built, text):
    from leon_amd import capi
    part = text[:9000]
    pay, crc = B.deflate_raw(part), zlib.crc32(part)
    good = B.member(text[:4000])
    damaged = [B.frame(pay, crc ^ 1, len(part)), B.frame(pay, crc, len(part) + 1), B.frame(pay, zlib.crc32(part[:-1]), len(part) - 1), B.frame(pay + b"\0", crc, len(part)),
               B.frame(pay[:-3], crc, len(part)), B.frame(b"\x07", 0, 0), B.frame(pay, crc, 65537)]
    for bad in damaged:
        with pytest.raises((zlib.error, EOFError, OSError, AssertionError)):
            assert gzip.decompress(bad) == part and len(bad) == 26 + len(pay)      # (gzip does not look for slack in front of the trailer: the size does)
        for members, n in (([good, bad, good], 1), ([good, good, good, bad, bad], 3), ([bad], 0)):
            data = b"".join(members)
            off = np.cumsum([0] + [len(m) for m in members]).astype(np.uint64)
            for threads in (1, 4):
                with pytest.raises(capi.LeonDnaError) as e:
                    capi.host_bgzf_inflate(data, off, n_threads=threads)
                assert e.value.code == -1 and str(e.value).endswith("BGZF member %d (at byte %d) does not decode" % (n, int(off[n]))), str(e.value)
    # a table that does not cut the bytes at the members: the member it names does not decode
    data = good + good
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_bgzf_inflate(data, [0, len(good) - 1, len(data)])
    assert "BGZF member 0 (at byte 0) does not decode" in str(e.value)
    # arguments
    for off, word in (([0, len(data) + 1], "end behind the bytes given"), ([len(good), 0], "not monotonic")):
        with pytest.raises(capi.LeonDnaError) as e:
            capi.host_bgzf_inflate(data, off)
        assert e.value.code == -1 and word in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_bgzf_inflate(data, [0, len(good), len(data)], text_cap=7999)
    assert e.value.code == -5 and e.value.n_text == 8000 and "needs 8000 bytes" in str(e.value)


def test_device_call_refuses_its_arguments_before_a_device(built, text):
    """the host function's refusals, in its words, with a d_text no device call could survive"""
    from leon_amd import capi
    good = B.member(text[:4000])
    data = good + good
    for off, cap in (([0, len(data) + 1], 8000), ([len(good), 0], 8000), ([0, len(good), len(data)], 7999)):
        with pytest.raises(capi.LeonDnaError) as want:
            capi.host_bgzf_inflate(data, off, text_cap=cap)
        with pytest.raises(capi.LeonDnaError) as got:
            capi.bgzf_inflate_device(data, off, 0x10, cap)
        assert (got.value.code, str(got.value), got.value.n_text) == (want.value.code, str(want.value), want.value.n_text)
    assert capi.bgzf_inflate_device(None, None, 0x10, 0, n_members=0) == (0, 0)
    if capi.device_count() == 0:                                  # (the library's own count: what the call itself would find)
        with pytest.raises(capi.LeonDnaError) as e:               # no device: a status, not a fallback
            capi.bgzf_inflate_device(data, [0, len(good), len(data)], 0x10, 8000)
        assert e.value.code in (-2, -3), (e.value.code, str(e.value))


def test_walk_and_inflate_under_asan_ubsan(tmp_path):
    """a stand-alone program (its own main) with host_streams.cpp, both compiled with the sanitizers; run as a child process"""
    exe = str(tmp_path / "bgzf_fuzz_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "bgzf_fuzz_check.cpp"),
                           os.path.join(ROOT, "leon_amd", "csrc", "host_streams.cpp"), "-lz", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bgzf fuzz: ok" in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]


def test_cli_refusals_that_need_no_device(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.fastq.gz")
    for args, word in ((["-c", "-input-inflate", "gpu"], "'gpu'"), (["-c", "-input-inflate"], "needs a value"), (["-d", "-input-inflate", "device"], "belongs to -c")):
        r = subprocess.run([leon, "-file", nothing] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.startswith("EXCEPTION: ") and "-input-inflate" in r.stderr and word in r.stderr, (args, r.stderr)
    # `host` is the way without the option: it gets as far as the file, which is not there
    r = subprocess.run([leon, "-file", nothing, "-c", "-input-inflate", "host"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: cannot open"), r.stderr
