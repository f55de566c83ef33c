"""No GPU: the three BAM entry points are declared, bound and exported, the ABI version stays 5; leon_bam_header and
leon_host_records_bam write what tests/bam_records.py's restatement of the format writes, on the calls of tests/bam_cases.py, refuse what
it refuses in its words, and the restatement's own parser gives back what went in; `-bam`'s option rules."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_cases
import bam_records as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("leon_records_bam_device", "leon_host_records_bam", "leon_bam_header")


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def host_format(capi, reads, heads, quals, fastq, first, **kw):
    """leon_host_records_bam on a case; the header offsets count from a set's first byte, not from 0"""
    hdr_text = hdr_off = None
    if heads is not None:
        hdr_text = b"".join(heads)
        hdr_off = 1000 + np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)
    kw.setdefault("hdr_off", hdr_off)
    return capi.host_records_bam(b"".join(reads), [len(s) for s in reads], fastq=fastq, first_read_index=first, hdr_text=hdr_text,
                                 quals=None if quals is None else b"".join(quals), **kw)


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    raw = C.CDLL(capi.lib_path())
    assert ("int leon_records_bam_device(int device_id, const leon_record_layout* lay, const uint8_t* d_bases, const uint32_t* d_len, uint64_t n_reads, "
            "uint64_t n_bases, const uint8_t* d_hdr_text, const uint64_t* d_hdr_off, const uint8_t* d_quals, uint8_t* d_out, uint64_t out_cap, "
            "uint64_t* d_rec_off, uint64_t* out_size);") in flat
    assert "int leon_bam_header(uint8_t* out, uint64_t cap, uint64_t* size);" in flat
    assert re.search(r"int leon_host_records_bam\(const leon_record_layout\* lay, [^;]*uint32_t n_threads\);", flat)
    for name in NAMES:
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS, name + " is not bound"
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert callable(capi.records_bam_device) and callable(capi.host_records_bam) and callable(capi.bam_header)


def test_the_restatement_on_a_record_written_out_by_hand():
    """the yardstick itself, against bytes put together here field by field"""
    assert B.bam_header() == b"BAM\x01\x17\x00\x00\x00@HD\tVN:1.6\tSO:unsorted\n\x00\x00\x00\x00"
    rec = B.bam_record(b"ACGTn", b"r1 first read", b"!I5~#", 0)
    body = (b"\xff\xff\xff\xff" * 2 + bytes([3, 0]) + struct.pack("<H", 4680) + struct.pack("<HH", 0, 4) + struct.pack("<I", 5) + b"\xff\xff\xff\xff" * 2 +
            b"\0\0\0\0" + b"r1\0" + bytes([0x12, 0x48, 0xF0]) + bytes([0, 40, 20, 93, 2]) + b"COZfirst read\0")
    assert rec == struct.pack("<i", len(body)) + body
    assert len(B.bam_record(b"", b"", b"", 0)) == 38
    assert B.bam_record(b"", b"", b"", 0)[36:] == b"*\0"
    assert B.bam_record(b"A", None, None, 1234)[36:] == b"1234\0\x10\xff"


def test_header(built):
    from leon_amd import capi
    assert capi.bam_header() == B.bam_header()
    lib = capi.load_library()
    size = C.c_uint64()
    buf = np.full(64, 0xA5, dtype=np.uint8)
    assert lib.leon_bam_header(C.c_void_p(buf.ctypes.data), len(B.bam_header()) - 1, C.byref(size)) == -5
    assert size.value == len(B.bam_header()) and (buf == 0xA5).all()
    assert lib.leon_bam_header(None, 0, C.byref(size)) == -5 and size.value == len(B.bam_header())
    assert lib.leon_bam_header(C.c_void_p(buf.ctypes.data), 64, None) == -1


@pytest.mark.parametrize("case", bam_cases.cases(), ids=lambda c: c[0])
def test_host_records_against_the_restatement(built, case):
    from leon_amd import capi
    what, reads, heads, quals, fastq, first = case
    want, want_off = B.bam_records(reads, heads, quals if fastq else None, first)
    for n_threads in (1, 3):
        got, rec_off = host_format(capi, reads, heads, quals, fastq, first, n_threads=n_threads)
        assert len(got) == len(want), (what, len(got), len(want))
        if got != want:
            i = next(j for j in range(len(want)) if got[j] != want[j])
            raise AssertionError("%s: the records differ at byte %d of %d: %r != %r" % (what, i, len(want), got[max(0, i - 20):i + 20], want[max(0, i - 20):i + 20]))
        assert list(rec_off) == want_off, what
    # ... and the restatement's own parser gives back what went in
    parsed = B.parse_bam(B.bam_header() + want)
    assert len(parsed) == len(reads)
    for r, (name, seq, qual, comment) in enumerate(parsed):
        want_name, want_comment = B.name_and_comment(heads[r]) if heads is not None else (b"%d" % (first + r), None)
        assert (name, comment) == (want_name or b"*", want_comment), (what, r)
        assert seq == B.fold(reads[r]), (what, r)
        if quals is not None and fastq:
            assert qual == quals[r] or (qual is None and quals[r] == b"\xff" * len(quals[r])), (what, r)
        else:
            assert qual is None or not reads[r], (what, r)


def test_parser_gives_back_the_comment_bytes_verbatim():
    heads = [b"a b", b"a\tb", b"a  b", b"a \tb ", b"a", b" b", b"a "]
    data, _ = B.bam_records([b"AC"] * len(heads), heads, [b"II"] * len(heads))
    assert [(n, c) for n, _, _, c in B.parse_bam(B.bam_header() + data)] == [(b"a", b"b"), (b"a", b"b"), (b"a", b" b"), (b"a", b"\tb "), (b"a", None),
                                                                                (b"*", b"b"), (b"a", None)]


def test_host_refusals_in_the_restatements_words(built):
    from leon_amd import capi
    for what, reads, heads, quals, first, read, nbytes in bam_cases.name_refusals():
        with pytest.raises(B.BamRefusal) as want:
            B.bam_records(reads, heads, quals, first)
        assert want.value.read == read
        with pytest.raises(capi.LeonDnaError) as e:
            host_format(capi, reads, heads, quals, True, first)
        assert e.value.code == -1 and str(e.value).endswith("leon_host_records_bam: " + str(want.value)), (what, str(e.value))
        assert "read %d: its name has %d bytes, BAM allows 254" % (read, nbytes) in str(e.value)
    for what, reads, heads, quals, first, read in bam_cases.quality_refusals():
        with pytest.raises(B.BamRefusal) as want:
            B.bam_records(reads, heads, quals, first)
        assert want.value.read == read
        for n_threads in (1, 4):
            with pytest.raises(capi.LeonDnaError) as e:
                host_format(capi, reads, heads, quals, True, first, n_threads=n_threads)
            assert e.value.code == -1 and str(e.value).endswith("leon_host_records_bam: read %d: a quality byte below 33" % read), (what, str(e.value))
    # a name refusal comes before a quality refusal, whichever read is the smaller
    what, reads, heads, quals, first, read, nbytes = bam_cases.name_refusals()[0]
    quals = [b" " * len(q) for q in quals]
    with pytest.raises(capi.LeonDnaError) as e:
        host_format(capi, reads, heads, quals, True, first)
    assert "its name has 255 bytes" in str(e.value)


def test_host_refusals_of_the_arguments(built):
    from leon_amd import capi
    what, reads, heads, quals, fastq, first = bam_cases.cases()[0]
    want, _ = B.bam_records(reads, heads, quals, first)
    n = len(reads)
    with pytest.raises(capi.LeonDnaError) as e:                    # a byte short: the need
        host_format(capi, reads, heads, quals, True, first, out_cap=len(want) - 1)
    assert e.value.code == -5 and e.value.out_size == len(want) and "need %d bytes" % len(want) in str(e.value)
    for delta in (-1, 1, 1000):
        with pytest.raises(capi.LeonDnaError) as e:
            host_format(capi, reads, heads, quals, True, first, n_bases=sum(map(len, reads)) + delta)
        assert e.value.code == -1 and "add up" in str(e.value)
    good = 1000 + np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)
    back = good.copy()
    back[2], back[3] = good[3], good[2]
    with pytest.raises(capi.LeonDnaError) as e:
        host_format(capi, reads, heads, quals, True, first, hdr_off=back)
    assert e.value.code == -1 and "backwards" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        host_format(capi, reads, heads, quals, True, first, hdr_bytes=int(good[n] - good[0]) + 1)
    assert e.value.code == -1 and "do not end" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        host_format(capi, reads, heads, quals, True, first, struct_size=C.sizeof(capi.RecordLayout) + 8)
    assert e.value.code == -1 and "struct_size" in str(e.value)
    got, _ = host_format(capi, reads, heads, quals, True, first)     # and the library still formats after all that
    assert got == want


def test_cli_option_rules(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.fastq")
    for args, words in ((["-c", "-bam"], "option -bam belongs to -d"),
                        (["-bam", "-c"], "option -bam belongs to -d"),
                        (["-d", "-gz", "-bam"], "options -gz and -bam name two output formats"),
                        (["-d", "-bam", "-gz", "-gz-records"], "options -gz and -bam name two output formats"),
                        (["-d", "-bam", "-test-file"], "option -test-file compares text: not with -bam"),
                        (["-d", "-gz-records"], "option -gz-records belongs to -gz"),
                        (["-d", "-gz-index"], "option -gz-index belongs to -gz"),
                        (["-d", "-gz-matches"], "option -gz-matches belongs to -gz")):
        r = subprocess.run([leon, "-file", nothing] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: " + words], (args, r.stderr)
    # beside -d -bam the three are accepted: the run gets as far as the file, which is not there, and leaves nothing behind
    r = subprocess.run([leon, "-file", nothing + ".leon", "-d", "-bam", "-gz-records", "-gz-index", "-gz-matches"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "belongs" not in r.stderr and "nothing.fastq.leon" in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_host_form_under_asan_ubsan(tmp_path):
    """a stand-alone program (its own main) with host_streams.cpp, both compiled with the sanitizers; run as a child process"""
    exe = str(tmp_path / "bam_records_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "bam_records_check.cpp"),
                           os.path.join(ROOT, "leon_amd", "csrc", "host_streams.cpp"), "-lz", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bam records: ok" in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
