"""No GPU: leon_text_bgzf_device is declared in include/leon_dna.h with LEON_BGZF_MEMBER_TEXT, bound by the Python binding and exported
by the library, the ABI version stays 5; its arguments are refused with their words before a device is touched and a well-formed call
fails without one; `leon -gz` belongs to -d and is refused beside -c while the options are parsed; and tests/bgzf_check.py, which the
GPU tests judge the output with, accepts the layout as zlib writes it and refuses a stream that is damaged."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_check as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "leon_text_bgzf_device"


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def test_entry_point_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    raw = C.CDLL(capi.lib_path())
    assert re.search(r"\bint\s+%s\s*\(\s*int\s+device_id\s*,\s*const\s+uint8_t\s*\*\s*d_text\s*,\s*uint64_t\s+n_text\s*,\s*int\s+last\s*,\s*leon_piece_sink\s+sink\s*,"
                     r"\s*void\s*\*\s*user\s*,\s*uint64_t\s*\*\s*n_taken\s*,\s*uint64_t\s*\*\s*out_bytes\s*,\s*uint64_t\s*\*\s*n_members\s*\)\s*;" % NAME, src)
    assert NAME in capi._EXPORTS and NAME in capi.EXPORTED_SYMBOLS
    assert hasattr(raw, NAME), "libleon_dna.so does not export " + NAME
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert re.search(r"#define\s+LEON_BGZF_MEMBER_TEXT\s+32768u?\b", src)
    assert capi.BGZF_MEMBER_TEXT == 32768 == B.MEMBER_TEXT and capi.BGZF_EOF == B.EOF
    assert callable(capi.text_bgzf_device)


def test_cli_option_belongs_to_d(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.fastq")
    for args in (["-c", "-gz"], ["-gz", "-c"]):
        r = subprocess.run([leon, "-file", nothing] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.splitlines() == ["EXCEPTION: option -gz belongs to -d"], r.stderr
    # beside -d the option is accepted: the run gets as far as the file, which is not there, and leaves nothing behind
    r = subprocess.run([leon, "-file", nothing + ".leon", "-d", "-gz"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-gz" not in r.stderr and "nothing.fastq.leon" in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def _call(lib, d_text, n_text, last, sink, taken, out_bytes, members=None):
    rc = lib.leon_text_bgzf_device(0, C.c_void_p(d_text), n_text, last, sink, None, taken, out_bytes, members)
    return rc, (lib.leon_last_error(None) or b"").decode()


def test_arguments_are_refused_with_their_words_before_a_device(built):
    from leon_amd import capi
    lib = capi.load_library()
    calls = []
    sink = capi.PIECE_SINK(lambda user, offset, address, size: calls.append((offset, size)) or 0)
    t, o = C.c_uint64(), C.c_uint64()
    fake = 1 << 20                                                # never dereferenced on the host: the device is asked only after the checks
    for args, words in (((0, 5, 1, sink, C.byref(t), C.byref(o)), "d_text is NULL with n_text != 0"),
                        ((fake, 5, 1, capi.PIECE_SINK(), C.byref(t), C.byref(o)), "sink is NULL"),
                        ((fake, 5, 1, sink, None, C.byref(o)), "n_taken is NULL"),
                        ((fake, 5, 1, sink, C.byref(t), None), "out_bytes is NULL"),
                        ((fake, 5, 2, sink, C.byref(t), C.byref(o)), "last is neither 0 nor 1"),
                        ((fake, 5, -1, sink, C.byref(t), C.byref(o)), "last is neither 0 nor 1")):
        rc, msg = _call(lib, *args)
        assert rc == -1 and msg == NAME + ": " + words, (rc, msg)
    assert calls == []


def test_nothing_to_compress_needs_no_device(built):
    from leon_amd import capi
    got, taken, members = capi.text_bgzf_device(0, 0, last=1)
    assert (got, taken, members) == (B.EOF, 0, 0)
    assert B.check(got, b"") == []
    for n in (0, 1, 32767):                                       # below one member without `last`: all of it is the caller's carry
        got, taken, members = capi.text_bgzf_device(1 << 20, n, last=0, sink=lambda offset, size: pytest.fail("the sink was called"))
        assert (got, taken, members) == (b"", 0, 0)


def test_no_device_no_members(built):
    import torch
    from leon_amd import capi
    if torch.cuda.is_available():
        return
    for n, last in ((5, 1), (32768, 0), (100000, 0)):
        with pytest.raises(capi.LeonDnaError) as e:
            capi.text_bgzf_device(1 << 20, n, last=last)
        assert e.value.code in (-2, -3), e.value


def test_the_checker_takes_zlibs_members_and_refuses_damage():
    rng = np.random.default_rng(5)
    text = (b"@SRR1.7 x\nACGTTGCA\n+\nIIIIHHGG\n" * 3000)[:65536] + rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    out = B.python_bgzf(text)
    sizes = B.check(out, text)
    assert len(sizes) == 4 and sizes[0] < 4000 and max(sizes) == 32768 + 5       # compressible members, and a stored one
    assert B.check(B.python_bgzf(b""), b"") == []
    members = B.walk(out)
    at, size = members[1]
    for pos, why in ((at + 3, "flags"), (at + 12, "subfield id"), (at + 16, "BSIZE"), (at + 40, "payload"), (at + size - 6, "CRC32"), (at + size - 2, "ISIZE"),
                     (len(out) - 10, "EOF marker")):
        bad = bytearray(out)
        bad[pos] ^= 0x10
        with pytest.raises((AssertionError, zlib.error, OSError, EOFError)):
            B.check(bytes(bad), text)
    with pytest.raises(AssertionError):
        B.check(out[:-28], text)                                  # no EOF marker
    with pytest.raises(AssertionError):
        B.check(out, text[:-1])
    assert B.check(out[:-28], text, eof=False) == sizes
