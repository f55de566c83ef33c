"""No GPU: leon_text_bgzf_device_ex is declared in include/leon_dna.h, bound by the Python binding and exported by the
library, the ABI version stays 5; an unknown bit of flags is refused with the arguments' refusals before a device is touched; and
`-gz-matches` belongs to -gz."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "leon_text_bgzf_device_ex"


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def test_entry_point_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    raw = C.CDLL(capi.lib_path())
    assert ("int %s(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records, int last, "
            "leon_piece_sink sink, void* user, uint64_t* n_taken, uint64_t* out_bytes, uint64_t* member_out_off, uint64_t* member_text_off, "
            "uint64_t members_cap, uint64_t* n_members, uint32_t flags);" % NAME) in flat
    assert re.search(r"#define\s+LEON_BGZF_F_MATCHES\s+1u\b", src) and capi.BGZF_F_MATCHES == 1
    assert NAME in capi._EXPORTS and NAME in capi.EXPORTED_SYMBOLS and hasattr(raw, NAME)
    assert capi._EXPORTS[NAME][1] == capi._EXPORTS["leon_text_bgzf_records_device"][1] + [C.c_uint32]
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # an addition
    assert callable(capi.text_bgzf_device_ex)


def test_flags_and_arguments_are_refused_before_a_device(built):
    from leon_amd import capi
    lib = capi.load_library()
    calls = []
    sink = capi.PIECE_SINK(lambda user, offset, address, size: calls.append((offset, size)) or 0)
    t, o, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
    T, O, M = C.byref(t), C.byref(o), C.byref(m)
    fake = 1 << 20                                                # never dereferenced on the host: the device is asked only after the checks

    def call(d_text, n_head, n_body, d_rec_off, n_records, last, sink, taken, out_bytes, members, flags):
        rc = lib.leon_text_bgzf_device_ex(0, C.c_void_p(d_text), n_head, n_body, C.c_void_p(d_rec_off), n_records, last, sink, None, taken, out_bytes,
                                          None, None, 0, members, flags)
        return rc, (lib.leon_last_error(None) or b"").decode()
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
        for args in ((fake, 0, 5, fake, 1, 1), (fake, 0, 32768, 0, 0, 1), (0, 0, 0, 0, 0, 1)):      # record mode, the fixed cuts, no text at all
            assert call(*args, sink, T, O, M, flags) == (-1, NAME + ": unknown bits in flags")
    # the older refusals, in this entry's name, whatever the flags
    for flags in (0, 1):
        assert call(0, 0, 5, fake, 1, 1, sink, T, O, M, flags) == (-1, NAME + ": d_text is NULL with text given")
        assert call(fake, 0, 5, fake, 1, 2, sink, T, O, M, flags) == (-1, NAME + ": bgzf records: last is neither 0 nor 1")
        assert call(fake, 0, 5, fake, 1, 1, sink, T, O, None, flags) == (-1, NAME + ": n_members is NULL")
    assert calls == []


def test_cli_option_belongs_to_gz(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.fastq")
    for args in (["-d", "-gz-matches"], ["-gz-matches", "-d", "-gz-records"], ["-c", "-gz-matches"]):
        r = subprocess.run([leon, "-file", nothing + ".leon"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.splitlines()[0].startswith("EXCEPTION: option -gz"), r.stderr
    r = subprocess.run([leon, "-file", nothing + ".leon", "-d", "-gz-matches"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: option -gz-matches belongs to -gz"], r.stderr
    # beside -d -gz it is accepted: the run gets as far as the file, which is not there, and leaves nothing behind
    r = subprocess.run([leon, "-file", nothing + ".leon", "-d", "-gz", "-gz-matches", "-gz-records", "-gz-index"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-gz" not in r.stderr and "nothing.fastq.leon" in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []
