"""No GPU: leon_fastq_split_device and its host twin leon_host_fastq_split are declared in include/leon_dna.h, bound by
the Python binding and exported by the library, the ABI version stays 5; the restatement of tests/fastq_shapes.py gives what its designed
texts were put together to give; the host twin gives what the restatement gives on every case, refuses bad arguments in its words and
reports capacities that are too small; and host_fastq.h passes the same cases in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fastq_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, TWIN = "leon_fastq_split_device", "leon_host_fastq_split"


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


@pytest.fixture(scope="module")
def expected():
    return {name: S.split(*case) for name, case in S.CASES.items()}


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    raw = C.CDLL(capi.lib_path())
    assert ("int %s(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, int plus_kind, uint8_t* d_headers, "
            "uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint8_t* d_quals, uint64_t bytes_cap, uint64_t records_cap, "
            "leon_fastq_split_result* res);" % NAME) in flat
    assert ("int %s(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, int plus_kind, uint8_t* headers, uint64_t* header_off, "
            "uint8_t* bases, uint64_t* base_off, uint8_t* quals, uint64_t bytes_cap, uint64_t records_cap, leon_fastq_split_result* res);" % TWIN) in flat
    for name in (NAME, TWIN):
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert callable(capi.fastq_split_device) and callable(capi.host_fastq_split)
    assert C.sizeof(capi.FastqSplitResult) == 56
    # the constants of the header, of the binding and of the restatement are the same
    for name, value in (("MAX", S.MAX), ("END", S.END), ("IRREGULAR", S.IRREGULAR), ("R_NONE", S.R_NONE), ("R_HEADER", S.R_HEADER), ("R_PLUS", S.R_PLUS),
                        ("R_LENGTH", S.R_LENGTH), ("R_PLUS_TEXT", S.R_PLUS_TEXT), ("R_PARTIAL", S.R_PARTIAL)):
        assert re.search(r"#define\s+LEON_FASTQ_%s\s+%du\b" % (name, value), src), name
        assert getattr(capi, "FASTQ_" + name) == value
    kernels = open(os.path.join(ROOT, "leon_amd", "csrc", "kernels.h")).read()
    assert re.search(r"FASTQ_TILE\s*=\s*%d\b" % S.TILE, kernels) and re.search(r"FASTQ_MAX_GROUPS\s*=\s*%d\b" % S.MAX_GROUPS, kernels)
    assert (capi.FASTQ_TILE, capi.FASTQ_MAX_GROUPS) == (S.TILE, S.MAX_GROUPS)


def test_the_restatement_on_the_designed_texts(expected):
    assert len(S.CASES) > 100
    for name, (n, consumed, stop, reason) in S.KNOWN.items():
        e = expected[name]
        assert (e["n_records"], e["stop"], e["reason"]) == (n, stop, reason), name
        if consumed is not None:
            assert e["consumed"] == consumed, name
    for name, e in expected.items():
        text, last, max_records, _ = S.CASES[name]
        assert e["n_records"] <= max_records and e["consumed"] <= len(text)
        assert (e["stop"] == S.IRREGULAR) == (e["reason"] != S.R_NONE), name
        assert len(e["quals"]) == len(e["bases"]) == e["base_off"][-1] and len(e["headers"]) == e["header_off"][-1], name
        if e["stop"] == S.END and last:
            assert e["consumed"] == len(text), name
    # what the texts are there for
    assert len(S.CASES["past_the_grid_cap"][0]) == (S.MAX_GROUPS + 1) * S.TILE
    assert [len(S.CASES[n][0]) for n in ("tile", "tile_minus_1", "tile_plus_1", "two_tiles")] == [S.TILE, S.TILE - 1, S.TILE + 1, 2 * S.TILE]
    assert S.CASES["newline_ends_tile"][0][S.TILE - 1] == 10 and S.CASES["newline_begins_tile"][0][S.TILE] == 10
    assert S.CASES["crlf_across_tiles"][0][S.TILE - 1:S.TILE + 1] == b"\r\n"
    assert max(b - a for a, b in zip(expected["long_sequence"]["base_off"], expected["long_sequence"]["base_off"][1:])) > S.TILE
    for name in ("tile", "two_tiles", "past_the_grid_cap", "newline_ends_tile", "crlf_across_tiles", "long_sequence", "sequence_lengths"):
        assert expected[name]["stop"] == S.END and expected[name]["consumed"] == len(S.CASES[name][0]), name
    assert sum(len(c[0]) for n, c in S.CASES.items() if n.startswith("mix_")) < 600 << 10


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_the_host_twin_on_every_case(built, expected, name):
    from leon_amd import capi
    text, last, max_records, plus_kind = S.CASES[name]
    e = expected[name]
    res, headers, header_off, bases, base_off, quals = capi.host_fastq_split(text, last, max_records, plus_kind)
    assert res == {k: e[k] for k in S.RESULT_FIELDS}
    assert headers == e["headers"] and bases == e["bases"] and quals == e["quals"]
    assert header_off.tolist() == e["header_off"] and base_off.tolist() == e["base_off"]


def test_the_host_twin_reports_what_it_needs(built, expected):
    from leon_amd import capi
    for name in ("records_65", "crlf_everywhere", "plus_other_text_middle"):
        text, last, max_records, plus_kind = S.CASES[name]
        e = expected[name]
        want = {k: e[k] for k in S.RESULT_FIELDS}
        for kw in (dict(records_cap=e["n_records"]), dict(bytes_cap=max(e["header_bytes"], e["base_bytes"]) - 1), dict(records_cap=0, bytes_cap=0)):
            with pytest.raises(capi.LeonDnaError) as err:
                capi.host_fastq_split(text, last, max_records, plus_kind, **kw)
            assert err.value.code == -5 and err.value.result == want, (name, kw, str(err.value))
        got = capi.host_fastq_split(text, last, max_records, plus_kind, records_cap=e["n_records"] + 1, bytes_cap=max(e["header_bytes"], e["base_bytes"]))
        assert got[0] == want and got[3] == e["bases"]


def test_arguments_are_refused_with_their_words_before_a_device(built):
    from leon_amd import capi
    lib = capi.load_library()
    res = capi.FastqSplitResult()
    R = C.byref(res)
    fake = 1 << 20                                                # never dereferenced: the checks come first
    for args, words in (((fake, 5, 1, 9, -1, fake, fake, fake, fake, fake, 5, 3, None), "res is NULL"),
                        ((fake, 1 << 32, 1, 9, -1, fake, fake, fake, fake, fake, 5, 3, R), "n_text is 2^32 or more"),
                        ((0, 5, 1, 9, -1, fake, fake, fake, fake, fake, 5, 3, R), "text is NULL with text given"),
                        ((fake, 5, 1, 9, 2, fake, fake, fake, fake, fake, 5, 3, R), "plus_kind is none of -1, 0, 1"),
                        ((fake, 5, 1, 9, -2, fake, fake, fake, fake, fake, 5, 3, R), "plus_kind is none of -1, 0, 1"),
                        ((fake, 5, 1, 9, 0, 0, fake, fake, fake, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, 0, fake, fake, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, fake, 0, fake, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, fake, fake, 0, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, fake, fake, fake, 0, 5, 3, R), "a NULL output")):
        for name, call in ((NAME, lambda *a: lib.leon_fastq_split_device(0, *a)), (TWIN, lib.leon_host_fastq_split)):
            rc = call(*args)
            msg = (lib.leon_last_error(None) or b"").decode()
            assert rc == -1 and msg == name + ": fastq split: " + words, (rc, msg, words)


def test_host_fastq_h_under_asan_ubsan(expected, tmp_path):
    """a stand-alone program (its own main) that includes host_fastq.h, compiled with the sanitizers and run as a child process on every case"""
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<Q", len(S.CASES)))
        for name in sorted(S.CASES):
            text, last, max_records, plus_kind = S.CASES[name]
            e = expected[name]
            f.write(struct.pack("<QQQq", len(text), last, max_records, plus_kind) + text)
            f.write(struct.pack("<8Q", *(e[k] for k in S.RESULT_FIELDS)))
            f.write(e["headers"] + np.array(e["header_off"], dtype="<u8").tobytes() + e["bases"] + np.array(e["base_off"], dtype="<u8").tobytes() + e["quals"])
    exe = str(tmp_path / "fastq_split_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "fastq_split_check.cpp")])
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "fastq split: ok (%d cases)" % len(S.CASES) in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
