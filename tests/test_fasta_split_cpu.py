"""No GPU: leon_fasta_split_device and its host twin leon_host_fasta_split are declared in include/leon_dna.h, bound by
the Python binding and exported by the library, the ABI version stays 5; the restatement of tests/fasta_shapes.py gives what its designed
texts were put together to give; the host twin gives what the restatement gives on every case, refuses bad arguments in its words and
reports capacities that are too small; host_fasta.h passes the same cases in a stand-alone program under AddressSanitizer and UBSan; and
the restatement is held against Bank itself: the reader's hand-off rule replayed over it gives the reads, the hashes and the line width
`leon -selftest-bank` prints for the same file."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fasta_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")
NAME, TWIN = "leon_fasta_split_device", "leon_host_fasta_split"


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
    assert ("int %s(int device_id, const uint8_t* d_text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* d_headers, "
            "uint64_t* d_header_off, uint8_t* d_bases, uint64_t* d_base_off, uint64_t bytes_cap, uint64_t records_cap, "
            "leon_fasta_split_result* res);" % NAME) in flat
    assert ("int %s(const uint8_t* text, uint64_t n_text, int last, uint64_t max_records, uint64_t wrap, uint8_t* headers, uint64_t* header_off, "
            "uint8_t* bases, uint64_t* base_off, uint64_t bytes_cap, uint64_t records_cap, leon_fasta_split_result* res);" % TWIN) in flat
    for name in (NAME, TWIN):
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert callable(capi.fasta_split_device) and callable(capi.host_fasta_split)
    assert C.sizeof(capi.FastaSplitResult) == 56
    # the constants of the header, of the binding and of the restatement are the same
    for name, value in (("MAX", S.MAX), ("END", S.END), ("IRREGULAR", S.IRREGULAR), ("R_NONE", S.R_NONE), ("R_HEADER", S.R_HEADER),
                        ("R_NO_SEQUENCE", S.R_NO_SEQUENCE), ("R_EMPTY_LINE", S.R_EMPTY_LINE), ("R_WIDTH", S.R_WIDTH), ("R_MULTILINE", S.R_MULTILINE)):
        assert re.search(r"#define\s+LEON_FASTA_%s\s+%du\b" % (name, value), src), name
        assert getattr(capi, "FASTA_" + name) == value
    assert re.search(r"#define\s+LEON_FASTA_ANY_WIDTH\s+\(~\(uint64_t\)0\)", src) and capi.FASTA_ANY_WIDTH == S.ANY == 2 ** 64 - 1
    kernels = open(os.path.join(ROOT, "leon_amd", "csrc", "kernels.h")).read()
    assert re.search(r"FASTQ_TILE\s*=\s*%d\b" % S.TILE, kernels) and re.search(r"FASTQ_MAX_GROUPS\s*=\s*%d\b" % S.MAX_GROUPS, kernels)


def test_the_restatement_on_the_designed_texts(expected):
    assert len(S.CASES) > 200 and len(S.KNOWN) > 200
    for name, (n, consumed, stop, reason) in S.KNOWN.items():
        e = expected[name]
        assert (e["stop"], e["reason"]) == (stop, reason), name
        if n is not None:
            assert e["n_records"] == n, name
        if consumed is not None:
            assert e["consumed"] == consumed, name
    for name, e in expected.items():
        text, last, max_records, wrap = S.CASES[name]
        assert e["n_records"] <= max_records and e["consumed"] <= len(text)
        assert (e["stop"] == S.IRREGULAR) == (e["reason"] != S.R_NONE), name
        assert len(e["bases"]) == e["base_off"][-1] and len(e["headers"]) == e["header_off"][-1], name
        if e["stop"] == S.IRREGULAR:
            assert e["consumed"] < e["next_header"] <= len(text), name
            assert e["next_header"] == len(text) or text[e["next_header"]:e["next_header"] + 1] == b">", name
        else:
            assert e["next_header"] == 0, name
        if e["stop"] == S.END and last:
            assert e["consumed"] == len(text), name
        if text.startswith(b">"):                                # record n_records begins at a header line, or nothing is left
            assert e["consumed"] == len(text) or text[e["consumed"]:e["consumed"] + 1] == b">", name
        if not last and e["stop"] == S.END:                      # the last record is never taken without `last`
            assert text[e["consumed"]:].count(b"\n>") == 0, name
        if wrap == S.ANY:
            assert e["reason"] in (S.R_NONE, S.R_HEADER), name
    # what the texts are there for
    assert len(S.CASES["past_the_grid_cap"][0]) > (S.MAX_GROUPS + 1) * S.TILE
    e = expected["contig_of_5000_lines"]
    assert e["base_off"] == [0, 100, 100 + 300000, 300200] and e["single_max"] == 0
    assert max(b - a for a, b in zip(expected["line_longer_than_a_tile"]["base_off"], expected["line_longer_than_a_tile"]["base_off"][1:])) > S.TILE
    assert expected["line_longer_than_a_tile"]["single_max"] == S.TILE + 905
    assert expected["record_line_counts"]["single_max"] == 60 and expected["one_line_too_long_at_64_w60"]["single_max"] == 0
    assert sum(len(c[0]) for n, c in S.CASES.items() if n.startswith("mix_")) < 1 << 20
    mixes = {c[3] for n, c in S.CASES.items() if n.startswith("mix_")}
    assert S.ANY in mixes and len(mixes) >= 3                   # the draws run under a width and under any width


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_the_host_twin_on_every_case(built, expected, name):
    from leon_amd import capi
    text, last, max_records, wrap = S.CASES[name]
    e = expected[name]
    res, headers, header_off, bases, base_off = capi.host_fasta_split(text, last, max_records, wrap)
    assert res == {k: e[k] for k in S.RESULT_FIELDS}
    assert headers == e["headers"] and bases == e["bases"]
    assert header_off.tolist() == e["header_off"] and base_off.tolist() == e["base_off"]


OVERFLOW_CASES = ("records_65_w7", "crlf_everywhere", "inner_line_short_at_64_w60", "contig_of_5000_lines")


def test_the_host_twin_reports_what_it_needs(built, expected):
    from leon_amd import capi
    for name in OVERFLOW_CASES:
        text, last, max_records, wrap = S.CASES[name]
        e = expected[name]
        want = {k: e[k] for k in S.RESULT_FIELDS}
        for kw in (dict(records_cap=e["n_records"]), dict(bytes_cap=max(e["header_bytes"], e["base_bytes"]) - 1), dict(records_cap=0, bytes_cap=0)):
            with pytest.raises(capi.LeonDnaError) as err:
                capi.host_fasta_split(text, last, max_records, wrap, **kw)
            assert err.value.code == -5 and err.value.result == want, (name, kw, str(err.value))
            assert "leon_host_fasta_split: %d records need" % e["n_records"] in str(err.value)
        got = capi.host_fasta_split(text, last, max_records, wrap, records_cap=e["n_records"] + 1, bytes_cap=max(e["header_bytes"], e["base_bytes"]))
        assert got[0] == want and got[3] == e["bases"]


def test_arguments_are_refused_with_their_words_before_a_device(built):
    from leon_amd import capi
    lib = capi.load_library()
    res = capi.FastaSplitResult()
    R = C.byref(res)
    fake = 1 << 20                                                # never dereferenced: the checks come first
    for args, words in (((fake, 5, 1, 9, 0, fake, fake, fake, fake, 5, 3, None), "res is NULL"),
                        ((fake, 1 << 32, 1, 9, 0, fake, fake, fake, fake, 5, 3, R), "n_text is 2^32 or more"),
                        ((0, 5, 1, 9, 60, fake, fake, fake, fake, 5, 3, R), "text is NULL with text given"),
                        ((fake, 5, 1, 9, 0, 0, fake, fake, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, 0, fake, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, S.ANY, fake, fake, 0, fake, 5, 3, R), "a NULL output"),
                        ((fake, 5, 1, 9, 0, fake, fake, fake, 0, 5, 3, R), "a NULL output")):
        for name, call in ((NAME, lambda *a: lib.leon_fasta_split_device(0, *a)), (TWIN, lib.leon_host_fasta_split)):
            rc = call(*args)
            msg = (lib.leon_last_error(None) or b"").decode()
            assert rc == -1 and msg == name + ": fasta split: " + words, (rc, msg, words)


def test_host_fasta_h_under_asan_ubsan(expected, tmp_path):
    """a stand-alone program (its own main) that includes host_fasta.h, compiled with the sanitizers and run as a child process on every case"""
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<Q", len(S.CASES)))
        for name in sorted(S.CASES):
            text, last, max_records, wrap = S.CASES[name]
            e = expected[name]
            f.write(struct.pack("<QQQQ", len(text), last, max_records, wrap) + text)
            f.write(struct.pack("<8Q", *(e[k] for k in S.RESULT_FIELDS)))
            f.write(e["headers"] + np.array(e["header_off"], dtype="<u8").tobytes() + e["bases"] + np.array(e["base_off"], dtype="<u8").tobytes())
    exe = str(tmp_path / "fasta_split_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "fasta_split_check.cpp")])
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "fasta split: ok (%d cases)" % len(S.CASES) in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]


# ---- the restatement against Bank itself ----
def fasta(n, L, W=None, eol=b"\n", first=0):
    return [S.rec(first + i, L, W=W, eol=eol) for i in range(n)]


def whole_files():
    J = b"".join
    files = {
        "single_line": J(fasta(300, 121)),
        "wrapped_at_60": J(fasta(300, 150, W=60)),
        "wrapped_120_at_60": J(fasta(300, 120, W=60)),
        "first_single_rest_wrapped": J(fasta(1, 40) + fasta(299, 150, W=60, first=1)),
        "single_longer_than_the_width": J(fasta(100, 150, W=60) + fasta(1, 61, first=100) + fasta(100, 150, W=60, first=101)),
        "single_then_wrapped_narrower": J(fasta(100, 100) + fasta(100, 150, W=60, first=100)),
        "ragged": J(fasta(150, 150, W=60) + [S.rec(150, lines=[S.bases(1, 60), S.bases(2, 59), S.bases(3, 60)])] + fasta(150, 150, W=60, first=151)),
        "blank_line": J(fasta(150, 150, W=60)) + b"\n" + J(fasta(150, 150, W=60, first=150)),
        "empty_record": J(fasta(150, 150, W=60) + [b">nothing\n"] + fasta(150, 150, W=60, first=151)),
        "crlf": J(fasta(300, 150, W=60, eol=b"\r\n")),
        "no_final_newline": J(fasta(300, 150, W=60))[:-1],
        "blank_lines_first": b"\n\r\n" + J(fasta(300, 150, W=60)),
        "one_record": J(fasta(1, 150, W=60)),
        "contig": J(fasta(50, 100, W=60) + fasta(1, 30000, W=60, first=50) + fasta(50, 100, W=60, first=51)),
    }
    return files


@pytest.mark.parametrize("name", sorted(whole_files()))
def test_the_replayed_reader_rule_against_bank(built, tmp_path, name):
    text = whole_files()[name]
    path = str(tmp_path / (name + ".fa"))
    open(path, "wb").write(text)
    r = subprocess.run([LEON, "-selftest-bank", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bank = json.loads(r.stdout)
    assert not bank["fastq"]
    got = S.replay(text)
    for k in ("reads", "bases", "header_bytes", "fnv_bases", "fnv_headers", "fasta_line_width"):
        assert got[k] == bank[k], (name, k, got[k], bank[k])
    # the device's share: at most four hand-offs of one record each, the first record and the last among them
    assert got["hand_offs"] <= 4 and got["by_host"] <= 4 and got["by_host"] + got["by_device"] == bank["reads"], got
    if name in ("single_line", "wrapped_at_60", "wrapped_120_at_60", "crlf", "no_final_newline", "blank_lines_first", "contig"):
        assert got["by_host"] <= 2, got
    want_width = {"single_line": 0, "wrapped_at_60": 60, "wrapped_120_at_60": 60, "first_single_rest_wrapped": 60, "single_longer_than_the_width": 0,
                  "single_then_wrapped_narrower": 0, "ragged": 0, "blank_line": 0, "empty_record": 0, "crlf": 60, "no_final_newline": 60,
                  "blank_lines_first": 60, "one_record": 60, "contig": 60}
    assert bank["fasta_line_width"] == want_width[name], name
