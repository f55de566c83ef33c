"""No GPU: leon_text_bgzf_records_device and its host twin leon_host_bgzf_record_cuts are declared in include/leon_dna.h,
bound by the Python binding and exported by the library, the ABI version stays 5; the call's arguments are refused with their words
before a device is touched; `-gz-records` and `-gz-index` belong to -gz; and the host twin cuts what tests/bgzf_records.py's restatement
of the rule cuts: on the shapes the GPU tests use, on 200 seeded random draws, and however a text is split into calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bgzf_records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "leon_text_bgzf_records_device"
TWIN = "leon_host_bgzf_record_cuts"
W = R.W


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    raw = C.CDLL(capi.lib_path())
    assert ("int %s(int device_id, const uint8_t* d_text, uint64_t n_head, uint64_t n_body, const uint64_t* d_rec_off, uint64_t n_records, int last, "
            "leon_piece_sink sink, void* user, uint64_t* n_taken, uint64_t* out_bytes, uint64_t* member_out_off, uint64_t* member_text_off, "
            "uint64_t members_cap, uint64_t* n_members);" % NAME) in flat
    assert ("int %s(const uint64_t* rec_off, uint64_t n_records, uint64_t n_head, int last, uint64_t* begin, uint32_t* len, uint64_t cap, "
            "uint64_t* n_members, uint64_t* n_taken);" % TWIN) in flat
    for name in (NAME, TWIN):
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert callable(capi.text_bgzf_records_device) and callable(capi.host_bgzf_record_cuts)
    assert capi.bgzf_members_bound(3 * W + 5) == 11 == R.bound(3 * W + 5)


def _call(lib, d_text, n_head, n_body, d_rec_off, n_records, last, sink, taken, out_bytes, m_out, m_text, cap, members):
    rc = lib.leon_text_bgzf_records_device(0, C.c_void_p(d_text), n_head, n_body, C.c_void_p(d_rec_off), n_records, last, sink, None, taken, out_bytes,
                                           C.c_void_p(m_out), C.c_void_p(m_text), cap, members)
    return rc, (lib.leon_last_error(None) or b"").decode()


def test_arguments_are_refused_with_their_words_before_a_device(built):
    from leon_amd import capi
    lib = capi.load_library()
    calls = []
    sink = capi.PIECE_SINK(lambda user, offset, address, size: calls.append((offset, size)) or 0)
    t, o, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
    T, O, M = C.byref(t), C.byref(o), C.byref(m)
    table = np.zeros(8, dtype=np.uint64)
    tab = table.ctypes.data
    fake = 1 << 20                                                # never dereferenced on the host: the device is asked only after the checks
    for args, words in (((0, 0, 5, fake, 1, 1, sink, T, O, 0, 0, 0, M), "d_text is NULL with text given"),
                        ((0, 5, 0, 0, 0, 1, sink, T, O, 0, 0, 0, M), "d_text is NULL with text given"),
                        ((fake, 0, 5, fake, 1, 1, capi.PIECE_SINK(), T, O, 0, 0, 0, M), "sink is NULL"),
                        ((fake, 0, 5, fake, 1, 1, sink, None, O, 0, 0, 0, M), "n_taken is NULL"),
                        ((fake, 0, 5, fake, 1, 1, sink, T, None, 0, 0, 0, M), "out_bytes is NULL"),
                        ((fake, 0, 5, fake, 1, 1, sink, T, O, 0, 0, 0, None), "n_members is NULL"),
                        ((fake, 0, 5, fake, 1, 2, sink, T, O, 0, 0, 0, M), "bgzf records: last is neither 0 nor 1"),
                        ((fake, 0, 5, fake, 1, -1, sink, T, O, 0, 0, 0, M), "bgzf records: last is neither 0 nor 1"),
                        ((fake, W + 1, 5, fake, 1, 1, sink, T, O, 0, 0, 0, M), "bgzf records: n_head is above LEON_BGZF_MEMBER_TEXT"),
                        ((fake, 0, 5, 0, 1, 1, sink, T, O, 0, 0, 0, M), "bgzf records: records given with rec_off NULL"),
                        ((fake, 7, 5, 0, 0, 1, sink, T, O, 0, 0, 0, M), "bgzf records: n_body != 0 without records in record mode"),
                        ((fake, 0, 5, fake, 0, 1, sink, T, O, 0, 0, 0, M), "bgzf records: n_body != 0 without records in record mode"),
                        ((fake, 0, 5, fake, 1, 1, sink, T, O, tab, 0, 8, M), "bgzf records: a half-given member table"),
                        ((fake, 0, 5, fake, 1, 1, sink, T, O, 0, tab, 8, M), "bgzf records: a half-given member table"),
                        ((fake, 0, 5, fake, 1, 1, sink, T, O, 0, 0, 8, M), "bgzf records: a half-given member table")):
        rc, msg = _call(lib, *args)
        assert rc == -1 and msg == NAME + ": " + words, (rc, msg, words)
    assert calls == [] and not table.any()


def test_the_host_twin_refuses_in_the_same_words(built):
    from leon_amd import capi
    for kw, words in ((dict(rec_off=[0, 5], last=2), "bgzf records: last is neither 0 nor 1"),
                      (dict(rec_off=[0, 5], n_head=W + 1), "bgzf records: n_head is above LEON_BGZF_MEMBER_TEXT"),
                      (dict(rec_off=None, n_records=1), "bgzf records: records given with rec_off NULL"),
                      (dict(rec_off=[5], n_records=0), "bgzf records: n_body != 0 without records in record mode"),
                      (dict(rec_off=[1, 5]), "bgzf records: the record offsets do not start at 0"),
                      (dict(rec_off=[0, 5, 5, 9]), "bgzf records: the record offsets are not strictly ascending"),
                      (dict(rec_off=[0, 5, 4, 9]), "bgzf records: the record offsets are not strictly ascending")):
        with pytest.raises(capi.LeonDnaError) as e:
            capi.host_bgzf_record_cuts(**kw)
        assert e.value.code == -1 and words in str(e.value), (kw, str(e.value))
    lib = capi.load_library()
    off = np.array([0, 5], dtype=np.uint64)
    b, n, t = np.zeros(4, dtype=np.uint64), C.c_uint64(), C.c_uint64()
    rc = lib.leon_host_bgzf_record_cuts(C.c_void_p(off.ctypes.data), 1, 0, 1, C.c_void_p(b.ctypes.data), C.c_void_p(0), 4, C.byref(n), C.byref(t))
    assert rc == -1 and "a half-given member table" in lib.leon_last_error(None).decode()
    # a table one entry too small: the need is reported, the entries it has room for are not overrun
    with pytest.raises(capi.LeonDnaError) as e:
        capi.host_bgzf_record_cuts(R.offsets([5, 100000, 5]), cap=5)
    assert e.value.code == -5 and e.value.n_members == 6, (e.value, e.value.n_members)
    assert capi.host_bgzf_record_cuts(R.offsets([5, 100000, 5]), tables=False) == (6, 100010)


def test_cli_options_belong_to_gz(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.fastq")
    for opt in ("-gz-records", "-gz-index"):
        for args in (["-d", opt], [opt, "-d"], ["-c", opt], [opt, "-c"]):
            r = subprocess.run([leon, "-file", nothing] + args, capture_output=True, text=True)
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert r.stderr.splitlines() == ["EXCEPTION: option %s belongs to -gz" % opt], r.stderr
    r = subprocess.run([leon, "-file", nothing, "-c", "-gz", "-gz-records"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: option -gz belongs to -d"], r.stderr
    # beside -d -gz they are accepted: the run gets as far as the file, which is not there, and leaves nothing behind
    r = subprocess.run([leon, "-file", nothing + ".leon", "-d", "-gz", "-gz-records", "-gz-index"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-gz" not in r.stderr and "nothing.fastq.leon" in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_host_twin_under_asan_ubsan(tmp_path):
    """a stand-alone program (its own main) with host_streams.cpp, both compiled with the sanitizers; run as a child process"""
    exe = str(tmp_path / "bgzf_cuts_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "bgzf_cuts_check.cpp"),
                           os.path.join(ROOT, "leon_amd", "csrc", "host_streams.cpp"), "-lz", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bgzf cuts: ok" in r.stdout and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]


def twin(rec_off, n_head=0, last=1):
    from leon_amd import capi
    begin, length, taken = capi.host_bgzf_record_cuts(rec_off, n_head=n_head, last=last)
    return [(int(a), int(m)) for a, m in zip(begin, length)], taken


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_the_host_twin_on_the_shapes(built, name):
    off = R.offsets(R.SHAPES[name])
    for n_head, last in ((0, 1), (0, 0), (1, 1), (W, 0), (W, 1), (12345, 0)):
        want, taken = R.cuts_call(off, n_head, last)
        assert twin(off, n_head, last) == (want, taken), (name, n_head, last)
        n_text = n_head + off[-1]
        assert len(want) <= R.bound(n_text), (name, len(want), n_text)
        assert all(1 <= m <= W for _, m in want)
        assert taken == n_text if last else n_text - taken <= W


def test_the_host_twin_on_random_draws(built):
    rng = np.random.default_rng(20240)
    for draw in range(200):
        lengths = rng.integers(1, 40001, int(rng.integers(1, 60)))
        if draw % 3 == 0:                                         # mostly small records, a few long ones
            lengths = np.where(rng.random(len(lengths)) < 0.8, lengths % 700 + 1, lengths)
        off = R.offsets(lengths)
        n_head = int(rng.choice([0, 0, 1, W, int(rng.integers(1, W + 1))]))
        last = int(rng.integers(0, 2))
        want, taken = R.cuts_call(off, n_head, last)
        assert twin(off, n_head, last) == (want, taken), (draw, list(lengths), n_head, last)
        assert len(want) <= R.bound(n_head + off[-1])


def by_calls(off, bounds):
    """the text's records through one call per part (records [bounds[i], bounds[i + 1])), each call's remainder carried as the next head"""
    members, done, head = [], 0, 0                                # done: text bytes taken by the calls so far; head: bytes carried
    bounds = [0] + list(bounds) + [len(off) - 1]
    for i in range(len(bounds) - 1):
        a, b = bounds[i], bounds[i + 1]
        assert head <= W and done + head == off[a]
        got, taken = twin([x - off[a] for x in off[a:b + 1]], n_head=head, last=1 if i == len(bounds) - 2 else 0)
        members += [(done + p, m) for p, m in got]
        done, head = done + taken, head + off[b] - off[a] - taken
    assert head == 0 and done == off[-1]
    return members


def test_split_into_calls_at_every_record_boundary(built):
    lengths = [256] * 128 + [100, 40000, 300, 16384, 16384, 5, 70000, 1, 32768, 32767, 2]
    off = R.offsets(lengths)
    whole = R.cuts(off)
    assert twin(off) == (whole, off[-1])
    heads = set()
    for b in range(0, len(lengths) + 1):
        assert by_calls(off, [b]) == whole, b
        got, taken = twin(off[:b + 1], last=0)
        heads.add(off[b] - taken)
    assert W in heads and 0 in heads                              # a head of exactly W (after record 128) and none (behind the 40 000)
    assert twin(off[:131], last=0)[1] == off[130]                 # the oversized record ends a non-last call and is taken whole
    short = [9, 40000, 20000, 12768, 1, 32768, 65537, 3, 3]
    off = R.offsets(short)
    whole = R.cuts(off)
    for b1 in range(len(short) + 1):
        for b2 in range(b1, len(short) + 1):
            assert by_calls(off, [b1, b2]) == whole, (b1, b2)
