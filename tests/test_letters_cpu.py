"""CPU tests of `-c -letters`: the four entry points are declared, exported and bound; leon_host_letters_apply against
the numpy model of letters_shapes.py on the shapes the device form is tested with (test_gpu_letters.py); what both forms of apply
refuse, in the same words, before a device is touched; the option's place on the command line.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import letters_shapes as S
from letters_shapes import REFUSALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")
SYMBOLS = ("leon_letters_count_device", "leon_letters_take_device", "leon_letters_apply_device", "leon_host_letters_apply")


@pytest.fixture(scope="module", autouse=True)
def capi():
    import leon_amd
    if not os.path.exists(leon_amd.lib_path()) or not os.path.exists(LEON):
        leon_amd.build_library()
    leon_amd.load_library()
    from leon_amd import capi
    return capi


@pytest.fixture(scope="module")
def shapes():
    cases = [(name, data, S.Model(data)) for name, data in S.small_shapes()]
    data, _ = S.past_the_grid_cap(0)
    return cases + [("past the grid cap", data, S.Model(data))]


def test_symbols_and_abi(capi):
    header = open(os.path.join(ROOT, "include", "leon_dna.h")).read()
    lib = capi.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/leon_dna.h"
        assert name in capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert "#define LEON_DNA_ABI_VERSION 5\n" in header
    assert lib.leon_dna_abi_version() == 5 and capi.ABI_VERSION == 5


def test_the_model_on_a_line_read_by_eye():
    m = S.Model(np.frombuffer(b"ACgtnNRr.acGT-y", dtype=np.uint8))
    assert m.runs.tolist() == [[2, 5], [7, 8], [9, 11], [14, 15]]
    assert m.odd_pos.tolist() == [6, 7, 8, 13, 14] and m.odd_byte.tobytes() == b"Rr.-y"
    assert m.folded.tobytes() == b"ACGTNNNNNACGTNN"
    assert S.restore(m.folded, m.runs, m.odd_pos, m.odd_byte).tobytes() == b"ACgtnNRr.acGT-y"


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_host_apply_restores_the_original(capi, shapes, threads):
    for name, data, m in shapes:
        got = m.folded.copy()
        capi.host_letters_apply(got, m.runs, m.odd_pos, m.odd_byte, n_threads=threads)
        assert np.array_equal(got, data), name
        assert np.array_equal(S.restore(m.folded, m.runs, m.odd_pos, m.odd_byte), data), name + ": the model does not invert itself"


def test_host_apply_order_and_clipping(capi):
    """the case first, then the bytes; only 'A'..'Z' inside a run get the bit; nothing outside the tables' positions changes"""
    got = np.frombuffer(b"ACGT[N@N]ACGT", dtype=np.uint8).copy()
    capi.host_letters_apply(got, [[1, 7], [9, 13]], [2, 12], np.frombuffer(b"R-", dtype=np.uint8))
    assert got.tobytes() == b"AcRt[n@N]acg-"


def test_host_apply_past_4_gib(capi):
    data, runs, pos, byte, places = S.huge()
    for p, _, folded in places:
        data[p] = folded
    capi.host_letters_apply(data, runs, pos, byte)
    for p, original, _ in places:
        assert data[p] == original, p
        data[p] = ord("A")
    for a in range(0, len(data), 1 << 28):
        assert np.all(data[a:a + (1 << 28)] == ord("A")), "a byte outside the tables changed near %d" % a


def test_nothing_to_do(capi):
    capi.host_letters_apply(None, None, None, None)
    capi.letters_apply_device(0, 0, None, None, None)
    got = np.frombuffer(b"acgtRY", dtype=np.uint8).copy()
    capi.host_letters_apply(got, None, None, None)
    assert got.tobytes() == b"acgtRY"
    # empty tables: no device is asked, whatever the pointer
    capi.letters_apply_device(0x1000, 64, None, None, None)
    assert capi.letters_count_device(0, 0) == (0, 0)


@pytest.mark.parametrize("what,kw,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(capi, what, kw, words):
    """both forms, the same code and words; the device form refuses before it touches a device (this machine has none)"""
    buf = np.full(64, ord("A"), dtype=np.uint8)
    with pytest.raises(capi.LeonDnaError) as h:
        capi.host_letters_apply(buf, **kw)
    assert h.value.code == -1 and str(h.value).endswith(": " + words)
    assert buf.tobytes() == b"A" * 64
    with pytest.raises(capi.LeonDnaError) as d:
        capi.letters_apply_device(0x1000, 64, **kw)
    assert d.value.code == -1 and str(d.value) == str(h.value)


def test_refuses_tables_without_bases(capi):
    for call in (lambda: capi.host_letters_apply(None, [[0, 4]], None, None, n_bytes=64), lambda: capi.letters_apply_device(0, 64, [[0, 4]], None, None)):
        with pytest.raises(capi.LeonDnaError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith(": letters: null argument")


def test_count_and_take_refuse_null_arguments(capi):
    lib = capi.load_library()
    assert lib.leon_letters_count_device(0, 0x1000, 64, None, None) == -1
    assert lib.leon_last_error(None).decode() == "letters: null argument"
    with pytest.raises(capi.LeonDnaError) as e:
        capi.letters_count_device(0, 64)
    assert e.value.code == -1 and str(e.value).endswith(": letters: null argument")
    assert lib.leon_letters_take_device(0, 0x1000, 64, None, 3, None, None, 0) == -1
    assert lib.leon_last_error(None).decode() == "letters: null argument"
    # an empty buffer holds nothing: tables sized for more are a call out of order
    with pytest.raises(capi.LeonDnaError) as e:
        capi.letters_take_device(0, 0, 1, 0)
    assert e.value.code == -4 and "holds 0 run(s) and 0 other byte(s)" in str(e.value)
    assert [len(a) for a in capi.letters_take_device(0, 0, 0, 0)] == [0, 0, 0]


def test_the_option_belongs_to_compression(tmp_path):
    path = str(tmp_path / "x.fastq.leon")
    open(path, "wb").write(b"not a container")
    r = subprocess.run([LEON, "-d", "-letters", "-file", path], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: option -letters belongs to -c"), r.stderr
    r = subprocess.run([LEON, "-d", "-file", path, "-letters"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: option -letters belongs to -c"), r.stderr
