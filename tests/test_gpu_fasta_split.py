"""-m gpu: leon_fasta_split_device (k_fq_newlines, k_fa_lines, k_fa_heads, k_fa_offsets, k_fa_split) against the Python restatement of
tests/fasta_shapes.py -- never against the code under test -- on every designed text: the result's fields, both blobs and both offset
tables.  Text, blobs and tables lie in one device buffer filled with a pattern, the blobs at odd addresses; every byte of it that the
contract does not give to the call comes back as the pattern."""
import ctypes as C

import numpy as np
import pytest

import fasta_shapes as S

pytestmark = pytest.mark.gpu

FILL = 0xA5
GAP = 64


@pytest.fixture(scope="module")
def expected():
    return {name: S.split(*case) for name, case in S.CASES.items()}


def device_split(text, last, max_records, wrap, shift=0, bytes_cap=None, records_cap=None):
    """the call on one arena: [gap | text at 16 k + shift | gap | headers | gap | bases | gap | header_off | gap | base_off | gap].
    Returns (result dict or LeonDnaError, headers, header_off, bases, base_off) as the capacities' worth of bytes / entries"""
    from leon_amd import capi
    lib = capi.load_library()
    n = len(text)
    bytes_cap = n if bytes_cap is None else bytes_cap
    records_cap = n // 2 + 2 if records_cap is None else records_cap
    at, places = GAP + shift, {}
    places["text"] = (at, n)
    at += n + GAP
    for k, name in enumerate(("headers", "bases")):
        at += (-at) % 16 + 2 * k + 1                              # odd addresses, a different one mod 16 each
        places[name] = (at, bytes_cap)
        at += bytes_cap + GAP
    for name in ("header_off", "base_off"):
        at += (-at) % 8
        places[name] = (at, 8 * records_cap)
        at += 8 * records_cap + GAP
    arena = np.full(at, FILL, dtype=np.uint8)
    if n:
        arena[places["text"][0]:places["text"][0] + n] = np.frombuffer(text, dtype=np.uint8)
    base = capi.device_alloc(at + 256)
    try:
        assert base % 256 == 0
        assert lib.leon_device_upload(0, C.c_void_p(base), C.c_void_p(arena.ctypes.data), at) == 0
        p = {k: base + v[0] for k, v in places.items()}
        try:
            res = capi.fasta_split_device(p["text"], n, last, max_records, wrap, p["headers"], p["header_off"], p["bases"], p["base_off"], bytes_cap, records_cap)
        except capi.LeonDnaError as e:
            res = e
        back = np.frombuffer(capi.device_download(base, at), dtype=np.uint8)
    finally:
        capi.device_free(base)
    # nothing outside the four outputs has changed
    mask = np.ones(at, dtype=bool)
    for name in ("headers", "bases", "header_off", "base_off"):
        mask[places[name][0]:places[name][0] + places[name][1]] = False
    assert np.array_equal(back[mask], arena[mask]), "bytes outside the outputs were written"
    part = {k: back[v[0]:v[0] + v[1]] for k, v in places.items()}
    return res, part["headers"], part["header_off"].view("<u8"), part["bases"], part["base_off"].view("<u8")


def check(case, e, **kw):
    res, headers, header_off, bases, base_off = device_split(*case, **kw)
    assert isinstance(res, dict), res
    assert res == {k: e[k] for k in S.RESULT_FIELDS}
    n, hb, bb = e["n_records"], e["header_bytes"], e["base_bytes"]
    assert headers[:hb].tobytes() == e["headers"] and bases[:bb].tobytes() == e["bases"]
    assert header_off[:n + 1].tolist() == e["header_off"] and base_off[:n + 1].tolist() == e["base_off"]
    # behind the blobs' and the tables' ends: the pattern
    assert (headers[hb:] == FILL).all() and (bases[bb:] == FILL).all()
    assert (header_off[n + 1:].view(np.uint8) == FILL).all() and (base_off[n + 1:].view(np.uint8) == FILL).all()


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_every_case(expected, name):
    check(S.CASES[name], expected[name])


@pytest.mark.parametrize("name", ["record_line_counts", "record_line_counts_no_last", "line_longer_than_a_tile", "contig_of_5000_lines", "crlf_on_some_lines",
                                  "one_open_last_w60", "cut_at_the_gt", "header_rule_text_first", "lines_257", "records_257", "mix_1", "mix_2"])
def test_every_text_alignment(expected, name):
    """the text's first byte at other addresses mod 16: the newline tiles are cut at aligned addresses, and the line copies start anywhere"""
    for shift in (1, 5, 8, 15):
        check(S.CASES[name], expected[name], shift=shift)


def test_capacities_exact_and_too_small(expected):
    from leon_amd import capi
    for name in ("records_65_w7", "crlf_everywhere", "inner_line_short_at_64_w60", "contig_of_5000_lines"):
        e = expected[name]
        want = {k: e[k] for k in S.RESULT_FIELDS}
        exact = dict(records_cap=e["n_records"] + 1, bytes_cap=max(e["header_bytes"], e["base_bytes"]))
        check(S.CASES[name], e, **exact)
        for kw in (dict(exact, records_cap=e["n_records"]), dict(exact, bytes_cap=exact["bytes_cap"] - 1), dict(records_cap=0, bytes_cap=0)):
            res, headers, header_off, bases, base_off = device_split(*S.CASES[name], **kw)
            assert isinstance(res, capi.LeonDnaError) and res.code == -5 and res.result == want, (name, kw, res)
            assert "leon_fasta_split_device: %d records need" % e["n_records"] in str(res)
            # a call that does not fit writes nothing at all
            assert (headers == FILL).all() and (bases == FILL).all() and (header_off.view(np.uint8) == FILL).all() and (base_off.view(np.uint8) == FILL).all()
