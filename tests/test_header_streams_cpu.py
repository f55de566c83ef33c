"""The header decoder against streams no encoder of ours writes (tests/header_cases.py), on the CPU: the pure-Python reader of
tests/header_streams.py against each case's literal, against the two encoders, and then the host decoder
(leon_host_header_decode_blocks, "route A") and the oracle's decoder against the reader."""
import pytest

import hdr_samples as H
import header_cases as HC
import header_streams as S
import oracle_lib as O
import py_header
from test_gpu_header_text import _edge_sets

MSG = "header block %d does not decode"


def _capi():
    from leon_amd import capi
    return capi


def _all_valid():
    return [(first, b) for first, blocks in HC.valid_groups() for b in blocks]


def test_cap_is_the_devices():
    assert HC.CAP == _capi().HEADER_TEXT_DEVICE_CAP


@pytest.mark.parametrize("group", range(len(HC.valid_groups())))
def test_reader_gives_the_literal(group):
    first, blocks = HC.valid_groups()[group]
    for b in blocks:
        r = S.read_full(b.payload, b.n_reads, first)
        assert not isinstance(r, S.Refused), (b.name, r)
        assert r[0] == b.want, b.name
        assert r[1] == 0, (b.name, "a whole payload is read to its end and no further")
        assert len(b.pairs) == r[2]
        # what the device can build, it must be given room to: only the named block exceeds its share of the symbol buffer
        assert (r[2] > HC.share(b)) == (b.name == "over_share"), (b.name, r[2], HC.share(b))
        assert (max(map(len, b.want)) > HC.CAP) == (b.name.startswith("cap1_") or b.name == "zeros_100000"), b.name
    assert len({b.name for b in blocks}) == len(blocks)


def test_reader_refuses_the_literal():
    for b in HC.refused():
        r = S.read(b.payload, b.n_reads, HC.F)
        assert isinstance(r, S.Refused), (b.name, r)
        if b.refused:
            assert r.kind == b.refused, (b.name, r)
        if b.name == "ascii_size_2_40":
            assert len(b.payload) <= 30


def test_reader_inverts_the_encoders():
    sets, over = _edge_sets()
    samples = [("sra", H.sra(40)), ("toy_like", H.toy_like(30)), ("nasty", H.nasty(40))] + list(sets.items()) + [(k, v[0]) for k, v in over.items()]
    samples.append(("colons", [b.want[0] for b in HC.valid_groups()[1][1]]))
    for name, hs in samples:
        for first in (hs[0], b"", b"q 12:0007\x00z"):
            for enc in (py_header.encode_block, O.header_encode_block):
                r = S.read(enc(hs, first), len(hs), first)
                assert not isinstance(r, S.Refused), (name, r)
                assert r == (hs, 0), (name, first)


def _route_a(blocks, first, n_threads=1):
    return _capi().host_header_decode_blocks([b.as_block(i) for i, b in enumerate(blocks)], first, n_threads=n_threads)


@pytest.mark.parametrize("group", range(len(HC.valid_groups())))
def test_host_decoder_valid(group):
    first, blocks = HC.valid_groups()[group]
    want = [h for b in blocks for h in S.read(b.payload, b.n_reads, first)[0]]
    for nt in (1, 4):
        assert _route_a(blocks, first, nt) == want


def test_oracle_decoder_valid():
    for first, b in _all_valid():
        assert O.header_decode_block(b.payload, b.n_reads, first, sum(map(len, b.want)) + 64) == b.want, b.name


@pytest.mark.parametrize("place", range(3))
def test_host_decoder_refuses(place):
    capi = _capi()
    good = [h for g in HC.GOOD for h in g.want]
    for b in HC.refused():
        blocks = list(HC.GOOD)
        blocks.insert(place, b)
        for nt in (1, 4):
            with pytest.raises(capi.LeonDnaError) as e:
                _route_a(blocks, HC.F, nt)
            assert e.value.code == -1 and MSG % place in str(e.value), (b.name, str(e.value))
        assert _route_a(HC.GOOD, HC.F) == good


def test_host_decoder_two_bad_blocks():
    capi = _capi()
    R = {b.name: b for b in HC.refused()}
    blocks = [HC.GOOD[0], R["type_0"], HC.GOOD[1], R["delta_on_007"]]
    for nt in (1, 4):
        with pytest.raises(capi.LeonDnaError) as e:
            _route_a(blocks, HC.F, nt)
        assert e.value.code == -1 and (MSG % 1 in str(e.value) or MSG % 3 in str(e.value))
    over = [b for b in HC.valid_groups()[4][1] if b.name == "over_share"][0]
    for blocks, bad in (([over, R["index_below_placed"]], 1), ([R["index_below_placed"], over], 0)):
        with pytest.raises(capi.LeonDnaError) as e:
            _route_a(blocks, HC.F, 4)
        assert e.value.code == -1 and MSG % bad in str(e.value)


def test_end_of_payload():
    """15 and 16 bytes beyond the end are read, the step that takes the 17th refuses the stream: the search finds all three
    (a condition on the inputs), and the host decoder answers as the reader does"""
    capi = _capi()
    found = HC.end_of_payload()
    assert set(found) == {15, 16, 17, "last"}, sorted(map(str, found))
    for k in (15, 16):
        first, payload, n_reads, (want, beyond) = found[k]
        assert beyond == k and len(want) == n_reads
        assert capi.host_header_decode_blocks([(0, payload, n_reads)], first, n_threads=1) == want, k
        assert O.header_decode_block(payload, n_reads, first, sum(map(len, want)) + 64) == want
    for k in (17, "last"):                                        # ("last": every symbol is there, the last one's step takes the 17th byte)
        first, payload, n_reads, r = found[k]
        assert isinstance(r, S.Refused) and r.kind == "end"
        with pytest.raises(capi.LeonDnaError) as e:
            capi.host_header_decode_blocks([(0, payload, n_reads)], first, n_threads=1)
        assert e.value.code == -1 and MSG % 0 in str(e.value), k
