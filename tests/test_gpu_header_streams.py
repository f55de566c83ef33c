"""-m gpu: the header decoder's three device routes against the pure-Python reader of tests/header_streams.py, on the directed
streams of tests/header_cases.py -- streams the grammar admits and our encoder never writes, streams the device declines and the
host decodes, and one stream per refusal ("what a decoder accepts").
  B: leon_header_decode_blocks         (k_hdr_decode_symbols, the text on host threads)
  C: leon_header_decode_blocks_device  (k_hdr_decode_symbols + k_hdr_text, declined blocks on the host)
  D: leon_header_decode_text + leon_header_text_fetch
(route A, the host decoder alone, is tests/test_header_streams_cpu.py's)"""
import pytest

import header_cases as HC
import header_streams as S

pytestmark = pytest.mark.gpu

MSG = "header block %d does not decode"


@pytest.fixture(scope="module")
def ctx():
    import leon_amd
    c = leon_amd.DnaEncodeContext(kmer_size=31, reads_per_block=64, bloom_tai=100000)
    yield c
    c.close()


def _capi():
    from leon_amd import capi
    return capi


def _blocks(bs):
    return [b.as_block(i) for i, b in enumerate(bs)]


def _good_batch(ctx):
    """the context decodes a good batch as before, all of it on the device"""
    want = [h for g in HC.GOOD for h in g.want]
    assert ctx.header_decode_blocks(_blocks(HC.GOOD), HC.F) == want
    assert ctx.header_decode_blocks_device(_blocks(HC.GOOD), HC.F) == (want, 0)


def _routes_valid(ctx, first, bs, want_per_block):
    """B, C and D give want_per_block; the blocks marked declined are exactly the ones the device leaves to the host"""
    capi = _capi()
    blocks = _blocks(bs)
    want = [h for w in want_per_block for h in w]
    n_declined = sum(b.declined for b in bs)
    for nt in (1, 4):
        assert ctx.header_decode_blocks(blocks, first, n_threads=nt) == want, "route B"
        got, n_host = ctx.header_decode_blocks_device(blocks, first, n_threads=nt)
        assert got == want, "route C: " + str([b.name for b, w, i in zip(bs, want_per_block, range(len(bs))) if got[sum(x.n_reads for x in bs[:i]):][:b.n_reads] != w])
        assert n_host == n_declined, "route C: %d blocks on the host, %d expected" % (n_host, n_declined)
    T = ctx.header_text_set(blocks, first)
    try:
        for i, b in enumerate(bs):
            if b.declined:
                with pytest.raises(capi.LeonDnaError) as e:
                    T.fetch(i, 1)
                assert e.value.code == -4, (b.name, e.value)
            else:
                assert T.fetch(i, 1) == want_per_block[i], "route D: " + b.name
    finally:
        T.close()


def test_cap_is_the_devices():
    assert HC.CAP == _capi().HEADER_TEXT_DEVICE_CAP


@pytest.mark.parametrize("group", range(len(HC.valid_groups())))
def test_valid_streams(ctx, group):
    first, bs = HC.valid_groups()[group]
    want = []
    for b in bs:
        r = S.read(b.payload, b.n_reads, first)
        assert not isinstance(r, S.Refused) and r[0] == b.want, b.name
        want.append(r[0])
    _routes_valid(ctx, first, bs, want)


def test_many_fields_round_trip(ctx):
    """the headers of the index cases (fields 254, 255, 256 and 300 of 301) through our own encoder and back"""
    hs = [b.want[0] for b in HC.valid_groups()[1][1]]
    ctx.reset_stream()
    blocks = ctx.header_encode_batch(hs, first_header=HC.COLONS)
    for b in blocks:
        assert S.read(b[1], b[2], HC.COLONS) == (hs, 0)
    assert ctx.header_decode_blocks(blocks, HC.COLONS) == hs
    assert ctx.header_decode_blocks_device(blocks, HC.COLONS) == (hs, 0)


def _refused_everywhere(ctx, bs, first, places, host_only=False, set_may_stand=False):
    """B, C and D refuse the call with code -1 and name one of `places`.  host_only: the device merely declines the block (a size
    beyond its cap), so D's set stands, the block's fetch says -4, and the refusal is the host decoder's"""
    capi = _capi()
    blocks = _blocks(bs)
    named = lambda e: e.value.code == -1 and any(MSG % p in str(e.value) for p in places)      # noqa: E731
    for nt in (1, 4):
        for route in (ctx.header_decode_blocks, ctx.header_decode_blocks_device):
            with pytest.raises(capi.LeonDnaError) as e:
                route(blocks, first, n_threads=nt)
            assert named(e), (route.__name__, str(e.value))
    if set_may_stand:                                             # (err[0] went to "does not fit" first: the refused block has no symbols)
        try:
            ctx.header_text_set(blocks, first).close()
            host_only = True
        except capi.LeonDnaError:
            pass
    if not host_only:
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.header_text_set(blocks, first)
        assert named(e), ("header_text_set", str(e.value))
    else:
        T = ctx.header_text_set(blocks, first)
        try:
            for i, b in enumerate(bs):
                if i in places:
                    with pytest.raises(capi.LeonDnaError) as e:
                        T.fetch(i, 1)
                    assert e.value.code == -4
                    with pytest.raises(capi.LeonDnaError) as e:
                        capi.host_header_decode_blocks([blocks[i]], first)
                    assert e.value.code == -1 and MSG % 0 in str(e.value)
                elif not b.declined:
                    assert T.fetch(i, 1) == b.want
        finally:
            T.close()


@pytest.mark.parametrize("place", range(3))
def test_refused_streams(ctx, place):
    for b in HC.refused():
        assert isinstance(S.read(b.payload, b.n_reads, HC.F), S.Refused), b.name
        bs = list(HC.GOOD)
        bs.insert(place, b)
        try:
            _refused_everywhere(ctx, bs, HC.F, [place], host_only=b.host_only)
        except (AssertionError, pytest.fail.Exception) as e:
            raise AssertionError("%s: %s" % (b.name, e))
        _good_batch(ctx)


def test_two_bad_blocks(ctx):
    """two refused blocks: one of them is named (neither side orders its first-wins).  A refused block beside one that merely
    exceeds its share of the symbol buffer, in both orders: the call is refused and the refused block is the one named, whichever
    of the two reports first on the device"""
    R = {b.name: b for b in HC.refused()}
    _refused_everywhere(ctx, [HC.GOOD[0], R["type_0"], HC.GOOD[1], R["delta_on_007"]], HC.F, [1, 3])
    _refused_everywhere(ctx, [R["col_beyond_field"], R["end_beyond_fields"]], HC.F, [0, 1])
    _good_batch(ctx)
    over = [b for b in HC.valid_groups()[4][1] if b.name == "over_share"][0]
    for bad in ("type_0", "index_below_placed", "payload_2_bytes"):
        _refused_everywhere(ctx, [over, R[bad]], HC.F, [1], set_may_stand=True)
        _refused_everywhere(ctx, [R[bad], over], HC.F, [0], set_may_stand=True)
        _refused_everywhere(ctx, [HC.GOOD[0], over, R[bad], over], HC.F, [2], set_may_stand=True)
    _good_batch(ctx)


def test_symbols_left_over_and_missing(ctx):
    """the symbols of a block read as one header fewer or one more than they hold: symbols left over, symbols that run out
    (the two halves of route B; the one-call routes count a block's symbols themselves)"""
    capi = _capi()
    g = HC.GOOD[0]
    T = ctx.header_symbol_set([g.as_block(), HC.GOOD[1].as_block(1)])
    try:
        assert T.text(0, 2, HC.F) == g.want + HC.GOOD[1].want
        for n_reads in (g.n_reads - 1, g.n_reads + 1):
            for nt in (1, 4):
                with pytest.raises(capi.LeonDnaError) as e:
                    T.text(0, 2, HC.F, n_threads=nt, n_reads=[n_reads, HC.GOOD[1].n_reads])
                assert e.value.code == -1 and MSG % 0 in str(e.value), str(e.value)
        assert T.text(1, 1, HC.F) == HC.GOOD[1].want
    finally:
        T.close()
    _good_batch(ctx)


def test_end_of_payload(ctx):
    """15 and 16 bytes beyond the payload's end are read, the 17th refuses the stream, on the device as on the host"""
    found = HC.end_of_payload()
    assert set(found) == {15, 16, 17, "last"}, sorted(map(str, found))
    for k in (15, 16):
        first, payload, n_reads, (want, beyond) = found[k]
        assert beyond == k
        _routes_valid(ctx, first, [HC.Block("beyond_%d" % k, [], want, payload=payload)], [want])
        assert _capi().host_header_decode_blocks([(0, payload, n_reads)], first) == want
    for k in (17, "last"):                                        # ("last": every symbol is there, the last one's step takes the 17th byte)
        first, payload, n_reads, r = found[k]
        assert isinstance(r, S.Refused) and r.kind == "end"
        _refused_everywhere(ctx, [HC.Block("beyond_%s" % k, [], n_reads=n_reads, refused="end", payload=payload)], first, [0])
    _good_batch(ctx)
