"""-m gpu: k_decode_blocks outside the conforming set (tests/dna_bad_streams.py, certified without a GPU by
tests/test_dna_bad_streams_cpu.py).  Every refusal is reached on purpose and held to its words and to the block it names; the caller's
device buffers stay as they were; the good call made next on the same context is still right; lists no decoder refuses decode to what
list membership gives (the oracle's output); a conforming call decodes whatever its share of N.  All through
leon_dna_decode_blocks_device, with the host form held to the same status and message."""
import functools

import pytest

import dna_bad_streams as B
import dna_streams as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

CACHE_SETTINGS = ("0", None, "1")                    # LEON_DC_CACHE_MB (read per call): no path cache, its default size, 1 MiB
CACHE_IDS = ["cache-off", "cache-default", "cache-1MiB"]
SLACK = 64
PREFIX = "leon_dna error -1: "                       # LEON_E_INVALID


def _set_cache(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("LEON_DC_CACHE_MB", raising=False)
    else:
        monkeypatch.setenv("LEON_DC_CACHE_MB", mb)


def _ctx(k):
    import leon_amd
    inp = S.base_input(k)
    ctx = leon_amd.DnaEncodeContext(kmer_size=k, reads_per_block=inp.rpb, bloom_tai=inp.tai, **inp.bloom_kw)
    ctx.bloom_upload(inp.bloom.bits)
    return ctx


@functools.lru_cache(maxsize=None)
def _good_oracle(k):
    inp, blocks, nbases = B.good(k)
    aw = S.words(inp.anchors, k)
    out = []
    for (b, payload, n), nb in zip(blocks, nbases):
        out += O.decode_block(k, inp.bloom, aw, payload, n, nb + 16)
    assert out == B.good_reads(k)
    return out


def _device_call(ctx, c):
    """the case through leon_dna_decode_blocks_device, both caller buffers filled with a pattern and with slack behind them:
    ("refused", message) with the buffers checked to be untouched, or ("decoded", reads)"""
    from leon_amd import capi
    total, n = int(sum(c.nbases)), int(sum(b[2] for b in c.blocks))
    d_bases = capi.device_upload_bytes(bytes([0x5A]) * (total + SLACK))
    d_len = capi.device_upload_bytes(bytes([0xA5]) * (4 * n + SLACK))
    try:
        try:
            lens = ctx.decode_blocks_device(S.words(c.anchors, c.k), c.blocks, c.nbases, d_bases, d_len)
        except capi.LeonDnaError as e:
            assert e.code == -1, c.name
            assert capi.device_download(d_bases, total + SLACK) == bytes([0x5A]) * (total + SLACK), "%s: the caller's bases were written" % c.name
            assert capi.device_download(d_len, 4 * n + SLACK) == bytes([0xA5]) * (4 * n + SLACK), "%s: the caller's lengths were written" % c.name
            return "refused", str(e)
        raw = capi.device_download(d_bases, total + SLACK)
        assert raw[total:] == bytes([0x5A]) * SLACK, "%s: bytes behind the bases were written" % c.name
        assert capi.device_download(d_len, 4 * n + SLACK)[4 * n:] == bytes([0xA5]) * SLACK, "%s: bytes behind the lengths were written" % c.name
        assert int(lens.sum()) == total, c.name
        reads, o = [], 0
        for x in lens:
            reads.append(raw[o:o + int(x)])
            o += int(x)
        return "decoded", reads
    finally:
        capi.device_free(d_bases)
        capi.device_free(d_len)


def _host_call(ctx, c):
    from leon_amd import capi
    try:
        return "decoded", ctx.decode_blocks(S.words(c.anchors, c.k), c.blocks, c.nbases)
    except capi.LeonDnaError as e:
        assert e.code == -1, c.name
        return "refused", str(e)


def _good_call_is_still_right(ctx, k, what):
    inp, blocks, nbases = B.good(k)
    got = ctx.decode_blocks(S.words(inp.anchors, k), blocks, nbases)
    assert got == B.good_reads(k), "the good call after %s: not the reads" % what
    assert got == _good_oracle(k), "the good call after %s: not what the oracle decodes" % what


def _check_refusal(ctx, c):
    allowed = [PREFIX + B.message(c.bad_block, code) for code in ((1, 2, 3, 4) if c.code == B.ANY else (c.code,))]
    dev = _device_call(ctx, c)
    host = _host_call(ctx, c)
    if dev[0] == "decoded":                               # only where the case says a cut of the last bytes may leave every symbol there
        assert c.may_decode, "%s: decoded, and must be refused" % c.name
        assert dev[1] == c.reads and host == dev, "%s: decoded, and not to the reads" % c.name
    else:
        assert dev[1] in allowed, "%s: %r, expected %r" % (c.name, dev[1], allowed)
        assert host == dev, "%s: the host form says %r, the device form %r" % (c.name, host, dev)
    _good_call_is_still_right(ctx, c.k, c.name)


@pytest.mark.parametrize("mb", CACHE_SETTINGS, ids=CACHE_IDS)
@pytest.mark.parametrize("k", [31, 63])
def test_every_refusal_by_its_words(k, mb, monkeypatch):
    """each guard of k_decode_blocks reached on purpose: LEON_E_INVALID, exactly `block 1 does not decode: ` + the code's words (any of the
    four where zero bytes behind a payload's end decide which guard is met), the caller's buffers untouched, and the good call right
    afterwards on the same context -- what a hostile walk published to the path cache is still true of the bloom"""
    _set_cache(monkeypatch, mb)
    ctx = _ctx(k)
    try:
        _good_call_is_still_right(ctx, k, "nothing")
        for c in B.refusal_cases(k):
            _check_refusal(ctx, c)
    finally:
        ctx.close()


@pytest.mark.parametrize("mb", CACHE_SETTINGS, ids=CACHE_IDS)
def test_two_bad_blocks_name_the_smaller(mb, monkeypatch):
    """block 0 fails at its last read, block 3 at its first: block 0 with block 0's reason, five calls out of five"""
    _set_cache(monkeypatch, mb)
    ctx = _ctx(31)
    try:
        c = B.two_bad_blocks()
        for call in range(5):
            _check_refusal(ctx, c)
    finally:
        ctx.close()


@pytest.mark.parametrize("mb", CACHE_SETTINGS, ids=CACHE_IDS)
@pytest.mark.parametrize("k", [31, 63])
def test_lists_no_decoder_refuses(k, mb, monkeypatch):
    """equal neighbours in a position list (before and behind the anchor), entries at and beyond len, an error entry inside the anchor and
    on an N, empty blocks: membership decides -- the reads as written, which is what the oracle decodes (certified without a GPU).  With
    the default cache every call is made twice: the second meets the table the first one filled."""
    _set_cache(monkeypatch, mb)
    ctx = _ctx(k)
    try:
        for c in B.decode_cases(k):
            for call in range(2 if mb is None else 1):
                dev = _device_call(ctx, c)
                assert dev[0] == "decoded", "%s, call %d: %r" % (c.name, call, dev[1])
                wrong = [i for i, (g, w) in enumerate(zip(dev[1], c.reads)) if g != w]
                assert not wrong and len(dev[1]) == len(c.reads), "%s, call %d: reads %r are not what was written" % (c.name, call, wrong[:5])
                assert _host_call(ctx, c) == dev, c.name
    finally:
        ctx.close()


@pytest.mark.parametrize("mb", CACHE_SETTINGS, ids=CACHE_IDS)
@pytest.mark.parametrize("name", ["many", "growing"])
def test_a_conforming_call_decodes_whatever_its_share_of_n(name, mb, monkeypatch):
    """N lists longer than a block's scratch in every read: more entries in all than the pool the call starts with (`many`), and blocks
    whose allocations together exhaust it, so that the call is decoded again with the larger pool (`growing`)"""
    _set_cache(monkeypatch, mb)
    c = B.pool_case(name)
    ctx = _ctx(31)
    try:
        for call in range(2 if mb is None else 1):
            dev = _device_call(ctx, c)
            assert dev[0] == "decoded", "%s, call %d: %r" % (c.name, call, dev[1])
            wrong = [i for i, (g, w) in enumerate(zip(dev[1], c.reads)) if g != w]
            assert not wrong and len(dev[1]) == len(c.reads), "%s, call %d: reads %r are not the input's" % (c.name, call, wrong[:5])
        _good_call_is_still_right(ctx, 31, c.name)
    finally:
        ctx.close()
