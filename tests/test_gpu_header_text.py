"""-m gpu: the header decoder with the TEXT rebuilt on the device (k_hdr_text, one wave per block, through
leon_header_decode_blocks_device and the leon_header_decode_text / leon_header_text_fetch pair) against the host decoder
(leon_host_header_decode_blocks) and the oracle's HeaderDecoder: the same headers, byte for byte, whatever the headers look like."""
import random
import time

import pytest

import hdr_samples as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = [("sra", H.sra, 12000, 5000), ("toy_like", H.toy_like, 3000, 700), ("nasty", H.nasty, 2000, 150),
         ("one_block", H.sra, 900, 50000), ("single", H.toy_like, 1, 10)]


def _ctx(rpb):
    import leon_amd
    return leon_amd.DnaEncodeContext(kmer_size=31, reads_per_block=rpb, bloom_tai=100000)


def _cap():
    from leon_amd import capi
    return capi.HEADER_TEXT_DEVICE_CAP


def _check(ctx, hs, rpb, first=None, on_host=None, oracle=True):
    """encode hs in blocks of rpb; the oracle's decoder, the host decoder and the device decoder all give hs back"""
    from leon_amd import capi
    first = hs[0] if first is None else first
    ctx.reset_stream()
    blocks = ctx.header_encode_batch(hs, first_header=first)
    if oracle:
        for i, b in enumerate(blocks):
            want = hs[i * rpb:(i + 1) * rpb]
            assert O.header_decode_block(b[1], len(want), first, sum(map(len, want)) + 64) == want, "oracle, block %d" % i
    assert capi.host_header_decode_blocks(blocks, first) == hs
    got, n_host = ctx.header_decode_blocks_device(blocks, first)
    assert got == hs, "the device's text differs from the input"
    if on_host is not None:
        assert n_host == on_host, "%d blocks were decoded on the host, expected %d" % (n_host, on_host)
    return blocks, n_host


@pytest.mark.parametrize("name,make,n,rpb", CASES)
def test_device_text_bit_exact(name, make, n, rpb):
    from leon_amd import capi
    hs = make(n)
    if name != "nasty":                                            # (checked on the CPU: these generators stay far below the kernel's cap)
        assert max(map(len, hs)) < _cap()
    ctx = _ctx(rpb)
    blocks = ctx.header_encode_batch(hs)
    want = capi.host_header_decode_blocks(blocks, hs[0])
    assert want == hs
    t0 = time.time()
    for nt in (0, 3):
        got, n_host = ctx.header_decode_blocks_device(blocks, hs[0], n_threads=nt)
        assert got == hs and got == want, (name, nt)
        # the kernel itself must have built the text, not the host decoder behind it ("nasty": hundreds of symbols per header, more
        # than a block's share of the symbol buffer -- any count)
        if name != "nasty":
            assert n_host == 0, (name, n_host)
        else:
            assert 0 <= n_host <= len(blocks)
    print("%s: %d blocks, %d on the host, %.3f s for two calls" % (name, len(blocks), n_host, time.time() - t0))
    assert ctx.header_decode_blocks_device([], b"") == ([], 0)
    ctx.close()


@pytest.mark.parametrize("name,make,n,rpb", [c for c in CASES if c[0] != "nasty"])
def test_text_set_fetch(name, make, n, rpb):
    from leon_amd import capi
    hs = make(n)
    ctx = _ctx(rpb)
    blocks = ctx.header_encode_batch(hs)
    nb = len(blocks)
    S = ctx.header_text_set(blocks, hs[0])
    for b0, k in ((0, nb), (nb - 1, 1), (1, max(nb - 2, 0)), (0, 0)):
        if b0 > nb:
            continue
        assert S.fetch(b0, k) == hs[b0 * rpb:(b0 + k) * rpb], (name, b0, k)
    d_text, d_off, size = S.device_ptr(0, nb)
    assert d_text and d_off and size == sum(map(len, hs))
    with pytest.raises(capi.LeonDnaError) as e:
        S.fetch(nb, 1)                                            # beyond the set
    assert e.value.code == -1
    with pytest.raises(capi.LeonDnaError):
        S.fetch(0, nb + 1)
    S.close()
    # a first header that is not the file's first, and an empty one
    for first in (b"some other first header 12", b""):
        ctx.reset_stream()
        blocks = ctx.header_encode_batch(hs, first_header=first)
        assert capi.host_header_decode_blocks(blocks, first) == hs
        S = ctx.header_text_set(blocks, first)
        assert S.fetch(0, nb) == hs
        S.close()
        assert ctx.header_decode_blocks_device(blocks, first) == (hs, 0)
    ctx.close()


def _edge_sets():
    cap = _cap()
    long_ = lambda L, tail: b"a" * (L - len(tail)) + tail                                  # noqa: E731
    sets = {
        "empty": [b"", b"", b"a", b"", b"", b"7", b""],
        "len63_64_65_129": [long_(L, b":%d" % (100 + i)) for i, L in enumerate((63, 64, 65, 129, 65, 64, 63, 129, 128, 127, 1, 64))],
        "len_fields_at_word_edges": [b"x" * 62 + b":" + b"12", b"x" * 62 + b":" + b"13", b"x" * 63 + b":7:8", b"x" * 63 + b":7:9", b"y" * 64 + b" 1 2 3",
                                     b"y" * 64 + b" 1 2 4", b":" * 130, b":" * 129 + b"5", b":" * 129 + b"6"],
        "digits18_19": [b"r 123456789012345678 x", b"r 123456789012345679 x", b"r 999999999999999999 x", b"r 1000000000000000000 x", b"r 1000000000000000001 x",
                        b"r 1234567890123456789 x", b"r 1234567890123456790 x", b"r 18446744073709551615 x", b"r 18446744073709551616 x", b"r 0 x", b"r 1 x"],
        "zeros": [b"000", b"0007", b"7", b"0007", b"007 0", b"0 00", b"00 0", b"0", b"00000000000000000000000", b"0000000000000000000000012", b"12"],
        "nul_separator": [b"ab\x0012\x0034", b"ab\x0013\x0035", b"ab\x0013\x0036\x00", b"\x00\x00\x00", b"\x001\x00", b"\x002\x00", b"7\x00", b"8\x00", b"8"],
        "field_count": [b"a b c d", b"a b", b"a b c d e f", b"a", b"a b c d e f g h i j", b"", b"a b c", b"a b c ", b"a b c  ", b"a b c", b"a b"],
        "delta_down": [b"id 1000 x", b"id 990 x", b"id 5 x", b"id 0 x", b"id 300 x", b"id 299 x", b"id 299 w 65535", b"id 298 w 255", b"id 297 w 4294967296", b"id 296 w 1"],
    }
    over = {
        "cap_under": ([long_(cap - 1, b" 17"), long_(cap - 1, b" 18"), long_(cap - 1, b" 19")], 0),
        "cap_at": ([long_(cap, b" 17"), long_(cap, b" 18"), long_(cap - 1, b" 99"), long_(cap, b" 100")], 0),
        "cap_grows_to": ([b"b" * (cap - 2), b"b" * (cap - 2) + b":1", b"b" * (cap - 2) + b":2"], 0),
        "cap_over": ([long_(cap - 1, b" 17"), long_(cap + 1, b" 18"), long_(cap + 1, b" 19"), b"short 1"], None),
        "cap_over_by_digit": ([long_(cap, b" 99"), long_(cap + 1, b" 100"), b"short 1"], None),
    }
    return sets, over


def test_edge_headers():
    sets, over = _edge_sets()
    ctx = _ctx(3)
    for name, hs in sets.items():
        for first in (None, b"", b"q 12:0007\x00z"):
            try:
                _check(ctx, hs, 3, first=first, on_host=0)
            except AssertionError as e:
                raise AssertionError("%s (first header %r): %s" % (name, first, e))
    for name, (hs, on_host) in over.items():
        blocks, n_host = _check(ctx, hs, 3, on_host=on_host)
        if on_host is None:                                       # a header over the cap: its block is the host decoder's, and is counted
            assert n_host >= 1, name
    # a first header over the cap: no block can be built on the device
    hs = [b"a 1", b"a 2", b"a 3", b"a 4"]
    blocks, n_host = _check(ctx, hs, 3, first=b"f" * (_cap() + 1))
    assert n_host == len(blocks) == 2
    ctx.close()
    # the same sets in one block each
    ctx = _ctx(1000)
    for name, hs in sets.items():
        _check(ctx, hs, 1000, on_host=0)
    ctx.close()


ALPHABET_SEPS = [b" ", b":", b"_", b".", b"/", b"=", b"\x00", b"-"]


def _fuzz_token(rnd):
    t = rnd.random()
    if t < 0.35:
        return b"%d" % rnd.choice([rnd.randint(0, 9), rnd.randint(0, 300), rnd.randint(0, 10 ** 6), rnd.randint(10 ** 17, 10 ** 18 - 1), rnd.randint(0, 2 ** 64 - 1)])
    if t < 0.5:
        return b"0" * rnd.randint(1, 4) + (b"%d" % rnd.randint(0, 5000) if rnd.random() < 0.7 else b"")
    if t < 0.6:
        return b""
    if t < 0.7:
        return bytes(rnd.choice(b"0123456789") for _ in range(rnd.randint(17, 22)))
    return bytes(rnd.choice(b"abAZ019") for _ in range(rnd.randint(1, 6)))


def _fuzz_headers(rnd, n):
    out = []
    fields = [(_fuzz_token(rnd), rnd.choice(ALPHABET_SEPS)) for _ in range(rnd.randint(0, 9))]
    walk = rnd.random() < 0.7
    for _ in range(n):
        if not walk or rnd.random() < 0.05:
            fields = [(_fuzz_token(rnd), rnd.choice(ALPHABET_SEPS)) for _ in range(rnd.randint(0, 9))]
        else:
            fields = list(fields)
            for j in range(len(fields)):
                u = rnd.random()
                tok, sep = fields[j]
                if u < 0.25 and tok.isdigit():
                    v = int(tok) + rnd.choice([1, 1, 1, -1, 7, 256, -300, 70000, 2 ** 33])
                    fields[j] = ((b"%d" % v) if 0 <= v < 2 ** 64 else tok, sep)
                elif u < 0.3:
                    fields[j] = (_fuzz_token(rnd), sep)
                elif u < 0.33:
                    fields[j] = (tok, rnd.choice(ALPHABET_SEPS))
            if rnd.random() < 0.05 and fields:
                fields.pop(rnd.randrange(len(fields)))
            if rnd.random() < 0.05:
                fields.insert(rnd.randint(0, len(fields)), (_fuzz_token(rnd), rnd.choice(ALPHABET_SEPS)))
        h = b"".join(t + s for t, s in fields)
        if fields and rnd.random() < 0.7:
            h = h[:-1]                                            # most headers end in a token, not in a separator
        out.append(h)
    return out


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz_device_equals_host(chunk):
    from leon_amd import capi
    rnd = random.Random(7100 + chunk)
    t0, on_host = time.time(), 0
    for it in range(50):                                           # 4 x 50 draws
        n = rnd.randint(1, 1500)
        rpb = rnd.choice([1, 2, 7, 64, 65, 333, 1000, 5000])
        if n // rpb > 300:
            rpb = 7
        hs = _fuzz_headers(rnd, n)
        first = rnd.choice([hs[0], b"", b"zz 9:1"])
        ctx = _ctx(rpb)
        blocks = ctx.header_encode_batch(hs, first_header=first)
        want = capi.host_header_decode_blocks(blocks, first)
        got, n_host = ctx.header_decode_blocks_device(blocks, first, n_threads=rnd.choice([0, 1, 4]))
        ctx.close()
        assert want == hs, (chunk, it)
        assert got == want, (chunk, it, n, rpb, [i for i in range(n) if got[i] != want[i]][:3])
        on_host += n_host
    print("fuzz chunk %d: %.2f s, %d blocks went to the host decoder" % (chunk, time.time() - t0, on_host))


@pytest.mark.parametrize("how", ["inverted", "truncated"])
def test_corrupt_payload(how):
    from leon_amd import capi
    rpb = 500
    hs = H.sra(2000)
    ctx = _ctx(rpb)
    blocks = ctx.header_encode_batch(hs)
    bad = list(blocks)
    p = bad[1][1]
    bad[1] = (bad[1][0], bytes(255 - x for x in p) if how == "inverted" else p[:len(p) // 2], bad[1][2])
    for dec in (lambda: ctx.header_decode_blocks_device(bad, hs[0])[0], lambda: capi.host_header_decode_blocks(bad, hs[0])):
        try:
            assert dec()[rpb:2 * rpb] != hs[rpb:2 * rpb]
        except capi.LeonDnaError as e:
            assert "does not decode" in str(e)
    try:
        S = ctx.header_text_set(bad, hs[0])
        try:
            assert S.fetch(1, 1) != hs[rpb:2 * rpb]
        except capi.LeonDnaError as e:                            # declined (its text is not the size the sizing pass said, ...): the host's turn
            assert e.code == -4
        S.close()
    except capi.LeonDnaError as e:
        assert "does not decode" in str(e)
    # the context is as good as before
    assert ctx.header_decode_blocks_device(blocks, hs[0]) == (hs, 0)
    ctx.close()


def test_text_bytes_from_the_block_table():
    from leon_amd import capi
    rpb = 700
    hs = H.sra(4000)
    ctx = _ctx(rpb)
    blocks = ctx.header_encode_batch(hs)
    nb = len(blocks)
    true = [sum(map(len, hs[b * rpb:(b + 1) * rpb])) for b in range(nb)]
    A = ctx.header_text_set(blocks, hs[0], text_bytes=true)
    B = ctx.header_text_set(blocks, hs[0])
    assert A.fetch(0, nb) == B.fetch(0, nb) == hs
    assert A.device_ptr(2, 2)[2] == B.device_ptr(2, 2)[2] == true[2] + true[3]
    A.close()
    B.close()
    for delta in (-1, +1):                                         # an entry that is not the block's size: that block is not handed out, its neighbours are
        wrong = list(true)
        wrong[2] += delta
        S = ctx.header_text_set(blocks, hs[0], text_bytes=wrong)
        for run in ((2, 1), (0, nb), (1, 2)):
            with pytest.raises(capi.LeonDnaError) as e:
                S.fetch(*run)
            assert e.value.code == -4, e.value                     # LEON_E_STATE
        assert S.fetch(0, 2) == hs[:2 * rpb]
        assert S.fetch(3, nb - 3) == hs[3 * rpb:]
        S.close()
    ctx.close()
