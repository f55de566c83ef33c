"""The anchor dictionary in independently coded pieces on the device (dict_kernels.hip: k_dict_encode_pieces, k_dict_decode_pieces, lane =
piece): the two context-free calls against their host twins and the oracle on the shapes of tests/dict_pieces.py, a second
wave with one active lane, more pieces than the grid's cap holds in one pass, the directed lists, a two-word poly-A dictionary, corrupted
pieces (the device's verdict is the host's), and the stream a context created with LEON_F_DICT_PIECES hands out."""
import numpy as np
import pytest

import dict_pieces as DP
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import leon_amd
    leon_amd.load_library()
    from leon_amd import capi
    return capi


def _device_encode(capi, kmers, n, k, P, **kw):
    d = capi.device_upload_bytes(np.ascontiguousarray(kmers, dtype=np.uint64).tobytes())
    try:
        return capi.anchor_dict_encode_pieces_device(d, n, k, P, **kw)
    finally:
        capi.device_free(d)


def _both_ways(capi, syms, n, k, P, oracle_pieces=None):
    """device encode == host twin (== the oracle where asked for), device decode of it == the k-mers; returns (stream, piece_off)"""
    kmers = DP.kmers_from_syms(syms, k)
    want, want_off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    got, off = _device_encode(capi, kmers, n, k, P)
    assert np.array_equal(off, want_off), (k, P, n)
    assert got == want, (k, P, n)
    pieces, bounds = DP.split(got, off), DP.piece_bounds(n, P)
    for p in (range(len(bounds)) if oracle_pieces is None else oracle_pieces):
        a, b = bounds[p]
        assert pieces[p] == DP.ref_piece(syms[a * k:b * k]), (k, P, n, p)
    assert np.array_equal(capi.anchor_dict_decode_pieces_device(got, off, n, k, P), kmers), (k, P, n)
    return got, off


@pytest.mark.parametrize("k", DP.KS)
def test_device_pieces_on_the_shapes(capi, k):
    for _, P, n in [s for s in DP.shapes() if s[0] == k]:
        _both_ways(capi, DP.random_syms(1000 * k + 7 * P + n, n, k), n, k, P)


def test_second_wave_with_one_active_lane(capi):
    k, P = 31, 4
    n = 64 * P + 1
    _both_ways(capi, DP.random_syms(64, n, k), n, k, P)


def test_more_pieces_than_the_grid_holds_in_one_pass(capi):
    """P = 1: a piece per anchor.  The grid is capped at 1024 waves of 64 pieces; 2 * 65 536 + 70 pieces go round its loop a second and a
    third time, the third with two waves, the last of them with 6 active lanes"""
    k, P = 3, 1
    per_pass = 1024 * 64
    n = 2 * per_pass + 70
    edges = [0, 63, 64, per_pass - 1, per_pass, per_pass + 64, 2 * per_pass - 1, 2 * per_pass, 2 * per_pass + 63, 2 * per_pass + 64, n - 1]
    _both_ways(capi, DP.random_syms(11, n, k), n, k, P, oracle_pieces=edges)


@pytest.mark.parametrize("name", sorted(DP.DIRECTED))
def test_directed_lists(capi, name):
    k, P, n, syms = DP.DIRECTED[name]()
    assert DP.rare_steps(name)                                     # (certified in test_dict_pieces_cpu.py)
    _both_ways(capi, syms, n, k, P)


def test_two_word_poly_a(capi):
    """k = 63, every base A: the most skewed model there is -- many symbols per byte, then several bytes at once"""
    k, P, n = 63, 64, 3 * 64 + 5
    _both_ways(capi, np.zeros(n * k, dtype=np.uint8), n, k, P)


def test_overflow_and_refusals_as_the_host(capi):
    k, P, n = 31, 64, 200
    kmers = DP.kmers_from_syms(DP.random_syms(9, n, k), k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    with pytest.raises(capi.LeonDnaError) as e:
        _device_encode(capi, kmers, n, k, P, out_cap=len(stream) - 1)
    assert e.value.code == -5 and "out_cap too small" in str(e.value) and e.value.size == len(stream) and np.array_equal(e.value.piece_off, off)
    assert _device_encode(capi, kmers, n, k, P, out_cap=len(stream))[0] == stream
    back = off.copy()
    back[1], back[2] = off[2], off[1]
    for args in ((stream, off, n, 64, P), (stream, off, n, k, (1 << 20) + 1), (stream, off, n + P, k, P), (stream, off[:-1], n, k, P), (stream, back, n, k, P)):
        assert DP.verdict(capi, capi.anchor_dict_decode_pieces_device, *args)[:2] == DP.verdict(capi, capi.host_anchor_dict_decode_pieces, *args)[:2] != (0, "")
    assert capi.anchor_dict_encode_pieces_device(0, 0, k, P)[0] == b""                      # no anchors: no piece, no device asked
    assert len(capi.anchor_dict_decode_pieces_device(b"", np.zeros(1, np.uint64), 0, k, P)) == 0


@pytest.mark.parametrize("k,P,n", [(31, 40, 5 * 40 + 2), (63, 3, 70 * 3 + 1), (3, 64, 64 * 66)])
def test_corrupted_pieces_get_the_hosts_verdict(capi, k, P, n):
    """code, message (the smallest failing piece), out_kmers untouched -- or, where the bytes still decode, the same k-mers"""
    kmers = DP.kmers_from_syms(DP.random_syms(21 + k, n, k), k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    refused = 0
    for name, (s, o) in DP.corruptions(stream, off).items():
        host = DP.verdict(capi, capi.host_anchor_dict_decode_pieces, s, o, n, k, P)
        dev = DP.verdict(capi, capi.anchor_dict_decode_pieces_device, s, o, n, k, P)
        assert dev[:2] == host[:2], name
        assert np.array_equal(dev[2], host[2]), name
        if host[0]:
            refused += 1
            assert np.all(dev[2] == 0x5EED), name
    assert refused >= 2


# ---- through a context: tests/test_gpu_chain_form.py's case ------------------------------------------------------------------------
K, RPB = 31, 50000


@pytest.fixture(scope="module")
def case():
    import common
    bases, off = common.synthetic(120000, 100, 400000, seed=61, err=0.01)
    bl, solid, tai = common.make_bloom(bases, off, K)
    ref = O.encode(bases, off, K, RPB, bl, trace=False)
    assert len(ref.blocks) == 3 and ref.n_anchors > 15000
    return bases, off, solid, tai, ref


def _run(ctx, case, batches):
    bases, off = case[0], case[1]
    blocks = []
    for a, b in batches:
        blocks += ctx.encode_batch(bases, off[a:b + 1])
    stream, n_anchors = ctx.finish()
    piece_off, P = ctx.dict_pieces()
    return [b[1] for b in blocks], stream, n_anchors, piece_off, P


@pytest.mark.parametrize("P", [1024, 7])
def test_through_a_context(capi, case, P):
    import leon_amd
    bases, off, solid, tai, ref = case
    n = len(off) - 1
    ctx = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=RPB, bloom_tai=tai, device_id=0, dict_pieces=True, dict_piece_anchors=0 if P == 1024 else P)
    try:
        ctx.bloom_insert(solid)
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.dict_pieces()
        assert e.value.code == -4
        blocks, stream, n_anchors, piece_off, p_used = _run(ctx, case, [(0, n)])
        assert blocks == ref.blocks and n_anchors == ref.n_anchors and p_used == P             # the flag does not move the blocks
        assert len(piece_off) == capi.dict_piece_count(n_anchors, P) + 1 and int(piece_off[-1]) == len(stream)
        kmers = ctx.anchor_kmers(n_anchors)
        assert np.array_equal(kmers, ref.anchor_kmers)
        want, want_off = capi.host_anchor_dict_encode_pieces(kmers, K, P)
        assert np.array_equal(piece_off, want_off) and stream == want
        assert DP.split(stream, piece_off) == DP.ref_pieces(DP.syms_from_kmers(kmers, K), n_anchors, K, P)      # every piece: the oracle's bytes for its slice
        decoded = capi.anchor_dict_decode_pieces_device(stream, piece_off, n_anchors, K, P)
        assert np.array_equal(decoded, O.decode_anchor_dict(ref.anchor_dict, ref.n_anchors, K))
        # two batches give the same pieces as one; a second file after reset_stream
        ctx.reset_stream()
        with pytest.raises(capi.LeonDnaError):
            ctx.dict_pieces()
        again = _run(ctx, case, [(0, 2 * RPB), (2 * RPB, n)])
        assert again[0] == blocks and again[1] == stream and again[2] == n_anchors and np.array_equal(again[3], piece_off)
        # every other rank of a job returns no stream
        ctx.reset_stream()
        ctx.set_shard(1, 2)
        _, s1, na1, off1, _ = _run(ctx, case, [(0, n)])
        assert s1 == b"" and na1 == n_anchors and off1.tolist() == [0]
    finally:
        ctx.close()


def test_context_without_the_flag(capi, case):
    import leon_amd
    bases, off, solid, tai, ref = case
    ctx = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=RPB, bloom_tai=tai, device_id=0)
    try:
        ctx.bloom_insert(solid)
        blocks = ctx.encode_batch(bases, off)
        stream, n_anchors = ctx.finish()
        assert [b[1] for b in blocks] == ref.blocks and stream == ref.anchor_dict and n_anchors == ref.n_anchors
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.dict_pieces()
        assert e.value.code == -4 and "without LEON_F_DICT_PIECES" in str(e.value)
    finally:
        ctx.close()
    for kw in (dict(dict_pieces=True, dict_on_device=True), dict(dict_piece_anchors=7), dict(dict_pieces=True, dict_piece_anchors=(1 << 20) + 1)):
        with pytest.raises(capi.LeonDnaError) as e:
            leon_amd.DnaEncodeContext(kmer_size=K, bloom_tai=tai, **kw)
        assert e.value.code == -1
