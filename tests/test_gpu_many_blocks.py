"""-m gpu: every kernel that gives a block to a wave or a workgroup, launched with more than twice its grid cap of blocks
(tests/many_blocks.py: 4099 blocks against caps of 2048 and 1024), so that the same wave takes a second and a third trip of its
`for (b = blockIdx.x; b < n_blocks; b += gridDim.x)` loop with another kind of block each time: what a block leaves in LDS or
registers (RcModeler::start_block's resets, k_rc_encode's rings and tile counts, k_rc_records4's turn hand-off and parked models,
k_decode_blocks' Dec and position lists, k_hdr_text's buffers, separator masks and staging) must not reach the next.  Everything is
compared byte for byte with the oracle or with the input; tests/test_many_blocks_cpu.py checks the inputs themselves.

Still open (not reached by a test of a few seconds, or not switchable inside one process):
  * k_deflate_chunks / k_deflate_gather: their cap is 2^20 chunks of 32 KB;
  * the inflate path has no block loop (launch_qual_inflate launches one workgroup per block), so its launch groups are not this
    file's subject;
  * the read-strided kernels carry no state between iterations and run at 2^20-read windows in tests/test_gpu_window.py;
  * LEON_DC_DEEP=0: its getenv is cached in a function-local static and cannot be switched inside one test process."""
import functools

import numpy as np
import pytest

import common
import many_blocks as MB
import oracle_lib as O

pytestmark = pytest.mark.gpu

_RC_ENV = ("LEON_RC_GROUP", "LEON_RC_FAST_TOTAL_LOG2", "LEON_RC_STREAMS_ON_HOST", "LEON_RC_HOST_CHUNKS", "LEON_RC_CMP", "LEON_RC_HOST_BLOCKS",
           "LEON_RC_RECORDS_WAVES", "LEON_DC_CACHE_MB")


def _ctx(k, rpb, tai):
    import leon_amd
    return leon_amd.DnaEncodeContext(kmer_size=k, reads_per_block=rpb, bloom_tai=tai)


def _env(monkeypatch, **env):
    """exactly these LEON_* switches, whatever the process inherited"""
    for name in _RC_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _device_memory_used():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 30


# ---- 1. the range coder ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _rc_want():
    syms, begin, sizes = MB.rc_streams()
    return tuple(O.rc_encode_stream(*MB.rc_stream(b), sizes) for b in range(MB.N_BLOCKS))


@pytest.mark.parametrize("env", [
    dict(),                                                                          # the launcher's own pick: G = 8
    dict(LEON_RC_GROUP="1"), dict(LEON_RC_GROUP="2"), dict(LEON_RC_GROUP="4"),
    dict(LEON_RC_FAST_TOTAL_LOG2="8"),                                               # the BIGOK instantiation: exact division from a total of 2^8 on
    dict(LEON_RC_STREAMS_ON_HOST="1", LEON_RC_HOST_CHUNKS="1"),                      # k_rc_records4, five trips, one launch
    dict(LEON_RC_STREAMS_ON_HOST="1", LEON_RC_HOST_CHUNKS="3"),                      # ... its models parked in global memory between three
], ids=lambda e: "-".join("%s=%s" % (k[8:].lower(), v) for k, v in e.items()) or "default")
def test_range_coder_past_the_grid_cap(monkeypatch, env):
    _env(monkeypatch, **env)
    syms, begin, _ = MB.rc_streams()
    want = _rc_want()
    ctx = _ctx(31, 1000, 1000)
    got = ctx.rc_encode_streams(syms, begin)
    used = _device_memory_used()
    ctx.close()
    assert len(got) == MB.N_BLOCKS
    bad = [b for b in range(MB.N_BLOCKS) if got[b] != want[b]]
    assert not bad, "%d streams differ from the oracle; the first: %s" % (
        len(bad), ", ".join("%d (trip %d, slot %d, %s after %s)" % (b, b // MB.CAP, b % MB.CAP, MB.KIND_NAMES[MB.kind(b)],
                                                                   MB.KIND_NAMES[MB.kind(b - MB.CAP)] if b >= MB.CAP else "nothing") for b in bad[:8]))
    print("range coder %r: %.2f GiB of device memory in use" % (env, used))


# ---- 2. the DNA stream ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dna(k):
    reads = MB.dna_reads()
    bases, off = O.reads_to_arrays(reads)
    bl, solid, tai = common.make_bloom(bases, off, k)
    ref = O.encode(bases, off, k, MB.DNA_RPB, bl, trace=False)
    rpb = MB.DNA_RPB
    nbases = [sum(len(r) for r in reads[rpb * b:rpb * (b + 1)]) for b in range(MB.N_BLOCKS)]
    return bases, off, bl, tai, ref, nbases, MB.dna_normalised(reads)


def _encode_and_compare(ctx, bases, off, ref, what):
    ctx.reset_stream()
    blocks = ctx.encode_batch(bases, off)
    d, na = ctx.finish()
    assert [b[0] for b in blocks] == list(range(MB.N_BLOCKS)), what
    assert [b[2] for b in blocks] == ref.block_nreads, what
    bad = [i for i in range(MB.N_BLOCKS) if blocks[i][1] != ref.blocks[i]]
    assert not bad, "%s: %d block payloads differ from the oracle, the first %r (trip, slot: %r)" % (
        what, len(bad), bad[:8], [(b // MB.CAP, b % MB.CAP) for b in bad[:8]])
    assert na == ref.n_anchors and d == ref.anchor_dict, what
    return blocks, d, na


def _first_wrong(got, want):
    return [(i, i // MB.DNA_RPB) for i in range(min(len(got), len(want))) if got[i] != want[i]][:5]


@pytest.mark.parametrize("k", [31, 47])
def test_dna_encode_and_decode_past_the_grid_cap(monkeypatch, k):
    from leon_amd import capi
    bases, off, bl, tai, ref, nbases, want = _dna(k)
    assert len(ref.blocks) == MB.N_BLOCKS
    _env(monkeypatch)
    ctx = _ctx(k, MB.DNA_RPB, tai)
    ctx.bloom_upload(bl.bits)
    blocks, d, na = _encode_and_compare(ctx, bases, off, ref, "default")
    # the CMP-true instantiations of k_rc_encode are reached from encode_batch only: the round-4 layout, and the other group sizes
    variants = [dict(LEON_RC_CMP="0")] + ([dict(LEON_RC_GROUP="1"), dict(LEON_RC_GROUP="4")] if k == 31 else [])
    for env in variants:
        _env(monkeypatch, **env)
        _encode_and_compare(ctx, bases, off, ref, repr(env))
    # and back: all 4099 blocks in one call, with the path cache and without it
    anchors = capi.anchor_dict_decode(d, na, k)
    full = None
    for mb in (None, "0"):
        _env(monkeypatch, **({} if mb is None else dict(LEON_DC_CACHE_MB=mb)))
        got = ctx.decode_blocks(anchors, blocks, nbases)
        assert len(got) == len(want)
        assert got == want, "cache %r: reads (read, block) %r do not round-trip" % (mb, _first_wrong(got, want))
        full = got
    _env(monkeypatch)
    # the blocks either side of the first trip's end on their own: the same reads as in the full call
    lo, hi = MB.CAP - 8, MB.CAP + 12
    part = ctx.decode_blocks(anchors, blocks[lo:hi], nbases[lo:hi])
    assert part == full[MB.DNA_RPB * lo:MB.DNA_RPB * hi]
    print("DNA k=%d: %.2f GiB of device memory in use" % (k, _device_memory_used()))
    ctx.close()


# ---- 3. the header stream -------------------------------------------------------------------------------------------------------
def _oracle_blocks(hs, rpb, first):
    return [O.header_encode_block(list(hs[b:b + rpb]), first) for b in range(0, len(hs), rpb)]


def _wrong_headers(got, want):
    return [(i, i // MB.HDR_RPB, (i // MB.HDR_RPB) // MB.CAP) for i in range(min(len(got), len(want))) if got[i] != want[i]][:5]


def test_header_streams_past_the_grid_cap(monkeypatch):
    from leon_amd import capi
    _env(monkeypatch)
    rpb, nb = MB.HDR_RPB, MB.N_BLOCKS
    hs, first = MB.headers()
    hs = list(hs)
    ctx = _ctx(31, rpb, 100000)
    blocks = ctx.header_encode_batch(hs, first_header=first)
    ref = _oracle_blocks(hs, rpb, first)
    assert [b[0] for b in blocks] == list(range(nb)) and [b[2] for b in blocks] == [rpb] * nb
    bad = [i for i in range(nb) if blocks[i][1] != ref[i]]
    assert not bad, "%d header blocks differ from the oracle, the first %r" % (len(bad), bad[:8])
    assert capi.host_header_decode_blocks(blocks, first) == hs
    got, n_host = ctx.header_decode_blocks_device(blocks, first)
    assert got == hs, "headers (header, block, trip) %r differ" % _wrong_headers(got, hs)
    assert n_host == 0, "%d blocks went to the host decoder: the kernel was to build every one" % n_host
    S = ctx.header_text_set(blocks, first)
    for b0, n in ((0, nb), (MB.CAP - 8, 20), (2 * MB.CAP, 3)):
        assert S.fetch(b0, n) == hs[rpb * b0:rpb * (b0 + n)], (b0, n)
    d_text, d_off, size = S.device_ptr(0, nb)
    assert d_text and d_off and size == sum(map(len, hs))
    S.close()
    # blocks the kernel declines (a header over its cap) or may decline, each between ordinary blocks of the same wave
    hs2, first2, replaced = MB.headers_with_fallbacks()
    hs2 = list(hs2)
    ctx.reset_stream()
    blocks2 = ctx.header_encode_batch(hs2, first_header=first2)
    assert [b[1] for b in blocks2] == _oracle_blocks(hs2, rpb, first2)
    got, n_host = ctx.header_decode_blocks_device(blocks2, first2)
    assert got == hs2, "headers (header, block, trip) %r differ" % _wrong_headers(got, hs2)
    assert 0 < n_host <= len(replaced), n_host
    # and the context is as good as before
    assert ctx.header_decode_blocks_device(blocks, first) == (hs, 0)
    print("headers: %.2f GiB of device memory in use" % _device_memory_used())
    ctx.close()


# ---- 4. a block that fails on one trip ----------------------------------------------------------------------------------------------
BAD_BLOCK = 5                                                                        # its wave's next block is 5 + 2048


def _inverted(blocks, b):
    bad = list(blocks)
    bad[b] = (bad[b][0], bytes(255 - x for x in bad[b][1]), bad[b][2])
    return bad


def test_a_bad_block_on_one_trip_leaves_the_next_alone(monkeypatch):
    from leon_amd import capi
    _env(monkeypatch)
    # the header decoder
    rpb = MB.HDR_RPB
    hs, first = MB.headers()
    hs = list(hs)
    ctx = _ctx(31, rpb, 100000)
    blocks = ctx.header_encode_batch(hs, first_header=first)
    try:
        got, n_host = ctx.header_decode_blocks_device(_inverted(blocks, BAD_BLOCK), first)
        lo, hi = rpb * BAD_BLOCK, rpb * (BAD_BLOCK + 1)
        assert len(got) == len(hs)
        assert got[:lo] == hs[:lo] and got[hi:] == hs[hi:], "headers (header, block, trip) %r differ, outside the bad block" % _wrong_headers(got, hs)
        assert got[lo:hi] != hs[lo:hi]
    except capi.LeonDnaError as e:
        assert "does not decode" in str(e)
    assert ctx.header_decode_blocks_device(blocks, first) == (hs, 0)
    ctx.close()
    # the DNA decoder
    k, rpb = 31, MB.DNA_RPB
    bases, off, bl, tai, ref, nbases, want = _dna(k)
    ctx = _ctx(k, rpb, tai)
    ctx.bloom_upload(bl.bits)
    blocks = [(b, ref.blocks[b], ref.block_nreads[b]) for b in range(MB.N_BLOCKS)]     # (the oracle's payloads: the encoder's are held equal to them above)
    anchors = capi.anchor_dict_decode(ref.anchor_dict, ref.n_anchors, k)
    try:
        got = ctx.decode_blocks(anchors, _inverted(blocks, BAD_BLOCK), nbases)
        lo, hi = rpb * BAD_BLOCK, rpb * (BAD_BLOCK + 1)
        assert len(got) == len(want)
        assert got[:lo] == want[:lo] and got[hi:] == want[hi:], "reads (read, block) %r differ, outside the bad block" % _first_wrong(got, want)
        assert got[lo:hi] != want[lo:hi]
    except capi.LeonDnaError as e:
        assert "does not decode" in str(e)
    got = ctx.decode_blocks(anchors, blocks, nbases)
    assert got == want, "after the bad call: reads (read, block) %r do not round-trip" % _first_wrong(got, want)
    ctx.close()
