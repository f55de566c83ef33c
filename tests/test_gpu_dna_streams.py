"""-m gpu: k_decode_blocks on read blocks a conforming writer may produce and the project's encoders never do (tests/dna_streams.py):
other anchors than the first, a shuffled non-canonical dictionary, anchors over an N, free delta types, padded numerics (all 72
numeric models: 58 in the global overflow area), errors listed where nothing forces them -- on one-successor steps (inside the
path cache's jumps), at dead ends, next to the anchor, at both ends of the read, more than the LDS and the block's scratch hold.
No encode comes first: the decoder is called on the written payloads, and must give the reads AND what the oracle's decoder gives."""
import functools
import random

import pytest

import dna_streams as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

CACHE_SETTINGS = ("0", None, "1")                    # LEON_DC_CACHE_MB (read per call): no path cache, its default size, 1 MiB


def _ctx(inp, rpb=100):
    import leon_amd
    ctx = leon_amd.DnaEncodeContext(kmer_size=inp.k, reads_per_block=rpb, bloom_tai=inp.tai, **inp.bloom_kw)
    ctx.bloom_upload(inp.bloom.bits)
    return ctx


def _oracle(inp, blocks, nbases):
    aw = S.words(inp.anchors, inp.k)
    out = []
    for (b, payload, n), nb in zip(blocks, nbases):
        out += O.decode_block(inp.k, inp.bloom, aw, payload, n, nb + 16)
    return out


def _set_cache(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("LEON_DC_CACHE_MB", raising=False)
    else:
        monkeypatch.setenv("LEON_DC_CACHE_MB", mb)


def _check(ctx, inp, blocks, nbases, reads, oracle_out, what, twice):
    want = [S.norm(r) for r in reads]
    aw = S.words(inp.anchors, inp.k)
    for call in range(2 if twice else 1):                 # the second call meets the table the first one filled
        got = ctx.decode_blocks(aw, blocks, nbases)
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s, call %d: read %d (block %d) is not what was written" % (what, call, i, i // max(blocks[0][2], 1))
        assert got == oracle_out, "%s, call %d: not what the oracle decodes" % (what, call)


@functools.lru_cache(maxsize=None)
def _streams(k, name):
    inp = S.base_input(k)
    blocks, nbases, facts = S.build_blocks(inp.reads, k, inp.rpb, inp.bloom, inp.anchors, random.Random(k), S.POLICIES[name], inp.cache)
    S.check_facts(name, facts)
    return blocks, nbases, _oracle(inp, blocks, nbases)


@pytest.mark.parametrize("mb", CACHE_SETTINGS, ids=["cache-off", "cache-default", "cache-1MiB"])
@pytest.mark.parametrize("k", [31, 32, 63, 21])            # 21: a bloom of 3 hash functions, the NH = 0 instantiation
def test_streams_of_every_policy(k, mb, monkeypatch):
    """all policies through one context, all blocks of a policy in one call; with the cache at its default size every call is made
    twice, so the errors listed by `extra` / `all_err` / `edges` fall inside table jumps; and what the table learnt from the odd streams
    must not change an ordinary one"""
    inp = S.base_input(k)
    _set_cache(monkeypatch, mb)
    ctx = _ctx(inp)
    for name in list(S.POLICIES) + ["base"]:
        blocks, nbases, oracle_out = _streams(k, name)
        _check(ctx, inp, blocks, nbases, inp.reads, oracle_out, "k %d, policy %s, cache %r" % (k, name, mb), twice=mb is None)
    ctx.close()


def _directed(inp, reads, rpb, policy, seed, monkeypatch, what, condition):
    blocks, nbases, facts = S.build_blocks(reads, inp.k, rpb, inp.bloom, inp.anchors, random.Random(seed), policy, inp.cache)
    condition(facts)
    oracle_out = _oracle(inp, blocks, nbases)
    for mb in CACHE_SETTINGS:
        _set_cache(monkeypatch, mb)
        ctx = _ctx(inp, rpb)
        _check(ctx, inp, blocks, nbases, reads, oracle_out, "%s, cache %r" % (what, mb), twice=mb is None)
        ctx.close()
    return blocks


@pytest.mark.parametrize("alone", [True, False], ids=["alone", "mid-block"])
def test_error_list_longer_than_the_block_scratch(alone, monkeypatch):
    """a 20 000-base read with every walked position listed: 19 969 entries, beyond the 64 in LDS and the 8 192 of the block's scratch
    -- the list lives in the shared pool, and both walks' cursors run over it"""
    inp = S.long_list_input()
    reads = [inp.long] if alone else inp.short[:150] + [inp.long] + inp.short[150:]

    def condition(f):
        assert f["longest_err_list"] > 8192, f
    _directed(inp, reads, 1000, S.Policy(anchor="random", extra_err=1.0), 2, monkeypatch, "long list", condition)


def test_anchor_that_is_its_own_reverse_complement(monkeypatch):
    """k = 32, the anchor s + revcomp(s): flag 0 and flag 1 name the same k-mer, and a reader of either gets the same read"""
    inp = S.selfrc_input()

    def condition(f):
        assert f["selfrc_flag0"] == f["selfrc_flag1"] == len(inp.reads) // 2, f
    _directed(inp, inp.reads, 8, S.Policy(anchor="given", given=inp.given), 4, monkeypatch, "self-complementary anchor", condition)


@pytest.mark.parametrize("rpb", [1, 7])
def test_blocks_of_one_and_of_seven_reads(rpb, monkeypatch):
    """400 and 58 blocks of the `mixed` policy: every block starts its models, its previous values and its numeric slots afresh"""
    inp = S.base_input(31)

    def condition(f):
        assert f["noanchor"] > 0 and f["anchored"] > 0, f
    blocks = _directed(inp, inp.reads, rpb, S.POLICIES["mixed"], rpb, monkeypatch, "rpb %d" % rpb, condition)
    assert len(blocks) == (400 + rpb - 1) // rpb


def test_a_read_that_is_only_its_anchor(monkeypatch):
    """len == k, anchored: no walk at all, with padded numerics around it"""
    inp = S.base_input(31)

    def condition(f):
        assert f["len_eq_k"] > 0, f
    _directed(inp, S.only_anchor_reads(inp), 100, S.POLICIES["pad"], 3, monkeypatch, "len == k", condition)
