"""The block writer of tests/dna_streams.py, without a GPU: it writes the format (the oracle encoder's own bytes when given the
encoder's own choices), every policy's streams decode to the reads through the oracle, and every policy's streams hold what its
GPU test (tests/test_gpu_dna_streams.py) is there to exercise."""
import random

import numpy as np
import pytest

import common
import dna_streams as S
import oracle_lib as O


@pytest.mark.parametrize("k", [21, 31, 47])
def test_writer_reproduces_the_oracle_encoder_byte_for_byte(k):
    """anchor = given, fed with the oracle encoder's traced choices, every other knob off: the same payloads.  Ties the writer to the
    format independently of any decoder (reads without an anchor, reads shorter than k, N, errors, ragged lengths among them)."""
    rpb = 70
    bases, off = common.synthetic(300, 120 if k < 32 else 200, 3000, seed=k, err=0.03, n_rate=0.005, ragged=True, junk_reads=10)
    bl, _, _ = common.make_bloom(bases, off, k)
    ref = O.encode(bases, off, k, rpb, bl, trace=True)
    reads = S.split_reads(bases, off)
    given = [None if ref.anchor_pos[i] < 0 else (int(ref.anchor_pos[i]), int(ref.anchor_addr[i]), int(ref.flags[i]) & 1)
             for i in range(len(reads))]
    assert sum(g is None for g in given) >= 10 and any(g and g[2] for g in given) and any(g and not g[2] for g in given)
    blocks, nbases, facts = S.build_blocks(reads, k, rpb, bl, O.kmers_to_ints(ref.anchor_kmers, k), random.Random(0),
                                           S.Policy(anchor="given", given=given))
    assert len(blocks) == len(ref.blocks) == 5
    for b in range(len(blocks)):
        assert blocks[b][1] == ref.blocks[b], "block %d" % b
        assert blocks[b][2] == ref.block_nreads[b]
    assert facts["noanchor"] == sum(g is None for g in given) and facts["n_err"] > 0


def _oracle_decodes(inp, blocks, nbases, reads):
    aw = S.words(inp.anchors, inp.k)
    r0 = 0
    for (b, payload, n), nb in zip(blocks, nbases):
        got = O.decode_block(inp.k, inp.bloom, aw, payload, n, nb + 16)
        assert got == [S.norm(r) for r in reads[r0:r0 + n]], "block %d" % b
        r0 += n


@pytest.mark.parametrize("k", [31, 32, 63, 21])
@pytest.mark.parametrize("name", list(S.POLICIES))
def test_every_policy_decodes_through_the_oracle_and_holds_what_it_is_for(name, k):
    inp = S.base_input(k)
    blocks, nbases, facts = S.build_blocks(inp.reads, k, inp.rpb, inp.bloom, inp.anchors, random.Random(k), S.POLICIES[name], inp.cache)
    S.check_facts(name, facts)
    _oracle_decodes(inp, blocks, nbases, inp.reads)


def test_the_dictionary_is_not_the_encoders():
    """shuffled, with unused k-mers, with k-mers present in both orientations, with k-mers over an N"""
    inp = S.base_input(31)
    d = set(inp.anchors)
    both = [x for x in d if S.revcomp(x, 31) in d and S.revcomp(x, 31) != x]
    assert len(both) >= 80
    f = S.build_blocks(inp.reads, 31, inp.rpb, inp.bloom, inp.anchors, random.Random(1), S.POLICIES["over_n"], inp.cache)[2]
    assert f["anchored_over_n"] >= 20


@pytest.mark.parametrize("rpb", [1, 7])
def test_block_shapes(rpb):
    inp = S.base_input(31)
    blocks, nbases, facts = S.build_blocks(inp.reads, 31, rpb, inp.bloom, inp.anchors, random.Random(rpb), S.POLICIES["mixed"], inp.cache)
    assert len(blocks) == (400 + rpb - 1) // rpb
    _oracle_decodes(inp, blocks, nbases, inp.reads)


def test_a_read_that_is_only_its_anchor():
    inp = S.base_input(31)
    reads = S.only_anchor_reads(inp)
    blocks, nbases, facts = S.build_blocks(reads, 31, 100, inp.bloom, inp.anchors, random.Random(3), S.POLICIES["pad"], inp.cache)
    assert facts["len_eq_k"] > 0
    _oracle_decodes(inp, blocks, nbases, reads)


def test_long_error_list():
    inp = S.long_list_input()
    pol = S.Policy(anchor="random", extra_err=1.0)
    for reads in ([inp.long], inp.short[:150] + [inp.long] + inp.short[150:]):
        blocks, nbases, facts = S.build_blocks(reads, inp.k, 1000, inp.bloom, inp.anchors, random.Random(2), pol, inp.cache)
        assert facts["longest_err_list"] > 8192
        _oracle_decodes(inp, blocks, nbases, reads)


def test_self_complementary_anchor():
    inp = S.selfrc_input()
    blocks, nbases, facts = S.build_blocks(inp.reads, inp.k, 8, inp.bloom, inp.anchors, random.Random(4),
                                           S.Policy(anchor="given", given=inp.given), inp.cache)
    assert facts["selfrc_flag0"] == facts["selfrc_flag1"] == len(inp.reads) // 2
    _oracle_decodes(inp, blocks, nbases, inp.reads)
