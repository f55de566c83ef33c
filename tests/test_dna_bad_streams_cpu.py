"""No GPU: the cases of tests/dna_bad_streams.py are what they claim to be, certified from the oracle and the writer alone -- so that
tests/test_gpu_dna_refusals.py holds the device decoder to statements nobody derived from a decoder under test."""
import hashlib
import random

import pytest

import dna_bad_streams as B
import dna_streams as S
import oracle_lib as O

# the oracle's refusals against the device's: -1 is a read without anchor that overflows the block's bases (device 2); -2 is what the
# oracle reports for an anchored read's address, position AND overflow together (device 1 or 2); -3 a list count above len (device 3).
# The oracle never notices a payload's end (device 4): it reads zero bytes for ever.
ORACLE_CODES = {1: ("-2",), 2: ("-1", "-2"), 3: ("-3",)}


def _oracle_block(case, blocks, b):
    _, payload, n = blocks[b]
    return O.decode_block(case.k, S.base_input(case.k).bloom, S.words(case.anchors, case.k), payload, n, case.nbases[b])


@pytest.mark.parametrize("k", [31, 63])
def test_refusal_cases_are_what_they_say(k):
    cases = B.refusal_cases(k)
    names = {c.name.split(",")[0] for c in cases}
    assert len(cases) >= (15 * 3 + 13 if k == 31 else len(B.K63_SUBSET)) and (k != 31 or "empty-dictionary" in names)
    seen = set()
    for c in cases:
        if c.bad_syms:                                         # the stream up to the bad read is the conforming one, and ends with that read's fields
            bad, twin, at = c.bad_syms
            assert 0 <= at < len(bad) < len(twin) and bad[:at] == twin[:at], c.name
            assert bad[at:] != twin[at:len(bad)], c.name
        for b in (0, 2, 3):                                    # the other blocks decode
            if c.name != "empty-dictionary":
                assert c.blocks[b] == B.good(k)[1][b]
        if c.code == B.ANY or not c.oracle:                    # marked: the oracle's checks are sums, and they wrap
            continue
        if c.name == "reads-1":                                # the oracle has no table to compare with: it stops a read short of the bases
            got = _oracle_block(c, c.blocks, 1)
            assert sum(len(r) for r in got) < c.nbases[1]
            continue
        with pytest.raises(ValueError) as e:
            _oracle_block(c, c.blocks, c.bad_block)
        assert str(e.value).split()[-1] in ORACLE_CODES[c.code], (c.name, str(e.value))
        seen.add(c.code)
    assert seen == {1, 2, 3}


def test_two_bad_blocks():
    c = B.two_bad_blocks()
    assert c.bad_block == 0 and c.blocks[1:3] == B.good(31)[1][1:3]
    for b, codes in ((0, ORACLE_CODES[1]), (3, ORACLE_CODES[2])):
        with pytest.raises(ValueError) as e:
            _oracle_block(c, c.blocks, b)
        assert str(e.value).split()[-1] in codes


@pytest.mark.parametrize("k", [31, 63])
def test_odd_lists_decode_through_the_oracle(k):
    cases = B.decode_cases(k)
    assert len(cases) >= (14 * 3 + 3 if k == 31 else len(B.K63_ODD) + 3)
    rpb = S.base_input(k).rpb
    for c in cases:
        got = []
        for b in range(len(c.blocks)):
            got += _oracle_block(c, c.blocks, b)
        assert got == c.reads, c.name
        if c.name.startswith("empty block"):
            assert sum(1 for _, p, n in c.blocks if n == 0 and p == b"") == 1 and len(c.blocks) == 5
            continue
        assert c.reads != B.good_reads(k)                      # the chosen read carries N the input does not
        mine = c.reads[rpb + c.ri]
        assert mine.count(b"N") == 6
        if "repeat-middle" in c.name or "repeat-both" in c.name or "thrice" in c.name:
            assert c.repeats_walked >= (2 if "both" in c.name else 1), c.name
        if c.twin:                                             # without the entries behind the repeats the read is another one: they matter
            try:                                               # (out of step with its symbols from there on: it may even stop decoding)
                other = _oracle_block(c, c.twin, 1)[c.ri]
            except ValueError:
                other = None
            assert other != mine, c.name


def test_pool_cases_need_what_they_say():
    many = B.pool_case("many")
    assert len(many.n_lists) == 124 and min(many.n_lists) > B.DC_LIST_CAP
    assert sum(many.n_lists) > B.FIRST_POOL_FLOOR and sum(many.nbases) < 2 * B.FIRST_POOL_FLOOR
    grow = B.pool_case("growing")
    assert sum(grow.nbases) < 2 * B.FIRST_POOL_FLOOR and min(grow.n_lists) > B.DC_LIST_CAP
    need = 0                                                   # what the blocks take from the first pool (DESIGN.md 4.5's rule)
    for b in range(len(grow.blocks)):
        a, z = grow.n_lists[2 * b], grow.n_lists[2 * b + 1]
        left = len(grow.reads[2 * b + 1])
        assert z > a
        need += a + min(max(z, 2 * a), left)
    assert need > B.FIRST_POOL_FLOOR
    assert 2 * sum(grow.nbases) >= need                        # ... and the second pool holds it
    # (the oracle's list membership is a linear search: these lists are beyond what it decodes in a test's time -- the expected reads are the input's)


# build_blocks on base_input(31) for every policy, payloads and read counts, before dna_streams.build_block took a `tamper`
DIGESTS = {
    "base": "ba67b6724512c34a7fd9ef463ba135c7b08a750e088802fb1f0a5485c074d52a",
    "last": "7096ac78e6937bf72fca749857f76c837fa55fa1bce972340f88bbd68e242c4e",
    "free": "9ac9929676f353ea4772c9335024652276fd7d8b775b03464440e4d667b3f76e",
    "pad": "2444ba615e8046fafb5b8062bdc3edaeaccc309f35e37bce6f6e05eab1fa990c",
    "over_n": "9eb6c9641b8364d8419b34a6cca8a7643751143e359475a59873b994ec7d3b09",
    "extra": "5ffadaff74105f6017aa40cb535de5745d3997cc222d8f5d1ce82d4cb40ea5fa",
    "all_err": "d594a6147b5192a2ec93bfff10e973cef9ba67f80216da813bac90bf6231f373",
    "mixed": "e257a41272cbabfcdcf141fd7ca1f8166563cff62e814d0d5d66486e45c26af1",
    "edges": "30da592abd1eeacb1953c5b426d030fbf949dc12a763d7a522f1ed7b28762bd5",
}


def test_the_hook_leaves_every_policy_as_it_was():
    inp = S.base_input(31)
    for name, pol in S.POLICIES.items():
        blocks, nbases, _ = S.build_blocks(inp.reads, 31, inp.rpb, inp.bloom, inp.anchors, random.Random(31), pol, inp.cache)
        h = hashlib.sha256()
        for b, payload, n in blocks:
            h.update(b"%d %d %d\n" % (b, n, len(payload)))
            h.update(payload)
        assert h.hexdigest() == DIGESTS[name], name
    # and a Tamper that replaces nothing is no change either
    payload, _, t, _, _, _ = B.write(31, 1, "first")
    reads, given, _, _, _, _ = B.layout(31, 1, "first")
    assert payload == S.build_block(reads, 31, inp.bloom, inp.anchors, random.Random(1), S.Policy(anchor="given", given=given), inp.cache)[0]
