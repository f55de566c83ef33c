"""No GPU: the dynamic-code streams of deflate_cases.py are what they are named for.  Every valid case inflates under zlib to the end
of its stream and has, by the scanner of deflate_tokens.py, the property in its name; every refusal is refused by zlib for the reason
it is built for; and the two host functions the device entries answer to -- leon_host_qual_decode_blocks, leon_host_bgzf_inflate --
give zlib's verdict on all of them.  test_gpu_inflate_dynamic.py then runs the same streams through the device."""
import gzip
import random
import zlib

import numpy as np
import pytest

import bgzf_input as B
import deflate_cases as C
import deflate_tokens as T
import test_gpu_bgzf_inflate as G                                  # (their host_verdict helpers need no device)
import test_gpu_qual_inflate as Q

VALID, REFUSED = C.cases()


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def ident(case):
    return case.name[:60].replace(" ", "_")


# ---- the scanner itself ------------------------------------------------------------------------------------------------------------

def test_scanner_reads_zlibs_own_streams():
    """the scanner against an encoder it did not come with: the text is zlib's, and no repeat of zlib's crosses the HLIT boundary"""
    rng = random.Random(1)
    text = B.match_text(1) + B.fastq_text(30000, seed=2) + bytes(rng.randrange(256) for _ in range(3000))
    kinds = set()
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                            (6, zlib.Z_FIXED), (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)):
        raw = B.deflate_raw(text, level=level, strategy=strategy, flush_at=40000)
        rep = T.scan(raw)
        assert rep["text"] == text and (rep["bits"] + 7) // 8 == len(raw)
        for b in rep["blocks"]:
            kinds.add(b["kind"])
            assert b["kind"] != "dynamic" or (not b["crossed"] and 14 <= b["hclen"] <= 19)
    assert kinds == {"stored", "fixed", "dynamic"}


def test_writer_pieces():
    assert T.complete_lengths(8, 7) == [1, 2, 3, 4, 5, 6, 7, 7] and T.complete_lengths(17, 7).count(7) == 2
    assert T.canonical([2, 1, 3, 3]) == [(2, 2), (0, 1), (6, 3), (7, 3)]                                    # RFC 1951 3.2.2's example: A 10, B 0, C 110, D 111
    assert T.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert T.expand([("len", 4), ("rep", 3), ("zeros", 11), ("rep", 4)]) == [4] * 4 + [0] * 15
    assert [T.item_symbol(i) for i in (("zeros", 3), ("zeros", 10), ("zeros", 11), ("zeros", 138), ("rep", 6))] == [(17, 0, 3), (17, 7, 3), (18, 0, 7), (18, 127, 7), (16, 3, 2)]
    assert T.length_symbol(258) == (285, 0) and T.length_symbol(257) == (284, 30) and T.distance_symbol(32768) == (29, 8191)
    # the same tokens in the fixed code: bgzf_input's writer and this one agree bit for bit
    tokens = [b"hello, hello\n", (5, 7), (258, 1), bytes([200, 143, 144, 255]), (3, 13)]
    assert T.Stream().fixed(tokens, final=True).done() == B.fixed_stream(tokens)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", VALID, ids=ident)
def test_valid_case_has_its_property(case):
    d = zlib.decompressobj(-15)
    text = d.decompress(case.raw)
    assert d.eof and not d.unused_data and text == case.text
    rep = T.scan(case.raw)
    assert rep["text"] == text and (rep["bits"] + 7) // 8 == len(case.raw)
    case.check(rep)
    assert any(b["kind"] == "dynamic" for b in rep["blocks"])
    if C.ZLIB in case.paths:
        pay, n_reads, n_bytes = case.block()
        d = zlib.decompressobj()
        assert d.decompress(pay) == text and d.eof and not d.unused_data
        assert text.endswith(b"\n") and text.count(b"\n") == n_reads and len(text) == n_reads + n_bytes
    if C.RAW in case.paths:
        assert gzip.decompress(case.member()) == text


@pytest.mark.parametrize("case", REFUSED, ids=ident)
def test_refused_case_is_refused_for_its_reason(case):
    why = T.refusal(case.raw)
    assert why is not None, "zlib accepts it"
    assert case.words in why if case.words else why == "", why
    assert Q.refused_by_zlib(case.block()[0])
    with pytest.raises((zlib.error, EOFError, OSError)):
        gzip.decompress(case.member())


def test_the_cases_cover_what_they_are_for():
    """over all valid cases, per path: 15-bit codes in both alphabets and a 7-bit code-length code in use, every repeat symbol across
    the boundary, HCLEN from 5 to 19, every length and distance symbol at both ends of its extra bits, block chains of every kind"""
    for path in (C.ZLIB, C.RAW):
        blocks = [b for c in VALID if path in c.paths for b in T.scan(c.raw)["blocks"]]
        dyn = [b for b in blocks if b["kind"] == "dynamic"]
        assert max(b["ll_used"] for b in dyn) == 15 and max(b["d_used"] for b in dyn) == 15 and max(b["cl_used"] for b in dyn) == 7
        assert set().union(*(b["crossed"] for b in dyn)) == {16, 17, 18}
        assert {5, 18, 19} <= {b["hclen"] for b in dyn} and {257, 286} <= {b["hlit"] for b in dyn} and {1, 30} <= {b["hdist"] for b in dyn}
        lens, dists = {}, {}
        for b in dyn:
            for s, seen in b["len_syms"].items():
                lens.setdefault(s, set()).update(seen)
            for s, seen in b["dist_syms"].items():
                dists.setdefault(s, set()).update(seen)
        assert T.extremes(lens, B.LEN_EXTRA, 257) == set(range(257, 286)) and T.extremes(dists, B.DIST_EXTRA, 0) == set(range(30)) and 31 in lens[284]
        kinds = [b["kind"] for b in blocks]
        pairs = set(zip(kinds, kinds[1:]))
        assert {("dynamic", "fixed"), ("fixed", "dynamic"), ("fixed", "fixed"), ("dynamic", "stored"), ("stored", "fixed")} <= pairs


# ---- the host functions give zlib's verdicts ---------------------------------------------------------------------------------------

def test_host_functions_accept_the_valid_cases(built):
    zs = [c for c in VALID if C.ZLIB in c.paths]
    blocks = [c.block() for c in zs]
    got = Q.host_verdict(blocks)
    assert isinstance(got, list), got
    assert b"".join(l + b"\n" for l in got) == b"".join(c.text for c in zs)
    for c in zs:                                                   # and each alone
        assert Q.host_verdict([c.block()]) == c.text[:-1].split(b"\n"), c.name
    rs = [c for c in VALID if C.RAW in c.paths]
    data = b"".join(c.member() for c in rs)
    assert G.host_verdict(data, B.offsets_of(data)) == b"".join(c.text for c in rs)


def test_host_functions_refuse_the_refused_cases(built):
    good = [c for c in VALID if C.RAW in c.paths]
    for i, case in enumerate(REFUSED):
        a, b = good[i % len(good)], good[(i + 5) % len(good)]
        got = Q.host_verdict([a.block(), case.block(), b.block()])
        assert isinstance(got, tuple) and got[0] == -1 and "quality block 1 does not decode" in got[1], (case.name, got)
        members = [a.member(), b.member(), case.member(), a.member()]
        off = np.cumsum([0] + [len(m) for m in members]).astype(np.uint64)
        got = G.host_verdict(b"".join(members), off)
        assert isinstance(got, tuple) and got[0] == -1 and ("BGZF member 2 (at byte %d) does not decode" % int(off[2])) in got[1], (case.name, got)
