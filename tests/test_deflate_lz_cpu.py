"""No GPU: tests/deflate_lz.py, the restatement of k_deflate_lz_chunks' parse, against zlib and against what every case
of tests/deflate_lz_cases.py is meant to be.  It guards the yardstick of test_gpu_bgzf_matches.py; no project code runs here."""
import pytest

import deflate_lz as Z
import deflate_lz_cases as K
import deflate_tokens as T

M = K.M
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 32767, 32768, 32769, 65541]


@pytest.fixture(scope="module")
def fastq():
    return K.fastq_fixture()


def code_of(freq, n_min):
    """{symbol: length} of a complete code over the used symbols (at least two of them)"""
    used = [s for s, f in enumerate(freq) if f]
    for s in range(n_min):
        if len(used) < 2 and s not in used:
            used.append(s)
    return T.balanced(sorted(used))


def through_zlib(text):
    """the restatement's tokens of one chunk, coded as a dynamic block and inflated by zlib; returns the tokens"""
    toks = Z.tokens(text)
    ll, dd, _ = Z.symbols(text, toks)
    raw = T.Stream().dynamic(code_of(ll, 2), code_of(dd, 2), Z.stream_tokens(text, toks), final=True).done()
    assert T.inflate(raw) == text
    at = 0
    for p, length, dist in toks:
        assert p == at and 1 <= length <= Z.MAX and p + length <= len(text)
        assert (dist == 0 and length == 1) or (1 <= dist <= p and length >= 3), (p, length, dist)
        assert dist <= 1 or length >= Z.MIN, "a hash token of %d bytes" % length
        at += length
    assert at == len(text)
    return toks


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case(name):
    through_zlib(K.CASES[name])


@pytest.mark.parametrize("n", SIZES)
def test_fastq_sizes(fastq, n):
    for a in range(0, max(n, 1), M):
        through_zlib(fastq[a:min(a + M, n)])


def test_the_cases_are_what_their_names_say():
    C = K.CASES
    match = {name: Z.matches(t) for name, t in C.items()}
    codes = {name: {i for i, f in enumerate(Z.symbols(C[name], Z.tokens(C[name]))[1]) if f} for name in C}
    # a source in the same step is not found; one step back it is; the longest distance a token of DF_LZ_MIN bytes can have
    assert match["gram_at_255"] == [] and match["gram_at_32764"] == []
    for d in (256, 257, 32763):
        assert match["gram_at_%d" % d] == [(d, 5, d)]
    n = len(C["ends_at_n"])
    assert match["ends_at_n"] == [(n - 40, 40, n - 40 - 20)] and match["cut_by_n"] == [(n - 40, 27, n - 40 - 20)]
    # matches of 258 back to back, one of them from a thread's last two positions into the third range behind it
    p300 = match["period_300"]
    assert all(l == 258 and d == 300 for _, l, d in p300[:-1]) and [p for p, _, _ in p300[:3]] == [300, 558, 816]
    assert any(p % 128 >= 126 and (p + l) // 128 == p // 128 + 3 for p, l, _ in p300)
    assert match["repeat_259"] == [(260, 258, 260)] and Z.tokens(C["repeat_259"])[-2:] == [(518, 1, 0), (519, 1, 0)]
    # runs against hash candidates: both kinds are taken
    for name in ("period_2", "period_3", "runs_and_repeats"):
        assert match[name], name
    assert {d for _, _, d in match["runs_and_repeats"]} >= {1, 8}
    assert codes["one_byte"] == {0} and all(l == 258 for _, l, _ in match["one_byte"][:-1])
    # the newest entry of the hash is another 4-gram: the repeat is found one byte late
    at = 3 * K.STEP + 10
    assert [m for m in match["collisions"] if m[0] <= at + 1] == [(at + 1, 9, 3 * K.STEP)]
    assert codes["no_distance_code"] == set() and Z.cost_bytes(C["no_distance_code"]) < len(C["no_distance_code"]) * 3 // 4
    assert len(codes["period_300"]) == 1
    assert codes["all_distance_codes"] == set(range(30))
    # 17 distance codes with Fibonacci counts: an unlimited Huffman code is 16 bits deep, the kernel's has to be cut to 15
    deep = Z.symbols(C["deep_distance_code"], Z.tokens(C["deep_distance_code"]))[1]
    assert sorted(f for f in deep if f) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    assert max(Z.huffman_lengths(deep)) == 16 and all(l == 5 for _, l, _ in match["deep_distance_code"])


def test_min_length_and_size_on_the_fastq_fixture(fastq):
    """DF_LZ_MIN by the token cost on the fixture, and the cap of test_gpu_bgzf_matches.py's size case cleared on the
    CPU: the restatement's tokens by unlimited Huffman codes plus 60 bytes of header a member, against zlib's Z_RLE"""
    import zlib
    parts = [fastq[a:a + M] for a in range(0, len(fastq), M)]
    cost = {m: sum(Z.cost_bytes(p, m) for p in parts) for m in (4, 5, 6)}
    rle = 0
    for p in parts:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        rle += len(c.compress(p) + c.flush())
    print("token cost on %d bytes, %d members: DF_LZ_MIN 4: %d, 5: %d, 6: %d; Z_RLE %d" % (len(fastq), len(parts), cost[4], cost[5], cost[6], rle))
    assert min(cost, key=cost.get) == Z.MIN
    assert cost[Z.MIN] + 2 * len(parts) <= 0.85 * rle
