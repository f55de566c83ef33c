"""CPU tests of the lossy quality smoothing's shapes (qual_shapes.py): conditions that must hold from the oracle alone, so that
test_gpu_qual_smooth.py compares the device with cases that are what their names say.  No GPU, and nothing of the library under test
but its binding's declarations."""
import numpy as np
import pytest

import oracle_lib as O
import qual_shapes as S


@pytest.mark.parametrize("name", S.DESIGNED)
def test_designed_cases_have_exactly_their_coverage(name):
    """coverage >= 2 on the designed positions and nowhere else: read off lo_qual_smooth with qualities of '!', and counted again from
    Bloom.contains at every k-mer position"""
    c = S.case(name)
    bl, k = c.bloom(), c.k
    assert c.n >= 256 and len(c.designed) == c.n
    some = 0
    for i in range(c.n):
        r = c.read(i)
        if len(r) < k:
            assert len(c.designed[i]) == 0
            continue
        assert np.array_equal(S.oracle_coverage(bl, k, r), c.designed[i]), (name, i)
        solid = [p for p, x in enumerate(S.canonical_kmers(r, k)) if bl.contains(x)]
        assert np.array_equal(S.covered_twice(solid, len(r), k), c.designed[i]), (name, i)
        some += len(c.designed[i]) > 0
    assert some >= 6


@pytest.mark.parametrize("k", S.DESIGNED_K)
def test_designed_cases_hold_what_the_kernels_can_get_wrong(k):
    """every read length from k to k + 65 the list names, and for the longest read the joins: two solid k-mers at 63 and 64 give coverage
    >= 2 on [64, 63 + k - 1] only; a pair k - 1 apart one base; a pair k apart none; one solid k-mer none"""
    c = S.case("designed-k%d-h7-b12" % k)
    by_what = {w: i for i, w in enumerate(c.what)}
    assert set(S.read_lengths(k)) >= {k, k + 1, k + 31, k + 32, k + 63, k + 64, k + 65, 191 + k}
    for length in S.read_lengths(k):
        assert "one, length %d" % length in by_what and "all, length %d" % length in by_what
        d = c.designed[by_what["all, length %d" % length]]
        assert np.array_equal(d, np.arange(1, length - 1)) if length > k else len(d) == 0
        assert len(c.designed[by_what["one, length %d" % length]]) == 0
    longest = 191 + k
    for a in S.PAIR_STARTS:
        assert np.array_equal(c.designed[by_what["pair %d, length %d" % (a, longest)]], np.arange(a + 1, a + k))
    assert len(c.designed[by_what["k - 1 apart, length %d" % longest]]) == 1
    assert len(c.designed[by_what["k apart, length %d" % longest]]) == 0
    assert np.array_equal(c.designed[by_what["pair last, length %d" % (k + 1)]], np.arange(1, k))


@pytest.mark.parametrize("k", S.DESIGNED_K)
def test_every_read_length_from_k_to_k_plus_65(k):
    c = S.case("lengths-k%d-to-k+65" % k)
    by_what = {w: i for i, w in enumerate(c.what)}
    assert sorted(set(int(x) for x in c.lengths())) == list(range(k, k + 66))
    for length in range(k + 1, k + 66):
        nk = length - k + 1
        assert np.array_equal(c.designed[by_what["all, length %d" % length]], np.arange(1, length - 1))
        assert np.array_equal(c.designed[by_what["pair 0, length %d" % length]], np.arange(1, k))
        assert np.array_equal(c.designed[by_what["pair last, length %d" % length]], np.arange(nk - 1, nk + k - 2))
        assert np.array_equal(c.designed[by_what["first and last, length %d" % length]], np.arange(nk - 1, k))


def test_every_geometry_and_k_is_a_case():
    for k in S.DESIGNED_K:
        for h, b in S.GEOMETRIES:
            c = S.case("designed-k%d-h%d-b%d" % (k, h, b))
            assert (c.k, c.geometry, c.tai) == (k, (h, b), 200000)
    assert {32, 33} <= set(S.DESIGNED_K) and len(S.GEOMETRIES) == 6


def test_n_is_read_as_a():
    for k in (31, 32):
        plain, poly = S.case("n-k%d-plain" % k), S.case("n-k%d-polyA" % k)
        for c, covered in ((plain, False), (poly, True)):
            seen = 0
            for i in range(c.n):
                r = c.read(i)
                if r and set(r) == {ord("N")} and len(r) > k:
                    assert np.array_equal(c.designed[i], np.arange(1, len(r) - 1) if covered else []), (c.name, i)
                    seen += 1
                if b"N" in r and 0 < r.count(b"N") <= 3 and len(r) == 150 and len(c.designed[i]):
                    assert np.array_equal(c.designed[i], np.arange(36, 35 + k)), (c.name, i)       # the pair at (35, 36), through the N
                    seen += 10
            assert seen >= 33, c.name
    c = S.case("n-k32-plain")
    i = [c.read(i) for i in range(c.n)].index(b"ACGT" * 16)                # solid at 0, 4, .., 32: twice covered from 4 to 59
    assert np.array_equal(c.designed[i], np.arange(4, 60))
    assert S.revcomp(b"AACGTNG") == b"CNACGTT" and S.revcomp(b"ACGT" * 8) == b"ACGT" * 8
    r = S.random_read(np.random.default_rng(1), 80)
    assert S.canonical_kmers(S.revcomp(r), 32) == S.canonical_kmers(r, 32)[::-1]


@pytest.mark.parametrize("name", S.RANDOM)
def test_random_cases_change_something_and_leave_something(name):
    c = S.case(name)
    want, q = S.expected(c), c.quals
    changed = left_low = 0
    for i in c.touched():
        s, e = int(c.off[i]), int(c.off[i + 1])
        changed += int(np.count_nonzero((want[s:e] != q[s:e]) & (q[s:e] < ord("@"))))     # changed by coverage, not by truncation
        left_low += int(np.count_nonzero((want[s:e] == q[s:e]) & (q[s:e] < ord("@"))))
    assert changed > 0 and left_low > 0, (name, changed, left_low)
    if name.startswith(("genome", "small")):                               # reads shorter than k and empty ones in between
        assert (c.lengths() == 0).any() and ((c.lengths() > 0) & (c.lengths() < c.k)).any()


def test_counts_sit_either_side_of_the_switches():
    assert S.COUNTS == [1, 255, 256, 257, 16389]
    for n in S.COUNTS:
        assert S.case("count-%d" % n).n == n
    c = S.case("long-read-70000")
    assert c.lengths().max() == 70000 and c.n == 301 and c.read(123).count(b"N") > 20
    g = S.case("genome-k31")
    assert g.n > 5000


def test_the_huge_case():
    c = S.case(S.HUGE)
    assert c.n == (1 << 21) + 300 and isinstance(c.bases, np.ndarray) and c.quals.dtype == np.uint8
    lengths = c.lengths()
    assert (lengths[:150] >= c.k).all() and (lengths[150:1 << 21] == 8).all() and (lengths[c.n - 150:] >= c.k).all() and (lengths[(1 << 21):c.n - 150] == 8).all()
    want = S.expected(c)
    behind = [i for i in c.check if i >= (1 << 21)]
    assert len(behind) == 150
    assert sum(not np.array_equal(want[int(c.off[i]):int(c.off[i + 1])], c.quals[int(c.off[i]):int(c.off[i + 1])]) for i in behind) >= 100
    untouched = np.ones(len(want), dtype=bool)
    for i in c.check:
        untouched[int(c.off[i]):int(c.off[i + 1])] = False
    assert np.array_equal(want[untouched], c.quals[untouched])


@pytest.mark.parametrize("name", ["designed-k32-h7-b12", "n-k31-polyA", "small-k5-h3-b9", "genome-k47", "count-257", "long-read-70000"])
def test_the_rule_is_idempotent(name):
    """the CLI does a failed call again in halves: a second application changes nothing"""
    c = S.case(name)
    bl, want = c.bloom(), S.expected(c)
    for i in c.touched():
        s, e = int(c.off[i]), int(c.off[i + 1])
        once = want[s:e].tobytes()
        assert O.qual_smooth(bl, c.k, c.read(i), once) == once, (name, i)


def test_stale_anchor_pair():
    a, b = S.stale_pair()
    assert a.n == b.n and len(b.bases) < len(a.bases) and a.solid == b.solid
    lb = b.lengths()
    assert (lb < b.k).sum() >= 100 and ((lb >= b.k) & (lb <= b.k + 2)).sum() >= 100 and (a.lengths() == 100).all()
    assert not np.array_equal(S.expected(b), b.quals)


def test_quality_lines_hold_every_byte_value():
    q = S.quality_lines([300] * 8, 1)
    assert len(np.unique(q[:300])) == 256 and set(np.unique(q[300:600])) == {ord("?"), ord("@"), ord("A")} and (q[600:900] == ord("@")).all()
    assert (q >= 0x80).any()


def test_the_device_entry_is_bound():
    import ctypes
    import os
    from leon_amd import capi
    assert capi.ABI_VERSION == 5
    assert "leon_qual_smooth_batch_device" in capi.EXPORTED_SYMBOLS and callable(capi.DnaEncodeContext.qual_smooth_batch_device)
    if os.path.exists(capi.lib_path()):
        assert hasattr(ctypes.CDLL(capi.lib_path()), "leon_qual_smooth_batch_device")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "leon_dna.h")).read()
    assert "int leon_qual_smooth_batch_device(leon_dna_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads," in header
