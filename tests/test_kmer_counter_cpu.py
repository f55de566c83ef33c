"""CPU tests of what the solid k-mer counter is checked against (test_gpu_kmer_counter.py): the plain Python count of kmer_shapes.py
gives the oracle's sets on every input, its automatic threshold is the rule of leon_kmer_auto_cutoff -- and the library's own (host-only)
leon_kmer_auto_cutoff follows that rule.  No GPU."""
import os

import numpy as np
import pytest

import kmer_shapes as S
import oracle_lib as O

INPUTS = list(S.all_inputs())


@pytest.fixture(scope="module")
def capi():
    import leon_amd
    if not os.path.exists(leon_amd.lib_path()):
        leon_amd.build_library()
    leon_amd.load_library()
    from leon_amd import capi
    return capi


@pytest.mark.parametrize("name,reads,k", INPUTS, ids=[i[0] for i in INPUTS])
def test_reference_counts_equal_the_oracle(name, reads, k):
    bases, off = S.arrays(reads)
    counts = S.ref_counts(reads, k)
    assert sum(counts.values()) <= S.total_positions(reads, k)
    top = max(counts.values())
    for t in S.THRESHOLDS:
        if t > 3 and t > top + 1:                                 # (the input has nothing there: one threshold above its largest count is enough)
            continue
        assert np.array_equal(S.sorted_words(O.count_solid(bases, off, k, t), k), S.ref_solid(reads, k, t)), (name, t)


def test_inputs_are_what_they_are_built_to_be():
    for k in S.EXACT_K:
        assert np.array_equal(S.ref_hist(S.ref_counts(S.exact_abundances(k), k)), S.spectrum_hist(S.EXACT_SPECTRUM))
        assert np.array_equal(S.ref_hist(S.ref_counts(S.valley(k), k)), S.spectrum_hist(S.VALLEY_SPECTRUM))
        assert np.array_equal(S.ref_hist(S.ref_counts(S.no_valley(k), k)), S.spectrum_hist(S.NO_VALLEY_SPECTRUM))
        assert sorted(S.ref_counts(S.exact_abundances(k), k).values()) == sorted(a for a, u in S.EXACT_SPECTRUM for _ in range(u))
        assert all(len(r) == k for r in S.valley(k))
    h = S.spectrum_hist(S.EXACT_SPECTRUM)
    assert [int(h[a]) for a in (1, 2, 3, 254, 255)] == [3, 3, 3, 3, 12] and int(h.sum()) == 24
    for k, distinct in ((3, 32), (4, 136)):
        h = S.ref_hist(S.ref_counts(S.tiny_k(k), k))
        assert int(h[255]) == distinct and int(h.sum()) == distinct
    for k in S.LONG_K:
        reads = S.long_reads(k)
        assert sorted(len(r) for r in reads) == [0, 4, k - 1, k] + [20000] * 7
        assert len(reads) <= 256 and sum((len(r) + 31) // 32 for r in reads) > S.PACK_MAP          # one workgroup of k_pack, by bisection
        assert sum(r.count(b"N") for r in reads) >= 7 * 55 and sum(sum(c not in b"ACGTN" for c in r) for r in reads) == 4
        h = S.ref_hist(S.ref_counts(reads, k))
        assert h[1] and h[2] and h[3]                             # k-mers repeat: the thresholds 1, 2, 3 select different sets


def test_reference_cutoff_on_the_constructed_spectra():
    assert S.ref_cutoff(S.spectrum_hist(S.VALLEY_SPECTRUM)) == 40
    assert S.ref_cutoff(S.spectrum_hist(S.NO_VALLEY_SPECTRUM)) == 2
    assert S.ref_cutoff(np.zeros(256, dtype=np.uint64)) == 2
    h = np.zeros(256, dtype=np.uint64)
    h[1], h[2] = 5, 9                                             # stops falling at 1: never below 2
    assert S.ref_cutoff(h) == 2
    h[:] = 0
    h[1:7] = [90, 40, 20, 10, 10, 30]                             # a plateau counts as "stops falling"
    assert S.ref_cutoff(h) == 4
    h[:] = 0
    h[1:255] = 1000 - np.arange(1, 255)
    h[255] = h[254]                                               # the last bin takes part
    assert S.ref_cutoff(h) == 254


def test_library_cutoff_follows_the_rule(capi):
    hists = [S.spectrum_hist(S.VALLEY_SPECTRUM), S.spectrum_hist(S.NO_VALLEY_SPECTRUM), S.spectrum_hist(S.EXACT_SPECTRUM), np.zeros(256, dtype=np.uint64)]
    hists += [S.ref_hist(S.ref_counts(reads, k)) for _, reads, k in INPUTS]
    rng = np.random.default_rng(46)
    for _ in range(50):                                           # and on spectra of any shape: a valley anywhere, gaps, a lone last bin
        h = np.zeros(256, dtype=np.uint64)
        n = int(rng.integers(1, 256))
        h[1:1 + n] = np.sort(rng.integers(0, 1000, n))[::-1]
        h[rng.integers(1, 256, 3)] = rng.integers(0, 1000, 3)
        hists.append(h)
    for h in hists:
        assert capi.kmer_auto_cutoff(h) == S.ref_cutoff(h), h.tolist()
