"""-m gpu: the solid k-mer counter (kmer_kernels.hip: leon_kmer_solid, leon_kmer_solid_device) against the plain Python count of
kmer_shapes.py -- the set AND every bin of the abundance spectrum -- on inputs that make k_part_kmers claim many chunks, k_flag_runs clip
at 255, the automatic threshold land above 6, k = 3 and 4, empty partitions, and the device form take its bases from where they lie.
Every expectation comes from kmer_shapes.ref_counts / ref_hist / ref_cutoff, never from a device result."""
import ctypes as C

import numpy as np
import pytest

import kmer_shapes as S

pytestmark = pytest.mark.gpu

LEON_OK, LEON_E_INVALID, LEON_E_OVERFLOW = 0, -1, -5
_u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def capi():
    from leon_amd import capi
    capi.load_library()
    return capi


def _count(capi, reads, k, min_abundance, parts=1):
    """the host form at `parts` hash partitions: (sorted rows, histogram)"""
    bases, off = S.arrays(reads)
    per = S.keys_per_pass(reads, k, parts) if parts > 1 else 0          # (0: sized from the free memory, one partition for anything small)
    got, hist = capi.kmer_solid(bases, off, k, min_abundance, with_histogram=True, max_keys_per_pass=per)
    return S.sorted_words(got, k), hist


def _host_raw(capi, reads, k, min_abundance, out_cap, fill=0):
    """leon_kmer_solid itself: (return code, *n_solid, out, histogram); *n_solid and the histogram hold `fill` going in"""
    lib = capi.load_library()
    bases, off = S.arrays(reads)
    out = np.zeros(max(out_cap, 1) * S.kwords(k), dtype=np.uint64)
    hist = np.full(256, fill, dtype=np.uint64)
    ns = C.c_uint64(fill)
    rc = lib.leon_kmer_solid(0, bases, off.ctypes.data_as(_u64p), len(reads), k, min_abundance, 0, out.ctypes.data_as(_u64p), out_cap,
                             C.byref(ns), hist.ctypes.data_as(_u64p))
    return rc, ns.value, out, hist


def _device_raw(capi, d_bases, d_off, n_reads, k, min_abundance, per=0, with_histogram=True, fill=0):
    """leon_kmer_solid_device itself: (return code, sorted rows, histogram or None)"""
    lib = capi.load_library()
    hist = np.full(256, fill, dtype=np.uint64) if with_histogram else None
    p, ns = C.c_void_p(), C.c_uint64(fill)
    rc = lib.leon_kmer_solid_device(0, C.c_void_p(d_bases), C.c_void_p(d_off), n_reads, k, min_abundance, per, C.byref(p), C.byref(ns),
                                    hist.ctypes.data_as(_u64p) if with_histogram else None)
    try:
        nbytes = ns.value * 8 * S.kwords(k)
        flat = np.frombuffer(capi.device_download(p.value, nbytes), dtype=np.uint64) if rc == 0 and nbytes else np.zeros(0, dtype=np.uint64)
    finally:
        capi.device_free(p.value)
    return rc, S.sorted_words(flat, k), hist


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d k-mers, the reference has %d" % (what, len(got), len(want))


def _same_bins(hist, want, what):
    bad = np.flatnonzero(hist != want)
    assert not len(bad), "%s: bins %s are %s, the reference has %s" % (what, bad[:8].tolist(), hist[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("k", S.LONG_K)
def test_chunks_of_the_partition_pass(capi, k):
    """reads of 20 000 bases: a wave of k_part_kmers fills chunk after chunk (the pad in mid-stream, the next claim, padding between real
    keys before the sort, n = cursor - pads), at 1, 2, 4 and 7 partitions; N over the mask words' edges, k_pack's bisection"""
    reads = S.long_reads(k)
    want_hist = S.ref_hist(S.ref_counts(reads, k))
    longest = max(len(r) for r in reads) - k + 1
    for parts in (1, 2, 4, 7):
        # what the case rests on: the wave of the longest read selects about longest / parts k-mers, two chunks (PART_CHUNK slots,
        # kmer_kernels.hip) and more of every partition
        assert longest >= (2 if parts == 7 else 3) * S.PART_CHUNK * parts
        for min_abundance in (1, 2, 3):
            got, hist = _count(capi, reads, k, min_abundance, parts)
            what = "k %d, %d partitions, abundance %d" % (k, parts, min_abundance)
            _same(got, S.ref_solid(reads, k, min_abundance), what)               # (the same reference at every parts: the same set and bins)
            _same_bins(hist, want_hist, what)


@pytest.mark.parametrize("k", S.EXACT_K)
def test_clip_at_255_and_thresholds_above_it(capi, k):
    """units of exactly k bases at abundances 1, 2, 3, 254, 255, 256, 257 and 700: every bin, the clip, and thresholds either side of it"""
    reads = S.exact_abundances(k)
    want_hist = S.ref_hist(S.ref_counts(reads, k))
    for parts in (1, 3):
        for min_abundance in (1, 254, 255, 256, 257, 258, 700, 701):
            got, hist = _count(capi, reads, k, min_abundance, parts)
            what = "k %d, %d partitions, abundance %d" % (k, parts, min_abundance)
            want = S.ref_solid(reads, k, min_abundance)
            assert len(want) == S.UNITS_PER_ABUNDANCE * sum(a >= min_abundance for a in S.EXACT_ABUNDANCES)
            _same(got, want, what)
            _same_bins(hist, want_hist, what)
        rc, n_solid, _, hist = _host_raw(capi, reads, k, 701, out_cap=8, fill=99)
        assert (rc, n_solid) == (LEON_OK, 0)
        _same_bins(hist, want_hist, "k %d, nothing solid" % k)


@pytest.mark.parametrize("shape,cutoff", [("valley", 40), ("no_valley", 2)])
@pytest.mark.parametrize("k", S.EXACT_K)
def test_automatic_threshold_from_a_known_spectrum(capi, k, shape, cutoff):
    """min_abundance 0: the threshold of a spectrum built to have its first minimum at 40 (the two units seen 300 times are kept
    through a count clipped at 255), and of one that falls all the way (2)"""
    reads = getattr(S, shape)(k)
    want_hist = S.ref_hist(S.ref_counts(reads, k))
    assert S.ref_cutoff(want_hist) == cutoff
    want = S.ref_solid(reads, k, cutoff)
    assert len(want) == sum(u for a, u in (S.VALLEY_SPECTRUM if shape == "valley" else S.NO_VALLEY_SPECTRUM) if a >= cutoff)
    for parts in (1, 3):
        got, hist = _count(capi, reads, k, 0, parts)
        _same(got, want, "%s, k %d, %d partitions" % (shape, k, parts))
        _same_bins(hist, want_hist, "%s, k %d, %d partitions" % (shape, k, parts))
    bases, off = S.arrays(reads)                                             # and with no histogram asked for
    d_bases, d_off = capi.device_upload_bytes(bases), capi.device_upload_bytes(off.tobytes())
    try:
        rc, got, _ = _device_raw(capi, d_bases, d_off, len(reads), k, 0, with_histogram=False)
    finally:
        capi.device_free(d_bases)
        capi.device_free(d_off)
    assert rc == LEON_OK
    _same(got, want, "%s, k %d, no histogram" % (shape, k))


@pytest.mark.parametrize("k", S.TINY_K)
def test_tiny_k_and_empty_partitions(capi, k):
    """k = 3 and 4: 32 and 136 canonical k-mers seen thousands of times each (k_flag_runs' doubling search, everything in bin 255), at one
    partition and at fifty -- more partitions than k = 3 has k-mers"""
    reads = S.tiny_k(k)
    want = S.ref_solid(reads, k, 1)
    want_hist = S.ref_hist(S.ref_counts(reads, k))
    assert len(want) == (32, 136)[k - 3] and int(want_hist[255]) == len(want) and not want_hist[:255].any()
    for parts in (1, 50):
        for min_abundance in (1, 300):
            got, hist = _count(capi, reads, k, min_abundance, parts)
            _same(got, S.ref_solid(reads, k, min_abundance), "k %d, %d partitions, abundance %d" % (k, parts, min_abundance))
            _same_bins(hist, want_hist, "k %d, %d partitions" % (k, parts))
            assert not hist[:255].any()


@pytest.mark.parametrize("k", [31, 32])
def test_device_form_takes_the_bases_where_they_lie(capi, k):
    """leon_kmer_solid_device on reads that begin 4 097 bytes into a buffer with other ACGT text either side of them: first with
    d_offsets[0] = 4097, then with offsets from 0 and the (odd) pointer moved.  A byte taken from outside the reads would show as k-mers
    the reference does not have (abundance 1 keeps every one)."""
    reads = S.long_reads(k)
    bases, off = S.arrays(reads)
    rng = np.random.default_rng(4600 + k)
    front, behind = S.random_bases(rng, 4097), S.random_bases(rng, 4096)
    want_hist = S.ref_hist(S.ref_counts(reads, k))
    host = {m: _count(capi, reads, k, m)[0] for m in (1, 2)}
    d_buf = capi.device_alloc(len(front) + len(bases) + len(behind) + 64)
    d_moved = capi.device_upload_bytes((off + np.uint64(4097)).tobytes())
    d_zero = capi.device_upload_bytes(off.tobytes())
    try:
        data = front + bases + behind
        lib = capi.load_library()
        assert lib.leon_device_upload(0, C.c_void_p(d_buf), C.c_char_p(data), len(data)) == LEON_OK
        for what, d_bases, d_off in (("offsets from 4097", d_buf, d_moved), ("odd pointer", d_buf + 4097, d_zero)):
            for min_abundance, parts in ((1, 1), (2, 4)):
                per = S.keys_per_pass(reads, k, parts) if parts > 1 else 0
                rc, got, hist = _device_raw(capi, d_bases, d_off, len(reads), k, min_abundance, per, fill=77)
                assert rc == LEON_OK
                _same(got, S.ref_solid(reads, k, min_abundance), "%s, k %d, abundance %d" % (what, k, min_abundance))
                _same(got, host[min_abundance], "%s, k %d: the host form's" % (what, k))
                _same_bins(hist, want_hist, "%s, k %d" % (what, k))
    finally:
        capi.device_free(d_buf)
        capi.device_free(d_moved)
        capi.device_free(d_zero)


def test_degenerate_calls(capi):
    k = 31
    zero = np.zeros(256, dtype=np.uint64)
    # every read shorter than k; no reads at all: nothing, and a histogram of zeros, whatever the caller's arrays held
    for reads in ((b"ACGT" * 7 + b"AC", b"", b"ACGT", b"N" * 30), ()):
        rc, n_solid, _, hist = _host_raw(capi, reads, k, 1, out_cap=4, fill=5)
        assert (rc, n_solid) == (LEON_OK, 0), len(reads)
        _same_bins(hist, zero, "host form, %d reads" % len(reads))
        bases, off = S.arrays(reads)
        d_bases, d_off = capi.device_upload_bytes(bases), capi.device_upload_bytes(off.tobytes())
        try:
            for min_abundance in (1, 0):
                rc, got, hist = _device_raw(capi, d_bases, d_off, len(reads), k, min_abundance, fill=5)
                assert rc == LEON_OK and len(got) == 0
                _same_bins(hist, zero, "device form, %d reads" % len(reads))
        finally:
            capi.device_free(d_bases)
            capi.device_free(d_off)
    # a result array one k-mer short: refused, with the count the caller needs
    reads = S.exact_abundances(21)
    want = S.ref_solid(reads, 21, 2)
    rc, n_solid, out, _ = _host_raw(capi, reads, 21, 2, out_cap=len(want))
    assert (rc, n_solid) == (LEON_OK, len(want))
    _same(S.sorted_words(out[:n_solid], 21), want, "a result array that just fits")
    rc, n_solid, out, _ = _host_raw(capi, reads, 21, 2, out_cap=len(want) - 1)
    assert (rc, n_solid) == (LEON_E_OVERFLOW, len(want))
    # k outside 3 .. 63
    for bad_k in (2, 64):
        rc, n_solid, _, _ = _host_raw(capi, S.tiny_k(3)[:5], bad_k, 1, out_cap=600)
        assert rc == LEON_E_INVALID, bad_k
        assert "3 <= k <= 63" in (capi.load_library().leon_last_error(None) or b"").decode()
