"""-m gpu: the lossy quality smoothing on the device (hdr_kernels.hip k_read_minimizer, k_mpos_from_anchors, k_solid_flags, k_qual_rewrite,
k_qual_smooth) against the oracle's lo_qual_smooth, byte for byte, on the cases of qual_shapes.py -- test_qual_smooth_cpu.py certifies
those from the oracle alone.  Every case goes through the three routes the library has: the reads ordered by their minimizers (from 256
reads on), every read for itself in file order (LEON_QUAL_ORDER=0, read at every call), and ordered by the anchors an encode of the same
reads left.  Then the device entry as `leon -c` calls it, stale anchors, and what the entries refuse."""
import ctypes as C

import numpy as np
import pytest

import qual_shapes as S

pytestmark = pytest.mark.gpu

ROUTES = ["minimizers", "file-order", "anchors"]
CANARY = 64
SHIFT = 5
FILL = 0xA5


def context(case):
    import leon_amd
    ctx = leon_amd.DnaEncodeContext(kmer_size=case.k, reads_per_block=500, bloom_tai=case.tai, bloom_n_hash=case.geometry[0],
                                    bloom_block_nbits=case.geometry[1])
    ctx.bloom_upload(case.bloom().bits)
    return ctx


def smooth(ctx, case):
    return np.frombuffer(ctx.qual_smooth_batch(case.bases, case.off, case.quals), dtype=np.uint8)


def same(case, got, want, what):
    assert len(got) == len(want), (case.name, what)
    if not np.array_equal(got, want):
        pytest.fail("%s, %s: %s" % (case.name, what, S.first_difference(case, got, want)))


def run(case, route, monkeypatch):
    ctx = context(case)
    try:
        if route == "file-order":
            monkeypatch.setenv("LEON_QUAL_ORDER", "0")
        if route == "anchors":
            ctx.encode_batch(case.bases, case.off)
            ctx.finish()
        same(case, smooth(ctx, case), S.expected(case), route)
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [n for n in S.NAMES if n != S.HUGE])
def test_equals_the_oracle(name, route, monkeypatch):
    """designed flags at every bloom geometry and k = 21, 31, 32, 33, 63 (solid pairs either side of the flag words' and the ballots' joins),
    every read length from k to k + 65, N, dense random cases, 1 / 255 / 256 / 257 reads, 16 389 reads (a wave's second trip), one read of
    70 000 bases"""
    run(S.case(name), route, monkeypatch)


def test_a_read_index_past_2097152():
    """2^21 + 300 reads: the second trip of k_iota's threads, the 129th of the waves"""
    case = S.case(S.HUGE)
    assert case.n > S.THREAD_GRID and min(i for i in case.check if i >= 150) >= S.THREAD_GRID
    ctx = context(case)
    try:
        same(case, smooth(ctx, case), S.expected(case), "minimizers")
    finally:
        ctx.close()


def test_stale_anchors():
    """encode_batch(A), then the smoothing of B -- as many reads, so the host entry finds the same buffers and the same count and takes A's
    anchors for B's reads: positions behind a read's last k-mer, reads shorter than k.  Anchors decide who shares probes, never a byte."""
    a, b = S.stale_pair()
    ctx = context(a)
    try:
        ctx.encode_batch(a.bases, a.off)
        ctx.finish()
        same(b, smooth(ctx, b), S.expected(b), "A's anchors")
        same(a, smooth(ctx, a), S.expected(a), "its own anchors, after B")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["count-255", "genome-k31"])
def test_host_entry_with_a_first_offset_above_zero(name):
    case = S.case(name)
    front, behind = np.arange(7, dtype=np.uint8) + 200, np.arange(9, dtype=np.uint8) + 100
    bases = np.concatenate((np.frombuffer(b"ACGTACG", dtype=np.uint8), case.bases, np.frombuffer(b"TTTTTTTTT", dtype=np.uint8)))
    quals = np.concatenate((front, case.quals, behind))
    ctx = context(case)
    try:
        got = np.frombuffer(ctx.qual_smooth_batch(bases, case.off + np.uint64(7), quals), dtype=np.uint8)
    finally:
        ctx.close()
    assert len(got) == len(quals)
    assert np.array_equal(got[:7], front) and np.array_equal(got[len(got) - 9:], behind), "bytes outside [off[0], off[n]) were written"
    same(case, got[7:len(got) - 9], S.expected(case), "off[0] = 7")


class OnDevice:
    """the case's bases, offsets and qualities in device memory, the qualities at base + CANARY + SHIFT between two canaries"""

    def __init__(self, case):
        from leon_amd import capi
        self.capi, self.case, self.nb = capi, case, len(case.quals)
        self.edge = np.full(CANARY + SHIFT, FILL, dtype=np.uint8)
        self.d_bases = capi.device_upload_bytes(case.bases)
        self.d_off = capi.device_upload_bytes(case.off.tobytes())
        self.base = capi.device_alloc(CANARY + SHIFT + self.nb + CANARY)
        self.d_quals = self.base + CANARY + SHIFT
        self.upload_quals()

    def upload_quals(self):
        lib = self.capi.load_library()
        for at, a in ((0, self.edge), (CANARY + SHIFT, self.case.quals), (CANARY + SHIFT + self.nb, self.edge[:CANARY])):
            a = np.ascontiguousarray(a)
            assert lib.leon_device_upload(0, C.c_void_p(self.base + at), C.c_void_p(a.ctypes.data), len(a)) == 0

    def call(self, ctx, r, n):
        """the CLI's call for reads [r, r + n): d_off + r, d_quals + off[r]"""
        ctx.qual_smooth_batch_device(self.d_bases, self.d_off + 8 * r, n, self.d_quals + int(self.case.off[r]))

    def quals(self):
        whole = np.frombuffer(self.capi.device_download(self.base, CANARY + SHIFT + self.nb + CANARY), dtype=np.uint8)
        assert np.array_equal(whole[:CANARY + SHIFT], self.edge), "bytes in front of d_quals were written"
        assert np.array_equal(whole[CANARY + SHIFT + self.nb:], self.edge[:CANARY]), "bytes behind d_quals were written"
        assert self.capi.device_download(self.d_bases, len(self.case.bases)) == self.case.bases.tobytes(), "d_bases was written"
        assert self.capi.device_download(self.d_off, 8 * (self.case.n + 1)) == self.case.off.tobytes(), "d_off was written"
        return whole[CANARY + SHIFT:CANARY + SHIFT + self.nb]

    def free(self):
        for p in (self.d_bases, self.d_off, self.base):
            self.capi.device_free(p)


def ranged(case, r, n):
    """the oracle's bytes for reads [r, r + n), the input's everywhere else"""
    want = case.quals.copy()
    s, e = int(case.off[r]), int(case.off[r + n])
    want[s:e] = S.expected(case)[s:e]
    return want


@pytest.mark.parametrize("r,n", [(0, None), (500, 1000), (500, 200), (1501, 255), (5000, 0)], ids=["every-read", "first-read-500-count-1000", "first-read-500-count-200", "first-read-1501-count-255", "first-read-5000-count-0"])
def test_device_entry_as_the_cli_calls_it(r, n):
    """leon_qual_smooth_batch_device on d_off + r and d_quals + off[r], r = 0 and r on and off a block boundary (500 reads a block): the
    range equals the oracle, nothing else is written; done again on its own output nothing changes; done in two halves, the same"""
    case = S.case("genome-k31")
    n = case.n if n is None else n
    assert r + n <= case.n and (r == 0 or int(case.off[r]) > 0)
    ctx, dev = context(case), OnDevice(case)
    try:
        want = ranged(case, r, n)
        dev.call(ctx, r, n)
        same(case, dev.quals(), want, "reads [%d, %d)" % (r, r + n))
        dev.call(ctx, r, n)
        same(case, dev.quals(), want, "reads [%d, %d) a second time" % (r, r + n))
        dev.upload_quals()
        half = n // 2
        dev.call(ctx, r, half)
        same(case, dev.quals(), ranged(case, r, half), "the first half of reads [%d, %d)" % (r, r + n))
        dev.call(ctx, r + half, n - half)
        same(case, dev.quals(), want, "reads [%d, %d) in two halves" % (r, r + n))
    finally:
        dev.free()
        ctx.close()


def test_refusals():
    from leon_amd import capi
    case = S.case("count-257")
    ctx, dev = context(case), OnDevice(case)
    try:
        assert ctx.qual_smooth_batch_device(0, 0, 0, 0) is None                       # nothing to do: no pointer is looked at
        assert ctx.qual_smooth_batch(b"", np.zeros(1, dtype=np.uint64), b"") == b""
        for args in ((0, dev.d_off, dev.d_quals), (dev.d_bases, 0, dev.d_quals), (dev.d_bases, dev.d_off, 0)):
            with pytest.raises(capi.LeonDnaError) as e:
                ctx.qual_smooth_batch_device(args[0], args[1], case.n, args[2])
            assert e.value.code == -1 and str(e.value).endswith(": null argument")
        backwards = case.off.copy()
        backwards[100], backwards[101] = backwards[101], backwards[100]
        d_bad = capi.device_upload_bytes(backwards.tobytes())
        try:
            with pytest.raises(capi.LeonDnaError) as e:
                ctx.qual_smooth_batch_device(dev.d_bases, d_bad, case.n, dev.d_quals)
            assert e.value.code == -1 and str(e.value).endswith(": offsets are not monotonic (or a read is longer than 2^31 bases)")
        finally:
            capi.device_free(d_bad)
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.qual_smooth_batch(case.bases, backwards, case.quals)
        assert e.value.code == -1 and str(e.value).endswith(": offsets are not monotonic (or a read is longer than 2^31 bases)")
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.qual_smooth_batch(case.bases, case.off[::-1].copy(), case.quals)
        assert e.value.code == -1 and str(e.value).endswith(": offsets are not monotonic")
        same(case, dev.quals(), case.quals, "after the refusals")                       # a refused call has written nothing
        dev.call(ctx, 0, case.n)                                                        # and the context goes on working
        same(case, dev.quals(), S.expected(case), "after the refusals")
    finally:
        dev.free()
        ctx.close()
