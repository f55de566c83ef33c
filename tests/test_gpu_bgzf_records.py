"""-m gpu: leon_text_bgzf_records_device (k_bgzf_check_recs, k_bgzf_cuts, k_bgzf_index in front of and behind k_deflate_chunks, the CRC
kernels, k_bgzf_sizes and k_bgzf_members) through capi.text_bgzf_records_device, judged by tests/bgzf_records.py -- the rule restated in
Python, zlib and gzip over every member -- never by the code under test.  The text lies in device memory between two canaries at an odd
address, the member tables in host memory between two canaries; all of them come back unchanged."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_check as B
import bgzf_records as R

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5
PAD = 8                                                           # canary entries either side of a member table
MARK = 0xC0FFEE0DDEADBEEF
W = R.W


def run(text, rec_off, n_head=0, last=1, cap="bound", sink=None, fixed=False):
    """the call on `text` (n_head bytes of head, then the body whose records start at rec_off) uploaded between two canaries:
    (output, n_taken, n_members, [(out offset, text offset)]).  cap: entries of the member tables ('bound': the header's), None: no tables.
    fixed: d_rec_off = NULL."""
    from leon_amd import capi
    lib = capi.load_library()
    data = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(data)
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    edge = np.full(CANARY + SHIFT, FILL, dtype=np.uint8)
    base = capi.device_alloc(CANARY + SHIFT + n + CANARY)
    d_off = 0 if fixed else capi.device_alloc(8 * len(off) + CANARY)
    tables = None
    try:
        for at, a in ((0, edge), (CANARY + SHIFT, data), (CANARY + SHIFT + n, edge[:CANARY])):
            if len(a):
                a = np.ascontiguousarray(a)
                assert lib.leon_device_upload(0, C.c_void_p(base + at), C.c_void_p(a.ctypes.data), len(a)) == 0
        if d_off:
            both = np.concatenate([off.view(np.uint8), edge[:CANARY]])
            assert lib.leon_device_upload(0, C.c_void_p(d_off), C.c_void_p(both.ctypes.data), len(both)) == 0
        kw = dict(tables=False)
        if cap is not None:
            cap = capi.bgzf_members_bound(n) if cap == "bound" else cap
            tables = np.full((2, cap + 2 * PAD), MARK, dtype=np.uint64)
            kw = dict(member_out=tables[0, PAD:PAD + cap], member_text=tables[1, PAD:PAD + cap], members_cap=cap)
        try:
            out, taken, members, m_out, m_text = capi.text_bgzf_records_device(base + CANARY + SHIFT, n_head, n - n_head, d_off, 0 if fixed else len(off) - 1,
                                                                               last=last, sink=sink, **kw)
        finally:
            back = np.frombuffer(capi.device_download(base, CANARY + SHIFT + n + CANARY), dtype=np.uint8)
            assert np.array_equal(back[:CANARY + SHIFT], edge), "bytes in front of d_text were written"
            assert np.array_equal(back[CANARY + SHIFT + n:], edge[:CANARY]), "bytes behind d_text were written"
            assert np.array_equal(back[CANARY + SHIFT:CANARY + SHIFT + n], data), "the text was written"
            if d_off:
                back = np.frombuffer(capi.device_download(d_off, 8 * len(off) + CANARY), dtype=np.uint8)
                assert np.array_equal(back[:8 * len(off)], off.view(np.uint8)) and np.array_equal(back[8 * len(off):], edge[:CANARY]), "the offsets were written"
            if tables is not None:
                assert (tables[:, :PAD] == MARK).all() and (tables[:, PAD + cap:] == MARK).all(), "entries outside the member tables were written"
        if tables is not None:
            assert (tables[:, PAD + members:PAD + cap] == MARK).all(), "entries behind the last member were written"
        return out, taken, members, None if m_out is None else list(zip(m_out.tolist(), m_text.tolist()))
    finally:
        capi.device_free(base)
        if d_off:
            capi.device_free(d_off)


def text_of(lengths, seed=3):
    """records of the given lengths: four letters, each record ending with a newline"""
    off = R.offsets(lengths)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, off[-1], dtype=np.uint8)]
    if off[-1]:
        text[np.asarray(off[1:], dtype=np.int64) - 1] = 10
    return text.tobytes(), off


def whole(text, off, **kw):
    """one call over the whole text with `last`, checked against the rule: (output, member table as check_records returns it)"""
    out, taken, members, table = run(text, off, **kw)
    assert taken == len(text)
    want = R.check_records(out, text, off)
    assert members == len(want) and table == [(at, a) for at, a, _ in want]
    return out, want


def fastq_offsets(text):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert len(nl) % 4 == 0
    return [0] + (nl[3::4] + 1).tolist()


@pytest.fixture(scope="module")
def fastq():
    from test_gpu_bgzf import fastq_text
    text = fastq_text(2500)
    return text, fastq_offsets(text)


@pytest.mark.parametrize("last", [1, 0])
def test_no_body(last):
    out, taken, members, table = run(b"", [0], last=last)
    assert (out, taken, members, table) == (B.EOF if last else b"", 0, 0, [])


@pytest.mark.parametrize("name", [n for n in sorted(R.SHAPES) if n != "no_text"])
def test_shapes(name):
    text, off = text_of(R.SHAPES[name])
    out, want = whole(text, off)
    assert len(want) <= R.bound(len(text))
    # without `last` the members are those cut while more than W bytes are left, and no marker follows them
    cut, taken_want = R.cuts_call(off, 0, 0)
    out0, taken, members, table = run(text, off, last=0)
    assert taken == taken_want and members == len(cut) and len(text) - taken <= W
    assert out0 == out[:len(out0)] and table == [(at, a) for at, a, _ in want[:members]]
    R.check_records(out0, text, off, eof=False, want=cut)


def test_oversized_record_last_in_a_non_last_call():
    text, off = text_of([300, 20, 100000])
    out0, taken, members, _ = run(text, off, last=0)
    assert taken == len(text) and members == 5                    # it is taken whole, its remainder too
    R.check_records(out0, text, off, eof=False)


def test_fastq_text_and_its_size(fastq):
    """DESIGN.md 4.8's bound, the one tests/test_gpu_bgzf.py holds the fixed cuts to, per member: the payload and its 03 00 against zlib's
    Z_RLE over the same slice, 3 % and the 7 bytes zlib's one stream does not have"""
    text, off = fastq
    out, want = whole(text, off)
    assert len(want) >= 10
    sizes = [size for _, size in B.walk(out)[:-1]]
    for i, ((at, a, m), size) in enumerate(zip(want, sizes)):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        ref = len(c.compress(text[a:a + m]) + c.flush())
        got = size - B.FRAME + 2
        print("member %d: %d bytes of text, payload + 2 = %d, Z_RLE %d, ratio %.4f" % (i, m, got, ref, got / ref))
        assert got <= 1.03 * ref + 7, (i, got, ref)


def by_calls(text, off, bounds):
    """the records through one call per part, each call's remainder carried as the next head: (output, table)"""
    out, table, done, head = [], [], 0, 0
    bounds = [0] + list(bounds) + [len(off) - 1]
    for i in range(len(bounds) - 1):
        a, b = bounds[i], bounds[i + 1]
        assert head <= W and done + head == off[a]
        last = 1 if i == len(bounds) - 2 else 0
        rel = [x - off[a] for x in off[a:b + 1]]
        got, taken, members, tab = run(text[done:off[b]], rel, n_head=head, last=last)
        want, taken_want = R.cuts_call(rel, head, last)
        assert taken == taken_want and members == len(want) and [t for _, t in tab] == [p for p, _ in want]
        at = sum(len(o) for o in out)
        table += [(at + o, done + t) for o, t in tab]
        out.append(got)
        done, head = done + taken, head + off[b] - off[a] - taken
    assert head == 0 and done == off[-1]
    return b"".join(out), table


def test_split_into_calls(fastq):
    text, off = fastq
    out, want = whole(text, off)
    n = len(off) - 1
    for bounds in ([1], [n - 1], [700, 701, 701, 1900], [n // 2], [n]):
        assert by_calls(text, off, bounds) == (out, [(at, a) for at, a, _ in want]), bounds
    # a head of exactly W: nothing of the first call's 128 records of 256 bytes is taken
    text, off = text_of(R.SHAPES["one_member_of_exactly_W"])
    out, want = whole(text, off)
    got, taken, members, _ = run(text, off, last=0)
    assert (got, taken, members) == (b"", 0, 0)
    assert by_calls(text, off, [128]) == (out, [(0, 0)])
    text, off = text_of([256] * 128 + [100, 40000, 300, 16384, 16384, 5, 70000, 1])
    out, want = whole(text, off)
    for bounds in ([128], [130], [129, 135], [134]):
        assert by_calls(text, off, bounds) == (out, [(at, a) for at, a, _ in want]), bounds


@pytest.mark.parametrize("slice_bytes", ["98304", "32768", "100000", "1"])
def test_slices(fastq, monkeypatch, slice_bytes):
    """a slice ends at a cut -- inside the 100 000-byte record too -- and the next begins there: the bytes and tables of the single slice"""
    ftext, foff = fastq
    k = 1200
    lengths = [b - a for a, b in zip(foff[:k], foff[1:k + 1])]
    lengths = lengths[:600] + [100000] + lengths[600:] + [65536]
    text, off = text_of(lengths)
    text = bytearray(text)
    at = 0
    for i, n in enumerate(lengths):                               # the FASTQ records' own bytes where they are records of the suite's text
        j = i if i < 600 else i - 1
        if n not in (100000, 65536):
            text[at:at + n] = ftext[foff[j]:foff[j + 1]]
        at += n
    text = bytes(text)
    out, want = whole(text, off)
    monkeypatch.setenv("LEON_BGZF_SLICE", slice_bytes)
    assert whole(text, off) == (out, want)
    assert by_calls(text, off, [300, 601, 1000]) == (out, [(at, a) for at, a, _ in want])


def test_past_the_caps():
    """about 4 100 members of 350-byte records: several tiles of k_bgzf_cuts, k_bgzf_members' grid cap of 4 096, the output in pieces from
    several threads"""
    n_rec = 383000
    rng = np.random.default_rng(17)
    lengths = rng.integers(340, 361, n_rec)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(off[-1]), dtype=np.uint8)]
    text[off[1:].astype(np.int64) - 1] = 10
    seen = []
    out, taken, members, table = run(text, off, sink=lambda offset, size: seen.append((offset, size)) or 0)
    assert taken == len(text) and members > 4096
    assert max(size for _, size in seen) <= 16 << 20 and sum(size for _, size in seen) == len(out)
    want = R.check_records(out, text.tobytes(), off.tolist())
    assert members == len(want) and table == [(at, a) for at, a, _ in want]


def test_without_records_the_fixed_cuts(fastq):
    from leon_amd import capi
    from test_gpu_bgzf import bgzf
    text, _ = fastq
    text = text[:5 * W + 777]
    out, taken, members, table = run(text, [0], fixed=True, cap=6)
    assert (out, taken, members) == bgzf(text)
    B.check(out, text)
    assert table == [(at, i * W) for i, (at, _) in enumerate(B.walk(out)[:-1])]
    out0, taken, members, table = run(text, [0], fixed=True, last=0, cap=5)
    assert (out0, taken, members) == (out[:len(out0)], 5 * W, 5) and len(table) == 5
    with pytest.raises(capi.LeonDnaError) as e:                   # a table one entry too small
        run(text, [0], fixed=True, cap=5, sink=lambda offset, size: pytest.fail("the sink was called"))
    assert e.value.code == -5 and e.value.n_members == 6


@pytest.mark.parametrize("bad, words", [([0, 700, 700, 900], "not strictly ascending"), ([0, 700, 650, 900], "not strictly ascending"),
                                        ([0, 700, 800, 899], "do not end at n_body"), ([0, 700, 800, 901], "do not end at n_body"),
                                        ([1, 700, 800, 900], "do not start at 0")])
def test_offsets_refused_on_the_device(bad, words):
    from leon_amd import capi
    text, _ = text_of([700, 100, 100])
    with pytest.raises(capi.LeonDnaError) as e:
        run(text, bad, sink=lambda offset, size: pytest.fail("the sink was called"))
    assert e.value.code == -1 and words in str(e.value), str(e.value)


def test_a_member_table_one_entry_too_small():
    from leon_amd import capi
    text, off = text_of(R.SHAPES["100000_between_small_records"])
    need = len(R.cuts(off))
    with pytest.raises(capi.LeonDnaError) as e:
        run(text, off, cap=need - 1, sink=lambda offset, size: pytest.fail("the sink was called"))
    assert e.value.code == -5 and e.value.n_members == need, (str(e.value), e.value.n_members)
    out, _, members, table = run(text, off, cap=need)            # exactly enough
    assert members == need and len(table) == need
    assert run(text, off, cap=None)[:3] == (out, len(text), need)          # and no table at all


def test_sink_contract(fastq):
    from leon_amd import capi
    text, off = fastq
    seen = []
    out, _, _, _ = run(text, off, sink=lambda offset, size: seen.append((offset, size)) or 0)
    seen.sort()
    assert seen[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(seen, seen[1:])) and sum(seen[-1]) == len(out)
    with pytest.raises(capi.LeonDnaError) as e:
        run(text, off, sink=lambda offset, size: 1)
    assert e.value.code == -6 and "sink" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:                   # the marker's piece is refused like any other
        run(b"", [0], sink=lambda offset, size: 1)
    assert e.value.code == -6
