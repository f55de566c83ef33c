"""-m gpu: the reads' FASTA / FASTQ text formatted on the device (leon_records_format_device: k_fmt_sizes, the scan, k_fmt_records)
against a formatter written here from the record's definition; leon_dna_decode_blocks_device against leon_dna_decode_blocks;
leon_device_download_pieces against what was uploaded.

A record:   lead  header | decimal(first_read_index + r)  '\\n'
            the sequence: len bytes + '\\n' (wrap == 0 or len <= wrap), else ceil(len / wrap) lines of at most wrap bytes, each + '\\n'
            FASTQ only:  '+'  [the header again when plus_kind == 1]  '\\n'  len quality bytes  '\\n'
"""
import ctypes
import random
import threading

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5                                                          # d_text = (a 16-byte-aligned address) + 5


def py_format(reads, heads, quals, fastq, plus_kind, wrap, first):
    """(text, rec_off) from the definition above; heads None: the read index stands in"""
    out, rec_off, at = [], [0], 0
    for r, seq in enumerate(reads):
        h = heads[r] if heads is not None else b"%d" % (first + r)
        rec = [b"@" if fastq else b">", h, b"\n"]
        if wrap == 0 or len(seq) <= wrap:
            rec += [seq, b"\n"]
        else:
            for o in range(0, len(seq), wrap):
                rec += [seq[o:o + wrap], b"\n"]
        if fastq:
            rec += [b"+", h if plus_kind == 1 else b"", b"\n", quals[r], b"\n"]
        rec = b"".join(rec)
        out.append(rec)
        at += len(rec)
        rec_off.append(at)
    return b"".join(out), rec_off


class Dev:
    """device buffers of one case, freed together"""

    def __init__(self):
        from leon_amd import capi
        self.capi, self.ptrs = capi, []

    def up(self, data):
        p = self.capi.device_upload_bytes(bytes(data))
        self.ptrs.append(p)
        return p

    def alloc(self, n):
        p = self.capi.device_alloc(n)
        self.ptrs.append(p)
        return p

    def close(self):
        for p in self.ptrs:
            self.capi.device_free(p)
        self.ptrs = []


def _np(rng):
    return np.random.default_rng(rng.randrange(1 << 30))


def _split(blob, lengths):
    out, at = [], 0
    for L in lengths:
        out.append(blob[at:at + L])
        at += L
    return out


def _quals_for(reads, rng):
    lengths = [len(s) for s in reads]
    return _split((33 + _np(rng).integers(0, 41, size=sum(lengths))).astype(np.uint8).tobytes(), lengths)


def device_format(reads, heads, quals, fastq, plus_kind, wrap, first, cap_delta=0, want_rec_off=True, n_bases=None, hdr_off=None, hdr_bytes=None,
                  struct_size=None, drop_quals=False, drop_heads_ptr=False):
    """run leon_records_format_device between two canaries at a misaligned address; returns (text, rec_off, size) after checking the canaries.
    cap_delta / n_bases / hdr_off / hdr_bytes / struct_size / drop_*: what the failure cases tell the call instead of the truth"""
    from leon_amd import capi
    want, _ = py_format(reads, heads, quals, fastq, plus_kind, wrap, first)
    n = len(reads)
    D = Dev()
    try:
        lens = np.array([len(s) for s in reads] + [0], dtype=np.uint32)
        bases = b"".join(reads)
        d_bases, d_len = D.up(bases + b"\0"), D.up(lens.tobytes())
        d_quals = D.up(b"".join(quals) + b"\0") if fastq and not drop_quals else None
        d_hdr = d_hoff = None
        hb = 0
        if heads is not None:
            base = 1000                                            # offsets counted from a set's first byte: d_hdr_off[0] is subtracted
            off = np.zeros(n + 1, dtype=np.uint64)
            off[0] = base
            if n:
                off[1:] = base + np.cumsum([len(h) for h in heads])
            hb = int(off[n] - off[0])
            if hdr_off is not None:
                off = np.asarray(hdr_off, dtype=np.uint64)
            d_hdr, d_hoff = (None if drop_heads_ptr else D.up(b"".join(heads) + b"\0")), D.up(off.tobytes())
        region = bytes([0xA5]) * (CANARY + SHIFT + len(want) + CANARY + 32)
        d_region = D.up(region)
        assert d_region % 16 == 0
        d_text = d_region + CANARY + SHIFT
        d_rec = D.up(bytes([0x5A]) * (8 * (n + 1) + 8)) if want_rec_off else None
        err = None
        try:
            size = capi.records_format_device(d_bases, d_len, n, len(bases) if n_bases is None else n_bases, d_text, len(want) + cap_delta,
                                              lead=b"@" if fastq else b">", fastq=fastq, plus_kind=plus_kind, wrap=wrap, first_read_index=first,
                                              d_hdr_text=d_hdr, d_hdr_off=d_hoff, hdr_bytes=hb if hdr_bytes is None else hdr_bytes, d_quals=d_quals,
                                              d_rec_off=d_rec, struct_size=struct_size)
        except capi.LeonDnaError as e:
            err, size = e, e.text_size
        got = capi.device_download(d_region, len(region))
        front, back = got[:CANARY + SHIFT], got[CANARY + SHIFT + len(want):]
        assert front == region[:len(front)] and back == region[:len(back)], "bytes outside the text buffer were written"
        text = got[CANARY + SHIFT:CANARY + SHIFT + len(want)]
        rec = np.frombuffer(capi.device_download(d_rec, 8 * (n + 1) + 8), dtype=np.uint64) if want_rec_off else None
        if err is not None:
            assert text == region[:len(text)], "a refused call wrote to the text buffer"
            if rec is not None:
                assert bytes(rec.tobytes()) == bytes([0x5A]) * (8 * (n + 1) + 8)
            raise err
        return text, rec, size
    finally:
        D.close()


def check(reads, heads, quals, fastq, plus_kind, wrap, first, what=""):
    want, want_off = py_format(reads, heads, quals, fastq, plus_kind, wrap, first)
    text, rec, size = device_format(reads, heads, quals, fastq, plus_kind, wrap, first)
    assert size == len(want), (what, size, len(want))
    if text != want:
        i = next(j for j in range(len(want)) if text[j] != want[j])
        raise AssertionError("%s: the text differs at byte %d of %d: %r != %r" % (what, i, len(want), text[max(0, i - 20):i + 20], want[max(0, i - 20):i + 20]))
    n = len(reads)
    assert list(rec[:n + 1]) == want_off if n else True, what
    assert rec[n + 1] == 0x5A5A5A5A5A5A5A5A, "rec_off was written past its n_reads + 1 entries"


def _reads(rng, lengths):
    return _split(np.frombuffer(b"ACGTN", dtype=np.uint8)[_np(rng).integers(0, 5, size=sum(lengths))].tobytes(), lengths)


def _heads(rng, n, special=True):
    hs = [b"SRR%d.%d %d length=%d" % (rng.randrange(10 ** 6), i + 1, i + 1, rng.randrange(300)) for i in range(n)]
    if special and n > 4:
        hs[1] = b""
        hs[n // 2] = bytes(33 + (i % 90) for i in range(4096))
        hs[n - 1] = b""
    return hs


WRAPS = (0, 1, 7, 60, 70)


def _lengths_for(wrap):
    base = [0, 1, 15, 16, 17, 4097, 150, 0, 33]
    if wrap:
        base += [max(wrap - 1, 0), wrap, wrap + 1, 2 * wrap, 2 * wrap + 1, 3 * wrap]
    return base + [300000, 5, 0]


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("fastq", [True, False])
def test_format_product(fastq, wrap):
    """FASTQ / FASTA x headers / read index (0, 9, 99 999 998: the digit count changes inside the call) x plus_kind x wrap, over lengths
    around the wrap width, around 16, 4 097 and ONE read of 300 000 bases; empty headers and one of 4 096 bytes"""
    rng = random.Random(1000 + wrap + (7 if fastq else 0))
    reads = _reads(rng, _lengths_for(wrap))
    quals = _quals_for(reads, rng)
    heads = _heads(rng, len(reads))
    for plus_kind in ((0, 1) if fastq else (0,)):
        check(reads, heads, quals, fastq, plus_kind, wrap, 0, "headers, plus %d" % plus_kind)
    for first in (0, 9, 99999998):
        check(reads, None, quals, fastq, 0, wrap, first, "read index from %d" % first)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 5000])
def test_format_read_counts(n):
    rng = random.Random(n)
    reads = _reads(rng, [rng.choice((0, 1, 36, 100, 101, 150)) for _ in range(n)])
    quals = _quals_for(reads, rng)
    heads = _heads(rng, n, special=n > 100)
    check(reads, heads, quals, True, 1, 0, 0, "fastq, header again")
    check(reads, heads, quals, False, 0, 60, 0, "fasta wrapped")
    check(reads, None, quals, True, 0, 0, 99999998 - n // 2, "fastq, read index")
    check(reads, None, quals, False, 0, 7, 9, "fasta, read index, wrapped at 7")


def test_format_three_byte_records():
    """200 000 records of the minimum size (empty header, empty read, FASTA): a tile of the output holds more records than one staging
    pass of the kernel; then the same with a few long records among them"""
    n = 200000
    reads, heads = [b""] * n, [b""] * n
    check(reads, heads, reads, False, 0, 0, 0, "3-byte records")
    check(reads, heads, reads, False, 0, 60, 0, "3-byte records, wrap 60")
    rng = random.Random(5)
    reads = list(reads)
    for i in (0, 1365, 1366, 70000, n - 1):
        reads[i] = _reads(rng, [4097])[0]
    heads = list(heads)
    heads[70001] = b"h" * 300
    check(reads, heads, reads, False, 0, 0, 0, "3-byte records with long ones among them")
    check([b"A"] * 1000 + [b""] * 50000, None, [b"I"] * 1000 + [b""] * 50000, True, 0, 0, 7, "minimum FASTQ records, read index")


def test_format_random_draws():
    rng = random.Random(20240)
    for draw in range(200):
        n = rng.choice((1, 2, 3, 17, 64, 100, 300))
        kind = rng.randrange(4)
        lens = [rng.choice((0, 1, 15, 16, 17, rng.randrange(0, 200), rng.randrange(0, 200), 4097 if kind == 0 else 50)) for _ in range(n)]
        if draw % 50 == 0:
            lens[rng.randrange(n)] = 300000
        reads = _reads(rng, lens)
        fastq = rng.random() < 0.5
        with_heads = rng.random() < 0.6
        heads = None
        if with_heads:
            hl = [rng.choice((0, 1, 15, 16, 17, 40, 60, 4096 if rng.random() < 0.01 else 30)) for _ in range(n)]
            heads = _split((33 + _np(rng).integers(0, 94, size=sum(hl))).astype(np.uint8).tobytes(), hl)
        plus_kind = 1 if (fastq and with_heads and rng.random() < 0.5) else 0
        wrap = rng.choice(WRAPS + (2, 16, 100000))
        first = rng.choice((0, 9, 99, 99999998, 10 ** 12 - 3, rng.randrange(10 ** 9)))
        quals = _quals_for(reads, rng)
        check(reads, heads, quals, fastq, plus_kind, wrap, first, "draw %d" % draw)


def test_format_refusals():
    from leon_amd import capi
    rng = random.Random(3)
    reads = _reads(rng, [10, 0, 150, 17, 99])
    quals = _quals_for(reads, rng)
    heads = _heads(rng, len(reads), special=False)
    want, _ = py_format(reads, heads, quals, True, 1, 0, 0)
    # a byte short: the size needed, nothing written (device_format checks buffer, rec_off and canaries before it re-raises)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 1, 0, 0, cap_delta=-1)
    assert e.value.code == -5 and e.value.text_size == len(want)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, None, quals, False, 0, 7, 99999998, cap_delta=-1)
    assert e.value.code == -5 and e.value.text_size == len(py_format(reads, None, quals, False, 0, 7, 99999998)[0])
    # the lengths do not add up to the bases given (found on the device, before anything is indexed with them)
    for delta in (-1, 1, 1000):
        with pytest.raises(capi.LeonDnaError) as e:
            device_format(reads, heads, quals, True, 0, 0, 0, n_bases=sum(map(len, reads)) + delta)
        assert e.value.code == -1 and "add up" in str(e.value)
    # a header offset table that runs backwards, and one that ends elsewhere than the header bytes given
    n = len(reads)
    good = 1000 + np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)
    back = good.copy()
    back[2], back[3] = good[3], good[2]
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 1, 0, 0, hdr_off=back)
    assert e.value.code == -1 and "backwards" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 1, 0, 0, hdr_bytes=int(good[n] - good[0]) + 1)
    assert e.value.code == -1 and "do not end" in str(e.value)
    far = good.copy()
    far[n] += 1 << 30
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, False, 0, 0, 0, hdr_off=far)
    assert e.value.code == -1
    # arguments that contradict one another
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 0, 0, 0, drop_quals=True)
    assert e.value.code == -1 and "d_quals" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 1, 0, 0, drop_heads_ptr=True)
    assert e.value.code == -1 and "d_hdr_text" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, 0, 0, 0, struct_size=ctypes.sizeof(capi.RecordLayout) + 8)
    assert e.value.code == -1 and "struct_size" in str(e.value)
    # and the library still formats after all that
    check(reads, heads, quals, True, 1, 0, 0, "after the refusals")


def test_decode_blocks_device_equals_the_host_form():
    import leon_amd
    from leon_amd import capi
    k, rpb, n = 25, 400, 1900
    bases, off = common.synthetic(n, 120, 7000, seed=31, n_rate=0.004, err=0.02, ragged=True)
    bl, solid, tai = common.make_bloom(bases, off, k)
    ctx = leon_amd.DnaEncodeContext(kmer_size=k, reads_per_block=rpb, bloom_tai=tai)
    ctx.bloom_insert(solid)
    blocks = ctx.encode_batch(bases, off)
    dict_payload, n_anchors = ctx.finish()
    assert len(blocks) == 5
    anchors = capi.anchor_dict_decode(dict_payload, n_anchors, k)
    nbases = [int(off[min(n, (b + 1) * rpb)] - off[b * rpb]) for b in range(len(blocks))]
    want_bases, want_lens = ctx.decode_blocks_raw(anchors, blocks, nbases)
    assert want_bases.tobytes() == bytes(c if c in b"ACGT" else ord("N") for c in bases)
    total = int(sum(nbases))
    D = Dev()
    try:
        d_bases, d_len = D.up(bytes([0x11]) * (total + 64)), D.up(bytes([0x22]) * (4 * n + 64))
        lens = ctx.decode_blocks_device(anchors, blocks, nbases, d_bases, d_len)
        assert np.array_equal(lens, want_lens)
        assert capi.device_download(d_bases, total + 64) == want_bases.tobytes() + bytes([0x11]) * 64        # nothing past the bases
        assert capi.device_download(d_len, 4 * n + 64) == want_lens.tobytes() + bytes([0x22]) * 64
        assert ctx.decode_blocks_device(anchors, blocks, nbases, d_bases, d_len, host_lens=False) is None
        # the decoded reads go straight into the formatter
        reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
        norm = [bytes(c if c in b"ACGT" else ord("N") for c in r) for r in reads]
        want, _ = py_format(norm, None, norm, False, 0, 60, 5)
        d_text = D.alloc(len(want) + 64)
        assert capi.records_format_device(d_bases, d_len, n, total, d_text, len(want), lead=b">", fastq=False, wrap=60, first_read_index=5) == len(want)
        assert capi.device_download(d_text, len(want)) == want
        # what does not decode is refused by both forms with the same status and message, and the caller's buffers stay as they were
        for fill in (0x33, 0x44):
            capi.device_copy(d_bases, D.up(bytes([fill]) * total), total)
            outcome = []
            for form in ("host", "device"):
                try:
                    if form == "host":
                        ctx.decode_blocks_raw(anchors, blocks, [x - 5 for x in nbases] if fill == 0x33 else nbases[:-1] + [nbases[-1] + 3])
                    else:
                        ctx.decode_blocks_device(anchors, blocks, [x - 5 for x in nbases] if fill == 0x33 else nbases[:-1] + [nbases[-1] + 3], d_bases, d_len)
                    outcome.append(None)
                except capi.LeonDnaError as e:
                    outcome.append((e.code, str(e)))
            assert outcome[0] is not None and outcome[0][0] == -1 and "does not decode" in outcome[0][1]
            assert outcome[1] == outcome[0]
            assert capi.device_download(d_bases, total) == bytes([fill]) * total
        # a corrupted payload: reported the same way by both forms (or decoded to the same wrong bases), never a crash
        bad = list(blocks)
        bad[1] = (bad[1][0], bytes(255 - x for x in bad[1][1]), bad[1][2])
        outcome = []
        for form in ("host", "device"):
            try:
                if form == "host":
                    outcome.append(ctx.decode_blocks_raw(anchors, bad, nbases)[0].tobytes())
                else:
                    ctx.decode_blocks_device(anchors, bad, nbases, d_bases, d_len)
                    outcome.append(capi.device_download(d_bases, total))
            except capi.LeonDnaError as e:
                outcome.append((e.code, str(e)))
        assert outcome[0] == outcome[1]
        with pytest.raises(capi.LeonDnaError) as e:
            ctx.decode_blocks_device(anchors, blocks, nbases, 0, d_len)
        assert e.value.code == -1
    finally:
        D.close()
        ctx.close()


def test_download_pieces():
    from leon_amd import capi
    n = 100 * 1000 * 1000 + 12345                                 # more than four 16 MiB pieces
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, size=n, dtype=np.uint8)
    D = Dev()
    try:
        d = D.alloc(n + 64)
        lib = capi.load_library()
        assert lib.leon_device_upload(0, ctypes.c_void_p(d), ctypes.c_void_p(data.ctypes.data), n) == 0
        out = np.zeros(n, dtype=np.uint8)
        seen = np.zeros(n, dtype=np.uint8)                        # a coverage count per byte
        lock = threading.Lock()
        pieces, threads = [], set()

        def sink(offset, address, size):
            piece = np.ctypeslib.as_array(ctypes.cast(address, ctypes.POINTER(ctypes.c_uint8)), shape=(size,))
            with lock:
                out[offset:offset + size] = piece
                seen[offset:offset + size] += 1
                pieces.append((offset, size))
                threads.add(threading.get_ident())
            return 0
        capi.device_download_pieces(d, n, sink)
        assert seen.min() == 1 and seen.max() == 1, "a byte was delivered %d..%d times" % (seen.min(), seen.max())
        assert np.array_equal(out, data)
        assert len(pieces) >= 6 and max(s for _, s in pieces) <= 16 << 20 and sum(s for _, s in pieces) == n
        print("%d pieces from %d thread(s)" % (len(pieces), len(threads)))
        # a small copy
        got = []
        capi.device_download_pieces(d + 3, 1000, lambda o, a, s: got.append((o, ctypes.string_at(a, s))) and 0)
        assert b"".join(p for _, p in sorted(got)) == data[3:1003].tobytes() and sum(len(p) for _, p in got) == 1000
        capi.device_download_pieces(d, 0, lambda o, a, s: 1)      # nothing to deliver: the sink is not called
        # a sink that refuses: LEON_E_SINK, for a small copy and for a large one
        for size in (1000, n):
            with pytest.raises(capi.LeonDnaError) as e:
                capi.device_download_pieces(d, size, lambda o, a, s: 1)
            assert e.value.code == -6
        # ... and the library goes on working
        got = []
        capi.device_download_pieces(d, 5000, lambda o, a, s: got.append(ctypes.string_at(a, s)) and 0)
        assert b"".join(got) == data[:5000].tobytes()
    finally:
        D.close()
