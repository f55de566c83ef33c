"""-m gpu: the reads as unaligned BAM records, formatted on the device (leon_records_bam_device: k_bam_sizes, the scan, k_bam_records;
DESIGN.md 4.19) against tests/bam_records.py's restatement of the format, bytes and record offsets, on the calls of tests/bam_cases.py;
d_out misaligned by 5 between two canaries; the refusals with the buffer untouched; and the records through the device's BGZF writer
behind the BAM header."""
import ctypes
import gzip

import numpy as np
import pytest

import bam_cases
import bam_records as B

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5                                                          # d_out = (a 16-byte-aligned address) + 5


class Dev:
    """device buffers of one case, freed together"""

    def __init__(self):
        from leon_amd import capi
        self.capi, self.ptrs = capi, []

    def up(self, data):
        p = self.capi.device_upload_bytes(bytes(data))
        self.ptrs.append(p)
        return p

    def close(self):
        for p in self.ptrs:
            self.capi.device_free(p)
        self.ptrs = []


def device_format(reads, heads, quals, fastq, first, room, cap=None, n_bases=None, hdr_off=None, hdr_bytes=None, struct_size=None):
    """leon_records_bam_device between two canaries at a misaligned address, with `room` bytes of buffer and `cap` (default: room) told to
    the call.  Returns (the buffer's bytes, rec_off, size) after checking the canaries; a refused call must have left buffer and rec_off
    untouched (a quality refusal excepted: its records may have been written) before its error is raised again."""
    from leon_amd import capi
    n = len(reads)
    D = Dev()
    try:
        lens = np.array([len(s) for s in reads] + [0], dtype=np.uint32)
        bases = b"".join(reads)
        d_bases, d_len = D.up(bases + b"\0"), D.up(lens.tobytes())
        d_quals = D.up(b"".join(quals) + b"\0") if quals is not None else None
        d_hdr = d_hoff = None
        hb = 0
        if heads is not None:
            off = 1000 + np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)      # counted from a set's first byte
            hb = int(off[n] - off[0])
            if hdr_off is not None:
                off = np.asarray(hdr_off, dtype=np.uint64)
            d_hdr, d_hoff = D.up(b"".join(heads) + b"\0"), D.up(off.tobytes())
        region = bytes([0xA5]) * (CANARY + SHIFT + room + CANARY + 32)
        d_region = D.up(region)
        assert d_region % 16 == 0
        d_out = d_region + CANARY + SHIFT
        d_rec = D.up(bytes([0x5A]) * (8 * (n + 1) + 8))
        err = None
        try:
            size = capi.records_bam_device(d_bases, d_len, n, len(bases) if n_bases is None else n_bases, d_out, room if cap is None else cap, fastq=fastq,
                                           first_read_index=first, d_hdr_text=d_hdr, d_hdr_off=d_hoff, hdr_bytes=hb if hdr_bytes is None else hdr_bytes,
                                           d_quals=d_quals, d_rec_off=d_rec, struct_size=struct_size)
        except capi.LeonDnaError as e:
            err, size = e, e.out_size
        got = capi.device_download(d_region, len(region))
        front, back = got[:CANARY + SHIFT], got[CANARY + SHIFT + room:]
        assert front == region[:len(front)] and back == region[:len(back)], "bytes outside the output buffer were written"
        out = got[CANARY + SHIFT:CANARY + SHIFT + room]
        rec = np.frombuffer(capi.device_download(d_rec, 8 * (n + 1) + 8), dtype=np.uint64)
        if err is not None:
            if "quality byte" not in str(err):
                assert out == region[:len(out)], "a refused call wrote to the output buffer"
                assert rec.tobytes() == bytes([0x5A]) * (8 * (n + 1) + 8), "a refused call wrote to rec_off"
            raise err
        return out, rec, size
    finally:
        D.close()


def check(case):
    what, reads, heads, quals, fastq, first = case
    want, want_off = B.bam_records(reads, heads, quals if fastq else None, first)
    out, rec, size = device_format(reads, heads, quals, fastq, first, len(want))
    assert size == len(want), (what, size, len(want))
    if out != want:
        i = next(j for j in range(len(want)) if out[j] != want[j])
        raise AssertionError("%s: the records differ at byte %d of %d: %r != %r" % (what, i, len(want), out[max(0, i - 20):i + 20], want[max(0, i - 20):i + 20]))
    n = len(reads)
    assert list(rec[:n + 1]) == want_off, what
    assert rec[n + 1] == 0x5A5A5A5A5A5A5A5A, "rec_off was written past its n_reads + 1 entries"
    return want, want_off


@pytest.mark.parametrize("case", bam_cases.cases(), ids=lambda c: c[0])
def test_records_against_the_restatement(case):
    check(case)


def test_fastq_layout_without_quals_pointer_and_fasta_with_one():
    """fastq == 0 ignores qualities that are given; fastq == 1 without d_quals writes 0xFF as well"""
    what, reads, heads, quals, fastq, first = bam_cases.cases()[0]
    want, _ = B.bam_records(reads, heads, None, first)
    for fq, q in ((False, quals), (True, None)):
        out, _, size = device_format(reads, heads, q, fq, first, len(want))
        assert size == len(want) and out == want


def test_name_refusals_name_the_smallest_read():
    from leon_amd import capi
    for what, reads, heads, quals, first, read, nbytes in bam_cases.name_refusals():
        with pytest.raises(B.BamRefusal) as want:
            B.bam_records(reads, heads, quals, first)
        with pytest.raises(capi.LeonDnaError) as e:
            device_format(reads, heads, quals, True, first, 4096)
        assert e.value.code == -1 and str(e.value).endswith("leon_records_bam_device: " + str(want.value)), (what, str(e.value))
        assert "read %d: its name has %d bytes, BAM allows 254" % (read, nbytes) in str(e.value)
    # names are checked before anything is written, so they come before a quality refusal, whichever read is the smaller
    what, reads, heads, quals, first, read, nbytes = bam_cases.name_refusals()[0]
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, [b" " * len(q) for q in quals], True, first, 4096)
    assert "its name has 255 bytes" in str(e.value)


def test_quality_refusals_name_their_read():
    from leon_amd import capi
    for what, reads, heads, quals, first, read in bam_cases.quality_refusals():
        with pytest.raises(B.BamRefusal) as want:
            B.bam_records(reads, heads, quals, first)
        assert want.value.read == read
        room = len(B.bam_records(reads, heads, None, first)[0])
        with pytest.raises(capi.LeonDnaError) as e:
            device_format(reads, heads, quals, True, first, room)
        assert e.value.code == -1 and str(e.value).endswith("leon_records_bam_device: read %d: a quality byte below 33" % read), (what, str(e.value))
    # two offenders: the smaller read
    what, reads, heads, quals, first, read = bam_cases.quality_refusals()[1]
    quals = list(quals)
    quals[33] = b" " * len(quals[33])
    quals[7] = quals[7][:-1] + b"\x00"
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, len(B.bam_records(reads, heads, None, first)[0]))
    assert str(e.value).endswith("read %d: a quality byte below 33" % (first + 7))


def test_refusals_leave_the_buffer_untouched():
    from leon_amd import capi
    what, reads, heads, quals, fastq, first = bam_cases.cases()[0]
    want, _ = B.bam_records(reads, heads, quals, first)
    n, room = len(reads), len(want)
    # a byte short: the size needed, nothing written (device_format checks buffer, rec_off and canaries before it raises again)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, cap=room - 1)
    assert e.value.code == -5 and e.value.out_size == room
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, None, quals, True, 99994, room, cap=0)
    assert e.value.code == -5 and e.value.out_size == len(B.bam_records(reads, None, quals, 99994)[0])
    for delta in (-1, 1, 1000):
        with pytest.raises(capi.LeonDnaError) as e:
            device_format(reads, heads, quals, True, first, room, n_bases=sum(map(len, reads)) + delta)
        assert e.value.code == -1 and "add up" in str(e.value)
    good = 1000 + np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)
    back = good.copy()
    back[2], back[3] = good[3], good[2]
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, hdr_off=back)
    assert e.value.code == -1 and "backwards" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, hdr_bytes=int(good[n] - good[0]) + 1)
    assert e.value.code == -1 and "do not end" in str(e.value)
    far = good.copy()
    far[n] += 1 << 30                                             # (no header byte is read through an offset outside the bytes given)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, hdr_off=far)
    assert e.value.code == -1 and "do not end" in str(e.value)
    low = good.copy()
    low[1:] -= 900                                                # offsets below the first one
    low[1] = good[1]
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, hdr_off=low)
    assert e.value.code == -1 and "backwards" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        device_format(reads, heads, quals, True, first, room, struct_size=ctypes.sizeof(capi.RecordLayout) + 8)
    assert e.value.code == -1 and "struct_size" in str(e.value)
    # and the library still formats after all that
    check(bam_cases.cases()[0])


@pytest.mark.parametrize("flags", [0, 1], ids=["runs", "matches"])
def test_records_through_the_bgzf_writer_behind_the_header(flags):
    """the device's records, the BAM header as the call's head, through leon_text_bgzf_device_ex: what any gzip reader reads back is
    header + records, and the stream ends with the EOF marker"""
    from leon_amd import capi
    assert capi.BGZF_F_MATCHES == 1
    case = next(c for c in bam_cases.cases() if c[0] == "3 000 reads of 150")
    head = B.bam_header()
    D = Dev()
    try:
        what, reads, heads, quals, fastq, first = case
        want, want_off = B.bam_records(reads, heads, quals, first)
        n = len(reads)
        lens = np.array([len(s) for s in reads] + [0], dtype=np.uint32)
        d_bases, d_len, d_quals = D.up(b"".join(reads) + b"\0"), D.up(lens.tobytes()), D.up(b"".join(quals) + b"\0")
        off = np.concatenate([[0], np.cumsum([len(h) for h in heads])]).astype(np.uint64)
        d_hdr, d_hoff = D.up(b"".join(heads) + b"\0"), D.up(off.tobytes())
        d_region = D.up(bytes(64 + len(want) + 64))
        d_rec = D.up(bytes(8 * (n + 1)))
        size = capi.records_bam_device(d_bases, d_len, n, sum(map(len, reads)), d_region + 64, len(want), fastq=True, first_read_index=first, d_hdr_text=d_hdr,
                                       d_hdr_off=d_hoff, hdr_bytes=int(off[n]), d_quals=d_quals, d_rec_off=d_rec)
        assert size == len(want)
        d_all = d_region + 64 - len(head)                        # the head lies right in front of the records
        assert capi.load_library().leon_device_upload(0, ctypes.c_void_p(d_all), ctypes.c_char_p(head), len(head)) == 0
        data, taken, members, m_out, m_text = capi.text_bgzf_device_ex(d_all, len(head), size, d_rec, n, flags=flags)
    finally:
        D.close()
    assert taken == len(head) + len(want) and members >= len(want) // capi.BGZF_MEMBER_TEXT
    assert data.endswith(capi.BGZF_EOF)
    assert gzip.decompress(data) == head + want
    # record-aligned: every member begins at the header or at a record start
    starts = {0} | {len(head) + o for o in want_off}
    assert all(int(t) in starts for t in m_text), "a member begins inside a record"
    assert [r[0] for r in B.parse_bam(gzip.decompress(data))] == [B.name_and_comment(h)[0] for h in heads]
