"""-m gpu: the quality blocks inflated on the device (leon_qual_inflate_blocks_device: k_qual_inflate and the line pass) against
Python's zlib and leon_host_qual_decode_blocks -- never against the code under test.  Every call runs between two canaries around
d_quals and around d_qual_off; d_quals sits at an odd address.

A block is one zlib stream over the block's quality lines, each followed by a newline; block_n_bytes counts the bytes without them.
"""
import random
import threading
import zlib

import numpy as np
import pytest

import common
import hdr_samples

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5


# ---- helpers -----------------------------------------------------------------------------------------------------------------------

def text_of(lines):
    return b"".join(l + b"\n" for l in lines)


def block_of(lines, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None, flush=zlib.Z_SYNC_FLUSH, tail=b""):
    """(payload, n_reads, n_bytes) for the lines, written by zlib.compressobj"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    t = text_of(lines)
    if flush_at is None:
        pay = c.compress(t) + c.flush()
    else:
        pay = c.compress(t[:flush_at]) + c.flush(flush) + c.compress(t[flush_at:]) + c.flush()
    assert zlib.decompress(pay) == t
    return pay + tail, len(lines), sum(len(l) for l in lines)


def host_verdict(blocks):
    """leon_host_qual_decode_blocks on [(payload, n_reads, n_bytes)]: the list of lines, or (code, message)"""
    from leon_amd import capi
    try:
        return capi.host_qual_decode_blocks([(i, b[0], b[1]) for i, b in enumerate(blocks)], [b[2] for b in blocks], n_threads=4)
    except capi.LeonDnaError as e:
        return (e.code, str(e))


def device_verdict(blocks, d_len_of=None, pay_shift=1, n_blocks=None):
    """leon_qual_inflate_blocks_device on the same blocks between canaries: the list of lines, or (code, message).
    pay_shift: the payloads start that many bytes into a host array (an odd address when 1)"""
    from leon_amd import capi
    nb = len(blocks) if n_blocks is None else n_blocks
    raw = np.frombuffer(bytes(pay_shift) + b"".join(b[0] for b in blocks) + bytes(8), dtype=np.uint8)
    pay = raw[pay_shift:]
    off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    if blocks:
        off[1:] = np.cumsum([len(b[0]) for b in blocks])
    nr = np.array([b[1] for b in blocks] + [0], dtype=np.uint32)
    nbytes = np.array([b[2] for b in blocks] + [0], dtype=np.uint64)
    total, cap = int(nr[:nb].sum()), int(nbytes[:nb].sum())
    ptrs = []
    try:
        d_q = capi.device_upload_bytes(bytes([FILL]) * (CANARY + SHIFT + cap + CANARY + 32))
        ptrs.append(d_q)
        d_o = capi.device_upload_bytes(bytes([FILL]) * (CANARY + 8 * (total + 1) + CANARY))
        ptrs.append(d_o)
        d_len = 0
        if d_len_of is not None:
            d_len = capi.device_upload_bytes(np.asarray(list(d_len_of) + [0], dtype=np.uint32).tobytes())
            ptrs.append(d_len)
        try:
            capi.qual_inflate_blocks_device(pay, off, nr, nbytes, d_q + CANARY + SHIFT, cap, d_o + CANARY, d_len, n_blocks=nb)
            verdict = None
        except capi.LeonDnaError as e:
            verdict = (e.code, str(e))
        q = capi.device_download(d_q, CANARY + SHIFT + cap + CANARY + 32)
        o = capi.device_download(d_o, CANARY + 8 * (total + 1) + CANARY)
        assert q[:CANARY + SHIFT] == bytes([FILL]) * (CANARY + SHIFT), "bytes in front of d_quals were written"
        assert q[CANARY + SHIFT + cap:] == bytes([FILL]) * (CANARY + 32), "bytes behind d_quals were written"
        assert o[:CANARY] == bytes([FILL]) * CANARY and o[CANARY + 8 * (total + 1):] == bytes([FILL]) * CANARY, "bytes around d_qual_off were written"
        if verdict is not None:
            return verdict
        if nb == 0:
            assert q == bytes([FILL]) * len(q) and o == bytes([FILL]) * len(o)
            return []
        offs = np.frombuffer(o[CANARY:CANARY + 8 * (total + 1)], dtype=np.uint64)
        assert offs[0] == 0 and offs[-1] == cap and np.all(offs[1:] >= offs[:-1])
        body = q[CANARY + SHIFT:CANARY + SHIFT + cap]
        return [body[int(offs[i]):int(offs[i + 1])] for i in range(total)]
    finally:
        for p in ptrs:
            capi.device_free(p)


def both_accept(blocks, **kw):
    want = host_verdict(blocks)
    assert isinstance(want, list), want
    for b in blocks:
        t = zlib.decompressobj().decompress(b[0])
        assert len(t) == b[1] + b[2] and t.count(b"\n") == b[1]
    got = device_verdict(blocks, **kw)
    assert isinstance(got, list), got
    assert got == want
    return got


def both_refuse(blocks, first_bad):
    """zlib (or the line rules) refuses the block first_bad, so does the host function, and the device names the same block"""
    want = host_verdict(blocks)
    assert isinstance(want, tuple) and want[0] == -1 and ("quality block %d does not decode" % first_bad) in want[1], want
    got = device_verdict(blocks)
    assert isinstance(got, tuple) and got[0] == -1 and ("quality block %d does not decode" % first_bad) in got[1], (got, want)


def lossy_lines(n, L, rng):
    """what the lossy form leaves: '@' nearly everywhere"""
    out = []
    for _ in range(n):
        l = bytearray(b"@" * L)
        for _ in range(rng.randrange(0, 4)):
            if L:
                l[rng.randrange(L)] = rng.choice(b"#,5<AFJ")
        out.append(bytes(l))
    return out


class Bits:
    """deflate's bit order: fields from the least significant bit on, Huffman codes from their most significant bit on"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        for i in range(n - 1, -1, -1):
            self.put(v >> i & 1, 1)

    def lit(self, s):                                   # the fixed literal/length code (RFC 1951, 3.2.6)
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def zstream(body, text=b""):
    return b"\x78\x9c" + body + zlib.adler32(text).to_bytes(4, "big")


def refused_by_zlib(payload):
    try:
        d = zlib.decompressobj()
        d.decompress(payload)
        return not d.eof
    except zlib.error:
        return True


# ---- valid streams -----------------------------------------------------------------------------------------------------------------

SAMPLE = None


def sample_lines():
    global SAMPLE
    if SAMPLE is None:
        SAMPLE = hdr_samples.fastq_quals(50000, 0, seed=11)
    return SAMPLE


@pytest.mark.parametrize("level,strategy,wbits", [(0, zlib.Z_DEFAULT_STRATEGY, 15), (1, zlib.Z_DEFAULT_STRATEGY, 15), (6, zlib.Z_DEFAULT_STRATEGY, 15),
                                                  (9, zlib.Z_DEFAULT_STRATEGY, 15), (6, zlib.Z_FILTERED, 15), (6, zlib.Z_HUFFMAN_ONLY, 15),
                                                  (6, zlib.Z_RLE, 15), (6, zlib.Z_FIXED, 15), (6, zlib.Z_DEFAULT_STRATEGY, 9), (9, zlib.Z_RLE, 9)])
def test_streams_of_every_writer(level, strategy, wbits):
    lines = sample_lines()
    assert len({len(l) for l in lines}) == 201
    rng = random.Random(level * 100 + strategy * 10 + wbits)
    blocks = [block_of(lines, level, strategy, wbits),
              block_of(lossy_lines(3000, 150, rng), level, strategy, wbits),
              block_of(lines[:700], level, strategy, wbits, flush_at=20000, flush=zlib.Z_SYNC_FLUSH),
              block_of(lines[700:1500], level, strategy, wbits, flush_at=1, flush=zlib.Z_FULL_FLUSH, tail=b"\x00trailing bytes\xff" * 3)]
    both_accept(blocks)


def test_texts():
    rng = random.Random(5)
    far = [bytes(rng.choice(b"#,-5:<>?@ABCDEFGHIJ") for _ in range(150)) for _ in range(218)]          # 218 x 151 = 32 918 bytes
    repeated = far + far + far[5:60] + [far[0][:70] + far[217][70:]] + far                                 # lines from up to 32 768 back, and across it
    blocks = [block_of(repeated, 9),
              block_of(lossy_lines(400, 700, rng), 6),                                                      # length-258 matches at distance 1
              block_of([b"", b"", b"", b"I", b""], 6),
              block_of([b""], 6),
              block_of([bytes(rng.choice(b"@@@@@@@@@FJ#") for _ in range(300000))], 6),                  # one 300 kb line
              block_of([b"IIIIIIII"], 6),                                                                   # a block of one read
              block_of([], 6)]                                                                              # an empty block
    both_accept(blocks)
    for shift in (0, 1, 2, 3):                                                                              # the payloads at every alignment
        both_accept(blocks[2:6] + blocks[:1], pay_shift=shift)
    assert device_verdict([]) == []                                                                         # a call of 0 blocks touches nothing


def test_a_full_block():
    rng = np.random.default_rng(3)
    q = (33 + rng.integers(0, 41, size=50000 * 150)).astype(np.uint8).tobytes()
    lines = [q[i * 150:(i + 1) * 150] for i in range(50000)]
    both_accept([block_of(lines, 6)])


def test_sixty_four_unequal_blocks():
    rng = random.Random(8)
    lines = sample_lines()
    blocks = []
    for b in range(64):
        n = rng.choice((0, 1, 2, 17, 300, 1200, 2500))
        at = rng.randrange(0, len(lines) - n)
        blocks.append(block_of(lines[at:at + n] if b % 5 else lossy_lines(n, rng.randrange(0, 400), rng), rng.choice((0, 1, 6, 9)),
                               rng.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_RLE, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)), tail=bytes(rng.randrange(0, 4))))
    both_accept(blocks)


def test_blocks_written_by_the_device():
    from leon_amd import capi
    rng = random.Random(9)
    lines = sample_lines()[:9000] + lossy_lines(3000, 150, rng)
    off = np.zeros(len(lines) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lines])
    d = capi.device_upload_bytes(b"".join(lines) + b"\0")
    try:
        written = capi.qual_deflate_blocks_device(d, off, 2500)
    finally:
        capi.device_free(d)
    blocks = []
    for (bid, pay, n) in written:
        part = lines[bid * 2500:bid * 2500 + n]
        assert zlib.decompress(pay) == text_of(part)
        blocks.append((pay, n, sum(len(l) for l in part)))
    assert len(blocks) == 5
    got = both_accept(blocks)
    assert got == lines
    quals, offsets = capi.qual_inflate_blocks([(i, b[0], b[1]) for i, b in enumerate(blocks)], [b[2] for b in blocks])     # the convenience form
    assert quals == b"".join(lines) and np.array_equal(offsets, off)


def test_d_len():
    lines = sample_lines()[:3000]
    blocks = [block_of(lines[:1000], 6), block_of(lines[1000:], 6)]
    lens = [len(l) for l in lines]
    assert device_verdict(blocks, d_len_of=lens) == lines
    r = next(i for i in range(1500, 2999) if lens[i + 1] > 0)
    moved = list(lines)
    moved[r], moved[r + 1] = lines[r] + lines[r + 1][:1], lines[r + 1][1:]                                  # one read a byte longer, its neighbour one shorter
    blocks = [block_of(moved[:1000], 6), block_of(moved[1000:], 6)]
    assert device_verdict(blocks) == moved                                                                   # the blocks themselves decode
    got = device_verdict(blocks, d_len_of=lens)
    assert isinstance(got, tuple) and got[0] == -1 and "read %d " % r in got[1] and "block 1" in got[1], got


# ---- streams that must be refused ---------------------------------------------------------------------------------------------------

def crafted():
    """(name, payload): each refused by zlib -- asserted by the test before the device sees it.  The block table says 1 read, 1 byte."""
    out = []
    b = Bits(); b.put(1, 1); b.put(1, 2); b.lit(65); b.lit(257); b.code(1, 5); b.lit(256)
    out.append(("a match that reaches before the first byte", zstream(b.done())))
    b = Bits(); b.put(1, 1); b.put(1, 2); b.lit(65); b.lit(286); b.lit(256)
    out.append(("literal/length symbol 286", zstream(b.done())))
    b = Bits(); b.put(1, 1); b.put(1, 2); b.lit(65); b.lit(65); b.lit(257); b.code(30, 5); b.lit(256)
    out.append(("distance symbol 30", zstream(b.done())))
    b = Bits(); b.put(1, 1); b.put(0, 2); b.align(); b.put(2, 16); b.put(0xFFFD ^ 1, 16); b.put(65, 8); b.put(10, 8)
    out.append(("stored LEN != ~NLEN", zstream(b.done(), b"A\n")))
    b = Bits(); b.put(1, 1); b.put(3, 2); b.put(0, 13)
    out.append(("block type 3", zstream(b.done())))
    b = Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    b.put(0, 32)
    out.append(("an over-subscribed code-length code", zstream(b.done())))
    # literal/length lengths 1, 1 and 255 zeros (no end-of-block code), one distance length 0; the code-length code: '1' -> 0, '18' -> 1
    b = Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(14, 4)
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        b.put(1 if sym in (18, 1) else 0, 3)
    b.code(0, 1); b.code(0, 1); b.code(1, 1); b.put(127, 7); b.code(1, 1); b.put(107, 7); b.put(0, 32)
    out.append(("a dynamic block without an end-of-block code", zstream(b.done())))
    good = zlib.compress(b"A\n")
    fdict = bytes([0x78, next(f for f in range(256) if f & 0x20 and (0x7800 + f) % 31 == 0)]) + good[2:]
    out.append(("FDICT set", fdict))
    out.append(("a wrong FCHECK", good[:1] + bytes([good[1] ^ 1]) + good[2:]))
    out.append(("CM != 8", bytes([0x77, next(f for f in range(256) if not f & 0x20 and (0x7700 + f) % 31 == 0)]) + good[2:]))
    out.append(("CINFO 8", bytes([0x88, next(f for f in range(256) if not f & 0x20 and (0x8800 + f) % 31 == 0)]) + good[2:]))
    out.append(("a flipped Adler-32 bit", good[:-2] + bytes([good[-2] ^ 0x10]) + good[-1:]))
    return out


def test_crafted_streams_are_refused_with_their_block():
    ok = (zlib.compress(b"A\n"), 1, 1)
    assert host_verdict([ok]) == [b"A"]
    for name, pay in crafted():
        assert refused_by_zlib(pay), name + ": zlib accepts it"
        both_refuse([ok, (pay, 1, 1), ok], 1)
    # the fixed-code machinery of the writer above is sound: the same blocks without their fault decode
    b = Bits(); b.put(1, 1); b.put(1, 2); b.lit(65); b.lit(65); b.lit(257); b.code(1, 5); b.lit(10); b.lit(256)
    both_accept([(zstream(b.done(), b"AAAAA\n"), 1, 5)])
    b = Bits(); b.put(0, 1); b.put(0, 2); b.align(); b.put(2, 16); b.put(0xFFFD, 16); b.put(65, 8); b.put(66, 8)
    b.put(1, 1); b.put(1, 2); b.lit(257); b.code(1, 5); b.lit(10); b.lit(256)
    both_accept([(zstream(b.done(), b"ABABA\n"), 1, 5)])


def test_cut_streams_and_wrong_tables():
    lines = sample_lines()[:400]
    pay, n, nb = block_of(lines, 6)
    ok = (pay, n, nb)
    rng = random.Random(12)
    cuts = sorted({0, 1, 2, 3, len(pay) - 1, len(pay) - 2, len(pay) - 4, len(pay) - 5} | {rng.randrange(4, len(pay) - 5) for _ in range(32)})
    for cut in cuts:
        assert refused_by_zlib(pay[:cut])
    both_refuse([ok] + [(pay[:cut], n, nb) for cut in cuts], 1)
    for i, cut in enumerate(cuts):                                                                          # each of them alone, behind a good block
        if i % 4 == 0:
            both_refuse([ok, (pay[:cut], n, nb)], 1)
    both_refuse([ok, (pay, n, nb - 1), ok], 1)                                                              # the stream is one byte LONGER than the table says
    both_refuse([ok, (pay, n, nb + 1), ok], 1)                                                              # ... one byte SHORTER
    both_refuse([ok, (pay, n + 1, nb - 1), ok], 1)                                                          # a read more in the table: a newline too few
    extra = text_of(lines)
    extra = extra[:50] + b"\n" + extra[51:] if extra[50:51] != b"\n" else extra[:51] + b"\n" + extra[52:]
    assert extra.count(b"\n") == n + 1 and len(extra) == n + nb
    both_refuse([ok, (zlib.compress(extra), n, nb), ok], 1)                                                 # a newline too many and a byte fewer
    no_last = bytearray(text_of(lines)[:-1] + b"I")
    no_last[next(i for i, c in enumerate(no_last) if c != 10)] = 10
    assert no_last.count(b"\n") == n and len(no_last) == n + nb
    both_refuse([ok, (zlib.compress(bytes(no_last)), n, nb), ok], 1)                                        # the right counts, but the last byte is no newline
    bad = (pay[:len(pay) // 2], n, nb)
    both_refuse([ok, ok, bad, ok, bad], 2)                                                                  # a good block between two bad ones: the smallest number
    both_accept([ok, ok])


def test_damaged_payloads_get_the_hosts_verdict():
    """200 seeded damages of good payloads: the device's verdict is leon_host_qual_decode_blocks', and where both accept, the same bytes"""
    rng = random.Random(2024)
    lines = sample_lines()
    goods = [block_of(lines[:300], 6), block_of(lines[300:900], 9), block_of(lossy_lines(200, 150, rng), 6), block_of(lines[900:1000], 6, zlib.Z_FIXED),
             block_of(lines[1000:1200], 0), block_of(lines[1200:1500], 6, zlib.Z_RLE)]
    accepted = refused = 0
    for case in range(200):
        pay, n, nb = goods[case % len(goods)]
        p = bytearray(pay)
        kind = rng.randrange(4)
        if kind == 0:
            p[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            at = rng.randrange(len(p))
            for i in range(at, min(len(p), at + rng.randrange(2, 9))):
                p[i] = rng.randrange(256)
        elif kind == 2:
            at = rng.randrange(len(p))
            del p[at:at + rng.randrange(1, 5)]
        else:
            at = rng.randrange(len(p))
            p[at:at] = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 5)))
        blocks = [goods[(case + 1) % len(goods)], (bytes(p), n, nb)]
        want, got = host_verdict(blocks), device_verdict(blocks)
        if isinstance(want, list):
            assert got == want, case
            accepted += 1
        else:
            assert isinstance(got, tuple) and got[0] == want[0] == -1 and "quality block 1 does not decode" in got[1] and "quality block 1 does not decode" in want[1], (case, got, want)
            refused += 1
    assert refused > 100 and accepted + refused == 200


def test_beside_a_dna_decode():
    """the call on its own stream while a context decodes DNA blocks on another thread: both results as when they run alone"""
    import leon_amd
    from leon_amd import capi
    k, rpb, n = 25, 400, 1900
    bases, off = common.synthetic(n, 120, 7000, seed=31, n_rate=0.004, err=0.02, ragged=True)
    bl, solid, tai = common.make_bloom(bases, off, k)
    ctx = leon_amd.DnaEncodeContext(kmer_size=k, reads_per_block=rpb, bloom_tai=tai)
    try:
        ctx.bloom_insert(solid)
        dna_blocks = ctx.encode_batch(bases, off)
        dict_payload, n_anchors = ctx.finish()
        anchors = capi.anchor_dict_decode(dict_payload, n_anchors, k)
        nbases = [int(off[min(n, (b + 1) * rpb)] - off[b * rpb]) for b in range(len(dna_blocks))]
        want_bases, want_lens = ctx.decode_blocks_raw(anchors, dna_blocks, nbases)
        lines = sample_lines()[:20000]
        qblocks = [block_of(lines[i:i + 2500], 6) for i in range(0, 20000, 2500)]
        alone = device_verdict(qblocks)
        assert alone == lines
        res = {}

        def dna():
            try:
                res["dna"] = [ctx.decode_blocks_raw(anchors, dna_blocks, nbases) for _ in range(3)]
            except Exception as e:                      # noqa: BLE001 -- reported by the assertion below
                res["dna"] = e

        def qual():
            try:
                res["qual"] = [device_verdict(qblocks) for _ in range(3)]
            except Exception as e:                      # noqa: BLE001
                res["qual"] = e
        th = [threading.Thread(target=dna), threading.Thread(target=qual)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert isinstance(res["dna"], list) and isinstance(res["qual"], list), res
        for got_bases, got_lens in res["dna"]:
            assert got_bases.tobytes() == want_bases.tobytes() and np.array_equal(got_lens, want_lens)
        for got in res["qual"]:
            assert got == lines
    finally:
        ctx.close()
