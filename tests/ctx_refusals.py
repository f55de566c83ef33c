"""The context calls' refusals, by name: replay() makes each refused call on the GPU and returns {name: [return code, leon_last_error text]}.
tests/golden/ctx_refusals.json holds what the library said before the context's calls were folded onto shared fronts (offset check,
host-batch upload, stream continuation, poisoned refusal, block table, raw range coder); tests/test_gpu_ctx_refusals.py replays the list
and compares.  All at 4 reads of 20 bases, k = 11.  The messages tests/test_gpu_parity.py pins by substring are not repeated there.

    python tests/ctx_refusals.py        # write the file (needs a GPU and the built library)"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ctx_refusals.json")
K = 11
GENOME = b"ACGTTGCATGCAAGCTTAGCTAGGATCCAGTCAGTCGATCGATTTAGC"
READS = [GENOME[5 * i:5 * i + 20] for i in range(4)]
HEADERS = [b"@r.%d len=20" % i for i in range(4)]


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def replay():
    import common
    import leon_amd
    import oracle_lib as O
    from leon_amd import capi
    lib = leon_amd.load_library()
    p64, p32, p8 = (lambda a: capi._ptr(a, capi._u64p)), (lambda a: capi._ptr(a, capi._u32p)), (lambda a: capi._ptr(a, capi._u8p))
    bases, off = O.reads_to_arrays(READS)
    bases = bytes(bases)
    off = _u64(off)
    n = len(READS)
    hdr = b"".join(HEADERS)
    hoff = _u64(np.concatenate([[0], np.cumsum([len(h) for h in HEADERS])]))
    quals = b"I" * len(bases)
    bl, solid, tai = common.make_bloom(bases, off, K, 1)
    out = {}

    def ctx(rpb, **kw):
        c = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=rpb, bloom_tai=tai, **kw)
        c.bloom_upload(bl.bits)
        return c

    def note(name, c, rc):
        assert rc != 0, name + ": the call was not refused"
        out[name] = [int(rc), (lib.leon_last_error(c.h) or b"").decode()]

    blocks = []
    keep = capi.SINK(lambda user, bid, ptr, size, nr: (blocks.append((bid, C.string_at(ptr, size), nr)), 0)[1])
    refuse = capi.SINK(lambda user, bid, ptr, size, nr: 1)
    vp = lambda b: C.cast(C.c_char_p(b), C.c_void_p)                                      # noqa: E731
    a = ctx(2)
    # ---- offsets that are no offsets array: in device memory (the kernel's check), in host memory (the entry point's) ----
    bad_mid, bad_ends = off.copy(), off.copy()
    bad_mid[2] = bad_mid[1] - 10
    bad_ends[0] = bad_ends[n] + 20
    bad_hmid, bad_hends = hoff.copy(), hoff.copy()
    bad_hmid[2] = bad_hmid[1] - 5
    bad_hends[0] = bad_hends[n] + 20
    d_bases, d_hdr, d_quals = (capi.device_upload_bytes(x) for x in (bases, hdr, quals))
    d_bad, d_hbad = capi.device_upload_bytes(bad_mid.tobytes()), capi.device_upload_bytes(bad_hmid.tobytes())
    note("encode: device offsets", a, lib.leon_dna_encode_batch_device(a.h, d_bases, d_bad, n, 0, keep, None))
    note("header: device offsets", a, lib.leon_header_encode_batch_device(a.h, d_hdr, d_hbad, n, 0, HEADERS[0], len(HEADERS[0]), keep, None))
    note("smooth: device offsets", a, lib.leon_qual_smooth_batch_device(a.h, d_bases, d_bad, n, d_quals))
    for p in (d_bases, d_hdr, d_quals, d_bad, d_hbad):
        capi.device_free(p)
    q = np.frombuffer(quals, dtype=np.uint8).copy()
    note("encode: host offsets", a, lib.leon_dna_encode_batch(a.h, vp(bases), p64(bad_ends), n, 0, keep, None))
    note("header: host offsets", a, lib.leon_header_encode_batch(a.h, hdr, p64(bad_hends), n, 0, HEADERS[0], len(HEADERS[0]), keep, None))
    note("smooth: host offsets", a, lib.leon_qual_smooth_batch(a.h, bases, p64(bad_ends), n, p8(q)))
    # ---- a stream goes on where it stopped, and a partial block ends it ----
    note("encode: first_read_index", a, lib.leon_dna_encode_batch(a.h, vp(bases), p64(off), n, 5, keep, None))
    note("header: first_read_index", a, lib.leon_header_encode_batch(a.h, hdr, p64(hoff), n, 5, HEADERS[0], len(HEADERS[0]), keep, None))
    b = ctx(3)
    assert lib.leon_dna_encode_batch(b.h, vp(bases), p64(off), n, 0, keep, None) == 0
    note("encode: after a partial block", b, lib.leon_dna_encode_batch(b.h, vp(bases), p64(off), n, n, keep, None))
    assert lib.leon_header_encode_batch(b.h, hdr, p64(hoff), n, 0, HEADERS[0], len(HEADERS[0]), keep, None) == 0
    note("header: after a partial block", b, lib.leon_header_encode_batch(b.h, hdr, p64(hoff), n, n, HEADERS[0], len(HEADERS[0]), keep, None))
    b.close()
    # ---- a sink that refuses a block poisons the stream ----
    note("encode: the sink refuses", a, lib.leon_dna_encode_batch(a.h, vp(bases), p64(off), n, 0, refuse, None))
    note("encode: poisoned", a, lib.leon_dna_encode_batch(a.h, vp(bases), p64(off), n, 0, keep, None))
    note("header: poisoned", a, lib.leon_header_encode_batch(a.h, hdr, p64(hoff), n, 0, HEADERS[0], len(HEADERS[0]), keep, None))
    pp, sz, na = capi._u8p(), C.c_uint64(), C.c_uint64()
    note("finish: poisoned", a, lib.leon_dna_finish(a.h, C.byref(pp), C.byref(sz), C.byref(na)))
    a.reset_stream()
    note("header: the sink refuses", a, lib.leon_header_encode_batch(a.h, hdr, p64(hoff), n, 0, HEADERS[0], len(HEADERS[0]), refuse, None))
    a.reset_stream()
    # ---- block tables ----
    del blocks[:]
    assert lib.leon_dna_encode_batch(a.h, vp(bases), p64(off), n, 0, keep, None) == 0 and len(blocks) == 2
    pay = np.frombuffer(b"".join(x[1] for x in blocks) + b"\0", dtype=np.uint8)
    good = _u64([0, len(blocks[0][1]), len(blocks[0][1]) + len(blocks[1][1])])
    back = _u64([0, good[2], good[1]])
    nreads, nbases = np.array([2, 2], dtype=np.uint32), _u64([40, 40])
    text, lens, anchors = np.zeros(96, dtype=np.uint8), np.zeros(8, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    note("decode: payload_off", a, lib.leon_dna_decode_blocks(a.h, p64(anchors), 0, p8(pay), p64(back), p32(nreads), p64(nbases), 2, p8(text), 80, p32(lens)))
    note("decode: out_cap", a, lib.leon_dna_decode_blocks(a.h, p64(anchors), 0, p8(pay), p64(good), p32(nreads), p64(nbases), 2, p8(text), 50, p32(lens)))
    hset = C.c_void_p()
    note("header symbols: payload_off", a, lib.leon_header_decode_symbols(a.h, p8(pay), p64(back), p32(nreads), 2, C.byref(hset)))
    # ---- the raw range coder ----
    syms, sizes = np.array([0, 0, 0, 1], dtype=np.uint8), np.zeros(2, dtype=np.uint64)
    rc_out = np.zeros(256, dtype=np.uint8)
    note("rc streams: begin[0]", a, lib.leon_rc_encode_streams(a.h, p8(syms), p64(_u64([1, 2])), 1, p8(rc_out), 256, p64(sizes)))
    syms[0] = 255
    note("rc streams: bad symbol", a, lib.leon_rc_encode_streams(a.h, p8(syms), p64(_u64([0, 2])), 1, p8(rc_out), 256, p64(sizes)))
    a.close()
    # ---- the dictionary's pieces exist from leon_dna_finish on ----
    d = ctx(2, dict_pieces=True)
    po, npieces, pa = capi._u64p(), C.c_uint64(), C.c_uint32()
    note("dict pieces: before finish", d, lib.leon_dna_dict_pieces(d.h, C.byref(po), C.byref(npieces), C.byref(pa)))
    d.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    got = replay()
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in sorted(got):
        print("%-34s %3d  %s" % (name, got[name][0], got[name][1]))
