"""No GPU: the inputs of tests/many_blocks.py are what they claim to be -- the layout of kinds over the workgroup slots and trips,
the streams', reads' and headers' stated shapes -- and the oracle alone handles them (round trips through its own decoders).
tests/test_gpu_many_blocks.py runs the same inputs through the kernels."""
import collections

import numpy as np

import common
import many_blocks as MB
import oracle_lib as O


def test_block_count_passes_every_grid_cap_twice():
    assert MB.CAP == 2048 and MB.CAP_RC_RECORDS == 1024 and MB.N_BLOCKS == 4099
    assert MB.N_BLOCKS // MB.CAP == 2 and MB.N_BLOCKS % MB.CAP == 3                  # two full trips, three blocks on the third
    assert (MB.N_BLOCKS + MB.CAP_RC_RECORDS - 1) // MB.CAP_RC_RECORDS == 5           # k_rc_records4: five trips
    assert [MB.N_BLOCKS % g for g in (2, 4, 8)] == [1, 3, 3]                         # the last group of G blocks is partial


def test_consecutive_trips_of_a_slot_see_every_pair_of_kinds():
    pairs = collections.Counter((MB.kind(s), MB.kind(s + MB.CAP)) for s in range(MB.CAP))
    assert len(pairs) == 56 and all(a != b for a, b in pairs)
    assert min(pairs.values()) >= 30, min(pairs.values())
    for s in range(3):                                                               # the third trip differs from the second as well
        assert MB.kind(s + 2 * MB.CAP) != MB.kind(s + MB.CAP)
    for g in range(0, MB.CAP, 8):                                                    # one G = 8 group: all 8 kinds, so 8 different tile counts
        assert sorted(MB.kind(b) for b in range(g, g + 8)) == list(range(8)), g
        assert sorted(MB.kind(b) for b in range(MB.CAP + g, MB.CAP + g + 8)) == list(range(8)), g


def test_symbol_streams_are_as_stated_and_the_oracle_round_trips_them():
    syms, begin, sizes = MB.rc_streams()
    assert len(begin) == MB.N_BLOCKS + 1 and begin[0] == 0 and len(syms) == 2 * int(begin[-1])
    assert 2_000_000 < int(begin[-1]) < 2_500_000
    assert sizes[:MB.N_SMALL] == [2, 5, 5, 2, 3, 3, 3, 2] and len(sizes) == 80
    m_all, v_all = syms[0::2], syms[1::2]
    assert m_all.max() < 80 and np.all(v_all.astype(np.int64) < np.array(sizes)[m_all])
    seen = set()
    for b in range(MB.N_BLOCKS):
        kd = MB.kind(b)
        m, v = MB.rc_stream(b)
        lo, hi = MB.STREAM_LEN[kd]
        assert lo <= len(m) <= hi, (b, MB.KIND_NAMES[kd], len(m))
        if kd == MB.ONE:
            assert m[0] < MB.N_SMALL
        elif kd == MB.NARROW:
            assert m.max() <= 9 and {8, 9} <= set(m.tolist())
        elif kd == MB.WIDE:
            # all 72 numeric models within the first two tiles: more than RC_NSLOT_BIG = 24, so the global overflow area is in use
            assert set(m[:128].tolist()) >= set(range(MB.N_SMALL, 80)), b
            assert len(set(m[128:].tolist()) - set(range(MB.N_SMALL))) > 60
        elif kd == MB.SKEW:
            assert len(set(m.tolist())) == 1 and m[0] >= MB.N_SMALL and len(set(v.tolist())) == 1 and len(m) + 256 > 2 * 256
        if kd not in seen or b >= MB.N_BLOCKS - 3:                                   # one stream of every kind, and the third trip's
            seen.add(kd)
            pay = O.rc_encode_stream(m, v, sizes)
            assert np.array_equal(O.rc_decode_stream(pay, m, sizes), v), (b, MB.KIND_NAMES[kd])
    assert len(seen) == 8


def test_reads_are_as_stated_and_the_oracle_round_trips_the_corner_blocks():
    reads = MB.dna_reads()
    rpb = MB.DNA_RPB
    assert len(reads) == MB.N_BLOCKS * rpb == 12297
    b0, b1 = MB.dna_long_read_blocks()
    assert b0 < MB.CAP <= b1 < 2 * MB.CAP and b0 % MB.CAP != b1 % MB.CAP
    assert MB.dna_heavy(b0) and not MB.dna_heavy(b0 + MB.CAP)                        # a light block follows the long read on its wave
    assert MB.dna_heavy(b1) and not MB.dna_heavy(b1 - MB.CAP)                        # a light block precedes the other on its wave
    long_at = [i for i, r in enumerate(reads) if len(r) > 1000]
    assert long_at == [rpb * b0 + 1, rpb * b1 + 1] and all(len(reads[i]) == MB.LONG_READ_LEN for i in long_at)
    for i in long_at:                                                                # N and error lists longer than DC_LIST_CAP = 8192
        assert reads[i].count(b"N") > 8192
    junk = MB.dna_junk_blocks()
    assert len(junk) >= 100 and all(len(reads[rpb * b]) > 255 for b in junk)
    for b in range(MB.N_BLOCKS):
        blk = reads[rpb * b:rpb * (b + 1)]
        if not MB.dna_heavy(b):
            assert all(len(r) == 100 and set(r) <= set(b"ACGT") for r in blk), b
        elif b not in (b0, b1):
            assert all(150 <= len(r) <= 600 for r in blk), b
    heavy = [r for b in range(MB.N_BLOCKS) if MB.dna_heavy(b) for r in reads[rpb * b:rpb * (b + 1)]]
    assert sum(r.find(b"N", 256) >= 0 for r in heavy) > 1000                         # N positions that need a second byte
    # the oracle alone: encode everything at k = 31, decode the corner blocks
    k = 31
    bases, off = O.reads_to_arrays(reads)
    bl, solid, tai = common.make_bloom(bases, off, k)
    ref = O.encode(bases, off, k, rpb, bl, trace=True)
    assert len(ref.blocks) == MB.N_BLOCKS and ref.block_nreads == [rpb] * MB.N_BLOCKS and ref.n_anchors > 1000
    # random bases hold no solid k-mer, but some 300 of them are tried against a bloom with a false-positive rate of a few in a
    # thousand: about half of the ~130 junk reads stay without an anchor, coded base by base over more than 255 bases
    assert int((ref.anchor_pos[[rpb * b for b in junk]] < 0).sum()) >= 20
    assert int((ref.anchor_pos > 255).sum()) > 100 and int(ref.anchor_addr.max()) > 255
    anchors = O.decode_anchor_dict(ref.anchor_dict, ref.n_anchors, k)
    want = MB.dna_normalised(reads)
    for b in (0, MB.CAP - 1, MB.CAP, MB.N_BLOCKS - 1, b0, b1):
        nb = sum(len(r) for r in reads[rpb * b:rpb * (b + 1)])
        assert O.decode_block(k, bl, anchors, ref.blocks[b], rpb, nb + 16) == want[rpb * b:rpb * (b + 1)], b


def _share(n_reads, payload):
    """hdr_symbols_launch's share of the symbol buffer for one block (hdr_kernels.hip): a block with more symbols goes to the host decoder"""
    return 24 * n_reads + 6 * len(payload) + 256


def test_headers_are_as_stated_and_the_oracle_round_trips_them():
    from leon_amd import capi
    assert MB.HDR_CAP == capi.HEADER_TEXT_DEVICE_CAP
    rpb = MB.HDR_RPB
    hs, first = MB.headers()
    assert len(hs) == MB.N_BLOCKS * rpb and 2900 <= len(first) <= 3000
    assert max(map(len, hs)) == MB.HDR_CAP - 1                                       # below the cap, and the longest one is there
    for w in range(0, len(first) - 64, 64):                                          # a separator in every 64-byte word of the template
        assert b":" in first[w:w + 64], w
    for b in range(MB.N_BLOCKS):
        blk = hs[rpb * b:rpb * (b + 1)]
        if MB.hdr_heavy(b):
            assert all(len(h) in MB.HDR_LENGTHS for h in blk), b
        else:
            assert all(h.startswith(b"SRR1.") and len(h) < 32 for h in blk), b
    assert {len(h) for h in hs} >= set(MB.HDR_LENGTHS)
    # every block within its share of the device's symbol buffer (the oracle's trace has one row per coded symbol)
    for b in range(MB.N_BLOCKS):
        pay, trace = O.header_encode_block(list(hs[rpb * b:rpb * (b + 1)]), first, with_trace=True)
        assert len(trace) <= _share(rpb, pay), (b, len(trace), len(pay))
        if b % 500 == 0 or b == MB.N_BLOCKS - 1:
            want = list(hs[rpb * b:rpb * (b + 1)])
            assert O.header_decode_block(pay, rpb, first, sum(map(len, want)) + 64) == want, b
    hs2, first2, replaced = MB.headers_with_fallbacks()
    assert first2 == first and list(replaced) == MB.fallback_blocks() and len(replaced) == 20
    slots = {b % MB.CAP for b in replaced}
    assert len(slots) == len(replaced)                                               # the same slot's other trips are ordinary blocks
    differ = {i // rpb for i in range(len(hs)) if hs[i] != hs2[i]}
    assert differ <= set(replaced) and len(differ) >= len(replaced) - 2
    over = [b for b in replaced if max(map(len, hs2[rpb * b:rpb * (b + 1)])) > MB.HDR_CAP]
    assert over == list(replaced[0::2])
    for b in list(replaced) + list(range(0, MB.N_BLOCKS, 500)):
        want = list(hs2[rpb * b:rpb * (b + 1)])
        pay = O.header_encode_block(want, first)
        assert O.header_decode_block(pay, rpb, first, sum(map(len, want)) + 64) == want, b
