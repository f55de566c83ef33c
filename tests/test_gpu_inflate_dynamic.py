"""-m gpu: the device's inflate (qi_stream of inflate_kernels.hip, behind leon_qual_inflate_blocks_device and leon_bgzf_inflate_device) on
the dynamic-code streams of deflate_cases.py -- valid streams zlib's encoder never writes (15-bit codes in both alphabets and 7-bit
code-length codes, repeats across the HLIT boundary, 284 + 31, every length and distance symbol at both ends of its extra bits, HCLEN
5 and 19, sparse distance sets, chains of all three block kinds, every copy route) and the dynamic headers and symbols zlib refuses.
test_deflate_tokens_cpu.py proves without a device that every case is what it is named for.  Accepted: the bytes are zlib's.
Refused: the device names the block the host function names, in its words.  The calls run in the harnesses of
test_gpu_qual_inflate.py and test_gpu_bgzf_inflate.py: canaries around the outputs, odd addresses, the payloads at every alignment."""
import pytest

import bgzf_input as B
import deflate_cases as C
import deflate_tokens as T
import test_gpu_bgzf_inflate as G
import test_gpu_qual_inflate as Q

pytestmark = pytest.mark.gpu

VALID, REFUSED = C.cases()


def test_valid_streams_as_quality_blocks():
    cases = [c for c in VALID if C.ZLIB in c.paths]
    assert len(cases) == len(VALID)
    blocks = [c.block() for c in cases]
    got = Q.both_accept(blocks)                                    # one wave per block, all in one launch
    assert b"".join(l + b"\n" for l in got) == b"".join(c.text for c in cases)          # zlib's bytes
    for shift in (0, 2, 3):                                        # the payloads at every alignment, in another order
        Q.both_accept(blocks[::-1], pay_shift=shift)
    for c in cases:                                                # each alone names itself when it fails
        assert Q.device_verdict([c.block()]) == c.text[:-1].split(b"\n"), c.name


def test_valid_streams_as_bgzf_members():
    cases = [c for c in VALID if C.RAW in c.paths]
    assert len(cases) == len(VALID) - 2                            # all but the two whose text does not fit a member
    members = [c.member() for c in cases]
    data = b"".join(members)
    off = B.offsets_of(data)
    got, _ = G.device_verdict(data, off)
    assert got == b"".join(c.text for c in cases)                  # zlib's bytes
    G.both_accept(data)
    G.both_accept(b"".join(members[::-1]), pay_shift=0)
    G.both_accept(b"".join(members[3:] + members[:3]), pay_shift=2, per_launch=1)      # every member alone in its launch
    G.both_accept(data + B.EOF, pay_shift=3, per_launch=5)


def test_refused_streams_as_quality_blocks():
    good = [c.block() for c in VALID if len(c.text) < 40000]
    for i, case in enumerate(REFUSED):
        bad = case.block()
        assert Q.refused_by_zlib(bad[0]), case.name + ": zlib accepts it"
        Q.both_refuse([good[i % len(good)], bad, good[(i + 7) % len(good)]], 1)
    # all of them in one call, a good block between every two: the smallest number is the one named
    blocks = []
    for i, case in enumerate(REFUSED):
        blocks += [good[(i + 3) % len(good)], case.block()]
    Q.both_refuse(blocks + good[:1], 1)
    Q.both_refuse(good[:5] + blocks[1:], 5)


def test_refused_streams_as_bgzf_members():
    good = [c.member() for c in VALID if C.RAW in c.paths]
    for i, case in enumerate(REFUSED):
        assert T.refusal(case.raw) is not None, case.name + ": zlib accepts it"
        a, b, c = good[i % len(good)], good[(i + 5) % len(good)], good[(i + 11) % len(good)]
        G.both_refuse([a, b, case.member(), c], 2)
        G.both_refuse([a, b, case.member(), c], 2, per_launch=2)   # the launch in front of the member's has written its text
    members = []
    for i, case in enumerate(REFUSED):
        members += [good[(i + 2) % len(good)], case.member()]
    G.both_refuse(members + good[:1], 1)
