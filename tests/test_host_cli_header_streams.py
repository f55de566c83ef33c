"""-m gpu: `leon -d -header-text host|device` on a container whose header block was replaced, in place, by a stream our encoder
never writes (tests/header_streams.py): both routes restore the file the reader says, and both refuse a block that is no record
sequence with the same words.  The foreign payload is padded to the original's length with bytes no decoder reaches: a valid
stream is read to its end and no further."""
import os
import random
import subprocess

import pytest

import common
import container_patch as P
import header_streams as S
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")
FIRST = b"q7 x:12:007 abcdefghijkl"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def _foreign(n):
    """n headers of len(FIRST) bytes each, from records the encoder does not write"""
    EM = S.end_match()
    recs = [EM]
    for r in range(1, n):
        recs += [[S.numeric(2, 10 + r, b":", bc=9), EM],
                 [S.numeric(S.count("idx", 2, escape=True, bc=8), 40 + r, b":"), S.zero_numeric(3, 2, 7, b" ", bc=200), EM],
                 [S.ascii(4, 0, b"abcdefgh:jkl"), EM],
                 [S.delta(2, 1, bc=8), S.ascii(4, 0, b"abcdefgh!jkl"), S.end(S.count("idx", 5, escape=True))],
                 [S.ascii(4, 4, b"EFGHIJKL"), S.end(5)]][r % 5]
    return S.write(S.block(*recs))


def test_foreign_header_block_in_a_container(leon_bin, tmp_path):
    n, L = 30, 60
    rnd = random.Random(5)
    alnum = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    heads = [FIRST] + [bytes(rnd.choice(alnum) for _ in range(len(FIRST))) for _ in range(n - 1)]      # costly to code: room for the foreign block
    bases, off = common.synthetic(n, L, 3000, seed=5)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    fq = str(tmp_path / "f.fastq")
    with open(fq, "wb") as f:
        for h, s in zip(heads, reads):
            f.write(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "21")
    assert r.returncode == 0, r.stderr
    original = O.header_encode_block(heads, FIRST)
    at = P.find_bytes(fq + ".leon", original)

    foreign = _foreign(n)
    got = S.read(foreign, n, FIRST)
    assert not isinstance(got, S.Refused) and got[1] == 0
    want_heads = got[0]
    assert want_heads != heads and [len(h) for h in want_heads] == [len(FIRST)] * n and len(set(want_heads)) > 10
    assert len(foreign) <= len(original), (len(foreign), len(original))
    P.patch(fq + ".leon", at, foreign + b"\xa5" * (len(original) - len(foreign)))
    want = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in zip(want_heads, reads))
    for route in ("host", "device"):
        if os.path.exists(fq + ".d"):
            os.remove(fq + ".d")
        r = run(leon_bin, "-d", "-file", fq + ".leon", "-header-text", route, "-verbose", "1")
        assert r.returncode == 0, (route, r.stderr)
        assert open(fq + ".d", "rb").read() == want, route
        if route == "device":
            assert " 0 of 1 blocks fell back" in r.stdout, r.stdout

    # a block that is no record sequence: a delta on "007", then more records
    bad = S.write(S.block(S.end_match(), S.delta(3, 1), S.end_match()))
    assert isinstance(S.read(bad, n, FIRST), S.Refused)
    P.patch(fq + ".leon", at, bad + b"\xa5" * (len(original) - len(bad)))
    said = []
    for route in ("host", "device"):
        r = run(leon_bin, "-d", "-file", fq + ".leon", "-header-text", route)
        assert r.returncode != 0 and "header block 0 does not decode" in r.stderr, (route, r.stderr)
        said.append(r.stderr)
    assert said[0] == said[1]
