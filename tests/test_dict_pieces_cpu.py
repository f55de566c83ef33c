"""The anchor dictionary in independently coded pieces, without a GPU: the host twins leon_host_anchor_dict_encode_pieces /
leon_host_anchor_dict_decode_pieces -- the verdict for the device calls -- against leon_host_anchor_dict_encode on every slice and against
the oracle's coder and decoder; the census of the directed lists (tests/dict_pieces.py), certified by the reference alone; every refusal
with its words; and the host header as a program of its own under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import dict_pieces as DP
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import leon_amd
    if not os.path.exists(leon_amd.lib_path()):
        leon_amd.build_library()
    leon_amd.load_library()
    from leon_amd import capi
    return capi


def _refused(capi, fn, *a, **kw):
    with pytest.raises(capi.LeonDnaError) as e:
        fn(*a, **kw)
    return e.value


@pytest.mark.parametrize("k", DP.KS)
def test_host_pieces_equal_the_slices_and_the_oracle(capi, k):
    """every piece == leon_host_anchor_dict_encode(its slice) == the oracle's bytes; the decode twin gives the k-mers back and the oracle's
    decoder reads every piece; the table is the pieces' sizes summed"""
    W = O.kwords(k)
    for _, P, n in [s for s in DP.shapes() if s[0] == k]:
        syms = DP.random_syms(1000 * k + 7 * P + n, n, k)
        kmers = DP.kmers_from_syms(syms, k)
        stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P, n_threads=3)
        bounds = DP.piece_bounds(n, P)
        assert len(off) == len(bounds) + 1 == capi.dict_piece_count(n, P) + 1 and off[0] == 0 and int(off[-1]) == len(stream), (k, P, n)
        pieces = DP.split(stream, off)
        want = DP.ref_pieces(syms, n, k, P)
        assert pieces == want, (k, P, n)
        for i, ((a, b), piece) in enumerate(zip(bounds, pieces)):
            assert len(piece) >= 8
            if i < 2 or i == len(bounds) - 1:                      # (a fresh chain worker with its helper threads per call: three slices a shape)
                assert piece == capi.host_anchor_dict_encode(kmers[a * W:b * W], k), (k, P, n, a)
            assert np.array_equal(O.decode_anchor_dict(piece, b - a, k), kmers[a * W:b * W]), (k, P, n, a)
        assert np.array_equal(capi.host_anchor_dict_decode_pieces(stream, off, n, k, P, n_threads=2), kmers), (k, P, n)
        s1, o1 = capi.host_anchor_dict_encode_pieces(kmers, k, P, n_threads=1)
        assert s1 == stream and np.array_equal(o1, off), (k, P, n)


def test_default_piece_size_is_1024(capi):
    k, n = 31, 2 * 1024 + 5
    syms = DP.random_syms(5, n, k)
    kmers = DP.kmers_from_syms(syms, k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, 0)
    assert len(off) == 4 and DP.split(stream, off) == DP.ref_pieces(syms, n, k, 1024)
    assert np.array_equal(capi.host_anchor_dict_decode_pieces(stream, off, n, k, 0), kmers)
    assert np.array_equal(capi.host_anchor_dict_decode_pieces(stream, off, n, k, 1024), kmers)


def test_census_of_the_directed_lists():
    """what the lists must hold, from the reference's per-step record alone"""
    R = DP.rare_steps("resets")
    k, P, n, syms = DP.resets()
    last = k * P - 1
    for p, at in DP.RESETS_AT.items():
        assert [s for s in R[p] if s[2]] == [s for s in R[p]] and [s[0] for s in R[p]] == [at], (p, R.get(p))
    assert any(p % 64 and any(s[2] for s in steps) for p, steps in R.items())                 # a reset in a piece that is not lane 0
    assert any(s[0] == last and s[2] for s in R[3])                                           # ... one as a piece's last step
    assert R[1][0][0] == R[2][0][0] != R[5][0][0]                                             # two pieces of one wave: same step, another step
    S = DP.rare_steps("strikes")
    k, P, n, syms = DP.strikes()
    assert n % P == DP.STRIKES_TAIL and k * P >= (1 << 17)
    for p, at in DP.STRIKES_AT.items():
        big = [s for s in S[p] if s[1] >= 4 and not s[2]]
        assert [s[0] for s in big] == [at] and 5 + at > (1 << 17) and p % 64, (p, big)
        assert not np.any(syms[p * k * P:p * k * P + at] == 3)                               # the piece has never used value 3 before
    assert DP.STRIKES_AT[1] == DP.STRIKES_AT[2] != DP.STRIKES_AT[3]
    assert any(s[2] for steps in S.values() for s in steps)                                   # (random symbols on so small a model reach resets too)


@pytest.mark.parametrize("name", sorted(DP.DIRECTED))
def test_host_pieces_on_the_directed_lists(capi, name):
    k, P, n, syms = DP.DIRECTED[name]()
    kmers = DP.kmers_from_syms(syms, k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    assert DP.split(stream, off) == DP.ref_pieces(syms, n, k, P)
    assert np.array_equal(capi.host_anchor_dict_decode_pieces(stream, off, n, k, P), kmers)
    for (a, b), piece in zip(DP.piece_bounds(n, P), DP.split(stream, off)):
        assert np.array_equal(O.decode_anchor_dict(piece, b - a, k), kmers[a * O.kwords(k):b * O.kwords(k)])


def test_overflow_reports_the_need(capi):
    k, P, n = 31, 64, 200
    kmers = DP.kmers_from_syms(DP.random_syms(9, n, k), k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    e = _refused(capi, capi.host_anchor_dict_encode_pieces, kmers, k, P, out_cap=len(stream) - 1)
    assert e.code == -5 and "out_cap too small" in str(e) and e.size == len(stream) and np.array_equal(e.piece_off, off)
    assert capi.host_anchor_dict_encode_pieces(kmers, k, P, out_cap=len(stream))[0] == stream


def test_refusals_with_their_words(capi):
    k, P, n = 31, 4, 10
    kmers = DP.kmers_from_syms(DP.random_syms(3, n, k), k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    out = np.full(n, 0xABCD, dtype=np.uint64)
    dec = capi.host_anchor_dict_decode_pieces
    for kk in (0, 64):
        assert "kmer_size must be in 1..63" in str(_refused(capi, capi.host_anchor_dict_encode_pieces, kmers, kk, P))
        assert "kmer_size must be in 1..63" in str(_refused(capi, dec, stream, off, n, kk, P, out=out))
    assert "piece_anchors must be in 1..2^20" in str(_refused(capi, capi.host_anchor_dict_encode_pieces, kmers, k, (1 << 20) + 1))
    assert "piece_anchors must be in 1..2^20" in str(_refused(capi, dec, stream, off, n, k, (1 << 20) + 1, out=out))
    for args in ((n + P, k, P), (n, k, P + 1), (n, k, P - 1)):                                   # ceil(n_anchors / P) is not the table's count
        e = _refused(capi, dec, stream, off, *args, out=np.zeros(2 * n, np.uint64))
        assert e.code == -1 and str(e).endswith("piece table does not match the anchor count")
    e = _refused(capi, dec, stream, off[:-1], n, k, P, out=out)
    assert str(e).endswith("piece table does not match the anchor count")
    back = off.copy()
    back[1], back[2] = off[2], off[1]
    e = _refused(capi, dec, stream, back, n, k, P, out=out)
    assert e.code == -1 and str(e).endswith("piece offsets run backwards")
    lib = capi.load_library()
    assert lib.leon_host_anchor_dict_decode_pieces(None, None, 0, 0, k, P, None, 0) == -1
    assert b"null argument" in lib.leon_last_error(None)
    assert lib.leon_host_anchor_dict_encode_pieces(None, 0, k, P, None, 0, None, None, 0) == -1
    assert b"null argument" in lib.leon_last_error(None)
    assert np.all(out == 0xABCD)
    # no anchors: no piece, an empty stream, and it decodes
    s0, o0 = capi.host_anchor_dict_encode_pieces(np.zeros(0, np.uint64), k, P)
    assert s0 == b"" and o0.tolist() == [0]
    assert len(capi.host_anchor_dict_decode_pieces(b"", o0, 0, k, P)) == 0


def test_corrupted_pieces_on_the_host(capi):
    """a corrupted piece is refused by name -- the smallest one -- and the output is left alone; what still decodes, decodes to other k-mers"""
    k, P, n = 31, 40, 5 * 40 + 2
    kmers = DP.kmers_from_syms(DP.random_syms(21, n, k), k)
    stream, off = capi.host_anchor_dict_encode_pieces(kmers, k, P)
    failed = 0
    for name, (s, o) in DP.corruptions(stream, off).items():
        code, msg, out = DP.verdict(capi, capi.host_anchor_dict_decode_pieces, s, o, n, k, P)
        if code:
            failed += 1
            assert code == -1 and "anchor dictionary piece " in msg and msg.endswith(" does not decode"), (name, msg)
            assert np.all(out == 0x5EED), name
            # the piece named is the smallest the oracle's decoder... (the reference ignores failures: the host's own single-piece decode says which)
            bad = int(msg.split("piece ")[1].split(" ")[0])
            for p in range(bad + 1):
                a, b = p * P, min(n, (p + 1) * P)
                one = DP.verdict(capi, capi.host_anchor_dict_decode_pieces, s[int(o[p]):int(o[p + 1])], np.array([0, int(o[p + 1] - o[p])], np.uint64), b - a, k, P)
                assert (one[0] != 0) == (p == bad), (name, p)
        else:
            assert not np.array_equal(out, kmers), name
    assert failed >= 2


def test_create_refuses_the_flag_combinations(capi):
    """leon_dna_ctx_create's refusals come before a device is looked for"""
    import leon_amd
    for kw, words in ((dict(dict_pieces=True, dict_on_device=True), "exclude each other"),
                      (dict(dict_piece_anchors=7), "dict_piece_anchors needs LEON_F_DICT_PIECES"),
                      (dict(dict_pieces=True, dict_piece_anchors=(1 << 20) + 1), "dict_piece_anchors must be in 1..2^20")):
        e = _refused(capi, leon_amd.DnaEncodeContext, kmer_size=31, bloom_tai=1000, **kw)
        assert e.code == -1 and words in str(e), kw


@pytest.mark.parametrize("sanitize", [False, True])
def test_dict_pieces_selftest(tmp_path, sanitize):
    """tests/dict_pieces_selftest.cpp includes host_dict_pieces.h alone: plain, and under AddressSanitizer and UndefinedBehaviorSanitizer with
    their runtimes linked statically; run as a child process, nothing of it is loaded into Python"""
    exe = str(tmp_path / "dict_pieces_selftest")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
             "-static-libubsan"] if sanitize else ["-O2"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-pthread", "-o", exe, os.path.join(ROOT, "tests", "dict_pieces_selftest.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LEON_CHAIN_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith("dict pieces selftest: ok")


@pytest.mark.parametrize("sanitize", [False, True])
def test_piece_table_validators_stand_alone(tmp_path, sanitize):
    """tests/dict_pieces_plan_check.cpp: leon_plan.hpp's check of the container's piece table (what `leon -d` refuses before a device is asked),
    every rule broken one at a time"""
    exe = str(tmp_path / "dict_pieces_plan_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
             "-static-libubsan"] if sanitize else ["-O2"]
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"), "-o", exe,
                            os.path.join(ROOT, "tests", "dict_pieces_plan_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "dict_pieces_plan_check: ok, " in run.stdout
