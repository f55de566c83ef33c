"""No GPU: (1) the directed streams of tests/rc_edges.py hold the events they are built for -- certified by the reference's own per-step
record (lo_rc_profile_stream), never by the code under test -- and the oracle's decoder gives them back; (2) the host chains
(leon_amd/csrc/host_blocks.h: HostBlockCoder::code and code2) code them to the oracle's bytes, in a stand-alone program
(tests/host_blocks_check.cpp) that makes its records itself, built plain and with AddressSanitizer + UBSan.
tests/test_gpu_rc_edges.py runs the same streams through the device's coder, the host chains behind k_rc_records, and the decoders."""
import os
import subprocess

import numpy as np
import pytest

import many_blocks as MB
import oracle_lib as O
import rc_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_is_the_encoder_step_by_step():
    """lo_rc_profile_stream: the bytes of lo_rc_encode_stream, and a per-step record that adds up to them"""
    cases = [MB.rc_stream(b) for b in range(0, 64)] + [E.streams()[n] for n in ("strike17", "resets", "resets5", "pair_b")]
    for m, v in cases:
        p = O.rc_profile_stream(m, v, E.MODEL_SIZES)
        assert p.payload == O.rc_encode_stream(m, v, E.MODEL_SIZES)
        assert len(p.n_bytes) == len(m) and int(p.n_bytes.sum()) + 8 == len(p.payload)       # + the flush
        assert set(np.unique(p.reset).tolist()) <= {0, 1}
        # a model's total before a step: its alphabet size + the symbols coded on it so far
        seen = np.zeros(E.N_MODELS, dtype=np.int64)
        for i in list(range(min(len(m), 300))):
            assert p.total[i] == E.MODEL_SIZES[m[i]] + seen[m[i]]
            seen[m[i]] += 1
    for name, model in (("strike20", E.PM), ("strike20_small", E.PM_SMALL)):                   # ... and far into a stream
        m, v = E.streams()[name]
        p = E.profiles()[name]
        at = np.nonzero(m == model)[0]
        assert np.array_equal(p.total[at], E.MODEL_SIZES[model] + np.arange(len(at)))


def test_census():
    S, P = E.streams(), E.profiles()
    assert tuple(S) == E.NAMES
    for name in E.NAMES:
        m, v = S[name]
        p = P[name]
        cs = E.census(name)
        print("%-14s %8d symbols, largest total %8d, steps by (bytes, reset): %s" % (
            name, len(m), int(p.total.max()), ", ".join("%r: %d" % kv for kv in sorted(cs.items()))))
        want = E.CENSUS[name]
        assert m.max() < E.N_MODELS and np.all(v.astype(np.int64) < np.array(E.MODEL_SIZES)[m])
        assert len(m) == want.get("length", len(m))
        if "length" not in want:
            assert len(m) <= E.MAX_LEN
        big, resets = E.big_steps(name), E.reset_steps(name)
        on_pm = big[m[big] == want.get("pm", E.PM)]
        assert len(on_pm) >= want.get("big", 0), (name, len(on_pm))
        if "big_total" in want:
            assert len(on_pm) and int(p.total[on_pm].min()) >= want["big_total"], name
        for lane in want.get("lanes", ()):
            assert np.any(big % 64 == lane), (name, lane)
        assert len(resets) >= want.get("resets", 0), (name, len(resets))
        for lane in want.get("reset_lanes", ()):
            assert np.any(resets % 64 == lane), (name, lane)
        assert cs[(5, 1)] >= want.get("reset5", 0) and cs[(6, 1)] >= want.get("reset6", 0), name
        if want.get("last") == "big":
            assert big[-1] == len(m) - 1, name
        if want.get("last") == "reset":
            assert resets[-1] == len(m) - 1, name
        if "tail" in want:                                          # the strikes at the full total are the stream's last symbols
            assert int((big >= len(m) - want["tail"]).sum()) >= want["big"], name
        assert np.array_equal(O.rc_decode_stream(p.payload, m, E.MODEL_SIZES), v), name
    # the 22-bit records: one numeric model, freq towards 2^21, then cumLow >= 2^21 and cumLow + freq up to the total, just below 2^22
    for name in ("pack22_host", "pack22_device"):
        m, v = S[name]
        half, tail = E.PACK22_HOST_LEN // 2, E.PACK22_HOST_LEN - 2000
        assert np.all(m == E.PM) and np.all(v[:half] == 0) and np.all(v[half:tail] == 255)
        assert (1 << 22) - 1024 < int(P[name].total.max()) < (1 << 22)
    assert len(S["pack22_host"][0]) + 1024 < (1 << 22) <= len(S["pack22_device"][0]) + 1024      # either side of the hand-over
    assert np.array_equal(S["pack22_device"][0][:-1], S["pack22_host"][0]) and np.array_equal(S["pack22_device"][1][:-1], S["pack22_host"][1])
    # the pair: rare steps (>= 4 bytes, or a reset) at the same step index in both, and in one alone
    assert len(S["pair_a"][0]) == len(S["pair_b"][0])
    ra, rb = set(E.rare_steps("pair_a").tolist()), set(E.rare_steps("pair_b").tolist())
    print("pair: %d rare steps in both, %d in pair_a alone, %d in pair_b alone" % (len(ra & rb), len(ra - rb), len(rb - ra)))
    assert len(ra & rb) >= E.PAIR_SHARED and len(ra - rb) >= E.PAIR_ONLY and len(rb - ra) >= E.PAIR_ONLY


def _lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rc_edges")
    (d / "sizes").write_bytes(bytes(s & 255 for s in E.MODEL_SIZES))
    want = E.want()
    for name, (m, v) in E.streams().items():
        (d / (name + ".sym")).write_bytes(np.stack([m, v], axis=1).tobytes())
        (d / (name + ".pay")).write_bytes(want[name])
    return d


_RUNS = ["one:" + n for n in E.NAMES if n != "pack22_device"] + ["pair:pair_a,resets", "pair:pack22_host,strike17", "pair:pair_a,pair_b",
                                                                     "pair:resets5,strike20_small"]


@pytest.mark.parametrize("san", ["plain", "address,undefined"])
def test_host_chains_stand_alone(tmp_path, stream_files, san):
    """HostBlockCoder::code in 1, 16 and 64 pieces and code2 on pairs of unequal length, records made from plain models: the oracle's bytes.
    Under ASan/UBSan this is also the growth rule of out_ (8 bytes a step and 64, per 4096 steps) against steps that emit 6 bytes."""
    flags = ["-O2"]
    if san != "plain":
        if not _lib("libasan.so") or not _lib("libubsan.so"):
            pytest.skip("no libasan / libubsan in this toolchain")
        flags = ["-O1", "-g", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    exe = str(tmp_path / "host_blocks_check")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_blocks_check.cpp"), "-lpthread"])
    r = subprocess.run([exe, str(stream_files)] + _RUNS, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "host_blocks_check: ok, %d runs" % len(_RUNS) in r.stdout
    print(r.stdout.strip())
