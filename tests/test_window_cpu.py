"""CPU tests (no GPU): synth.window_reads, the generator of tests/test_gpu_window.py's 2.3 M-read inputs, and the golden file those are
checked against (tests/golden/self_golden_window.json).  A read range regenerated on its own must equal the same slice of the whole file
at any thread count, and the first and last block of every golden case must still be what the oracle encoded: numpy's streams drifting
under the golden shows here, in seconds, instead of as a failure of the GPU suite."""
import copy
import json

import numpy as np
import pytest

import make_golden_window as W
import synth

GOLD = json.load(open(W.PATH))


def _small(spec, n=200000):
    s = copy.deepcopy(spec)
    s["n_reads"] = n
    s["genome"]["length"] = max(20000, s["genome"]["length"] * n // spec["n_reads"])
    return s


def test_window_reads_slices_equal_the_whole():
    # the pairs63 spec at 200 000 reads: ragged reads, mates, skew, a structured genome (placement is drawn for the whole file in every
    # order alike; the other cases' streams are pinned by their golden blocks below)
    spec = _small(next(c for c in GOLD["cases"] if c["id"] == "pairs63")["spec"])
    bases, off = synth.window_reads(spec, threads=4)
    n = spec["n_reads"]
    assert len(off) == n + 1 and off[0] == 0 and int(off[-1]) == len(bases)
    lens = np.diff(off.astype(np.int64))
    assert lens.max() <= spec["read_len"] and (lens.min() < spec["read_len"]) == bool(spec.get("ragged"))
    assert set(np.unique(bases).tolist()) <= set(b"ACGTN")
    C = synth.WINDOW_CHUNK
    # off chunk boundaries, across them, the file's end, empty ranges; one thread and several (the whole file: four)
    for r0, r1, threads in ((0, 1, 1), (C - 7, C + 9, 1), (12345, 2 * C + 1, 3), (n - 1000, n, 2), (n, n, 1), (77, 77, 1)):
        b, o = synth.window_reads(spec, r0, r1, threads=threads)
        assert np.array_equal(o, off[r0:r1 + 1] - off[r0]), (r0, r1)
        assert np.array_equal(b, bases[int(off[r0]):int(off[r1])]), (r0, r1)


def test_window_reads_noise_rates():
    # substitutions and N at the rates asked for, a substitution never the base it replaces
    spec = _small(GOLD["cases"][0]["spec"], 50000)
    spec.update(err=0.02, n_rate=0.005)
    noisy, off = synth.window_reads(spec)
    clean, off0 = synth.window_reads(dict(spec, err=0, n_rate=0))
    assert np.array_equal(off, off0) and not (clean == ord("N")).any()
    n_sub, n_n = ((noisy != clean) & (noisy != ord("N"))).mean(), (noisy == ord("N")).mean()
    assert abs(n_sub - 0.02) < 0.001 and abs(n_n - 0.005) < 0.0005, (n_sub, n_n)


@pytest.mark.parametrize("cid", [c["id"] for c in GOLD["cases"]])
def test_first_and_last_block_inputs_equal_the_golden(cid):
    case = next(c for c in GOLD["cases"] if c["id"] == cid)
    for blk in (case["blocks"][0], case["blocks"][-1]):
        r0, r1 = blk["reads"]
        bases, off = synth.window_reads(case["spec"], r0, r1)
        assert W.input_digests(bases, off) == (blk["bases_sha256"], blk["offsets_sha256"]), \
            "generator drift in %s, reads [%d, %d): regenerate with python tests/make_golden_window.py" % (cid, r0, r1)


def test_golden_file_is_consistent():
    assert "SELF-golden" in GOLD["_note"]
    assert [c["id"] for c in GOLD["cases"]] == ["random", "sorted", "pairs63"]
    for case in GOLD["cases"]:
        n, rpb = case["n_reads"], case["reads_per_block"]
        assert n == case["spec"]["n_reads"] > W.FIRST_WINDOW + W.WINDOW and rpb == W.RPB and case["min_abundance"] == 3
        assert len(case["blocks"]) == (n + rpb - 1) // rpb and sum(b["n_reads"] for b in case["blocks"]) == n
        assert [b["reads"] for b in case["blocks"]] == [list(W.block_range(i, n)) for i in range(len(case["blocks"]))]
        assert all(b["windows"] == [W.window_of(b["reads"][0]), W.window_of(b["reads"][1] - 1)] for b in case["blocks"])
        # blocks in the short first window, across each hand-over, inside the full window, in the short last one
        assert case["n_windows"] == 3 and {tuple(b["windows"]) for b in case["blocks"]} == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)}
        assert case["bloom_tai"] == max(case["n_solid"] * 12, 1000)
        assert case["max_addr_delta"] == max(b["max_addr_delta"] for b in case["blocks"])
        assert all(b["n_anchored"] <= b["n_reads"] for b in case["blocks"]) and case["n_anchors"] <= sum(b["n_anchored"] for b in case["blocks"])
        if case["id"] != "sorted":
            assert case["n_anchors"] > 65536 and case["max_addr_delta"] >= 65536      # what the case is there for: 3-byte address numerics
    assert GOLD["cases"][2]["k"] > 32                                                 # two-word k-mers


def test_max_addr_delta_is_the_coded_value():
    # getDeltaValue: the delta to the previous anchored read's address when it is smaller than the address itself, else the address
    pos = np.array([3, -1, 0, 5, 2, 1], dtype=np.int32)
    addr = np.array([70000, 99, 69990, 10, 200000, 200001], dtype=np.uint32)
    assert W.max_addr_delta(pos, addr) == 199990                   # 70000 (the first: raw), 10, 10 (raw: 69980 > 10), 199990, 1
    assert W.max_addr_delta(pos[:4], addr[:4]) == 70000
    assert W.max_addr_delta(pos[4:], addr[4:]) == 200000
    assert W.max_addr_delta(pos[1:2], addr[1:2]) == 0
