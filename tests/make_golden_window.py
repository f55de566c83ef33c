"""Generates tests/golden/self_golden_window.json: SELF-golden digests of the CPU restatement (oracle/leon_oracle.c) encoding inputs of
2.3 M reads -- a short first resolution window (2^17 reads), one full default window (2^21) and a short last one, in 46 blocks of
50 000 reads.  They are NOT reference Leon output.  The oracle takes minutes and ~9 GB per case here, too much for the GPU suite, so this
file freezes what it computed; tests/test_gpu_window.py regenerates the reads (synth.window_reads) and checks the HIP path against it,
block by block and stage by stage.

    python tests/make_golden_window.py [--jobs N]      # write the file (one process per case)
    python tests/make_golden_window.py --check         # recompute everything and compare with the committed file, writing nothing"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

PATH = os.path.join(HERE, "golden", "self_golden_window.json")
RPB = 50000                 # bench.RPB
MIN_ABUNDANCE = 3
FIRST_WINDOW, WINDOW = 1 << 17, 1 << 21      # capi.hip: first_window(), the default resolve_window
N_READS = 2300000

CASES = [
    # the bench's shape: i.i.d. genome, reads at random places in random order; ~338 k anchors: in-block address deltas past 65 535
    {"id": "random", "k": 31,
     "spec": {"genome": {"kind": "iid", "length": 11500000, "seed": 301}, "n_reads": N_READS, "read_len": 150, "seed": 302,
              "order": "random", "err": 0.01, "n_rate": 0.001}},
    # position-sorted reads over a genome with repeats and microsatellites, PCR duplicates: most of a window left to the sequential pass
    {"id": "sorted", "k": 31,
     "spec": {"genome": {"kind": "structured", "length": 11500000, "seed": 311, "dispersed": 400, "tandem": 4000},
              "n_reads": N_READS, "read_len": 150, "seed": 312, "order": "sorted", "err": 0.01, "n_rate": 0.001, "dup_rate": 0.1}},
    # interleaved mates, ragged reads (62 .. 250 bp: some shorter than k), coverage skew, two-word k-mers
    {"id": "pairs63", "k": 63,
     "spec": {"genome": {"kind": "structured", "length": 12000000, "seed": 321, "dispersed": 400, "tandem": 4000},
              "n_reads": N_READS, "read_len": 250, "ragged": True, "seed": 322, "order": "pairs", "err": 0.01, "n_rate": 0.001,
              "skew": 0.3}},
]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def window_of(r):
    """the resolution window read r of a one-batch encode lies in"""
    return 0 if r < FIRST_WINDOW else 1 + (r - FIRST_WINDOW) // WINDOW


def block_range(b, n):
    return b * RPB, min(n, (b + 1) * RPB)


def input_digests(bases, off):
    """sha256 of a block's bases and of its offsets (from 0)"""
    o = np.asarray(off, dtype=np.uint64)
    return sha(bases[int(o[0]):int(o[-1])]), sha((o - o[0]).astype("<u8").tobytes())


def solid_digest(solid, k):
    """sha256 of the solid k-mers in sorted order (the counters' own orders differ)"""
    a = np.asarray(solid, dtype=np.uint64).reshape(-1, 2 if k >= 32 else 1)
    a = a[np.lexsort(a.T[::-1])]                     # by the first word, then the second
    return sha(a.astype("<u8").tobytes())


def anchor_digests(pos, addr, flags):
    """a block's anchor trace: positions as they are, addresses and flags where the read has an anchor (0 elsewhere)"""
    anchored = pos >= 0
    return (sha(pos.astype("<i4").tobytes()), sha(np.where(anchored, addr, 0).astype("<u4").tobytes()),
            sha(np.where(anchored, flags, 0).astype(np.uint8).tobytes()))


def max_addr_delta(pos, addr):
    """the largest anchor-address value a block codes (getDeltaValue: min(|a - previous a|, a), the previous one 0 at the block's
    start): from 65 536 on, encodeNumeric writes a third byte"""
    a = addr[pos >= 0].astype(np.int64)
    if len(a) == 0:
        return 0
    prev = np.concatenate([[0], a[:-1]])
    return int(np.minimum(np.abs(a - prev), a).max())


def run_case(case):
    import common
    import oracle_lib as O
    t0 = time.time()
    k, spec = case["k"], case["spec"]
    bases, off = synth.window_reads(spec)
    n = len(off) - 1
    raw = bases.tobytes()
    t1 = time.time()
    bl, solid, tai = common.make_bloom(raw, off, k, MIN_ABUNDANCE)
    t2 = time.time()
    res = O.encode(raw, off, k, RPB, bl)
    t3 = time.time()
    pos, addr, flags, ev = res.anchor_pos, res.anchor_addr, res.flags, res.events
    blocks = []
    for b in range(len(res.blocks)):
        r0, r1 = block_range(b, n)
        o0, o1 = int(off[r0]), int(off[r1])
        in_b, in_o = input_digests(bases, off[r0:r1 + 1])
        p, a, f = anchor_digests(pos[r0:r1], addr[r0:r1], flags[r0:r1])
        blocks.append({"reads": [r0, r1], "windows": [window_of(r0), window_of(r1 - 1)], "bases_sha256": in_b, "offsets_sha256": in_o,
                       "n_reads": res.block_nreads[b], "size": len(res.blocks[b]), "payload_sha256": sha(res.blocks[b]),
                       "anchor_pos_sha256": p, "anchor_addr_sha256": a, "flags_sha256": f, "events_sha256": sha(ev[o0:o1]),
                       "n_anchored": int((pos[r0:r1] >= 0).sum()), "max_addr_delta": max_addr_delta(pos[r0:r1], addr[r0:r1])})
    out = {"id": case["id"], "spec": spec, "k": k, "reads_per_block": RPB, "min_abundance": MIN_ABUNDANCE, "n_reads": n,
           "n_bases": len(bases), "n_solid": len(solid) // O.kwords(k), "solid_sha256": solid_digest(solid, k), "bloom_tai": tai,
           "bloom_sha256": sha(bl.bits.tobytes()), "n_anchors": res.n_anchors, "anchor_kmers_sha256": sha(res.anchor_kmers.astype("<u8").tobytes()),
           "anchor_dict_sha256": sha(res.anchor_dict), "anchor_dict_bytes": len(res.anchor_dict), "n_symbols": res.n_symbols,
           "n_windows": window_of(n - 1) + 1, "max_addr_delta": max(b["max_addr_delta"] for b in blocks), "blocks": blocks}
    print("%-8s %d reads, %d blocks, %d solid, %d anchors, largest address delta %d: reads %.0f s, count + bloom %.0f s, encode %.0f s"
          % (case["id"], n, len(blocks), out["n_solid"], res.n_anchors, out["max_addr_delta"], t1 - t0, t2 - t1, t3 - t2), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed file; write nothing")
    ap.add_argument("--jobs", type=int, default=1, help="cases computed at once, one process each (~9 GB apiece)")
    ap.add_argument("--case", action="append", help="only this case (with --check)")
    args = ap.parse_args()
    cases = [c for c in CASES if not args.case or c["id"] in args.case]
    if args.jobs > 1:
        from concurrent.futures import ProcessPoolExecutor
        with ProcessPoolExecutor(min(args.jobs, len(cases))) as ex:
            got = list(ex.map(run_case, cases))
    else:
        got = [run_case(c) for c in cases]
    if args.check:
        want = {c["id"]: c for c in json.load(open(PATH))["cases"]}
        bad = [g["id"] for g in got if want.get(g["id"]) != g]
        for i in bad:
            w, g = want.get(i) or {}, next(x for x in got if x["id"] == i)
            print("MISMATCH %s: %s" % (i, sorted(key for key in set(w) | set(g) if w.get(key) != g.get(key))))
        print("check %s" % ("FAILED" if bad else "ok: %d cases equal %s" % (len(got), os.path.relpath(PATH))))
        sys.exit(1 if bad else 0)
    assert not args.case, "--case only with --check: the file holds every case"
    out = {"_note": "SELF-golden digests of oracle/leon_oracle.c over synth.window_reads inputs (parity with reference Leon is "
                    "UNPINNED).  Re-run: python tests/make_golden_window.py", "cases": got}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", PATH)


if __name__ == "__main__":
    main()
