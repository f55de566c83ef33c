"""The anchor dictionary in independently coded pieces (k_dict_encode_pieces, k_dict_decode_pieces; LEON_F_DICT_PIECES, `leon -c -dict-pieces`;
DESIGN.md 4.4).  bench.py's `value` keeps measuring the default path; this script measures the option beside it.

  dict_pieces.py --step [N]            bench.py's encode step on N synthetic reads x 150 bp (default 100 M) through two contexts on the same
                                       resident reads, LEON_F_DICT_PIECES off, on, off, ... alternating, three each after one warm-up each:
                                       ms_total, ms_anchor_wait, the finish call's wall time and the step's wall time, the two streams' sizes.
                                       LEON_LIB=<another build's libleon_dna.so> (the parent commit's: the yardstick) runs the flag-off
                                       steps alone on that library; --off-only does the same on this one (one context, three steps in a row)
  dict_pieces.py --kernel [A]          A random anchors (default 14 M), k = 31, P = 1024: one warm-up and two calls each of
                                       leon_anchor_dict_encode_pieces_device and leon_anchor_dict_decode_pieces_device -- the run to put under
                                       `rocprofv3 --kernel-trace --stats` (kernel times come from there; the JSON line has the calls' wall
                                       times, copies included), and the host twins on all CPUs beside them
  dict_pieces.py --cli N --parent LEON `leon -c -lossless` with and without -dict-pieces and the parent commit's, then `leon -d` of the
                                       containers (the parent's on its own), on an N-read 150 bp FASTQ in a RAM-backed directory, alternating,
                                       three each; the dictionary datasets' sizes
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import leon_amd  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--step", type=int, nargs="?", const=100_000_000, default=0)
ap.add_argument("--off-only", action="store_true", help="--step: the flag-off steps alone, as a library from before the option runs them")
ap.add_argument("--kernel", type=int, nargs="?", const=14_000_000, default=0)
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_dict_pieces")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
OTHER_LIB = os.environ.get("LEON_LIB")
NEW = ("leon_dna_dict_pieces", "leon_anchor_dict_encode_pieces_device", "leon_anchor_dict_decode_pieces_device", "leon_host_anchor_dict_encode_pieces",
       "leon_host_anchor_dict_decode_pieces")
if OTHER_LIB:                                                     # a build from before the pieces: bind what it has
    capi.lib_path = lambda: OTHER_LIB
    for name in NEW:
        capi._EXPORTS.pop(name, None)
K, RPB, L = bench.K, bench.RPB, bench.L


def step():
    n = (args.step // RPB) * RPB or RPB
    G = max(n * L // 30, 10 * L)
    genome = bench.gen_genome(G, dev)
    reads = torch.empty((n, L), dtype=torch.uint8, device=dev)
    for c0 in range(0, (n + bench.CHUNK - 1) // bench.CHUNK):
        lo, hi = c0 * bench.CHUNK, min(n, (c0 + 1) * bench.CHUNK)
        reads[lo:hi] = bench.gen_reads_chunk(genome, c0, bench.CHUNK, 0.01, dev)[:hi - lo]
    del genome
    offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L).contiguous()
    torch.cuda.synchronize()
    d_solid, n_solid = capi.kmer_solid_device(reads.data_ptr(), offsets.data_ptr(), n, K, bench.ABUNDANCE, device_id=0)
    ways = ["off"] if OTHER_LIB or args.off_only else ["off", "on"]
    ctx = {}
    for w in ways:
        ctx[w] = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=RPB, bloom_tai=n_solid * bench.BITS_PER_KMER, bloom_n_hash=bench.N_HASH, device_id=0,
                                           **({"dict_pieces": True} if w == "on" else {}))
        ctx[w].reserve(n, n * L)
        ctx[w].bloom_insert_device(d_solid, n_solid)
    capi.device_free(d_solid)
    cb = capi.SINK(lambda user, block_id, p, size, n_reads: 0)

    def one(w):
        c = ctx[w]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.reset_stream()
        c.encode_batch_device(reads.data_ptr(), offsets.data_ptr(), n, sink=cb)
        st = c.stats()
        t1 = time.perf_counter()
        size, n_anchors = c.finish(copy=False)
        t2 = time.perf_counter()
        return {"ms_total": round(st["ms_total"], 2), "ms_anchor_wait": round(c.stats()["ms_anchor_wait"], 2), "finish_call_ms": round((t2 - t1) * 1e3, 2),
                "step_wall_ms": round((t2 - t0) * 1e3, 2), "dict_bytes": size, "n_anchors": n_anchors}
    for w in ways:
        one(w)                                                   # warm-up: code objects, buffers
    runs = {w: [] for w in ways}
    for _ in range(3):
        for w in ways:
            runs[w].append(one(w))
            print(w, runs[w][-1], file=sys.stderr, flush=True)
    print(json.dumps({"mode": "step", "reads": n, "library": OTHER_LIB or capi.lib_path(), "cpus": len(os.sched_getaffinity(0)), "runs": runs}))


def kernel():
    A, P = args.kernel, 1024
    rng = np.random.default_rng(5)
    kmers = rng.integers(0, 1 << 62, A, dtype=np.uint64)
    d = torch.from_numpy(kmers.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    out = {"mode": "kernel", "anchors": A, "k": K, "piece_anchors": P, "pieces": capi.dict_piece_count(A, P), "cpus": len(os.sched_getaffinity(0))}
    capi.anchor_dict_encode_pieces_device(d.data_ptr(), min(A, 4 * P), K, P)
    enc, dec = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        stream, off = capi.anchor_dict_encode_pieces_device(d.data_ptr(), A, K, P, out_cap=A * K // 3 + 64)
        enc.append(round((time.perf_counter() - t0) * 1e3, 2))
    capi.anchor_dict_decode_pieces_device(stream[:int(off[4])], off[:5], min(A, 4 * P), K, P) if A >= 4 * P else None
    for _ in range(2):
        t0 = time.perf_counter()
        back = capi.anchor_dict_decode_pieces_device(stream, off, A, K, P)
        dec.append(round((time.perf_counter() - t0) * 1e3, 2))
    assert np.array_equal(back, kmers)
    t0 = time.perf_counter()
    h_stream, h_off = capi.host_anchor_dict_encode_pieces(kmers, K, P, out_cap=A * K // 3 + 64)
    t1 = time.perf_counter()
    h_back = capi.host_anchor_dict_decode_pieces(h_stream, h_off, A, K, P)
    t2 = time.perf_counter()
    assert h_stream == stream and np.array_equal(h_back, kmers)
    t3 = time.perf_counter()
    single = capi.host_anchor_dict_encode(kmers, K)
    t4 = time.perf_counter()
    out.update({"device_encode_call_ms": enc, "device_decode_call_ms": dec, "host_twin_encode_ms": round((t1 - t0) * 1e3, 1), "host_twin_decode_ms": round((t2 - t1) * 1e3, 1),
                "pieced_bytes": len(stream), "single_stream_bytes": len(single), "single_stream_host_chain_ms": round((t4 - t3) * 1e3, 1),
                "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process"})
    print(json.dumps(out))


def cli():
    N = args.cli
    assert args.parent, "--cli needs --parent: the parent commit's leon"
    os.makedirs(args.dir, exist_ok=True)
    fq = os.path.join(args.dir, "reads.fastq")
    bench.write_fastq(fq, N, L, dev)
    torch.cuda.empty_cache()
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    out = {"mode": "cli", "reads": N, "blocks": (N + RPB - 1) // RPB, "fastq_bytes": os.path.getsize(fq), "cpus": len(os.sched_getaffinity(0))}

    def timed(cmd):
        t = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stdout[-400:], r.stderr[-400:])
        return round(time.time() - t, 2), r.stdout
    ways = [("plain", leon, []), ("pieces", leon, ["-dict-pieces"]), ("parent", args.parent, [])]
    c_s, d_s, lines = {w: [] for w, _, _ in ways}, {w: [] for w, _, _ in ways}, {}
    for rep in range(3):
        for w, binary, opts in ways:
            s, log = timed([binary, "-file", fq, "-c", "-lossless", "-verbose", "1"] + opts)
            c_s[w].append(s)
            os.replace(fq + ".leon", os.path.join(args.dir, w + ".fastq.leon"))
            if rep == 0:
                lines[w + " -c"] = [l for l in log.splitlines() if l.startswith(("time:", "dictionary:", "DNA stream:"))]
            print("compress %s: %.2f s" % (w, s), file=sys.stderr, flush=True)
    for rep in range(3):
        for w, binary, opts in ways:
            s, log = timed([binary, "-file", os.path.join(args.dir, w + ".fastq.leon"), "-d", "-verbose", "1"])
            d_s[w].append(s)
            os.remove(os.path.join(args.dir, w + ".fastq.d"))
            if rep == 0:
                lines[w + " -d"] = [l for l in log.splitlines() if l.startswith(("time:", "dictionary:"))]
            print("decompress %s: %.2f s" % (w, s), file=sys.stderr, flush=True)
    sizes = {w: os.path.getsize(os.path.join(args.dir, w + ".fastq.leon")) for w, _, _ in ways}
    r = subprocess.run([args.parent, "-file", os.path.join(args.dir, "pieces.fastq.leon"), "-d"], capture_output=True, text=True)
    out.update({"compress_s": c_s, "decompress_s": d_s, "container_bytes": sizes, "verbose": lines,
                "parent_on_a_pieced_container": {"status": r.returncode, "stderr": r.stderr.strip()[-300:]}})
    for f in os.listdir(args.dir):
        os.remove(os.path.join(args.dir, f))
    print(json.dumps(out))


step() if args.step else kernel() if args.kernel else cli()
