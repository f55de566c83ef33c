"""Block checksums (k_crc32_tiles, k_crc32_final; `leon -c -checksum`, verified by `leon -d`) against zlib's crc32 on the host threads.

  checksum.py --kernel N [--block-bytes B]  N random bytes in device memory, cut into segments of B bytes (default 7 500 000: a block of
                                          50 000 reads x 150): one warm-up call of leon_crc32_segments_device on the first segment and TWO
                                          whole calls, the words compared with leon_host_crc32_segments on the same bytes with 16 threads in
                                          the same run (two calls, timed) and, for the first four segments, with Python's zlib.crc32.  The run
                                          to put under `rocprofv3 --kernel-trace --stats` (kernel times come from there; the JSON line carries
                                          the calls' wall times); bytes / k_crc32_tiles' time is to be read against the float4 copy measured on
                                          this chip, 6.29 TB/s
  checksum.py --cli N --parent LEON         `leon -c -lossless` and `leon -d` on an N-read 150 bp FASTQ in a RAM-backed directory, with and
                                          without the table, alternating with the parent commit's binary (which knows no -checksum and reads
                                          the container written without it), three each; -d under -header-text device -record-text device
                                          -qual-inflate device (every digest on the device) and once on the host threads
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, default=0)
ap.add_argument("--block-bytes", type=int, default=7500000)
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_checksum")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
L, THREADS = 150, 16
COPY_TBS = 6.29                                                   # the float4 copy on this chip


def kernel():
    N, B = args.kernel, args.block_bytes
    g = torch.Generator(device=dev); g.manual_seed(13)
    d = torch.empty(N + 64, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for a in range(0, N, step):
        m = min(step, N - a)
        d[a:a + m] = torch.randint(0, 256, (m,), device=dev, generator=g, dtype=torch.uint8)
    torch.cuda.synchronize()
    off = np.append(np.arange(0, N, B, dtype=np.uint64), np.uint64(N))
    n_seg = len(off) - 1
    capi.crc32_segments_device(d.data_ptr(), N, off[:2])          # (code object loaded)
    ms, words = [], None
    for _ in range(2):
        t0 = time.perf_counter()
        words = capi.crc32_segments_device(d.data_ptr(), N, off)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    h = d[:N].cpu().numpy()
    host_ms, host_words = [], None
    for _ in range(2):
        t0 = time.perf_counter()
        host_words = capi.host_crc32_segments(h, off, n_threads=THREADS)
        host_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    pinned = [zlib.crc32(h[int(off[s]):int(off[s + 1])]) for s in range(min(n_seg, 4))]
    print(json.dumps({"bytes": N, "segments": n_seg, "segment_bytes": B, "host_threads": THREADS,
                      "leon_crc32_segments_device_ms": ms, "leon_host_crc32_segments_ms": host_ms,
                      "device_equals_host": bool(np.array_equal(words, host_words)), "first_segments_equal_zlib": host_words[:len(pinned)].tolist() == pinned,
                      "float4_copy_tb_s": COPY_TBS,
                      "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process; bytes / k_crc32_tiles' time against float4_copy_tb_s"}))


def cli():
    N = args.cli
    assert args.parent, "--cli needs --parent: the parent commit's leon"
    os.makedirs(args.dir, exist_ok=True)
    fq = os.path.join(args.dir, "reads.fastq")
    bench.write_fastq(fq, N, L, dev)
    torch.cuda.empty_cache()
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    out = {"reads": N, "fastq_bytes": os.path.getsize(fq), "cpus": len(os.sched_getaffinity(0))}
    device = ["-header-text", "device", "-record-text", "device", "-qual-inflate", "device"]

    def timed(cmd):
        t = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stdout[-400:], r.stderr[-400:])
        return round(time.time() - t, 2), r.stdout

    # -c -lossless: with the table, without it, the parent's binary -- alternating; the containers of the last turn are kept apart
    ways = [("checksum", [leon, "-checksum"]), ("plain", [leon]), ("parent", [args.parent])]
    times = {w: [] for w, _ in ways}
    for rep in range(3):
        for w, cmd in ways:
            s, _ = timed([cmd[0], "-file", fq, "-c", "-lossless"] + cmd[1:])
            times[w].append(s)
            print("compress %s: %.2f s" % (w, s), file=sys.stderr, flush=True)
            os.replace(fq + ".leon", os.path.join(args.dir, w + ".fastq.leon"))
    out["compress_lossless_s"] = times
    # -d: the container with the table (verified), the one without (this build, the parent's binary) -- alternating
    ways = [("checksum", leon, "checksum"), ("plain", leon, "plain"), ("parent", args.parent, "plain")]
    times = {w: [] for w, _, _ in ways}
    lines = {}
    for rep in range(3):
        for w, binary, container in ways:
            c = os.path.join(args.dir, container + ".fastq.leon")
            s, log = timed([binary, "-file", c, "-d", "-verbose", "1"] + device)
            times[w].append(s)
            print("decompress %s: %.2f s" % (w, s), file=sys.stderr, flush=True)
            if rep == 0:
                lines[w] = [l for l in log.splitlines() if l.startswith(("time:", "checksums:"))]
            os.remove(c[:-5] + ".d")
    out["decompress_s"] = {"seconds": times, "verbose": lines}
    s, log = timed([leon, "-file", os.path.join(args.dir, "checksum.fastq.leon"), "-d", "-verbose", "1"])
    out["decompress_host_threads_s"] = {"seconds": s, "verbose": [l for l in log.splitlines() if l.startswith(("time:", "checksums:"))]}
    for f in os.listdir(args.dir):
        os.remove(os.path.join(args.dir, f))
    print(json.dumps(out))


kernel() if args.kernel else cli()
