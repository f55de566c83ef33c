"""Quality blocks inflated on the device (k_qual_inflate, k_qual_tiles, k_qual_lines) against zlib on the host threads.

  qual_inflate.py --kernel N [--sets a,b,c]  N synthetic 150 bp quality lines (bench.py's structured qualities) in blocks of 50 000, written
                                          (a) by zlib at the default level (leon_host_qual_encode_blocks), (b) by leon_qual_deflate_blocks_device,
                                          (c) lossy-looking (97 % '@') by zlib; per set one warm-up call of leon_qual_inflate_blocks_device on
                                          8 blocks and TWO whole calls, the result compared with the qualities that were written, beside
                                          leon_host_qual_decode_blocks on the same blocks with 16 threads in the same run.  The run to put under
                                          `rocprofv3 --kernel-trace --stats` (kernel times come from there; the JSON line carries the calls' wall
                                          times, the payload bytes and the literal/length symbols decoded)
  qual_inflate.py --cli N [--parent LEON]  `leon -d` and `leon -d -test-file` on an N-read 150 bp FASTQ in a RAM-backed directory:
                                          -qual-inflate host and device alternating, three each, under -header-text device -record-text device;
                                          with --parent another build's binary (no -qual-inflate) in the same alternation; then one pair under
                                          -record-text host
Prints one JSON line."""
import argparse
import ctypes as C
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
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, default=0)
ap.add_argument("--sets", default="a,b,c")
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_qual_inflate")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
RPB, L, THREADS = 50000, 150, 16


def kernel():
    N = args.kernel
    lib = capi.load_library()
    g = torch.Generator(device=dev); g.manual_seed(11)
    qalpha = torch.tensor(list(b"#5:?ABCDEFGHIJ"), dtype=torch.uint8, device=dev)
    d_src = torch.empty((N, L), dtype=torch.uint8, device=dev)
    step = 1 << 21
    for a in range(0, N, step):
        m = min(step, N - a)
        d_src[a:a + m] = qalpha[torch.minimum(torch.randint(0, 14, (m, L), device=dev, generator=g), torch.randint(4, 14, (m, 1), device=dev, generator=g))]
    off = np.arange(N + 1, dtype=np.uint64) * L
    n_blocks = (N + RPB - 1) // RPB
    nr = np.array([min(RPB, N - b * RPB) for b in range(n_blocks)], dtype=np.uint32)
    nb = nr.astype(np.uint64) * L
    d_out = torch.empty(N * L + 64, dtype=torch.uint8, device=dev)
    d_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
    h_out, h_off = np.empty(N * L + 1, dtype=np.uint8), np.empty(N + 1, dtype=np.uint64)
    out = {"reads": N, "read_len": L, "blocks": n_blocks, "text_bytes": N * (L + 1), "host_threads": THREADS, "sets": {}}
    for name in args.sets.split(","):
        src = d_src
        if name == "c":
            src = torch.where(torch.rand((N, L), device=dev, generator=g) < 0.97, torch.full_like(d_src, 64), d_src)
        torch.cuda.synchronize()
        if name == "b":
            blocks = capi.qual_deflate_blocks_device(src.data_ptr(), off, RPB)
        else:
            blocks = capi.host_qual_encode_blocks(src.cpu().numpy().tobytes(), off, RPB, n_threads=THREADS)
        blocks.sort()
        pay = np.frombuffer(b"".join(b[1] for b in blocks), dtype=np.uint8)
        poff = np.zeros(n_blocks + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(b[1]) for b in blocks])
        del blocks

        def device_call(n):
            t0 = time.perf_counter()
            syms = capi.qual_inflate_blocks_device(pay, poff, nr, nb, d_out.data_ptr(), N * L, d_off.data_ptr(), 0, n_blocks=n)
            return syms, (time.perf_counter() - t0) * 1e3
        device_call(min(n_blocks, 8))                             # (code objects loaded, pinned buffers made)
        ms, syms = [], 0
        for _ in range(2):
            d_out.zero_()
            syms, dt = device_call(n_blocks)
            ms.append(round(dt, 1))
        same = bool(torch.equal(d_out[:N * L].view(N, L), src)) and bool(torch.equal(d_off, torch.arange(N + 1, device=dev, dtype=torch.int64) * L))
        host_ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            rc = lib.leon_host_qual_decode_blocks(capi._ptr(pay, capi._u8p), capi._ptr(poff, capi._u64p), capi._ptr(nr, capi._u32p), capi._ptr(nb, capi._u64p),
                                                  n_blocks, capi._ptr(h_out, capi._u8p), N * L, capi._ptr(h_off, capi._u64p), THREADS)
            host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
            assert rc == 0
        same_host = bool(np.array_equal(h_out[:RPB * L], src[:RPB].cpu().numpy().reshape(-1)))
        out["sets"][name] = {"payload_bytes": int(poff[-1]), "leon_qual_inflate_blocks_device_ms": ms, "leon_host_qual_decode_blocks_ms": host_ms,
                             "literal_length_symbols": int(syms), "symbols_per_block": int(syms // max(n_blocks, 1)),
                             "device_equals_what_was_written": same, "host_equals_what_was_written": same_host}
        del pay
    out["note"] = "kernel times: the rocprofv3 --kernel-trace --stats run around this process; symbols per second of one wave's chain = symbols_per_block / k_qual_inflate's time"
    print(json.dumps(out))


def cli():
    N = args.cli
    os.makedirs(args.dir, exist_ok=True)
    fq = os.path.join(args.dir, "reads.fastq")
    import threading
    done = threading.Event()

    def heartbeat():                                              # (a 36 GB file takes minutes to write: say so on stderr)
        while not done.wait(60):
            print("writing %s: %.1f GB" % (fq, os.path.getsize(fq) / 1e9 if os.path.exists(fq) else 0), file=sys.stderr, flush=True)
    threading.Thread(target=heartbeat, daemon=True).start()
    bench.write_fastq(fq, N, L, dev)
    done.set()
    torch.cuda.empty_cache()
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    out = {"reads": N, "fastq_bytes": os.path.getsize(fq), "cpus": len(os.sched_getaffinity(0))}
    t = time.time()
    r = subprocess.run([leon, "-file", fq, "-c", "-lossless"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out["compress_s"] = round(time.time() - t, 2)

    def alternate(name, mode, rec, reps, with_parent):
        ways = [("host", [leon, "-qual-inflate", "host"]), ("device", [leon, "-qual-inflate", "device"])]
        if with_parent and args.parent:
            ways.append(("parent", [args.parent]))
        times = {w: [] for w, _ in ways}
        lines = {}
        for rep in range(reps):
            for w, cmd in ways:
                if os.path.exists(fq + ".d"):
                    os.remove(fq + ".d")
                t = time.time()
                r = subprocess.run([cmd[0], "-file", fq + ".leon", "-verbose", "1", "-header-text", "device", "-record-text", rec] + mode + cmd[1:], capture_output=True, text=True)
                times[w].append(round(time.time() - t, 2))
                print("%s %s: %.2f s" % (name, w, times[w][-1]), file=sys.stderr, flush=True)
                assert r.returncode == 0 and ("identical" in r.stdout or "-test-file" not in mode), (w, r.stdout[-400:], r.stderr[-400:])
                if rep == 0:
                    lines[w] = [l for l in r.stdout.splitlines() if l.startswith(("time:", "header text:", "record text:", "quality blocks:"))]
        out[name] = {"seconds": times, "verbose": lines}
    alternate("decompress_s", ["-d"], "device", 3, True)
    alternate("decompress_test_file_s", ["-d", "-test-file"], "device", 3, True)
    alternate("decompress_record_text_host_s", ["-d"], "host", 1, False)
    for f in (fq, fq + ".leon", fq + ".d"):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


kernel() if args.kernel else cli()
