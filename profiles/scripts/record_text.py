"""Record text on the device (k_fmt_sizes, k_fmt_records) against the host threads' formatter.

  record_text.py --kernel N               N synthetic FASTQ records x 150 bp with SRA-style headers in device memory, one warm-up call of
                                          leon_records_format_device on a slice and TWO whole calls; the first and last records checked against
                                          the definition.  The run to put under `rocprofv3 --kernel-trace --stats` (kernel times come from
                                          there; the JSON line carries the bytes the kernel reads and writes and the calls' wall time)
  record_text.py --cli N [--parent LEON]  `leon -d` and `leon -d -test-file` on an N-read 150 bp FASTQ in a RAM-backed directory:
                                          -record-text host and device alternating, three each, -header-text device on both sides; with
                                          --parent another build's binary (no -record-text) in the same alternation; then one pair under
                                          -header-text host
Prints one JSON line."""
import argparse
import ctypes
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
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_record_text")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
COPY_TBS = 6.29                                                   # the float4 copy measured on this chip: the yardstick


def kernel():
    N, L = args.kernel, 150
    blob, hoff = bench.sra_headers(N, seed=7)
    g = torch.Generator(device=dev); g.manual_seed(5)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    d_bases = torch.empty(N * L, dtype=torch.uint8, device=dev)
    d_quals = torch.empty(N * L, dtype=torch.uint8, device=dev)
    step = 1 << 28                                                # (random integers come as 64-bit words: a slice at a time)
    for a in range(0, N * L, step):
        m = min(step, N * L - a)
        d_bases[a:a + m] = acgt[torch.randint(0, 4, (m,), device=dev, generator=g)]
        d_quals[a:a + m] = (torch.randint(0, 41, (m,), device=dev, generator=g) + 33).to(torch.uint8)
    d_len = torch.full((N,), L, dtype=torch.int32, device=dev)
    d_hdr = torch.from_numpy(blob).to(dev)
    d_hoff = torch.from_numpy(hoff).to(dev)
    hdr_bytes = int(hoff[-1])
    text_size = 2 * N + hdr_bytes + N * (L + 1) + N * (3 + L)
    d_text = torch.empty(text_size + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def call(n):
        hb = int(hoff[n] - hoff[0])
        t0 = time.perf_counter()
        size = capi.records_format_device(d_bases.data_ptr(), d_len.data_ptr(), n, n * L, d_text.data_ptr(), text_size, lead=b"@", fastq=True,
                                          d_hdr_text=d_hdr.data_ptr(), d_hdr_off=d_hoff.data_ptr(), hdr_bytes=hb, d_quals=d_quals.data_ptr())
        return size, (time.perf_counter() - t0) * 1e3
    call(min(N, 1000))                                            # (code objects loaded)
    ms = []
    for _ in range(2):
        size, dt = call(N)
        assert size == text_size, (size, text_size)
        ms.append(round(dt, 2))
    # the first and the last 1 000 records against the definition
    k = min(N, 1000)
    for lo in (0, N - k):
        bases = d_bases[lo * L:(lo + k) * L].cpu().numpy().tobytes()
        quals = d_quals[lo * L:(lo + k) * L].cpu().numpy().tobytes()
        want = b"".join(b"@" + blob[int(hoff[lo + i]):int(hoff[lo + i + 1])].tobytes() + b"\n" + bases[i * L:(i + 1) * L] + b"\n+\n" + quals[i * L:(i + 1) * L] + b"\n"
                        for i in range(k))
        at = 2 * lo + int(hoff[lo]) + lo * (L + 1) + lo * (3 + L)
        assert d_text[at:at + len(want)].cpu().numpy().tobytes() == want, "the text differs from the definition near record %d" % lo
    moved = text_size + 2 * N * L + hdr_bytes + 4 * N + 8 * (N + 1) + 16 * (N + 1)    # written; bases, qualities, headers, lengths, header offsets, scanned offsets read
    print(json.dumps({"records": N, "read_len": L, "text_bytes": text_size, "header_bytes": hdr_bytes, "k_fmt_records_bytes_moved": moved,
                      "leon_records_format_device_ms": ms, "copy_yardstick_TBs": COPY_TBS,
                      "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process"}))


def cli():
    N, L = args.cli, 150
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

    def alternate(name, mode, hdr, reps, with_parent):
        ways = [("host", [leon, "-record-text", "host"]), ("device", [leon, "-record-text", "device"])]
        if with_parent and args.parent:
            ways.append(("parent", [args.parent]))
        times = {w: [] for w, _ in ways}
        lines = {}
        for rep in range(reps):
            for w, cmd in ways:
                if os.path.exists(fq + ".d"):
                    os.remove(fq + ".d")
                t = time.time()
                r = subprocess.run([cmd[0], "-file", fq + ".leon", "-verbose", "1", "-header-text", hdr] + mode + cmd[1:], capture_output=True, text=True)
                times[w].append(round(time.time() - t, 2))
                print("%s %s: %.2f s" % (name, w, times[w][-1]), file=sys.stderr, flush=True)
                assert r.returncode == 0 and ("identical" in r.stdout or "-test-file" not in mode), (w, r.stdout[-400:], r.stderr[-400:])
                if rep == 0:
                    lines[w] = [l for l in r.stdout.splitlines() if l.startswith(("time:", "header text:", "record text:"))]
        out[name] = {"seconds": times, "verbose": lines}
    alternate("decompress_s", ["-d"], "device", 3, True)
    alternate("decompress_test_file_s", ["-d", "-test-file"], "device", 3, True)
    alternate("decompress_header_text_host_s", ["-d"], "host", 1, False)
    for f in (fq, fq + ".leon", fq + ".d"):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


kernel() if args.kernel else cli()
