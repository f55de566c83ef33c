"""The restored file written as BGZF on the device (k_deflate_chunks, k_crc32_tiles, k_bgzf_members; `leon -d -gz`).

  bgzf.py --kernel [N]                 the FASTQ text of N synthetic reads x 150 bp (default 10 M: 3.65 GB) in device memory: one warm-up
                                       call of leon_text_bgzf_device on its first member and TWO whole calls whose output is counted and
                                       dropped by the sink; then, for the first 64 MiB, the output kept and read back with gzip.decompress,
                                       and the same text through zlib (level 6, and Z_RLE) on one thread for the sizes.  The run to put under
                                       `rocprofv3 --kernel-trace --stats` (kernel times come from there; the JSON line carries the calls'
                                       wall times, which include the copy of the output to the host); text bytes / a kernel's time is to be
                                       read against the float4 copy measured on this chip, 6.29 TB/s
  bgzf.py --kernel [N] --records       the same, and behind it leon_text_bgzf_records_device on the same text with every
                                       record's offset (found on the device: every fourth newline), one warm-up call on the first records
                                       and TWO whole calls, with member tables; the JSON line gains the calls' wall times, members and
                                       bytes.  Under `rocprofv3 --kernel-trace --stats`: k_bgzf_cuts beside k_deflate_chunks
  bgzf.py --kernel [N] --matches       the same calls through leon_text_bgzf_device_ex with LEON_BGZF_F_MATCHES (fixed cuts, no member table;
                                       DESIGN.md 4.18): k_deflate_lz_chunks in the place of k_deflate_chunks, on the same text; the JSON line's
                                       keys keep their names and gain "matches": true.  (--records keeps the encoder without matches.)
  bgzf.py --cli N --parent LEON        `leon -d`, `leon -d -gz` and the parent commit's `leon -d` on the lossless container of an N-read
                                       150 bp FASTQ in a RAM-backed directory, alternating, three each, -header-text device -record-text
                                       device -qual-inflate device on every side; the output sizes and the `time:` and `output:` lines of
                                       -verbose 1
Prints one JSON line."""
import argparse
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import threading
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, nargs="?", const=10_000_000, default=0)
ap.add_argument("--records", action="store_true")
ap.add_argument("--matches", action="store_true")
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_bgzf")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
L = 150
COPY_TBS = 6.29                                                   # the float4 copy on this chip
SAMPLE = 64 << 20


def kernel():
    N = args.kernel
    os.makedirs(args.dir, exist_ok=True)
    fq = os.path.join(args.dir, "reads.fastq")
    bench.write_fastq(fq, N, L, dev)
    text = np.fromfile(fq, dtype=np.uint8)
    n = len(text)
    d = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    d[:n] = torch.from_numpy(text).to(dev)
    torch.cuda.synchronize()
    os.remove(fq)
    lib = capi.load_library()
    counted, lock = [0], threading.Lock()

    def drop(user, offset, address, size):                        # (called from the library's copy threads)
        with lock:
            counted[0] += size
        return 0
    sink = capi.PIECE_SINK(drop)
    taken, out_bytes, members = C.c_uint64(), C.c_uint64(), C.c_uint64()

    def call(n_text):
        counted[0] = 0
        if args.matches:
            rc = lib.leon_text_bgzf_device_ex(0, C.c_void_p(d.data_ptr()), 0, n_text, None, 0, 1, sink, None, C.byref(taken), C.byref(out_bytes), None, None, 0,
                                              C.byref(members), capi.BGZF_F_MATCHES)
        else:
            rc = lib.leon_text_bgzf_device(0, C.c_void_p(d.data_ptr()), n_text, 1, sink, None, C.byref(taken), C.byref(out_bytes), C.byref(members))
        assert rc == 0, lib.leon_last_error(None)
        assert counted[0] == out_bytes.value and taken.value == n_text
    call(capi.BGZF_MEMBER_TEXT)                                   # (code objects loaded, scratch for one member)
    ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        call(n)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    whole = {"members": members.value, "out_bytes": out_bytes.value}
    m = min(n, SAMPLE)
    sample = text[:m].tobytes()
    got = capi.text_bgzf_device_ex(d.data_ptr(), 0, m, 0, 0, flags=capi.BGZF_F_MATCHES, tables=False)[0] if args.matches else capi.text_bgzf_device(d.data_ptr(), m)[0]
    t0 = time.perf_counter()
    z6 = len(zlib.compress(sample, 6))
    z6_s = time.perf_counter() - t0
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
    zrle = len(c.compress(sample) + c.flush())
    rec = {}
    if args.records:
        nl = (d[:n] == 10).nonzero().flatten()
        assert len(nl) == 4 * N
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), nl[3::4] + 1]).contiguous()
        del nl
        torch.cuda.synchronize()
        cap = capi.bgzf_members_bound(n)
        m_out, m_text = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)

        def call_records(n_records, last):
            counted[0] = 0
            n_body = int(off[n_records])
            rc = lib.leon_text_bgzf_records_device(0, C.c_void_p(d.data_ptr()), 0, n_body, C.c_void_p(off.data_ptr()), n_records, last, sink, None, C.byref(taken),
                                                   C.byref(out_bytes), C.c_void_p(m_out.ctypes.data), C.c_void_p(m_text.ctypes.data), cap, C.byref(members))
            assert rc == 0, lib.leon_last_error(None)
            assert counted[0] == out_bytes.value and (not last or taken.value == n_body)
        call_records(min(N, 1000), 1)
        rms = []
        for _ in range(2):
            t0 = time.perf_counter()
            call_records(N, 1)
            rms.append(round((time.perf_counter() - t0) * 1e3, 2))
        assert m_text[0] == 0 and (np.diff(m_text[:members.value].astype(np.int64)) <= capi.BGZF_MEMBER_TEXT).all()
        rec = {"leon_text_bgzf_records_device_ms": rms, "records_members": members.value, "records_out_bytes": out_bytes.value,
               "records_out_per_fixed_out": round(out_bytes.value / whole["out_bytes"], 6)}
    print(json.dumps({"reads": N, "text_bytes": n, "matches": args.matches, "leon_text_bgzf_device_ms": ms, **whole, **rec, "text_per_out": round(n / whole["out_bytes"], 4),
                      "sample_bytes": m, "sample_out_bytes": len(got), "sample_reads_back": gzip.decompress(got) == sample,
                      "sample_zlib6_bytes": z6, "sample_zlib6_one_thread_gb_s": round(m / z6_s / 1e9, 4), "sample_zlib_rle_bytes": zrle,
                      "float4_copy_tb_s": COPY_TBS,
                      "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process; text bytes / a kernel's time against float4_copy_tb_s"}))


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
    s, _ = timed([leon, "-file", fq, "-c", "-lossless", "-qual-deflate", "device"])
    out["compress_s"] = s
    container = fq + ".leon"
    ways = [("plain", leon, [], ".d"), ("gz", leon, ["-gz"], ".d.gz"), ("parent", args.parent, [], ".d")]
    times = {w: [] for w, _, _, _ in ways}
    lines, sizes = {}, {}
    for rep in range(3):
        for w, binary, opts, suffix in ways:
            s, log = timed([binary, "-file", container, "-d", "-verbose", "1"] + opts + device)
            times[w].append(s)
            print("decompress %s: %.2f s" % (w, s), file=sys.stderr, flush=True)
            if rep == 0:
                lines[w] = [l for l in log.splitlines() if l.startswith(("time:", "output:"))]
                sizes[w] = os.path.getsize(fq + suffix)
            os.remove(fq + suffix)
    out["decompress_s"] = {"seconds": times, "verbose": lines, "output_bytes": sizes}
    for f in os.listdir(args.dir):
        os.remove(os.path.join(args.dir, f))
    print(json.dumps(out))


kernel() if args.kernel else cli()
