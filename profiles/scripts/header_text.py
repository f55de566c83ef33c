"""Header text on the device (k_hdr_text) against the two decoders that were there before it, on SRA-style headers at scale.

  header_text.py [--headers N]            the C calls, payloads in and text out in host memory, three alternating repeats each:
                                          leon_host_header_decode_blocks, leon_header_decode_blocks (symbols on the device, text on
                                          the host threads), leon_header_decode_blocks_device (symbols and text on the device)
  header_text.py --once [--headers N]     one leon_header_decode_text call and nothing else timed: the run to put under
                                          `rocprofv3 --kernel-trace --stats` (k_hdr_decode_symbols beside k_hdr_text)
  header_text.py --cli N [--parent LEON]  `leon -d -test-file` on an N-read 150 bp FASTQ with -header-text host and device, alternating,
                                          three each; with --parent, another build's binary (no option) in the same alternation
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
import leon_amd  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--headers", type=int, default=10_000_000)
ap.add_argument("--once", action="store_true")
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--dir", default="/dev/shm/leon_header_text")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)


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
    out = {"reads": N, "fastq_bytes": os.path.getsize(fq)}
    r = subprocess.run([leon, "-file", fq, "-c", "-lossless"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ways = [("host", [leon, "-header-text", "host"]), ("device", [leon, "-header-text", "device"])]
    if args.parent:
        ways.append(("parent", [args.parent]))
    times = {w: [] for w, _ in ways}
    for rep in range(3):
        for w, cmd in ways:
            t = time.time()
            r = subprocess.run([cmd[0], "-file", fq + ".leon", "-d", "-test-file", "-verbose", "1"] + cmd[1:], capture_output=True, text=True)
            times[w].append(round(time.time() - t, 2))
            print("%s: %.2f s" % (w, times[w][-1]), file=sys.stderr, flush=True)
            assert r.returncode == 0 and "identical" in r.stdout, (w, r.stdout[-400:], r.stderr[-400:])
            if rep == 0:
                out[w + "_stdout"] = [l for l in r.stdout.splitlines() if l.startswith("time:") or l.startswith("header text:")]
    out["decompress_test_file_s"] = times
    for f in (fq, fq + ".leon", fq + ".d"):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


def calls():
    nh = args.headers
    blob, hoff = bench.sra_headers(nh, seed=7)
    first = blob[:int(hoff[1])].tobytes()
    ctx = leon_amd.DnaEncodeContext(kmer_size=31, reads_per_block=50000, bloom_tai=1000, device_id=0)
    d_blob = torch.from_numpy(blob.copy()).to(dev); d_hoff = torch.from_numpy(hoff).to(dev)
    hblocks = []
    keep = capi.SINK(lambda user, bid, ptr, size, nreads: (hblocks.append((int(bid), ctypes.string_at(ptr, size), int(nreads))), 0)[1])
    rc = ctx.lib.leon_header_encode_batch_device(ctx.h, ctypes.c_void_p(d_blob.data_ptr()), ctypes.c_void_p(d_hoff.data_ptr()), nh, 0, first, len(first), keep, None)
    assert rc == 0
    del d_blob, d_hoff
    torch.cuda.empty_cache()
    pay, poff, pnr = capi._join_blocks(hblocks)
    nb = len(hblocks)
    P = (capi._ptr(pay, capi._u8p), capi._ptr(poff, capi._u64p), capi._ptr(pnr, capi._u32p), nb, first, len(first))
    out = {"headers": nh, "blocks": nb, "text_bytes": int(hoff[-1]), "payload_bytes": int(poff[-1]), "cpus": len(os.sched_getaffinity(0))}
    if args.once:
        S = ctx.header_text_set(hblocks[:2], first)               # (code objects loaded, buffers' first touch)
        S.close()
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = ctx.lib.leon_header_decode_text(ctx.h, P[0], P[1], P[2], None, nb, first, len(first), ctypes.byref(h))
        out["leon_header_decode_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert rc == 0, rc
        ctx.lib.leon_header_text_free(h)
        print(json.dumps(out))
        return
    out_off = np.zeros(nh + 1, dtype=np.uint64); need = ctypes.c_uint64(); on_host = ctypes.c_uint64(); cap = int(hoff[-1]) + 64
    ways = (("host_threads", lambda o: ctx.lib.leon_host_header_decode_blocks(*P, capi._ptr(o, capi._u8p), cap, capi._ptr(out_off, capi._u64p), ctypes.byref(need), 0)),
            ("device_symbols", lambda o: ctx.lib.leon_header_decode_blocks(ctx.h, *P, capi._ptr(o, capi._u8p), cap, capi._ptr(out_off, capi._u64p), ctypes.byref(need), 0)),
            ("device_text", lambda o: ctx.lib.leon_header_decode_blocks_device(ctx.h, *P, capi._ptr(o, capi._u8p), cap, capi._ptr(out_off, capi._u64p), ctypes.byref(need), 0,
                                                                                 ctypes.byref(on_host))))
    times = {w: [] for w, _ in ways}
    equal = True
    for rep in range(4):                                           # the first turn warms every way up and is not kept
        for w, call in ways:
            o = np.empty(cap, dtype=np.uint8)
            out_off[:] = 0
            t0 = time.perf_counter(); rc = call(o); dt = time.perf_counter() - t0
            assert rc == 0, (w, rc)
            equal = equal and bool(np.array_equal(o[:int(hoff[-1])], blob)) and bool(np.array_equal(out_off.astype(np.int64), hoff))
            if rep:
                times[w].append(round(dt * 1e3, 1))
    out.update({"ms": times, "equal_input": equal, "device_text_blocks_on_host": int(on_host.value)})
    print(json.dumps(out))


cli() if args.cli else calls()
