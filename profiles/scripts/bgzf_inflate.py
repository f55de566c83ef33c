"""BGZF input inflated on the device (k_bgzf_inflate, the CRC-32 of the shares, k_bgzf_gather) against zlib on the host.

  bgzf_inflate.py --kernel N [--chunks-mb 8,32]  an N-read 150 bp synthetic FASTQ (bench.py's generator) as BGZF, members of 65 280 bytes written by zlib
                                          at level 6.  Per chunk size: the file's first chunk of that many compressed bytes walked by
                                          leon_host_bgzf_members; one warm-up call of leon_bgzf_inflate_device on 64 members and TWO calls on
                                          the chunk, the text compared with the file's; leon_host_bgzf_inflate on the same members with 16
                                          threads and with 1, in the same run.  The run to put under `rocprofv3 --kernel-trace --stats`
                                          (kernel times come from there; the JSON line carries the calls' wall times, the bytes and the
                                          literal/length symbols decoded)
  bgzf_inflate.py --cli N [--parent LEON] [--pairs 3]  `leon -c -lossless -verbose 1` on the N-read file as BGZF in a RAM-backed directory:
                                          -input-inflate host and device in alternating pairs, and -- with --parent, another build's
                                          binary -- that build without the option in the same alternation, beside this build without
                                          the option.  Reports the wall times and each run's "waited for the reader" seconds.
Prints one JSON line."""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, default=0)
ap.add_argument("--chunks-mb", default="8,32")
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--dir", default="/dev/shm/leon_bgzf_inflate")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
L, THREADS, MEMBER_TEXT = 150, 16, 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(part):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pay = c.compress(part) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(pay) + 25) + pay +
            struct.pack("<II", zlib.crc32(part), len(part)))


def write_bgzf(fq, gz):
    """fq as BGZF (what bgzip writes: members of 65 280 bytes of text, zlib level 6), on THREADS threads"""
    t0 = time.time()
    with open(fq, "rb") as f, open(gz, "wb") as out, ThreadPoolExecutor(THREADS) as pool:
        while True:
            slab = f.read(MEMBER_TEXT * 1024)
            if not slab:
                break
            for m in pool.map(member, [slab[a:a + MEMBER_TEXT] for a in range(0, len(slab), MEMBER_TEXT)]):
                out.write(m)
        out.write(EOF)
    return round(time.time() - t0, 1)


def make_files(n):
    os.makedirs(args.dir, exist_ok=True)
    fq, gz = os.path.join(args.dir, "reads.fastq"), os.path.join(args.dir, "reads.fastq.gz")
    bench.write_fastq(fq, n, L, dev)
    torch.cuda.empty_cache()
    secs = write_bgzf(fq, gz)
    return fq, gz, secs


def kernel():
    fq, gz, secs = make_files(args.kernel)
    data = np.fromfile(gz, dtype=np.uint8)
    text = np.fromfile(fq, dtype=np.uint8)
    out = {"reads": args.kernel, "fastq_bytes": int(len(text)), "bgzf_bytes": int(len(data)), "bgzf_written_s": secs, "host_threads": THREADS, "chunks": {}}
    lib = capi.load_library()
    import ctypes as C
    for mb in [int(x) for x in args.chunks_mb.split(",")]:
        chunk = data[:mb << 20]
        w = capi.host_bgzf_members(chunk, last=len(chunk) == len(data))
        assert w["rc"] == 0 and w["n_members"] > 64, w
        off, n, n_text = w["member_off"], w["n_members"], w["n_text"]
        d_text = torch.empty(n_text + 64, dtype=torch.uint8, device=dev)
        capi.bgzf_inflate_device(chunk, off[:65], d_text.data_ptr(), n_text)           # (code objects loaded, pinned buffers made)
        ms, syms = [], 0
        for _ in range(2):
            d_text.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, syms = capi.bgzf_inflate_device(chunk, off, d_text.data_ptr(), n_text)
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            assert got == n_text
        same = bool(torch.equal(d_text[:n_text].cpu(), torch.from_numpy(text[:n_text])))
        h_text = np.empty(n_text + 1, dtype=np.uint8)
        host = {}
        for threads in (THREADS, 1):
            t = []
            for _ in range(2 if threads > 1 else 1):
                need = C.c_uint64()
                t0 = time.perf_counter()
                rc = lib.leon_host_bgzf_inflate(C.c_void_p(chunk.ctypes.data), int(w["consumed"]), C.c_void_p(off.ctypes.data), n, C.c_void_p(h_text.ctypes.data), n_text,
                                                C.byref(need), threads)
                t.append(round((time.perf_counter() - t0) * 1e3, 2))
                assert rc == 0
            host[str(threads)] = t
        out["chunks"]["%d MiB" % mb] = {"members": int(n), "payload_bytes": int(w["consumed"]), "text_bytes": int(n_text), "leon_bgzf_inflate_device_ms": ms,
                                        "leon_host_bgzf_inflate_ms_by_threads": host, "literal_length_symbols": int(syms),
                                        "device_equals_the_file": same, "host_equals_the_file": bool(np.array_equal(h_text[:n_text], text[:n_text]))}
        del d_text
    out["note"] = "kernel times (k_bgzf_inflate, k_crc32_tiles, k_bgzf_gather): the rocprofv3 --kernel-trace --stats run around this process"
    for f in (fq, gz):
        os.remove(f)
    print(json.dumps(out))


def cli():
    fq, gz, secs = make_files(args.cli)
    out = {"reads": args.cli, "fastq_bytes": os.path.getsize(fq), "bgzf_bytes": os.path.getsize(gz), "bgzf_written_s": secs, "cpus": len(os.sched_getaffinity(0))}
    os.remove(fq)
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    ways = [("host", [leon, "-input-inflate", "host"]), ("device", [leon, "-input-inflate", "device"]), ("no_option", [leon])]
    if args.parent:
        ways.append(("parent", [args.parent]))
    wall, reader, lines, sizes = {w: [] for w, _ in ways}, {w: [] for w, _ in ways}, {}, {}
    container = fq + ".leon"
    for rep in range(args.pairs):
        for w, cmd in ways:
            if os.path.exists(container):
                os.remove(container)
            t = time.time()
            r = subprocess.run([cmd[0], "-c", "-lossless", "-verbose", "1", "-file", gz] + cmd[1:], capture_output=True, text=True)
            wall[w].append(round(time.time() - t, 2))
            assert r.returncode == 0, (w, r.stderr[-400:])
            m = re.search(r"waited for the reader ([0-9.e+-]+) s", r.stdout)
            reader[w].append(round(float(m.group(1)), 2) if m else None)
            print("%s: %.2f s, reader %s" % (w, wall[w][-1], reader[w][-1]), file=sys.stderr, flush=True)
            sizes.setdefault(w, os.path.getsize(container))
            if rep == 0:
                lines[w] = [l for l in r.stdout.splitlines() if l.startswith(("time:", "input:", "the pass over the file:"))]
    out.update({"wall_s": wall, "w_reader_s": reader, "container_bytes": sizes, "verbose": lines})
    for f in (gz, container):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


kernel() if args.kernel else cli()
