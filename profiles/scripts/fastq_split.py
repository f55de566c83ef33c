"""FASTQ text split into records on the device (k_fq_newlines, k_fq_check, k_fq_split) beside a device copy of the same bytes.

  fastq_split.py --kernel MIB [--bases L]   a text of about MIB MiB of L-base records (default 150; bare '+' lines, headers of 13 bytes) in
                                            device memory: one warm-up call of leon_fastq_split_device on the first records and THREE whole
                                            calls (wall times, each complete on return), the three blobs and both tables compared with what
                                            the text was made from; then the same number of bytes copied device to device three times
                                            (leon_device_copy, wall) and, from a host clock around torch's copy_ with a synchronise, once
                                            more.  The run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times, which
                                            are to be read against the text's bytes (k_fq_newlines reads them once per pass, k_fq_split moves
                                            header, bases and qualities: about 0.99 of them in and as many out).
  fastq_split.py --cli N [--pairs 3]        `leon -c -lossless -verbose 1` on an N-read 150-base FASTQ in a RAM-backed directory, plain and as
                                            BGZF under -input-inflate device: -record-parse host (the parent commit's behaviour) against
                                            -record-parse device in alternating pairs; wall times, the reader's share ("waited for the reader")
                                            and whether the two containers are the same bytes.
Prints one JSON line."""
import argparse
import hashlib
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
ap.add_argument("--bases", type=int, default=150)
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--dir", default="/dev/shm/leon_fastq_split")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)


def main():
    L = args.bases
    H = 13                                                        # "@r" + 11 digits
    rec = 1 + (H - 1) + 1 + L + 1 + 2 + L + 1
    R = (args.kernel << 20) // rec
    rng = np.random.default_rng(16)
    t = np.empty((R, rec), dtype=np.uint8)
    t[:, 0] = ord("@"); t[:, 1] = ord("r")
    idx = np.arange(R, dtype=np.uint64)
    for d in range(11):
        t[:, 2 + d] = (idx // np.uint64(10 ** (10 - d)) % np.uint64(10)).astype(np.uint8) + ord("0")
    t[:, H] = 10
    t[:, H + 1:H + 1 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (R, L), dtype=np.uint8)]
    t[:, H + 1 + L] = 10; t[:, H + 2 + L] = ord("+"); t[:, H + 3 + L] = 10
    t[:, H + 4 + L:H + 4 + 2 * L] = rng.integers(35, 75, (R, L), dtype=np.uint8)
    t[:, rec - 1] = 10
    n_text = R * rec
    d_text = torch.from_numpy(t.reshape(-1)).to(dev)
    blobs = [torch.empty(n_text + 64, dtype=torch.uint8, device=dev) for _ in range(3)]
    offs = [torch.empty(n_text // 4 + 2, dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def call(n):
        return capi.fastq_split_device(d_text.data_ptr(), n, 0, 1 << 62, 0, blobs[0].data_ptr(), offs[0].data_ptr(), blobs[1].data_ptr(), offs[1].data_ptr(),
                                       blobs[2].data_ptr(), n_text, n_text // 4 + 2)
    call(64 * rec)                                                # (code objects loaded)
    ms, res = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        res = call(n_text)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    ok = (res["n_records"] == R and res["consumed"] == n_text and res["stop"] == capi.FASTQ_END and res["plus_bare"] == R
          and res["header_bytes"] == R * (H - 1) and res["base_bytes"] == R * L)
    ok = ok and np.array_equal(blobs[0][:R * (H - 1)].cpu().numpy().reshape(R, H - 1), t[:, 1:H])
    ok = ok and np.array_equal(blobs[1][:R * L].cpu().numpy().reshape(R, L), t[:, H + 1:H + 1 + L])
    ok = ok and np.array_equal(blobs[2][:R * L].cpu().numpy().reshape(R, L), t[:, H + 4 + L:H + 4 + 2 * L])
    ok = ok and np.array_equal(offs[0][:R + 1].cpu().numpy(), np.arange(R + 1) * (H - 1)) and np.array_equal(offs[1][:R + 1].cpu().numpy(), np.arange(R + 1) * L)
    moved = R * (H - 1 + 2 * L)
    dst = torch.empty(moved, dtype=torch.uint8, device=dev)
    capi.device_copy(dst.data_ptr(), d_text.data_ptr(), 4096)
    copy_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        capi.device_copy(dst.data_ptr(), d_text.data_ptr(), moved)
        copy_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dst.copy_(d_text[:moved])
    torch.cuda.synchronize()
    torch_ms = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps({"text_bytes": n_text, "records": R, "bases_per_record": L, "bytes_moved_by_k_fq_split": moved, "leon_fastq_split_device_ms": ms,
                      "outputs_equal_their_source": bool(ok), "leon_device_copy_same_bytes_ms": copy_ms, "torch_copy_same_bytes_ms": torch_ms,
                      "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process"}))
    assert ok


THREADS, MEMBER_TEXT = 16, 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(part):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pay = c.compress(part) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(pay) + 25) + pay +
            struct.pack("<II", zlib.crc32(part), len(part)))


def write_bgzf(fq, gz):
    """fq as BGZF (what bgzip writes: members of 65 280 bytes of text, zlib level 6), on THREADS threads"""
    with open(fq, "rb") as f, open(gz, "wb") as out, ThreadPoolExecutor(THREADS) as pool:
        while True:
            slab = f.read(MEMBER_TEXT * 1024)
            if not slab:
                break
            for m in pool.map(member, [slab[a:a + MEMBER_TEXT] for a in range(0, len(slab), MEMBER_TEXT)]):
                out.write(m)
        out.write(EOF)


def cli():
    os.makedirs(args.dir, exist_ok=True)
    fq, gz = os.path.join(args.dir, "reads.fastq"), os.path.join(args.dir, "reads.fastq.gz")
    bench.write_fastq(fq, args.cli, args.bases, dev)
    torch.cuda.empty_cache()
    write_bgzf(fq, gz)
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    container = fq + ".leon"
    out = {"reads": args.cli, "fastq_bytes": os.path.getsize(fq), "bgzf_bytes": os.path.getsize(gz), "cpus": len(os.sched_getaffinity(0)), "inputs": {}}
    for name, path, more in (("plain", fq, []), ("bgzf_input_inflate_device", gz, ["-input-inflate", "device"])):
        wall, reader, digest, lines = {"host": [], "device": []}, {"host": [], "device": []}, {}, {}
        for rep in range(args.pairs):
            for route in ("host", "device"):
                if os.path.exists(container):
                    os.remove(container)
                t = time.time()
                r = subprocess.run([leon, "-c", "-lossless", "-verbose", "1", "-file", path, "-record-parse", route] + more, capture_output=True, text=True)
                wall[route].append(round(time.time() - t, 2))
                assert r.returncode == 0, (route, r.stderr[-400:])
                m = re.search(r"waited for the reader ([0-9.e+-]+) s", r.stdout)
                reader[route].append(round(float(m.group(1)), 2) if m else None)
                print("%s %s: %.2f s, reader %s" % (name, route, wall[route][-1], reader[route][-1]), file=sys.stderr, flush=True)
                if rep == 0:
                    digest[route] = hashlib.sha256(open(container, "rb").read()).hexdigest()
                    lines[route] = [l for l in r.stdout.splitlines() if l.startswith(("time:", "input:", "parse:", "the pass over the file:"))]
        out["inputs"][name] = {"wall_s": wall, "waited_for_the_reader_s": reader, "same_container": digest["host"] == digest["device"], "verbose": lines}
    for f in (fq, gz, container):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


main() if args.kernel else cli()
