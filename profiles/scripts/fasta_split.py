"""FASTA text split into records on the device (k_fq_newlines, k_fa_lines, k_fa_heads, k_fa_offsets, k_fa_split) beside a
device copy of the same bytes.

  fasta_split.py --kernel MIB --shape S     a text of about MIB MiB in device memory, S one of
                                              single   150-base records on one line (wrap 0),
                                              wrapped  150-base records wrapped at 60 (wrap 60),
                                              contig   records of 8 MiB wrapped at 60 (wrap 60);
                                            headers of 13 bytes.  One warm-up call of leon_fasta_split_device on the first record and THREE
                                            whole calls (wall times, each complete on return; last = 1), both blobs and both tables compared
                                            with what the text was made from; then the bytes k_fa_split moves copied device to device three
                                            times (leon_device_copy, wall).  The run to put under `rocprofv3 --kernel-trace --stats` for the
                                            kernels' own times.
  fasta_split.py --cli N [--pairs 3]        `leon -c -verbose 1` on an N-read FASTA (150 bases wrapped at 60) in a RAM-backed directory,
                                            plain and as BGZF under -input-inflate device: the host route against -record-parse device
                                            -record-parse-fasta in alternating pairs; wall times, the reader's share ("waited for the
                                            reader") and whether the two containers are the same bytes.
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
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, default=0)
ap.add_argument("--shape", default="single", choices=["single", "wrapped", "contig"])
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--dir", default="/dev/shm/leon_fasta_split")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)
H = 13                                                            # ">r" + 11 digits


def records(R, L, W, rng, first=0):
    """R records of L bases on lines of W as one array (R, record bytes); the header and base columns"""
    n_lines = (L + W - 1) // W
    rec = H + 1 + L + n_lines
    t = np.empty((R, rec), dtype=np.uint8)
    t[:, 0] = ord(">"); t[:, 1] = ord("r")
    idx = np.arange(first, first + R, dtype=np.uint64)
    for d in range(11):
        t[:, 2 + d] = (idx // np.uint64(10 ** (10 - d)) % np.uint64(10)).astype(np.uint8) + ord("0")
    t[:, H] = 10
    cols = np.arange(L) + (np.arange(L) // W) + H + 1
    t[:, cols] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (R, L), dtype=np.uint8)]
    ends = np.minimum((np.arange(n_lines) + 1) * W, L) + np.arange(n_lines) + H + 1
    t[:, ends] = 10
    return t, cols


def main():
    L, W = {"single": (150, 150), "wrapped": (150, 60), "contig": (8 << 20, 60)}[args.shape]
    wrap = 0 if args.shape == "single" else W
    rng = np.random.default_rng(17)
    rec = H + 1 + L + (L + W - 1) // W
    R = max((args.kernel << 20) // rec, 1)
    t, cols = records(R, L, W, rng)
    n_text = R * rec
    n_lines = R * (1 + (L + W - 1) // W)
    d_text = torch.from_numpy(t.reshape(-1)).to(dev)
    blobs = [torch.empty(n_text + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
    offs = [torch.empty(n_text // 2 + 2, dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def call(n):
        return capi.fasta_split_device(d_text.data_ptr(), n, 1, 1 << 62, wrap, blobs[0].data_ptr(), offs[0].data_ptr(), blobs[1].data_ptr(), offs[1].data_ptr(),
                                       n_text, n_text // 2 + 2)
    call(rec)                                                     # (code objects loaded)
    ms, res = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        res = call(n_text)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    ok = (res["n_records"] == R and res["consumed"] == n_text and res["stop"] == capi.FASTA_END and res["header_bytes"] == R * (H - 1) and res["base_bytes"] == R * L
          and res["single_max"] == (L if args.shape == "single" else 0))
    ok = ok and np.array_equal(blobs[0][:R * (H - 1)].cpu().numpy().reshape(R, H - 1), t[:, 1:H])
    ok = ok and np.array_equal(blobs[1][:R * L].cpu().numpy().reshape(R, L), t[:, cols])
    ok = ok and np.array_equal(offs[0][:R + 1].cpu().numpy(), np.arange(R + 1) * (H - 1)) and np.array_equal(offs[1][:R + 1].cpu().numpy(), np.arange(R + 1) * L)
    moved = R * (H - 1 + L)
    dst = torch.empty(moved, dtype=torch.uint8, device=dev)
    capi.device_copy(dst.data_ptr(), d_text.data_ptr(), 4096)
    copy_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        capi.device_copy(dst.data_ptr(), d_text.data_ptr(), moved)
        copy_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    print(json.dumps({"shape": args.shape, "text_bytes": n_text, "records": R, "lines": n_lines, "bases_per_record": L, "line_width": W,
                      "bytes_moved_by_k_fa_split": moved, "leon_fasta_split_device_ms": ms, "outputs_equal_their_source": bool(ok),
                      "leon_device_copy_same_bytes_ms": copy_ms, "note": "kernel times: the rocprofv3 --kernel-trace --stats run around this process"}))
    assert ok


THREADS, MEMBER_TEXT = 16, 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(part):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pay = c.compress(part) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(pay) + 25) + pay +
            struct.pack("<II", zlib.crc32(part), len(part)))


def write_bgzf(fa, gz):
    """fa as BGZF (what bgzip writes: members of 65 280 bytes of text, zlib level 6), on THREADS threads"""
    with open(fa, "rb") as f, open(gz, "wb") as out, ThreadPoolExecutor(THREADS) as pool:
        while True:
            slab = f.read(MEMBER_TEXT * 1024)
            if not slab:
                break
            for m in pool.map(member, [slab[a:a + MEMBER_TEXT] for a in range(0, len(slab), MEMBER_TEXT)]):
                out.write(m)
        out.write(EOF)


def write_fasta(path, n, L, W):
    """n reads drawn with 1 % errors from a 2 M-base genome, so that the coder has what it has on real reads"""
    rng = np.random.default_rng(18)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2 << 20, dtype=np.uint8)]
    with open(path, "wb") as f:
        for first in range(0, n, 1 << 20):
            R = min(1 << 20, n - first)
            t, cols = records(R, L, W, rng, first)
            start = rng.integers(0, len(genome) - L, R)
            seq = genome[start[:, None] + np.arange(L)[None, :]]
            err = rng.random((R, L)) < 0.01
            seq = np.where(err, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (R, L), dtype=np.uint8)], seq)
            t[:, cols] = seq
            f.write(t.tobytes())


def cli():
    os.makedirs(args.dir, exist_ok=True)
    fa, gz = os.path.join(args.dir, "reads.fasta"), os.path.join(args.dir, "reads.fasta.gz")
    write_fasta(fa, args.cli, 150, 60)
    write_bgzf(fa, gz)
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    container = fa + ".leon"
    out = {"reads": args.cli, "fasta_bytes": os.path.getsize(fa), "bgzf_bytes": os.path.getsize(gz), "cpus": len(os.sched_getaffinity(0)), "inputs": {}}
    routes = {"host": [], "device": ["-record-parse", "device", "-record-parse-fasta"]}
    for name, path, more in (("plain", fa, []), ("bgzf_input_inflate_device", gz, ["-input-inflate", "device"])):
        wall, reader, digest, lines = {"host": [], "device": []}, {"host": [], "device": []}, {}, {}
        for rep in range(args.pairs):
            for route in ("host", "device"):
                if os.path.exists(container):
                    os.remove(container)
                t = time.time()
                r = subprocess.run([leon, "-c", "-verbose", "1", "-file", path] + routes[route] + more, capture_output=True, text=True)
                wall[route].append(round(time.time() - t, 2))
                assert r.returncode == 0, (route, r.stderr[-400:])
                m = re.search(r"waited for the reader ([0-9.e+-]+) s", r.stdout)
                reader[route].append(round(float(m.group(1)), 2) if m else None)
                print("%s %s: %.2f s, reader %s" % (name, route, wall[route][-1], reader[route][-1]), file=sys.stderr, flush=True)
                if rep == 0:
                    digest[route] = hashlib.sha256(open(container, "rb").read()).hexdigest()
                    lines[route] = [l for l in r.stdout.splitlines() if l.startswith(("time:", "input:", "parse:", "the pass over the file:"))]
        out["inputs"][name] = {"wall_s": wall, "waited_for_the_reader_s": reader, "same_container": digest["host"] == digest["device"], "verbose": lines}
    for f in (fa, gz, container):
        if os.path.exists(f):
            os.remove(f)
    print(json.dumps(out))


main() if args.kernel else cli()
