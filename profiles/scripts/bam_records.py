"""Unaligned BAM records on the device (k_bam_sizes, k_bam_records) beside the record text (k_fmt_sizes, k_fmt_records)
on the same reads.

  bam_records.py --kernel N    N synthetic FASTQ records x 150 bp with SRA-style headers in device memory (record_text.py's); one warm-up
                               call of each formatter on a slice, then TWO whole calls of leon_records_format_device and TWO of
                               leon_records_bam_device; the first and last 1 000 BAM records checked against tests/bam_records.py.  The run
                               to put under `rocprofv3 --kernel-trace --stats` (kernel times come from there; the JSON line carries both
                               outputs' bytes and the calls' wall time)
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import bam_records as BAM  # noqa: E402
from leon_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", type=int, required=True)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda", 0)

N, L = args.kernel, 150
blob, hoff = bench.sra_headers(N, seed=7)
g = torch.Generator(device=dev); g.manual_seed(5)
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
d_bases = torch.empty(N * L, dtype=torch.uint8, device=dev)
d_quals = torch.empty(N * L, dtype=torch.uint8, device=dev)
step = 1 << 28                                                    # (random integers come as 64-bit words: a slice at a time)
for a in range(0, N * L, step):
    m = min(step, N * L - a)
    d_bases[a:a + m] = acgt[torch.randint(0, 4, (m,), device=dev, generator=g)]
    d_quals[a:a + m] = (torch.randint(0, 41, (m,), device=dev, generator=g) + 33).to(torch.uint8)
d_len = torch.full((N,), L, dtype=torch.int32, device=dev)
d_hdr = torch.from_numpy(blob).to(dev)
d_hoff = torch.from_numpy(hoff).to(dev)
hdr_bytes = int(hoff[-1])
text_size = 2 * N + hdr_bytes + N * (L + 1) + N * (3 + L)
d_out = torch.empty(text_size + 64, dtype=torch.uint8, device=dev)       # (a record's text is larger than its BAM record at this length)
d_rec = torch.empty(N + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()


def call(which, n):
    kw = dict(fastq=True, d_hdr_text=d_hdr.data_ptr(), d_hdr_off=d_hoff.data_ptr(), hdr_bytes=int(hoff[n] - hoff[0]), d_quals=d_quals.data_ptr(),
              d_rec_off=d_rec.data_ptr())
    t0 = time.perf_counter()
    if which == "text":
        size = capi.records_format_device(d_bases.data_ptr(), d_len.data_ptr(), n, n * L, d_out.data_ptr(), text_size, lead=b"@", **kw)
    else:
        size = capi.records_bam_device(d_bases.data_ptr(), d_len.data_ptr(), n, n * L, d_out.data_ptr(), text_size, **kw)
    return size, (time.perf_counter() - t0) * 1e3


out = {"records": N, "read_len": L, "header_bytes": hdr_bytes}
for which in ("text", "bam"):
    call(which, min(N, 1000))                                     # (code objects loaded)
    ms = []
    for _ in range(2):
        size, dt = call(which, N)
        ms.append(round(dt, 2))
    out[which + "_bytes"] = size
    out[which + "_call_ms"] = ms
assert out["text_bytes"] == text_size
# the first and the last 1 000 BAM records against the restatement (the last call was the BAM formatter's)
rec_off = d_rec.cpu().numpy().astype(np.uint64)
k = min(N, 1000)
for lo in (0, N - k):
    bases = d_bases[lo * L:(lo + k) * L].cpu().numpy().tobytes()
    quals = d_quals[lo * L:(lo + k) * L].cpu().numpy().tobytes()
    heads = [blob[int(hoff[lo + i]):int(hoff[lo + i + 1])].tobytes() for i in range(k)]
    want, _ = BAM.bam_records([bases[i * L:(i + 1) * L] for i in range(k)], heads, [quals[i * L:(i + 1) * L] for i in range(k)], lo)
    at = int(rec_off[lo])
    assert int(rec_off[lo + k]) - at == len(want) and d_out[at:at + len(want)].cpu().numpy().tobytes() == want, "the records differ from the restatement near read %d" % lo
out["note"] = "kernel times: the rocprofv3 --kernel-trace --stats run around this process"
print(json.dumps(out))
