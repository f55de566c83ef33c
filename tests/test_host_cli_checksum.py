"""-m gpu: block checksums through the built binary.  `leon -c -checksum` writes leon/metadata/checksums -- zlib's CRC-32 per read block
of the bases, the headers and the qualities, pinned here by Python's zlib.crc32 -- and `leon -d` verifies it whenever it is there,
whichever way (device or host threads) each stream was restored.  A container changed from outside (container_patch.py) ends -d with
the block and stream by name; the same change in a container without the table goes unnoticed: that contrast is the feature."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import common
import container_patch as P
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

RPB = 50000                                                        # reads per block
TABLE = "leon/metadata/checksums"
STREAMS = ("dna", "header", "quality")
WAYS = {"host": "host threads", "device": "device"}
ALL_DEVICE = ["-record-text", "device", "-header-text", "device", "-qual-inflate", "device"]
ALL_HOST = ["-record-text", "host", "-header-text", "host", "-qual-inflate", "host"]


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def make_reads(n, seed, lo=36, hi=70):
    """n reads of lo..hi bases, SRA-style headers, qualities of the reads' lengths"""
    bases, off = common.synthetic(n, hi, 6000, seed=seed, n_rate=0.002, err=0.02)
    lens = np.random.default_rng(seed).integers(lo, hi + 1, n)
    reads = [bases[int(off[i]):int(off[i]) + int(lens[i])] for i in range(n)]
    heads = H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    return reads, heads, quals


def write_fastq(path, reads, heads, quals):
    with open(path, "wb") as f:
        for h, s, q in zip(heads, reads, quals):
            f.write(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
    return open(path, "rb").read()


def block_sums(items):
    return [zlib.crc32(b"".join(items[b:b + RPB])) for b in range(0, len(items), RPB)]


def table_of(container):
    t = P.h5_dataset(container, TABLE, np.uint64)
    assert t[0] == 1 and (len(t) - 1) % 3 == 0, t[:4]
    return t[1:].reshape(-1, 3)


def compress(fq, *opts):
    r = run(LEON, "-c", "-file", fq, "-kmer-size", "25", *opts)
    assert r.returncode == 0, r.stderr
    return fq + ".leon", r.stdout


def decode(container, *opts, expect=0):
    out = container[:-5] + ".d"
    if os.path.exists(out):
        os.remove(out)
    r = run(LEON, "-d", "-file", container, "-verbose", "1", *opts)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    return (open(out, "rb").read() if os.path.exists(out) else None), r


def verified_line(log):
    lines = [l for l in log.splitlines() if l.startswith("checksums: ")]
    assert len(lines) == 1, log
    return lines[0]


def quals_of(text):
    return text.split(b"\n")[3::4]


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """110 000 reads (three blocks): the lossless container without the table (before and after -checksum was used), with it, and the
    lossy container with it"""
    d = tmp_path_factory.mktemp("checksum")
    reads, heads, quals = make_reads(2 * RPB + 10000, seed=31)
    fq = str(d / "SRR.fastq")
    original = write_fastq(fq, reads, heads, quals)
    container, _ = compress(fq, "-lossless")
    before = open(container, "rb").read()
    container, log = compress(fq, "-lossless", "-checksum")
    assert "checksums: CRC-32 of 3 blocks (dna, header, quality)" in log, log
    lossless = str(d / "lossless.fastq.leon")
    shutil.copy(container, lossless)
    container, _ = compress(fq, "-lossless")
    plain = str(d / "plain.fastq.leon")
    shutil.copy(container, plain)
    container, _ = compress(fq, "-checksum")
    lossy = str(d / "lossy.fastq.leon")
    shutil.copy(container, lossy)
    return dict(reads=reads, heads=heads, quals=quals, original=original, before=before, lossless=lossless, plain=plain, lossy=lossy, dir=d)


def test_table_is_zlib_crc32_of_the_original(three_blocks):
    T = three_blocks
    t = table_of(T["lossless"])
    assert t.shape == (3, 3)
    assert t[:, 0].tolist() == block_sums(T["reads"])
    assert t[:, 1].tolist() == block_sums(T["heads"])
    assert t[:, 2].tolist() == block_sums(T["quals"])


def test_lossy_table_covers_the_stored_qualities(three_blocks):
    T = three_blocks
    t = table_of(T["lossy"])
    assert t[:, 0].tolist() == block_sums(T["reads"]) and t[:, 1].tolist() == block_sums(T["heads"])
    restored, r = decode(T["lossy"])
    smoothed = quals_of(restored)[:len(T["quals"])]
    assert smoothed != T["quals"], "the lossy mode left every quality as it was: the case shows nothing"
    assert t[:, 2].tolist() == block_sums(smoothed)
    assert "checksums: 3 blocks verified" in r.stdout


def test_without_the_option_nothing_changes(three_blocks):
    T = three_blocks
    assert not P.h5_has(T["plain"], TABLE) and P.h5_has(T["lossless"], TABLE)
    assert open(T["plain"], "rb").read() == T["before"], "-c without -checksum no longer writes what it wrote before the option was used"
    restored, r = decode(T["plain"], *ALL_DEVICE)
    assert restored == T["original"] and "checksums:" not in r.stdout


@pytest.mark.parametrize("record", ["host", "device"])
@pytest.mark.parametrize("header", ["host", "device"])
def test_every_way_verifies_and_says_where(three_blocks, record, header):
    T = three_blocks
    for inflate in ("host", "device"):
        restored, r = decode(T["lossless"], "-record-text", record, "-header-text", header, "-qual-inflate", inflate)
        assert restored == T["original"], (record, header, inflate)
        assert verified_line(r.stdout) == "checksums: 3 blocks verified (dna: %s, header: %s, quality: %s)" % (WAYS[record], WAYS[header], WAYS[inflate]), r.stdout
    if record == header:
        # rounds of one block: every round is verified, the smallest block first
        env = dict(os.environ, LEON_DECODE_BLOCKS="1")
        out = T["lossless"][:-5] + ".d"
        r = run(LEON, "-d", "-file", T["lossless"], "-verbose", "1", "-record-text", record, "-header-text", header, "-qual-inflate", record, env=env)
        assert r.returncode == 0 and open(out, "rb").read() == T["original"], r.stderr
        assert verified_line(r.stdout).startswith("checksums: 3 blocks verified (dna: %s," % WAYS[record])


def test_lossy_container_both_ways(three_blocks):
    T = three_blocks
    host, r = decode(T["lossy"], *ALL_HOST)
    assert verified_line(r.stdout) == "checksums: 3 blocks verified (dna: host threads, header: host threads, quality: host threads)"
    device, r = decode(T["lossy"], *ALL_DEVICE)
    assert verified_line(r.stdout) == "checksums: 3 blocks verified (dna: device, header: device, quality: device)"
    assert host == device and len(host) == len(T["original"])


def test_absent_streams_hold_zero(three_blocks, tmp_path):
    T = three_blocks
    fq = str(tmp_path / "seq.fastq")
    write_fastq(fq, T["reads"][:60000], T["heads"][:60000], T["quals"][:60000])
    container, log = compress(fq, "-seq-only", "-checksum")
    assert "checksums: CRC-32 of 2 blocks (dna)" in log
    t = table_of(container)
    assert t[:, 0].tolist() == block_sums(T["reads"][:60000]) and t[:, 1].tolist() == [0, 0] and t[:, 2].tolist() == [0, 0]
    for opts in (ALL_HOST, ALL_DEVICE):
        restored, r = decode(container, *opts)
        assert restored == b"".join(b">%d\n" % i + s + b"\n" for i, s in enumerate(T["reads"][:60000]))
        assert verified_line(r.stdout) == "checksums: 2 blocks verified (dna: %s, header: not stored, quality: not stored)" % WAYS[opts[1]]
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for h, s in zip(T["heads"][:3000], T["reads"][:3000]):
            f.write(b">" + h + b"\n" + s + b"\n")
    container, _ = compress(fa, "-checksum")
    t = table_of(container)
    assert t.tolist() == [[zlib.crc32(b"".join(T["reads"][:3000])), zlib.crc32(b"".join(T["heads"][:3000])), 0]]
    for opts in (ALL_HOST, ALL_DEVICE):
        restored, r = decode(container, *opts)
        assert restored == open(fa, "rb").read()
        assert verified_line(r.stdout) == "checksums: 1 blocks verified (dna: %s, header: %s, quality: not stored)" % (WAYS[opts[1]], WAYS[opts[3]])


@pytest.mark.parametrize("column", [0, 1, 2], ids=STREAMS)
def test_tamper_with_the_table(three_blocks, tmp_path, column):
    """one bit of block 1's word of one stream: -d names the stream and the block, the same text whichever way restored it"""
    T = three_blocks
    container = str(tmp_path / "flipped.fastq.leon")
    shutil.copy(T["lossless"], container)
    table, at = P.find_dataset(container, TABLE, np.uint64)
    word = 1 + 3 * 1 + column
    P.flip_bit(container, at + 8 * word + 2, bit=5)                # bit 21 of the word
    stored, restored = int(table[word]) ^ (1 << 21), int(table[word])
    assert int(P.h5_dataset(container, TABLE, np.uint64)[word]) == stored
    text = "checksum: %s block 1 does not match what was compressed (stored 0x%08x, restored 0x%08x)" % (STREAMS[column], stored, restored)
    for opts in (ALL_DEVICE, ALL_HOST):
        out, r = decode(container, *opts, expect=1)
        assert r.stderr.splitlines() == ["EXCEPTION: " + text], (opts, r.stderr)
        assert out is None, "a failed run left its output behind"
    out, r = decode(container, "-ignore-checksum", *ALL_DEVICE)
    assert out == T["original"]
    assert r.stderr.splitlines() == ["WARNING: " + text], r.stderr
    assert verified_line(r.stdout).endswith("1 mismatch(es) ignored (-ignore-checksum)")


def test_table_of_another_kind_and_misplaced_options(three_blocks, tmp_path):
    T = three_blocks
    container = str(tmp_path / "kind.fastq.leon")
    shutil.copy(T["lossless"], container)
    _, at = P.find_dataset(container, TABLE, np.uint64)
    P.patch(container, at, (7).to_bytes(8, "little"))
    out, r = decode(container, expect=1)
    assert r.stderr.startswith("EXCEPTION: ") and "unknown checksum kind 7 in leon/metadata/checksums" in r.stderr and out is None, r.stderr
    # the options are refused where they do not belong, while the arguments are parsed
    for args in (["-d", "-checksum"], ["-c", "-ignore-checksum"]):
        r = run(LEON, "-file", T["lossless"], *args)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: option -"), (args, r.stderr)


@pytest.mark.parametrize("with_table", [True, False], ids=["with the table", "without it"])
def test_swapped_quality_payloads(tmp_path, with_table):
    """two quality blocks that are valid zlib streams of the wrong text: equal lengths, so every size in the container still holds.
    With the table -d names quality block 0; without it the same swap decodes, exit 0, to a wrong file: that contrast is the feature."""
    n, L = 2 * RPB, 36
    reads, heads, _ = make_reads(n, seed=32, lo=L, hi=L)
    quals = [b"I" * L] * RPB + [b"H" * L] * RPB
    pay = [zlib.compress((c * L + b"\n") * RPB) for c in (b"I", b"H")]
    assert len(pay[0]) == len(pay[1]) and pay[0] != pay[1]
    fq = str(tmp_path / "flat.fastq")
    original = write_fastq(fq, reads, heads, quals)
    container, _ = compress(fq, "-lossless", *(["-checksum"] if with_table else []))
    assert P.h5_has(container, TABLE) == with_table
    at = [P.find_bytes(container, p) for p in pay]
    P.patch(container, at[0], pay[1])
    P.patch(container, at[1], pay[0])
    for ways in (ALL_HOST, ALL_DEVICE):
        out, r = decode(container, *ways, expect=1 if with_table else 0)
        if with_table:
            assert out is None and r.stderr.splitlines() == ["EXCEPTION: checksum: quality block 0 does not match what was compressed (stored 0x%08x, restored 0x%08x)"
                                                             % (zlib.crc32(b"I" * L * RPB), zlib.crc32(b"H" * L * RPB))], r.stderr
        else:
            assert out is not None and out != original and len(out) == len(original) and "checksums:" not in r.stdout
            assert quals_of(out)[:n] == quals[RPB:] + quals[:RPB]


def test_lower_case_input(tmp_path):
    """a lower-case letter comes back as N: the table says so (dna block 0), and -ignore-checksum still restores the file"""
    reads, heads, quals = make_reads(3000, seed=33)
    reads = [r[:5] + r[5:9].lower() + r[9:] if i % 500 == 7 else r for i, r in enumerate(reads)]
    fq = str(tmp_path / "lower.fastq")
    write_fastq(fq, reads, heads, quals)
    container, _ = compress(fq, "-lossless", "-checksum")
    t = table_of(container)
    assert t[0, 0] == zlib.crc32(b"".join(reads))
    restored = b"".join(bytes(c if c in b"ACGTN" else ord("N") for c in r) for r in reads)
    for ways in (ALL_HOST, ALL_DEVICE):
        out, r = decode(container, *ways, expect=1)
        assert out is None and r.stderr.splitlines() == ["EXCEPTION: checksum: dna block 0 does not match what was compressed (stored 0x%08x, restored 0x%08x)" % (
            zlib.crc32(b"".join(reads)), zlib.crc32(restored))], r.stderr
    out, r = decode(container, "-ignore-checksum")
    assert r.stderr.startswith("WARNING: checksum: dna block 0 does not match")
    assert out.split(b"\n")[1::4][:3000] == [bytes(c if c in b"ACGTN" else ord("N") for c in r) for r in reads]
    assert out.split(b"\n")[3::4][:3000] == quals
