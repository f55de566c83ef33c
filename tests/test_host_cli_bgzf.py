"""-m gpu: `leon -d -gz` through the built binary: X.d.gz is BGZF that gzip reads back to the original, the same bytes whoever formatted
the records and however many rounds the text came in (the carry between rounds), judged member by member by tests/bgzf_check.py; plain
`-d` is what it was; a failed run leaves nothing behind."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_check as B
import common
import container_patch as P
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

ALL_DEVICE = ["-record-text", "device", "-header-text", "device", "-qual-inflate", "device"]
LINE = "output: BGZF on the device (k_deflate_chunks, k_bgzf_members), "


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def _reads(n, L, seed, **kw):
    bases, off = common.synthetic(n, L, 6000, seed=seed, **kw)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    heads = H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    return reads, heads, quals


def _write_fastq(path, reads, heads, quals, plus=lambda i, h: b""):
    with open(path, "wb") as f:
        for i, (h, s, q) in enumerate(zip(heads, reads, quals)):
            f.write(b"@" + h + b"\n" + s + b"\n+" + plus(i, h) + b"\n" + q + b"\n")
    return open(path, "rb").read()


def compress(path, *opts):
    r = run(LEON, "-c", "-file", path, "-kmer-size", "25", *opts)
    assert r.returncode == 0, r.stderr
    return path + ".leon"


def decode_gz(container, *opts, env=None, expect=0):
    """(bytes of X.d.gz or None, the run)"""
    out = container[:-5] + ".d.gz"
    for p in (out, out + ".tmp"):
        if os.path.exists(p):
            os.remove(p)
    r = run(LEON, "-d", "-gz", "-file", container, "-verbose", "1", *opts, env=env)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    assert not os.path.exists(out + ".tmp"), "the temporary file was left behind"
    return (open(out, "rb").read() if os.path.exists(out) else None), r


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """the 110 000 x 70 FASTQ of three read blocks, its lossless container, and the .d.gz of a run with everything on the device"""
    d = tmp_path_factory.mktemp("bgzf")
    reads, heads, quals = _reads(110000, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(d / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    gz, r = decode_gz(container, *ALL_DEVICE)
    return dict(dir=d, fq=fq, original=original, container=container, gz=gz, log=r.stdout)


def test_round_trip_member_by_member(three_blocks):
    T = three_blocks
    assert gzip.decompress(T["gz"]) == T["original"]
    payloads = B.check(T["gz"], T["original"])
    n = (len(T["original"]) + B.MEMBER_TEXT - 1) // B.MEMBER_TEXT
    assert len(payloads) == n
    # -verbose 1 names the kernels, the members and both sizes
    lines = [l for l in T["log"].splitlines() if l.startswith("output: ")]
    assert lines == [LINE + "%d member(s), %d -> %d bytes" % (n, len(T["original"]), len(T["gz"]))], T["log"]
    assert "written to " + T["container"][:-5] + ".d.gz" in T["log"]


@pytest.mark.parametrize("record", ["host", "device"])
@pytest.mark.parametrize("header", ["host", "device"])
def test_same_file_whoever_formats(three_blocks, record, header):
    got, r = decode_gz(three_blocks["container"], "-record-text", record, "-header-text", header)
    assert got == three_blocks["gz"]
    assert ("record text: device (k_fmt_records)" in r.stdout) == (record == "device"), r.stdout


@pytest.mark.parametrize("env,opts", [(dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "device", "-header-text", "device"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "host"]),
                                      (dict(LEON_DECODE_BLOCKS="1", LEON_DECODE_DNA_ROUNDS="2"), ALL_DEVICE),
                                      (dict(LEON_DECODE_BLOCKS="1", LEON_BGZF_SLICE="1000000"), ["-record-text", "host", "-qual-inflate", "device"])],
                         ids=["rounds-device", "rounds-host", "rounds-two-per-call", "rounds-host-small-pieces"])
def test_same_file_however_many_rounds(three_blocks, env, opts):
    """three rounds of one block: no round's text is a multiple of 32 768, so the second and third begin with a carry"""
    got, r = decode_gz(three_blocks["container"], *opts, env=dict(os.environ, **env))
    assert "(3 round(s);" in r.stdout, r.stdout
    assert got == three_blocks["gz"]


def test_test_file_and_plain_d(three_blocks):
    T = three_blocks
    r = run(LEON, "-d", "-gz", "-test-file", "-file", T["container"], *ALL_DEVICE)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr
    # without the option: the plain .d, the bytes of the original, and no .d.gz of its own
    os.remove(T["container"][:-5] + ".d.gz")
    for opts in ([], ALL_DEVICE):
        r = run(LEON, "-d", "-file", T["container"], "-verbose", "1", *opts)
        assert r.returncode == 0, r.stderr
        assert open(T["fq"] + ".d", "rb").read() == T["original"]
        assert "output: BGZF" not in r.stdout and not os.path.exists(T["container"][:-5] + ".d.gz")


def test_own_output_is_read_by_c(three_blocks, tmp_path):
    """the reader of -c (gzread) takes the file -d -gz wrote"""
    T = three_blocks
    again = str(tmp_path / "Y.fastq.gz")
    with open(again, "wb") as f:
        f.write(T["gz"])
    r = run(LEON, "-c", "-lossless", "-file", again, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    r = run(LEON, "-d", "-file", str(tmp_path / "Y.fastq.leon"))
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "Y.fastq.d"), "rb").read() == T["original"]


def test_lossy_container(three_blocks):
    T = three_blocks
    lossy = str(T["dir"] / "lossy.fastq")
    shutil.copy(T["fq"], lossy)
    container = compress(lossy)
    r = run(LEON, "-d", "-file", container)
    assert r.returncode == 0, r.stderr
    plain = open(lossy + ".d", "rb").read()
    assert len(plain) == len(T["original"]) and plain != T["original"]
    for opts in (ALL_DEVICE, []):
        got, _ = decode_gz(container, *opts)
        B.check(got, plain)


def test_wrapped_fasta(tmp_path):
    lens = (59, 60, 61, 120, 121)
    bases, off = common.synthetic(2500, 121, 6000, seed=24)
    fa = str(tmp_path / "wrapped.fa")
    with open(fa, "wb") as f:
        for i in range(2500):
            s = bases[int(off[i]):int(off[i]) + lens[i % 5]]
            f.write(b">read_%d some text\n" % i + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60)))
    original = open(fa, "rb").read()
    r = run(LEON, "-file", fa, "-c", "-kmer-size", "21", "-abundance", "2")
    assert r.returncode == 0, r.stderr
    files = [decode_gz(fa + ".leon", *opts)[0] for opts in ([], ["-record-text", "device"], ALL_DEVICE[:4])]
    B.check(files[0], original)
    assert files[1] == files[0] and files[2] == files[0]
    r = run(LEON, "-d", "-gz", "-test-file", "-file", fa + ".leon", "-record-text", "device")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_mixed_plus_lines_are_formatted_on_the_host(tmp_path):
    reads, heads, quals = _reads(60000, 50, seed=22)               # two read blocks
    fp = str(tmp_path / "plus_mixed.fastq")
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: (b"", h, b"", b"", h, b"free text %d" % i)[i % 6] if i % 1000 < 6 else h)
    container = compress(fp, "-lossless")
    got, r = decode_gz(container, *ALL_DEVICE, env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert "record text: host threads (the '+' lines are mixed" in r.stdout, r.stdout
    B.check(got, original)
    assert decode_gz(container)[0] == got


def test_checksum_mismatch_leaves_nothing(three_blocks, tmp_path):
    """one bit of block 1's DNA word in a -checksum container: -d -gz ends with the checksum's words and neither X.d.gz nor its
    temporary file is left"""
    T = three_blocks
    fq = str(tmp_path / "sum.fastq")
    shutil.copy(T["fq"], fq)
    container = compress(fq, "-lossless", "-checksum")
    good, _ = decode_gz(container, *ALL_DEVICE)
    assert good == T["gz"]
    table, at = P.find_dataset(container, "leon/metadata/checksums", np.uint64)
    word = 1 + 3 * 1 + 0
    P.flip_bit(container, at + 8 * word + 2, bit=5)
    stored, restored = int(table[word]) ^ (1 << 21), int(table[word])
    text = "checksum: dna block 1 does not match what was compressed (stored 0x%08x, restored 0x%08x)" % (stored, restored)
    for opts in (ALL_DEVICE, []):
        out, r = decode_gz(container, *opts, expect=1)
        assert r.stderr.splitlines() == ["EXCEPTION: " + text], (opts, r.stderr)
        assert out is None, "a failed run left its output behind"
        assert sorted(os.listdir(str(tmp_path))) == ["sum.fastq", "sum.fastq.leon"]
