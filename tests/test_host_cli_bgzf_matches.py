"""-m gpu: `leon -d -gz -gz-matches` through the built binary: X.d.gz is BGZF whose members k_deflate_lz_chunks wrote
-- smaller than `-gz` alone writes, read back by gzip member by member, the same bytes whoever formatted the records and however many
rounds the text came in, record-aligned and indexed like `-gz-records -gz-index` --, `leon -c -input-inflate device` reads it (the
device inflate on distance codes a device wrote), the option alone is refused and a failed run leaves nothing behind."""
import gzip
import os
import shutil

import numpy as np
import pytest

import bgzf_check as B
import bgzf_records as R
import container_patch as P
from test_host_cli_bgzf import ALL_DEVICE, LEON, _reads, _write_fastq, compress, decode_gz, run
from test_host_cli_bgzf_records import decode, fastq_offsets

pytestmark = pytest.mark.gpu

LINE = "output: BGZF on the device (k_deflate_lz_chunks, k_bgzf_members), "


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """the 110 000 x 70 FASTQ of three read blocks, its lossless container, the .d.gz of `-gz` and of `-gz -gz-matches`, everything
    on the device"""
    d = tmp_path_factory.mktemp("bgzf_matches")
    reads, heads, quals = _reads(110000, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(d / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    runs, _ = decode_gz(container, *ALL_DEVICE)
    gz, r = decode_gz(container, "-gz-matches", *ALL_DEVICE)
    return dict(dir=d, fq=fq, original=original, container=container, gz=gz, runs=runs, log=r.stdout)


def test_round_trip_member_by_member_and_smaller(three_blocks):
    T = three_blocks
    assert gzip.decompress(T["gz"]) == T["original"]
    payloads = B.check(T["gz"], T["original"])
    n = (len(T["original"]) + B.MEMBER_TEXT - 1) // B.MEMBER_TEXT
    assert len(payloads) == n
    B.check(T["runs"], T["original"])
    print("%d bytes of FASTQ, %d members: -gz %d bytes, -gz -gz-matches %d bytes (%.4f)"
          % (len(T["original"]), n, len(T["runs"]), len(T["gz"]), len(T["gz"]) / len(T["runs"])))
    assert len(T["gz"]) < len(T["runs"])
    # -verbose 1 says which encoder wrote the members
    lines = [l for l in T["log"].splitlines() if l.startswith("output: ")]
    assert lines == [LINE + "%d member(s), %d -> %d bytes" % (n, len(T["original"]), len(T["gz"]))], T["log"]


@pytest.mark.parametrize("env,opts", [({}, ["-record-text", "host", "-header-text", "host"]),
                                      ({}, ["-record-text", "device", "-header-text", "host"]),
                                      ({}, ["-record-text", "host", "-header-text", "device"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "device", "-header-text", "device"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "host"])],
                         ids=["host-host", "device-host", "host-device", "rounds-device", "rounds-host"])
def test_same_file_whoever_formats_and_however_many_rounds(three_blocks, env, opts):
    got, r = decode_gz(three_blocks["container"], "-gz-matches", *opts, env=dict(os.environ, **env))
    if env:
        assert "(3 round(s);" in r.stdout, r.stdout
    assert got == three_blocks["gz"]


@pytest.mark.parametrize("opts", [ALL_DEVICE, ["-record-text", "host"]], ids=["device", "host"])
def test_records_and_index(three_blocks, opts):
    """every index entry points at a member's first byte, and the text from its offset on -- a record start -- is what that member holds"""
    T = three_blocks
    gz, gzi, r = decode(T["container"], "-gz-matches", "-gz-records", "-gz-index", *opts)
    off = fastq_offsets(T["original"])
    table = R.check_records(gz, T["original"], off)
    assert gzi == R.gzi_bytes(table)
    entries = R.check_gzi(gzi, gz, T["original"])
    assert entries == [(at, a) for at, a, _ in table[1:]] and {a for _, a in entries} <= set(off)
    assert [l for l in r.stdout.splitlines() if l.startswith("output: ")][0].startswith(LINE) and "record-aligned, index " in r.stdout
    plain, plain_gzi, _ = decode(T["container"], "-gz-records", "-gz-index", *opts)
    assert len(gz) < len(plain) and [a for _, a in R.read_gzi(plain_gzi)] == [a for _, a in entries]       # the same cuts, smaller members


def test_c_reads_its_own_output_with_the_device_inflate(three_blocks, tmp_path):
    """k_bgzf_inflate on distance codes a device wrote: the container made from the file is the one made from the plain FASTQ"""
    T = three_blocks
    again = str(tmp_path / "SRR.fastq.gz")
    with open(again, "wb") as f:
        f.write(T["gz"])
    r = run(LEON, "-c", "-lossless", "-file", again, "-kmer-size", "25", "-verbose", "1", "-input-inflate", "device", "-record-parse", "device")
    assert r.returncode == 0, r.stderr
    assert "k_bgzf_inflate" in r.stdout, r.stdout
    assert open(str(tmp_path / "SRR.fastq.leon"), "rb").read() == open(T["container"], "rb").read()


def test_the_option_belongs_to_gz(three_blocks):
    T = three_blocks
    out = T["container"][:-5] + ".d"
    for p in (out, out + ".gz"):
        if os.path.exists(p):
            os.remove(p)
    r = run(LEON, "-d", "-gz-matches", "-file", T["container"])
    assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: option -gz-matches belongs to -gz"], r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".gz")


def test_checksum_mismatch_leaves_nothing(three_blocks, tmp_path):
    T = three_blocks
    fq = str(tmp_path / "sum.fastq")
    shutil.copy(T["fq"], fq)
    container = compress(fq, "-lossless", "-checksum")
    good, _ = decode_gz(container, "-gz-matches", *ALL_DEVICE)
    assert good == T["gz"]
    table, at = P.find_dataset(container, "leon/metadata/checksums", np.uint64)
    word = 1 + 3 * 1 + 0
    P.flip_bit(container, at + 8 * word + 2, bit=5)
    stored, restored = int(table[word]) ^ (1 << 21), int(table[word])
    text = "checksum: dna block 1 does not match what was compressed (stored 0x%08x, restored 0x%08x)" % (stored, restored)
    for opts in (ALL_DEVICE, []):
        out, r = decode_gz(container, "-gz-matches", *opts, expect=1)
        assert r.stderr.splitlines() == ["EXCEPTION: " + text], (opts, r.stderr)
        assert out is None, "a failed run left its output behind"
        assert sorted(os.listdir(str(tmp_path))) == ["sum.fastq", "sum.fastq.leon"]
