"""-m gpu: `leon -d -gz -gz-records -gz-index` through the built binary: X.d.gz holds members that begin at record starts and X.d.gz.gzi
lists them, the same two files whoever formatted the records and however many rounds the text came in, judged by tests/bgzf_records.py
against record offsets parsed from the plain `-d` output; `-gz-index` alone indexes the fixed cuts; `-d -gz` alone is what it was; `-c`
reads the record-aligned file back; a failed run leaves neither file."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_check as B
import bgzf_records as R
import common
from test_host_cli_bgzf import ALL_DEVICE, LEON, LINE, _reads, _write_fastq, compress, run

pytestmark = pytest.mark.gpu

BOTH = ["-gz-records", "-gz-index"]


def decode(container, *opts, env=None, expect=0):
    """`leon -d -gz` with opts: (bytes of X.d.gz or None, bytes of X.d.gz.gzi or None, the run)"""
    out = container[:-5] + ".d.gz"
    for p in (out, out + ".tmp", out + ".gzi", out + ".gzi.tmp"):
        if os.path.isfile(p):
            os.remove(p)
    r = run(LEON, "-d", "-gz", "-file", container, "-verbose", "1", *opts, env=env)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    assert not os.path.isfile(out + ".tmp") and not os.path.isfile(out + ".gzi.tmp"), "a temporary file was left behind"
    read = lambda p: open(p, "rb").read() if os.path.isfile(p) else None
    return read(out), read(out + ".gzi"), r


def plain(container):
    r = run(LEON, "-d", "-file", container)
    assert r.returncode == 0, r.stderr
    return open(container[:-5] + ".d", "rb").read()


def fastq_offsets(text):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert len(nl) % 4 == 0
    return [0] + (nl[3::4] + 1).tolist()


def fasta_offsets(text):
    a = np.frombuffer(text, dtype=np.uint8)
    starts = np.flatnonzero((a == ord(">")) & np.concatenate([[True], a[:-1] == 10]))
    return starts.tolist() + [len(text)]


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """the 110 000 x 70 FASTQ of three read blocks, its lossless container, its plain -d output and that text's record offsets, and the
    .d.gz and .gzi of a run with everything on the device"""
    d = tmp_path_factory.mktemp("bgzf_records")
    reads, heads, quals = _reads(110000, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(d / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    text = plain(container)
    assert text == original
    gz, gzi, r = decode(container, *BOTH, *ALL_DEVICE)
    return dict(dir=d, fq=fq, text=text, off=fastq_offsets(text), container=container, gz=gz, gzi=gzi, log=r.stdout)


def test_members_begin_at_record_starts_and_the_index_lists_them(three_blocks):
    T = three_blocks
    assert gzip.decompress(T["gz"]) == T["text"]
    table = R.check_records(T["gz"], T["text"], T["off"])
    assert T["gzi"] == R.gzi_bytes(table)
    assert R.check_gzi(T["gzi"], T["gz"], T["text"]) == [(at, a) for at, a, _ in table[1:]]
    lines = [l for l in T["log"].splitlines() if l.startswith("output: ")]
    assert lines == [LINE + "%d member(s), %d -> %d bytes, record-aligned, index %s.d.gz.gzi (%d entries)"
                     % (len(table), len(T["text"]), len(T["gz"]), T["container"][:-5], len(table) - 1)], T["log"]


@pytest.mark.parametrize("env,opts", [({}, ["-record-text", "host"]),
                                      ({}, ["-record-text", "device", "-header-text", "host"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "device", "-header-text", "device"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "host"]),
                                      (dict(LEON_DECODE_BLOCKS="1", LEON_DECODE_DNA_ROUNDS="2"), ALL_DEVICE),
                                      (dict(LEON_DECODE_BLOCKS="1", LEON_BGZF_SLICE="1000000"), ["-record-text", "host", "-qual-inflate", "device"])],
                         ids=["host", "device", "rounds-device", "rounds-host", "rounds-two-per-call", "rounds-host-small-pieces"])
def test_same_files_whoever_formats_and_however_many_rounds(three_blocks, env, opts):
    gz, gzi, r = decode(three_blocks["container"], *BOTH, *opts, env=dict(os.environ, **env))
    if env:
        assert "(3 round(s);" in r.stdout, r.stdout
    assert ("record text: device (k_fmt_records)" in r.stdout) == ("device" in opts[:2] or opts is ALL_DEVICE), r.stdout
    assert gz == three_blocks["gz"] and gzi == three_blocks["gzi"]


@pytest.fixture(scope="module")
def fixed(three_blocks):
    """`-d -gz` with neither option: (the file, the index -- none --, the log)"""
    gz, gzi, r = decode(three_blocks["container"], *ALL_DEVICE)
    return gz, gzi, r.stdout


def test_neither_option_is_what_it_was(three_blocks, fixed):
    """the fixed layout, pinned by bgzf_check.check, the line of before, and no index"""
    T = three_blocks
    gz, gzi, log = fixed
    B.check(gz, T["text"])
    assert gzi is None
    n = (len(T["text"]) + B.MEMBER_TEXT - 1) // B.MEMBER_TEXT
    assert [l for l in log.splitlines() if l.startswith("output: ")] == [LINE + "%d member(s), %d -> %d bytes" % (n, len(T["text"]), len(gz))]
    print("110 000 x 70: -d -gz %d bytes, -d -gz -gz-records %d bytes (%.4f)" % (len(gz), len(T["gz"]), len(T["gz"]) / len(gz)))


@pytest.mark.parametrize("opts", [ALL_DEVICE, ["-record-text", "host"]], ids=["device", "host"])
def test_index_alone(three_blocks, fixed, opts):
    """the bytes of `-d -gz`, and an index of the fixed cuts"""
    gz, gzi, r = decode(three_blocks["container"], "-gz-index", *opts, env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert gz == fixed[0]
    walk = B.walk(gz)[:-1]
    assert R.read_gzi(gzi) == [(at, i * B.MEMBER_TEXT) for i, (at, _) in enumerate(walk)][1:]
    R.check_gzi(gzi, gz, three_blocks["text"])
    assert ", index " in r.stdout and "record-aligned" not in r.stdout


def test_records_alone(three_blocks):
    T = three_blocks
    gz, gzi, r = decode(T["container"], "-gz-records", *ALL_DEVICE)
    assert gz == T["gz"] and gzi is None and "record-aligned" in r.stdout and ", index " not in r.stdout


def test_test_file(three_blocks):
    T = three_blocks
    r = run(LEON, "-d", "-gz", *BOTH, "-test-file", "-file", T["container"], *ALL_DEVICE)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("way", [[], ["-input-inflate", "device"]], ids=["host", "input-inflate-device"])
def test_c_reads_the_record_aligned_file(three_blocks, tmp_path, way):
    """the container made from the record-aligned .gz is the one made from the plain file"""
    T = three_blocks
    again = str(tmp_path / "SRR.fastq.gz")
    with open(again, "wb") as f:
        f.write(T["gz"])
    r = run(LEON, "-c", "-lossless", "-file", again, "-kmer-size", "25", "-verbose", "1", *way)
    assert r.returncode == 0, r.stderr
    if way:
        assert "k_bgzf_inflate" in r.stdout, r.stdout
    assert open(str(tmp_path / "SRR.fastq.leon"), "rb").read() == open(T["container"], "rb").read()


def test_wrapped_fasta(tmp_path):
    lens = (59, 60, 61, 120, 121)
    bases, off = common.synthetic(2500, 121, 6000, seed=24)
    fa = str(tmp_path / "wrapped.fa")
    with open(fa, "wb") as f:
        for i in range(2500):
            s = bases[int(off[i]):int(off[i]) + lens[i % 5]]
            f.write(b">read_%d some text\n" % i + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60)))
    r = run(LEON, "-file", fa, "-c", "-kmer-size", "21", "-abundance", "2")
    assert r.returncode == 0, r.stderr
    text = plain(fa + ".leon")
    files = [decode(fa + ".leon", *BOTH, *opts)[:2] for opts in ([], ["-record-text", "device"], ALL_DEVICE[:4])]
    table = R.check_records(files[0][0], text, fasta_offsets(text))
    assert len(table) > 5 and files[0][1] == R.gzi_bytes(table)
    assert files[1] == files[0] and files[2] == files[0]


def test_mixed_plus_lines_are_formatted_on_the_host(tmp_path):
    reads, heads, quals = _reads(60000, 50, seed=22)               # two read blocks
    fp = str(tmp_path / "plus_mixed.fastq")
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: (b"", h, b"", b"", h, b"free text %d" % i)[i % 6] if i % 1000 < 6 else h)
    container = compress(fp, "-lossless")
    gz, gzi, r = decode(container, *BOTH, *ALL_DEVICE, env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert "record text: host threads (the '+' lines are mixed" in r.stdout, r.stdout
    table = R.check_records(gz, original, fastq_offsets(original))
    assert gzi == R.gzi_bytes(table)
    assert decode(container, *BOTH)[:2] == (gz, gzi)


def test_a_failed_run_leaves_neither_file(three_blocks, tmp_path):
    T = three_blocks
    container = str(tmp_path / "SRR.fastq.leon")
    shutil.copy(T["container"], container)
    # the index cannot be opened (a directory has its temporary name): the data file, already created, goes too
    os.mkdir(container[:-5] + ".d.gz.gzi.tmp")
    gz, gzi, r = decode(container, *BOTH, *ALL_DEVICE, expect=1)
    assert r.stderr.splitlines() == ["EXCEPTION: cannot write " + container[:-5] + ".d.gz.gzi"], r.stderr
    assert (gz, gzi) == (None, None) and sorted(os.listdir(str(tmp_path))) == ["SRR.fastq.d.gz.gzi.tmp", "SRR.fastq.leon"]
    os.rmdir(container[:-5] + ".d.gz.gzi.tmp")
    if os.geteuid() != 0:                                         # the output directory is not writable
        os.chmod(str(tmp_path), 0o555)
        try:
            gz, gzi, r = decode(container, *BOTH, *ALL_DEVICE, expect=1)
            assert r.stderr.startswith("EXCEPTION: cannot write "), r.stderr
            assert (gz, gzi) == (None, None) and os.listdir(str(tmp_path)) == ["SRR.fastq.leon"]
        finally:
            os.chmod(str(tmp_path), 0o755)
