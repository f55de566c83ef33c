"""-m gpu: `leon -d -bam` through the built binary: X.d.bam is BGZF whose content is the BAM header and the records of
tests/bam_records.py's restatement built from the original reads, closed by the EOF marker; the same bytes whoever formatted the records,
however many rounds they came in and whatever the slice; record-aligned and indexed like `-gz -gz-records -gz-index`; a FASTA, a
`-noheader`, a `-letters` and an empty container; a name or a quality BAM cannot hold ends the run and leaves nothing; the option rules; and
`-d -gz` and plain `-d` are what they were."""
import gzip
import os

import pytest

import bam_records as BAM
import bgzf_records as R
import common
from test_host_cli_bgzf import ALL_DEVICE, LEON, _reads, _write_fastq, compress, decode_gz, run
from test_host_cli_bgzf_records import plain

pytestmark = pytest.mark.gpu

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
N_READS = 100001                                                   # the fewest reads that make three blocks of 50 000


def decode_bam(container, *opts, env=None, expect=0):
    """`leon -d -bam` with opts: (bytes of X.d.bam or None, bytes of X.d.bam.gzi or None, the run)"""
    out = container[:-5] + ".d.bam"
    for p in (out, out + ".tmp", out + ".gzi", out + ".gzi.tmp"):
        if os.path.isfile(p):
            os.remove(p)
    r = run(LEON, "-d", "-bam", "-file", container, "-verbose", "1", *opts, env=env)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    assert not os.path.isfile(out + ".tmp") and not os.path.isfile(out + ".gzi.tmp"), "a temporary file was left behind"
    read = lambda p: open(p, "rb").read() if os.path.isfile(p) else None
    return read(out), read(out + ".gzi"), r


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """a 100 001 x 70 FASTQ of three read blocks, its lossless container, the restatement's content for it, and the .d.bam of a run with
    everything on the device"""
    d = tmp_path_factory.mktemp("bam")
    reads, heads, quals = _reads(N_READS, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(d / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    records, rec_off = BAM.bam_records(reads, heads, quals)
    head = BAM.bam_header()
    bam, _, r = decode_bam(container, *ALL_DEVICE)
    return dict(dir=d, fq=fq, original=original, container=container, reads=reads, heads=heads, quals=quals, content=head + records,
                starts=[0] + [len(head) + o for o in rec_off], bam=bam, log=r.stdout)


def test_content_is_the_restatement_and_parses_back(three_blocks):
    T = three_blocks
    content = gzip.decompress(T["bam"])
    assert content == T["content"]
    assert T["bam"].endswith(EOF_MARKER)
    parsed = BAM.parse_bam(content)
    assert len(parsed) == N_READS
    for (name, seq, qual, comment), h, s, q in zip(parsed, T["heads"], T["reads"], T["quals"]):
        assert (name, comment) == BAM.name_and_comment(h) and seq == BAM.fold(s) and qual == q
    assert any(c for _, _, _, c in parsed), "no header of the file has a comment"
    lines = [l for l in T["log"].splitlines() if l.startswith("output: ")]
    assert len(lines) == 1 and lines[0].startswith("output: BGZF on the device (k_deflate_chunks, k_bgzf_members), "), T["log"]
    assert lines[0].endswith(", %d -> %d bytes, records: BAM (device (k_bam_records), 1 round(s))" % (len(content), len(T["bam"]))), T["log"]
    assert "written to " + T["container"][:-5] + ".d.bam" in T["log"] and "record text:" not in T["log"]


@pytest.mark.parametrize("env,opts", [({}, ["-record-text", "host"]),
                                      ({}, ["-record-text", "device", "-header-text", "host"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "device", "-header-text", "device"]),
                                      (dict(LEON_DECODE_BLOCKS="1"), ["-record-text", "host"]),
                                      (dict(LEON_DECODE_BLOCKS="1", LEON_BGZF_SLICE="1000000"), ["-record-text", "host", "-qual-inflate", "device"]),
                                      (dict(LEON_BGZF_SLICE="1000000"), ALL_DEVICE)],
                         ids=["host", "device", "rounds-device", "rounds-host", "rounds-host-small-slices", "device-small-slices"])
def test_same_file_whoever_formats_however_many_rounds_whatever_the_slice(three_blocks, env, opts):
    bam, _, r = decode_bam(three_blocks["container"], *opts, env=dict(os.environ, **env))
    if "LEON_DECODE_BLOCKS" in env:
        assert "(3 round(s);" in r.stdout, r.stdout
    device = "device" in opts[:2] or opts is ALL_DEVICE
    assert ("records: BAM (device (k_bam_records), %d round(s))" % (3 if "LEON_DECODE_BLOCKS" in env else 1) in r.stdout) == device, r.stdout
    assert ("records: BAM (host threads)" in r.stdout) == (not device), r.stdout
    assert bam == three_blocks["bam"]


@pytest.mark.parametrize("opts", [ALL_DEVICE, ["-record-text", "host"]], ids=["device", "host"])
def test_records_and_index(three_blocks, opts):
    """the members are those of the cut rule over the header and the records' starts; every index entry names a member's first byte and
    a record start (or the inside of an oversized record: there is none here); -gz-matches changes the members' bytes alone"""
    T = three_blocks
    env = dict(os.environ, LEON_DECODE_BLOCKS="1", LEON_BGZF_SLICE="1000000")
    bam, gzi, r = decode_bam(T["container"], "-gz-records", "-gz-index", *opts, env=env)
    table = R.check_records(bam, T["content"], T["starts"])
    assert gzi == R.gzi_bytes(table)
    entries = R.check_gzi(gzi, bam, T["content"])
    assert entries == [(at, a) for at, a, _ in table[1:]] and {a for _, a in entries} <= set(T["starts"])
    assert "record-aligned, index " + T["container"][:-5] + ".d.bam.gzi (%d entries), records: BAM (" % (len(table) - 1) in r.stdout, r.stdout
    lz, lz_gzi, r = decode_bam(T["container"], "-gz-records", "-gz-index", "-gz-matches", *opts)
    assert "k_deflate_lz_chunks" in r.stdout
    assert gzip.decompress(lz) == T["content"] and lz.endswith(EOF_MARKER)
    assert [a for _, a in R.read_gzi(lz_gzi)] == [a for _, a in entries]
    print("BAM %d bytes of content: record-aligned %d bytes, with matches %d bytes" % (len(T["content"]), len(bam), len(lz)))


def test_gz_and_plain_d_are_what_they_were(three_blocks):
    T = three_blocks
    gz, _ = decode_gz(T["container"], *ALL_DEVICE)
    assert gzip.decompress(gz) == T["original"]
    assert plain(T["container"]) == T["original"]
    print("%d reads: FASTQ text %d bytes, BAM content %d bytes (%.3f); -d -gz %d bytes, -d -bam %d bytes (%.3f)"
          % (N_READS, len(T["original"]), len(T["content"]), len(T["content"]) / len(T["original"]), len(gz), len(T["bam"]), len(T["bam"]) / len(gz)))


def test_noheader_container_names_reads_by_their_index(three_blocks, tmp_path):
    T = three_blocks
    fq = str(tmp_path / "bare.fastq")
    with open(fq, "wb") as f:
        f.write(T["original"])
    container = compress(fq, "-lossless", "-noheader")
    want = BAM.bam_header() + BAM.bam_records(T["reads"], None, T["quals"])[0]
    files = [decode_bam(container, *opts, env=dict(os.environ, LEON_DECODE_BLOCKS="1"))[0] for opts in (ALL_DEVICE, ["-record-text", "host"])]
    assert gzip.decompress(files[0]) == want and files[1] == files[0]
    parsed = BAM.parse_bam(want)
    assert [p[0] for p in parsed[9:11]] == [b"9", b"10"] and parsed[100000][0] == b"100000" and not any(p[3] for p in parsed)


def test_fasta_container_has_no_qualities(tmp_path):
    n = 2500
    bases, off = common.synthetic(n, 121, 6000, seed=24)
    reads = [bases[int(off[i]):int(off[i]) + (59, 60, 61, 120, 121)[i % 5]] for i in range(n)]
    heads = [b"read_%d\tsome text %d" % (i, i) if i % 3 else b"read_%d" % i for i in range(n)]
    fa = str(tmp_path / "wrapped.fa")
    with open(fa, "wb") as f:
        for h, s in zip(heads, reads):
            f.write(b">" + h + b"\n" + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60)))
    r = run(LEON, "-file", fa, "-c", "-kmer-size", "21", "-abundance", "2")
    assert r.returncode == 0, r.stderr
    want = BAM.bam_header() + BAM.bam_records(reads, heads, None)[0]
    files = [decode_bam(fa + ".leon", *opts)[0] for opts in (["-record-text", "device"], ["-record-text", "host"])]
    assert gzip.decompress(files[0]) == want and files[1] == files[0]
    parsed = BAM.parse_bam(want)
    assert all(p[2] is None for p in parsed) and parsed[1][3] == b"some text 1" and parsed[0][3] is None


@pytest.mark.parametrize("more", [[], ["-gz-records", "-gz-index"]], ids=["fixed", "records"])
def test_a_file_without_a_read_is_the_header_and_the_eof_marker(tmp_path, more):
    empty = str(tmp_path / "empty.fa")
    open(empty, "w").close()
    assert run(LEON, "-file", empty, "-c").returncode == 0
    bam, gzi, r = decode_bam(empty + ".leon", *more)
    assert gzip.decompress(bam) == BAM.bam_header() and bam.endswith(EOF_MARKER) and BAM.parse_bam(gzip.decompress(bam)) == []
    assert R.check_records(bam, BAM.bam_header(), [0, len(BAM.bam_header())]) and (gzi is None or R.read_gzi(gzi) == [])


def test_letters_container_keeps_iupac_codes_and_folds_case(tmp_path):
    reads, heads, quals = _reads(3000, 70, seed=23)
    reads = list(reads)
    for i in range(0, 3000, 7):                                   # lower-case runs and IUPAC codes, as -letters keeps them
        s = bytearray(reads[i])
        s[5:25] = bytes(s[5:25]).lower()
        for j, c in zip(range(30, len(s), 9), b"RYKMSWBDHVryn"):
            s[j] = c
        reads[i] = bytes(s)
    fq = str(tmp_path / "letters.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless", "-letters")
    assert plain(container) == original
    want = BAM.bam_header() + BAM.bam_records(reads, heads, quals)[0]
    files = [decode_bam(container, *opts)[0] for opts in (ALL_DEVICE, ["-record-text", "host"])]
    assert gzip.decompress(files[0]) == want and files[1] == files[0]
    seqs = [p[1] for p in BAM.parse_bam(want)]
    assert seqs == [BAM.fold(s) for s in reads] and seqs[0] == reads[0].upper() and any(c in seqs[0] for c in b"RYKMSWBDHV")


@pytest.mark.parametrize("opts", [ALL_DEVICE, ["-record-text", "host"]], ids=["device", "host"])
def test_a_read_bam_cannot_hold_ends_the_run_and_leaves_nothing(tmp_path, opts):
    reads, heads, quals = _reads(3000, 70, seed=25)
    heads, quals = list(heads), list(quals)
    # a name of 255 bytes (two of them: the smaller read is named), in a file whose names are otherwise fine
    heads[1234] = b"n" * 255 + b" comment"
    heads[2000] = b"m" * 300
    heads[17] = b"k" * 254 + b" comment"
    fq = str(tmp_path / "longname.fastq")
    _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    bam, gzi, r = decode_bam(container, "-gz-records", "-gz-index", *opts, expect=1)
    assert r.stderr.splitlines() == ["EXCEPTION: %s: -bam: read 1234: its name has 255 bytes, BAM allows 254" % container], r.stderr
    assert (bam, gzi) == (None, None) and sorted(os.listdir(str(tmp_path))) == ["longname.fastq", "longname.fastq.leon"]
    os.remove(fq), os.remove(container)
    # a quality byte 32
    heads[1234], heads[2000] = b"fine", b"fine too"
    quals[2999] = quals[2999][:-1] + b" "
    quals[777] = quals[777][:10] + b" " + quals[777][11:]
    fq = str(tmp_path / "lowqual.fastq")
    _write_fastq(fq, reads, heads, quals)
    container = compress(fq, "-lossless")
    bam, gzi, r = decode_bam(container, "-gz-index", *opts, expect=1)
    assert r.stderr.splitlines() == ["EXCEPTION: %s: -bam: read 777: a quality byte below 33" % container], r.stderr
    assert (bam, gzi) == (None, None) and sorted(os.listdir(str(tmp_path))) == ["lowqual.fastq", "lowqual.fastq.leon"]
    assert plain(container) == open(fq, "rb").read()             # (the text paths take such a file as they did)


def test_option_rules(three_blocks):
    T = three_blocks
    stem = T["container"][:-5]
    for p in (stem + ".d", stem + ".d.gz", stem + ".d.bam"):
        if os.path.exists(p):
            os.remove(p)
    before = sorted(os.listdir(str(T["dir"])))
    for args, words in ((["-c", "-bam"], "option -bam belongs to -d"),
                        (["-d", "-gz", "-bam"], "options -gz and -bam name two output formats"),
                        (["-d", "-bam", "-test-file"], "option -test-file compares text: not with -bam"),
                        (["-d", "-gz-records"], "option -gz-records belongs to -gz"),
                        (["-d", "-gz-index"], "option -gz-index belongs to -gz"),
                        (["-d", "-gz-matches"], "option -gz-matches belongs to -gz")):
        r = run(LEON, "-file", T["fq"] if "-c" in args else T["container"], *args)
        assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: " + words], (args, r.stderr)
    assert sorted(os.listdir(str(T["dir"]))) == before
