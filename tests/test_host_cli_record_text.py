"""-m gpu: `leon -d -record-text host|device|auto` through the built binary: the restored file is the same bytes whoever formats the
records (the host threads, or k_fmt_records on the device with the text written from pinned pieces), crossed with `-header-text`, and
`-verbose 1` names the way that ran."""
import os
import subprocess

import pytest

import common
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

RECORD = ([], ["-record-text", "host"], ["-record-text", "device"], ["-record-text", "auto"])
HEADER = (["-header-text", "host"], ["-header-text", "device"])
ON_DEVICE = "record text: device (k_fmt_records)"
ON_HOST = "record text: host threads"


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


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


def _decode(leon_bin, container, *opts, env=None):
    out = container[:-5] + ".d"
    if os.path.exists(out):
        os.remove(out)
    r = run(leon_bin, "-d", "-file", container, "-verbose", "1", *opts, env=env)
    assert r.returncode == 0, (opts, r.stderr)
    return open(out, "rb").read(), r.stdout


def _all_ways(leon_bin, container, want, device_expected=True, env=None, headers=HEADER, records=RECORD):
    """the restored file is `want` for every -record-text x -header-text; the line of -verbose 1 names who formatted"""
    for rec in records:
        for hdr in headers:
            got, log = _decode(leon_bin, container, *rec, *hdr, env=env)
            assert got == want, (rec, hdr)
            if rec == ["-record-text", "device"]:
                assert (ON_DEVICE if device_expected else ON_HOST) in log, (rec, hdr, log)
                if device_expected:
                    assert "for want of device memory" not in log, log
            elif rec != ["-record-text", "auto"]:
                assert ON_HOST in log and ON_DEVICE not in log, (rec, hdr, log)
            else:
                assert ON_HOST in log or ON_DEVICE in log, log


def test_lossless_fastq_of_three_blocks(leon_bin, tmp_path):
    reads, heads, quals = _reads(110000, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(tmp_path / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fq + ".leon", original)
    # rounds of one block, and two rounds per device call (the rounds share the call's device buffers)
    for env in (dict(os.environ, LEON_DECODE_BLOCKS="1"), dict(os.environ, LEON_DECODE_BLOCKS="1", LEON_DECODE_DNA_ROUNDS="2"),
                dict(os.environ, LEON_DECODE_BLOCKS="2", LEON_DECODE_DNA_ROUNDS="2", LEON_HEADER_DEVICE_BLOCKS="0")):
        for hdr in HEADER:
            got, log = _decode(leon_bin, fq + ".leon", "-record-text", "device", *hdr, env=env)
            assert got == original, (hdr, env.get("LEON_DECODE_DNA_ROUNDS"))
            assert ON_DEVICE in log and (" 3 round(s)" in log or " 2 round(s)" in log), log
    r = run(leon_bin, "-d", "-test-file", "-file", fq + ".leon", "-record-text", "device", "-header-text", "device")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr
    # the lossy container of the same file restores to the same bytes either way
    r = run(leon_bin, "-c", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    host, _ = _decode(leon_bin, fq + ".leon", "-record-text", "host")
    assert len(host) == len(original)
    _all_ways(leon_bin, fq + ".leon", host, records=RECORD[2:])


def test_plus_lines(leon_bin, tmp_path):
    reads, heads, quals = _reads(60000, 50, seed=22)               # two read blocks
    # every '+' line repeats its header: the device writes the header twice
    fp = str(tmp_path / "plus_all.fastq")
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: h)
    r = run(leon_bin, "-c", "-lossless", "-file", fp, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fp + ".leon", original)
    _all_ways(leon_bin, fp + ".leon", original, env=dict(os.environ, LEON_DECODE_BLOCKS="1"), records=RECORD[2:3])
    # mixed '+' lines (bare, the header again, own text): exception records -> formatted on the host whatever the option says
    fp = str(tmp_path / "plus_mixed.fastq")
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: (b"", h, b"", b"", h, b"free text %d" % i)[i % 6] if i % 1000 < 6 else h)
    r = run(leon_bin, "-c", "-lossless", "-file", fp, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fp + ".leon", original, device_expected=False, headers=HEADER[1:])
    got, log = _decode(leon_bin, fp + ".leon", "-record-text", "device", "-header-text", "device", env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert got == original
    assert "record text: host threads (the '+' lines are mixed" in log, log


def test_stream_selection_and_wrapped_fasta(leon_bin, tmp_path):
    reads, heads, quals = _reads(3000, 120, seed=23, n_rate=0.003, ragged=True, err=0.02)
    fq = str(tmp_path / "x.fastq")
    _write_fastq(fq, reads, heads, quals)
    norm = [bytes(c if c in b"ACGT" else ord("N") for c in r) for r in reads]
    wants = {
        ("-noheader", "-lossless"): b"".join(b"@%d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(zip(norm, quals))),
        ("-noqual",): b"".join(b">" + h + b"\n" + s + b"\n" for h, s in zip(heads, norm)),
        ("-seq-only",): b"".join(b">%d\n" % i + s + b"\n" for i, s in enumerate(norm)),
    }
    for flags, want in wants.items():
        if os.path.exists(fq + ".leon"):
            os.remove(fq + ".leon")
        r = run(leon_bin, "-file", fq, "-c", "-kmer-size", "21", "-abundance", "2", *flags)
        assert r.returncode == 0, r.stderr
        # (a container without a header stream: -header-text has nothing to decide)
        _all_ways(leon_bin, fq + ".leon", want, headers=HEADER if flags == ("-noqual",) else (["-header-text", "device"],))
        _all_ways(leon_bin, fq + ".leon", want, env=dict(os.environ, LEON_DECODE_BLOCKS="1"), headers=HEADER[1:], records=RECORD[2:3])
    # a FASTA wrapped at 60 with reads of 59, 60, 61, 120 and 121 bases: lines of 60, the last one 1..60
    lens = (59, 60, 61, 120, 121)
    bases, off = common.synthetic(2500, 121, 6000, seed=24)
    fa = str(tmp_path / "wrapped.fa")
    with open(fa, "wb") as f:
        for i in range(2500):
            s = bases[int(off[i]):int(off[i]) + lens[i % 5]]
            f.write(b">read_%d some text\n" % i + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60)))
    original = open(fa, "rb").read()
    r = run(leon_bin, "-file", fa, "-c", "-kmer-size", "21", "-abundance", "2")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fa + ".leon", original)
    r = run(leon_bin, "-d", "-test-file", "-file", fa + ".leon", "-record-text", "device")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_header_over_the_device_cap(leon_bin, tmp_path):
    """-header-text device -record-text device with a header k_hdr_text declines: its block's headers come from the host decoder and are
    uploaded for the formatter; the file is the same"""
    from leon_amd import capi
    reads, heads, quals = _reads(3000, 80, seed=25)
    heads[1500] = b"x" * (capi.HEADER_TEXT_DEVICE_CAP + 1) + b" 77"
    fq = str(tmp_path / "long.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    got, log = _decode(leon_bin, fq + ".leon", "-header-text", "device", "-record-text", "device")
    assert got == original
    assert " 1 of 1 blocks fell back" in log and ON_DEVICE in log, log
    r = run(leon_bin, "-d", "-test-file", "-file", fq + ".leon", "-header-text", "device", "-record-text", "device")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_record_text_option_is_checked(leon_bin, tmp_path):
    for args in (["-record-text", "gpu"], ["-record-text"]):
        r = run(leon_bin, "-file", str(tmp_path / "nothing.leon"), "-d", *args)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-record-text" in r.stderr, (args, r.stderr)
