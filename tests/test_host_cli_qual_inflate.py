"""-m gpu: `leon -d -qual-inflate host|device|auto` through the built binary: the restored file is the same bytes whoever inflates the
quality blocks (zlib on the host threads, or k_qual_inflate on the device), crossed with `-record-text` and `-header-text`; `-verbose 1`
names the way that ran; a damaged quality block and a quality line of the wrong length end the same way both ways."""
import os
import subprocess
import zlib

import pytest

import common
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

INFLATE = ([], ["-qual-inflate", "host"], ["-qual-inflate", "device"], ["-qual-inflate", "auto"])
RECORD = (["-record-text", "host"], ["-record-text", "device"])
HEADER = (["-header-text", "host"], ["-header-text", "device"])
ON_DEVICE = "quality blocks: device (k_qual_inflate)"
ON_HOST = "quality blocks: host threads"
RPB = 50000                                                        # reads per block


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


def _all_ways(leon_bin, container, want, env=None, inflates=INFLATE[1:3], records=RECORD, headers=HEADER[1:], has_quals=True):
    """the restored file is `want` for every -qual-inflate x -record-text x -header-text; the line of -verbose 1 names who inflated"""
    for inf in inflates:
        for rec in records:
            for hdr in headers:
                got, log = _decode(leon_bin, container, *inf, *rec, *hdr, env=env)
                assert got == want, (inf, rec, hdr)
                if not has_quals:
                    assert "quality blocks:" not in log, log      # a container without a quality stream ignores the option
                elif inf == ["-qual-inflate", "device"]:
                    assert ON_DEVICE in log and "for want of device memory" not in log, (inf, rec, hdr, log)
                elif inf != ["-qual-inflate", "auto"]:
                    assert ON_HOST in log and ON_DEVICE not in log, (inf, rec, hdr, log)
                else:
                    assert ON_HOST in log or ON_DEVICE in log, log


def test_lossless_fastq_of_three_blocks(leon_bin, tmp_path):
    reads, heads, quals = _reads(110000, 70, seed=21, n_rate=0.002, err=0.02, ragged=True)
    fq = str(tmp_path / "SRR.fastq")
    original = _write_fastq(fq, reads, heads, quals)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fq + ".leon", original, inflates=INFLATE, headers=HEADER)             # the full cross
    # rounds of one block, and two rounds per device call (the rounds share the call's device buffers)
    for env in (dict(os.environ, LEON_DECODE_BLOCKS="1"), dict(os.environ, LEON_DECODE_BLOCKS="1", LEON_DECODE_DNA_ROUNDS="2")):
        for rec in RECORD:
            got, log = _decode(leon_bin, fq + ".leon", "-qual-inflate", "device", *rec, "-header-text", "device", env=env)
            assert got == original, (rec, env.get("LEON_DECODE_DNA_ROUNDS"))
            assert ON_DEVICE + ", 3 round(s)" in log and "for want of device memory" not in log, log
    for rec in RECORD:
        r = run(leon_bin, "-d", "-test-file", "-file", fq + ".leon", "-qual-inflate", "device", *rec, "-header-text", "device")
        assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr
    # the lossy container of the same file restores to the same bytes either way
    r = run(leon_bin, "-c", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    host, _ = _decode(leon_bin, fq + ".leon")
    assert len(host) == len(original)
    _all_ways(leon_bin, fq + ".leon", host)
    # ... and a container whose quality blocks the device's deflate wrote
    r = run(leon_bin, "-c", "-lossless", "-qual-deflate", "device", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fq + ".leon", original)
    _all_ways(leon_bin, fq + ".leon", original, env=dict(os.environ, LEON_DECODE_BLOCKS="1", LEON_DECODE_DNA_ROUNDS="2"), inflates=INFLATE[2:3])


def test_plus_lines_and_fasta(leon_bin, tmp_path):
    reads, heads, quals = _reads(60000, 50, seed=22)               # two read blocks
    fp = str(tmp_path / "plus_all.fastq")                          # every '+' line repeats its header
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: h)
    r = run(leon_bin, "-c", "-lossless", "-file", fp, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fp + ".leon", original)
    # mixed '+' lines: formatted on the host whatever -record-text says; the option still applies to the quality blocks
    fp = str(tmp_path / "plus_mixed.fastq")
    original = _write_fastq(fp, reads, heads, quals, plus=lambda i, h: (b"", h, b"", b"", h, b"free text %d" % i)[i % 6] if i % 1000 < 6 else h)
    r = run(leon_bin, "-c", "-lossless", "-file", fp, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fp + ".leon", original)
    _all_ways(leon_bin, fp + ".leon", original, env=dict(os.environ, LEON_DECODE_BLOCKS="1"), inflates=INFLATE[2:3])
    # a FASTA input: no quality stream, the option is accepted and ignored
    bases, off = common.synthetic(2500, 121, 6000, seed=24)
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for i in range(2500):
            f.write(b">read_%d some text\n" % i + bases[int(off[i]):int(off[i + 1])] + b"\n")
    original = open(fa, "rb").read()
    r = run(leon_bin, "-file", fa, "-c", "-kmer-size", "21", "-abundance", "2")
    assert r.returncode == 0, r.stderr
    _all_ways(leon_bin, fa + ".leon", original, has_quals=False)


def _three_blocks(leon_bin, tmp_path, name):
    reads, heads, quals = _reads(2 * RPB + 9000, 60, seed=26, ragged=True)
    fq = str(tmp_path / name)
    original = _write_fastq(fq, reads, heads, quals)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    return fq + ".leon", original, quals


def _payload_at(container, quals, block):
    """where quality block `block` lies in the container: the bytes zlib.compress gives for its lines"""
    pay = zlib.compress(b"".join(q + b"\n" for q in quals[block * RPB:(block + 1) * RPB]))
    data = open(container, "rb").read()
    at = data.find(pay)
    assert at >= 0 and data.find(pay, at + 1) < 0, "quality block %d is not in the container as zlib.compress writes it" % block
    return data, at, pay


def test_damaged_quality_block(leon_bin, tmp_path):
    container, original, quals = _three_blocks(leon_bin, tmp_path, "damaged.fastq")
    data, at, pay = _payload_at(container, quals, 1)
    bad = bytearray(data)
    bad[at + len(pay) // 2] ^= 0x5A
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(bad[at:at + len(pay)]))
    open(container, "wb").write(bytes(bad))
    out = container[:-5] + ".d"
    for inf in INFLATE[1:3]:
        for rec in RECORD:
            if os.path.exists(out):
                os.remove(out)
            r = run(leon_bin, "-d", "-file", container, *inf, *rec, "-header-text", "device")
            assert r.returncode == 1, (inf, rec, r.stdout, r.stderr)
            assert r.stderr.startswith("EXCEPTION: ") and "quality block 1 does not decode" in r.stderr, (inf, rec, r.stderr)
            assert not os.path.exists(out), "a failed run left its output behind"


def test_quality_line_of_the_wrong_length(leon_bin, tmp_path):
    """one read's quality line a byte longer, its neighbour's a byte shorter: the block decodes, the lengths disagree.  (-c refuses such a
    file, so the container is edited: the payload overwritten by a shorter stream, padded to the old length -- bytes behind a stream's
    end are ignored)"""
    container, original, quals = _three_blocks(leon_bin, tmp_path, "lengths.fastq")
    data, at, pay = _payload_at(container, quals, 1)
    lens = [len(q) for q in quals[RPB:2 * RPB]]
    r0 = next(i for i in range(100, RPB - 1) if lens[i + 1] > 0)
    lens[r0] += 1
    lens[r0 + 1] -= 1
    text = b"".join(b"I" * n + b"\n" for n in lens)
    new = zlib.compress(text)
    assert len(new) <= len(pay)
    padded = new + bytes(len(pay) - len(new))
    assert zlib.decompressobj().decompress(padded) == text
    open(container, "wb").write(data[:at] + padded + data[at + len(pay):])
    out = container[:-5] + ".d"
    for inf in INFLATE[1:3]:
        for rec in RECORD:
            if os.path.exists(out):
                os.remove(out)
            r = run(leon_bin, "-d", "-file", container, *inf, *rec, "-header-text", "device")
            assert r.returncode == 1, (inf, rec, r.stdout, r.stderr)
            assert r.stderr.startswith("EXCEPTION: ") and "a read's quality and sequence lengths differ" in r.stderr, (inf, rec, r.stderr)
            assert not os.path.exists(out), "a failed run left its output behind"


def test_qual_inflate_option_is_checked(leon_bin, tmp_path):
    for args in (["-qual-inflate", "gpu"], ["-qual-inflate"]):
        r = run(leon_bin, "-file", str(tmp_path / "nothing.leon"), "-d", *args)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-qual-inflate" in r.stderr, (args, r.stderr)
