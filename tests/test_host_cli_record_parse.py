"""-m gpu: `leon -c -record-parse host|device` through the built binary: with the records split on the device
(k_fq_split) the container is the one the host parser gives from the same file, byte for byte -- plain and BGZF input, every quality
route, CRLF files, files without a final newline, files whose irregular records go back to the host parser, batches of one block; a
file either route refuses is refused by both in the same words; FASTA and plain gzip take the host route whatever the option says.
LEON_PARSE_SPAN_KB makes these small files span many spans."""
import gzip
import os
import subprocess

import pytest

import bgzf_input as B
import common
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

ON_DEVICE = "parse: records split on the device (k_fq_split), spans of 16384 bytes"
H5BIN = "/opt/conda/bin"
HANDED = " handed to the host parser ("
ENV = {"LEON_PARSE_SPAN_KB": "16", "LEON_INPUT_CHUNK_KB": "16"}


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def records(n=3000, L=90, seed=41):
    bases, off = common.synthetic(n, L, 6000, seed=seed, n_rate=0.002, err=0.02, ragged=True)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    heads = H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    return list(zip(heads, reads, quals))


def fastq(recs, end=b"\n", plus=lambda i, h: b"+"):
    return b"".join(b"@" + h + end + s + end + plus(i, h) + end + q + end for i, (h, s, q) in enumerate(recs))


def compress(leon_bin, path, *opts, env=None):
    """`leon -c` on path: (the process, the container's bytes or None); nothing of the run stays behind"""
    stem = path[:-3] if path.endswith(".gz") else path
    container = stem + ".leon"
    if os.path.exists(container):
        os.remove(container)
    r = run(leon_bin, "-c", "-file", path, "-kmer-size", "25", "-verbose", "1", *opts, env=dict(os.environ, **dict(ENV, **(env or {}))))
    data = open(container, "rb").read() if os.path.exists(container) else None
    assert not os.path.exists(container + ".tmp"), "a temporary container was left behind"
    return r, data


def both_routes(leon_bin, path, *opts, env=None, keep=False):
    """the container of `-record-parse device`, which is the one of `-record-parse host` and of no option at all; the device run's stdout"""
    r, want = compress(leon_bin, path, "-record-parse", "host", *opts, env=env)
    assert r.returncode == 0 and want, r.stderr
    assert "parse:" not in r.stdout
    r, plain = compress(leon_bin, path, *opts, env=env)
    assert r.returncode == 0 and plain == want and "parse:" not in r.stdout
    r, got = compress(leon_bin, path, "-record-parse", "device", *opts, env=env)
    assert r.returncode == 0, r.stderr
    assert ON_DEVICE in r.stdout, r.stdout
    assert got == want, "the container of -record-parse device differs from the host route's"
    if keep:
        open((path[:-3] if path.endswith(".gz") else path) + ".leon", "wb").write(got)
    return r.stdout


OPTS = [["-lossless"], [], ["-lossless", "-checksum", "-letters"], ["-lossless", "-qual-deflate", "device"], ["-lossless", "-qual-deflate", "auto"],
        ["-qual-deflate", "auto"]]


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "+".join(o) or "lossy")
@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_same_container_as_the_host_route(leon_bin, tmp_path, kind, opts):
    text = fastq(records())
    assert len(text) > 20 * 16384
    if kind == "plain":
        path = str(tmp_path / "reads.fastq")
        open(path, "wb").write(text)
        out = both_routes(leon_bin, path, *opts)
    else:
        path = str(tmp_path / "reads.fastq.gz")
        open(path, "wb").write(B.bgzf(text, level=6))
        out = both_routes(leon_bin, path, "-input-inflate", "device", *opts)
        assert "input: BGZF members inflated on the device" in out
    assert "2999 records split on the device" in out and "1 read by the host parser in 1 hand-off(s)" in out, out


def test_qualities_that_do_not_stay_resident(leon_bin, tmp_path):
    path = str(tmp_path / "twice.fastq")
    open(path, "wb").write(fastq(records(seed=43)))
    both_routes(leon_bin, path, env={"LEON_QUAL_RESIDENT_MB": "0"})
    both_routes(leon_bin, path, "-checksum", env={"LEON_QUAL_RESIDENT_MB": "0"})


def test_crlf_and_no_final_newline(leon_bin, tmp_path):
    recs = records(1500, seed=45)
    for name, text in (("crlf.fastq", fastq(recs, end=b"\r\n")), ("open.fastq", fastq(recs)[:-1]), ("open_crlf.fastq", fastq(recs, end=b"\r\n")[:-2]),
                       ("blank_end.fastq", fastq(recs) + b"\n\n\n\n\n")):
        path = str(tmp_path / name)
        open(path, "wb").write(text)
        out = both_routes(leon_bin, path, "-lossless")
        assert "records split on the device" in out, out


def test_irregular_records_go_to_the_host_parser(leon_bin, tmp_path):
    """blank lines between some records, '+' lines that repeat the header on all but a few records, one '+other': the same container, the
    hand-offs named.  The parser drops blank lines on either route, so `-d -test-file` says identical for the file without them, and the
    file with them comes back as that one."""
    recs = records(3000, seed=47)
    odd = {5: b"+", 700: b"+", 701: b"+", 2999: b"+", 1500: b"+other text"}
    texts = {}
    for name, blanks in (("odd.fastq", {}), ("odd_blank.fastq", {3: b"\n", 900: b"\r\n\n", 2500: b"\n"})):
        texts[name] = b"".join(blanks.get(i, b"") + b"@" + h + b"\n" + s + b"\n" + odd.get(i, b"+" + h) + b"\n" + q + b"\n" for i, (h, s, q) in enumerate(recs))
        path = str(tmp_path / name)
        open(path, "wb").write(texts[name])
        out = both_routes(leon_bin, path, "-lossless", keep=True)
        lines = [l for l in out.splitlines() if HANDED in l]
        assert lines and lines[0] == "parse: record 1 handed to the host parser (the file's first record)", out
        assert lines[1] == ("parse: record 4 handed to the host parser (its first line does not begin with '@')" if blanks else
                            "parse: record 6 handed to the host parser (a '+' line of another kind)"), out
        assert "hand-off(s)" in out and " records split on the device" in out and " 0 records split on the device" not in out
        r = run(leon_bin, "-d", "-file", path + ".leon", *([] if blanks else ["-test-file"]))
        assert r.returncode == 0 and (blanks or "identical" in r.stdout), r.stdout + r.stderr
        assert open(path + ".d", "rb").read() == texts["odd.fastq"]


def test_batches_of_one_block(leon_bin, tmp_path):
    """120 000 reads of 30 bases: three batches under LEON_BATCH_BLOCKS=1, the last one partial, on both routes"""
    n = 120000
    bases, off = common.synthetic(n, 30, 3000, seed=49)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bases[int(off[i]):int(off[i + 1])], b"FFFF:FFFFF,FFFFFFFFF:FFFFFFFFFF"[:int(off[i + 1] - off[i])]) for i in range(n))
    path = str(tmp_path / "many.fastq")
    open(path, "wb").write(text)
    got = {}
    for route in ("host", "device"):
        for blocks in (None, "1"):
            env = {"LEON_PARSE_SPAN_KB": "1024"}
            if blocks:
                env["LEON_BATCH_BLOCKS"] = blocks
            r, got[route, blocks] = compress(leon_bin, path, "-lossless", "-record-parse", route, env=env)
            assert r.returncode == 0 and got[route, blocks], r.stderr
    # the routes write the same bytes at either batch size; across batch sizes the datasets are made in another order, so the files are
    # compared dataset by dataset (h5diff, as tests/test_host_cli.py compares the DNA stream's batches)
    assert got["device", None] == got["host", None] and got["device", "1"] == got["host", "1"]
    for name, data in (("whole.leon", got["host", None]), ("blocks.leon", got["device", "1"])):
        open(str(tmp_path / name), "wb").write(data)
    r = run(os.path.join(H5BIN, "h5diff"), str(tmp_path / "whole.leon"), str(tmp_path / "blocks.leon"))
    assert r.returncode == 0, r.stdout + r.stderr


def refused_alike(leon_bin, path, *opts):
    r_host, c_host = compress(leon_bin, path, "-record-parse", "host", *opts)
    r_dev, c_dev = compress(leon_bin, path, "-record-parse", "device", *opts)
    assert r_host.returncode == 1 and r_dev.returncode == 1, (r_host.stderr, r_dev.stderr)
    assert c_host is None and c_dev is None
    assert r_dev.stderr == r_host.stderr and r_host.stderr.startswith("EXCEPTION: "), (r_host.stderr, r_dev.stderr)
    assert ON_DEVICE in r_dev.stdout
    return r_host.stderr


def test_both_routes_refuse_in_the_same_words(leon_bin, tmp_path):
    recs = records(3000, seed=51)
    bad = list(recs)
    h, s, q = bad[2800]
    bad[2800] = (h, s, q[:-1])
    path = str(tmp_path / "lengths.fastq")
    open(path, "wb").write(fastq(bad))
    assert "FASTQ record 2801 of " in refused_alike(leon_bin, path, "-lossless")
    text = fastq(recs)
    path = str(tmp_path / "cut.fastq")
    open(path, "wb").write(text[:text.rfind(b"\n+\n")])
    assert "truncated FASTQ record" in refused_alike(leon_bin, path, "-lossless")
    data = B.bgzf(text, level=6)
    path = str(tmp_path / "cut.fastq.gz")
    open(path, "wb").write(data[:len(data) * 2 // 3])
    assert "is truncated or corrupt" in refused_alike(leon_bin, path, "-lossless", "-input-inflate", "device")
    assert sorted(os.listdir(str(tmp_path))) == ["cut.fastq", "cut.fastq.gz", "lengths.fastq"]


def test_host_route_whatever_the_option_says(leon_bin, tmp_path):
    bases, off = common.synthetic(2000, 121, 6000, seed=53)
    fasta = b"".join(b">read_%d\n%s\n" % (i, bases[int(off[i]):int(off[i + 1])]) for i in range(2000))
    path = str(tmp_path / "reads.fasta")
    open(path, "wb").write(fasta)
    r, want = compress(leon_bin, path)
    r, got = compress(leon_bin, path, "-record-parse", "device")
    assert r.returncode == 0 and got == want and "parse: records cut on the host (FASTA input)" in r.stdout, r.stdout + r.stderr
    path = str(tmp_path / "reads.fastq.gz")
    open(path, "wb").write(gzip.compress(fastq(records(1000, seed=55))))
    r, want = compress(leon_bin, path, "-lossless")
    for more in ([], ["-input-inflate", "device"]):
        r, got = compress(leon_bin, path, "-lossless", "-record-parse", "device", *more)
        assert r.returncode == 0 and got == want, r.stderr
        assert "parse: records cut on the host (gzip input that is not inflated on the device)" in r.stdout, r.stdout


def test_option_rules(leon_bin, tmp_path):
    nothing = str(tmp_path / "nothing.fastq")
    for args in (["-d", "-record-parse", "device"], ["-record-parse", "host", "-d"]):
        r = run(leon_bin, "-file", nothing + ".leon", *args)
        assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: option -record-parse belongs to -c"], r.stderr
    for value in ("auto", "gpu", ""):
        r = run(leon_bin, "-c", "-file", nothing, "-record-parse", value) if value else run(leon_bin, "-c", "-file", nothing, "-record-parse")
        words = "option -record-parse: '%s': expected host or device" % value if value else "option -record-parse needs a value"
        assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: " + words], r.stderr
    assert os.listdir(str(tmp_path)) == []
