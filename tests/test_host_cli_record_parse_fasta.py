"""-m gpu: `leon -c -record-parse device -record-parse-fasta` through the built binary: with a FASTA file's records split
on the device (k_fa_split) the container is the one the host parser gives from the same file, byte for byte, the FASTA line width in
`params` included -- single-line and wrapped reads, CRLF, no final newline, a first record on one line before wrapped ones, a ragged
record, a blank line, a record without sequence, a contig of 5 000 lines between short reads, the same files as BGZF under
`-input-inflate device`, batches of one block, `-noheader`, `-letters -checksum`.  The report line says how the records were shared out:
at most four hand-offs of one record each, the numbers the reader's rule replayed over the restatement (tests/fasta_shapes.py) gives --
so a pass cannot be a silent fall-back to the host parser.  LEON_PARSE_SPAN_KB=4 makes these small files span many spans."""
import os
import random
import re
import subprocess

import pytest

import bgzf_input as B
import common
import fasta_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

ON_DEVICE = "parse: records split on the device (k_fa_split), spans of 4096 bytes"
SWITCH = ("-record-parse", "device", "-record-parse-fasta")
ENV = {"LEON_PARSE_SPAN_KB": "4", "LEON_INPUT_CHUNK_KB": "16"}
REPORT = re.compile(r"^parse: (\d+) records split on the device \(k_fa_split\), (\d+) read by the host parser in (\d+) hand-off\(s\)$", re.M)


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def reads(n, L, seed):
    bases, off = common.synthetic(n, L, 6000, seed=seed, n_rate=0.002, err=0.02)
    return [bytes(bases[int(off[i]):int(off[i + 1])]) for i in range(n)]


def record(i, seq, W=None, eol=b"\n"):
    lines = [seq] if W is None else [seq[a:a + W] for a in range(0, len(seq), W)]
    return b">read_%d some text\n".replace(b"\n", eol) % i + b"".join(l + eol for l in lines)


def fasta(seqs, W=None, eol=b"\n"):
    return [record(i, s, W, eol) for i, s in enumerate(seqs)]


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


def both_routes(leon_bin, path, text, *opts, env=None, keep=False, regular=False):
    """the container of the device route is the host route's; the report line holds what the replayed rule gives; returns the device run's stdout"""
    r, want = compress(leon_bin, path, *opts, env=env)
    assert r.returncode == 0 and want, r.stderr
    assert "parse:" not in r.stdout
    r, got = compress(leon_bin, path, *SWITCH, *opts, env=env)
    assert r.returncode == 0, r.stderr
    assert ON_DEVICE in r.stdout, r.stdout
    assert got == want, "the container of -record-parse-fasta differs from the host route's"
    m = REPORT.search(r.stdout)
    assert m, r.stdout
    by_device, by_host, hand_offs = map(int, m.groups())
    rule = S.replay(text)
    print(path, "device", by_device, "host", by_host, "hand-offs", hand_offs, "replay", rule)
    assert by_device + by_host == rule["reads"]
    assert hand_offs <= 4 and by_host <= (2 if regular else 2 + 2 * 1024) and by_device > by_host
    assert (by_device, by_host, hand_offs) == (rule["by_device"], rule["by_host"], rule["hand_offs"])
    assert len([l for l in r.stdout.splitlines() if " handed to the host parser (" in l]) == hand_offs
    if keep:
        open((path[:-3] if path.endswith(".gz") else path) + ".leon", "wb").write(got)
    return r.stdout


def files():
    s121, s150, s120 = reads(2500, 121, 61), reads(2500, 150, 62), reads(2000, 120, 63)
    J = b"".join
    wrapped = fasta(s150, 60)
    out = {
        "single_line_121": (J(fasta(s121)), True),
        "wrapped_150_at_60": (J(wrapped), True),
        "wrapped_120_at_60": (J(fasta(s120, 60)), True),
        "crlf": (J(fasta(s150, 60, b"\r\n")), True),
        "no_final_newline": (J(wrapped)[:-1], True),
        "blank_lines_first": (b"\n\r\n" + J(wrapped), True),
        "first_on_one_line": (J([record(0, s150[0][:50])] + wrapped[1:]), False),
        "ragged_in_the_middle": (J(wrapped[:1200] + [b">ragged\n" + s150[1200][:60] + b"\n" + s150[1200][60:119] + b"\n" + s150[1200][119:] + b"\n"] + wrapped[1201:]), False),
        "blank_line_in_the_middle": (J(wrapped[:1200]) + b"\n" + J(wrapped[1200:]), False),
        "record_without_sequence": (J(wrapped[:1200] + [b">nothing here\n"] + wrapped[1200:]), False),
    }
    short = fasta(reads(2000, 100, 64), 60)
    contig = bytes(random.Random(65).choices(b"ACGT", k=300000))
    out["contig_between_short_reads"] = (J(short[:1000] + [record(1000, contig, 60)] + short[1000:]), True)
    return out


FILES = None


def the_files():
    global FILES
    if FILES is None:
        FILES = files()
    return FILES


NAMES = ["single_line_121", "wrapped_150_at_60", "wrapped_120_at_60", "crlf", "no_final_newline", "blank_lines_first", "first_on_one_line", "ragged_in_the_middle",
         "blank_line_in_the_middle", "record_without_sequence", "contig_between_short_reads"]
WIDTHS = {"single_line_121": 0, "wrapped_150_at_60": 60, "wrapped_120_at_60": 60, "crlf": 60, "no_final_newline": 60, "blank_lines_first": 60, "first_on_one_line": 60,
          "ragged_in_the_middle": 0, "blank_line_in_the_middle": 0, "record_without_sequence": 0, "contig_between_short_reads": 60}


@pytest.mark.parametrize("kind", ["plain", "bgzf"])
@pytest.mark.parametrize("name", NAMES)
def test_same_container_as_the_host_route(leon_bin, tmp_path, name, kind):
    text, regular = the_files()[name]
    assert len(text) > 20 * 4096 and S.replay(text)["fasta_line_width"] == WIDTHS[name]
    if kind == "plain":
        path = str(tmp_path / (name + ".fasta"))
        open(path, "wb").write(text)
        out = both_routes(leon_bin, path, text, regular=regular)
    else:
        path = str(tmp_path / (name + ".fasta.gz"))
        open(path, "wb").write(B.bgzf(text, level=6))
        out = both_routes(leon_bin, path, text, "-input-inflate", "device", regular=regular)
        assert "input: BGZF members inflated on the device" in out
    assert "parse: record 1 handed to the host parser (the file's first record)" in out, out
    why = {"first_on_one_line": "the first record on more than one line", "ragged_in_the_middle": "a line of another width",
           "blank_line_in_the_middle": "a line of another width", "record_without_sequence": "a record without sequence"}.get(name)
    if why:
        assert "handed to the host parser (%s)" % why in out, out


def test_letters_checksum_and_back(leon_bin, tmp_path):
    """a half soft-masked file under -letters -checksum: the same container, and -d -test-file gives the file back"""
    seqs = reads(2000, 150, 66)
    text = b"".join(fasta([s.lower() if i % 2 else s[:40] + s[40:90].lower() + s[90:] for i, s in enumerate(seqs)], 60))
    path = str(tmp_path / "masked.fasta")
    open(path, "wb").write(text)
    both_routes(leon_bin, path, text, "-letters", "-checksum", keep=True, regular=True)
    r = run(leon_bin, "-d", "-file", path + ".leon", "-test-file")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_noheader(leon_bin, tmp_path):
    text = the_files()["wrapped_150_at_60"][0]
    path = str(tmp_path / "reads.fasta")
    open(path, "wb").write(text)
    both_routes(leon_bin, path, text, "-noheader", regular=True)


def test_batches_of_one_block(leon_bin, tmp_path):
    """120 000 reads of 30 bases: three batches under LEON_BATCH_BLOCKS=1, the last one partial, on both routes"""
    n = 120000
    bases, off = common.synthetic(n, 30, 3000, seed=67)
    text = b"".join(b">r%d\n%s\n" % (i, bytes(bases[int(off[i]):int(off[i + 1])])) for i in range(n))
    path = str(tmp_path / "many.fasta")
    open(path, "wb").write(text)
    env = {"LEON_PARSE_SPAN_KB": "1024", "LEON_BATCH_BLOCKS": "1"}
    r, want = compress(leon_bin, path, env=env)
    assert r.returncode == 0 and want, r.stderr
    r, got = compress(leon_bin, path, *SWITCH, env=env)
    assert r.returncode == 0 and got == want, r.stderr
    m = REPORT.search(r.stdout)
    assert m and int(m.group(1)) == n - 2 and int(m.group(2)) == 2 and int(m.group(3)) == 2, r.stdout


def test_both_routes_refuse_in_the_same_words(leon_bin, tmp_path):
    """a BGZF FASTA file cut short: both routes end with the same words and leave nothing behind"""
    data = B.bgzf(the_files()["wrapped_150_at_60"][0], level=6)
    path = str(tmp_path / "cut.fasta.gz")
    open(path, "wb").write(data[:len(data) * 2 // 3])
    r_host, c_host = compress(leon_bin, path, "-input-inflate", "device")
    r_dev, c_dev = compress(leon_bin, path, "-input-inflate", "device", *SWITCH)
    assert r_host.returncode == 1 and r_dev.returncode == 1, (r_host.stderr, r_dev.stderr)
    assert c_host is None and c_dev is None
    assert r_dev.stderr == r_host.stderr and r_host.stderr.startswith("EXCEPTION: ") and "is truncated or corrupt" in r_host.stderr, (r_host.stderr, r_dev.stderr)
    assert os.listdir(str(tmp_path)) == ["cut.fasta.gz"]


def test_option_rules(leon_bin, tmp_path):
    nothing = str(tmp_path / "nothing.fasta")
    for args in (["-c", "-record-parse-fasta"], ["-c", "-record-parse", "host", "-record-parse-fasta"], ["-d", "-record-parse-fasta"]):
        r = run(leon_bin, "-file", nothing, *args)
        assert r.returncode == 1 and r.stderr.splitlines() == ["EXCEPTION: option -record-parse-fasta belongs to -record-parse device"], r.stderr
    assert os.listdir(str(tmp_path)) == []
    # FASTA without the switch keeps its route and its line; a FASTQ input under the switch is treated as without it
    text = the_files()["wrapped_150_at_60"][0]
    path = str(tmp_path / "reads.fasta")
    open(path, "wb").write(text)
    r, want = compress(leon_bin, path)
    r, got = compress(leon_bin, path, "-record-parse", "device")
    assert r.returncode == 0 and got == want and "parse: records cut on the host (FASTA input)" in r.stdout and "k_fa_split" not in r.stdout, r.stdout + r.stderr
    seqs = reads(1000, 90, 68)
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    path = str(tmp_path / "reads.fastq")
    open(path, "wb").write(fq)
    r, want = compress(leon_bin, path, "-lossless", "-record-parse", "device")
    assert r.returncode == 0 and want, r.stderr
    r, got = compress(leon_bin, path, "-lossless", *SWITCH)
    assert r.returncode == 0 and got == want and "(k_fq_split), spans of" in r.stdout and "k_fa_split" not in r.stdout, r.stdout + r.stderr
    import gzip
    path = str(tmp_path / "plain.fasta.gz")
    open(path, "wb").write(gzip.compress(text))
    r, want = compress(leon_bin, path)
    r, got = compress(leon_bin, path, *SWITCH)
    assert r.returncode == 0 and got == want and "parse: records cut on the host (gzip input that is not inflated on the device)" in r.stdout, r.stdout + r.stderr
