"""-m gpu: `leon -c -letters` through the built binary.  A sequence line with lower-case stretches, IUPAC codes and gaps
comes back byte for byte -- and verifies against its checksums -- whichever way `-d` restores each stream; without the option the same
file comes back with Ns (today's behaviour: that contrast is the feature), and a file of plain ACGTN gives the container it gave
before.  The tables in the container are pinned by the numpy model of letters_shapes.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import container_patch as P
import hdr_samples as H
import letters_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

RPB = 50000                                                        # reads per block
RUNS, ODD_POS, ODD_BYTES = "leon/metadata/letter_runs", "leon/metadata/letter_odd_pos", "leon/metadata/letter_odd_bytes"
ALL_DEVICE = ["-record-text", "device", "-header-text", "device", "-qual-inflate", "device"]
ALL_HOST = ["-record-text", "host", "-header-text", "host", "-qual-inflate", "host"]
WAYS = {"host": "host threads", "device": "device"}
SLICE = 65536


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def make_reads(n, seed, lo=36, hi=70):
    """n reads of lo..hi bases (ACGT and a few N), SRA-style headers, qualities of the reads' lengths"""
    bases, off = common.synthetic(n, hi, 6000, seed=seed, n_rate=0.002, err=0.02)
    lens = np.random.default_rng(seed).integers(lo, hi + 1, n)
    reads = [bases[int(off[i]):int(off[i]) + int(lens[i])] for i in range(n)]
    heads = H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    return reads, heads, quals


def with_letters(reads):
    """lower-case stretches inside reads; stretches from the end of a read into the start of the next, the block boundary at reads
    49 999 / 50 000 among them; whole reads in lower case where a slice of SLICE bases ends; IUPAC codes, n, '.', '-' and '*'"""
    reads = [bytearray(r) for r in reads]
    for i in range(3, len(reads), 97):
        reads[i][5:20] = reads[i][5:20].lower()
    for i in list(range(10, len(reads) - 1, 1009)) + [RPB - 1, 2 * RPB - 1]:
        reads[i][-6:] = reads[i][-6:].lower()
        reads[i + 1][:8] = reads[i + 1][:8].lower()
    for i in range(5, len(reads), 211):
        reads[i][10:12] = b"Ry"
        reads[i][20:26] = b"n.-*Kk"
    reads[0][0:1] = b"m"
    reads[-1][-1:] = b"W"
    ends = np.cumsum([len(r) for r in reads])
    for k in range(1, 6):
        i = int(np.searchsorted(ends, k * SLICE, side="right"))
        reads[i] = bytearray(bytes(reads[i]).lower())
    return [bytes(r) for r in reads]


def write_fastq(path, reads, heads, quals):
    with open(path, "wb") as f:
        for h, s, q in zip(heads, reads, quals):
            f.write(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
    return open(path, "rb").read()


def compress(path, *opts, env=None):
    r = run(LEON, "-c", "-file", path, "-kmer-size", "25", "-verbose", "1", *opts, env=env)
    assert r.returncode == 0, r.stderr
    return path + ".leon", r.stdout


def decode(container, *opts, expect=0, env=None):
    out = container[:-5] + ".d"
    if os.path.exists(out):
        os.remove(out)
    r = run(LEON, "-d", "-file", container, "-verbose", "1", *opts, env=env)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    return (open(out, "rb").read() if os.path.exists(out) else None), r


def line(log, prefix):
    lines = [l for l in log.splitlines() if l.startswith(prefix)]
    assert len(lines) == 1, log
    return lines[0]


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def three_blocks(tmp_path_factory):
    """110 000 reads (three blocks) with letters of every kind: the model's tables, and the container of -c -lossless -letters -checksum"""
    d = tmp_path_factory.mktemp("letters")
    reads, heads, quals = make_reads(2 * RPB + 10000, seed=41)
    reads = with_letters(reads)
    fq = str(d / "SRR.fastq")
    original = write_fastq(fq, reads, heads, quals)
    model = S.Model(np.frombuffer(b"".join(reads), dtype=np.uint8))
    assert any(a // SLICE != (b - 1) // SLICE for a, b in model.runs.tolist()), "no run crosses a slice's end: case (e) would show nothing"
    container, log = compress(fq, "-lossless", "-letters", "-checksum")
    kept = str(d / "letters.fastq.leon")                            # (with the original beside it: -test-file looks for letters.fastq)
    shutil.copy(container, kept)
    shutil.copy(fq, str(d / "letters.fastq"))
    return dict(reads=reads, heads=heads, quals=quals, original=original, model=model, fq=fq, container=kept, log=log, dir=d)


def test_tables_are_the_models(three_blocks):
    T, m = three_blocks, three_blocks["model"]
    runs = P.h5_dataset(T["container"], RUNS, np.uint64)
    assert runs[0] == 1 and np.array_equal(runs[1:].reshape(-1, 2), m.runs)
    assert np.array_equal(P.h5_dataset(T["container"], ODD_POS, np.uint64), m.odd_pos)
    assert np.array_equal(P.h5_dataset(T["container"], ODD_BYTES, np.uint8), m.odd_byte)
    assert m.n_runs > 1000 and m.n_odd > 1000
    size = 8 * (1 + 2 * m.n_runs) + 9 * m.n_odd
    assert line(T["log"], "letters: ") == "letters: %d lower-case run(s), %d other byte(s) kept (%d bytes)" % (m.n_runs, m.n_odd, size)


@pytest.mark.parametrize("way", ["host", "device"])
def test_every_letter_comes_back_and_verifies(three_blocks, way):
    """(a) -c -lossless -letters -checksum, then -d: the input's bytes, every block verified, nothing ignored"""
    T, m = three_blocks, three_blocks["model"]
    opts = ALL_HOST if way == "host" else ALL_DEVICE
    restored, r = decode(T["container"], "-test-file", *opts)      # (-test-file: the binary's own comparison with letters.fastq, status 0)
    assert restored == T["original"]
    assert line(r.stdout, "checksums: ") == "checksums: 3 blocks verified (dna: %s, header: %s, quality: %s)" % ((WAYS[way],) * 3)
    assert line(r.stdout, "letters: ") == "letters: %d run(s), %d byte(s) restored (%s)" % (m.n_runs, m.n_odd, WAYS[way])
    assert "WARNING" not in r.stderr
    # rounds of one block: the tables are cut at the blocks' ends, a run across reads 49 999 / 50 000 is clipped on both sides
    restored, r = decode(T["container"], *opts, env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert restored == T["original"] and line(r.stdout, "checksums: ").startswith("checksums: 3 blocks verified (dna: %s," % WAYS[way])


def test_without_the_option_the_letters_are_lost(three_blocks):
    """(b) today's behaviour, and the contrast"""
    T = three_blocks
    container, log = compress(T["fq"], "-lossless")
    assert not any(P.h5_has(container, name) for name in (RUNS, ODD_POS, ODD_BYTES)) and "letters:" not in log
    restored, r = decode(container, *ALL_DEVICE)
    assert "letters:" not in r.stdout
    n = len(T["reads"])
    assert restored.split(b"\n")[1::4][:n] == [folded_n(s) for s in T["reads"]]
    assert restored.split(b"\n")[3::4][:n] == T["quals"]


def folded_n(read):
    """what the coder alone gives back: everything but A C G T is an N"""
    return bytes(c if c in b"ACGT" else ord("N") for c in read)


def test_plain_file_gives_the_container_it_gave(three_blocks, tmp_path):
    """(c) no such letters: not a byte of the container differs"""
    reads, heads, quals = make_reads(3000, seed=42)
    fq = str(tmp_path / "plain.fastq")
    write_fastq(fq, reads, heads, quals)
    container, _ = compress(fq, "-lossless")
    before = open(container, "rb").read()
    container, log = compress(fq, "-lossless", "-letters")
    assert open(container, "rb").read() == before
    assert line(log, "letters: ") == "letters: none"
    assert not P.h5_has(container, RUNS)


def test_soft_masked_fasta(tmp_path):
    """(d) a contig of 300 000 bases, half of it soft-masked, and short ones, wrapped at 60"""
    rng = np.random.default_rng(43)
    contig = S.plain(300000, 44)
    for a in range(0, 300000, 10000):
        S.lower(contig, a + 2500, a + 7500)
    contig[123456:123460] = np.frombuffer(b"RYnN", dtype=np.uint8)
    seqs = [contig.tobytes()] + [S.mixed(int(n), 45 + i, 0.02, 0.01).tobytes() for i, n in enumerate(rng.integers(61, 900, 300))]
    fa = str(tmp_path / "assembly.fasta")
    with open(fa, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">contig_%d len=%d\n" % (i, len(s)) + b"".join(s[a:a + 60] + b"\n" for a in range(0, len(s), 60)))
    original = open(fa, "rb").read()
    container, log = compress(fa, "-letters", "-checksum")
    m = S.Model(np.frombuffer(b"".join(seqs), dtype=np.uint8))
    assert line(log, "letters: ").startswith("letters: %d lower-case run(s), %d other byte(s) kept" % (m.n_runs, m.n_odd))
    for way, opts in (("host", ALL_HOST), ("device", ALL_DEVICE)):
        restored, r = decode(container, *opts)
        assert restored == original, way
        assert line(r.stdout, "checksums: ").startswith("checksums: 1 blocks verified (dna: %s," % WAYS[way]) and "ignored" not in r.stdout


def test_slices_and_devices_give_the_same_container(three_blocks):
    """(e) slices of 64 KiB, runs across their joins merged; (f) two replicas folded, device 0's tables kept"""
    T = three_blocks
    want = open(T["container"], "rb").read()
    container, _ = compress(T["fq"], "-lossless", "-letters", "-checksum", env=dict(os.environ, LEON_LETTERS_SLICE=str(SLICE)))
    assert open(container, "rb").read() == want, "LEON_LETTERS_SLICE changed the container"
    container, _ = compress(T["fq"], "-lossless", "-letters", "-checksum", "-gpus", "2", env=dict(os.environ, LEON_SHARE_GPU="1"))
    assert open(container, "rb").read() == want, "-gpus 2 changed the container"


def test_lossy_default_keeps_sequences_and_headers(three_blocks):
    """(g) -c -letters: the qualities are smoothed, the sequences and headers are not touched"""
    T = three_blocks
    container, _ = compress(T["fq"], "-letters")
    n = len(T["reads"])
    for opts in (ALL_HOST, ALL_DEVICE):
        restored, _ = decode(container, *opts)
        lines = restored.split(b"\n")
        assert lines[1::4][:n] == T["reads"]
        assert lines[0::4][:n] == [b"@" + h for h in T["heads"]]


@pytest.mark.parametrize("damage", ["runs overlap", "position behind the bases"])
def test_damaged_tables(three_blocks, tmp_path, damage):
    """(h) -d checks the tables before anything is decoded and names the dataset"""
    T, m = three_blocks, three_blocks["model"]
    container = str(tmp_path / "damaged.fastq.leon")
    shutil.copy(T["container"], container)
    if damage == "runs overlap":
        table, at = P.find_dataset(container, RUNS, np.uint64)
        P.patch(container, at + 8 * 3, int(table[2] - 1).to_bytes(8, "little"))       # run 1 begins inside run 0
        name = RUNS
    else:
        table, at = P.find_dataset(container, ODD_POS, np.uint64)
        P.patch(container, at + 8 * (len(table) - 1), len(b"".join(T["reads"])).to_bytes(8, "little"))
        name = ODD_POS
    for opts in (ALL_HOST, ALL_DEVICE):
        out, r = decode(container, *opts, expect=1)
        assert r.stderr.startswith("EXCEPTION: letters: " + name + " ") and len(r.stderr.splitlines()) == 1, r.stderr
        assert out is None, "a failed run left its output behind"
