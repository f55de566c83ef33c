"""-m gpu: `leon -c -input-inflate host|device|auto` through the built binary: a BGZF input inflated by the device (k_bgzf_inflate) gives
the container the host way (zlib's gzread, which is what runs without the option) gives from the same file, byte for byte; lines, records
and \\r\\n pairs that straddle members and chunks are not noticed by the parser; a file that is not BGZF takes the host way; a truncated
or damaged file ends as it ends on the host way.  LEON_INPUT_CHUNK_KB makes these small files span several chunks."""
import gzip
import os
import random
import subprocess

import pytest

import bgzf_input as B
import common
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

ON_DEVICE = "input: BGZF members inflated on the device (k_bgzf_inflate)"
ON_HOST = "input: read on the host"
CHUNK_KB = "16"                                                    # smaller than most members: a chunk may hold no whole member


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def fastq_text(n=3000, L=90, seed=31, end=b"\n", last_newline=True):
    bases, off = common.synthetic(n, L, 6000, seed=seed, n_rate=0.002, err=0.02, ragged=True)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    heads = H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    text = b"".join(b"@" + h + end + s + end + b"+" + end + q + end for h, s, q in zip(heads, reads, quals))
    return text if last_newline else text[:-len(end)]


def fasta_text(n=2500, L=121, width=60, seed=33):
    bases, off = common.synthetic(n, L, 6000, seed=seed)
    out = []
    for i in range(n):
        s = bases[int(off[i]):int(off[i + 1])]
        out.append(b">read_%d some text\n" % i + b"\n".join(s[a:a + width] for a in range(0, len(s), width)) + b"\n")
    return b"".join(out)


def cuts_of(text, seed):
    """members cut at arbitrary bytes (some of them tiny, one empty) and at 65 280"""
    rng = random.Random(seed)
    cuts, at = [], 0
    while at < len(text):
        at += rng.choice((65280, 65280, rng.randrange(1, 65280), rng.randrange(1, 300), 0))
        if at < len(text):
            cuts.append(at)
    return cuts


def compress(leon_bin, path, *opts, env=None):
    """`leon -c` on path: (the process, the container's bytes or None).  The container is removed: the next way writes its own."""
    stem = path[:-3] if path.endswith(".gz") else path
    container = stem + ".leon"
    if os.path.exists(container):
        os.remove(container)
    r = run(leon_bin, "-c", "-file", path, "-kmer-size", "25", "-verbose", "1", *opts, env=dict(os.environ, LEON_INPUT_CHUNK_KB=CHUNK_KB, **(env or {})))
    data = None
    if os.path.exists(container):
        data = open(container, "rb").read()
    assert not os.path.exists(container + ".tmp"), "a temporary container was left behind"
    return r, data


def same_container_every_way(leon_bin, path, *opts, env=None, device_line=ON_DEVICE, keep=False):
    r, want = compress(leon_bin, path, "-input-inflate", "host", *opts, env=env)
    assert r.returncode == 0 and want, r.stderr
    assert "input:" not in r.stdout
    r, plain = compress(leon_bin, path, *opts, env=env)            # without the option: the same
    assert r.returncode == 0 and plain == want and "input:" not in r.stdout
    for way in ("auto", "device"):                                 # (`auto`: its size threshold set to 0, or these small files would all take the host way)
        r, got = compress(leon_bin, path, "-input-inflate", way, *opts, env=dict(env or {}, LEON_INPUT_INFLATE_AUTO_KB="0"))
        assert r.returncode == 0, (way, r.stderr)
        assert device_line in r.stdout, (way, r.stdout)
        assert got == want, "the container of -input-inflate %s differs from the host way's" % way
    if keep:
        stem = path[:-3] if path.endswith(".gz") else path
        open(stem + ".leon", "wb").write(got)
    return r.stdout


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
@pytest.mark.parametrize("opts", [["-lossless"], [], ["-lossless", "-checksum", "-letters"], ["-checksum", "-letters"]], ids=lambda o: "+".join(o) or "lossy")
def test_same_container_as_the_host_way(leon_bin, tmp_path, kind, opts):
    text = fastq_text() if kind == "fastq" else fasta_text()
    data = B.bgzf(text, cuts=cuts_of(text, seed=len(opts)), level=6)
    assert gzip.decompress(data) == text and len(data) > 3 * int(CHUNK_KB) * 1024
    path = str(tmp_path / ("reads.%s.gz" % kind))
    open(path, "wb").write(data)
    same_container_every_way(leon_bin, path, *opts, keep=True)
    if kind == "fasta" or "-lossless" in opts:
        r = run(leon_bin, "-d", "-test-file", "-file", path[:-3] + ".leon")
        assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr
    else:                                                          # lossy qualities: every other line of the file comes back
        r = run(leon_bin, "-d", "-file", path[:-3] + ".leon")
        assert r.returncode == 0, r.stderr
        got, want = open(path[:-3] + ".d", "rb").read().split(b"\n"), text.split(b"\n")
        assert len(got) == len(want) and all(g == w for i, (g, w) in enumerate(zip(got, want)) if i % 4 != 3)


def test_second_pass_over_the_file(leon_bin, tmp_path):
    """lossy qualities that do not stay resident: the second reader takes the device way too"""
    text = fastq_text(seed=35)
    path = str(tmp_path / "twice.fastq.gz")
    open(path, "wb").write(B.bgzf(text, cuts=cuts_of(text, seed=9)))
    log = same_container_every_way(leon_bin, path, env={"LEON_QUAL_RESIDENT_MB": "0"})
    assert log.count(ON_DEVICE) == 2, log
    # `auto` as it comes: a file below its threshold (64 MiB) is read on the host, without a word
    r, got = compress(leon_bin, path, "-input-inflate", "auto", env={"LEON_QUAL_RESIDENT_MB": "0"})
    r2, want = compress(leon_bin, path, env={"LEON_QUAL_RESIDENT_MB": "0"})
    assert r.returncode == 0 and r2.returncode == 0 and got == want and "input:" not in r.stdout, r.stdout


def test_line_ends_and_member_boundaries(leon_bin, tmp_path):
    # \r\n, with pairs split across member boundaries (and, with chunks of 16 KiB, across chunks)
    text = fastq_text(seed=36, end=b"\r\n")
    cuts, at = [], 0
    while True:
        at = text.find(b"\r\n", at + 40000)
        if at < 0:
            break
        cuts.append(at + 1)
    assert len(cuts) >= 5 and all(text[c - 1:c + 1] == b"\r\n" for c in cuts)
    path = str(tmp_path / "crlf.fastq.gz")
    open(path, "wb").write(B.bgzf(text, cuts=cuts))
    same_container_every_way(leon_bin, path, "-lossless")
    # a file that ends without a newline, its last member a single byte
    text = fastq_text(seed=37, last_newline=False)
    path = str(tmp_path / "no_newline.fastq.gz")
    open(path, "wb").write(B.bgzf(text, cuts=cuts_of(text, seed=2) + [len(text) - 1], eof=False))
    same_container_every_way(leon_bin, path, "-lossless")


def test_two_files_joined_and_leons_own_gz(leon_bin, tmp_path):
    a, b = fastq_text(n=1500, seed=38), fastq_text(n=1500, seed=39)
    path = str(tmp_path / "joined.fastq.gz")
    open(path, "wb").write(B.bgzf(a, member_text=20000) + B.bgzf(b, member_text=65280))       # an EOF marker in the middle
    same_container_every_way(leon_bin, path, "-lossless", keep=True)
    # what `leon -d -gz` writes, fed back
    r = run(leon_bin, "-d", "-gz", "-file", path[:-3] + ".leon")
    assert r.returncode == 0, r.stderr
    own = str(tmp_path / "own.fastq.gz")
    os.rename(path[:-3] + ".d.gz", own)
    assert gzip.decompress(open(own, "rb").read()) == a + b
    same_container_every_way(leon_bin, own, "-lossless")


def test_files_that_are_not_bgzf_take_the_host_way(leon_bin, tmp_path):
    text = fastq_text(n=1200, seed=40)
    path = str(tmp_path / "plain.fastq.gz")
    open(path, "wb").write(gzip.compress(text))
    log = same_container_every_way(leon_bin, path, "-lossless", device_line=ON_HOST)
    assert ON_DEVICE not in log and "is gzip, but not BGZF" in log
    path = str(tmp_path / "text.fastq")
    open(path, "wb").write(text)
    log = same_container_every_way(leon_bin, path, "-lossless", device_line=ON_HOST)
    assert ON_DEVICE not in log and "is not gzip" in log


def test_a_member_that_is_not_bgzf_behind_members_that_are(leon_bin, tmp_path):
    text = fastq_text(n=1200, seed=41)
    half = text.find(b"\n@", len(text) // 2) + 1
    front = B.bgzf(text[:half], member_text=30000, eof=False)
    path = str(tmp_path / "mixed.fastq.gz")
    open(path, "wb").write(front + gzip.compress(text[half:]))
    r, want = compress(leon_bin, path, "-lossless", "-input-inflate", "host")
    assert r.returncode == 0 and want, r.stderr                     # (gzread reads any series of members)
    r, got = compress(leon_bin, path, "-lossless", "-input-inflate", "device")
    assert r.returncode == 1 and got is None, r.stdout
    assert r.stderr.startswith("EXCEPTION: ") and path in r.stderr and "bytes at %d " % len(front) in r.stderr and "-input-inflate host" in r.stderr, r.stderr


def test_truncated_and_damaged_files(leon_bin, tmp_path):
    text = fastq_text(n=2500, seed=42)
    members = [B.member(text[a:a + 50000]) for a in range(0, len(text), 50000)]
    assert len(members) >= 8
    whole = b"".join(members)

    def both(name, data):
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        out = []
        for way in ("host", "device"):
            r, got = compress(leon_bin, path, "-lossless", "-input-inflate", way)
            out.append((r, got))
        return path, out

    # cut inside a member (its payload, then its header): the status, the line and the absence of a container of the host way
    for name, cut in (("cut_payload.fastq.gz", len(whole) - len(members[-1]) // 2), ("cut_header.fastq.gz", sum(len(m) for m in members[:5]) + 7)):
        path, ((rh, ch), (rd, cd)) = both(name, whole[:cut])
        assert rh.returncode == 1 and rh.stderr.startswith("EXCEPTION: " + path + " is truncated or corrupt"), rh.stderr
        assert rd.returncode == rh.returncode and rd.stderr.startswith("EXCEPTION: " + path + " is truncated or corrupt"), rd.stderr
        assert ch is None and cd is None
    # cut between two members, no EOF marker: a shorter file, and fine
    keep = sum(len(m) for m in members[:6])
    end = text.rfind(b"\n@", 0, 6 * 50000) + 1                      # (the text cut at a record's end, so that the parser has no complaint either)
    short = B.bgzf(text[:end], member_text=50000, eof=False)
    assert short[:keep - len(members[5])] == whole[:keep - len(members[5])]
    path, ((rh, ch), (rd, cd)) = both("no_eof.fastq.gz", short)
    assert rh.returncode == 0 and rd.returncode == 0 and ch and cd == ch, (rh.stderr, rd.stderr)
    # one damaged member: zlib's words on the host way, the member's number on the device way, the same line around them
    bad = bytearray(whole)
    bad[sum(len(m) for m in members[:3]) + len(members[3]) // 2] ^= 0x5A
    path, ((rh, ch), (rd, cd)) = both("damaged.fastq.gz", bytes(bad))
    assert rh.returncode == 1 and ch is None and rh.stderr.startswith("EXCEPTION: "), rh.stderr
    assert rd.returncode == 1 and cd is None, rd.stderr
    shape = rh.stderr.split(path)[0]                               # "EXCEPTION: read error in " (or the truncated-or-corrupt form, whichever zlib's verdict leads to)
    assert rd.stderr.startswith(shape + path) and path in rh.stderr, (rh.stderr, rd.stderr)
    assert "BGZF member 3 (at byte %d) does not decode" % sum(len(m) for m in members[:3]) in rd.stderr, rd.stderr     # counted in the file, not in the chunk
