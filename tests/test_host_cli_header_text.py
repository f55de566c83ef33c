"""-m gpu: `leon -d -header-text host|device|auto` through the built binary: the restored file is the same bytes whoever
rebuilds the header text (the host threads, or k_hdr_text on the device with the host decoder behind it)."""
import os
import subprocess

import pytest

import common
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def leon_bin():
    import leon_amd
    leon_amd.build_library()
    return LEON


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def _fastq(path, n, L, seed, heads=None):
    bases, off = common.synthetic(n, L, 6000, seed=seed)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(n)]
    heads = heads or H.sra(n, seed=seed)
    quals = [(q * (len(r) // max(len(q), 1) + 1))[:len(r)] if q else b"I" * len(r) for q, r in zip(H.fastq_quals(n, 0, seed=seed), reads)]
    with open(path, "wb") as f:
        for h, s, q in zip(heads, reads, quals):
            f.write(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
    return open(path, "rb").read()


def test_header_text_option_restores_the_same_file(leon_bin, tmp_path):
    fq = str(tmp_path / "SRR.fastq")
    original = _fastq(fq, 6000, 80, seed=11)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    for opt in ([], ["-header-text", "host"], ["-header-text", "device"], ["-header-text", "auto"]):
        if os.path.exists(fq + ".d"):
            os.remove(fq + ".d")
        r = run(leon_bin, "-d", "-file", fq + ".leon", "-verbose", "1", *opt)
        assert r.returncode == 0, (opt, r.stderr)
        assert open(fq + ".d", "rb").read() == original, opt
        if opt == ["-header-text", "device"]:
            assert "header text: device" in r.stdout and " 0 of 1 blocks fell back" in r.stdout, r.stdout
        if opt in ([], ["-header-text", "host"]):
            assert "header text: host threads" in r.stdout, r.stdout
    r = run(leon_bin, "-d", "-test-file", "-file", fq + ".leon", "-header-text", "device")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_header_text_device_in_rounds_and_over_the_cap(leon_bin, tmp_path):
    from leon_amd import capi
    # two read blocks decoded in rounds of one: each round fetches its own block from the one device call
    fq = str(tmp_path / "two.fastq")
    original = _fastq(fq, 50300, 40, seed=12)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "21")
    assert r.returncode == 0, r.stderr
    r = run(leon_bin, "-d", "-file", fq + ".leon", "-header-text", "device", "-verbose", "1", env=dict(os.environ, LEON_DECODE_BLOCKS="1"))
    assert r.returncode == 0, r.stderr
    assert open(fq + ".d", "rb").read() == original
    assert " 0 of 2 blocks fell back" in r.stdout, r.stdout
    # one header longer than the kernel builds: its block is rebuilt by the host decoder, the file is the same
    fq = str(tmp_path / "long.fastq")
    heads = H.sra(3000, seed=13)
    heads[1500] = b"x" * (capi.HEADER_TEXT_DEVICE_CAP + 1) + b" 77"
    original = _fastq(fq, 3000, 80, seed=13, heads=heads)
    r = run(leon_bin, "-c", "-lossless", "-file", fq, "-kmer-size", "25")
    assert r.returncode == 0, r.stderr
    r = run(leon_bin, "-d", "-test-file", "-file", fq + ".leon", "-header-text", "device", "-verbose", "1")
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr
    assert open(fq + ".d", "rb").read() == original
    assert " 1 of 1 blocks fell back" in r.stdout, r.stdout


def test_header_text_option_is_checked(leon_bin, tmp_path):
    for args in (["-header-text", "gpu"], ["-header-text"]):
        r = run(leon_bin, "-file", str(tmp_path / "nothing.leon"), "-d", *args)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-header-text" in r.stderr, (args, r.stderr)
