"""-m gpu: the anchor dictionary in independently coded pieces through the built binary.  `leon -c -dict-pieces [-dict-piece-anchors N]` writes
leon/anchors/dict_pieces and leon/anchors/dict_piece_table INSTEAD of leon/anchors/dict (coded on the device, k_dict_encode_pieces); `leon -d`
needs no option: it checks the table (leon_plan.hpp) and decodes the pieces on the device (k_dict_decode_pieces).  Everything else of the
container is what the run without the option writes.  A container changed from outside ends -d with `EXCEPTION: <file>: dictionary pieces:
...`, status 1 and no output file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import container_patch as CP
import hdr_samples as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEON = os.path.join(ROOT, "leon_amd", "lib", "leon")

pytestmark = pytest.mark.gpu

RPB, K = 50000, 25
PIECES, TABLE, SINGLE = "leon/anchors/dict_pieces", "leon/anchors/dict_piece_table", "leon/anchors/dict"
P_N_ANCHORS = 6                                                    # leon/metadata/params (leon_container.hpp)


def run(*args, **kw):
    return subprocess.run(list(args), capture_output=True, text=True, **kw)


def write_fastq(path, n, seed):
    bases, off = common.synthetic(n, 70, 6000, seed=seed, n_rate=0.002, err=0.02)
    lens = np.random.default_rng(seed).integers(36, 71, n)
    heads = H.sra(n, seed=seed)
    with open(path, "wb") as f:
        for i in range(n):
            s = bases[int(off[i]):int(off[i]) + int(lens[i])]
            f.write(b"@" + heads[i] + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def compress(fq, *opts, env=None):
    r = run(LEON, "-c", "-file", fq, "-kmer-size", str(K), "-lossless", *opts, env=env)
    assert r.returncode == 0, r.stderr
    return fq + ".leon", r.stdout


def decode(container, *opts, expect=0):
    out = container[:-5] + ".d"
    if os.path.exists(out):
        os.remove(out)
    r = run(LEON, "-d", "-file", container, "-verbose", "1", *opts)
    assert r.returncode == expect, (opts, r.stdout, r.stderr)
    return os.path.exists(out), r


def datasets_but_the_dictionary(path):
    r = run(os.path.join(CP.H5BIN, "h5ls"), "-r", path)
    assert r.returncode == 0, r.stderr
    names = [l.split()[0][1:] for l in r.stdout.splitlines() if "Dataset" in l]
    return sorted(n for n in names if not n.startswith("leon/anchors/"))


@pytest.fixture(scope="module", autouse=True)
def leon_bin():
    import leon_amd
    if not (os.path.exists(LEON) and os.path.exists(leon_amd.lib_path())):
        leon_amd.build_library()
    return LEON


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """110 000 reads (three blocks): the container without the option, with it, and with pieces of 5 anchors"""
    d = tmp_path_factory.mktemp("dict_pieces")
    fq = str(d / "SRR.fastq")
    write_fastq(fq, 2 * RPB + 10000, seed=47)
    out = {"fq": fq, "dir": d}
    for name, opts in (("plain", ()), ("pieced", ("-dict-pieces", "-verbose", "1")), ("five", ("-dict-pieces", "-dict-piece-anchors", "5"))):
        container, log = compress(fq, *opts)
        out[name] = str(d / (name + ".fastq.leon"))
        shutil.copy(container, out[name])
        out[name + "_log"] = log
    shutil.copy(fq, str(d / "pieced.fastq"))                       # (-test-file looks for the original beside the output)
    shutil.copy(fq, str(d / "five.fastq"))
    shutil.copy(fq, str(d / "plain.fastq"))
    return out


def test_round_trip_and_the_way_is_named(files):
    n_anchors = int(CP.h5_dataset(files["pieced"], "leon/metadata/params", np.uint64)[P_N_ANCHORS])
    n_pieces = (n_anchors + 1023) // 1024
    size = len(CP.h5_dataset(files["pieced"], PIECES))
    assert "dictionary: %d pieces of 1024 anchors on the device (k_dict_encode_pieces), %d bytes" % (n_pieces, size) in files["pieced_log"], files["pieced_log"]
    ok, r = decode(files["pieced"], "-test-file")
    assert ok and "is identical to" in r.stdout and "dictionary: %d pieces of 1024 anchors decoded on the device (k_dict_decode_pieces)" % n_pieces in r.stdout, r.stdout
    ok, r = decode(files["plain"], "-test-file")                    # a container without the option takes the way it took
    assert ok and "is identical to" in r.stdout and "dictionary: one stream" in r.stdout and "k_dict_decode_pieces" not in r.stdout


def test_datasets_and_table(files):
    from leon_amd import capi
    assert CP.h5_has(files["pieced"], PIECES) and CP.h5_has(files["pieced"], TABLE) and not CP.h5_has(files["pieced"], SINGLE)
    assert CP.h5_has(files["plain"], SINGLE) and not CP.h5_has(files["plain"], PIECES) and not CP.h5_has(files["plain"], TABLE)
    params = CP.h5_dataset(files["pieced"], "leon/metadata/params", np.uint64)
    assert np.array_equal(params, CP.h5_dataset(files["plain"], "leon/metadata/params", np.uint64))      # the container revision included
    n_anchors = int(params[P_N_ANCHORS])
    assert n_anchors > 3 * 1024
    kmers = capi.anchor_dict_decode(CP.h5_dataset(files["plain"], SINGLE).tobytes(), n_anchors, K)
    for name, P in (("pieced", 1024), ("five", 5)):
        t = CP.h5_dataset(files[name], TABLE, np.uint64)
        pieces = CP.h5_dataset(files[name], PIECES).tobytes()
        assert t[0] == 1 and t[1] == P and len(t) - 2 == (n_anchors + P - 1) // P and int(t[2:].sum()) == len(pieces) and t[2:].min() >= 8
        want, off = capi.host_anchor_dict_encode_pieces(kmers, K, P)
        assert pieces == want and np.array_equal(np.diff(off), t[2:]), name


def test_the_rest_of_the_container_does_not_move(files):
    names = datasets_but_the_dictionary(files["plain"])
    assert names == datasets_but_the_dictionary(files["pieced"]) == datasets_but_the_dictionary(files["five"])
    assert sum(n.startswith("leon/dna/block_") for n in names) == 3
    for n in names:
        a = CP.h5_dataset(files["plain"], n)                        # (the raw bytes, whatever the dataset's type)
        assert np.array_equal(a, CP.h5_dataset(files["pieced"], n)) and np.array_equal(a, CP.h5_dataset(files["five"], n)), n


def test_pieces_of_five_anchors_round_trip(files):
    ok, r = decode(files["five"], "-test-file")
    assert ok and "is identical to" in r.stdout and " pieces of 5 anchors decoded on the device" in r.stdout


def test_two_contexts_on_the_one_device_write_the_same_container(files):
    container, _ = compress(files["fq"], "-dict-pieces", "-gpus", "2", env=dict(os.environ, LEON_SHARE_GPU="1"))
    assert run(os.path.join(CP.H5BIN, "h5diff"), files["pieced"], container).returncode == 0


def test_option_refusals(files):
    for args, words in ((["-d", "-dict-pieces"], "option -dict-pieces belongs to -c"),
                        (["-c", "-dict-piece-anchors", "5"], "option -dict-piece-anchors belongs to -dict-pieces"),
                        (["-d", "-dict-piece-anchors", "5"], "option -dict-piece-anchors belongs to -dict-pieces"),
                        (["-c", "-dict-pieces", "-dict-piece-anchors", "0"], "-dict-piece-anchors must be in 1..1048576"),
                        (["-c", "-dict-pieces", "-dict-piece-anchors", "1048577"], "-dict-piece-anchors must be in 1..1048576"),
                        (["-c", "-dict-pieces", "-dict-piece-anchors", "many"], "is not a number"),
                        (["-c", "-dict-pieces", "-dict-piece-anchors"], "needs a value")):
        r = run(LEON, "-file", "/nonexistent/x.fastq", *args)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and words in r.stderr, (args, r.stderr)
    assert not os.path.exists("/nonexistent/x.fastq.leon")


def _refused(container, words):
    ok, r = decode(container, expect=1)
    assert not ok, "a refused container left an output file"
    assert r.stderr.startswith("EXCEPTION: %s: dictionary pieces: " % container) and words in r.stderr, r.stderr


def test_patched_containers_are_refused(files):
    d = files["dir"]
    # a table size off by one
    c = str(d / "size.fastq.leon")
    shutil.copy(files["pieced"], c)
    t, at = CP.find_dataset(c, TABLE, np.uint64)
    CP.patch(c, at + 8 * 3, np.array([t[3] + 1], dtype="<u8").tobytes())
    _refused(c, "the piece sizes add up to")
    # both forms in one file: the single stream of the run without the option, copied in with HDF5's own h5copy
    c = str(d / "both.fastq.leon")
    shutil.copy(files["pieced"], c)
    r = run(os.path.join(CP.H5BIN, "h5copy"), "-i", files["plain"], "-o", c, "-s", "/" + SINGLE, "-d", "/" + SINGLE)
    assert r.returncode == 0 and CP.h5_has(c, SINGLE) and CP.h5_has(c, PIECES), r.stderr
    _refused(c, "holds %s as well" % SINGLE)
    # a piece corrupted: piece 1 begins with eight 0xFF bytes -- its first symbol decodes as a fifth one
    c = str(d / "corrupt.fastq.leon")
    shutil.copy(files["pieced"], c)
    _, at = CP.find_dataset(c, PIECES)
    CP.patch(c, at + int(t[2]), b"\xff" * 8)
    _refused(c, "anchor dictionary piece 1 does not decode")
