"""Editing a `.leon` container from outside, for the tests that damage one: a dataset's values through HDF5's own h5dump, the place of
its raw bytes in the file (the container's datasets are contiguous and unfiltered, so the values lie in the file as they are), and a
patch of bytes at a place."""
import os
import subprocess

import numpy as np

H5BIN = "/opt/conda/bin"


def h5_has(path, name):
    r = subprocess.run([os.path.join(H5BIN, "h5ls"), "-r", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return "/" + name in {l.split()[0] for l in r.stdout.splitlines() if l.strip()}


def h5_dataset(path, name, dtype=np.uint8):
    out = path + ".dump"
    r = subprocess.run([os.path.join(H5BIN, "h5dump"), "-d", "/" + name, "-b", "LE", "-o", out, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, dtype=dtype)
    os.remove(out)
    return data


def find_bytes(path, content):
    """the one place where `content` lies in the file"""
    content = bytes(content)
    assert content, "nothing to look for"
    data = open(path, "rb").read()
    at = data.find(content)
    assert at >= 0, "the bytes are not in %s as they are" % path
    assert data.find(content, at + 1) < 0, "the bytes lie in %s more than once" % path
    return at


def find_dataset(path, name, dtype=np.uint8):
    """(values, offset of the dataset's raw bytes in the file)"""
    values = h5_dataset(path, name, dtype)
    return values, find_bytes(path, values.astype(np.dtype(dtype).newbyteorder("<")).tobytes())


def patch(path, at, new):
    """overwrites len(new) bytes at offset `at`; the file keeps its size"""
    new = bytes(new)
    size = os.path.getsize(path)
    assert 0 <= at and at + len(new) <= size
    with open(path, "r+b") as f:
        f.seek(at)
        f.write(new)
    assert os.path.getsize(path) == size


def flip_bit(path, at, bit=0):
    with open(path, "rb") as f:
        f.seek(at)
        old = f.read(1)[0]
    patch(path, at, bytes([old ^ (1 << bit)]))
