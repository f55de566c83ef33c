"""No GPU: leon_qual_inflate_blocks_device is declared in include/leon_dna.h, bound by the Python binding and exported by the library; the
ABI version stays 5; `leon -d -qual-inflate` refuses a value it does not know while it parses its options, before any device is opened;
the entry point refuses its arguments before it touches a device, with leon_host_qual_decode_blocks' words, and fails with a status --
no fallback -- where there is no HIP device."""
import ctypes
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "leon_qual_inflate_blocks_device"


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()                                      # hipcc --offload-arch=gfx950 over the tree, inflate_kernels.hip included
    return leon_amd


def test_entry_point_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    raw = ctypes.CDLL(capi.lib_path())
    assert re.search(r"\bint\s+%s\s*\(\s*int\s+device_id\s*,\s*const\s+uint8_t\s*\*\s*payloads\s*,\s*const\s+uint64_t\s*\*\s*payload_off" % NAME, src)
    assert NAME in capi._EXPORTS and NAME in capi.EXPORTED_SYMBOLS, NAME + " is not bound"
    assert hasattr(raw, NAME), "libleon_dna.so does not export " + NAME
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # an addition
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    assert callable(capi.qual_inflate_blocks_device) and callable(capi.qual_inflate_blocks)
    assert os.path.exists(os.path.join(ROOT, "leon_amd", "csrc", "inflate_kernels.hip"))
    assert "inflate_kernels.o" in open(os.path.join(ROOT, "leon_amd", "csrc", "Makefile")).read()


def test_cli_refuses_unknown_qual_inflate_without_a_device(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.leon")
    for args, word in ((["-qual-inflate", "gpu"], "'gpu'"), (["-qual-inflate"], "needs a value")):
        r = subprocess.run([leon, "-file", nothing, "-d"] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.startswith("EXCEPTION: ") and "-qual-inflate" in r.stderr and word in r.stderr, (args, r.stderr)
    # a known value gets as far as the file (which is not there): the option itself was accepted
    for value in ("host", "device", "auto"):
        r = subprocess.run([leon, "-file", nothing, "-d", "-qual-inflate", value, "-record-text", "device"], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-qual-inflate" not in r.stderr, (value, r.stderr)


def test_arguments_are_refused_before_the_device(built):
    """the refusals of leon_host_qual_decode_blocks, in its words, with pointers no device call could survive"""
    import torch
    from leon_amd import capi
    pay = np.frombuffer(zlib.compress(b"II\n") * 2, dtype=np.uint8)
    n = len(pay) // 2
    off = np.array([0, n, 2 * n], dtype=np.uint64)
    nr, nb = np.array([1, 1], dtype=np.uint32), np.array([2, 2], dtype=np.uint64)

    def host(payloads, offsets, cap):
        out, out_off = np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
        lib = capi.load_library()
        vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        f = lib.leon_host_qual_decode_blocks
        saved = f.argtypes
        f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32]
        try:
            rc = f(vp(payloads), vp(offsets), vp(nr), vp(nb), 2, vp(out), cap, vp(out_off), 1)
        finally:
            f.argtypes = saved
        return rc, (lib.leon_last_error(None) or b"").decode()

    for payloads, offsets, cap, word in ((None, off, 4, "null argument"),
                                         (pay, np.array([0, 2 * n, n], dtype=np.uint64), 4, "payload offsets are not monotonic"),
                                         (pay, off, 3, "output capacity below the sum of block_n_bytes")):
        want = host(payloads, offsets, cap)
        assert want[0] == -1 and word in want[1], want
        with pytest.raises(capi.LeonDnaError) as e:
            capi.qual_inflate_blocks_device(payloads, offsets, nr, nb, 0x10, cap, 0x10, 0, n_blocks=2)     # (d_quals: not a pointer anything may touch)
        assert e.value.code == -1 and str(e.value).endswith(want[1]), (str(e.value), want)
    with pytest.raises(capi.LeonDnaError) as e:
        capi.qual_inflate_blocks_device(pay, off, nr, nb, 0, 4, 0x10, 0, n_blocks=2)                      # no d_quals
    assert e.value.code == -1 and "null argument" in str(e.value)
    assert capi.qual_inflate_blocks_device(None, None, None, None, 0, 0, 0, 0, n_blocks=0) == 0            # a call of 0 blocks: nothing to do, as on the host
    if not torch.cuda.is_available():
        with pytest.raises(capi.LeonDnaError) as e:                                                        # no device: a status, not a fallback
            capi.qual_inflate_blocks_device(pay, off, nr, nb, 0x10, 4, 0x10, 0, n_blocks=2)
        assert e.value.code in (-2, -3), (e.value.code, str(e.value))
        with pytest.raises(capi.LeonDnaError) as e:
            capi.qual_inflate_blocks([(0, pay[:n].tobytes(), 1)], [2])
        assert e.value.code in (-2, -3)
