"""No GPU: the device header-text entry points are declared in include/leon_dna.h, bound by the Python binding and exported by
the library; and `leon -d -header-text` refuses a value it does not know while it parses its options, before any device is opened."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("leon_header_decode_blocks_device", "leon_header_decode_text", "leon_header_text_fetch", "leon_header_text_device_ptr",
         "leon_header_text_free")


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()
    return leon_amd


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    raw = ctypes.CDLL(capi.lib_path())
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/leon_dna.h"
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS, name + " is not bound"
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert "typedef struct leon_header_text leon_header_text;" in src
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    for method in ("header_decode_blocks_device", "header_text_set"):
        assert callable(getattr(capi.DnaEncodeContext, method))
    assert capi.HEADER_TEXT_DEVICE_CAP == 4096


def test_cli_refuses_unknown_header_text_without_a_device(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.leon")
    for args, word in ((["-header-text", "gpu"], "'gpu'"), (["-header-text"], "needs a value")):
        r = subprocess.run([leon, "-file", nothing, "-d"] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.startswith("EXCEPTION: ") and "-header-text" in r.stderr and word in r.stderr, (args, r.stderr)
    # a known value gets as far as the file (which is not there): the option itself was accepted
    for value in ("host", "device", "auto"):
        r = subprocess.run([leon, "-file", nothing, "-d", "-header-text", value], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-header-text" not in r.stderr, (value, r.stderr)
