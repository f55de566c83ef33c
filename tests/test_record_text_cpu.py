"""No GPU: the record-text entry points (leon_records_format_device, leon_dna_decode_blocks_device, leon_device_download_pieces) with
leon_record_layout and leon_piece_sink are declared in include/leon_dna.h, bound by the Python binding and exported by the library; the
ABI version stays 5; and `leon -d -record-text` refuses a value it does not know while it parses its options, before any device is opened."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("leon_records_format_device", "leon_dna_decode_blocks_device", "leon_device_download_pieces")


@pytest.fixture(scope="module")
def built():
    import leon_amd
    leon_amd.build_library()                                      # hipcc --offload-arch=gfx950 over the tree, fmt_kernels.hip included
    return leon_amd


def test_entry_points_declared_bound_exported(built):
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    raw = ctypes.CDLL(capi.lib_path())
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/leon_dna.h"
        assert name in capi._EXPORTS and name in capi.EXPORTED_SYMBOLS, name + " is not bound"
        assert hasattr(raw, name), "libleon_dna.so does not export " + name
    assert re.search(r"typedef\s+struct\s+leon_record_layout\s*\{", src) and re.search(r"\}\s*leon_record_layout\s*;", src)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*leon_piece_sink\s*\)\s*\(\s*void\s*\*\s*user\s*,\s*uint64_t\s+offset\s*,\s*const\s+void\s*\*\s*bytes\s*,\s*uint64_t\s+size\s*\)", src)
    assert capi.ABI_VERSION == 5 and raw.leon_dna_abi_version() == 5          # additions only
    assert re.search(r"#define\s+LEON_DNA_ABI_VERSION\s+5\b", src)
    for fn in ("records_format_device", "device_download_pieces", "device_alloc"):
        assert callable(getattr(capi, fn))
    assert callable(capi.DnaEncodeContext.decode_blocks_device)


def test_layout_binding_matches_the_header(built):
    """the ctypes mirror of leon_record_layout has the header's fields in the header's order, and no padding the C struct lacks"""
    from leon_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "leon_dna.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+leon_record_layout\s*\{(.*?)\}\s*leon_record_layout\s*;", src, flags=re.S).group(1)
    fields = re.findall(r"(uint8_t|uint32_t|uint64_t)\s+([a-z0-9_]+)\s*;", body)
    assert [f[1] for f in fields] == [n for n, _ in capi.RecordLayout._fields_]
    for want in ("struct_size", "lead", "fastq", "plus_kind", "wrap", "first_read_index"):
        assert want in [f[1] for f in fields]
    sizes = {"uint8_t": 1, "uint32_t": 4, "uint64_t": 8}
    assert ctypes.sizeof(capi.RecordLayout) == sum(sizes[t] for t, _ in fields)          # naturally aligned: the same bytes on both sides
    for (t, name), (_, ct) in zip(fields, capi.RecordLayout._fields_):
        assert ctypes.sizeof(ct) == sizes[t], name


def test_cli_refuses_unknown_record_text_without_a_device(built, tmp_path):
    leon = os.path.join(ROOT, "leon_amd", "lib", "leon")
    nothing = str(tmp_path / "nothing.leon")
    for args, word in ((["-record-text", "gpu"], "'gpu'"), (["-record-text"], "needs a value")):
        r = subprocess.run([leon, "-file", nothing, "-d"] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.startswith("EXCEPTION: ") and "-record-text" in r.stderr and word in r.stderr, (args, r.stderr)
    # a known value gets as far as the file (which is not there): the option itself was accepted
    for value in ("host", "device", "auto"):
        r = subprocess.run([leon, "-file", nothing, "-d", "-record-text", value, "-header-text", "device"], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("EXCEPTION: ") and "-record-text" not in r.stderr, (value, r.stderr)


def test_no_device_no_formatting(built):
    """without a HIP device the entry points fail with a status and a message (the product has no CPU path); arguments are refused first"""
    import torch
    from leon_amd import capi
    with pytest.raises(capi.LeonDnaError) as e:
        capi.records_format_device(0, 0, 0, 0, 0, 0, struct_size=8)
    assert e.value.code == -1 and "struct_size" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        capi.records_format_device(0, 0, 0, 0, 0, 0, fastq=True, d_quals=None)
    assert e.value.code == -1 and "d_quals" in str(e.value)
    with pytest.raises(capi.LeonDnaError) as e:
        capi.records_format_device(0, 0, 0, 0, 0, 0, fastq=False, plus_kind=1)
    assert e.value.code == -1 and "d_hdr_text" in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(capi.LeonDnaError) as e:
            capi.records_format_device(16, 16, 1, 0, 16, 64, fastq=False)
        assert e.value.code in (-2, -3)
