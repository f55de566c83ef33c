"""No GPU: the arithmetic of `leon -d` that needs no device (leon_amd/host/leon_plan.hpp: record lengths, the rounds' shares of the letter
tables, the checks on a container's metadata) in a stand-alone program (tests/host_plan_check.cpp) that holds its own brute-force models,
built plain and with AddressSanitizer + UBSan.  The GPU tests of the CLI (tests/test_host_cli*.py) reach the same code through `leon -d`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.parametrize("san", ["plain", "address,undefined"])
def test_host_plan_stand_alone(tmp_path, san):
    flags = ["-O2"]
    if san != "plain":
        if not _lib("libasan.so") or not _lib("libubsan.so"):
            pytest.skip("no libasan / libubsan in this toolchain")
        flags = ["-O1", "-g", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    exe = str(tmp_path / "host_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "host_plan_check: ok, " in r.stdout
    print(r.stdout.strip())
