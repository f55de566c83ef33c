"""tests/chain_selftest.cpp -- the host dictionary chain (host_rc.h: ChainFeed's helpers and ring, both record loops) as a program
of its own under AddressSanitizer and UndefinedBehaviorSanitizer: built here with g++ and run as a child process.  Nothing of it is
loaded into Python.  The sanitizers' runtimes are linked statically, so the program does not depend on what else the loader brings."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_selftest_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chain_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-static-libasan", "-static-libubsan", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "chain_selftest.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LEON_CHAIN_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith("chain selftest: ok")
