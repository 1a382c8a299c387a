"""Host-side varchar pieces — the spill codec's string datum and the arena
reference-word helpers — checked by a stand-alone C++ program
(tests/varchar_host_check.cpp), built with the host compiler and run twice:
plain, and under AddressSanitizer + UBSan. Nothing is loaded into Python.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "varchar_host_check.cpp")


@pytest.mark.parametrize("flags", [
    [],
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"],
], ids=["plain", "asan_ubsan"])
def test_varchar_host_check(flags, tmp_path):
    exe = str(tmp_path / "varchar_host_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "varchar host check ok" in run.stdout
