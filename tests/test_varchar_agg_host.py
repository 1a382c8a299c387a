"""Host-side pieces of HashAgg's varchar group keys — the memcomparable
string datum of the spill key (rw_codec.hpp memcmp_encode_str: pinned
vectors, order preservation, injectivity) and the value-encoded string
inside a multi-column row — checked by a stand-alone C++ program
(tests/agg_varchar_host_check.cpp), built with the host compiler and run
twice: plain, and under AddressSanitizer + UBSan. Nothing is loaded into
Python.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "agg_varchar_host_check.cpp")


@pytest.mark.parametrize("flags", [
    [],
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"],
], ids=["plain", "asan_ubsan"])
def test_agg_varchar_host_check(flags, tmp_path):
    exe = str(tmp_path / "agg_varchar_host_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "agg varchar host check ok" in run.stdout
