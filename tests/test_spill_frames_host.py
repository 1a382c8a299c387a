"""Host side of the checkpoint spill (rw_codec.hpp put_frame / for_each_frame /
merge_frames, KeyedDelta, write_sorted, RowReader): round trip, the pinned
frame layout, truncated and over-long streams, the replay rule, writer order
and cut value rows — checked by a stand-alone C++ program
(tests/spill_frames_host_check.cpp), built with the host compiler and run
twice: plain, and under AddressSanitizer + UBSan. Nothing is loaded into
Python.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "spill_frames_host_check.cpp")


@pytest.mark.parametrize("flags", [
    [],
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"],
], ids=["plain", "asan_ubsan"])
def test_spill_frames_host_check(flags, tmp_path):
    exe = str(tmp_path / "spill_frames_host_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "spill frames host check ok" in run.stdout
