"""Host side of the RwChunk boundary (rw_chunkbuild.hpp free_chunk / Builder /
slice_ranges / ChunkQueue, rw_varlen.hpp check_column / ref_words): fixed,
decimal, raw and varchar fillers over row-major and column-major blocks, the
over-long varchar refusal, builders abandoned half way, the slicing table, the
queue, the column check and the reference words — checked by a stand-alone C++
program (tests/chunk_build_host_check.cpp), built with the host compiler and
run twice: plain, and under AddressSanitizer + UBSan, where every chunk is
freed through free_chunk so allocation/free pairing and leaks are checked.
Nothing is loaded into Python.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "chunk_build_host_check.cpp")


@pytest.mark.parametrize("flags", [
    [],
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"],
], ids=["plain", "asan_ubsan"])
def test_chunk_build_host_check(flags, tmp_path):
    exe = str(tmp_path / "chunk_build_host_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "chunk build host check ok" in run.stdout
