"""Host check of include/rw_xpayload.hpp — the exchange block layout and the
host version of the varchar vnode CRC feed — by a stand-alone C++ program
(tests/xpayload_host_check.cpp), built with the host compiler and run twice:
plain, and under AddressSanitizer + UBSan. Nothing is loaded into Python.

The CRC vectors are computed here with zlib over the hash_datum byte feed
(rwtest/xpayload.py) and handed to the program in a file.
"""
import os
import subprocess
import zlib

import pytest

from rwtest import xpayload as xp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "xpayload_host_check.cpp")


def _s(n, seed=1):
    return bytes((seed * 131 + 17 * i) & 0xFF for i in range(n))


CASES = (
    [[_s(n, n)] for n in (0, 1, 7, 8, 9, 15, 16, 17, 300)]
    + [[None],
       [12345, _s(9), None],
       [None, _s(0), -7],
       [_s(16), _s(17), 2**62],
       [b"\xff"], [b"\x00"], [b"\xff" * 8]])


def _vector_file(path):
    with open(path, "w") as f:
        for datums in CASES:
            toks = []
            for v in datums:
                if v is None:
                    toks.append("n")
                elif isinstance(v, bytes):
                    toks.append("s" + v.hex())
                else:
                    toks.append(f"i{v}")
            f.write(f"{zlib.crc32(xp.feed(datums)):08x} {' '.join(toks)}\n")


def test_feed_distinguishes_empty_from_null():
    assert xp.feed([b""]) == b"\xff"
    assert xp.feed([None]) == b"\xf0\xff\xff\xff"
    assert xp.feed([b"ab", 1]) == b"ab\xff" + (1).to_bytes(8, "little")


@pytest.mark.parametrize("flags", [
    [],
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"],
], ids=["plain", "asan_ubsan"])
def test_xpayload_host_check(flags, tmp_path):
    exe = str(tmp_path / "xpayload_host_check")
    vec = str(tmp_path / "crc_vectors.txt")
    _vector_file(vec)
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, vec], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"xpayload host check ok ({len(CASES)} crc vectors)" in run.stdout
