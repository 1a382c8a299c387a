"""Varchar dist keys through rw_vnode_compute and varchar columns through
rw_dispatch_compute.

Reference: zlib.crc32 over the hash_datum byte feed (rwtest/xpayload.py):
a non-NULL varchar feeds its bytes then one 0xFF, NULL the 4-byte sentinel.
The CPU oracle has no string type and is not a reference here.
"""
import ctypes as C

import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest import xpayload as xp
from rwtest.ffi import T_I64
from rwtest.varchar import RW_E_INVAL, T_VARCHAR, VChunk
from test_vnode_dispatch import RwDispatchDesc, RwVnodeDesc, bind

pytestmark = pytest.mark.gpu

OP_INSERT, OP_DELETE, OP_UD, OP_UI = 0, 1, 2, 3


@pytest.fixture(scope="module")
def gpu():
    import risingwave_amd

    lib = ffi.Lib(risingwave_amd.lib_path())
    bind(lib)
    return lib


def vnodes_rc(lib, cc, n_rows, keys, vnode_count=256):
    d = RwVnodeDesc()
    ki = (C.c_uint32 * len(keys))(*keys)
    d.n_keys = len(keys)
    d.key_indices = ki
    d.vnode_count = vnode_count
    out = (C.c_uint16 * max(n_rows, 1))()
    rc = lib.lib.rw_vnode_compute(C.byref(d), C.byref(cc), out)
    return rc, list(out)[:n_rows]


def vnodes(lib, chunk, keys, vnode_count=256):
    rc, out = vnodes_rc(lib, chunk.to_c(), chunk.n_rows, keys, vnode_count)
    assert rc == 0, lib.last_error()
    return out


# 1. single varchar key, 1000 rows: not a multiple of 64 or 256, > 1 block
def test_vnode_single_varchar_key(gpu):
    rng = np.random.default_rng(1401)
    names = xp.name_column(rng, 1000)
    assert b"" in names and None in names and xp.HUGE in names
    assert {len(s) for s in names if s is not None} >= set(range(0, 18))
    c = VChunk([T_VARCHAR], [0] * 1000, [names])
    got = vnodes(gpu, c, [0])
    want = [xp.expected_vnode([s]) for s in names]
    assert got == want, next((r, names[r][:20] if names[r] else names[r])
                             for r in range(1000) if got[r] != want[r])
    # "" and NULL were fed differently (and land apart under this CRC)
    assert xp.feed([b""]) != xp.feed([None])
    assert got[names.index(b"")] == xp.expected_vnode([b""])
    assert got[names.index(None)] == xp.expected_vnode([None])
    assert xp.expected_vnode([b""]) != xp.expected_vnode([None])


# 2. key tuples with NULLs in each position; non-power-of-two vnode_count
@pytest.mark.parametrize("vnode_count", [256, 100])
@pytest.mark.parametrize("shape", ["iv", "vi", "vv"])
def test_vnode_key_tuples(gpu, shape, vnode_count):
    rng = np.random.default_rng(1402)
    n = 333
    ints = [None if rng.random() < 0.15 else int(rng.integers(-2**62, 2**62))
            for _ in range(n)]
    s1 = xp.name_column(rng, n)
    s2 = list(reversed(xp.name_column(rng, n)))
    cols = {"iv": [ints, s1], "vi": [s1, ints], "vv": [s1, s2]}[shape]
    types = [T_I64 if ch == "i" else T_VARCHAR for ch in shape]
    for col in cols:
        assert None in col
    # an unkeyed column in front: key_indices need not start at 0
    c = VChunk([T_I64] + types, [0] * n, [list(range(n))] + cols)
    got = vnodes(gpu, c, [1, 2], vnode_count)
    want = [xp.expected_vnode([cols[0][r], cols[1][r]], vnode_count)
            for r in range(n)]
    assert got == want


# 3. degenerate sizes
def test_vnode_one_and_zero_rows(gpu):
    c = VChunk([T_VARCHAR], [0], [[b"solo"]])
    assert vnodes(gpu, c, [0]) == [xp.expected_vnode([b"solo"])]
    c = VChunk([T_VARCHAR], [], [[]])
    assert vnodes(gpu, c, [0]) == []


# 4. malformed offsets: RW_E_INVAL with a message; a valid call still works
@pytest.mark.parametrize("offsets,n", [
    ([0, 5, 4, 9], 3),          # non-monotone
    ([1, 2, 3], 2),             # offsets[0] != 0
    ([0, 1 << 24], 1),          # a claimed length of 2^24
], ids=["non_monotone", "first_nonzero", "len_2p24"])
def test_vnode_malformed_offsets(gpu, offsets, n):
    vd, keep = vc.raw_varchar_chunk(n, offsets)
    valid = np.ones(n, np.uint8)
    ops = np.zeros(n, np.uint8)
    cols = (ffi.RwColumn * 1)()
    cols[0].type = T_VARCHAR
    cols[0].valid = valid.ctypes.data
    cols[0].data = C.addressof(vd)
    cc = ffi.RwChunkC()
    cc.n_rows, cc.n_cols = n, 1
    cc.ops = C.cast(ops.ctypes.data, C.POINTER(C.c_uint8))
    cc.vis = None
    cc.cols = cols
    rc, _ = vnodes_rc(gpu, cc, n, [0])
    assert rc == RW_E_INVAL
    assert "varchar" in gpu.last_error()
    # dispatch validates the same way, before building any output
    d = RwDispatchDesc()
    ki = (C.c_uint32 * 1)(0)
    d.v.n_keys, d.v.key_indices, d.v.vnode_count = 1, ki, 256
    d.n_outputs = 2
    v2o = (C.c_uint32 * 256)(*[v % 2 for v in range(256)])
    d.vnode_to_output = v2o
    outs = (C.POINTER(ffi.RwChunkC) * 2)()
    assert gpu.lib.rw_dispatch_compute(C.byref(d), C.byref(cc), outs) == \
        RW_E_INVAL
    assert not outs[0] and not outs[1]
    good = VChunk([T_VARCHAR], [0, 0], [[b"after", None]])
    assert vnodes(gpu, good, [0]) == [xp.expected_vnode([b"after"]),
                                      xp.expected_vnode([None])]


def dispatch(lib, chunk, keys, n_outputs, vnode_count=256):
    d = RwDispatchDesc()
    ki = (C.c_uint32 * len(keys))(*keys)
    d.v.n_keys, d.v.key_indices, d.v.vnode_count = len(keys), ki, vnode_count
    d.n_outputs = n_outputs
    v2o = (C.c_uint32 * vnode_count)(*[v % n_outputs
                                       for v in range(vnode_count)])
    d.vnode_to_output = v2o
    outs = (C.POINTER(ffi.RwChunkC) * n_outputs)()
    cc = chunk.to_c()
    rc = lib.lib.rw_dispatch_compute(C.byref(d), C.byref(cc), outs)
    assert rc == 0, lib.last_error()
    # the type-7-aware reader; it frees each output with rw_chunk_free
    return [vc.read_chunk(lib, outs[o]) for o in range(n_outputs)]


# 5. 4 outputs, schema (i64, varchar, varchar, i64), some rows invisible
@pytest.mark.parametrize("key", [0, 1], ids=["key_i64", "key_varchar"])
def test_dispatch_carries_varchar(gpu, key):
    rng = np.random.default_rng(1405)
    n = 300
    a = [None if rng.random() < 0.1 else int(rng.integers(0, 80))
         for _ in range(n)]
    s1 = xp.name_column(rng, n)
    s2 = list(reversed(xp.name_column(rng, n)))
    uniq = list(range(n))  # makes every row distinct
    vis = (rng.random(n) > 0.2).astype(np.uint8)
    assert 0 < vis.sum() < n
    types = [T_I64, T_VARCHAR, T_VARCHAR, T_I64]
    c = VChunk(types, [0] * n, [a, s1, s2, uniq], vis)
    outs = dispatch(gpu, c, [key], 4)
    seen = {}
    for o, oc in enumerate(outs):
        assert oc.types == types and oc.n_rows == n
        for _, row in oc.visible_rows():
            assert row[3] not in seen, "row on two outputs"
            seen[row[3]] = o
            r = row[3]
            assert row == (a[r], s1[r], s2[r], r)  # strings and NULLs intact
            assert xp.expected_vnode([row[key]]) % 4 == o
    assert sorted(seen) == [r for r in range(n) if vis[r]]  # invisible: nowhere


# 6. update pairs on a varchar dist key
def test_dispatch_update_pairs_varchar_key(gpu):
    base = b"k" * 40
    pairs = [
        (base + b"x", base + b"x", True),      # same bytes: stays a pair
        (base + b"x", base + b"y", False),     # last byte differs
        (base, base + b"x", False),            # shared prefix, other length
        (None, b"value", False),               # NULL -> value
        (None, None, True),                    # NULL -> NULL: stays a pair
    ]
    ops, keys = [], []
    for old, new, _ in pairs:
        ops += [OP_UD, OP_UI]
        keys += [old, new]
    c = VChunk([T_VARCHAR, T_I64], ops, [keys, list(range(len(ops)))])
    (out,) = dispatch(gpu, c, [0], 1)
    got = {row[1]: tok for tok, row in out.visible_rows()}
    for i, (_, _, stays) in enumerate(pairs):
        want = ("U-", "U+") if stays else ("-", "+")
        assert (got[2 * i], got[2 * i + 1]) == want, f"pair {i}"
    assert [row[0] for _, row in out.visible_rows()] == keys
