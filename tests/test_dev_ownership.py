"""Device memory has one owner per executor (rw_devmem.hpp): whatever an
executor, a call or an exchange context allocated is back when it is gone.

Each case records `rw_debug_dev_bytes_live`, builds an executor, drives it
through every lazily allocated buffer it has, closes it and asserts the
counter is back at the recorded value. The counter is process-local and
exact, so the assertion is equality. Outputs are not checked here; the
parity suites do that.

Shapes: chunks of 64-256 rows, table capacity 1024. Two things the code
fixes are larger than that: the staging batches start at 4096 rows, so the
DISTINCT case pushes one 4097-row chunk to make the stage regrow; and the
epoch buffer starts at 2^21 rows whatever the hints, so the epoch-ingest
case does two appends into the first buffer (no regrow, no copy).
"""
import ctypes as C

import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest import varchar_agg as va
from rwtest import xpayload as xp
from rwtest.ffi import (AGG_COUNT, AGG_COUNT_STAR, AGG_SUM, JOIN_INNER,
                        JOIN_LEFT_OUTER, OP_INSERT, SIDE_LEFT, SIDE_RIGHT,
                        T_I64, T_TS)
from rwtest.varchar import T_VARCHAR, VChunk
from test_varchar_dispatch import vnodes
from test_vnode_dispatch import bind as bind_vnode

pytestmark = pytest.mark.gpu

ALL_VNODES = [0xFF] * 32  # 256 vnodes, every one owned: nothing is dropped


@pytest.fixture(scope="module")
def gpu():
    import risingwave_amd

    return ffi.Lib(risingwave_amd.lib_path())


def i64_chunk(n, n_cols, seed, n_keys=50):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, n_keys, n)] + \
           [rng.integers(0, 1000, n) for _ in range(n_cols - 1)]
    return ffi.Chunk([T_I64] * n_cols, np.zeros(n, np.uint8), cols,
                     [np.ones(n, np.uint8)] * n_cols)


def test_hash_agg_distinct_and_vnode_scope(gpu):
    start = gpu.dev_bytes_live()
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_COUNT, 1, T_I64, 1),
             (AGG_SUM, 1, T_I64, 1)]
    g = ffi.HashAgg(gpu, [T_I64, T_I64], [0], calls, 0,
                    state_capacity_hint=1024)
    assert gpu.dev_bytes_live() > start
    # dedup tables + dirty lists on the first push; hidden buffers regrow
    # on every larger chunk, the stage (4096 rows) on the last
    for e, n in enumerate((64, 256, 4097)):
        g.push(i64_chunk(n, 2, 100 + e))
        g.flush(e + 1)
        assert g.poll_all()
    g.update_vnode_bitmap(ALL_VNODES)
    g.close()
    assert gpu.dev_bytes_live() == start


def test_hash_agg_epoch_ingest_and_varchar_keys(gpu):
    start = gpu.dev_bytes_live()
    L = gpu.lib
    L.rw_hash_agg_ingest_mode.restype = C.c_int
    L.rw_hash_agg_ingest_mode.argtypes = [C.c_void_p, C.c_int]
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 1, T_I64)]
    g = ffi.HashAgg(gpu, [T_I64, T_I64], [0], calls, 0, append_only=True,
                    state_capacity_hint=1024)
    assert L.rw_hash_agg_ingest_mode(g.h, 1) == 0, gpu.last_error()
    g.push(i64_chunk(128, 2, 200))  # allocates the epoch buffer
    g.push(i64_chunk(256, 2, 201))  # appends behind it
    g.flush(1)
    assert g.poll_all()
    g.close()
    assert gpu.dev_bytes_live() == start

    # varchar group key from the smallest reservation: 64 arena bytes and
    # 16 strings, then 256 distinct 12-byte strings -> the arena and the
    # intern table both double more than once
    types = [T_VARCHAR, T_I64]
    g = ffi.HashAgg(gpu, types, [0], calls, 0, state_capacity_hint=1024)
    assert va.varlen_reserve(gpu, g.h, 64, 16) == 0, gpu.last_error()
    caps = []
    for e in range(2):
        rows = [(b"string-%05d" % (128 * e + i), i) for i in range(128)]
        g.push(VChunk.from_rows(types, [OP_INSERT] * 128, rows))
        g.flush(e + 1)
        assert va.poll_all(g)
        ffi.agg_checkpoint_drain_bytes(gpu, g.h)
        caps.append(va.varlen_stats(gpu, g.h))
    assert caps[0][1] > 64 and caps[0][3] > 32        # grew on the first push
    assert caps[1][1] > caps[0][1] and caps[1][3] > caps[0][3]  # and again
    g.close()
    assert gpu.dev_bytes_live() == start


J_LEFT = [T_I64, T_I64, T_VARCHAR, T_VARCHAR]  # key, uniq, str, str
J_RIGHT = [T_I64, T_VARCHAR, T_I64]            # key, str, uniq
J_KW = dict(key_l=[0], key_r=[0], pk_l=[1], pk_r=[2],
            state_capacity_hint=1024, row_capacity_hint=4096)


def test_hash_join_outer_varchar_drain_compact_restore(gpu):
    start = gpu.dev_bytes_live()
    g = ffi.HashJoin(gpu, JOIN_LEFT_OUTER, J_LEFT, J_RIGHT, **J_KW)
    for s in (SIDE_LEFT, SIDE_RIGHT):
        assert vc.varlen_reserve(gpu, g.h, s, 256) == 0, gpu.last_error()
    # an outer join: the degree dirty buffers exist. 64 + 256 rows a side,
    # 20-byte strings: each arena passes 256 bytes on the first push and
    # doubles again on the second
    for e, n in enumerate((64, 256)):
        base = 1000 * e
        left = [(i % 40, base + i, b"left-%015d" % i,
                 None if i % 7 == 0 else b"also-%015d" % i) for i in range(n)]
        right = [(i % 50, b"right-%014d" % i, base + i) for i in range(n)]
        g.push(SIDE_LEFT, VChunk.from_rows(J_LEFT, [OP_INSERT] * n, left))
        g.push(SIDE_RIGHT, VChunk.from_rows(J_RIGHT, [OP_INSERT] * n, right))
        # retract a few, so compaction has dead records and strings
        g.push(SIDE_LEFT, VChunk.from_rows(J_LEFT, [ffi.OP_DELETE] * 8,
                                           left[:8]))
        g.flush(e + 1)
        assert vc.poll_all(g)
    for s in (SIDE_LEFT, SIDE_RIGHT):
        used, cap = vc.varlen_stats(gpu, g.h, s)
        assert cap > 256 and used > 256
    state = [ffi.join_checkpoint_drain(gpu, g.h, s) for s in (0, 1)]
    degs = [ffi.join_degree_drain(gpu, g.h, s) for s in (0, 1)]
    assert state[0] and state[1]
    assert ffi.join_compact(gpu, g.h, SIDE_LEFT) > 0
    ffi.join_compact(gpu, g.h, SIDE_RIGHT)
    g.update_vnode_bitmap(ALL_VNODES)
    g.close()
    assert gpu.dev_bytes_live() == start

    b = ffi.HashJoin(gpu, JOIN_LEFT_OUTER, J_LEFT, J_RIGHT, **J_KW)
    for s in (0, 1):
        ffi.join_restore(gpu, b.h, s, state[s], degs[s])
    assert vc.varlen_stats(gpu, b.h, SIDE_LEFT)[0] > 0
    b.close()
    assert gpu.dev_bytes_live() == start


def topn_chunk(n, seed, first_id):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, 30, n), rng.integers(0, 1000, n),
            np.arange(n) + first_id]  # (group, order key, unique id)
    return ffi.Chunk([T_I64] * 3, np.zeros(n, np.uint8), cols,
                     [np.ones(n, np.uint8)] * 3)


def test_group_top_n_regrow_compact_drain(gpu):
    start = gpu.dev_bytes_live()
    t = ffi.GroupTopN(gpu, [T_I64] * 3, [0], [(1, False)], [(2, False)],
                      limit=2, state_capacity_hint=1024,
                      row_capacity_hint=4096)
    for e, n in enumerate((64, 256)):  # the second chunk regrows every cap
        t.push(topn_chunk(n, 400 + e, 1000 * e))
        t.flush(e + 1)
        assert t.poll_all()
    assert ffi.topn_checkpoint_drain(gpu, t.h)
    ffi.topn_compact(gpu, t.h)
    t.push(topn_chunk(64, 402, 5000))  # its output stays queued, unpolled
    t.flush(3)
    t.close()
    assert gpu.dev_bytes_live() == start


def test_vnode_compute_and_exchange_partition(gpu):
    bind_vnode(gpu)
    start = gpu.dev_bytes_live()
    assert len(vnodes(gpu, i64_chunk(200, 2, 500), [0, 1])) == 200
    assert gpu.dev_bytes_live() == start
    names = [None if i % 9 == 0 else b"name-%d" % i * (1 + i % 4)
             for i in range(200)]
    c = VChunk([T_I64, T_VARCHAR], [0] * 200, [list(range(200)), names])
    assert len(vnodes(gpu, c, [1, 0])) == 200
    assert gpu.dev_bytes_live() == start

    # the exchange library keeps its own counter
    xl = xp.XLib(handle=False)
    xl.L.rw_exchange_debug_dev_bytes_live.restype = C.c_uint64
    xstart = xl.L.rw_exchange_debug_dev_bytes_live()
    sz = xl.L.rw_exchange_unique_id_size()
    uid = (C.c_uint8 * sz)()
    assert xl.L.rw_exchange_get_unique_id(uid) == 0, xl.err()
    xl.adopt(xl.L.rw_exchange_create(1, 0, uid), 1)
    ts = [10**15 + i for i in range(200)]
    batch = xp.Batch(xl, [T_I64, T_VARCHAR, T_TS],
                     [list(range(200)), names, ts], np.zeros(200, np.uint8))
    for _ in (0, 1):  # second call: scratch is reused, not regrown
        got = xp.partition(xl, batch, [0, 1], 3)
        assert got.rc == 0, got.err
        assert sum(got.rows) == 200
    assert xl.L.rw_exchange_debug_dev_bytes_live() > xstart
    batch.free()
    xl.close()
    assert xl.L.rw_exchange_debug_dev_bytes_live() == xstart


def test_create_refused_after_first_allocation(gpu):
    # Every descriptor check of the three init()s (varchar join key or
    # condition included) comes before the first allocation; what can fail
    # later is an allocation. A 2^40-row record store (64 TiB) is refused
    # by hipMalloc after side 0's slot table was allocated.
    start = gpu.dev_bytes_live()
    kw = dict(J_KW, row_capacity_hint=1 << 40)
    with pytest.raises(RuntimeError) as ei:
        ffi.HashJoin(gpu, JOIN_INNER, J_LEFT, J_RIGHT, **kw)
    assert "HIP error" in str(ei.value)
    # the runtime keeps the refused call's error for hipGetLastError, which
    # later launches in this thread would report as theirs: take it
    with open("/proc/self/maps") as f:
        hip = next(ln.split()[-1] for ln in f if "libamdhip64.so" in ln)
    C.CDLL(hip).hipGetLastError()
    assert gpu.dev_bytes_live() == start
