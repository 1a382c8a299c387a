"""The checkpoint flush carried by the dense span apply launch
(rw_agg_apply_flush_launch) against the oracle and against
the two-launch path.

Every scenario runs two epochs through the entry, each followed by
rw_agg_sync and a counter scan, and a third epoch through the
host-synchronous rw_hash_agg_flush. The third epoch's rows equal the
oracle's only if the fused tail inferred the first two epochs' changes and
wrote `prev` exactly as agg_flush_fast_kernel does. Mode 1 forces fusion
wherever the launch is eligible, mode 2 forbids it; the launch counter says
which path a scenario really took. Nothing here depends on timing.
"""
import ctypes
import functools

import numpy as np
import pytest

from rwtest import ffi
from rwtest.ffi import (
    AGG_COUNT_STAR, AGG_MAX, AGG_SUM, OP_INSERT, OP_UPDATE_DELETE,
    OP_UPDATE_INSERT, T_I64, oracle,
)

pytestmark = pytest.mark.gpu

COUNT = (AGG_COUNT_STAR, -1, T_I64)
# (calls, row_count_index): the three count-star span instantiations, the
# single-call one with both orders of the two-call shape around it
SHAPES = {
    "max_count": ([(AGG_MAX, 1, T_I64), COUNT], 1),
    "sum_count": ([(AGG_SUM, 1, T_I64), COUNT], 1),
    "count_max": ([COUNT, (AGG_MAX, 1, T_I64)], 0),
    "count": ([COUNT], 0),
}
FUSED, UNFUSED = 1, 2


class AggDebug(ctypes.Structure):
    _fields_ = [("ready_slots", ctypes.c_uint64), ("dup_keys", ctypes.c_uint64),
                ("dirty_count", ctypes.c_uint64), ("out_cursor", ctypes.c_uint64)]


@functools.lru_cache(maxsize=None)
def gpu():
    import risingwave_amd

    glib = ffi.Lib(risingwave_amd.lib_path())
    L = glib.lib
    vp, u32, u64, ci = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64,
                        ctypes.c_int)
    L.rw_agg_bench_preload.restype = vp
    L.rw_agg_bench_preload.argtypes = [vp, ctypes.POINTER(ffi.RwChunkC)]
    L.rw_agg_bench_apply.restype = ci
    L.rw_agg_bench_apply.argtypes = [vp, vp]
    L.rw_agg_apply_flush_launch.restype = ci
    L.rw_agg_apply_flush_launch.argtypes = [vp, vp, u32, u32, u64]
    L.rw_agg_flush_launch.restype = ci
    L.rw_agg_flush_launch.argtypes = [vp, u64]
    L.rw_agg_sync.restype = ci
    L.rw_agg_sync.argtypes = [vp]
    L.rw_agg_debug_scan.restype = ci
    L.rw_agg_debug_scan.argtypes = [vp, ctypes.POINTER(AggDebug)]
    L.rw_agg_debug_set_span_tiles.restype = ci
    L.rw_agg_debug_set_span_tiles.argtypes = [vp, u32]
    L.rw_agg_debug_set_fuse.restype = ci
    L.rw_agg_debug_set_fuse.argtypes = [vp, ci]
    L.rw_agg_debug_fuse_allowed.restype = ci
    L.rw_agg_debug_fuse_allowed.argtypes = [vp]
    L.rw_agg_debug_fused_launches.restype = ctypes.c_longlong
    L.rw_agg_debug_fused_launches.argtypes = [vp]
    L.rw_agg_debug_fuse_max.restype = u32
    L.rw_agg_debug_fuse_max.argtypes = []
    return glib


def fuse_max():
    return int(gpu().lib.rw_agg_debug_fuse_max())


def chunk(keys, vals, extra=()):
    n = len(keys)
    cols = [keys, vals, *extra]
    return ffi.Chunk([T_I64] * len(cols), np.full(n, OP_INSERT, np.uint8), cols,
                     [np.ones(n, np.uint8)] * len(cols))


def sorted_batch(rng, n_rows, n_groups, first_key):
    """Sorted keys as in q7: exactly `n_groups` distinct ones from `first_key`
    on, so the epoch's dirty count is `n_groups`."""
    assert n_rows >= n_groups
    k = np.concatenate([np.arange(n_groups),
                        rng.integers(0, n_groups, n_rows - n_groups)])
    keys = (np.sort(k) + first_key) * 10_000_000
    return keys.astype(np.int64), rng.integers(1, 10**7, n_rows)


def rows_array(chunks):
    mats = []
    for c in chunks:
        cols = [c.ops.astype(np.int64)]
        for d, v in zip(c.cols, c.valids):
            cols.append(np.where(v != 0, d, 0).astype(np.int64))
            cols.append((v != 0).astype(np.int64))
        m = np.stack(cols, axis=1)
        if c.vis is not None:
            m = m[c.vis != 0]
        mats.append(m)
    if not mats:
        return np.zeros((0, 1), np.int64)
    return np.concatenate(mats, axis=0)


def as_multiset(rows):
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def assert_same_multiset(got, want, what):
    assert got.shape == want.shape, (
        f"{what}: {got.shape[0]} rows vs {want.shape[0]}")
    g, w = as_multiset(got), as_multiset(want)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert not len(bad), (
        f"{what}: {len(bad)} rows differ, first {g[bad[0]]} vs {w[bad[0]]}")


def assert_pairs_adjacent(rows, what):
    ops, keys = rows[:, 0], rows[:, 1]
    um = np.nonzero(ops == OP_UPDATE_DELETE)[0]
    up = np.nonzero(ops == OP_UPDATE_INSERT)[0]
    assert len(um) == len(up), f"{what}: {len(um)} U- vs {len(up)} U+"
    assert not len(um) or um[-1] + 1 < len(rows), f"{what}: trailing U-"
    assert (um + 1 == up).all(), f"{what}: a U- is not followed by a U+"
    assert (keys[um] == keys[up]).all(), f"{what}: U-/U+ keys differ"


def oracle_third_epoch(make, epochs):
    """epochs: three lists of chunks. Returns the oracle's third-epoch rows."""
    o = make(oracle())
    try:
        for e, chunks in enumerate(epochs):
            for c in chunks:
                o.push(c)
            o.flush(e + 1)
            want = rows_array(o.poll_all())
        return want
    finally:
        o.close()


def gpu_third_epoch(make, batches, ranges, mode, span_tiles=0, repeat=1,
                    empty_flush=False, expect_fused=None, what=""):
    """Rows ranges[e] of batches[e], e = 0 and 1, go through the entry
    `repeat` times, every call an epoch of its own (a repeated batch leaves
    the max as it was and changes only the count); then batches[2] is applied
    whole and flushed synchronously. Returns that last epoch's rows."""
    glib = gpu()
    L = glib.lib
    g = make(glib)
    try:
        assert L.rw_agg_debug_set_fuse(g.h, mode) == 0
        assert L.rw_agg_debug_set_span_tiles(g.h, span_tiles) == 0
        handles = []
        for b in batches:
            cc = b.to_c()
            h = L.rw_agg_bench_preload(g.h, ctypes.byref(cc))
            assert h, glib.last_error()
            handles.append(h)

        def synced_and_idle(tag):
            assert L.rw_agg_sync(g.h) == 0, glib.last_error()
            d = AggDebug()
            assert L.rw_agg_debug_scan(g.h, ctypes.byref(d)) == 0
            assert d.dirty_count == 0 and d.out_cursor == 0, (
                f"{what} {tag}: dirty_count {d.dirty_count}, out_cursor "
                f"{d.out_cursor}")
            assert d.dup_keys == 0

        launches = 0
        for e in range(2):
            r0, r1 = ranges[e]
            for _ in range(repeat):
                assert L.rw_agg_apply_flush_launch(g.h, handles[e], r0, r1,
                                                   e + 1) == 0, glib.last_error()
                launches += 1
                synced_and_idle(f"after epoch {e + 1}")
            if empty_flush:
                assert L.rw_agg_flush_launch(g.h, 100 + e) == 0
                synced_and_idle(f"after the empty flush behind epoch {e + 1}")
        if expect_fused is not None:
            n = L.rw_agg_debug_fused_launches(g.h)
            assert n == (launches if expect_fused else 0), (
                f"{what}: {n} of {launches} launches carried the flush")
        assert L.rw_agg_bench_apply(g.h, handles[2]) == 0, glib.last_error()
        g.flush(3)
        return rows_array(g.poll_all())
    finally:
        g.close()


def check(shape, batches, ranges=None, span_tiles=0, repeat=1,
          empty_flush=False, eligible=True, make=None, what=""):
    """Fused and unfused runs of one scenario against the oracle and each
    other. `batches`: three (keys, vals[, extra cols]) tuples."""
    calls, rci = SHAPES[shape] if isinstance(shape, str) else shape
    n_cols = len(batches[0])
    if make is None:
        def make(lib):
            return ffi.HashAgg(lib, [T_I64] * n_cols, [0], calls, rci,
                               append_only=True, state_capacity_hint=8192)
    chunks = [chunk(b[0], b[1], b[2:]) for b in batches]
    if ranges is None:
        ranges = [(0, len(b[0])) for b in batches[:2]]
    epochs = []
    for e in range(2):
        r0, r1 = ranges[e]
        part = chunk(*[c[r0:r1] for c in batches[e][:2]],
                     [c[r0:r1] for c in batches[e][2:]])
        epochs.append([part] * repeat)
    epochs.append([chunks[2]])
    want = oracle_third_epoch(make, epochs)
    got = {}
    for mode in (FUSED, UNFUSED):
        got[mode] = gpu_third_epoch(
            make, chunks, ranges, mode, span_tiles, repeat, empty_flush,
            expect_fused=eligible and mode == FUSED, what=f"{what} mode {mode}")
        assert_same_multiset(got[mode], want, f"{what} mode {mode} vs oracle")
        assert_pairs_adjacent(got[mode], f"{what} mode {mode}")
    assert_same_multiset(got[FUSED], got[UNFUSED], f"{what} fused vs unfused")
    assert len(want), f"{what}: the third epoch emits nothing, nothing checked"
    return want


def overlapping(rng, n_rows, n_groups, rows3=None):
    """Three epochs whose key ranges overlap by half: each updates old groups
    and opens new ones."""
    return [sorted_batch(rng, rows3 if e == 2 and rows3 else n_rows, n_groups,
                         e * (n_groups // 2 + 1)) for e in range(3)]


# one block (1024 rows at one tile per wave); with 4 tiles per wave: waves
# with no tile, a ragged last tile, a run carried across tiles
@pytest.mark.parametrize("n_rows,span_tiles",
                         [(1024, 1), (1024, 4), (4096 + 3, 1), (4096 + 3, 4)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_epochs_match_oracle(shape, n_rows, span_tiles):
    rng = np.random.default_rng(n_rows * 8 + span_tiles)
    want = check(shape, overlapping(rng, n_rows, 40), span_tiles=span_tiles,
                 what=f"{shape} n={n_rows} span_tiles={span_tiles}")
    ops = set(want[:, 0].tolist())
    assert OP_UPDATE_DELETE in ops and OP_INSERT in ops


# 64 blocks: the last arriver is some block other than 0, and the blocks
# are spread over every XCD
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_many_blocks(shape):
    rng = np.random.default_rng(65536)
    check(shape, overlapping(rng, 65536, 700, rows3=4096), span_tiles=1,
          what=f"{shape} 64 blocks")


# around the wave (64) and block (256) sizes, several passes of the flusher,
# and past the policy's limit, where the tail is slow but still right
@pytest.mark.parametrize("n_groups",
                         [1, 63, 64, 65, 255, 256, 257, 700, "fuse_max+37"])
def test_fused_dirty_counts(n_groups):
    if n_groups == "fuse_max+37":
        n_groups = fuse_max() + 37
    rng = np.random.default_rng(n_groups)
    n_rows = max(1024, 2 * n_groups)
    check("max_count", overlapping(rng, n_rows, n_groups),
          what=f"{n_groups} dirty groups")


def test_fused_sub_range_and_unaligned_fallback():
    rng = np.random.default_rng(8192)
    batches = overlapping(rng, 8192, 300, rows3=2048)
    check("max_count", batches, ranges=[(2048, 8192)] * 2, what="r0=2048")
    # one row further the span path's 32-byte alignment test fails: the
    # entry issues the two launches
    check("max_count", batches, ranges=[(2049, 8192)] * 2, eligible=False,
          what="r0=2049")
    # below the dense path's 1024-row minimum
    check("max_count", batches, ranges=[(0, 1000)] * 2, eligible=False,
          what="1000 rows")


def test_fused_same_batch_twice_changes_only_the_count():
    rng = np.random.default_rng(2)
    first = sorted_batch(rng, 2048, 100, 0)
    third = sorted_batch(rng, 1024, 100, 50)
    check("max_count", [first, first, third], repeat=2, what="same batch twice")


def test_fused_launch_after_an_empty_flush():
    rng = np.random.default_rng(3)
    check("sum_count", overlapping(rng, 2048, 70), empty_flush=True,
          what="empty flush between epochs")


def test_generic_dense_shape_falls_back():
    # three calls take the generic dense kernel, which has no tail
    rng = np.random.default_rng(4)
    batches = overlapping(rng, 2048, 90)
    shape = ([(AGG_SUM, 1, T_I64), COUNT, (AGG_MAX, 1, T_I64)], 1)
    check(shape, batches, eligible=False, what="[sum, count, max]")


def test_materialized_input_falls_back():
    # a retractable max keeps materialized input: generic flush kernel
    rng = np.random.default_rng(5)
    batches = []
    for e, (k, v) in enumerate(overlapping(rng, 1200, 30)):
        batches.append((k, v, np.arange(len(k), dtype=np.int64) + e * 10_000))

    def make(lib):
        return ffi.HashAgg(lib, [T_I64] * 3, [0], SHAPES["max_count"][0], 1,
                           stream_key=[2], append_only=False,
                           state_capacity_hint=8192)

    check("max_count", batches, eligible=False, make=make,
          what="materialized-input max")


def test_policy_turns_fusion_off_after_a_large_flush(monkeypatch):
    monkeypatch.setenv("RW_AGG_FUSE_FLUSH", "1")  # read at executor creation
    glib = gpu()
    L = glib.lib
    calls, rci = SHAPES["max_count"]
    rng = np.random.default_rng(6)
    big = sorted_batch(rng, 4096, fuse_max() + 37, 0)
    small = overlapping(rng, 2048, 50)

    def make(lib):
        return ffi.HashAgg(lib, [T_I64, T_I64], [0], calls, rci,
                           append_only=True, chunk_size=4096,
                           state_capacity_hint=8192)

    g, o = make(glib), make(oracle())
    try:
        assert L.rw_agg_debug_fuse_allowed(g.h) == 0  # no sync seen yet
        assert L.rw_agg_sync(g.h) == 0
        assert L.rw_agg_debug_fuse_allowed(g.h) == 1
        for x in (g, o):
            x.push(chunk(*big))
            x.flush(1)
            x.poll_all()
        assert L.rw_agg_sync(g.h) == 0
        assert L.rw_agg_debug_fuse_allowed(g.h) == 0
        for e, b in enumerate(small):
            c = chunk(*b)
            cc = c.to_c()
            h = L.rw_agg_bench_preload(g.h, ctypes.byref(cc))
            assert h, glib.last_error()
            o.push(c)
            o.flush(e + 2)
            want = rows_array(o.poll_all())
            if e < 2:
                assert L.rw_agg_apply_flush_launch(g.h, h, 0, len(b[0]),
                                                   e + 2) == 0
                assert L.rw_agg_sync(g.h) == 0, glib.last_error()
            else:
                assert L.rw_agg_bench_apply(g.h, h) == 0
                g.flush(e + 2)
                got = rows_array(g.poll_all())
        assert L.rw_agg_debug_fused_launches(g.h) == 0
        assert_same_multiset(got, want, "epochs after a large flush")
        assert_pairs_adjacent(got, "epochs after a large flush")
    finally:
        g.close()
        o.close()


def test_policy_fuses_small_epochs_after_a_sync(monkeypatch):
    monkeypatch.setenv("RW_AGG_FUSE_FLUSH", "1")
    glib = gpu()
    L = glib.lib
    rng = np.random.default_rng(7)
    calls, rci = SHAPES["max_count"]
    g = ffi.HashAgg(glib, [T_I64, T_I64], [0], calls, rci, append_only=True,
                    state_capacity_hint=8192)
    try:
        assert L.rw_agg_sync(g.h) == 0
        for e, b in enumerate(overlapping(rng, 2048, 50)):
            c = chunk(*b)  # owns the arrays the C view points into
            cc = c.to_c()
            h = L.rw_agg_bench_preload(g.h, ctypes.byref(cc))
            assert h, glib.last_error()
            assert L.rw_agg_apply_flush_launch(g.h, h, 0, 2048, e + 1) == 0
            assert L.rw_agg_sync(g.h) == 0, glib.last_error()
        assert L.rw_agg_debug_fused_launches(g.h) == 3
        assert L.rw_agg_debug_fuse_allowed(g.h) == 1
    finally:
        g.close()


def test_fusion_is_off_without_the_switch(monkeypatch):
    # measured slower than two launches at every dirty count
    monkeypatch.delenv("RW_AGG_FUSE_FLUSH", raising=False)
    glib = gpu()
    L = glib.lib
    rng = np.random.default_rng(8)
    calls, rci = SHAPES["max_count"]
    g = ffi.HashAgg(glib, [T_I64, T_I64], [0], calls, rci, append_only=True,
                    state_capacity_hint=8192)
    try:
        assert L.rw_agg_sync(g.h) == 0
        assert L.rw_agg_debug_fuse_allowed(g.h) == 0
        c = chunk(*sorted_batch(rng, 2048, 50, 0))
        cc = c.to_c()
        h = L.rw_agg_bench_preload(g.h, ctypes.byref(cc))
        assert h, glib.last_error()
        assert L.rw_agg_apply_flush_launch(g.h, h, 0, 2048, 1) == 0
        assert L.rw_agg_sync(g.h) == 0, glib.last_error()
        assert L.rw_agg_debug_fused_launches(g.h) == 0
    finally:
        g.close()
