"""Varchar group keys through the GPU HashAgg (rw_stream.h "varchar GROUP
KEYS in HashAgg"): interning pre-pass, emit, checkpoint
spill, restore, watermark clean, growth, rejections.

Reference: the unchanged CPU oracle on surrogate ids, its outputs mapped
back to strings and its drains re-encoded (rwtest/varchar_agg.py). Compared
per flush as the sorted multiset of (op, row), exact. The seeded stream is
the one tests/test_varchar_agg_workload.py pins.
"""
import ctypes as C

import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest import varchar_agg as va
from rwtest.ffi import OP_DELETE, OP_INSERT, T_I64
from rwtest.varchar import T_VARCHAR, VChunk

pytestmark = pytest.mark.gpu

WN = [va.COL_WINDOW, va.COL_NAME]


def gpu():
    import risingwave_amd

    return ffi.Lib(risingwave_amd.lib_path())


@pytest.fixture(scope="module")
def wl():
    """The pinned workload and its (window, name) oracle reference, once."""
    epochs = va.make_workload()
    ref, sur = va.oracle_run(epochs, WN)
    return epochs, ref, sur


def check_key_columns(out_chunks, types, group_key):
    for ch in out_chunks:
        assert ch.types[:len(group_key)] == [types[k] for k in group_key]


# 1. parity on the pinned workload, every key shape
@pytest.mark.parametrize("group_key,chunk_size", [
    ([va.COL_NAME], 1024),
    (WN, 100),
    ([va.COL_NAME, va.COL_WINDOW], 1024),
    ([va.COL_NAME, va.COL_NAME2], 1024),
], ids=["name", "window_name", "name_window", "name_name2"])
def test_parity_key_shapes(wl, group_key, chunk_size):
    epochs = wl[0]
    ref, _ = va.oracle_run(epochs, group_key)
    lib = gpu()
    got, agg = va.gpu_run(lib, epochs, group_key, chunk_size=chunk_size)
    agg.close()
    for e in range(len(epochs)):
        assert got.outs[e] == ref.outs[e], f"flush {e}"
    assert sum(len(o) for o in got.outs) > 500
    check_key_columns(got.out_chunks, va.TYPES, group_key)
    assert T_VARCHAR in got.out_chunks[0].types
    if chunk_size == 100:
        assert len(got.out_chunks) > 6  # sliced: offsets rebased per chunk
    assert got.drains == ref.drains


def test_parity_append_only_min_max():
    epochs = va.make_workload(p_del=0.0)
    ref, _ = va.oracle_run(epochs, WN, calls=va.CALLS_APPEND, append_only=True)
    got, agg = va.gpu_run(gpu(), epochs, WN, calls=va.CALLS_APPEND,
                          append_only=True)
    agg.close()
    assert got.outs == ref.outs
    assert any(op == "U+" for o in got.outs for op, _ in o)
    check_key_columns(got.out_chunks, va.TYPES, WN)


# 2. one launch, many lanes, the same never-seen string
RACE_TYPES = [T_VARCHAR, T_I64]
RACE_CALLS = [(ffi.AGG_COUNT_STAR, -1, T_I64), (ffi.AGG_SUM, 1, T_I64)]


def test_in_batch_race():
    n = 4096
    rng = np.random.default_rng(5)
    one = b"never-seen-before-string"
    three = [b"alpha", b"alpha-but-longer-than-eight", b""]
    a = [(one, int(v)) for v in rng.integers(0, 100, n)]
    b = [(three[int(i)], int(v)) for i, v in zip(rng.integers(0, 3, n),
                                                 rng.integers(0, 100, n))]
    c = [(b"d%05d" % i + b"x" * (i % 23), i) for i in range(n)]
    chunks = [VChunk.from_rows(RACE_TYPES, [OP_INSERT] * n, rows)
              for rows in (a, b, c)]
    # each chunk twice: the second push must find every string
    epochs = [[ch] for ch in chunks for _ in (0, 1)]
    ref, _ = va.oracle_run(epochs, [0], calls=RACE_CALLS, types=RACE_TYPES)
    header, align = va.header_consts()
    lib = gpu()
    agg = ffi.HashAgg(lib, RACE_TYPES, [0], RACE_CALLS, row_count_index=0)
    run = va.Run()
    seen = set()
    for e, chunks_e in enumerate(epochs):
        before = va.varlen_stats(lib, agg.h)
        va.gpu_epoch(lib, agg, chunks_e, e + 1, run)
        seen |= {r[0] for r in chunks_e[0].rows() if r[0] is not None}
        used, cap, n_str, tcap = va.varlen_stats(lib, agg.h)
        assert n_str == len(seen), (e, n_str, len(seen))
        assert used <= (sum(len(s) for s in seen) + header +
                        n_str * (align - 1)), (e, used)
        assert used >= sum(len(s) for s in seen) and used <= cap
        assert n_str * 10 <= tcap * 7  # the host keeps the load <= 0.7
        if e % 2 == 1:  # the same chunk again: nothing new
            assert (used, n_str) == (before[0], before[2]), e
        assert run.outs[e] == ref.outs[e], f"flush {e}"
    agg.close()
    assert run.drains == ref.drains


# 3. arena and table growth from a tiny reservation
def test_growth_from_small_reserve():
    rng = np.random.default_rng(11)
    strings = sorted({bytes(rng.integers(33, 127, int(rng.integers(1, 41)),
                                         dtype=np.uint8))
                      for _ in range(2600)})[:2000]
    assert len(strings) == 2000
    per = 400
    epochs = []
    for e in range(5):
        fresh = strings[e * per:(e + 1) * per]
        old = strings[:e * per]
        rows = [(s, 1) for s in fresh]
        rows += [(old[int(i)], 2) for i in rng.integers(0, max(len(old), 1),
                                                       150 if old else 0)]
        rows += [(fresh[int(i)], 3) for i in rng.integers(0, per, 100)]
        order = rng.permutation(len(rows))
        rows = [rows[int(i)] for i in order]
        half = len(rows) // 2
        epochs.append([VChunk.from_rows(RACE_TYPES, [OP_INSERT] * len(part),
                                        part)
                       for part in (rows[:half], rows[half:])])
    # retract every row of the first epoch: the groups only it fed reach 0
    first = [r for ch in epochs[0] for r in ch.rows()]
    epochs.append([VChunk.from_rows(RACE_TYPES, [OP_DELETE] * len(first),
                                    first)])
    ref, _ = va.oracle_run(epochs, [0], calls=RACE_CALLS, types=RACE_TYPES)
    assert sum(op == "-" for op, _ in ref.outs[-1]) >= 100
    lib = gpu()
    agg = ffi.HashAgg(lib, RACE_TYPES, [0], RACE_CALLS, row_count_index=0)
    assert va.varlen_reserve(lib, agg.h, 64, 16) == 0, lib.last_error()
    run = va.Run()
    caps = []
    for e, chunks_e in enumerate(epochs):
        va.gpu_epoch(lib, agg, chunks_e, e + 1, run)
        assert run.outs[e] == ref.outs[e], f"flush {e}"
        used, cap, n_str, tcap = va.varlen_stats(lib, agg.h)
        caps.append((cap, tcap))
        assert n_str == min((e + 1) * per, 2000)
        assert used <= cap and n_str * 10 <= tcap * 7
    # the reservation was honoured, then both grew, more than once
    assert va.varlen_reserve(lib, agg.h, 64, 16) == va.RW_E_INVAL
    agg.close()
    assert caps[0][0] < caps[-1][0] and caps[0][1] < caps[-1][1]
    assert len({c for c, _ in caps}) >= 2 and len({t for _, t in caps}) >= 3
    assert caps[-1][0] < 64 * 4096 and caps[-1][1] <= 8192
    assert run.drains == ref.drains


# 4. spill bytes against the re-encoded oracle drain (independent encoder)
def test_spill_bytes(wl):
    epochs, ref, _ = wl
    got, agg = va.gpu_run(gpu(), epochs, WN)
    agg.close()
    for e in range(len(epochs)):
        assert got.drains[e] == ref.drains[e], f"drain {e}"
    frames = [f for d in got.drains for f in vc.decode_frames(d)]
    assert sum(1 for put, _, _ in frames if not put) >= 20  # DELETE frames
    ot = va.out_types_of(va.TYPES, WN, va.CALLS)
    names = {vc.decode_row(v, ot)[1] for put, _, v in frames if put}
    assert {None, b"", vc.LONG, vc.UTF8} <= names


# 5. restore into a fresh executor
def test_restore(wl):
    epochs, ref, _ = wl
    lib = gpu()
    a = ffi.HashAgg(lib, va.TYPES, WN, va.CALLS, row_count_index=0)
    run = va.Run()
    for e in (0, 1):
        va.gpu_epoch(lib, a, epochs[e], e + 1, run)
    a.close()
    b = ffi.HashAgg(lib, va.TYPES, WN, va.CALLS, row_count_index=0)
    ffi.agg_restore(lib, b.h, run.drains[0] + run.drains[1])
    # live groups after two epochs, from the reference outputs
    live = set()
    for out in ref.outs[:2]:
        for op, row in out:
            if op in ("+", "U+"):
                live.add(row[:2])
            elif op == "-":
                live.discard(row[:2])
    want = {k[1] for k in live if k[1] is not None}
    assert va.varlen_stats(lib, b.h)[2] == len(want)
    va.gpu_epoch(lib, b, epochs[2], 3, run)
    b.close()
    assert run.outs[2] == ref.outs[2]
    assert run.drains[2] == ref.drains[2]


# 6. watermark on the fixed-width key next to a varchar key
def test_watermark(wl):
    epochs = va.make_workload(stop_below=(1, 20))
    wms = {0: (0, 20)}
    ref, _ = va.oracle_run(epochs, WN, watermarks=wms)
    lib = gpu()
    got, agg = va.gpu_run(lib, epochs, WN, watermarks=wms)
    for e in range(len(epochs)):
        assert got.outs[e] == ref.outs[e], f"flush {e}"
        assert got.drains[e] == ref.drains[e], f"drain {e}"
    # the clean's DELETE frames carry string keys of windows below 20
    dels = [k for put, k, _ in vc.decode_frames(got.drains[0]) if not put]
    cleaned = [k for k in dels if k[:9] < va.memcmp_i64(20)]
    assert len(cleaned) >= 20
    assert any(len(k) > 9 + 11 for k in cleaned)  # a multi-group string key
    # rows at or below the watermark arrived later and restarted groups
    assert any(op == "+" and row[0] < 20 for op, row in got.outs[1])
    rc = lib.lib.rw_hash_agg_watermark(agg.h, 1, 5)
    assert rc == va.RW_E_INVAL and "varchar" in lib.last_error()
    agg.close()


# 7a. the scope list: rejected loudly
def test_rejections():
    lib = gpu()
    L = lib.lib

    def create_fails(**kw):
        args = dict(input_types=va.TYPES, group_key=WN, calls=va.CALLS,
                    row_count_index=0)
        args.update(kw)
        with pytest.raises(RuntimeError) as ei:
            ffi.HashAgg(lib, **args)
        assert "varchar" in str(ei.value) or "unsupported" in str(ei.value)

    create_fails(calls=va.CALLS_APPEND)  # materialized-input min/max
    create_fails(calls=[va.CALLS[0], (ffi.AGG_COUNT, va.COL_W, T_I64, 1)])
    create_fails(emit_on_window_close=True)
    create_fails(calls=[va.CALLS[0], (ffi.AGG_COUNT, va.COL_NAME2, T_I64)])
    create_fails(calls=va.CALLS_APPEND, stream_key=[va.COL_NAME2])

    agg = ffi.HashAgg(lib, va.TYPES, WN, va.CALLS, row_count_index=0)
    join = ffi.HashJoin(lib, ffi.JOIN_INNER, [T_I64, T_I64], [T_I64, T_I64],
                        key_l=[0], key_r=[0], pk_l=[1], pk_r=[1])
    h, jh, vp = agg.h, join.h, C.c_void_p
    null = vp(None)

    def inval(name, argtypes, *args):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = argtypes
        assert fn(*args) == va.RW_E_INVAL, name
        assert "varchar" in lib.last_error(), (name, lib.last_error())

    inval("rw_hash_agg_ingest_mode", [vp, C.c_int], h, 1)
    bitmap = (C.c_uint8 * 32)(*([0xFF] * 32))
    inval("rw_hash_agg_update_vnode_bitmap", [vp, vp, C.c_uint32], h,
          C.cast(bitmap, vp), 256)
    inval("rw_agg_bench_apply", [vp, vp], h, null)
    inval("rw_agg_bench_run", [vp, vp] + [C.c_int] * 4, h, null, 1, 1, 0, 0)
    inval("rw_agg_bench_run_epochs",
          [vp, vp, C.c_uint64] + [C.c_int] * 4, h, null, 1, 1, 1, 1, 0)
    inval("rw_agg_apply_payload", [vp, vp, vp] + [C.c_int] * 3, h, null, null,
          0, 5, 0)
    inval("rw_agg_apply_joinout", [vp, vp], h, jh)
    inval("rw_agg_flush_launch", [vp, C.c_uint64], h, 1)
    inval("rw_agg_apply_flush_launch",
          [vp, vp, C.c_uint32, C.c_uint32, C.c_uint64], h, null, 0, 0, 1)
    inval("rw_q7pipe_bench_run",
          [vp, vp, vp, vp] + [C.c_int] * 3 + [vp, C.c_int, C.c_int], h, jh,
          null, null, 1, 1, 0, null, 0, 0)
    good = va.make_workload()[0][0]
    cc = good.to_c()
    L.rw_agg_bench_preload.restype = vp
    L.rw_agg_bench_preload.argtypes = [vp, C.POINTER(ffi.RwChunkC)]
    assert not L.rw_agg_bench_preload(h, C.byref(cc))
    assert "varchar" in lib.last_error()
    # none of it disturbed the executor
    agg.push(good)
    agg.flush(1)
    ref, _ = va.oracle_run([[good]], WN)
    assert vc.rows_of(va.poll_all(agg)) == ref.outs[0]
    join.close()
    agg.close()


# 7b. malformed chunks are refused before any state changes
@pytest.mark.parametrize("how", ["decreasing", "offs0", "null_bytes",
                                 "too_long"])
def test_malformed_chunk_refused(how):
    epochs = va.make_workload()
    first, second = epochs[0][0], epochs[0][1]
    ref, _ = va.oracle_run([[first, second]], WN)
    lib = gpu()
    agg = ffi.HashAgg(lib, va.TYPES, WN, va.CALLS, row_count_index=0)
    agg.push(first)
    before = va.varlen_stats(lib, agg.h)
    bad = VChunk(second.types, second.ops, second.cols)
    cc = bad.to_c()
    vd = C.cast(cc.cols[va.COL_NAME].data,
                C.POINTER(vc.RwVarlenData)).contents
    n = bad.n_rows
    if how == "decreasing":
        r = next(i for i in range(1, n) if vd.offsets[i + 1] > vd.offsets[i])
        vd.offsets[r] = vd.offsets[r + 1] + 1
    elif how == "offs0":
        vd.offsets[0] = 1
    elif how == "null_bytes":
        vd.bytes = C.POINTER(C.c_uint8)()
    else:
        for i in range(1, n + 1):  # one string of 2^24 bytes: over the limit
            vd.offsets[i] = 1 << 24
    rc = lib.lib.rw_hash_agg_push_chunk(agg.h, C.byref(cc))
    assert rc == va.RW_E_INVAL, (rc, lib.last_error())
    assert "varchar column" in lib.last_error()
    assert va.varlen_stats(lib, agg.h) == before
    agg.push(second)
    agg.flush(1)
    assert vc.rows_of(va.poll_all(agg)) == ref.outs[0]
    agg.close()


# 8. executors without varchar keys are untouched
def test_i64_executor_has_no_arena():
    lib = gpu()
    v = ffi.HashAgg(lib, va.TYPES, WN, va.CALLS, row_count_index=0)
    i = ffi.HashAgg(lib, [T_I64, T_I64], [0], RACE_CALLS, row_count_index=0)
    assert va.varlen_stats(lib, v.h) == (0, 0, 0, 0)  # nothing pushed yet
    n = 300
    ch = ffi.Chunk([T_I64, T_I64], [OP_INSERT] * n,
                   [np.arange(n) % 7, np.arange(n)],
                   [np.ones(n, np.uint8)] * 2)
    i.push(ch)
    v.push(va.make_workload()[0][0])
    i.flush(1)
    v.flush(1)
    assert va.varlen_stats(lib, i.h) == (0, 0, 0, 0)
    assert va.varlen_reserve(lib, i.h, 1 << 20, 100) == va.RW_E_INVAL
    assert va.varlen_stats(lib, v.h)[2] > 0
    assert len(ffi.rows_multiset(i.poll_all())) == 7
    i.close()
    v.close()
