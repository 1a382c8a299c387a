"""Varchar payload columns through the GPU hash join (rw_stream.h "varchar
payload columns"): build, probe, emit, retraction by string
content, checkpoint drain, restore, compaction, arena growth, rejections.

Reference: the unchanged CPU oracle on surrogate ids (rwtest/varchar.py).
The q8-shaped stream is the one tests/test_varchar_workload.py pins.
"""
import ctypes as C

import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest.ffi import (JOIN_FULL_OUTER, JOIN_INNER, JOIN_LEFT_OUTER,
                        JOIN_LEFT_SEMI, SIDE_LEFT, SIDE_RIGHT, T_I64, T_TS)
from rwtest.varchar import T_VARCHAR, VChunk
from test_gpu_parity import net_rows

pytestmark = pytest.mark.gpu

TL, TR = vc.schema_types(vc.Q8_LEFT), vc.schema_types(vc.Q8_RIGHT)


def gpu():
    import risingwave_amd

    return ffi.Lib(risingwave_amd.lib_path())


def gpu_join(join_type, types_l, types_r, kw, **extra):
    return ffi.HashJoin(gpu(), join_type, types_l, types_r, **kw, **extra)


@pytest.fixture(scope="module")
def q8():
    """The pinned workload and its oracle reference, computed once."""
    epochs = vc.q8_workload()
    outs, drains, sur = vc.oracle_run(JOIN_INNER, TL, TR, vc.Q8_KW, epochs,
                                      drains=True)
    return epochs, outs, drains, sur


def drain_both(g):
    return [ffi.join_checkpoint_drain(g.lib, g.h, s) for s in (0, 1)]


def run_gpu(g, epochs, first_epoch=0, drain=True):
    """Push epochs; returns (per-push sorted rows, per-epoch [drain0, drain1])."""
    outs, drains = [], []
    for e, chunks in enumerate(epochs):
        for side, c in chunks:
            g.push(side, c)
            outs.append(vc.rows_of(vc.poll_all(g)))
        g.flush(first_epoch + e + 1)
        if drain:
            drains.append(drain_both(g))
    return outs, drains


# 1. inner join, q8-shaped, ~20 % retractions on both sides
def test_inner_q8_parity(q8):
    epochs, want, _, _ = q8
    g = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW, chunk_size=100)
    got, _ = run_gpu(g, epochs, drain=False)
    g.close()
    i = 0
    for e, chunks in enumerate(epochs):
        eg, ew = [], []
        for _ in chunks:
            assert got[i] == want[i], (
                f"epoch {e} push {i}: {len(got[i])} vs {len(want[i])} rows; "
                f"{next(((a, b) for a, b in zip(got[i], want[i]) if a != b), None)}")
            eg += got[i]
            ew += want[i]
            i += 1
        assert vc.sort_rows(eg) == vc.sort_rows(ew)  # the per-epoch multiset


# 2. the inner probe's pre-assigned sparse output: sentinel slots for the
#    unmatched rows, the overflow region past n for rows with > 1 match
def test_sparse_path_exact_strings():
    names = [b"", vc.UTF8, vc.LONG, vc.PREFIX_A, vc.PREFIX_B, None]
    left_rows = []
    for i in range(150):
        k = i % 60  # keys 0..59: 2-3 persons each
        nm = names[i % len(names)] if i % 4 == 0 else b"person-%d" % i
        left_rows.append((k, nm, 1000 + i))
    left = VChunk.from_rows(TL, [0] * len(left_rows), left_rows)
    # 256 all-insert, all-valid probe rows: sellers 0..59 match 2-3 rows,
    # sellers 60..127 match nothing
    right_rows = [(r % 128, 5 * r, 7000 + r) for r in range(256)]
    right = VChunk.from_rows(TR, [0] * 256, right_rows)
    # then the varchar on the PROBE side: 256 fresh persons, non-NULL names
    left2_rows = [(r % 128, b"late-%d" % r * (1 + r % 3), 9000 + r)
                  for r in range(256)]
    left2 = VChunk.from_rows(TL, [0] * 256, left2_rows)
    pushes = [[(SIDE_LEFT, left), (SIDE_RIGHT, right), (SIDE_LEFT, left2)]]
    want, _, _ = vc.oracle_run(JOIN_INNER, TL, TR, vc.Q8_KW, pushes)
    g = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    got, _ = run_gpu(g, pushes, drain=False)
    g.close()
    assert got[0] == want[0] == []
    per_probe = {}
    for _, row in want[1]:
        per_probe[row[-1]] = per_probe.get(row[-1], 0) + 1
    assert max(per_probe.values()) >= 2 and len(per_probe) < 256
    assert len(want[1]) > 256  # overflow region in use
    assert got[1] == want[1]
    assert got[2] == want[2] and len(want[2]) > 256


# 3. varchar on both sides, two varchar columns on one side, non-inner types
NI_LEFT = [(T_I64, "key"), (T_I64, "uniq"), (T_VARCHAR, "str"),
           (T_VARCHAR, "str")]
NI_RIGHT = [(T_I64, "key"), (T_VARCHAR, "str"), (T_I64, "uniq")]
NI_KW = dict(key_l=[0], key_r=[0], pk_l=[1], pk_r=[2])


@pytest.mark.parametrize("jt", [JOIN_LEFT_OUTER, JOIN_FULL_OUTER,
                                JOIN_LEFT_SEMI])
def test_noninner_two_sided_varchar(jt):
    tl, tr = vc.schema_types(NI_LEFT), vc.schema_types(NI_RIGHT)
    epochs = vc.make_workload(4100 + jt, [NI_LEFT, NI_RIGHT], [50, 70],
                              chunks_per_epoch=4)
    want, _, _ = vc.oracle_run(jt, tl, tr, NI_KW, epochs)
    g = gpu_join(jt, tl, tr, NI_KW)
    got, _ = run_gpu(g, epochs, drain=False)
    g.close()
    saw_null_side = False
    for i, (a, b) in enumerate(zip(got, want)):
        assert net_rows(a) == net_rows(b), f"type {jt} push {i}"
        if jt != JOIN_LEFT_SEMI:
            saw_null_side |= any(all(v is None for v in row[len(tl):])
                                 for _, row in a)
    assert jt == JOIN_LEFT_SEMI or saw_null_side  # NULL strings were emitted


# 4. arena growth: words are offsets, so rows inserted before a reallocation
#    still resolve after it
def test_arena_growth():
    lib = gpu()
    g = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    assert vc.varlen_reserve(lib, g.h, SIDE_RIGHT, 4096) == vc.RW_E_INVAL
    assert vc.varlen_reserve(lib, g.h, SIDE_LEFT, 4096) == 0
    assert vc.varlen_stats(lib, g.h, SIDE_LEFT) == (0, 4096)
    early = [(k, b"early-%03d" % k, 100 + k) for k in range(64)]
    bulk = [(1000 + i, bytes([65 + i % 26]) * 160, 5000 + i)
            for i in range(420)]  # ~67 KB
    probe = [(k, 0, 9000 + k) for k in range(64)] + \
            [(1000 + i, 0, 9500 + i) for i in range(0, 420, 7)]
    pushes = [[(SIDE_LEFT, VChunk.from_rows(TL, [0] * 64, early))],
              [(SIDE_LEFT, VChunk.from_rows(TL, [0] * 210, bulk[:210])),
               (SIDE_LEFT, VChunk.from_rows(TL, [0] * 210, bulk[210:]))],
              [(SIDE_RIGHT, VChunk.from_rows(TR, [0] * len(probe), probe))]]
    want, _, _ = vc.oracle_run(JOIN_INNER, TL, TR, vc.Q8_KW, pushes)
    run_gpu(g, pushes[:1], drain=False)
    used0, cap0 = vc.varlen_stats(lib, g.h, SIDE_LEFT)
    assert cap0 == 4096 and 0 < used0 <= 4096
    assert vc.varlen_reserve(lib, g.h, SIDE_LEFT, 8192) == vc.RW_E_INVAL
    run_gpu(g, pushes[1:2], drain=False)
    used1, cap1 = vc.varlen_stats(lib, g.h, SIDE_LEFT)
    assert used1 >= 64 * 1024 and cap1 > cap0 and cap1 >= used1
    got, _ = run_gpu(g, pushes[2:], drain=False)
    g.close()
    assert got[0] == want[3] and len(got[0]) == len(probe)


def _assert_drains_match(gd, od, sur, types, what):
    """GPU frames vs the oracle's surrogate frames: same frame order, same
    put flags, byte-equal keys (varchar is never in a key); values equal
    after mapping the surrogate ids back to strings."""
    gf, of = vc.decode_frames(gd), vc.decode_frames(od)
    assert [(p, k) for p, k, _ in gf] == [(p, k) for p, k, _ in of], what
    st = sur.types(types)
    for (put, _, gv), (_, _, ov) in zip(gf, of):
        if not put:
            assert gv == ov == b"", what
            continue
        orow = vc.decode_row(ov, st)
        orow = tuple(sur.str_of[v] if t == T_VARCHAR and v is not None else v
                     for t, v in zip(types, orow))
        assert vc.decode_row(gv, types) == orow, what


# 5. checkpoint drain of both sides every epoch
def test_checkpoint_drain_parity(q8):
    epochs, _, odr, sur = q8
    g = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    _, gdr = run_gpu(g, epochs)
    g.close()
    n_put_str = 0
    for e in range(len(epochs)):
        for s, types in ((0, TL), (1, TR)):
            _assert_drains_match(gdr[e][s], odr[e][s], sur, types,
                                 f"epoch {e} side {s}")
        n_put_str += sum(p for p, _, _ in vc.decode_frames(gdr[e][0]))
    assert n_put_str > 100  # the left table really spilled strings


# 6a. restore: run, drain, destroy, restore into a fresh executor, continue
def test_restore_continues_identically(q8):
    epochs, want, _, _ = q8
    lib = gpu()
    ref = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    ref_out, ref_dr = run_gpu(ref, epochs)
    ref.close()
    a = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    _, dr = run_gpu(a, epochs[:2])
    a.close()
    b = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    for s in (0, 1):
        ffi.join_restore(lib, b.h, s, b"".join(d[s] for d in dr))
    assert vc.varlen_stats(lib, b.h, SIDE_LEFT)[0] > 0
    out2, dr2 = run_gpu(b, epochs[2:], first_epoch=2)
    b.close()
    n2 = len(epochs[2])
    assert out2 == ref_out[-n2:] == want[-n2:]
    # restored rows are not re-PUT: the epoch's delta equals the
    # uninterrupted run's
    assert dr2[0] == ref_dr[2]


# 6b. compaction twin run
def test_compact_twin(q8):
    epochs, _, _, _ = q8
    lib = gpu()
    a = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    b = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    run_gpu(a, epochs[:2])
    run_gpu(b, epochs[:2])
    used_before = vc.varlen_stats(lib, b.h, SIDE_LEFT)[0]
    assert used_before == vc.varlen_stats(lib, a.h, SIDE_LEFT)[0]
    rec_l = ffi.join_compact(lib, b.h, SIDE_LEFT)
    rec_r = ffi.join_compact(lib, b.h, SIDE_RIGHT)
    used_after = vc.varlen_stats(lib, b.h, SIDE_LEFT)[0]
    assert rec_l > 0 and rec_r > 0
    assert 0 < used_after < used_before
    assert rec_l >= used_before - used_after  # arena bytes are counted
    out_a, dr_a = run_gpu(a, epochs[2:], first_epoch=2)
    out_b, dr_b = run_gpu(b, epochs[2:], first_epoch=2)
    a.close()
    b.close()
    assert out_a == out_b
    assert dr_a == dr_b


# 7. rejections
@pytest.mark.parametrize("what,kw", [
    ("join key", dict(key_l=[1], key_r=[0], pk_l=[0, 2], pk_r=[2])),
    ("pk", dict(key_l=[0], key_r=[0], pk_l=[1], pk_r=[2])),
    ("condition", dict(**vc.Q8_KW, cond=(ffi.CMP_LT, 1, 4))),
    ("inequality", dict(**vc.Q8_KW, wm_ineq=[(1, 1, True, True)])),
])
def test_create_rejects_varchar_outside_payload(what, kw):
    with pytest.raises(RuntimeError) as ei:
        gpu_join(JOIN_INNER, TL, TR, kw)
    assert "varchar" in str(ei.value) and what in str(ei.value)


def test_entry_points_reject_varchar_executor():
    lib = gpu()
    L = lib.lib
    g = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    h = C.c_void_p(g.h)
    nul = C.c_void_p(None)
    L.rw_hash_join_ingest_mode.restype = C.c_int
    L.rw_hash_join_ingest_mode.argtypes = [C.c_void_p, C.c_int]
    calls = {
        "ingest_mode": lambda: L.rw_hash_join_ingest_mode(h, 1),
        "bench_apply": lambda: L.rw_join_bench_apply(h, C.c_int(0), nul),
        "bench_run": lambda: L.rw_join_bench_run(h, C.c_int(0), nul,
                                                 C.c_int(0), C.c_int(0)),
        "apply_aggout": lambda: L.rw_join_apply_aggout(
            h, nul, C.c_int(0), nul, C.c_int(0), C.c_uint64(0)),
        "marshal_output": lambda: L.rw_join_marshal_output(h),
        "agg_apply_joinout": lambda: L.rw_agg_apply_joinout(nul, h),
        "vnode_hop": lambda: L.rw_join_vnode_hop(
            h, nul, C.c_uint32(0), C.c_uint8(0), C.c_uint32(256)),
        "q7pipe_bench_run": lambda: L.rw_q7pipe_bench_run(
            nul, h, nul, nul, C.c_int(0), C.c_int(0), C.c_int(0), nul,
            C.c_int(0), C.c_int(0)),
    }
    for name, call in calls.items():
        assert call() == vc.RW_E_INVAL, name
        assert "varchar" in lib.last_error(), name
    assert L.rw_hash_join_ingest_mode(h, 0) == 0
    g.close()


def test_push_rejects_bad_offsets_before_any_copy():
    lib = gpu()
    L = lib.lib
    types = [T_I64, T_VARCHAR, T_I64]
    g = gpu_join(JOIN_INNER, types, TR,
                 dict(key_l=[0], key_r=[0], pk_l=[2], pk_r=[2]))

    def push_raw(n, offsets):
        vd, keep = vc.raw_varchar_chunk(n, offsets)
        ones = np.ones(n, np.uint8)
        ids = np.arange(n, dtype=np.int64)
        cols = (ffi.RwColumn * 3)()
        for i, t in enumerate(types):
            cols[i].type = t
            cols[i].valid = ones.ctypes.data
            cols[i].data = C.addressof(vd) if t == T_VARCHAR else ids.ctypes.data
        ops = np.zeros(n, np.uint8)
        ch = ffi.RwChunkC()
        ch.n_rows, ch.n_cols = n, 3
        ch.ops = C.cast(ops.ctypes.data, C.POINTER(C.c_uint8))
        ch.vis = None
        ch.cols = cols
        return L.rw_hash_join_push_chunk(g.h, SIDE_LEFT, C.byref(ch))

    # a string of 2^24 bytes: one past the word's 24-bit length field. The
    # offsets CLAIM it; the byte buffer is one byte long and never read.
    assert push_raw(1, [0, 1 << 24]) == vc.RW_E_INVAL
    assert "2^24" in lib.last_error()
    assert push_raw(2, [0, 5, 3]) == vc.RW_E_INVAL      # non-monotone
    assert push_raw(1, [1, 1]) == vc.RW_E_INVAL         # offsets[0] != 0
    assert vc.varlen_stats(lib, g.h, SIDE_LEFT)[0] == 0  # nothing appended
    # the executor still works
    g.push(SIDE_LEFT, VChunk.from_rows(types, [0], [(7, b"ok", 1)]))
    g.push(SIDE_RIGHT, VChunk.from_rows(TR, [0], [(7, 0, 2)]))
    assert vc.rows_of(vc.poll_all(g)) == [("+", (7, b"ok", 1, 7, 0, 2))]
    g.close()


# 8. an i64-only join is unaffected by a varchar executor in the process
def test_i64_join_unchanged_around_varchar_executor():
    def q8_i64():
        rng = np.random.default_rng(8)
        t4 = [T_I64, T_TS, T_TS, T_I64]
        kw = dict(key_l=[0, 1, 2], key_r=[0, 1, 2], pk_l=[3], pk_r=[3])
        g = ffi.HashJoin(gpu(), JOIN_INNER, t4, t4, **kw)
        o = ffi.HashJoin(ffi.oracle(), JOIN_INNER, t4, t4, **kw)
        outs, rowid = [], 0
        for i in range(4):
            n = 1024
            ids = rng.integers(0, 1500, n)
            ws = rng.integers(0, 4, n) * 10_000_000
            rid = np.arange(rowid, rowid + n)
            rowid += n
            c = ffi.Chunk(t4, np.zeros(n, np.uint8),
                          [ids, ws, ws + 10_000_000, rid],
                          [np.ones(n, np.uint8)] * 4)
            g.push(i % 2, c)
            o.push(i % 2, c)
            mg = ffi.rows_multiset(g.poll_all())
            assert mg == ffi.rows_multiset(o.poll_all())
            outs.append(mg)
        g.close()
        o.close()
        return outs

    before = q8_i64()
    v = gpu_join(JOIN_INNER, TL, TR, vc.Q8_KW)
    v.push(SIDE_LEFT, VChunk.from_rows(TL, [0, 0], [(1, b"a", 1), (2, None, 2)]))
    v.push(SIDE_RIGHT, VChunk.from_rows(TR, [0], [(1, 0, 3)]))
    assert vc.rows_of(vc.poll_all(v)) == [("+", (1, b"a", 1, 1, 0, 3))]
    after_alive = q8_i64()  # while the varchar executor still lives
    v.close()
    after = q8_i64()
    assert before == after_alive == after
    assert sum(len(o) for o in before) > 0
