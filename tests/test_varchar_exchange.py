"""Typed columns and a varchar byte payload through librw_exchange's
partition (rw_exchange_partition) and run (rw_exchange_run_typed) entries
(DESIGN.md §14), on one GPU: the destination count is an argument, so the
partition kernels run at 1..64 destinations without a second device.

Reference: the Python partition of the input by zlib.crc32 over the
hash_datum feed; blocks are decoded by rwtest/xpayload.py from the layout
text, which also asserts the byte-region invariants on every block.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest import xpayload as xp
from rwtest.ffi import JOIN_INNER, T_I64, T_TS
from rwtest.varchar import T_VARCHAR, VChunk

pytestmark = pytest.mark.gpu

PERSON = [T_I64, T_VARCHAR, T_TS]
AUCTION = [T_I64, T_TS, T_I64]


@pytest.fixture(scope="module")
def xl():
    x = xp.XLib()
    yield x
    x.close()


def person_cols(seed, n):
    rng = np.random.default_rng(seed)
    ids = [None if rng.random() < 0.03 else int(rng.integers(0, 400))
           for _ in range(n)]
    names = xp.name_column(rng, n)
    ts = [int(t) for t in rng.integers(10**15, 2 * 10**15, n)]
    ops = rng.integers(0, 2, n).astype(np.uint8)
    return [ids, names, ts], ops


@pytest.fixture(scope="module")
def person(xl):
    """1000 and 20 person rows, staged once and shared (read-only)."""
    out = {}
    for n in (1000, 20):
        cols, ops = person_cols(1407 + n, n)
        out[n] = (cols, ops, xp.Batch(xl, PERSON, cols, ops))
    yield out
    for _, _, b in out.values():
        b.free()


def check_partition(xl, types, cols, ops, batch, keys, n_dests,
                    vnode_count=256):
    got = xp.partition(xl, batch, keys, n_dests, vnode_count)
    assert got.rc == 0, got.err
    want = xp.python_partition(types, cols, ops, keys, n_dests, vnode_count)
    off = 0
    for d in range(n_dests):
        assert xp.sort_block(got.blocks[d]) == xp.sort_block(want[d]), \
            f"destination {d}"
        # reported rows / bytes / offsets match the decoded blocks
        assert got.rows[d] == len(want[d])
        assert got.vbytes[d] == sum(
            len(v) for _, row in want[d] for v in row if isinstance(v, bytes))
        assert got.offs[d] == off and off % 32 == 0
        off += xp.Layout(got.rows[d], len(types), got.vbytes[d]).total
    return got


# 7. partition-only, q8-person shape, every destination count and key choice
@pytest.mark.parametrize("keys", [[0], [1], [0, 1]],
                         ids=["by_id", "by_name", "by_id_name"])
@pytest.mark.parametrize("n_dests", [1, 2, 3, 8, 64])
def test_partition_person(xl, person, n_dests, keys):
    cols, ops, batch = person[1000]
    assert xp.HUGE in cols[1] and None in cols[1] and b"" in cols[1]
    got = check_partition(xl, PERSON, cols, ops, batch, keys, n_dests)
    assert any(got.rows)  # at 64 destinations too, by the reference's input
    assert sum(got.rows) == 1000
    # 20 rows into up to 64 destinations: empty ones by pigeonhole
    cols, ops, batch = person[20]
    got = check_partition(xl, PERSON, cols, ops, batch, keys, n_dests)
    if n_dests == 64:
        empty = [d for d in range(64) if got.rows[d] == 0]
        assert len(empty) >= 44
        assert all(got.vbytes[d] == 0 for d in empty)
        assert all(o % 32 == 0 for o in got.offs)


def test_partition_rejects_bad_dest_counts(xl, person):
    _, _, batch = person[20]
    for nd in (0, 65, -1):
        got = xp.partition(xl, batch, [0], nd)
        assert got.rc == -1 and "n_dests" in got.err
    got = xp.partition(xl, batch, [0], 4)  # a valid call afterwards works
    assert got.rc == 0 and sum(got.rows) == 20


# 8. two varchar + two i64 columns, NULLs independent per column; a
#    non-power-of-two vnode_count for the clamp
def test_partition_two_varchar_columns(xl):
    rng = np.random.default_rng(1408)
    n = 700
    types = [T_VARCHAR, T_I64, T_VARCHAR, T_I64]
    cols = [xp.name_column(rng, n),
            [None if rng.random() < 0.2 else int(rng.integers(-2**62, 2**62))
             for _ in range(n)],
            list(reversed(xp.name_column(rng, n))),
            list(range(n))]
    ops = rng.integers(0, 4, n).astype(np.uint8)
    both = sum(1 for a, b in zip(cols[0], cols[2]) if a is None or b is None)
    assert 0 < both < n
    batch = xp.Batch(xl, types, cols, ops)
    try:
        for keys, nd, vnc in ([[3], 8, 256], [[2, 1], 5, 100], [[0], 64, 100]):
            check_partition(xl, types, cols, ops, batch, keys, nd, vnc)
    finally:
        batch.free()


def _old_run(xl, batch, n_cols, keys, send, recv, cap):
    vals = (C.c_void_p * n_cols)(*[batch.desc[c].vals for c in range(n_cols)])
    valids = (C.c_void_p * n_cols)(*[batch.desc[c].valid
                                     for c in range(n_cols)])
    kc = (C.c_uint32 * len(keys))(*keys)
    sc, rc_ = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    rc = xl.L.rw_exchange_run(xl.h, vals, valids, batch.ops, batch.n, n_cols,
                              kc, len(keys), 256, send, cap, recv, cap, sc, rc_)
    assert rc == 0, xl.err()
    return sc[0], rc_[0]


def _run_typed(xl, batch, keys, send, send_cap, recv, recv_cap):
    R = xl.world
    kc = (C.c_uint32 * len(keys))(*keys)
    arrs = [(C.c_uint64 * R)() for _ in range(4)]
    rc = xl.L.rw_exchange_run_typed(
        xl.h, batch.desc, len(batch.types), batch.ops, batch.n, kc, len(keys),
        256, send, send_cap, recv, recv_cap, *arrs)
    return rc, [list(a) for a in arrs]


# 9. all-i64 batch: the old entry against the typed entry at R = 1
def test_all_i64_old_entry_equals_typed(xl):
    rng = np.random.default_rng(1409)
    n = 1000
    types = [T_I64, T_I64, T_TS]
    cols = [[None if rng.random() < 0.1 else int(rng.integers(0, 50))
             for _ in range(n)],
            [int(v) for v in rng.integers(-2**62, 2**62, n)],
            list(range(n))]
    ops = rng.integers(0, 4, n).astype(np.uint8)
    batch = xp.Batch(xl, types, cols, ops)
    cap = 1 << 20
    bufs = [xl.alloc(cap) for _ in range(4)]
    try:
        s_old, r_old = _old_run(xl, batch, 3, [0], bufs[0], bufs[1], cap)
        rc, (s_rows, s_vb, r_rows, r_vb) = _run_typed(
            xl, batch, [0], bufs[2], cap, bufs[3], cap)
        assert rc == 0, xl.err()
        assert (s_old, r_old) == (n, n) == (s_rows[0], r_rows[0])
        assert s_vb == [0] and r_vb == [0]
        size = xp.Layout(n, 3, 0).total
        assert size == xp.old_block_bytes(n, 3)  # equal block size
        old = xp.decode_block(xl.download(bufs[1], size), n, types, 0)
        new = xp.decode_block(xl.download(bufs[3], size), n, types, 0)
        assert xp.sort_block(old) == xp.sort_block(new)
        assert xp.sort_block(new) == xp.sort_block(
            [(int(ops[r]), tuple(c[r] for c in cols)) for r in range(n)])
        # and at several destinations the typed partition runs the same
        # all-i64 kernels
        check_partition(xl, types, cols, ops, batch, [0], 3)
        check_partition(xl, types, cols, ops, batch, [0, 2], 64)
    finally:
        batch.free()
        for b in bufs:
            xl.free(b)


def _crc_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, np.uint32(0xEDB88320) ^ (t >> 1), t >> 1)
    return t.astype(np.uint32)


def np_vnode_i64(vals, vnode_count=256):
    """Vectorised IEEE CRC-32 of one non-NULL i64 per row (8 LE bytes)."""
    tab = _crc_table()
    crc = np.full(len(vals), 0xFFFFFFFF, np.uint32)
    v = vals.astype(np.int64).view(np.uint64)
    for i in range(8):
        byte = ((v >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.uint32)
        crc = tab[(crc ^ byte) & np.uint32(0xFF)] ^ (crc >> np.uint32(8))
    return (crc ^ np.uint32(0xFFFFFFFF)) % np.uint32(vnode_count)


def _name_of_id(ids):
    return (ids.astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345)
            ).astype(np.uint32)


# 10. the grid-stride path: the grid is capped at 2048 blocks of 256 threads,
#     so this is the smallest size with a second stride iteration
def test_partition_grid_stride(xl):
    n = 2048 * 256 + 777
    n_dests = 8
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    names = _name_of_id(ids)                     # 4 bytes per row
    lead = 3                                     # unaligned strings
    arena = np.concatenate([np.full(lead, 0xA5, np.uint8),
                            names.view(np.uint8), np.zeros(1, np.uint8)])
    words = (np.uint64(lead) + np.arange(n, dtype=np.uint64) * np.uint64(4)) \
        | (np.uint64(4) << np.uint64(xp.OFF_BITS))
    ones = np.ones(n, np.uint8)
    ops = (ids & 1).astype(np.uint8)
    # the vectorised reference agrees with zlib on a sample
    vn = np_vnode_i64(ids)
    for r in (0, 1, 777, n // 2, n - 1):
        assert vn[r] == xp.expected_vnode([int(ids[r])])
    want_dest = np.minimum(vn // (256 // n_dests), n_dests - 1)
    want_rows = np.bincount(want_dest, minlength=n_dests).tolist()

    batch = xp.Batch(xl, PERSON, [(ids, ones, None),
                                  (words.view(np.int64), ones, arena),
                                  (ids + 7, ones, None)], ops)
    try:
        got = xp.partition(xl, batch, [0], n_dests, send_cap=n * 40 + (1 << 20),
                           decode=False)
    finally:
        batch.free()
    assert got.rc == 0, got.err
    assert got.rows == want_rows and got.vbytes == [4 * r for r in want_rows]
    seen = []
    for d in range(n_dests):
        nr = got.rows[d]
        ops_d, w, valid, region = xp.decode_block_np(got.raw[d], nr, PERSON,
                                                     got.vbytes[d])
        assert all(np.all(v == 1) for v in valid)
        rid = w[0].view(np.int64)
        assert np.all(want_dest[(rid - 1) // 3] == d)
        assert np.all(w[2].view(np.int64) == rid + 7)
        assert np.all(ops_d == (rid & 1))
        assert np.all(w[1] >> np.uint64(xp.OFF_BITS) == 4)
        off = (w[1] & np.uint64(xp.MAX_OFF)).astype(np.int64)
        name = region[off[:, None] + np.arange(4)]
        name = np.ascontiguousarray(name).view(np.uint32).ravel()
        assert np.array_equal(name, _name_of_id(rid)), f"id->name, dest {d}"
        seen.append(rid)
    assert np.array_equal(np.sort(np.concatenate(seen)), ids)


# 11. typed run at R = 1; caps one byte short of the reported need
def test_run_typed_single_rank_and_caps(xl, person):
    cols, ops, batch = person[1000]
    part = xp.partition(xl, batch, [0], 1)
    assert part.rc == 0, part.err
    need = part.sizes[0]
    send, recv = xl.alloc(need), xl.alloc(need)
    try:
        rc, (s_rows, s_vb, r_rows, r_vb) = _run_typed(
            xl, batch, [0], send, need, recv, need)
        assert rc == 0, xl.err()
        assert s_rows == r_rows == [1000] and s_vb == r_vb == part.vbytes
        sent = xl.download(send, need)
        got = xl.download(recv, need)
        want = xp.python_partition(PERSON, cols, ops, [0], 1)[0]
        assert xp.sort_block(xp.decode_block(got, 1000, PERSON, r_vb[0])) == \
            xp.sort_block(want)
        # the recv buffer equals the send block (pad bytes are unspecified)
        used = xp.Layout(1000, 3, r_vb[0])
        assert np.array_equal(got[:used.ops_off + 1000],
                              sent[:used.ops_off + 1000])
        assert np.array_equal(
            got[used.vbytes_off:used.vbytes_off + r_vb[0]],
            sent[used.vbytes_off:used.vbytes_off + r_vb[0]])

        fill = np.full(need, 0xCD, np.uint8)
        for which, code in (("send", -2), ("recv", -3)):
            xl.L.rw_xbuf_write(send, fill.ctypes.data, need)
            xl.L.rw_xbuf_write(recv, fill.ctypes.data, need)
            rc, _ = _run_typed(xl, batch, [0], send,
                               need - 1 if which == "send" else need, recv,
                               need - 1 if which == "recv" else need)
            assert rc == code
            assert "too small" in xl.err()
            if which == "send":  # nothing was written at all
                assert np.array_equal(xl.download(send, need), fill)
            assert np.array_equal(xl.download(recv, need), fill)
        rc, _ = _run_typed(xl, batch, [0], send, need, recv, need)
        assert rc == 0, xl.err()
    finally:
        xl.free(send)
        xl.free(recv)


# ---- 12. sharded q8 on one GPU ----

def q8_stream(seed, n_epochs=3, chunks_per_epoch=4, n_rows=240):
    """Two-sided q8 stream with retractions on both sides in which no pk
    occurs twice within one chunk (a delete only retracts a row of an
    EARLIER chunk, at most once per chunk), so the row order inside a block
    cannot matter. person pk = (id, ts), auction pk = column 2."""
    rng = np.random.default_rng(seed)
    live = {0: [], 1: []}
    uniq = [0]
    epochs = []
    for _ in range(n_epochs):
        chunks = []
        for ci in range(chunks_per_epoch):
            side = ci % 2
            ops, rows = [], []
            n_del = min(len(live[side]), n_rows // 5)
            picks = rng.choice(len(live[side]), n_del, replace=False) \
                if n_del else []
            for i in sorted((int(p) for p in picks), reverse=True):
                ops.append(1)
                rows.append(live[side].pop(i))
            fresh = []
            for _r in range(n_rows - n_del):
                uniq[0] += 1
                if side == 0:
                    nm = xp.SPECIAL_NAMES[uniq[0] % 40] if uniq[0] % 40 < len(
                        xp.SPECIAL_NAMES) - 1 else b"person-%d" % uniq[0]
                    fresh.append((int(rng.integers(0, 120)), nm, uniq[0]))
                else:
                    fresh.append((int(rng.integers(0, 160)),
                                  int(rng.integers(0, 10**6)), uniq[0]))
            ops += [0] * len(fresh)
            rows += fresh
            order = rng.permutation(len(rows))
            ops = [ops[i] for i in order]
            rows = [rows[i] for i in order]
            live[side].extend(fresh)
            pks = [(r[0], r[2]) if side == 0 else r[2] for r in rows]
            assert len(set(pks)) == len(pks), "pk twice within one chunk"
            chunks.append((side, ops, rows))
        epochs.append(chunks)
    assert any(op == 1 for ch in epochs for s, ops, _ in ch for op in ops
               if s == 0)
    assert any(op == 1 for ch in epochs for s, ops, _ in ch for op in ops
               if s == 1)
    return epochs


Q8_TYPES = {0: PERSON, 1: AUCTION}


def gpu_join():
    import risingwave_amd

    return ffi.HashJoin(ffi.Lib(risingwave_amd.lib_path()), JOIN_INNER,
                        PERSON, AUCTION, **vc.Q8_KW)


def single_executor_epochs(epochs):
    g = gpu_join()
    out = []
    for e, chunks in enumerate(epochs):
        rows = []
        for side, ops, crows in chunks:
            g.push(side, VChunk.from_rows(Q8_TYPES[side], ops, crows))
            for c in vc.poll_all(g):
                rows.extend(c.visible_rows())
        g.flush(e + 1)
        out.append(vc.sort_rows(rows))
    g.close()
    return out


def test_sharded_q8_union_equals_single(xl):
    epochs = q8_stream(1412)
    want = single_executor_epochs(epochs)
    assert all(len(w) > 0 for w in want)
    n_shards = 4
    joins = [gpu_join() for _ in range(n_shards)]
    routed = [0] * n_shards
    for e, chunks in enumerate(epochs):
        rows = []
        for side, ops, crows in chunks:
            types = Q8_TYPES[side]
            cols = [[r[i] for r in crows] for i in range(3)]
            batch = xp.Batch(xl, types, cols, ops)
            try:
                part = xp.partition(xl, batch, [0], n_shards)
            finally:
                batch.free()
            assert part.rc == 0, part.err
            for d in range(n_shards):
                if not part.blocks[d]:
                    continue
                routed[d] += len(part.blocks[d])
                joins[d].push(side, VChunk.from_rows(
                    types, [op for op, _ in part.blocks[d]],
                    [row for _, row in part.blocks[d]]))
                for c in vc.poll_all(joins[d]):
                    rows.extend(c.visible_rows())
        for j in joins:
            j.flush(e + 1)
        assert vc.sort_rows(rows) == want[e], f"epoch {e}: shard union diverged"
    for j in joins:
        j.close()
    assert all(routed), routed  # every shard took part
