"""HashAgg key-table compaction (rw_hash_agg_compact): GPU vs
the CPU oracle on identical input. The oracle has no capacity and gets no
compaction call; it is the reference as it stands.

Tables are at state_capacity_hint 1, 2 and 64 with the aimed keys of
test_state_table_pressure.py: agg_keys(64) puts a 24-key cluster on home
slot 63 that wraps through slot 0, so a reinsert that mishandles the wrap or
a clear that misses an array shows at these sizes. Every comparison is exact:
output rows per epoch, spill drains byte for byte. A small Python model of
the slot occupancy (SlotModel) says what rw_hash_agg_state_stats and the
`reclaimed` count must read.
"""
import numpy as np
import pytest

from rwtest import ffi
from rwtest import varchar_agg as va
from rwtest.agg_compact import (RW_E_INVAL, compact, compact_rc, ingest_mode,
                                state_stats)
from rwtest.ffi import (AGG_COUNT, AGG_COUNT_STAR, AGG_MAX, AGG_MIN, AGG_SUM,
                        OP_DELETE, OP_INSERT, T_DECIMAL, T_I64,
                        agg_checkpoint_drain_bytes, agg_dedup_drain_bytes,
                        agg_minput_drain_bytes, agg_restore, dec_col, oracle)
from rwtest.streams import retract_mix
from rwtest.varchar import T_VARCHAR, VChunk
from test_state_table_pressure import (COUNT_SUM, DENSE_SHAPES, I3, SPLIT, G,
                                       agg_epoch, agg_keys, agg_pair,
                                       all_keys_chunk, chunk, covering,
                                       multiword_keys, owned_bitmap)
from test_vnode_dispatch import expected_vnode

pytestmark = pytest.mark.gpu

FRESH = 5 * 10**12  # keys no other set uses, above every watermark here


class SlotModel:
    """READY slots and live groups as the key table must hold them: a key
    takes a slot when first applied and keeps it until a compaction; it is
    live while its row count is positive and it has not been cleaned."""

    def __init__(self, cap):
        self.cap, self.ready, self.cnt = cap, set(), {}

    def apply(self, keys, ops=None):
        for i, k in enumerate(keys):
            sign = -1 if ops is not None and ops[i] == OP_DELETE else 1
            self.ready.add(k)
            self.cnt[k] = self.cnt.get(k, 0) + sign

    def clean(self, pred):
        for k in self.ready:
            if pred(k):
                self.cnt[k] = 0

    def live(self):
        return {k for k in self.ready if self.cnt.get(k, 0) > 0}

    def stats(self):
        return (len(self.ready), len(self.live()), self.cap)

    def compact(self):
        n = len(self.ready) - len(self.live())
        self.ready = self.live()
        return n


def check_compact(g, model):
    """Stats before, the reclaimed count and stats after against the model;
    a second call finds nothing."""
    assert state_stats(G(), g.h) == model.stats()
    want = model.compact()
    assert compact(G(), g.h) == want
    assert state_stats(G(), g.h) == model.stats()
    assert compact(G(), g.h) == 0
    return want


def clean(execs, wm, pos=0):
    for _, a in execs:
        a.watermark(pos, wm)


def close(execs):
    for _, a in execs:
        a.close()


# ----------------------------------------------------------------------
# 1. Slots come back
# ----------------------------------------------------------------------


def test_slots_come_back():
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9001)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 2)
    assert state_stats(G(), g.h) == (64, 32, 64)
    assert compact(G(), g.h) == 32
    assert state_stats(G(), g.h) == (32, 32, 64)
    fresh = [FRESH + i for i in range(32)]
    out = agg_epoch(execs, [all_keys_chunk(rng, fresh, 100)], 3)
    assert len(out) == 32 and all(op == "+" for op, _ in out)
    assert state_stats(G(), g.h) == (64, 64, 64)
    with pytest.raises(RuntimeError, match="agg state table full"):
        g.push(chunk([[FRESH + 32], [1]]))
        g.flush(4)
    close(execs)


def test_all_slots_come_back():
    keys = [k for k in agg_keys(64) if k < 10**15] + [3 * 10**12]
    assert len(keys) == 64
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9002)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    clean(execs, 10**15)
    agg_epoch(execs, [], 2)
    assert compact(G(), g.h) == 64
    assert state_stats(G(), g.h) == (0, 0, 64)
    other = [7 * 10**15 + 3 * i for i in range(64)]
    out = agg_epoch(execs, [all_keys_chunk(rng, other)], 3)
    assert len(out) == 64 and all(op == "+" for op, _ in out)
    agg_epoch(execs, [all_keys_chunk(rng, other)], 4)
    close(execs)


# ----------------------------------------------------------------------
# 2. State moves with its key: generic, multiword and dense apply
# ----------------------------------------------------------------------

GENERIC = [(AGG_COUNT_STAR, -1, T_I64), (AGG_COUNT, 1, T_I64),
           (AGG_SUM, 1, T_I64)]


def generic_chunk(rng, universe, pick, live, p_del, model):
    """agg_apply_kernel, non-dense: deletes, NULL arguments and a visibility
    mask whose hidden rows carry keys that are not in the table. `pick`
    indexes `universe`; live: earlier (index, value, valid) rows that
    deletes may retract."""
    nv = 4 * len(pick) + 8
    n = nv + 24
    kidx = covering(rng, np.asarray(pick, np.int64), nv)
    vals = rng.integers(1, 1000, nv)
    valid = (rng.random(nv) > 0.25).astype(np.int64)
    ops_v = retract_mix(rng, live, [kidx, vals, valid], p_del)
    model.apply([int(i) for i in kidx], ops_v)
    pos = np.sort(rng.choice(n, nv, replace=False))
    k = 7 * 10**15 + rng.integers(0, 1000, n)  # foreign, invisible
    v = rng.integers(1, 1000, n)
    va_ = np.ones(n, np.uint8)
    ops = np.zeros(n, np.uint8)
    vis = np.zeros(n, np.uint8)
    k[pos], v[pos] = np.asarray(universe, np.int64)[kidx], vals
    va_[pos], ops[pos], vis[pos] = valid, ops_v, 1
    return chunk([k, v], ops, [np.ones(n, np.uint8), va_], vis)


@pytest.mark.parametrize("hint", [1, 2, 64])
def test_state_moves_generic(hint):
    keys = list(agg_keys(hint))
    # what the watermark takes: half of the 64, the smaller of the two, the
    # only one
    wm = {64: SPLIT, 2: max(keys), 1: keys[0] + 1}[hint]
    dead = [i for i, k in enumerate(keys) if k < wm]
    surv = [i for i, k in enumerate(keys) if k >= wm]
    assert len(dead) == {64: 32, 2: 1, 1: 1}[hint]
    n_late = len(dead) // 2 if hint == 64 else 0
    universe = keys + [FRESH + i for i in range(len(dead) - n_late)]
    fresh = list(range(len(keys), len(universe)))
    g, o = agg_pair(GENERIC, 0, hint)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9100 + hint)
    model, live = SlotModel(hint), []
    every = list(range(len(keys)))
    agg_epoch(execs, [generic_chunk(rng, universe, every, live, 0.0, model)], 1)
    agg_epoch(execs, [generic_chunk(rng, universe, every, live, 0.3, model)], 2)
    clean(execs, wm)
    model.clean(lambda i: universe[i] < wm)
    live[:] = [r for r in live if universe[r[0]] >= wm]
    agg_epoch(execs, [], 3)
    assert check_compact(g, model) == len(dead)
    if surv:
        # the survivors' U-/U+ pairs carry the pre-compaction values
        was_live = model.live()
        assert len(was_live) >= (len(surv) + 1) // 2
        out = agg_epoch(execs, [generic_chunk(rng, universe, surv, live, 0.3,
                                              model)], 4)
        assert sum(op == "U-" for op, _ in out) >= (len(was_live) + 1) // 2
        assert sum(op == "+" for op, _ in out) == \
            len(model.live() - was_live)
    # the slots given back take new keys and late rows of dropped ones
    back = fresh + dead[:n_late]
    out = agg_epoch(execs, [generic_chunk(rng, universe, back, live, 0.0,
                                          model)], 5)
    assert sum(op == "+" for op, _ in out) == len(back)
    assert state_stats(G(), g.h) == model.stats()
    check_compact(g, model)
    now = sorted(model.live())
    agg_epoch(execs, [generic_chunk(rng, universe, now, live, 0.3, model)], 6)
    close(execs)


def mw_chunk(rng, keys, idx_pick, n, kw):
    idx = covering(rng, np.asarray(idx_pick), n)
    cols, valids = [], []
    for p in range(kw):
        w = np.array([keys[i][1][p] for i in idx], np.int64)
        va_ = np.array([not (keys[i][0] >> p) & 1 for i in idx], np.uint8)
        w[va_ == 0] = 777  # a NULL part carries a nonzero data word
        cols.append(w)
        valids.append(va_)
    cols.append(rng.integers(1, 1000, n))
    valids.append(np.ones(n, np.uint8))
    return chunk(cols, None, valids), [int(i) for i in idx]


@pytest.mark.parametrize("kw", [2, 3, 4])
def test_state_moves_multiword(kw):
    # 64 keys of kw words, 14 with a NULL part, 8 told from a NULL-part twin
    # by the null mask alone. A watermark of 3 on word 0 takes the keys whose
    # word 0 is a non-NULL 0.
    keys = list(multiword_keys(kw))
    dead = [i for i, (nm, w) in enumerate(keys) if not nm & 1 and w[0] < 3]
    surv = [i for i in range(64) if i not in dead]
    assert len(dead) >= 16 and len(surv) >= 16
    assert sum(1 for i in surv if keys[i][0]) >= 5  # NULL parts that move
    fresh_keys = [(0, (9,) + (-2,) * (kw - 2) + (v,))
                  for v in range(len(dead) - 8)]
    keys += fresh_keys
    fresh = list(range(64, len(keys)))
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, kw, T_I64)]
    g, o = agg_pair(calls, 0, 64, types=[T_I64] * (kw + 1),
                    group_key=tuple(range(kw)))
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9200 + kw)
    model = SlotModel(64)
    nonnull = [i for i in range(64) if not keys[i][0]]
    chunks = []
    for pick in (nonnull, list(range(64))):  # dense, then non-dense
        c, idx = mw_chunk(rng, keys, pick, 300, kw)
        model.apply(idx)
        chunks.append(c)
    agg_epoch(execs, chunks, 1)
    clean(execs, 3)
    model.clean(lambda i: i in dead)
    agg_epoch(execs, [], 2)
    assert check_compact(g, model) == len(dead)
    c, idx = mw_chunk(rng, keys, surv, 200, kw)
    model.apply(idx)
    out = agg_epoch(execs, [c], 3)
    assert sorted(op for op, _ in out) == ["U+"] * len(surv) + ["U-"] * len(surv)
    # new keys and 8 dropped ones that come back fill the table again
    c, idx = mw_chunk(rng, keys, fresh + dead[:8], 200, kw)
    model.apply(idx)
    out = agg_epoch(execs, [c], 4)
    assert [op for op, _ in out] == ["+"] * len(dead)
    assert state_stats(G(), g.h) == (64, 64, 64)
    c, idx = mw_chunk(rng, keys, sorted(model.live()), 300, kw)
    agg_epoch(execs, [c], 5)
    close(execs)


@pytest.mark.parametrize("n", [1024, 1025])
@pytest.mark.parametrize("shape", ["dense4_4", "span_max_count"])
def test_state_moves_dense(shape, n):
    # the dense KW=1 kernels (all-valid inserts, at least 1024 rows) find the
    # moved groups: max / min / sum continue from the pre-compaction values
    calls, rci = DENSE_SHAPES[shape]
    keys = agg_keys(64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(calls, rci, 64, append_only=True)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9300 + n)
    big = lambda ks: chunk([covering(rng, ks, n), rng.integers(1, 10**6, n)])
    agg_epoch(execs, [big(keys), big(keys)], 1)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 2)
    assert compact(G(), g.h) == 32
    out = agg_epoch(execs, [big(surv)], 3)
    assert sum(op == "U+" for op, _ in out) == 32
    assert not any(op == "+" for op, _ in out)
    fresh = [FRESH + i for i in range(32)]
    out = agg_epoch(execs, [big(surv + fresh)], 4)
    assert sum(op == "+" for op, _ in out) == 32
    assert state_stats(G(), g.h) == (64, 64, 64)
    close(execs)


# ----------------------------------------------------------------------
# 3. Every column moves
# ----------------------------------------------------------------------


def test_columns_value_states():
    # count(*), sum, append-only min and max: acc / has / prev / prev_null of
    # four calls, NULL arguments included (has stays 0 for some groups)
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 1, T_I64),
             (AGG_MIN, 1, T_I64), (AGG_MAX, 1, T_I64)]
    keys = agg_keys(64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(calls, 0, 64, append_only=True)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9400)

    def rows(ks, n, p_null):
        k = covering(rng, ks, n)
        valid = (rng.random(n) >= p_null).astype(np.uint8)
        # 8 of the survivors see NULL arguments only in the first epoch
        valid[np.isin(k, surv[:8])] &= p_null < 0.5
        return chunk([k, rng.integers(-10**6, 10**6, n)], None,
                     [np.ones(n, np.uint8), valid])

    agg_epoch(execs, [rows(keys, 300, 0.5)], 1)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 2)
    assert compact(G(), g.h) == 32
    out = agg_epoch(execs, [rows(surv, 200, 0.2)], 3)
    assert sum(op == "U-" for op, _ in out) == 32
    late = [k for k in keys if k < SPLIT][:16]
    agg_epoch(execs, [rows(surv + late, 300, 0.2)], 4)
    close(execs)


def dec_chunk(ks, decs, ops=None):
    n = len(ks)
    ops = np.zeros(n, np.uint8) if ops is None else np.asarray(ops, np.uint8)
    return ffi.Chunk([T_I64, T_DECIMAL], ops,
                     [np.asarray(ks, np.int64), dec_col(decs)],
                     [np.ones(n, np.uint8)] * 2)


def test_columns_decimal_sum():
    # dsum / dscl / dspec and the prev2 high halves; retractions of
    # pre-compaction rows arrive after the compaction
    import decimal

    calls = [(AGG_SUM, 1, T_DECIMAL), (AGG_COUNT_STAR, -1, T_I64)]
    keys = agg_keys(64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(calls, 1, 64, types=[T_I64, T_DECIMAL])
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9410)

    def rand_dec():
        return decimal.Decimal(int(rng.integers(-10**9, 10**9))).scaleb(
            -int(rng.integers(0, 6)))

    def inserts(ks, n):
        k = [int(x) for x in covering(rng, ks, n)]
        return k, [rand_dec() for _ in k]

    k1, d1 = inserts(keys, 300)
    # specials in three surviving groups (never retracted below)
    spec = ["NaN", "Inf", "-Inf"]
    agg_epoch(execs, [dec_chunk(k1 + surv[:3], d1 + spec)], 1)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 2)
    assert compact(G(), g.h) == 32
    old = [(k, d) for k, d in zip(k1, d1) if k >= SPLIT]
    pick = rng.choice(len(old), 60, replace=False)
    k3, d3 = inserts(surv, 100)
    out = agg_epoch(execs, [
        dec_chunk([old[i][0] for i in pick], [old[i][1] for i in pick],
                  np.ones(60, np.uint8)),
        dec_chunk(k3, d3)], 3)
    assert sum(op == "U-" for op, _ in out) >= 24
    late = [k for k in keys if k < SPLIT][:16]
    k4, d4 = inserts(surv + late, 200)
    out = agg_epoch(execs, [dec_chunk(k4, d4)], 4)
    assert sum(op == "+" for op, _ in out) == 16
    close(execs)


MINMAX2 = [(AGG_MIN, 1, T_I64), (AGG_MAX, 1, T_I64),
           (AGG_COUNT_STAR, -1, T_I64)]


def minput_epoch(execs, chunks, epoch, n_tables=2):
    out = agg_epoch(execs, chunks, epoch)
    for mi in range(n_tables):
        md = [agg_minput_drain_bytes(lib, a.h, mi) for lib, a in execs]
        for i in range(len(execs) - 1):
            assert md[i] == md[-1], (
                f"epoch {epoch} executor {i} minput table {mi}: "
                f"{len(md[i])} vs {len(md[-1])} bytes")
    return out


def test_columns_retractable_min_max():
    # two materialized-input calls: the chain heads of both move with the
    # group and every live row's owner is rewritten. Retractions of
    # pre-compaction rows arrive afterwards; the minput drains stay
    # byte-equal to the oracle's.
    keys = np.array(agg_keys(64), np.int64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(MINMAX2, 2, 64, types=I3, stream_key=(2,))
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9420)

    def inserts(ks, rid0, n):
        return [covering(rng, ks, n), rng.integers(-500, 500, n),
                np.arange(rid0, rid0 + n)]

    def deletes(rows, idx):
        return chunk([c[idx] for c in rows], np.ones(len(idx), np.uint8))

    # the row store of a hint-64 executor holds 512 rows and each of the
    # two calls keeps its own copy of a row: 200 input rows take 400
    e1 = inserts(keys, 0, 200)
    minput_epoch(execs, [chunk(e1)], 1)
    # some rows of surviving groups die before the compaction:
    # minput_compact renumbers the rest
    gone = rng.choice(np.flatnonzero(e1[0] >= SPLIT), 30, replace=False)
    minput_epoch(execs, [deletes(e1, gone)], 2)
    clean(execs, SPLIT)
    minput_epoch(execs, [], 3)
    assert compact(G(), g.h) >= 32  # groups emptied by epoch 2 are dead too
    ready, live, cap = state_stats(G(), g.h)
    assert ready == live <= 32 and cap == 64
    left = np.array([i for i in range(200)
                     if i not in set(gone) and e1[0][i] >= SPLIT])
    assert 50 < len(left) < 120
    half = rng.choice(left, len(left) // 2, replace=False)
    out = minput_epoch(execs, [deletes(e1, half),
                               chunk(inserts(surv, 1000, 60))], 4)
    assert sum(op == "U-" for op, _ in out) >= 16
    rest = np.array([i for i in left if i not in set(half)])
    minput_epoch(execs, [deletes(e1, rest)], 5)
    late = [k for k in keys if k < SPLIT][:8]
    minput_epoch(execs, [chunk(inserts(surv + late, 2000, 60))], 6)
    close(execs)


def test_columns_distinct():
    # DISTINCT calls: the dedup table is keyed by (group, datum) and stays
    # as it is; the key table of such an executor still compacts
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_COUNT, 1, T_I64, 1),
             (AGG_SUM, 1, T_I64, 1)]
    keys = np.array(agg_keys(64), np.int64)
    surv = np.array([k for k in keys if k >= SPLIT], np.int64)
    g, o = agg_pair(calls, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9430)
    live = []

    def epoch(ks, n, p_del, e):
        cols = [covering(rng, ks, n), rng.integers(0, 6, n)]
        ops = retract_mix(rng, live, cols, p_del)
        out = agg_epoch(execs, [chunk(cols, ops)], e)
        ds = [agg_dedup_drain_bytes(lib, a.h, 0) for lib, a in execs]
        assert ds[0] == ds[1], f"epoch {e}: dedup drain"
        return out

    epoch(keys, 400, 0.0, 1)
    clean(execs, SPLIT)
    live[:] = [r for r in live if r[0] >= SPLIT]
    epoch(surv, 100, 0.3, 2)
    assert compact(G(), g.h) >= 32
    out = epoch(surv, 200, 0.4, 3)
    assert any(op == "U-" for op, _ in out)
    epoch(surv, 200, 0.4, 4)
    close(execs)


# ----------------------------------------------------------------------
# 4. Steady state: a windowed plan in a table sized for its live windows
# ----------------------------------------------------------------------


def test_steady_state_windows():
    # 16 new window keys per epoch, the watermark trails by two epochs, so
    # at most 48 windows are live in a 64-slot table. 40 epochs bring 640
    # keys through it.
    PER, EPOCHS = 16, 40
    win = lambda e: [10**6 * (PER * e + i) + 17 for i in range(PER)]
    g, o = agg_pair(COUNT_SUM, 0, 64)
    g_never = agg_pair(COUNT_SUM, 0, 64)
    g_never[1].close()
    g_never = g_never[0]
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9500)
    drains = [bytearray(), bytearray()]
    n_compactions, never_failed_at = 0, None

    def epoch_chunk(e):
        ks = win(e) + (win(e - 1) if e else [])
        return all_keys_chunk(rng, ks, 80)

    for e in range(EPOCHS):
        c = epoch_chunk(e)
        agg_epoch(execs, [c], e + 1, drains=drains)
        if never_failed_at is None:
            try:
                g_never.push(c)
                g_never.flush(e + 1)
                g_never.poll_all()
                agg_checkpoint_drain_bytes(G(), g_never.h)
            except RuntimeError as err:
                assert "agg state table full" in str(err)
                never_failed_at = e
        if e >= 1:
            clean(execs, win(e - 1)[0])
            if never_failed_at is None:
                g_never.watermark(0, win(e - 1)[0])
        ready, live, cap = state_stats(G(), g.h)
        assert live <= 32 and ready <= 64 and cap == 64
        if ready > 48:
            assert compact(G(), g.h) == ready - live
            n_compactions += 1
    # the same stream without compaction does not fit: the test exercises
    # what it claims
    assert never_failed_at is not None and never_failed_at <= 4
    assert n_compactions >= 10
    g_never.close()
    # the watermark's DELETE frames of the last epoch
    for d, (lib, a) in zip(drains, execs):
        d.extend(agg_checkpoint_drain_bytes(lib, a.h))
    assert drains[0] == drains[1]
    g2, o2 = agg_pair(COUNT_SUM, 0, 64)
    agg_restore(G(), g2.h, bytes(drains[0]))
    agg_restore(oracle(), o2.h, bytes(drains[1]))
    assert state_stats(G(), g2.h) == (32, 32, 64)
    all4 = [(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)]
    for e in range(EPOCHS, EPOCHS + 3):
        agg_epoch(all4, [epoch_chunk(e)], e + 1)
        clean(all4, win(e - 1)[0])
        for a in (g, g2):
            if state_stats(G(), a.h)[0] > 48:
                compact(G(), a.h)
    close(all4)


# ----------------------------------------------------------------------
# 5. Nothing to do
# ----------------------------------------------------------------------


def test_nothing_to_do():
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9600)
    assert compact(G(), g.h) == 0  # an empty table
    assert state_stats(G(), g.h) == (0, 0, 64)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    assert compact(G(), g.h) == 0  # full, no dead group
    assert state_stats(G(), g.h) == (64, 64, 64)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 2)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 3)
    assert compact(G(), g.h) == 32
    assert compact(G(), g.h) == 0  # twice in a row
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 4)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 5)
    close(execs)


# ----------------------------------------------------------------------
# 6. Refusals: RW_E_INVAL, state untouched
# ----------------------------------------------------------------------


def refused(g, word):
    before = state_stats(G(), g.h)
    rc, got = compact_rc(G(), g.h)
    assert rc == RW_E_INVAL and got == 0
    assert word in G().last_error(), G().last_error()
    assert state_stats(G(), g.h) == before


@pytest.mark.parametrize("staged", [False, True], ids=["dirty", "ingest"])
def test_refused_before_the_flush(staged):
    # a push without a flush; in ingest mode the push only stages rows
    keys = agg_keys(64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9700)
    if staged:
        ingest_mode(G(), g.h, True)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    clean(execs, SPLIT)
    agg_epoch(execs, [], 2)
    c = all_keys_chunk(rng, surv, 100)
    g.push(c)
    refused(g, "staged" if staged else "dirty")
    o.push(c)
    out = agg_epoch(execs, [], 3)  # the missing step
    assert sum(op == "U+" for op, _ in out) == 32
    assert compact(G(), g.h) == 32
    fresh = [FRESH + i for i in range(32)]
    agg_epoch(execs, [all_keys_chunk(rng, surv + fresh, 200)], 4)
    close(execs)


def test_refused_with_undrained_minput():
    keys = np.array(agg_keys(64), np.int64)
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(MINMAX2, 2, 64, types=I3, stream_key=(2,))
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9710)
    e1 = [covering(rng, keys, 200), rng.integers(-500, 500, 200),
          np.arange(200)]  # 400 of the store's 512 rows: one per call
    minput_epoch(execs, [chunk(e1)], 1)
    clean(execs, SPLIT)  # the cleaned rows' deltas wait for a minput drain
    agg_epoch(execs, [], 2)
    refused(g, "undrained")
    minput_epoch(execs, [], 3)  # the missing step
    assert compact(G(), g.h) == 32
    idx = np.array([i for i in range(200) if e1[0][i] >= SPLIT][::2])
    minput_epoch(execs, [chunk([c[idx] for c in e1],
                               np.ones(len(idx), np.uint8)),
                         chunk([covering(rng, surv, 64),
                                rng.integers(-500, 500, 64),
                                np.arange(1000, 1064)])], 4)
    close(execs)


# ----------------------------------------------------------------------
# 7. Emit on window close
# ----------------------------------------------------------------------


def test_eowc_closed_windows_reclaimed():
    keys = agg_keys(64)
    closed = [k for k in keys if k < SPLIT]
    surv = [k for k in keys if k >= SPLIT]
    g, o = agg_pair(COUNT_SUM, 0, 64, emit_on_window_close=True)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9800)
    drains = [bytearray(), bytearray()]
    ep = lambda cs, e: agg_epoch(execs, cs, e, ordered=True, drains=drains)
    ep([all_keys_chunk(rng, keys)], 1)
    assert compact(G(), g.h) == 0  # mid-window groups are kept
    clean(execs, SPLIT)
    assert len(ep([], 2)) == 32
    assert state_stats(G(), g.h) == (64, 32, 64)
    assert compact(G(), g.h) == 32
    # mid-window survivors, 16 new windows and 16 closed ones that come back
    fresh = [FRESH + i for i in range(16)]
    assert ep([all_keys_chunk(rng, surv + fresh + closed[:16])], 3) == []
    assert state_stats(G(), g.h) == (64, 64, 64)
    clean(execs, FRESH + 8)
    out = ep([], 4)
    assert len(out) >= 32 + 8
    left = [k for k in surv + fresh if k >= FRESH + 8]  # still mid-window
    assert len(left) == 9
    assert compact(G(), g.h) == 64 - len(left)
    # a fresh EOWC executor restored from the drains holds its windows with
    # neither flag set: their row counts keep them through a compaction
    g2, o2 = agg_pair(COUNT_SUM, 0, 64, emit_on_window_close=True)
    agg_restore(G(), g2.h, bytes(drains[0]))
    agg_restore(oracle(), o2.h, bytes(drains[1]))
    assert compact(G(), g2.h) == 0
    all4 = [(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)]
    agg_epoch(all4, [all_keys_chunk(rng, left, 100)], 5, ordered=True)
    clean(all4, (1 << 63) - 1)
    out = agg_epoch(all4, [], 6, ordered=True)
    assert len(out) >= len(left) - 1
    close(all4)


# ----------------------------------------------------------------------
# 8. Vnode re-scope
# ----------------------------------------------------------------------


def test_vnode_rescope_reclaimed():
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(9900)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    for _, a in execs:
        a.update_vnode_bitmap(owned_bitmap(0))
    kept = [k for k in keys if expected_vnode([k]) % 2 == 0]
    assert 8 <= len(kept) <= 56
    assert compact(G(), g.h) == 64 - len(kept)
    assert state_stats(G(), g.h) == (len(kept), len(kept), 64)
    out = agg_epoch(execs, [all_keys_chunk(rng, kept)], 2)
    assert sorted(op for op, _ in out) == ["U+"] * len(kept) + ["U-"] * len(kept)
    fresh = [k for k in range(FRESH, FRESH + 400)
             if expected_vnode([k]) % 2 == 0][:64 - len(kept)]
    out = agg_epoch(execs, [all_keys_chunk(rng, kept + fresh)], 3)
    assert sum(op == "+" for op, _ in out) == len(fresh)
    close(execs)


# ----------------------------------------------------------------------
# 9. Varchar group keys: strings of dead groups
# ----------------------------------------------------------------------

VTYPES = [T_I64, T_VARCHAR, T_I64]
VCALLS = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 2, T_I64)]
VKEY = [0, 1]


def test_varchar_dead_strings():
    rng = np.random.default_rng(9950)
    rs = lambda: bytes(rng.integers(97, 123, int(rng.integers(8, 33)),
                                    dtype=np.uint8))
    both, two_live, only_dead = b"dead-and-live-" + rs(), b"two-live-" + rs(), \
        b"only-dead-" + rs()
    dead_pool = sorted({b"d-" + rs() for _ in range(220)})[:200]
    live_pool = sorted({b"l-" + rs() for _ in range(40)})[:30]
    DEAD_W, LIVE_W, LIVE_W2 = 10, 30, 40
    groups0 = ([(DEAD_W, both), (LIVE_W, both), (LIVE_W, two_live),
                (LIVE_W2, two_live), (DEAD_W, only_dead), (DEAD_W, b""),
                (LIVE_W, b""), (DEAD_W, None), (LIVE_W, None)]
               + [(DEAD_W, s) for s in dead_pool]
               + [(LIVE_W, s) for s in live_pool])

    def rows_for(groups, n):
        idx = covering(rng, np.arange(len(groups)), n)
        return [groups[int(i)] + (int(rng.integers(-1000, 1000)),)
                for i in idx]

    e0 = rows_for(groups0, 700)
    live_groups = [gk for gk in groups0 if gk[0] >= 20]
    # epoch 1: survivors change, some pre-compaction rows are retracted, a
    # dropped string comes back under a live window and under its old one
    back = [(LIVE_W, only_dead), (DEAD_W, only_dead), (LIVE_W2, dead_pool[0]),
            (LIVE_W2, b"brand-new")]
    old_live = [r for r in e0 if r[0] >= 20]
    retract = [old_live[int(i)] for i in rng.choice(len(old_live), 40,
                                                    replace=False)]
    e1 = rows_for(live_groups + back, 300)
    e2 = rows_for(live_groups + back, 300)
    ins = lambda rows: VChunk.from_rows(VTYPES, [OP_INSERT] * len(rows), rows)
    epochs = [[ins(e0[:350]), ins(e0[350:])],
              [VChunk.from_rows(VTYPES, [OP_DELETE] * 40, retract), ins(e1)],
              [ins(e2)]]
    wms = {0: (0, 20)}
    ref, _ = va.oracle_run(epochs, VKEY, calls=VCALLS, types=VTYPES,
                           watermarks=wms)
    lib = G()
    header, _align = va.header_consts()

    def mk():
        a = ffi.HashAgg(lib, VTYPES, VKEY, VCALLS, row_count_index=0,
                        state_capacity_hint=512)
        assert va.varlen_reserve(lib, a.h, 64, 16) == 0, lib.last_error()
        return a

    a = mk()
    run = va.Run()
    va.gpu_epoch(lib, a, epochs[0], 1, run, wms[0])
    assert run.outs[0] == ref.outs[0] and run.drains[0] == ref.drains[0]
    used0, acap0, n0, tcap0 = va.varlen_stats(lib, a.h)
    all0 = {s for _, s in groups0 if s is not None}
    assert n0 == len(all0) and acap0 > 64 and tcap0 > 32  # both grew
    n_dead = sum(1 for gk in groups0 if gk[0] < 20)
    assert state_stats(lib, a.h) == (len(groups0), len(live_groups), 512)
    assert compact(lib, a.h) == n_dead
    live_strs = {s for _, s in live_groups if s is not None}
    assert both in live_strs and two_live in live_strs and b"" in live_strs
    assert only_dead not in live_strs
    used, acap, n_str, tcap = va.varlen_stats(lib, a.h)
    assert n_str == len(live_strs)
    assert used == header + sum(len(s) for s in live_strs)
    assert (acap, tcap) == (acap0, tcap0)  # capacities stay
    assert used < used0
    assert compact(lib, a.h) == 0
    assert va.varlen_stats(lib, a.h) == (used, acap, n_str, tcap)

    va.gpu_epoch(lib, a, epochs[1], 2, run)
    assert run.outs[1] == ref.outs[1], "flush 1"
    assert run.drains[1] == ref.drains[1], "drain 1"
    assert any(op == "U-" for op, _ in run.outs[1])
    assert ("+", (LIVE_W, only_dead)) in [(op, r[:2]) for op, r in run.outs[1]]
    now = live_strs | {s for _, s in back}
    used1, _, n1, _ = va.varlen_stats(lib, a.h)
    assert n1 == len(now)
    assert used1 == header + sum(len(s) for s in now)
    # a fresh executor restored from the drains continues like this one
    b = mk()
    ffi.agg_restore(lib, b.h, run.drains[0] + run.drains[1])
    runb = va.Run()
    runb.outs, runb.drains = [None, None], [None, None]
    assert compact(lib, a.h) == 0
    va.gpu_epoch(lib, a, epochs[2], 3, run)
    va.gpu_epoch(lib, b, epochs[2], 3, runb)
    for r in (run, runb):
        assert r.outs[2] == ref.outs[2], "flush 2"
        assert r.drains[2] == ref.drains[2], "drain 2"
    a.close()
    b.close()
