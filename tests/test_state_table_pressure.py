"""State tables under collisions and at capacity: GPU vs the CPU oracle on
identical input, with every executor created at a tiny capacity hint and fed
keys aimed at chosen slots (rwtest/slots.py; the mirror is pinned to the
library's hash by test_slot_mirror.py).

HashAgg (hint 1, 2, 64) runs every apply kernel on an exactly full
open-addressed table whose probe cluster wraps from the last slot to slot 0;
HashJoin (hint 1, 4: two and eight chained buckets per side) makes every
chain walk reject records by full key behind a saturated bloom; GroupTopN
(hint 4: eight slots) and the DISTINCT dedup table get a wrapped cluster.
All values are i64 words and every comparison is exact: multisets of output
rows per epoch or push, spill drains byte for byte.

What the file catches was checked once with three deliberately wrong,
memory-safe builds of the library (never committed):
 - jhdr_key_eq returning true without comparing: 28 cases fail, every inner
   join case that walks a chain through jhdr_key_eq (multi-match second
   walk, wide records, append-only) and the cases that end in a small inner
   parity run; the non-inner probe filters keys inline and is not reached by
   this change.
 - table_find_or_insert probing `< cap_mask` steps instead of `<=`: 42 cases
   fail with "agg state table full", all of section A at one word per key
   and the agg error cases (the multi-word case stayed green: no key of its
   set happened to need the last probe step).
 - agg_clean_kernel writing SLOT_EMPTY into a cleaned slot:
   test_agg_watermark_clean_then_late_rows_full_table fails.
The suite before this file kept 50 to 1000 keys in tables of 2^15 to 2^21
slots (a few keys in 2^20 for the watermark cases), where two keys meet in
one bucket or one probe cluster about once in several hundred runs: none of
the three would have failed it.
"""
import ctypes
import functools

import numpy as np
import pytest

from rwtest import ffi, slots
from rwtest.ffi import (
    AGG_COUNT, AGG_COUNT_STAR, AGG_MAX, AGG_MIN, AGG_SUM, CMP_GE, CMP_LT,
    JOIN_FULL_OUTER, JOIN_INNER, JOIN_LEFT_ANTI, JOIN_LEFT_OUTER,
    JOIN_LEFT_SEMI, JOIN_RIGHT_ANTI, JOIN_RIGHT_OUTER, JOIN_RIGHT_SEMI,
    SIDE_LEFT, SIDE_RIGHT, T_I64, agg_checkpoint_drain_bytes,
    agg_dedup_drain_bytes, agg_dedup_restore, agg_minput_compact,
    agg_minput_drain_bytes, agg_restore, join_checkpoint_drain, join_compact,
    join_degree_drain, join_restore, oracle, rows_multiset, rows_ordered,
    topn_checkpoint_drain, topn_compact, topn_restore,
)
from rwtest.streams import join_mix_push, retract_mix, topn_mix_chunk
from test_gpu_parity import net_rows
from test_vnode_dispatch import expected_vnode

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I2, I3 = [T_I64, T_I64], [T_I64, T_I64, T_I64]
SIDES = (SIDE_LEFT, SIDE_RIGHT)
ROWS = 8192  # row_capacity_hint unless a case is about the row store


@functools.lru_cache(None)
def G():
    import risingwave_amd

    return ffi.Lib(risingwave_amd.lib_path())


def chunk(cols, ops=None, valids=None, vis=None):
    cols = [np.asarray(c, np.int64) for c in cols]
    n = len(cols[0])
    ops = np.zeros(n, np.uint8) if ops is None else ops
    if valids is None:
        valids = [np.ones(n, np.uint8) for _ in cols]
    return ffi.Chunk([T_I64] * len(cols), ops, cols, valids, vis)


def owned_bitmap(mod):
    bm = bytearray(32)
    for v in range(256):
        if v % 2 == mod:
            bm[v >> 3] |= 1 << (v & 7)
    return bytes(bm)


def first_diff(a, b):
    return next(((x, y) for x, y in zip(a, b) if x != y), None)


def covering(rng, keys, n):
    """n draws from keys, every key at least once, in random order."""
    ks = np.asarray(keys, np.int64)
    out = np.concatenate([ks, rng.choice(ks, n - len(ks))])
    rng.shuffle(out)
    return out


# ----------------------------------------------------------------------
# A. HashAgg at state_capacity_hint 1, 2 and 64: the table is exactly full
# ----------------------------------------------------------------------

SPLIT = 10**10  # half of the 64 keys sort below it, half above


@functools.lru_cache(None)
def agg_keys(hint):
    """`hint` distinct keys that fill the table. 64: 24 keys with home slot
    63 (their cluster wraps through slot 0), 8 with home slot 0 (displaced
    by it), the four extreme words and 28 more; 32 of the 64 sort below
    SPLIT. 2: both keys have home slot 1, so one wraps to slot 0."""
    if hint == 1:
        return (I64_MIN,)
    if hint == 2:
        return tuple(slots.keys_with_home(1, 2, 2, "agg"))
    edge = [0, -1, I64_MIN, I64_MAX]
    hi = 10**12
    k63 = (slots.keys_with_home(63, 64, 12, "agg", avoid=edge)
           + slots.keys_with_home(63, 64, 12, "agg", start=hi))
    k0 = (slots.keys_with_home(0, 64, 4, "agg", avoid=edge)
          + slots.keys_with_home(0, 64, 4, "agg", start=hi))
    rest = list(range(10**6, 10**6 + 13)) + list(range(2 * hi, 2 * hi + 15))
    keys = k63 + k0 + edge + rest
    assert len(set(keys)) == 64
    home = slots.agg_home(slots.hash_key([np.array(keys, np.int64)]), 64)
    assert int((home == 63).sum()) >= 24 and int((home == 0).sum()) >= 8
    assert sum(k < SPLIT for k in keys) == 32
    return tuple(keys)


def agg_pair(calls, rci, hint, types=I2, group_key=(0,), **kw):
    mk = lambda lib, **cap: ffi.HashAgg(lib, list(types), list(group_key),
                                        calls, rci, **kw, **cap)
    return mk(G(), state_capacity_hint=hint), mk(oracle())


def agg_epoch(execs, chunks, epoch, ordered=False, drains=None):
    """Push + flush one epoch on (lib, executor) pairs; outputs and
    checkpoint drains of all of them must equal the last one's (the
    oracle's). drains: optional list of per-executor bytearrays to extend."""
    outs, drs = [], []
    for lib, a in execs:
        for c in chunks:
            a.push(c)
        a.flush(epoch)
        got = a.poll_all()
        outs.append(rows_ordered(got) if ordered else rows_multiset(got))
        drs.append(agg_checkpoint_drain_bytes(lib, a.h))
    for i in range(len(execs) - 1):
        assert outs[i] == outs[-1], (
            f"epoch {epoch} executor {i}: {len(outs[i])} rows vs oracle "
            f"{len(outs[-1])}; first diff {first_diff(outs[i], outs[-1])}")
        assert drs[i] == drs[-1], (
            f"epoch {epoch} executor {i}: drain {len(drs[i])} vs "
            f"{len(drs[-1])} bytes")
    if drains is not None:
        for d, x in zip(drains, drs):
            d.extend(x)
    return outs[-1]


@pytest.mark.parametrize("hint", [1, 2, 64])
def test_agg_generic_retract_full_table(hint):
    # agg_apply_kernel, non-dense: 300-row chunks with deletes, NULL
    # arguments and a visibility mask. The 40 invisible rows of each chunk
    # carry keys that are not in the table: applying one would overflow it.
    keys = np.array(agg_keys(hint), np.int64)
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_COUNT, 1, T_I64),
             (AGG_SUM, 1, T_I64)]
    g, o = agg_pair(calls, 0, hint)
    rng = np.random.default_rng(100 + hint)
    live = []
    for epoch in (1, 2):
        chunks = []
        for ci in range(2):
            nv, n = 260, 300
            first = epoch == 1 and ci == 0
            kidx = covering(rng, np.arange(len(keys)), nv)
            vals = rng.integers(1, 1000, nv)
            valid = (rng.random(nv) > 0.25).astype(np.int64)
            ops_v = retract_mix(rng, live, [kidx, vals, valid],
                                0.0 if first else 0.3)
            pos = np.sort(rng.choice(n, nv, replace=False))
            k = 7 * 10**15 + rng.integers(0, 1000, n)  # foreign, invisible
            v = rng.integers(1, 1000, n)
            va = np.ones(n, np.uint8)
            ops = np.zeros(n, np.uint8)
            vis = np.zeros(n, np.uint8)
            k[pos], v[pos], va[pos] = keys[kidx], vals, valid
            ops[pos], vis[pos] = ops_v, 1
            chunks.append(chunk([k, v], ops, [np.ones(n, np.uint8), va], vis))
        agg_epoch([(G(), g), (oracle(), o)], chunks, epoch)
    g.close()
    o.close()


@functools.lru_cache(None)
def multiword_keys(kw):
    """64 distinct kw-word keys as (nullmask, words). 24 have home slot 63
    and 8 home slot 0; 14 have a NULL part, and 8 more are the non-NULL
    twins of NULL-part keys: the same words (a NULL part hashes and compares
    as 0), told apart by the null mask alone."""
    zeros = (0,) * (kw - 1)
    masks = (1,) if kw == 2 else (1, 2)  # which leading part is NULL

    def mk(home, n, prefix, nm, start=1):
        vs = slots.keys_with_home(home, 64, n, "agg", fixed_prefix=prefix,
                                  nullmask=nm, start=start)
        return [(nm, prefix + (v,)) for v in vs]

    keys = mk(63, 14, zeros, 0)
    for i, nm in enumerate(masks):
        keys += mk(63, 10 // len(masks), zeros, nm, start=1 + 10**6 * i)
    keys += mk(0, 4, zeros, 0) + mk(0, 4, zeros, masks[-1])
    nulls = [k for k in keys if k[0]]
    keys += [(0, w) for _, w in nulls[:8]]
    other = (5,) + (-1,) * (kw - 2)
    keys += [(0, other + (v,)) for v in range(100, 124)]
    assert len(keys) == 64 and len(set(keys)) == 64, len(set(keys))
    words = [np.array([w[i] for _, w in keys], np.int64) for i in range(kw)]
    nms = np.array([nm for nm, _ in keys], np.uint64)
    home = slots.agg_home(slots.hash_key(words, nms), 64)
    assert int((home == 63).sum()) >= 24 and int((home == 0).sum()) >= 8
    return tuple(keys)


@pytest.mark.parametrize("kw", [2, 3])
def test_agg_generic_multiword_full_table(kw):
    # agg_apply_kernel with KW 2 and 3 at 100 % load. Each epoch's first
    # chunk is all-valid inserts over the 50 non-NULL keys (the dense
    # instantiation); its second has every key, a key part NULL in the rows
    # of 14 of them (non-dense), so the null mask takes part in the hash and
    # in the slot compare. A NULL part carries a nonzero data word.
    keys = multiword_keys(kw)
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, kw, T_I64)]
    g, o = agg_pair(calls, 0, 64, types=[T_I64] * (kw + 1),
                    group_key=tuple(range(kw)))
    rng = np.random.default_rng(200 + kw)
    nonnull = [i for i, k in enumerate(keys) if not k[0]]
    for epoch in (1, 2):
        chunks = []
        for pick in (nonnull, list(range(64))):
            n = 300
            idx = covering(rng, pick, n)
            cols, valids = [], []
            for p in range(kw):
                w = np.array([keys[i][1][p] for i in idx], np.int64)
                va = np.array([not (keys[i][0] >> p) & 1 for i in idx],
                              np.uint8)
                w[va == 0] = 777
                cols.append(w)
                valids.append(va)
            cols.append(rng.integers(1, 1000, n))
            valids.append(np.ones(n, np.uint8))
            chunks.append(chunk(cols, None, valids))
        out = agg_epoch([(G(), g), (oracle(), o)], chunks, epoch)
        assert len([r for r in out if r[0] in ("+", "U+")]) == 64
    g.close()
    o.close()


DENSE_SHAPES = {
    # agg_apply_dense4_kernel<3> and <4>
    "dense4_3": ([(AGG_SUM, 1, T_I64), (AGG_MAX, 1, T_I64),
                  (AGG_COUNT_STAR, -1, T_I64)], 2),
    "dense4_4": ([(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 1, T_I64),
                  (AGG_MIN, 1, T_I64), (AGG_MAX, 1, T_I64)], 0),
    # the count-star span kernels
    "span_max_count": ([(AGG_MAX, 1, T_I64), (AGG_COUNT_STAR, -1, T_I64)], 1),
    "span_count_sum": ([(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 1, T_I64)], 0),
    "span_count": ([(AGG_COUNT_STAR, -1, T_I64)], 0),
}


@pytest.mark.parametrize("hint", [1, 2, 64])
@pytest.mark.parametrize("n", [1024, 1025])
@pytest.mark.parametrize("shape", list(DENSE_SHAPES))
def test_agg_dense_full_table(shape, n, hint):
    # the dense KW=1 kernels (all-valid inserts, 1024 rows is their
    # minimum, 1025 leaves a one-row tail tile). The first chunk fills the
    # table; the second chunk, sorted into runs, and the second epoch meet
    # only existing groups. Sums stay below 2^33.
    calls, rci = DENSE_SHAPES[shape]
    keys = agg_keys(hint)
    g, o = agg_pair(calls, rci, hint, append_only=True)
    rng = np.random.default_rng(300 + hint + n)
    for epoch in (1, 2):
        chunks = []
        for ci in range(2):
            k = covering(rng, keys, n)
            if ci:
                k = np.sort(k)
            chunks.append(chunk([k, rng.integers(1, 10**6, n)]))
        agg_epoch([(G(), g), (oracle(), o)], chunks, epoch)
    g.close()
    o.close()


COUNT_SUM = [(AGG_COUNT_STAR, -1, T_I64), (AGG_SUM, 1, T_I64)]


def all_keys_chunk(rng, keys, n=300):
    return chunk([covering(rng, keys, n), rng.integers(1, 1000, n)])


def test_agg_watermark_clean_then_late_rows_full_table():
    # agg_clean_kernel leaves cleaned groups READY so that linear probing is
    # undisturbed: after the 32 keys below SPLIT are cleaned out of the full,
    # wrapped cluster, late rows for them and rows for the 32 survivors that
    # sit behind their slots must still find their own slots.
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(401)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    for _, a in execs:
        a.watermark(0, SPLIT)
    agg_epoch(execs, [], 2)
    survivors = [k for k in keys if k >= SPLIT]
    agg_epoch(execs, [all_keys_chunk(rng, survivors)], 3)
    out = agg_epoch(execs, [all_keys_chunk(rng, keys)], 4)
    assert len(out) >= 64
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 5)
    g.close()
    o.close()


def test_agg_cleaned_slots_are_not_returned():
    # capacity contract: a cleaned group keeps its slot. After
    # all 64 groups are cleaned the same 64 keys come back, a 65th distinct
    # key still finds the table full.
    keys = [k for k in agg_keys(64) if k != I64_MAX] + [3 * 10**12]
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(402)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    for _, a in execs:
        a.watermark(0, 10**15)
    agg_epoch(execs, [], 2)
    out = agg_epoch(execs, [all_keys_chunk(rng, keys)], 3)
    assert len(out) == 64 and all(op == "+" for op, _ in out)
    with pytest.raises(RuntimeError, match="agg state table full"):
        g.push(chunk([[4 * 10**12], [1]]))
        g.flush(4)
    g.close()
    o.close()


def test_agg_vnode_rescope_full_table():
    # update_vnode_bitmap on a full table: half the vnodes go, then rows
    # arrive for the keys that stay
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(403)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1)
    for _, a in execs:
        a.update_vnode_bitmap(owned_bitmap(0))
    kept = [k for k in keys if expected_vnode([k]) % 2 == 0]
    assert 8 <= len(kept) <= 56
    agg_epoch(execs, [all_keys_chunk(rng, kept)], 2)
    agg_epoch(execs, [all_keys_chunk(rng, kept)], 3)
    g.close()
    o.close()


def test_agg_restore_full_table():
    # agg_restore_kernel at 100 % load: a fresh 64-slot executor restored
    # from the drains continues like the uninterrupted one and the oracle
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64)
    rng = np.random.default_rng(404)
    drains = [bytearray(), bytearray()]
    live = []
    for epoch in (1, 2):
        n = 300
        kidx = covering(rng, np.arange(64), n)
        vals = rng.integers(1, 1000, n)
        ops = retract_mix(rng, live, [kidx, vals], 0.0 if epoch == 1 else 0.3)
        c = chunk([np.array(keys, np.int64)[kidx], vals], ops)
        agg_epoch([(G(), g), (oracle(), o)], [c], epoch, drains=drains)
    g2, o2 = agg_pair(COUNT_SUM, 0, 64)
    agg_restore(G(), g2.h, bytes(drains[0]))
    agg_restore(oracle(), o2.h, bytes(drains[1]))
    execs = [(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)]
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 3)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 4)
    for _, a in execs:
        a.close()


def test_agg_eowc_full_table():
    # emit-on-window-close at hint 64: agg_eowc_close_kernel closes the 32
    # windows below SPLIT inside the full cluster, the same 64 keys arrive
    # again, then all but the last window close
    keys = agg_keys(64)
    g, o = agg_pair(COUNT_SUM, 0, 64, emit_on_window_close=True)
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(405)
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 1, ordered=True)
    for _, a in execs:
        a.watermark(0, SPLIT)
    out = agg_epoch(execs, [], 2, ordered=True)
    assert len(out) == 32
    agg_epoch(execs, [all_keys_chunk(rng, keys)], 3, ordered=True)
    for _, a in execs:
        a.watermark(0, I64_MAX)
    out = agg_epoch(execs, [], 4, ordered=True)
    assert len(out) >= 31
    g.close()
    o.close()


MINMAX = [(AGG_MIN, 1, T_I64), (AGG_COUNT_STAR, -1, T_I64)]


def minput_pair():
    return agg_pair(MINMAX, 1, 64, types=I3, stream_key=(2,))


def minput_epoch(execs, chunks, epoch):
    agg_epoch(execs, chunks, epoch)
    md = [agg_minput_drain_bytes(lib, a.h, 0) for lib, a in execs]
    assert md[0] == md[1], (f"epoch {epoch}: minput drain {len(md[0])} vs "
                            f"{len(md[1])} bytes")


def test_agg_minput_store_exactly_full_then_compact():
    # retractable min at hint 64: the materialised-input store holds
    # 8 * 64 = 512 rows, deletes do not free them. 300 inserts, 100 deletes
    # and 212 inserts reach row 512 exactly; agg_minput_compact drops the
    # 100 dead rows, 100 more inserts fill the store again.
    keys = np.array(agg_keys(64), np.int64)
    g, o = minput_pair()
    execs = [(G(), g), (oracle(), o)]
    rng = np.random.default_rng(406)

    def inserts(rid0, n):
        kidx = covering(rng, np.arange(64), n) if n >= 64 else \
            rng.integers(0, 64, n)
        return [keys[kidx], rng.integers(-500, 500, n),
                np.arange(rid0, rid0 + n)]

    def deletes(rows, n):
        pick = rng.choice(len(rows[0]), n, replace=False)
        return chunk([c[pick] for c in rows], np.ones(n, np.uint8))

    e1 = inserts(0, 300)
    minput_epoch(execs, [chunk(e1)], 1)
    e2 = inserts(300, 212)
    minput_epoch(execs, [deletes(e1, 100), chunk(e2)], 2)
    assert agg_minput_compact(G(), g.h) > 0
    assert agg_minput_compact(oracle(), o.h) == 0
    e3 = inserts(512, 100)
    minput_epoch(execs, [chunk(e3)], 3)
    minput_epoch(execs, [deletes(e2, 50), deletes(e3, 50)], 4)
    g.close()
    o.close()


# ----------------------------------------------------------------------
# B. HashJoin at state_capacity_hint 1 and 4: 2 and 8 buckets per side
# ----------------------------------------------------------------------

ALL_JOIN_TYPES = [JOIN_INNER, JOIN_LEFT_OUTER, JOIN_RIGHT_OUTER,
                  JOIN_FULL_OUTER, JOIN_LEFT_SEMI, JOIN_LEFT_ANTI,
                  JOIN_RIGHT_SEMI, JOIN_RIGHT_ANTI]


def join_pair(jt=JOIN_INNER, hint=1, rows=ROWS, tl=I2, tr=I2, n_gpu=1,
              net=None, **kw):
    """net: compare netted rows (net_rows). The oracle, like the reference,
    drops a +/- pair of one row where the two happen to be ADJACENT in its
    sequential output (eliminate_adjacent_noop_update, on every chunk it
    yields, inner joins included). That happens when a chunk deletes a row
    it inserted itself, so every stream with such chunks is compared
    netted, as test_join_noninner_random is; the inner cases whose chunks
    never do that compare the plain multiset."""
    kw.setdefault("key_l", [0])
    kw.setdefault("key_r", [0])
    kw.setdefault("pk_l", [1])
    kw.setdefault("pk_r", [1])
    js = [ffi.HashJoin(G(), jt, tl, tr, state_capacity_hint=hint,
                       row_capacity_hint=rows, **kw) for _ in range(n_gpu)]
    js.append(ffi.HashJoin(oracle(), jt, tl, tr, **kw))
    for j in js:
        j.net = jt != JOIN_INNER if net is None else net
    return tuple(js)


def join_push(execs, side, c, tag):
    """Push to every executor; each output multiset must equal the last
    one's (the oracle's). Returns the oracle's rows."""
    outs = []
    for j in execs:
        j.push(side, c)
        rows = rows_multiset(j.poll_all())
        outs.append(net_rows(rows) if j.net else rows)
    for i in range(len(execs) - 1):
        assert outs[i] == outs[-1], (
            f"{tag} side {side} executor {i}: {len(outs[i])} rows vs oracle "
            f"{len(outs[-1])}; first diff {first_diff(outs[i], outs[-1])}")
    return outs[-1]


def join_drains(pairs, tag, state=None, degs=None):
    """(lib, executor) pairs: per side, checkpoint and degree drains equal
    the last pair's byte for byte. state/degs: per-pair {side: bytearray}
    to extend."""
    for s in SIDES:
        ds = [join_checkpoint_drain(lib, j.h, s) for lib, j in pairs]
        dd = [join_degree_drain(lib, j.h, s) for lib, j in pairs]
        for i in range(len(pairs) - 1):
            assert ds[i] == ds[-1], (f"{tag} side {s} executor {i}: state "
                                     f"drain {len(ds[i])} vs {len(ds[-1])}")
            assert dd[i] == dd[-1], (f"{tag} side {s} executor {i}: degree "
                                     f"drain {len(dd[i])} vs {len(dd[-1])}")
        if state is not None:
            for i in range(len(pairs)):
                state[i][s].extend(ds[i])
                degs[i][s].extend(dd[i])


def bucket_report(keys, n_buckets, nullmask=0):
    """{bucket: (distinct keys, set of bloom bits)} by the mirror."""
    ks = np.array(sorted(set(int(k) for k in keys)), np.int64)
    h = slots.hash_key([ks], nullmask)
    home = slots.top_home(h, n_buckets)
    bit = slots.bloom_bit(h)
    return {b: (int((home == b).sum()),
                set(int(x) for x in bit[home == b]))
            for b in range(n_buckets)}


@functools.lru_cache(None)
def filler_keys():
    """256 keys for each of the two buckets of a hint-1 side."""
    return tuple(slots.keys_with_home(0, 2, 256, "top", start=1000)
                 + slots.keys_with_home(1, 2, 256, "top", start=1000))


@pytest.mark.parametrize("jt", ALL_JOIN_TYPES)
def test_join_all_types_two_buckets(jt):
    # hint 1: two buckets a side. Each side first takes 512 filler keys,
    # 256 aimed at each bucket, then the test_join_noninner_random stream
    # (120 keys, 30 % deletes, 512-row pushes, 8 pushes) runs through the
    # same two buckets: every chain walk of a probe, a delete-by-pk or a
    # degree update passes records of more than 200 other keys, and no
    # bloom bit is left clear to reject a probe early.
    fk = np.array(filler_keys(), np.int64)
    g, o = join_pair(jt, 1, net=True)
    rng = np.random.default_rng(2000 + jt)
    seen = {s: set(int(k) for k in fk) for s in SIDES}
    for s in SIDES:
        pk = np.arange(100_000 * (s + 1), 100_000 * (s + 1) + len(fk))
        join_push((g, o), s, chunk([fk, pk]), f"type {jt} filler")
    live = {SIDE_LEFT: [], SIDE_RIGHT: []}
    for i in range(8):
        side, c = join_mix_push(rng, live, i * 512, 512, 120, 0.3)
        seen[side].update(int(k) for k in c.cols[0][c.ops == ffi.OP_INSERT])
        join_push((g, o), side, c, f"type {jt} push {i}")
    for s in SIDES:
        for b, (n_keys, bits) in bucket_report(seen[s], 2).items():
            assert n_keys >= 200, (s, b, n_keys)
            assert len(bits) == 32, (s, b, sorted(bits))
    g.close()
    o.close()


def mixed_pushes(rng, n_pushes, n, draw, p_delete=0.25, pk_col=1):
    """(side, chunk) list over `draw(n)` columns with a unique pk put in
    column pk_col; deletes target earlier rows of the same side, rows of
    the same chunk included."""
    live = {SIDE_LEFT: [], SIDE_RIGHT: []}
    out = []
    for i in range(n_pushes):
        side = i % 2 if i < 2 else int(rng.integers(0, 2))
        cols = draw(n)
        cols.insert(pk_col, np.arange(i * n, (i + 1) * n))
        ops = retract_mix(rng, live[side], cols, p_delete)
        out.append((side, chunk(cols, ops)))
    return out


@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_nonequi_two_conjuncts(hint):
    # val_l < val_r + 10 AND val_l >= val_r - 40 over 40 keys: every match
    # is decided by the key filter first, then by both conjuncts
    rng = np.random.default_rng(2100 + hint)
    g, o = join_pair(JOIN_INNER, hint, tl=I3, tr=I3, net=True,
                     cond=(CMP_LT, 2, 5, 10), cond2=(CMP_GE, 2, 5, -40))
    draw = lambda n: [rng.integers(0, 40, n), rng.integers(0, 100, n)]
    total = 0
    for i, (side, c) in enumerate(mixed_pushes(rng, 8, 300, draw)):
        total += len(join_push((g, o), side, c, f"push {i}"))
    assert total > 500
    g.close()
    o.close()


@functools.lru_cache(None)
def null_twin_values():
    """12 values v for which the keys (NULL, v) and (0, v) share a bucket in
    an 8-bucket table (so in a 2-bucket one too)."""
    cand = np.arange(1, 1 << 16, dtype=np.int64)
    zero = np.zeros(len(cand), np.int64)
    hn = slots.top_home(slots.hash_key([zero, cand], 1), 8)
    hz = slots.top_home(slots.hash_key([zero, cand], 0), 8)
    vs = [int(v) for v in cand[hn == hz][:12]]
    assert len(vs) == 12
    return tuple(vs)


@pytest.mark.parametrize("null_safe", [0, 1])
@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_null_keys_share_bucket_with_zero(hint, null_safe):
    # two-word key (a, b): rows with a NULL and rows with a literally 0 sit
    # in the same bucket and differ in the record's valid bit alone. With
    # null_safe NULL matches NULL, without it NULL matches nothing; 0
    # matches 0 either way and never a NULL.
    vs = np.array(null_twin_values(), np.int64)
    g, o = join_pair(JOIN_INNER, hint, tl=I3, tr=I3, key_l=[0, 1],
                     key_r=[0, 1], pk_l=[2], pk_r=[2],
                     null_safe=[null_safe, 0])
    rng = np.random.default_rng(2200 + hint)
    made = {s: [] for s in SIDES}

    def rows(side, pk0, n=96):
        b = rng.choice(vs, n)
        a_null = rng.random(n) < 0.5
        a = np.where(a_null | (rng.random(n) < 0.7), 0, 9)
        pk = np.arange(pk0, pk0 + n)
        va = (~a_null).astype(np.uint8)
        made[side].append((a, b, pk, va))
        n1 = np.ones(n, np.uint8)
        return chunk([a, b, pk], None, [va, n1, n1])

    def delete_half(side, which):
        a, b, pk, va = (x[::2] for x in made[side][which])
        n1 = np.ones(len(a), np.uint8)
        return chunk([a, b, pk], np.ones(len(a), np.uint8), [va, n1, n1])

    pushes = [(SIDE_LEFT, rows(SIDE_LEFT, 0)),
              (SIDE_RIGHT, rows(SIDE_RIGHT, 1000)),
              (SIDE_LEFT, rows(SIDE_LEFT, 2000)),
              (SIDE_RIGHT, delete_half(SIDE_RIGHT, 0)),
              (SIDE_LEFT, delete_half(SIDE_LEFT, 0)),
              (SIDE_RIGHT, rows(SIDE_RIGHT, 3000))]
    total = 0
    for i, (side, c) in enumerate(pushes):
        out = join_push((g, o), side, c, f"push {i}")
        total += len(out)
        for _, r in out:  # a NULL never meets a 0
            assert (r[0] is None) == (r[3] is None)
            assert null_safe or r[0] is not None
    assert total > 100
    g.close()
    o.close()


@pytest.mark.parametrize("kw", [2, 3])
@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_multiword_keys(hint, kw):
    rng = np.random.default_rng(2300 + 10 * hint + kw)
    t = [T_I64] * (kw + 1)
    keys = list(range(kw))
    g, o = join_pair(JOIN_INNER, hint, tl=t, tr=t, key_l=keys, key_r=keys,
                     pk_l=[kw], pk_r=[kw], net=True)
    draw = lambda n: [rng.integers(0, 6 - p, n) for p in range(kw)]
    total = 0
    for i, (side, c) in enumerate(mixed_pushes(rng, 8, 300, draw, pk_col=kw)):
        total += len(join_push((g, o), side, c, f"push {i}"))
    assert total > 500
    g.close()
    o.close()


@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_append_only(hint):
    # the append-only inner path: keys unique within a side, half of them
    # shared across sides, 300-row insert batches through 2 or 8 buckets
    g, o = join_pair(JOIN_INNER, hint, tl=I3, tr=I3, key_l=[0, 1],
                     key_r=[0, 1], pk_l=[], pk_r=[], null_safe=[0, 0],
                     append_only=True)

    def batch(k0, base):
        return chunk([k0, k0 * 2 + 1, np.arange(base, base + len(k0))])

    a = np.arange(100, 700, dtype=np.int64)
    b = np.arange(400, 1000, dtype=np.int64)
    pushes = [(SIDE_LEFT, batch(a[::2], 10_000)),
              (SIDE_RIGHT, batch(b[::2], 20_000)),
              (SIDE_LEFT, batch(a[1::2], 30_000)),
              (SIDE_RIGHT, batch(b[1::2], 40_000))]
    total = 0
    for i, (side, c) in enumerate(pushes):
        total += len(join_push((g, o), side, c, f"push {i}"))
    assert total == 300
    g.close()
    o.close()


@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_ingest_mode(hint):
    # rw_hash_join_ingest_mode(h, 1) merges same-side runs into one launch:
    # equal to chunk-at-a-time and to the oracle, outputs and left drains
    g_epoch, g_plain, o = join_pair(JOIN_INNER, hint, n_gpu=2)
    L = G().lib
    L.rw_hash_join_ingest_mode.restype = ctypes.c_int
    L.rw_hash_join_ingest_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.rw_hash_join_ingest_mode(g_epoch.h, 1) == 0, G().last_error()
    rng = np.random.default_rng(2400 + hint)
    live = {SIDE_LEFT: [], SIDE_RIGHT: []}
    pk = 0
    for epoch in range(2):
        for side in (SIDE_LEFT, SIDE_LEFT, SIDE_RIGHT, SIDE_RIGHT, SIDE_LEFT):
            _, c = join_mix_push(rng, live, pk, 512, 120, 0.25, side=side)
            pk += 512
            for x in (g_epoch, g_plain, o):
                x.push(side, c)
        outs = []
        for x in (g_epoch, g_plain, o):
            x.flush(epoch + 1)
            outs.append(net_rows(rows_multiset(x.poll_all())))
        assert outs[0] == outs[2], f"epoch {epoch}: ingest mode vs oracle"
        assert outs[1] == outs[2], f"epoch {epoch}: per chunk vs oracle"
        join_drains([(G(), g_epoch), (G(), g_plain), (oracle(), o)],
                    f"epoch {epoch}")
    for x in (g_epoch, g_plain, o):
        x.close()


@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_wide_records(hint):
    # a 7-column right side: 96-byte records, past the register-resident
    # walk, so the probe's field-by-field walk, its second multi-match walk
    # and the delete walk all filter by jhdr_key_eq inside mixed buckets
    tr = [T_I64] * 7
    g, o = join_pair(JOIN_INNER, hint, tl=I2, tr=tr)
    rng = np.random.default_rng(2500 + hint)
    n = 300

    def right(keys, pk0, op=ffi.OP_INSERT):
        pk = np.arange(pk0, pk0 + len(keys))
        cols = [keys, pk] + [pk * 10 + c for c in range(2, 7)]
        valids = [np.ones(len(keys), np.uint8) for _ in tr]
        valids[4] = (pk % 3 != 0).astype(np.uint8)
        return chunk(cols, np.full(len(keys), op, np.uint8), valids)

    def left(keys, pk0, op=ffi.OP_INSERT):
        pk = np.arange(pk0, pk0 + len(keys))
        return chunk([keys, pk], np.full(len(keys), op, np.uint8))

    uniq = np.arange(n, dtype=np.int64)
    rep = np.concatenate([np.repeat(np.arange(1000, 1050), 3),
                          np.arange(2000, 2150)]).astype(np.int64)
    l1 = np.concatenate([uniq[::2], np.arange(5000, 5150)])
    l2 = np.concatenate([np.arange(1000, 1050), np.arange(6000, 6250)])
    pushes = [(SIDE_RIGHT, right(uniq, 0)),
              (SIDE_LEFT, left(l1, 100_000)),
              (SIDE_RIGHT, right(rep, n)),
              (SIDE_LEFT, left(l2, 200_000)),
              (SIDE_LEFT, left(l1[:100], 100_000, ffi.OP_DELETE)),
              (SIDE_RIGHT, right(uniq[150:250], 150, ffi.OP_DELETE)),
              (SIDE_LEFT, left(rng.integers(0, n, n), 300_000))]
    counts = []
    for i, (side, c) in enumerate(pushes):
        counts.append(len(join_push((g, o), side, c, f"push {i}")))
    assert counts[:6] == [0, 150, 0, 150, 100, 25], counts
    join_drains([(G(), g), (oracle(), o)], "end")
    g.close()
    o.close()


@pytest.mark.parametrize("hint", [1, 4])
def test_join_inner_delete_of_same_chunk_insert(hint):
    # mixed-op chunks in which a delete targets a row inserted earlier in
    # the SAME chunk (the conflict-segment pre-pass), inside shared buckets
    g, o = join_pair(JOIN_INNER, hint, net=True)
    rng = np.random.default_rng(2600 + hint)
    pk = 0
    for i in range(6):
        side = i % 2
        n = 150
        keys = rng.integers(0, 30, n)
        pks = np.arange(pk, pk + n)
        pk += n
        gone = rng.choice(n, 60, replace=False)
        c = chunk([np.concatenate([keys, keys[gone]]),
                   np.concatenate([pks, pks[gone]])],
                  np.concatenate([np.zeros(n, np.uint8),
                                  np.ones(60, np.uint8)]))
        join_push((g, o), side, c, f"push {i}")
    join_drains([(G(), g), (oracle(), o)], "end")
    g.close()
    o.close()


@pytest.mark.parametrize("hint", [1, 4])
def test_join_bloom_false_positive_and_reject(hint):
    # an unsaturated bloom: the right side holds 16 keys. By the mirror,
    # one absent probe key has its bloom bit SET in its bucket (a false
    # positive: the probe walks the chain and must match nothing) and
    # another has it CLEAR (rejected at the bucket word).
    nb = 2 * hint
    build = np.arange(500, 516, dtype=np.int64)
    rep = bucket_report(build, nb)
    fp = clear = None
    for k in range(10_000, 20_000):
        h = slots.hash_key([np.int64(k)])
        b = int(slots.top_home(h, nb)[0])
        bit = int(slots.bloom_bit(h)[0])
        if rep[b][0] and bit in rep[b][1] and fp is None:
            fp = (k, b, bit)
        if rep[b][0] and bit not in rep[b][1] and clear is None:
            clear = (k, b, bit)
        if fp and clear:
            break
    assert fp and fp[2] in rep[fp[1]][1], "no key with its bloom bit set"
    assert clear and clear[2] not in rep[clear[1]][1], "no key with it clear"
    for jt in (JOIN_INNER, JOIN_LEFT_OUTER):
        g, o = join_pair(jt, hint)
        join_push((g, o), SIDE_RIGHT, chunk([build, np.arange(16)]), "build")
        probe = np.array([fp[0], clear[0], 500, 515, fp[0], clear[0]])
        out = join_push((g, o), SIDE_LEFT, chunk([probe, np.arange(100, 106)]),
                        f"type {jt} probe")
        matched = [r for _, r in out if r[2] is not None]
        assert sorted(r[0] for r in matched) == [500, 515]
        g.close()
        o.close()


@pytest.mark.parametrize("jt", [JOIN_INNER, JOIN_LEFT_OUTER, JOIN_FULL_OUTER,
                                JOIN_LEFT_SEMI])
def test_join_spill_two_buckets(jt):
    # test_join_degree_spill_parity's stream at hint 1: state and degree
    # drains byte-equal to the oracle's, per epoch
    rng = np.random.default_rng(2700 + jt)
    g, o = join_pair(jt, 1, net=True)
    live = {SIDE_LEFT: [], SIDE_RIGHT: []}
    pk = 0
    for epoch in range(4):
        for side in SIDES:
            _, c = join_mix_push(rng, live, pk, 768, 60, 0.3, side=side)
            pk += 768
            join_push((g, o), side, c, f"type {jt} epoch {epoch}")
        join_drains([(G(), g), (oracle(), o)], f"type {jt} epoch {epoch}")
    g.close()
    o.close()


def stream_epoch(execs, rng, live, pk, n_pushes=4, n=256, key_space=60,
                 p_delete=0.3, tag=""):
    for i in range(n_pushes):
        side, c = join_mix_push(rng, live, pk[0], n, key_space, p_delete,
                                side=i % 2)
        pk[0] += n
        join_push(execs, side, c, f"{tag} push {i}")


@pytest.mark.parametrize("jt", [JOIN_INNER, JOIN_LEFT_OUTER])
def test_join_key_watermark_clean_two_buckets(jt):
    # join_clean_kernel kills the rows below the watermark inside buckets
    # that also hold surviving keys; the stream goes on above it
    g, o = join_pair(jt, 1, net=True, wm_jk=[(0, True)])
    rng = np.random.default_rng(2800 + jt)
    live, pk = {SIDE_LEFT: [], SIDE_RIGHT: []}, [0]
    pairs = [(G(), g), (oracle(), o)]
    stream_epoch((g, o), rng, live, pk, tag="epoch 0")
    join_drains(pairs, "epoch 0")
    wms = [[j.watermark(s, 0, 30) for s in SIDES] for j in (g, o)]
    assert wms[0] == wms[1]
    join_drains(pairs, "clean")
    # the cleaned rows are gone, so later deletes leave them alone; the
    # stream goes on over keys 30..59 as key index 0..29
    for s in SIDES:
        live[s] = [(k - 30, p) for k, p in live[s] if k >= 30]
    above = np.arange(30, 60)
    for epoch in (1, 2):
        for i in range(4):
            side, c = join_mix_push(rng, live, pk[0], 256, 30, 0.3,
                                    side=i % 2, key_map=above)
            pk[0] += 256
            join_push((g, o), side, c, f"epoch {epoch} push {i}")
        join_drains(pairs, f"epoch {epoch}")
    g.close()
    o.close()


def test_join_inequality_clean_two_buckets():
    # val_l >= val_r with the inequality-pair watermark cleaning the left
    # side's rows below min(watermarks) out of mixed buckets
    g, o = join_pair(JOIN_INNER, 1, tl=I3, tr=I3, cond=(CMP_GE, 2, 5),
                     wm_ineq=((2, 2, True, True),))
    rng = np.random.default_rng(2900)
    pairs = [(G(), g), (oracle(), o)]
    pk = [0]

    def push_inserts(side, lo, hi, tag, n=256):
        c = chunk([rng.integers(0, 40, n), np.arange(pk[0], pk[0] + n),
                   rng.integers(lo, hi, n)])
        pk[0] += n
        return join_push((g, o), side, c, tag)

    for i in range(4):
        push_inserts(i % 2, 0, 100, f"epoch 0 push {i}")
    join_drains(pairs, "epoch 0")
    wms = [[j.watermark(SIDE_LEFT, 2, 60), j.watermark(SIDE_RIGHT, 2, 40)]
           for j in (g, o)]
    assert wms[0] == wms[1] and wms[0][1], wms
    join_drains(pairs, "clean")
    total = 0
    for i in range(4):
        total += len(push_inserts(i % 2, 40, 100, f"epoch 1 push {i}"))
    assert total > 0
    join_drains(pairs, "epoch 1")
    g.close()
    o.close()


@pytest.mark.parametrize("jt", [JOIN_INNER, JOIN_LEFT_OUTER])
def test_join_compact_two_buckets(jt):
    # join_compact relinks both sides' live records into the two buckets
    g, o = join_pair(jt, 1, net=True)
    rng = np.random.default_rng(3000 + jt)
    live, pk = {SIDE_LEFT: [], SIDE_RIGHT: []}, [0]
    pairs = [(G(), g), (oracle(), o)]
    for epoch in range(3):
        stream_epoch((g, o), rng, live, pk, tag=f"epoch {epoch}")
        join_drains(pairs, f"epoch {epoch}")
        for s in SIDES:
            freed = join_compact(G(), g.h, s)
            assert freed > 0, f"epoch {epoch} side {s}: nothing reclaimed"
            assert join_compact(oracle(), o.h, s) == 0
    g.close()
    o.close()


@pytest.mark.parametrize("jt", [JOIN_LEFT_OUTER, JOIN_INNER])
def test_join_restore_two_buckets(jt):
    # drain, then join_restore (with degrees) into a fresh hint-1 executor:
    # it continues like the uninterrupted one and like the oracle
    g, o = join_pair(jt, 1, net=True)
    rng = np.random.default_rng(3100 + jt)
    live, pk = {SIDE_LEFT: [], SIDE_RIGHT: []}, [0]
    state = [{s: bytearray() for s in SIDES} for _ in range(2)]
    degs = [{s: bytearray() for s in SIDES} for _ in range(2)]
    for epoch in range(2):
        stream_epoch((g, o), rng, live, pk, tag=f"epoch {epoch}")
        join_drains([(G(), g), (oracle(), o)], f"epoch {epoch}", state, degs)
    g2, o2 = join_pair(jt, 1, net=True)
    for s in SIDES:
        join_restore(G(), g2.h, s, bytes(state[0][s]), bytes(degs[0][s]))
        join_restore(oracle(), o2.h, s, bytes(state[1][s]), bytes(degs[1][s]))
    for epoch in (2, 3):
        stream_epoch((g, g2, o2, o), rng, live, pk, tag=f"epoch {epoch}")
        join_drains([(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)],
                    f"epoch {epoch}")
    for j in (g, g2, o, o2):
        j.close()


@pytest.mark.parametrize("jt", [JOIN_INNER, JOIN_LEFT_OUTER])
def test_join_vnode_rescope_two_buckets(jt):
    # update_vnode_bitmap drops the rows of half the vnodes out of both
    # buckets; inserts go on for every key
    g, o = join_pair(jt, 1, net=True)
    rng = np.random.default_rng(3200 + jt)
    live, pk = {SIDE_LEFT: [], SIDE_RIGHT: []}, [0]
    pairs = [(G(), g), (oracle(), o)]
    stream_epoch((g, o), rng, live, pk, tag="epoch 0")
    join_drains(pairs, "epoch 0")
    for j in (g, o):
        j.update_vnode_bitmap(owned_bitmap(1))
    for epoch in (1, 2):
        for i in range(4):
            c = chunk([rng.integers(0, 60, 256),
                       np.arange(pk[0], pk[0] + 256)])
            pk[0] += 256
            join_push((g, o), i % 2, c, f"epoch {epoch} push {i}")
        join_drains(pairs, f"epoch {epoch}")
    g.close()
    o.close()


N_ROWS = 2048


@pytest.mark.parametrize("path", ["preassigned", "jown"])
def test_join_row_store_exactly_full_then_compact(path):
    # row_capacity_hint = N = 2048. Exactly N records fit. Deletes do not
    # free records: after N/2 rows are deleted N/2 more inserts find the row
    # store full; after join_compact the same inserts fit and parity holds.
    # preassigned: the inner probe reserves a batch's records with one
    # cursor bump (jprobe_setup_kernel), all-insert chunks. jown: the other
    # types reserve per inserting lane (jown_insert), mixed-op chunks.
    inner = path == "preassigned"
    jt = JOIN_INNER if inner else JOIN_LEFT_OUTER
    g, g2, o = join_pair(jt, 1, rows=N_ROWS, n_gpu=2)
    rng = np.random.default_rng(3300 + inner)
    N = N_ROWS
    keys = rng.integers(0, 200, N + 1024)
    pks = np.arange(N + 1024)
    every = (g, g2, o)

    def rows(sel, op):
        return chunk([keys[sel], pks[sel]], np.full(len(keys[sel]), op,
                                                    np.uint8))

    join_push(every, SIDE_RIGHT, chunk([np.arange(0, 200, 2),
                                        np.arange(10**6, 10**6 + 100)]),
              "right")
    if inner:
        join_push(every, SIDE_LEFT, rows(slice(0, 1024), 0), "fill 0")
        join_push(every, SIDE_LEFT, rows(slice(1024, N), 0), "fill 1")
        join_push(every, SIDE_LEFT, rows(slice(0, 1024), 1), "delete")
        more = rows(slice(N, N + 1024), 0)
    else:
        join_push(every, SIDE_LEFT, rows(slice(0, 1024), 0), "fill 0")
        c = chunk([np.concatenate([keys[1024:2024], keys[:24]]),
                   np.concatenate([pks[1024:2024], pks[:24]])],
                  np.concatenate([np.zeros(1000, np.uint8),
                                  np.ones(24, np.uint8)]))
        join_push(every, SIDE_LEFT, c, "fill 1 (mixed)")
        join_push(every, SIDE_LEFT, rows(slice(2024, N), 0), "fill 2")
        join_push(every, SIDE_LEFT, rows(slice(24, 1024), 1), "delete")
        more = chunk([np.concatenate([keys[1024:1029], keys[N:N + 1020]]),
                      np.concatenate([pks[1024:1029], pks[N:N + 1020]])],
                     np.concatenate([np.ones(5, np.uint8),
                                     np.zeros(1020, np.uint8)]))
    with pytest.raises(RuntimeError, match="row store full"):
        g.push(SIDE_LEFT, more)
    g.close()
    pairs = [(G(), g2), (oracle(), o)]
    join_drains(pairs, "before compact")
    assert join_compact(G(), g2.h, SIDE_LEFT) > 0
    join_push((g2, o), SIDE_LEFT, more, "after compact")
    probe = chunk([np.arange(0, 200), np.arange(2 * 10**6, 2 * 10**6 + 200)])
    assert len(join_push((g2, o), SIDE_RIGHT, probe, "probe")) > 1000
    join_drains(pairs, "end")
    g2.close()
    o.close()


# ----------------------------------------------------------------------
# C. GroupTopN at state_capacity_hint 4: eight slots
# ----------------------------------------------------------------------


@functools.lru_cache(None)
def topn_groups():
    """Eight group keys that fill the table; five have home slot 7, so the
    cluster wraps through slot 0."""
    ks = slots.keys_with_home(7, 8, 5, "top") + [0, -1, I64_MIN]
    assert len(set(ks)) == 8
    home = slots.top_home(slots.hash_key([np.array(ks, np.int64)]), 8)
    assert int((home == 7).sum()) >= 4
    return tuple(ks)


def topn_pair(n_gpu=1, rows=ROWS, **kw):
    mk = lambda lib, **cap: ffi.GroupTopN(lib, I3, [0], **kw, **cap)
    gs = [mk(G(), state_capacity_hint=4, row_capacity_hint=rows)
          for _ in range(n_gpu)]
    return (*gs, mk(oracle()))


def topn_push(execs, c, tag):
    outs = []
    for t in execs:
        t.push(c)
        outs.append(rows_multiset(t.poll_all()))
    for i in range(len(execs) - 1):
        assert outs[i] == outs[-1], (
            f"{tag} executor {i}: {len(outs[i])} rows vs oracle "
            f"{len(outs[-1])}; first diff {first_diff(outs[i], outs[-1])}")
    return outs[-1]


def topn_drains(pairs, tag, keep=None):
    ds = [topn_checkpoint_drain(lib, t.h) for lib, t in pairs]
    for i in range(len(pairs) - 1):
        assert ds[i] == ds[-1], (f"{tag} executor {i}: drain {len(ds[i])} "
                                 f"vs {len(ds[-1])} bytes")
    if keep is not None:
        for k, d in zip(keep, ds):
            k.extend(d)


TOPN_RANDOM = dict(order_by=[(1, True)], rest=[(2, False)], offset=1, limit=3)
TOPN_TIES = dict(order_by=[(1, False)], rest=[(2, False)], offset=0, limit=3,
                 with_ties=True)
# (executor arguments, the stream's order values / pks / delete share)
TOPN_STREAMS = {"random": (TOPN_RANDOM, (200, 10**6, 0.35)),
                "with_ties": (TOPN_TIES, (6, 10**7, 0.4))}


@pytest.mark.parametrize("stream", list(TOPN_STREAMS))
def test_topn_streams_eight_slots(stream):
    # the test_topn_random and WITH TIES streams over the eight groups, a
    # byte-compared drain every second push
    kw, (ords, pks, p_del) = TOPN_STREAMS[stream]
    g, o = topn_pair(**kw)
    rng = np.random.default_rng(4000 + len(stream))
    live = []
    for i in range(10 if stream == "random" else 8):
        c = topn_mix_chunk(rng, live, 512, 8, ords, pks, p_del,
                           key_map=topn_groups())
        topn_push((g, o), c, f"push {i}")
        if i % 2:
            topn_drains([(G(), g), (oracle(), o)], f"push {i}")
    g.close()
    o.close()


@pytest.mark.parametrize("stream", list(TOPN_STREAMS))
def test_topn_compact_and_restore_eight_slots(stream):
    # topn_compact relinks the live records under the wrapped cluster;
    # topn_restore rebuilds it in a fresh eight-slot executor
    kw, (ords, pks, p_del) = TOPN_STREAMS[stream]
    g, o = topn_pair(**kw)
    rng = np.random.default_rng(4100 + len(stream))
    live = []
    keep = [bytearray(), bytearray()]
    mix = lambda: topn_mix_chunk(rng, live, 256, 8, ords, pks, p_del,
                                 key_map=topn_groups())
    freed = 0
    for i in range(4):
        topn_push((g, o), mix(), f"push {i}")
        topn_drains([(G(), g), (oracle(), o)], f"push {i}", keep)
        freed += topn_compact(G(), g.h)
        assert topn_compact(oracle(), o.h) == 0
    assert freed > 0, "compaction reclaimed nothing despite deletes"
    g2, o2 = topn_pair(**kw)
    topn_restore(G(), g2.h, bytes(keep[0]))
    topn_restore(oracle(), o2.h, bytes(keep[1]))
    for i in range(4, 8):
        topn_push((g, g2, o2, o), mix(), f"push {i}")
        topn_drains([(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)],
                    f"push {i}")
    for t in (g, g2, o, o2):
        t.close()


def test_topn_watermark_eight_slots():
    # rw_group_top_n_watermark cleans the four smallest groups out of the
    # wrapped cluster; the stream goes on over the four that stay
    groups = sorted(topn_groups())
    kw, (ords, pks, p_del) = TOPN_STREAMS["random"]
    g, o = topn_pair(**kw)
    rng = np.random.default_rng(4200)
    live = []
    pairs = [(G(), g), (oracle(), o)]
    for i in range(3):
        c = topn_mix_chunk(rng, live, 256, 8, ords, pks, p_del,
                           key_map=groups)
        topn_push((g, o), c, f"push {i}")
    topn_drains(pairs, "before")
    assert [t.watermark(0, groups[4]) for t in (g, o)] == [1, 1]
    topn_drains(pairs, "clean")
    # groups[4:] stay: index i of the four-group stream is groups[4 + i]
    live = [(gi - 4, v, p) for gi, v, p in live if gi >= 4]
    for i in range(3, 7):
        c = topn_mix_chunk(rng, live, 256, 4, ords, pks, p_del,
                           key_map=groups[4:])
        topn_push((g, o), c, f"push {i}")
    topn_drains(pairs, "after")
    g.close()
    o.close()


# ----------------------------------------------------------------------
# D. The DISTINCT dedup table: a wrapped cluster in its 65 536 slots
# ----------------------------------------------------------------------


@functools.lru_cache(None)
def dedup_pairs():
    """48 (group, datum) pairs: 40 with home slot 65 535 of the dedup
    table, 8 with home slot 0."""
    cap = 1 << 16
    out = []
    for grp in range(4):
        out += [(grp, d) for d in slots.keys_with_home(
            cap - 1, cap, 10, "top", fixed_prefix=(grp,))]
    for grp in (4, 5):
        out += [(grp, d) for d in slots.keys_with_home(
            0, cap, 4, "top", fixed_prefix=(grp,))]
    gs = np.array([p[0] for p in out], np.int64)
    ds = np.array([p[1] for p in out], np.int64)
    home = slots.top_home(slots.hash_key([gs, ds]), cap)
    assert int((home == cap - 1).sum()) == 40 and int((home == 0).sum()) == 8
    return tuple(out)


def test_distinct_dedup_wrapped_cluster():
    # count(distinct) / sum(distinct) over pairs that all probe from the
    # last slot of the dedup table (its floor of 65 536 slots, reached with
    # a small agg hint) on through slot 0. Per epoch: outputs, the dedup
    # drain and the intermediate drain; then a restore that continues.
    pairs = np.array(dedup_pairs(), np.int64)
    calls = [(AGG_COUNT_STAR, -1, T_I64), (AGG_COUNT, 1, T_I64, 1),
             (AGG_SUM, 1, T_I64, 1)]
    g, o = agg_pair(calls, 0, 64)
    rng = np.random.default_rng(5000)
    live = []
    keep = [bytearray(), bytearray()]
    inter = [bytearray(), bytearray()]

    def epoch_chunk(first):
        n = 400
        idx = covering(rng, np.arange(len(pairs)), n)
        ops = retract_mix(rng, live, [idx], 0.0 if first else 0.4)
        return chunk([pairs[idx, 0], pairs[idx, 1]], ops)

    def run(execs, epoch, c):
        agg_epoch(execs, [c], epoch, drains=inter if len(execs) == 2 else None)
        ds = [agg_dedup_drain_bytes(lib, a.h, 0) for lib, a in execs]
        for i in range(len(execs) - 1):
            assert ds[i] == ds[-1], (f"epoch {epoch} executor {i}: dedup "
                                     f"drain {len(ds[i])} vs {len(ds[-1])}")
        return ds

    for epoch in (1, 2, 3):
        ds = run([(G(), g), (oracle(), o)], epoch, epoch_chunk(epoch == 1))
        keep[0].extend(ds[0])
        keep[1].extend(ds[1])
    g2, o2 = agg_pair(calls, 0, 64)
    for lib, a, k, it in ((G(), g2, keep[0], inter[0]),
                          (oracle(), o2, keep[1], inter[1])):
        agg_dedup_restore(lib, a.h, 0, bytes(k))
        agg_restore(lib, a.h, bytes(it))
    execs = [(G(), g), (G(), g2), (oracle(), o2), (oracle(), o)]
    for epoch in (4, 5):
        run(execs, epoch, epoch_chunk(False))
    for _, a in execs:
        a.close()


# ----------------------------------------------------------------------
# E. The documented error returns of a full table. Each runs once; what the
# failed handle does afterwards is not pinned, a fresh executor must work.
# ----------------------------------------------------------------------


def small_agg_parity():
    g, o = agg_pair(COUNT_SUM, 0, 64)
    rng = np.random.default_rng(6000)
    agg_epoch([(G(), g), (oracle(), o)], [all_keys_chunk(rng, agg_keys(64))],
              1)
    g.close()
    o.close()


def small_join_parity():
    g, o = join_pair(JOIN_INNER, 1)
    c = chunk([np.arange(50) % 10, np.arange(50)])
    join_push((g, o), SIDE_LEFT, c, "left")
    assert len(join_push((g, o), SIDE_RIGHT, c, "right")) == 250
    g.close()
    o.close()


def small_topn_parity():
    g, o = topn_pair(**TOPN_RANDOM)
    rng = np.random.default_rng(6001)
    c = topn_mix_chunk(rng, [], 200, 8, 50, 10**6, 0.2,
                       key_map=topn_groups())
    assert len(topn_push((g, o), c, "fresh")) > 0
    g.close()
    o.close()


@pytest.mark.parametrize("kernel", ["generic", "dense"])
def test_error_agg_65th_key(kernel):
    keys = agg_keys(64)
    dense = kernel == "dense"
    calls, rci = DENSE_SHAPES["dense4_3"] if dense else (COUNT_SUM, 0)
    g, o = agg_pair(calls, rci, 64, append_only=dense)
    rng = np.random.default_rng(6100 + dense)
    n = 1024 if dense else 300
    agg_epoch([(G(), g), (oracle(), o)], [all_keys_chunk(rng, keys, n)], 1)
    extra = all_keys_chunk(rng, keys + (5 * 10**12,), n)
    with pytest.raises(RuntimeError, match="agg state table full"):
        g.push(extra)
        g.flush(2)
    assert "agg state table full" in G().last_error()
    g.close()
    o.close()
    small_agg_parity()


def test_error_agg_minput_513th_row():
    keys = np.array(agg_keys(64), np.int64)
    g, o = minput_pair()
    rng = np.random.default_rng(6200)
    n = 512
    cols = [keys[covering(rng, np.arange(64), n)],
            rng.integers(-500, 500, n), np.arange(n)]
    minput_epoch([(G(), g), (oracle(), o)], [chunk(cols)], 1)
    with pytest.raises(RuntimeError, match="agg minput row store full"):
        g.push(chunk([[keys[0]], [1], [n]]))
        g.flush(2)
    assert "agg minput row store full" in G().last_error()
    g.close()
    o.close()
    g, o = minput_pair()
    minput_epoch([(G(), g), (oracle(), o)], [chunk(cols)], 1)
    g.close()
    o.close()


@pytest.mark.parametrize("jt", [JOIN_INNER, JOIN_LEFT_OUTER])
def test_error_join_row_n_plus_1(jt):
    n = 1024
    g, o = join_pair(jt, 1, rows=n)
    rng = np.random.default_rng(6300 + jt)
    join_push((g, o), SIDE_LEFT, chunk([rng.integers(0, 50, n),
                                        np.arange(n)]), "exactly full")
    with pytest.raises(RuntimeError, match="join row store full"):
        g.push(SIDE_LEFT, chunk([[7], [n]]))
    assert "join row store full" in G().last_error()
    g.close()
    o.close()
    small_join_parity()


def test_error_topn_ninth_group():
    g, o = topn_pair(**TOPN_RANDOM)
    c = chunk([np.repeat(topn_groups(), 4), np.arange(32), np.arange(32)])
    assert len(topn_push((g, o), c, "eight groups")) > 0
    with pytest.raises(RuntimeError, match="group table full"):
        g.push(chunk([[123_456_789], [1], [99]]))
    assert "group table full" in G().last_error()
    g.close()
    o.close()
    small_topn_parity()


def test_error_topn_row_store_exact():
    n = 1024
    g, o = topn_pair(rows=n, **TOPN_RANDOM)
    rng = np.random.default_rng(6400)
    groups = np.array(topn_groups(), np.int64)
    c = chunk([groups[rng.integers(0, 8, n)], rng.integers(0, 200, n),
               np.arange(n)])
    assert len(topn_push((g, o), c, "exactly full")) > 0
    with pytest.raises(RuntimeError, match="row store full"):
        g.push(chunk([[groups[0]], [5], [n]]))
    assert "row store full" in G().last_error()
    g.close()
    o.close()
    small_topn_parity()
