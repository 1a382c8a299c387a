"""Helpers for HashAgg with RW_T_VARCHAR group keys (include/rw_stream.h
"varchar GROUP KEYS in HashAgg").

As for the join (rwtest/varchar.py) the CPU oracle has no string type and
stays untouched: a varchar group key influences aggregation only through
key equality, so the reference is the oracle run on a SURROGATE — every
distinct string maps to a distinct i64 id, NULL maps to NULL — with its
output ids mapped back to strings and its drain frames re-encoded.
"""
import ctypes as C
import os
import re
import struct

import numpy as np

from rwtest import ffi
from rwtest import varchar as vc
from rwtest.ffi import OP_DELETE, OP_INSERT, T_I64
from rwtest.varchar import T_VARCHAR, VChunk, sort_rows

RW_E_INVAL = -1


def header_consts():
    """AGG_ARENA_HEADER / AGG_ARENA_ALIGN as include/rw_varlen.hpp has them."""
    path = os.path.join(ffi.REPO, "include", "rw_varlen.hpp")
    src = open(path).read()
    out = {}
    for name in ("AGG_ARENA_HEADER", "AGG_ARENA_ALIGN"):
        m = re.search(r"constexpr\s+uint64_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out["AGG_ARENA_HEADER"], out["AGG_ARENA_ALIGN"]


# ---- the new C entries ----

def varlen_reserve(lib, h, arena_bytes, n_strings):
    L = lib.lib
    L.rw_hash_agg_varlen_reserve.restype = C.c_int
    L.rw_hash_agg_varlen_reserve.argtypes = [C.c_void_p, C.c_uint64,
                                             C.c_uint64]
    return L.rw_hash_agg_varlen_reserve(h, arena_bytes, n_strings)


def varlen_stats(lib, h):
    """(arena_used, arena_cap, n_strings, table_cap); synchronises."""
    L = lib.lib
    L.rw_hash_agg_varlen_stats.restype = C.c_int
    L.rw_hash_agg_varlen_stats.argtypes = [C.c_void_p] + [
        C.POINTER(C.c_uint64)] * 4
    v = [C.c_uint64() for _ in range(4)]
    rc = L.rw_hash_agg_varlen_stats(h, *[C.byref(x) for x in v])
    assert rc == 0, lib.last_error()
    return tuple(x.value for x in v)


def poll_all(agg):
    """agg.poll_all() for executors whose output has varchar columns."""
    out = []
    while True:
        p = agg.lib.lib.rw_hash_agg_poll(agg.h)
        if not p:
            return out
        out.append(vc.read_chunk(agg.lib, p))


def out_types_of(types, group_key, calls):
    return [types[k] for k in group_key] + [c[2] for c in calls]


# ---- spill frames: independent Python encoders ----

def memcmp_str(s):
    """Memcomparable varchar datum, ASC NULLS LAST (rw_codec.hpp): written
    here independently of the C++ (tests compare the two)."""
    if s is None:
        return b"\x01"
    if not s:
        return b"\x00\x00"
    out = bytearray(b"\x00\x01")
    for off in range(0, len(s), 8):
        g = s[off:off + 8]
        out += g + b"\0" * (8 - len(g))
        out.append(9 if off + 8 < len(s) else len(g))
    return bytes(out)


def memcmp_i64(v):
    if v is None:
        return b"\x01"
    return b"\x00" + struct.pack(">Q", (v + (1 << 63)) & ((1 << 64) - 1))


def decode_memcmp_i64_key(key, n):
    """n surrogate (i64) datums of an oracle key -> list of int-or-None."""
    vals, off = [], 0
    for _ in range(n):
        tag = key[off]
        off += 1
        if tag == 1:
            vals.append(None)
        else:
            (u,) = struct.unpack_from(">Q", key, off)
            vals.append(u - (1 << 63))
            off += 8
    assert off == len(key), "trailing key bytes"
    return vals


def encode_value_row(row, types):
    out = bytearray()
    for v, t in zip(row, types):
        if v is None:
            out.append(0)
        elif t == T_VARCHAR:
            out.append(1)
            out += struct.pack("<I", len(v)) + v
        else:
            out.append(1)
            out += struct.pack("<q", v)
    return bytes(out)


def reencode_drain(buf, sur, key_types, out_types):
    """An oracle drain over surrogate ids -> the byte stream an executor
    with the real (varchar) key types must produce: keys re-encoded with
    memcmp_str, values with the varchar value layout, frames in key order
    (stable, as sort_spill_frames)."""
    frames = []
    nk = len(key_types)
    sur_out = sur.types(out_types)
    for put, key, val in vc.decode_frames(buf):
        ids = decode_memcmp_i64_key(key, nk)
        k = b"".join(
            memcmp_str(sur.str_of[i] if i is not None else None)
            if t == T_VARCHAR else memcmp_i64(i)
            for i, t in zip(ids, key_types))
        v = b""
        if put:
            row = vc.decode_row(val, sur_out)
            row = tuple(sur.str_of[x] if t == T_VARCHAR and x is not None
                        else x for x, t in zip(row, out_types))
            v = encode_value_row(row, out_types)
        else:
            assert val == b""
        frames.append((put, k, v))
    frames.sort(key=lambda f: f[1])  # list.sort is stable
    out = bytearray()
    for put, k, v in frames:
        out.append(put)
        out += struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v
    return bytes(out)


# ---- seeded workload shared by the CPU workload test and the GPU tests ----

# The issue's schema (window i64, name varchar, v i64, w i64) plus a second
# varchar column for the two-varchar-key shape.
TYPES = [T_I64, T_VARCHAR, T_I64, T_I64, T_VARCHAR]
COL_WINDOW, COL_NAME, COL_V, COL_W, COL_NAME2 = range(5)
CALLS = [(ffi.AGG_COUNT_STAR, -1, T_I64), (ffi.AGG_SUM, COL_V, T_I64),
         (ffi.AGG_COUNT, COL_W, T_I64)]
CALLS_APPEND = [(ffi.AGG_COUNT_STAR, -1, T_I64), (ffi.AGG_MIN, COL_V, T_I64),
                (ffi.AGG_MAX, COL_V, T_I64)]
WINDOWS = [0, 10, 20, 30, 40, 50]
NAME2 = [b"web", b"app", None, b""]
SIZES = [64, 100, 255, 256, 301, 512]
# pinned by tests/test_varchar_agg_workload.py: chosen among neighbouring
# seeds for margin on every coverage condition that test states
SEED = 20241026


def make_workload(seed=SEED, n_epochs=3, chunks_per_epoch=4, p_del=0.2,
                  p_revive=0.06, stop_below=None):
    """Seeded insert/retract stream over TYPES. ~p_del of the rows retract
    a live row (full row content, possibly one inserted earlier in the same
    chunk); ~p_revive insert a fresh row for a (window, name) whose last row
    was retracted earlier, so groups get re-created after deletion.
    stop_below = (epoch, window): from that epoch on, rows with a smaller
    window are no longer retracted (their groups may have been cleaned by a
    watermark). Returns epochs: list of lists of VChunk."""
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(97, 123, int(rng.integers(8, 33)),
                               dtype=np.uint8)) for _ in range(40)]
    live, dead = [], []

    def new_row():
        if dead and rng.random() < p_revive:
            win, name = dead.pop(int(rng.integers(0, len(dead))))
        else:
            win = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
            name = vc._name(rng, pool)
        w = None if rng.random() < 0.25 else int(rng.integers(0, 1000))
        return (win, name, int(rng.integers(-10**6, 10**6)), w,
                NAME2[int(rng.integers(0, len(NAME2)))])

    epochs = []
    for e in range(n_epochs):
        if stop_below and e == stop_below[0]:
            live = [r for r in live if r[COL_WINDOW] >= stop_below[1]]
        chunks = []
        for _ in range(chunks_per_epoch):
            n = SIZES[int(rng.integers(0, len(SIZES)))]
            ops, rows = [], []
            for _r in range(n):
                if live and rng.random() < p_del:
                    row = live.pop(int(rng.integers(0, len(live))))
                    ops.append(OP_DELETE)
                    dead.append((row[COL_WINDOW], row[COL_NAME]))
                else:
                    row = new_row()
                    if not (stop_below and e >= stop_below[0]
                            and row[COL_WINDOW] < stop_below[1]):
                        live.append(row)
                    ops.append(OP_INSERT)
                rows.append(row)
            chunks.append(VChunk.from_rows(TYPES, ops, rows))
        epochs.append(chunks)
    return epochs


def naive_group_by(epochs, group_key):
    """CALLS (count(*), sum(v), count(w)) grouped by the STRINGS themselves
    in a Python dict, with the executor's change inference at each flush:
    '+' for a group first seen (or seen again after its Delete), '-' with
    the previous output when its row count reaches 0, 'U-'/'U+' when the
    output changed, nothing when it did not. Per flush the sorted rows."""
    state, prev, outs = {}, {}, []
    for chunks in epochs:
        dirty = []
        for c in chunks:
            for op, row in zip(c.ops, c.rows()):
                key = tuple(row[k] for k in group_key)
                st = state.setdefault(key, [0, 0, 0])
                sign = 1 if op == OP_INSERT else -1
                st[0] += sign
                st[1] += sign * row[COL_V]
                st[2] += sign * (row[COL_W] is not None)
                if key not in dirty:
                    dirty.append(key)
        rows = []
        for key in dirty:
            st = state[key]
            cur = key + tuple(st) if st[0] > 0 else None
            old = prev.get(key)
            if old is None and cur is not None:
                rows.append(("+", cur))
            elif old is not None and cur is None:
                rows.append(("-", old))
            elif old is not None and cur != old:
                rows.append(("U-", old))
                rows.append(("U+", cur))
            if cur is None:
                prev.pop(key, None)
                state.pop(key)
            else:
                prev[key] = cur
        outs.append(sort_rows(rows))
    return outs


class Run:
    """outs[e] = sorted (op, row) of flush e; drains[e] = drain bytes taken
    at the end of epoch e (after that epoch's watermark, if any)."""

    def __init__(self):
        self.outs, self.drains = [], []


def oracle_run(epochs, group_key, calls=CALLS, sur=None, append_only=False,
               watermarks=None, types=TYPES, state=None):
    """The UNCHANGED oracle on the surrogate stream; outputs mapped back to
    strings, drains re-encoded (reencode_drain). watermarks: {epoch index:
    (group_key_pos, val)}, applied after that epoch's flush."""
    sur = sur or vc.Surrogate()
    ot = out_types_of(types, group_key, calls)
    kt = ot[:len(group_key)]
    o = ffi.HashAgg(ffi.oracle(), sur.types(types), group_key, calls,
                    row_count_index=0, append_only=append_only)
    run = Run()
    for e, chunks in enumerate(epochs):
        for c in chunks:
            o.push(sur.chunk(c))
        o.flush(e + 1)
        rows = []
        for ch in o.poll_all():
            rows.extend(ch.visible_rows())
        run.outs.append(sort_rows(sur.rows_back(rows, ot)))
        if watermarks and e in watermarks:
            o.watermark(*watermarks[e])
        run.drains.append(reencode_drain(
            ffi.agg_checkpoint_drain_bytes(ffi.oracle(), o.h), sur, kt, ot))
    o.close()
    return run, sur


def gpu_epoch(lib, agg, chunks, epoch, run, watermark=None):
    """Push, flush, poll, optional watermark, drain: one epoch on `agg`."""
    for c in chunks:
        agg.push(c)
    agg.flush(epoch)
    out = poll_all(agg)
    run.outs.append(vc.rows_of(out))
    if watermark:
        agg.watermark(*watermark)
    run.drains.append(ffi.agg_checkpoint_drain_bytes(lib, agg.h))
    return out


def gpu_run(lib, epochs, group_key, calls=CALLS, append_only=False,
            watermarks=None, types=TYPES, reserve=None, **extra):
    agg = ffi.HashAgg(lib, types, group_key, calls, row_count_index=0,
                      append_only=append_only, **extra)
    if reserve:
        assert varlen_reserve(lib, agg.h, *reserve) == 0, lib.last_error()
    run = Run()
    out_chunks = []
    for e, chunks in enumerate(epochs):
        out_chunks.extend(gpu_epoch(lib, agg, chunks, e + 1, run,
                                    (watermarks or {}).get(e)))
    run.out_chunks = out_chunks
    return run, agg
