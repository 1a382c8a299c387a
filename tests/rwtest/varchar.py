"""Bindings and helpers for RW_T_VARCHAR payload columns (include/rw_chunk.h
RwVarlenData, include/rw_stream.h "varchar payload columns").

The CPU oracle has no string type and stays untouched: a varchar payload
influences join semantics only through row equality, so the tests run the
oracle on a SURROGATE — every distinct string maps to a distinct i64 id,
NULL maps to NULL — and map the oracle's output ids back to strings.
"""
import ctypes as C
import struct

import numpy as np

from rwtest import ffi
from rwtest.ffi import OP_DELETE, OP_INSERT, T_I64, T_TS, TOKEN_BY_OP

T_VARCHAR = 7
RW_E_INVAL = -1


class RwVarlenData(C.Structure):
    _fields_ = [("offsets", C.POINTER(C.c_uint32)),
                ("bytes", C.POINTER(C.c_uint8))]


class VChunk:
    """Python-side chunk that may hold varchar columns. A varchar column is
    a list of bytes-or-None (None = NULL); other columns are int lists.
    Duck-types ffi.Chunk (n_rows / to_c / visible_rows)."""

    def __init__(self, types, ops, cols, vis=None):
        self.types = list(types)
        self.ops = np.asarray(ops, dtype=np.uint8)
        self.cols = [list(c) for c in cols]
        self.vis = None if vis is None else np.asarray(vis, dtype=np.uint8)

    @classmethod
    def from_rows(cls, types, ops, rows):
        cols = [[r[i] for r in rows] for i in range(len(types))]
        return cls(types, ops, cols)

    @property
    def n_rows(self):
        return len(self.ops)

    def rows(self):
        return [tuple(c[r] for c in self.cols) for r in range(self.n_rows)]

    def to_c(self):
        n = self.n_rows
        cols = (ffi.RwColumn * len(self.cols))()
        self._keep = [cols]
        for i, (t, col) in enumerate(zip(self.types, self.cols)):
            valid = np.array([v is not None for v in col], dtype=np.uint8)
            cols[i].type = t
            cols[i].valid = valid.ctypes.data
            self._keep.append(valid)
            if t == T_VARCHAR:
                lens = [len(v) if v is not None else 0 for v in col]
                offs = np.zeros(n + 1, dtype=np.uint32)
                np.cumsum(lens, out=offs[1:])
                raw = b"".join(v for v in col if v is not None)
                buf = np.frombuffer(raw + b"\0", dtype=np.uint8).copy()
                vd = RwVarlenData()
                vd.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
                vd.bytes = buf.ctypes.data_as(C.POINTER(C.c_uint8))
                cols[i].data = C.addressof(vd)
                self._keep.extend([offs, buf, vd])
            else:
                data = np.array([v if v is not None else 0 for v in col],
                                dtype=np.int64)
                cols[i].data = data.ctypes.data
                self._keep.append(data)
        ch = ffi.RwChunkC()
        ch.n_rows = n
        ch.n_cols = len(self.cols)
        ch.ops = C.cast(self.ops.ctypes.data, C.POINTER(C.c_uint8))
        ch.vis = (C.cast(self.vis.ctypes.data, C.POINTER(C.c_uint8))
                  if self.vis is not None else None)
        ch.cols = cols
        return ch

    def visible_rows(self):
        for r in range(self.n_rows):
            if self.vis is not None and not self.vis[r]:
                continue
            yield (TOKEN_BY_OP[int(self.ops[r])],
                   tuple(c[r] for c in self.cols))


def raw_varchar_chunk(n_rows, offsets, raw=b"x"):
    """A one-column varchar RwChunkC with a caller-chosen offsets array (for
    malformed / over-long inputs: `raw` may be shorter than offsets claim)."""
    keep = []
    offs = np.asarray(offsets, dtype=np.uint32)
    buf = np.frombuffer(raw, dtype=np.uint8).copy()
    vd = RwVarlenData()
    vd.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
    vd.bytes = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    keep.extend([offs, buf, vd])
    return vd, keep


def read_chunk(lib, p):
    """rw_*_poll result -> VChunk (understands type 7); frees the chunk."""
    ch = p.contents
    n, m = ch.n_rows, ch.n_cols
    types, cols = [], []
    for ci in range(m):
        col = ch.cols[ci]
        t = col.type
        types.append(t)
        valid = C.string_at(col.valid, n) if n else b""
        if t == T_VARCHAR:
            vd = C.cast(col.data, C.POINTER(RwVarlenData)).contents
            offs = [vd.offsets[r] for r in range(n + 1)]
            assert offs[0] == 0 and all(a <= b for a, b in zip(offs, offs[1:]))
            raw = C.string_at(vd.bytes, offs[n]) if offs[n] else b""
            vals = []
            for r in range(n):
                if valid[r]:
                    vals.append(raw[offs[r]:offs[r + 1]])
                else:
                    # output contract: NULL rows have zero length
                    assert offs[r] == offs[r + 1], "NULL row with bytes"
                    vals.append(None)
        else:
            assert t in (T_I64, T_TS), t
            data = np.frombuffer(C.string_at(col.data, n * 8), dtype=np.int64)
            vals = [int(data[r]) if valid[r] else None for r in range(n)]
        cols.append(vals)
    ops = np.frombuffer(C.string_at(ch.ops, n), dtype=np.uint8).copy()
    vis = None
    if ch.vis:
        vis = np.frombuffer(C.string_at(ch.vis, n), dtype=np.uint8).copy()
    lib.lib.rw_chunk_free(p)
    return VChunk(types, ops, cols, vis)


def poll_all(join):
    """join.poll_all() for executors whose output has varchar columns."""
    out = []
    while True:
        p = join.lib.lib.rw_hash_join_poll(join.h)
        if not p:
            return out
        out.append(read_chunk(join.lib, p))


class Surrogate:
    """distinct string <-> distinct i64 id (NULL <-> NULL)."""

    def __init__(self):
        self.id_of = {}
        self.str_of = {}

    def sid(self, s):
        if s is None:
            return None
        if s not in self.id_of:
            i = 1_000_000_007 + 7919 * len(self.id_of)
            self.id_of[s] = i
            self.str_of[i] = s
        return self.id_of[s]

    def types(self, types):
        return [T_I64 if t == T_VARCHAR else t for t in types]

    def chunk(self, vc):
        """VChunk -> ffi.Chunk with varchar columns replaced by id columns."""
        cols, valids = [], []
        for t, col in zip(vc.types, vc.cols):
            vals = [self.sid(v) if t == T_VARCHAR else v for v in col]
            valids.append([v is not None for v in vals])
            cols.append([v if v is not None else 0 for v in vals])
        return ffi.Chunk(self.types(vc.types), vc.ops, cols, valids, vc.vis)

    def rows_back(self, rows, out_types):
        """(op, row) list from the oracle -> the same with ids as strings."""
        out = []
        for op, row in rows:
            out.append((op, tuple(
                self.str_of[v] if t == T_VARCHAR and v is not None else v
                for t, v in zip(out_types, row))))
        return out


def sort_rows(rows):
    """rows_multiset's ordering for rows that hold bytes cells."""
    def cell(v):
        if v is None:
            return (2, 0, b"")
        if isinstance(v, bytes):
            return (1, 0, v)
        return (0, v, b"")
    return sorted(rows, key=lambda r: (r[0], tuple(cell(v) for v in r[1])))


def rows_of(chunks):
    rows = []
    for c in chunks:
        rows.extend(c.visible_rows())
    return sort_rows(rows)


# ---- spill frames ([put u8][klen u32][key][vlen u32][value], rw_stream.h) ----

def decode_frames(buf):
    out, off = [], 0
    while off < len(buf):
        put = buf[off]
        (klen,) = struct.unpack_from("<I", buf, off + 1)
        key = buf[off + 5:off + 5 + klen]
        (vlen,) = struct.unpack_from("<I", buf, off + 5 + klen)
        val = buf[off + 9 + klen:off + 9 + klen + vlen]
        assert len(key) == klen and len(val) == vlen, "truncated frame"
        out.append((put, key, val))
        off += 9 + klen + vlen
    return out


def decode_row(val, types):
    """value-encoded row -> tuple (varchar: presence, u32 LE length, bytes)."""
    row, off = [], 0
    for t in types:
        present = val[off]
        off += 1
        if not present:
            row.append(None)
        elif t == T_VARCHAR:
            (n,) = struct.unpack_from("<I", val, off)
            row.append(bytes(val[off + 4:off + 4 + n]))
            assert len(row[-1]) == n
            off += 4 + n
        else:
            (v,) = struct.unpack_from("<q", val, off)
            row.append(v)
            off += 8
    assert off == len(val), "trailing bytes in value"
    return tuple(row)


# ---- arena entry points ----

def varlen_reserve(lib, h, side, nbytes):
    L = lib.lib
    L.rw_hash_join_varlen_reserve.restype = C.c_int
    L.rw_hash_join_varlen_reserve.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    return L.rw_hash_join_varlen_reserve(h, side, nbytes)


def varlen_stats(lib, h, side):
    L = lib.lib
    L.rw_hash_join_varlen_stats.restype = C.c_int
    L.rw_hash_join_varlen_stats.argtypes = [
        C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    used, cap = C.c_uint64(), C.c_uint64()
    rc = L.rw_hash_join_varlen_stats(h, side, C.byref(used), C.byref(cap))
    assert rc == 0, lib.last_error()
    return used.value, cap.value


def varlen_emit_stats(lib, h):
    L = lib.lib
    L.rw_hash_join_varlen_emit_stats.restype = C.c_int
    L.rw_hash_join_varlen_emit_stats.argtypes = [
        C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    ms, cms, nb, nl = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
    rc = L.rw_hash_join_varlen_emit_stats(h, C.byref(ms), C.byref(cms),
                                          C.byref(nb), C.byref(nl))
    assert rc == 0, lib.last_error()
    return ms.value, cms.value, nb.value, nl.value


# ---- seeded workload shared by the CPU workload test and the GPU tests ----

LONG = bytes(range(256)) + b"tail-over-255"          # > 255 bytes
UTF8 = "naïve — 日本語 ✓".encode()                    # multi-byte UTF-8
PREFIX_A = b"p" * 64 + b"A"                          # share a 64-byte prefix
PREFIX_B = b"p" * 64 + b"B"
SPECIALS = [b"", None, UTF8, LONG, PREFIX_A, PREFIX_B]


def _name(rng, pool):
    x = rng.random()
    if x < 0.12:
        return SPECIALS[int(rng.integers(0, len(SPECIALS)))]
    if x < 0.45:  # equal strings across rows
        return pool[int(rng.integers(0, len(pool)))]
    n = int(rng.integers(1, 40))
    return bytes(rng.integers(32, 127, n, dtype=np.uint8))


def make_workload(seed, schemas, key_spaces, n_epochs=3, chunks_per_epoch=4,
                  p_del=0.2, p_same_chunk=0.15, all_insert_chunks=()):
    """Seeded two-sided insert/retract stream.

    schemas[side] = list of (type, role): role 'key' (join key, drawn from
    key_spaces[side]), 'uniq' (unique counter — the pk), 'val' (random i64)
    or 'str' (varchar payload). Returns epochs: list of lists of
    (side, VChunk). ~p_del of the rows retract a live row of the same side
    (full row content); some retract a row inserted EARLIER IN THE SAME
    chunk. Chunks listed in all_insert_chunks (global index) are all-insert.
    Chunk sizes vary in 64..512."""
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(97, 123, int(rng.integers(8, 33)),
                               dtype=np.uint8)) for _ in range(40)]
    live = {0: [], 1: []}
    uniq = [0]

    def new_row(side):
        row = []
        for t, role in schemas[side]:
            if role == "key":
                row.append(int(rng.integers(0, key_spaces[side])))
            elif role == "uniq":
                uniq[0] += 1
                row.append(uniq[0])
            elif role == "val":
                row.append(int(rng.integers(0, 10**6)))
            else:
                row.append(_name(rng, pool))
        return tuple(row)

    sizes = [64, 100, 255, 256, 301, 512]
    epochs, gidx = [], 0
    for _ in range(n_epochs):
        chunks = []
        for ci in range(chunks_per_epoch):
            side = ci % 2
            n = sizes[int(rng.integers(0, len(sizes)))]
            no_del = gidx in all_insert_chunks
            ops, rows, fresh = [], [], []
            for _r in range(n):
                x = rng.random()
                if not no_del and x < p_del and (live[side] or fresh):
                    if fresh and (not live[side] or rng.random() < p_same_chunk):
                        row = fresh.pop(int(rng.integers(0, len(fresh))))
                    else:
                        row = live[side].pop(
                            int(rng.integers(0, len(live[side]))))
                    ops.append(OP_DELETE)
                    rows.append(row)
                else:
                    row = new_row(side)
                    fresh.append(row)
                    ops.append(OP_INSERT)
                    rows.append(row)
            live[side].extend(fresh)
            types = [t for t, _ in schemas[side]]
            chunks.append((side, VChunk.from_rows(types, ops, rows)))
            gidx += 1
        epochs.append(chunks)
    return epochs


# q8 shape: person (id, name, ts) x auction (seller, ts, pk) on id = seller.
# Person ids repeat (pk = (id, ts)) so an auction row can match >1 person;
# sellers range past the person ids so some probes match nothing.
Q8_LEFT = [(T_I64, "key"), (T_VARCHAR, "str"), (T_TS, "uniq")]
Q8_RIGHT = [(T_I64, "key"), (T_TS, "val"), (T_I64, "uniq")]
Q8_KW = dict(key_l=[0], key_r=[0], pk_l=[0, 2], pk_r=[2])
# The seed is pinned by tests/test_varchar_workload.py; among other things
# it keeps every same-chunk insert/delete pair from being emitted ADJACENT
# with one match each, which the oracle would eliminate as a no-op.
Q8_SEED = 20240810
Q8_ALL_INSERT = (5,)  # global chunk index 5: right side, epoch 2


def q8_workload():
    return make_workload(Q8_SEED, [Q8_LEFT, Q8_RIGHT], [120, 160],
                         chunks_per_epoch=6, all_insert_chunks=Q8_ALL_INSERT)


def naive_inner_join(epochs, key_l=0, key_r=0):
    """Row-at-a-time inner join on the STRINGS themselves (no surrogate, no
    oracle): per push the sorted (op, left ++ right) rows. NULL keys never
    occur in these workloads. It applies no adjacent-no-op elimination, so
    agreeing with the oracle's raw output also shows the oracle eliminated
    nothing on this stream (its elimination is emission-order dependent,
    which a parallel emitter cannot reproduce — see net_rows)."""
    live = {0: [], 1: []}
    kc = {0: key_l, 1: key_r}
    outs = []
    for chunks in epochs:
        for side, c in chunks:
            rows = []
            for op, row in zip(c.ops, c.rows()):
                tok = "+" if op == OP_INSERT else "-"
                for other in live[1 - side]:
                    if other[kc[1 - side]] == row[kc[side]]:
                        rows.append((tok, row + other if side == 0
                                     else other + row))
                if op == OP_INSERT:
                    live[side].append(row)
                else:
                    live[side].remove(row)
            outs.append(sort_rows(rows))
    return outs


def schema_types(schema):
    return [t for t, _ in schema]


def out_types_of(join_type, types_l, types_r):
    if join_type in (ffi.JOIN_LEFT_SEMI, ffi.JOIN_LEFT_ANTI):
        return list(types_l)
    if join_type in (ffi.JOIN_RIGHT_SEMI, ffi.JOIN_RIGHT_ANTI):
        return list(types_r)
    return list(types_l) + list(types_r)


def oracle_run(join_type, types_l, types_r, kw, epochs, sur=None, drains=False):
    """Run the UNCHANGED oracle on the surrogate stream. Returns
    (per-push output rows mapped back to strings, per-epoch drains, sur).
    drains[e][side] = raw frame bytes of the surrogate tables."""
    sur = sur or Surrogate()
    o = ffi.HashJoin(ffi.oracle(), join_type, sur.types(types_l),
                     sur.types(types_r), **kw)
    ot = out_types_of(join_type, types_l, types_r)
    outs, dr = [], []
    for e, chunks in enumerate(epochs):
        for side, vc in chunks:
            o.push(side, sur.chunk(vc))
            rows = []
            for c in o.poll_all():
                rows.extend(c.visible_rows())
            outs.append(sort_rows(sur.rows_back(rows, ot)))
        o.flush(e + 1)
        if drains:
            dr.append([ffi.join_checkpoint_drain(ffi.oracle(), o.h, s)
                       for s in (0, 1)])
    o.close()
    return outs, dr, sur
