"""The exchange hop's typed payload, Python side.

Everything here is written from the layout TEXT of include/rw_xpayload.hpp,
not by calling the library, so it pins the layout:

    block(n rows, C columns, V varchar bytes) =
        vals[C][npad] i64   npad = n rounded up to 4
        valid[C][n]   u8
        ops[n]        u8
        pad to 32
        vbytes[V]     u8    one region shared by all varchar columns
        pad to 32

A varchar cell's vals entry is off | len << 40 with off relative to vbytes; a
NULL cell is word 0 with valid 0. The reference for routing is zlib.crc32 over
the hash_datum byte feed: i64 = 8 LE bytes, NULL = u32 0xfffffff0, varchar =
its bytes followed by one 0xFF (str's Hash: write(bytes); write_u8(0xff)).
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

T_I64, T_TS, T_VARCHAR = 0, 5, 7
OFF_BITS = 40
MAX_OFF = (1 << OFF_BITS) - 1


# ---- the reference feed ----

def feed(row_datums):
    buf = b""
    for v in row_datums:
        if v is None:
            buf += struct.pack("<I", 0xFFFFFFF0)
        elif isinstance(v, (bytes, bytearray)):
            buf += bytes(v) + b"\xff"
        else:
            buf += struct.pack("<q", v)
    return buf


def expected_vnode(row_datums, vnode_count=256):
    """tests/test_vnode_dispatch.py's expected_vnode, extended to bytes."""
    return zlib.crc32(feed(row_datums)) % vnode_count


def dest_of_vnode(vnode, vnode_count, n_dests):
    return min(vnode // (vnode_count // n_dests), n_dests - 1)


def expected_dest(row_datums, vnode_count, n_dests):
    return dest_of_vnode(expected_vnode(row_datums, vnode_count), vnode_count,
                         n_dests)


# the length set of the vnode test: "" and NULL, every length 1..17, a long
# common prefix, multi-byte UTF-8, 0x00 / 0xFF inside, one 70 000-byte string
HUGE = bytes((i * 7 + 3) & 0xFF for i in range(70_000))
SPECIAL_NAMES = (
    [b"", None]
    + [bytes((37 * n + i) & 0xFF for i in range(n)) for n in range(1, 18)]
    + [b"p" * 64 + b"A", b"p" * 64 + b"B", b"p" * 64,
       "naïve — 日本語 ✓".encode(), b"\x00", b"\xff", b"a\x00b\xffc",
       b"\xff\xff\xff\xff\xff\xff\xff\xff\xff", HUGE])


def name_column(rng, n):
    """n names: the specials first, then random 1..40-byte strings with a few
    NULLs and repeats."""
    out = list(SPECIAL_NAMES[:n])
    while len(out) < n:
        x = rng.random()
        if x < 0.05:
            out.append(None)
        elif x < 0.15:
            out.append(out[int(rng.integers(0, len(out)))])
        else:
            out.append(bytes(rng.integers(0, 256, int(rng.integers(1, 41)),
                                          dtype=np.uint8)))
    return out


# ---- layout ----

def pad32(x):
    return (x + 31) & ~31


class Layout:
    def __init__(self, n, n_cols, vbytes):
        self.n, self.n_cols, self.V = n, n_cols, vbytes
        self.npad = (n + 3) & ~3
        self.valid_off = n_cols * self.npad * 8
        self.ops_off = self.valid_off + n_cols * n
        self.vbytes_off = pad32(self.ops_off + n)
        self.total = self.vbytes_off + pad32(vbytes)

    def vals_off(self, c):
        return c * self.npad * 8


def old_block_bytes(n, n_cols):
    """rw_exchange_run's all-i64 block size."""
    npad = (n + 3) & ~3
    return (n_cols * npad * 8 + n_cols * n + n + 31) & ~31


def decode_block_np(buf, n, types, vbytes):
    """One block (numpy uint8 array of exactly Layout.total bytes) -> (ops,
    words[C][n] u64, valid[C][n] u8, region u8[V]); asserts the region
    invariants: NULL => word 0; live ranges in bounds, pairwise disjoint,
    lengths summing to V with no gaps."""
    L = Layout(n, len(types), vbytes)
    assert len(buf) == L.total, (len(buf), L.total)
    words = [np.frombuffer(buf, np.uint64, n, L.vals_off(c))
             for c in range(len(types))]
    valid = [np.frombuffer(buf, np.uint8, n, L.valid_off + c * n)
             for c in range(len(types))]
    ops = np.frombuffer(buf, np.uint8, n, L.ops_off)
    region = np.frombuffer(buf, np.uint8, vbytes, L.vbytes_off)
    for c in range(len(types)):
        assert np.all(valid[c] <= 1)
        assert np.all(words[c][valid[c] == 0] == 0), "NULL cell with a word"
    offs, lens = [], []
    for c, t in enumerate(types):
        if t == T_VARCHAR:
            live = valid[c] == 1
            offs.append((words[c][live] & np.uint64(MAX_OFF)).astype(np.int64))
            lens.append((words[c][live] >> np.uint64(OFF_BITS)).astype(np.int64))
    if offs:
        off, ln = np.concatenate(offs), np.concatenate(lens)
        assert np.all(off + ln <= vbytes), "range out of bounds"
        assert int(ln.sum()) == vbytes, (int(ln.sum()), vbytes)
        nz = ln > 0
        off, ln = off[nz], ln[nz]
        order = np.argsort(off, kind="stable")
        off, ln = off[order], ln[order]
        if len(off):
            assert off[0] == 0, "gap at the start of vbytes"
            assert np.all(off[1:] == off[:-1] + ln[:-1]), "overlap or gap"
    else:
        assert vbytes == 0
    return ops, words, valid, region


def decode_block(buf, n, types, vbytes):
    """One block -> list of (op, row tuple); varchar cells as bytes / None."""
    ops, words, valid, region = decode_block_np(buf, n, types, vbytes)
    raw = region.tobytes()
    cols = []
    for c, t in enumerate(types):
        if t == T_VARCHAR:
            col = []
            for w, ok in zip(words[c].tolist(), valid[c].tolist()):
                if ok:
                    o, ln = w & MAX_OFF, w >> OFF_BITS
                    col.append(raw[o:o + ln])
                else:
                    col.append(None)
        else:
            vals = words[c].view(np.int64).tolist()
            col = [v if ok else None for v, ok in zip(vals, valid[c].tolist())]
        cols.append(col)
    return [(int(ops[r]), tuple(col[r] for col in cols)) for r in range(n)]


def encode_column(t, col, lead=3):
    """A column as the typed entries take it: (words i64[n], valid u8[n],
    arena bytes or None). The arena starts with `lead` filler bytes so that
    strings sit at unaligned addresses."""
    valid = np.array([v is not None for v in col], dtype=np.uint8)
    if t != T_VARCHAR:
        return (np.array([v if v is not None else 0 for v in col], np.int64),
                valid, None)
    words = np.zeros(len(col), np.uint64)
    parts, off = [b"\xa5" * lead], lead
    for r, v in enumerate(col):
        if v is None:
            # the word of a NULL row is ignored: make it hostile
            words[r] = MAX_OFF | (0xFFFFFF << OFF_BITS)
            continue
        words[r] = off | (len(v) << OFF_BITS)
        parts.append(v)
        off += len(v)
    return words.view(np.int64), valid, np.frombuffer(b"".join(parts) + b"\0",
                                                      np.uint8)


# ---- librw_exchange bindings ----

class RwXCol(C.Structure):
    _fields_ = [("type", C.c_uint8), ("vals", C.c_void_p),
                ("valid", C.c_void_p), ("bytes", C.c_void_p)]


_U64P = C.POINTER(C.c_uint64)


class XLib:
    """librw_exchange.so with a one-rank Exchange handle."""

    def __init__(self, handle=True):
        import risingwave_amd

        path = os.path.join(os.path.dirname(risingwave_amd.lib_path()),
                            "librw_exchange.so")
        L = self.L = C.CDLL(path)
        L.rw_exchange_last_error.restype = C.c_char_p
        L.rw_exchange_create.restype = C.c_void_p
        L.rw_exchange_create.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.rw_exchange_destroy.argtypes = [C.c_void_p]
        L.rw_xbuf_alloc.restype = C.c_void_p
        L.rw_xbuf_alloc.argtypes = [C.c_uint64]
        L.rw_xbuf_free.argtypes = [C.c_void_p]
        L.rw_xbuf_write.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.rw_xbuf_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.rw_exchange_partition.argtypes = [
            C.c_void_p, C.POINTER(RwXCol), C.c_int, C.c_void_p, C.c_uint32,
            C.POINTER(C.c_uint32), C.c_int, C.c_uint32, C.c_int, C.c_void_p,
            C.c_uint64, _U64P, _U64P, _U64P]
        L.rw_exchange_partition_phases.argtypes = [C.c_void_p,
                                                   C.POINTER(C.c_double)]
        L.rw_exchange_run_typed.argtypes = [
            C.c_void_p, C.POINTER(RwXCol), C.c_int, C.c_void_p, C.c_uint32,
            C.POINTER(C.c_uint32), C.c_int, C.c_uint32, C.c_void_p, C.c_uint64,
            C.c_void_p, C.c_uint64, _U64P, _U64P, _U64P, _U64P]
        L.rw_exchange_run.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
            C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_uint32, C.c_void_p,
            C.c_uint64, C.c_void_p, C.c_uint64, _U64P, _U64P]
        self.h = None
        self.world = 1
        if handle:
            sz = L.rw_exchange_unique_id_size()
            uid = (C.c_uint8 * sz)()
            assert L.rw_exchange_get_unique_id(uid) == 0, self.err()
            self.adopt(L.rw_exchange_create(1, 0, uid), 1)

    def adopt(self, h, world):
        assert h, self.err()
        self.h, self.world = h, world

    def err(self):
        return self.L.rw_exchange_last_error().decode()

    def close(self):
        if self.h:
            self.L.rw_exchange_destroy(self.h)
            self.h = None

    def alloc(self, nbytes):
        p = self.L.rw_xbuf_alloc(max(nbytes, 32))
        assert p, "rw_xbuf_alloc failed"
        return p

    def free(self, p):
        self.L.rw_xbuf_free(p)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        assert self.L.rw_xbuf_write(p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def download(self, dev, nbytes, offset=0):
        out = np.empty(nbytes, np.uint8)
        assert self.L.rw_xbuf_read(out.ctypes.data, dev + offset, nbytes) == 0
        return out


class Batch:
    """A typed batch staged on the device through rw_xbuf_write."""

    def __init__(self, xl, types, cols, ops):
        self.xl, self.types, self.n = xl, list(types), len(ops)
        self.bufs = []
        self.desc = (RwXCol * len(types))()
        for c, (t, col) in enumerate(zip(types, cols)):
            if isinstance(col, tuple):      # pre-encoded (words, valid, arena)
                words, valid, arena = col
            else:
                words, valid, arena = encode_column(t, col)
            self.desc[c].type = t
            self.desc[c].vals = self._up(words)
            self.desc[c].valid = self._up(valid)
            self.desc[c].bytes = self._up(arena) if arena is not None else None
        self.ops = self._up(np.asarray(ops, np.uint8))

    def _up(self, arr):
        p = self.xl.upload(arr)
        self.bufs.append(p)
        return p

    def free(self):
        for p in self.bufs:
            self.xl.free(p)
        self.bufs = []


class Partitioned:
    pass


def partition(xl, batch, keys, n_dests, vnode_count=256, send=None,
              send_cap=None, decode=True):
    """rw_exchange_partition + read-back. Returns an object with rc, rows,
    vbytes, offs, and (rc == 0 and decode) blocks[d] = [(op, row), ...]."""
    own = send is None
    if own:
        send_cap = (1 << 20) + 80 * batch.n * len(batch.types) \
            if send_cap is None else send_cap
        send = xl.alloc(send_cap)
    rows = (C.c_uint64 * 64)()
    vb = (C.c_uint64 * 64)()
    offs = (C.c_uint64 * 64)()
    kc = (C.c_uint32 * len(keys))(*keys)
    out = Partitioned()
    out.rc = xl.L.rw_exchange_partition(
        xl.h, batch.desc, len(batch.types), batch.ops, batch.n, kc, len(keys),
        vnode_count, n_dests, send, send_cap, rows, vb, offs)
    out.err = xl.err() if out.rc else ""
    if out.rc == 0:
        out.rows, out.vbytes = list(rows)[:n_dests], list(vb)[:n_dests]
        out.offs = list(offs)[:n_dests]
        out.sizes = [Layout(r, len(batch.types), v).total
                     for r, v in zip(out.rows, out.vbytes)]
        out.raw = [xl.download(send, sz, off)
                   for sz, off in zip(out.sizes, out.offs)]
        if decode:
            out.blocks = [decode_block(raw, r, batch.types, v) for raw, r, v
                          in zip(out.raw, out.rows, out.vbytes)]
    if own:
        xl.free(send)
    return out


def python_partition(types, cols, ops, keys, n_dests, vnode_count=256):
    """The reference partition: per destination the sorted (op, row) list."""
    want = [[] for _ in range(n_dests)]
    for r in range(len(ops)):
        row = tuple(col[r] for col in cols)
        d = expected_dest([row[k] for k in keys], vnode_count, n_dests)
        want[d].append((int(ops[r]), row))
    return want


def sort_block(rows):
    def cell(v):
        if v is None:
            return (2, 0, b"")
        if isinstance(v, bytes):
            return (1, 0, v)
        return (0, v, b"")
    return sorted(rows, key=lambda r: (r[0], tuple(cell(v) for v in r[1])))
