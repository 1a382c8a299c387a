#!/usr/bin/env python3
"""q8-shaped emit with a varchar payload (measurement infrastructure,
DESIGN.md §13.5): 1M probe rows per launch, every row matching one person
whose `name` (8-32 random bytes) is materialised on emit, against the same
shape with an i64 payload in the name's place.

Reports, per copy-kernel variant (RW_VARLEN_COPY=dword|b16|lane): the probe
launch time, the materialisation's device time (length + scan + copy) and
the copy kernel's share, the gather's achieved bytes/s and strings/s, and
the latter as a fraction of the measured random 64-B line rate
(profiles/r02_membw_probes.json, 1 GiB region) — each 8-32-byte string is
one random line touch (two when it straddles a line). Prints one JSON line
and writes it to profiles/varchar_emit.json; not a pytest test.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import risingwave_amd
from rwtest import ffi
from rwtest import varchar as vc

N = 1 << 20
LAUNCHES = 5
T_V = vc.T_VARCHAR

lib = ffi.Lib(risingwave_amd.lib_path())
L = lib.lib
rng = np.random.default_rng(12)


def raw_chunk(types, cols_np, varlen=None):
    """RwChunkC straight from numpy (a python list of 1M bytes objects is
    too slow to build); varlen = {col: (offsets u32, bytes u8)}."""
    n = len(cols_np[0])
    keep = [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
    cols = (ffi.RwColumn * len(types))()
    for i, t in enumerate(types):
        cols[i].type = t
        cols[i].valid = keep[1].ctypes.data
        if t == T_V:
            offs, raw = varlen[i]
            vd = vc.RwVarlenData()
            vd.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
            vd.bytes = raw.ctypes.data_as(C.POINTER(C.c_uint8))
            cols[i].data = C.addressof(vd)
            keep.extend([offs, raw, vd])
        else:
            a = np.ascontiguousarray(cols_np[i], dtype=np.int64)
            cols[i].data = a.ctypes.data
            keep.append(a)
    ch = ffi.RwChunkC()
    ch.n_rows, ch.n_cols = n, len(types)
    ch.ops = C.cast(keep[0].ctypes.data, C.POINTER(C.c_uint8))
    ch.vis = None
    ch.cols = cols
    keep.append(cols)
    return ch, keep


def run(payload_type, variant):
    os.environ["RW_VARLEN_COPY"] = variant
    tl = [ffi.T_I64, payload_type, ffi.T_TS]
    tr = [ffi.T_I64, ffi.T_TS, ffi.T_I64]
    j = ffi.HashJoin(lib, ffi.JOIN_INNER, tl, tr, key_l=[0], key_r=[0],
                     pk_l=[0, 2], pk_r=[2], chunk_size=N,
                     state_capacity_hint=8 * N, row_capacity_hint=8 * N)
    ids = rng.permutation(N).astype(np.int64)
    lens = rng.integers(8, 33, N).astype(np.uint32)
    offs = np.zeros(N + 1, np.uint32)
    np.cumsum(lens, out=offs[1:])
    raw = rng.integers(32, 127, int(offs[-1]), dtype=np.uint8)
    ch, keep = raw_chunk(tl, [ids, np.arange(N), np.arange(N)],
                         {1: (offs, raw)})
    assert L.rw_hash_join_push_chunk(j.h, 0, C.byref(ch)) == 0, lib.last_error()
    wall = []
    for it in range(LAUNCHES + 1):  # first launch = warm-up
        sellers = rng.permutation(N).astype(np.int64)
        pk = np.arange(N, dtype=np.int64) + (it + 1) * N
        ch, keep = raw_chunk(tr, [sellers, pk, pk])
        if it == 1:
            L.rw_join_stats_reset(C.c_void_p(j.h))
            s0 = vc.varlen_emit_stats(lib, j.h)
        t0 = time.perf_counter()
        rc = L.rw_hash_join_push_chunk(j.h, 1, C.byref(ch))
        wall.append(time.perf_counter() - t0)
        assert rc == 0, lib.last_error()
        n_out = 0
        while True:
            p = L.rw_hash_join_poll(j.h)
            if not p:
                break
            n_out += p.contents.n_rows
            L.rw_chunk_free(p)
        assert n_out == N, n_out
    s1 = vc.varlen_emit_stats(lib, j.h)

    class KS(C.Structure):
        _fields_ = [("launches", C.c_uint64), ("total_ms", C.c_double),
                    ("rows", C.c_uint64)]
    ks = KS()
    assert L.rw_join_kernel_stats(C.c_void_p(j.h), C.byref(ks)) == 0
    j.close()
    res = {"payload": "varchar" if payload_type == T_V else "i64",
           "push_wall_ms": round(1e3 * float(np.median(wall[1:])), 2),
           "probe_kernel_ms": round(ks.total_ms / max(ks.launches, 1), 4)}
    if payload_type == T_V:
        n = s1[3] - s0[3]
        ms, cms, nb = (s1[0] - s0[0]) / n, (s1[1] - s0[1]) / n, (s1[2] - s0[2]) / n
        res.update({"copy_variant": variant,
                    "materialise_ms": round(ms, 4),
                    "copy_kernel_ms": round(cms, 4),
                    "bytes_per_launch": int(nb),
                    "copy_GBps_payload": round(nb / cms / 1e6, 1),
                    "copy_Gstrings_per_s": round(N / cms / 1e6, 2)})
    return res


rows = [run(ffi.T_I64, "b16"), run(T_V, "dword"), run(T_V, "b16"),
        run(T_V, "lane")]
ref = json.load(open(os.path.join(HERE, "..", "profiles",
                                  "r02_membw_probes.json")))
rand = next(r for r in ref["membw_random_64B"] if r["region"] == "1 GiB")
for r in rows:
    if "copy_Gstrings_per_s" in r:
        r["frac_of_random_line_rate"] = round(
            r["copy_Gstrings_per_s"] / rand["Glines_per_s"], 3)
out = {"bench": "varchar_emit", "rows_per_launch": N, "launches": LAUNCHES,
       "random_line_Glines_per_s": rand["Glines_per_s"], "results": rows}
line = json.dumps(out)
print(line)
dst = os.environ.get("RW_BENCH_OUT",
                     os.path.join(HERE, "..", "profiles", "varchar_emit.json"))
with open(dst, "w") as f:
    f.write(line + "\n")
