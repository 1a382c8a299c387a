#!/usr/bin/env python3
"""GROUP BY (window, channel) with a varchar `channel` (measurement
infrastructure): chunks of 1M rows, count(*) and sum(v),
`channel` 8-32 random bytes drawn from D distinct values, against the same
stream with an i64 surrogate in the channel's place.

Per D, medians over 5 pushes after one warm-up: the push's wall time, the
three interning kernels and the apply kernel (device events;
RW_AGG_INTERN_TIMING=1, rw_hash_agg_varlen_intern_stats /
rw_agg_kernel_stats), the flush's wall time and the device time of its
string materialisation. The lookup kernel's rate in G strings/s is set
against the measured random 64-B line rate (profiles/r02_membw_probes.json,
1 GiB region): each lookup is one random slot line plus one random string
line.

One D per process, so each timed step can run under its own time limit,
chained with &&:

    timeout -k 10 300 python tests/bench_varchar_agg.py --distinct 4 \\
        --part /tmp/va_4.json && \\
    timeout -k 10 300 python tests/bench_varchar_agg.py --distinct 1000 \\
        --part /tmp/va_1000.json && \\
    timeout -k 10 300 python tests/bench_varchar_agg.py --distinct 1000000 \\
        --part /tmp/va_1000000.json && \\
    python tests/bench_varchar_agg.py --merge /tmp/va_4.json \\
        /tmp/va_1000.json /tmp/va_1000000.json

--merge prints one JSON line and writes it to profiles/varchar_agg.json
(RW_BENCH_OUT overrides); it needs no GPU. Not a pytest test.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

N = 1 << 20
PUSHES = 5
WINDOWS = 4


def merge(parts):
    results = [json.load(open(p)) for p in parts]
    ref = json.load(open(os.path.join(HERE, "..", "profiles",
                                      "r02_membw_probes.json")))
    rand = next(r for r in ref["membw_random_64B"] if r["region"] == "1 GiB")
    for r in results:
        v = r["varchar"]
        v["lookup_frac_of_random_line_rate"] = round(
            v["lookup_Gstrings_per_s"] / rand["Glines_per_s"], 4)
    out = {"bench": "varchar_agg", "rows_per_push": N, "pushes": PUSHES,
           "random_line_Glines_per_s": rand["Glines_per_s"],
           "results": results}
    line = json.dumps(out)
    print(line)
    dst = os.environ.get("RW_BENCH_OUT", os.path.join(
        HERE, "..", "profiles", "varchar_agg.json"))
    with open(dst, "w") as f:
        f.write(line + "\n")


def measure(distinct, part):
    os.environ["RW_AGG_INTERN_TIMING"] = "1"
    import risingwave_amd
    from rwtest import ffi
    from rwtest import varchar as vc
    from rwtest import varchar_agg as va

    lib = ffi.Lib(risingwave_amd.lib_path())
    L = lib.lib
    rng = np.random.default_rng(17)
    T_V = vc.T_VARCHAR

    # the D distinct channels, packed
    plens = rng.integers(8, 33, distinct).astype(np.int64)
    poffs = np.zeros(distinct + 1, np.int64)
    np.cumsum(plens, out=poffs[1:])
    praw = rng.integers(32, 127, int(poffs[-1]), dtype=np.uint8)

    class KS(C.Structure):
        _fields_ = [("launches", C.c_uint64), ("total_ms", C.c_double),
                    ("rows", C.c_uint64)]

    def chunk(varchar, idx, window, v):
        n = len(idx)
        keep = [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
        types = [ffi.T_I64, T_V if varchar else ffi.T_I64, ffi.T_I64]
        cols = (ffi.RwColumn * 3)()
        for i, a in ((0, window), (2, v)):
            a = np.ascontiguousarray(a, dtype=np.int64)
            cols[i].data = a.ctypes.data
            keep.append(a)
        if varchar:
            lens = plens[idx]
            offs = np.zeros(n + 1, np.uint32)
            np.cumsum(lens, out=offs[1:])
            pos = (np.arange(int(offs[-1]), dtype=np.int64)
                   - np.repeat(offs[:-1].astype(np.int64), lens)
                   + np.repeat(poffs[idx], lens))
            raw = praw[pos]
            vd = vc.RwVarlenData()
            vd.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
            vd.bytes = raw.ctypes.data_as(C.POINTER(C.c_uint8))
            cols[1].data = C.addressof(vd)
            keep.extend([offs, raw, vd])
        else:
            a = np.ascontiguousarray(idx + 1_000_000_007, dtype=np.int64)
            cols[1].data = a.ctypes.data
            keep.append(a)
        for i, t in enumerate(types):
            cols[i].type = t
            cols[i].valid = keep[1].ctypes.data
        ch = ffi.RwChunkC()
        ch.n_rows, ch.n_cols = n, 3
        ch.ops = C.cast(keep[0].ctypes.data, C.POINTER(C.c_uint8))
        ch.vis = None
        ch.cols = cols
        keep.append(cols)
        return ch, keep

    def run(varchar):
        types = [ffi.T_I64, T_V if varchar else ffi.T_I64, ffi.T_I64]
        calls = [(ffi.AGG_COUNT_STAR, -1, ffi.T_I64),
                 (ffi.AGG_SUM, 2, ffi.T_I64)]
        agg = ffi.HashAgg(lib, types, [0, 1], calls, row_count_index=0,
                          chunk_size=N, state_capacity_hint=1 << 23)
        r2 = np.random.default_rng(23)  # the same stream for both runs
        push_ms, flush_ms, k_ms, apply_ms, fetch_ms = [], [], [], [], []
        prev_k, prev_f, prev_a = [0.0, 0.0, 0.0], 0.0, 0.0
        n_out = 0
        for it in range(PUSHES + 1):  # first push = warm-up
            idx = r2.integers(0, distinct, N)
            window = r2.integers(0, WINDOWS, N) * 10
            v = r2.integers(0, 1000, N)
            ch, keep = chunk(varchar, idx, window, v)
            t0 = time.perf_counter()
            rc = L.rw_hash_agg_push_chunk(agg.h, C.byref(ch))
            t1 = time.perf_counter()
            assert rc == 0, lib.last_error()
            rc = L.rw_hash_agg_flush(agg.h, it + 1)
            t2 = time.perf_counter()
            assert rc == 0, lib.last_error()
            n_out = 0
            while True:
                p = L.rw_hash_agg_poll(agg.h)
                if not p:
                    break
                n_out += p.contents.n_rows
                L.rw_chunk_free(p)
            # drop the epoch's spill (untimed) so it does not pile up
            buf, ln = C.POINTER(C.c_uint8)(), C.c_uint64()
            L.rw_agg_checkpoint_drain.argtypes = [
                C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)),
                C.POINTER(C.c_uint64)]
            assert L.rw_agg_checkpoint_drain(agg.h, C.byref(buf),
                                             C.byref(ln)) == 0
            L.rw_spill_free.argtypes = [C.c_void_p]
            L.rw_spill_free(C.cast(buf, C.c_void_p))
            ks = KS()
            assert L.rw_agg_kernel_stats(C.c_void_p(agg.h), C.byref(ks)) == 0
            km = (C.c_double * 3)()
            fm, nl = C.c_double(), C.c_uint64()
            if varchar:
                L.rw_hash_agg_varlen_intern_stats.argtypes = [
                    C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                    C.POINTER(C.c_uint64)]
                assert L.rw_hash_agg_varlen_intern_stats(
                    agg.h, km, C.byref(fm), C.byref(nl)) == 0
            if it:
                push_ms.append(1e3 * (t1 - t0))
                flush_ms.append(1e3 * (t2 - t1))
                k_ms.append([km[k] - prev_k[k] for k in range(3)])
                fetch_ms.append(fm.value - prev_f)
                apply_ms.append(ks.total_ms - prev_a)
            prev_k, prev_f, prev_a = list(km), fm.value, ks.total_ms
        med = lambda xs: round(float(np.median(xs)), 4)
        res = {"push_wall_ms": med(push_ms), "apply_kernel_ms": med(apply_ms),
               "flush_wall_ms": med(flush_ms), "flush_rows_last": n_out}
        if varchar:
            lk = med([k[0] for k in k_ms])
            res.update({
                "intern_lookup_ms": lk,
                "intern_commit_ms": med([k[1] for k in k_ms]),
                "intern_resolve_ms": med([k[2] for k in k_ms]),
                "flush_materialise_ms": med(fetch_ms),
                "lookup_Gstrings_per_s": round(N / lk / 1e6, 3),
                "stats": dict(zip(("arena_used", "arena_cap", "n_strings",
                                   "table_cap"),
                                  va.varlen_stats(lib, agg.h)))})
        agg.close()
        return res

    out = {"distinct": distinct, "i64": run(False), "varchar": run(True)}
    with open(part, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


ap = argparse.ArgumentParser()
ap.add_argument("--distinct", type=int)
ap.add_argument("--part")
ap.add_argument("--merge", nargs="+")
a = ap.parse_args()
if a.merge:
    merge(a.merge)
else:
    measure(a.distinct, a.part)
