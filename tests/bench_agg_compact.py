#!/usr/bin/env python3
"""rw_hash_agg_compact against the restore route (measurement infrastructure,
DESIGN.md §19): a q7-shaped executor, max(price) and count(*) by a 10 s
window key, in a key table of 2^24 slots of which 1/16 hold live windows and
--ready-frac (default 1/2) are READY, the rest of the READY ones cleaned by a
watermark. The varchar variant adds a second group key of 8-32 bytes, one
string per group.

Per run a fresh executor is filled (1M-row pushes, one flush and drain
each), the watermark cleans all but the newest 2^20 windows, and two ways of
getting the slots back are timed by a host clock around calls that end in a
device synchronise:
  compact : rw_hash_agg_compact on that executor
  restore : the only way before it, a fresh executor of the same capacity
            restored from the concatenated drains (create + restore)
Medians over --runs (default 5) after one warm-up run of the same shape. The
pass's bytes are computed from the shapes (bytes_model) and its rate is set
against the 5.78 TB/s read rate of DESIGN.md §8; it is a whole-call rate, the
host round trips of the call included, not a kernel's share of peak.

One variant per process, each under its own time limit, chained with &&:

    timeout -k 10 900 python tests/bench_agg_compact.py --variant i64 \\
        --part /tmp/ac_i64.json && \\
    timeout -k 10 900 python tests/bench_agg_compact.py --variant varchar \\
        --part /tmp/ac_varchar.json && \\
    python tests/bench_agg_compact.py --merge /tmp/ac_i64.json \\
        /tmp/ac_varchar.json

--merge prints one JSON line and writes it to profiles/agg_compact.json
(RW_BENCH_OUT overrides); it needs no GPU. --budget-s stops starting new
runs once that much time has gone and reports the runs completed. Not a
pytest test.
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

PUSH = 1 << 20
READ_RATE_TBPS = 5.78  # DESIGN.md §8, measured streaming read rate


def bytes_model(cap, ready, live, kw, n_calls):
    """Bytes the pass has to move, from the shapes (value-state calls, no
    decimal or minput columns). Per slot the table keeps state 4, key words
    8 kw, null mask 4, and per call acc 8, has 1, prev 8, prev_null 1, then
    has_prev 1 and dirty_flag 4."""
    rec = 8 * kw + 4 + n_calls * 18 + 1
    per_slot = 4 + rec + 4
    scan = cap * 4 + ready * (1 + 4 + 8)       # state; liveness of READY slots
    pack = live * (rec + rec + 4)              # read the slot, write the record
    clear = cap * per_slot                     # every per-slot array rewritten
    reinsert = live * (rec + rec + 4 + 4)      # read the record, write the slot
    return {"scan": scan, "pack": pack, "clear": clear, "reinsert": reinsert,
            "total": scan + pack + clear + reinsert}


def merge(parts):
    results = [json.load(open(p)) for p in parts]
    out = {"bench": "agg_compact", "read_rate_TBps": READ_RATE_TBPS,
           "results": results}
    line = json.dumps(out)
    print(line)
    dst = os.environ.get("RW_BENCH_OUT", os.path.join(
        HERE, "..", "profiles", "agg_compact.json"))
    with open(dst, "w") as f:
        f.write(line + "\n")


def measure(a):
    import risingwave_amd
    from rwtest import ffi
    from rwtest import varchar as vc
    from rwtest import varchar_agg as va
    from rwtest.agg_compact import compact, state_stats

    lib = ffi.Lib(risingwave_amd.lib_path())
    L = lib.lib
    varchar = a.variant == "varchar"
    cap = 1 << a.log2_slots
    n_live = cap // 16
    n_ready = int(cap * a.ready_frac)
    assert n_live < n_ready <= cap
    kw = 2 if varchar else 1
    types = ([ffi.T_I64, vc.T_VARCHAR, ffi.T_I64] if varchar
             else [ffi.T_I64, ffi.T_I64])
    price_col = kw
    calls = [(ffi.AGG_MAX, price_col, ffi.T_I64),
             (ffi.AGG_COUNT_STAR, -1, ffi.T_I64)]
    L.rw_agg_checkpoint_drain.restype = C.c_int
    L.rw_agg_checkpoint_drain.argtypes = [
        C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
    L.rw_spill_free.argtypes = [C.c_void_p]

    def chunk(rng, window):
        n = len(window)
        keep = [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
        cols = (ffi.RwColumn * len(types))()
        fixed = [(0, window), (price_col, rng.integers(1, 10**7, n))]
        for i, arr in fixed:
            arr = np.ascontiguousarray(arr, dtype=np.int64)
            cols[i].data = arr.ctypes.data
            keep.append(arr)
        if varchar:  # one string of 8-32 random bytes per row
            lens = rng.integers(8, 33, n).astype(np.uint32)
            offs = np.zeros(n + 1, np.uint32)
            np.cumsum(lens, out=offs[1:])
            raw = rng.integers(32, 127, int(offs[-1]), dtype=np.uint8)
            vd = vc.RwVarlenData()
            vd.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint32))
            vd.bytes = raw.ctypes.data_as(C.POINTER(C.c_uint8))
            cols[1].data = C.addressof(vd)
            keep.extend([offs, raw, vd])
        for i, t in enumerate(types):
            cols[i].type = t
            cols[i].valid = keep[1].ctypes.data
        ch = ffi.RwChunkC()
        ch.n_rows, ch.n_cols = n, len(types)
        ch.ops = C.cast(keep[0].ctypes.data, C.POINTER(C.c_uint8))
        ch.vis = None
        ch.cols = cols
        keep.append(cols)
        return ch, keep

    def drain(agg, into):
        buf, ln = C.POINTER(C.c_uint8)(), C.c_uint64()
        assert L.rw_agg_checkpoint_drain(agg.h, C.byref(buf),
                                         C.byref(ln)) == 0, lib.last_error()
        into.append(C.string_at(buf, ln.value))
        L.rw_spill_free(C.cast(buf, C.c_void_p))

    def mk():
        return ffi.HashAgg(lib, types, list(range(kw)), calls,
                           row_count_index=1, append_only=True,
                           chunk_size=PUSH, state_capacity_hint=cap)

    def build(seed):
        """n_ready windows in the table, all but the newest n_live cleaned;
        returns the executor and its concatenated drains."""
        rng = np.random.default_rng(seed)
        agg = mk()
        drains = []
        for e, lo in enumerate(range(0, n_ready, PUSH)):
            window = np.arange(lo, min(lo + PUSH, n_ready), dtype=np.int64) * 10
            ch, keep = chunk(rng, window)
            assert L.rw_hash_agg_push_chunk(agg.h, C.byref(ch)) == 0, \
                lib.last_error()
            assert L.rw_hash_agg_flush(agg.h, e + 1) == 0, lib.last_error()
            while True:
                p = L.rw_hash_agg_poll(agg.h)
                if not p:
                    break
                L.rw_chunk_free(p)
            drain(agg, drains)
            del keep
        agg.watermark(0, (n_ready - n_live) * 10)
        drain(agg, drains)
        return agg, b"".join(drains)

    t_start = time.perf_counter()
    runs = []
    for it in range(a.runs + 1):  # first run = warm-up
        t0 = time.perf_counter()
        agg, drains = build(100 + it)
        t1 = time.perf_counter()
        before = state_stats(lib, agg.h)
        vbefore = va.varlen_stats(lib, agg.h) if varchar else None
        t2 = time.perf_counter()
        got = compact(lib, agg.h)
        t3 = time.perf_counter()
        after = state_stats(lib, agg.h)
        vafter = va.varlen_stats(lib, agg.h) if varchar else None
        agg.close()
        assert before == (n_ready, n_live, cap), before
        assert got == n_ready - n_live and after == (n_live, n_live, cap)
        t4 = time.perf_counter()
        fresh = mk()
        ffi.agg_restore(lib, fresh.h, drains)
        t5 = time.perf_counter()
        assert state_stats(lib, fresh.h) == (n_live, n_live, cap)
        fresh.close()
        r = {"build_s": round(t1 - t0, 3),
             "compact_ms": round(1e3 * (t3 - t2), 3),
             "restore_ms": round(1e3 * (t5 - t4), 3),
             "drain_bytes": len(drains)}
        if varchar:
            r["varlen_before"] = vbefore
            r["varlen_after"] = vafter
        print(json.dumps({"run": it, **r}), flush=True)
        if it:
            runs.append(r)
        if time.perf_counter() - t_start > a.budget_s and runs:
            break
    med = lambda k: round(float(np.median([r[k] for r in runs])), 3)
    bm = bytes_model(cap, n_ready, n_live, kw, len(calls))
    c_ms = med("compact_ms")
    out = {"variant": a.variant, "slots": cap, "slots_ready": n_ready,
           "groups_live": n_live, "runs": len(runs),
           "compact_ms": c_ms, "restore_ms": med("restore_ms"),
           "restore_over_compact": round(med("restore_ms") / c_ms, 2),
           "compact_ms_all": [r["compact_ms"] for r in runs],
           "restore_ms_all": [r["restore_ms"] for r in runs],
           "bytes_model": bm,
           "compact_GBps": round(bm["total"] / c_ms / 1e6, 1),
           "frac_of_read_rate": round(
               bm["total"] / c_ms / 1e6 / (READ_RATE_TBPS * 1e3), 4)}
    if varchar:
        out["varlen_before"] = runs[-1]["varlen_before"]
        out["varlen_after"] = runs[-1]["varlen_after"]
        out["note"] = ("bytes_model counts the key table only; the string "
                       "re-interning is extra work inside compact_ms")
    with open(a.part, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["i64", "varchar"])
ap.add_argument("--part")
ap.add_argument("--merge", nargs="+")
ap.add_argument("--log2-slots", type=int, default=24)
ap.add_argument("--ready-frac", type=float, default=0.5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--budget-s", type=float, default=800)
a = ap.parse_args()
if a.merge:
    merge(a.merge)
else:
    measure(a)
