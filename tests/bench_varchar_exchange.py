#!/usr/bin/env python3
"""The exchange partition with a varchar payload (measurement infrastructure,
DESIGN.md §14): 1M person-shaped rows (i64 id, name of 8-32 random bytes,
i64 ts) partitioned by id to 8 destinations through rw_exchange_partition,
against the same rows with an i64 in the name's place, which run the all-i64
kernels. Per-phase device time (count, scan, scatter, byte copy), medians of
5 after one warm-up; rows/s and bytes/s of packed output; the ratio to the
i64 baseline.

Without arguments this is a driver that touches no GPU itself: it runs each
measurement as a child process under its own `timeout` and stops at the
first failure. Prints one JSON line and writes it to
profiles/varchar_exchange.json; not a pytest test.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
N = 1 << 20
N_DESTS = 8
RUNS = 5
STEP_TIMEOUT_S = 180


def step(kind):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, ".."))
    import ctypes as C

    import numpy as np

    from rwtest import xpayload as xp

    rng = np.random.default_rng(14)
    xl = xp.XLib()
    ids = rng.permutation(N).astype(np.int64)
    ts = np.arange(N, dtype=np.int64)
    ones = np.ones(N, np.uint8)
    if kind == "varchar":
        lens = rng.integers(8, 33, N).astype(np.uint64)
        offs = np.zeros(N + 1, np.uint64)
        np.cumsum(lens, out=offs[1:])
        arena = rng.integers(32, 127, int(offs[-1]) + 1, dtype=np.uint8)
        words = (offs[:-1] | (lens << np.uint64(xp.OFF_BITS))).view(np.int64)
        name = (words, ones, arena)
        types = [xp.T_I64, xp.T_VARCHAR, xp.T_TS]
    else:
        name = (rng.integers(0, 2**62, N).astype(np.int64), ones, None)
        types = [xp.T_I64, xp.T_I64, xp.T_TS]
    batch = xp.Batch(xl, types, [(ids, ones, None), name, (ts, ones, None)],
                     np.zeros(N, np.uint8))
    cap = 96 << 20
    send = xl.alloc(cap)
    kc = (C.c_uint32 * 1)(0)
    rows, vb, offs_o = [(C.c_uint64 * 64)() for _ in range(3)]
    ms = (C.c_double * 4)()
    phases = []
    for it in range(RUNS + 1):  # first = warm-up
        rc = xl.L.rw_exchange_partition(xl.h, batch.desc, 3, batch.ops, N, kc,
                                        1, 256, N_DESTS, send, cap, rows, vb,
                                        offs_o)
        assert rc == 0, xl.err()
        xl.L.rw_exchange_partition_phases(xl.h, ms)
        if it:
            phases.append(list(ms))
    assert sum(list(rows)[:N_DESTS]) == N
    med = [float(np.median([p[i] for p in phases])) for i in range(4)]
    packed = sum(xp.Layout(rows[d], 3, vb[d]).total for d in range(N_DESTS))
    total = sum(med)
    res = {"payload": kind,
           "count_ms": round(med[0], 4), "scan_ms": round(med[1], 4),
           "scatter_ms": round(med[2], 4), "byte_copy_ms": round(med[3], 4),
           "device_ms": round(total, 4),
           "Grows_per_s": round(N / total / 1e6, 3),
           "packed_bytes": int(packed),
           "varchar_bytes": int(sum(list(vb)[:N_DESTS])),
           "packed_GBps": round(packed / total / 1e6, 1)}
    if kind == "varchar":
        res["copy_Gstrings_per_s"] = round(N / med[3] / 1e6, 2)
        res["copy_GBps_of_varchar_bytes"] = round(
            res["varchar_bytes"] / med[3] / 1e6, 1)
    batch.free()
    xl.free(send)
    xl.close()
    print("RESULT " + json.dumps(res))


def main():
    results = []
    for kind in ("i64", "varchar"):
        p = subprocess.run(
            ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable,
             os.path.abspath(__file__), "--step", kind],
            capture_output=True, text=True)
        if p.returncode != 0:  # stop at the first failure
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"step {kind} failed with exit status {p.returncode}")
        line = next(ln for ln in p.stdout.splitlines()
                    if ln.startswith("RESULT "))
        results.append(json.loads(line[len("RESULT "):]))
    base, var = results
    out = {"bench": "varchar_exchange", "rows": N, "n_dests": N_DESTS,
           "runs": RUNS, "results": results,
           "varchar_over_i64_device_ms": round(
               var["device_ms"] / base["device_ms"], 3)}
    line = json.dumps(out)
    print(line)
    dst = os.environ.get(
        "RW_BENCH_OUT",
        os.path.join(HERE, "..", "profiles", "varchar_exchange.json"))
    with open(dst, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        step(sys.argv[2])
    else:
        main()
