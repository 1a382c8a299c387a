"""The dense apply kernel's span mapping (each wave owns adjacent 256-row
tiles and carries an open run across them) against the oracle.
`rw_agg_debug_set_span_tiles` fixes tiles-per-wave so that small batches
reach multi-tile spans; the key patterns put run boundaries on and off
tile and span boundaries. The control flow is modelled on the host in
tests/test_span_carry_model.py.
"""
import ctypes

import numpy as np
import pytest

from rwtest import ffi
from rwtest.ffi import AGG_COUNT_STAR, AGG_MAX, AGG_SUM, OP_INSERT, T_I64, oracle

pytestmark = pytest.mark.gpu

TILE = 256
MAX_COUNT = [(AGG_MAX, 1, T_I64), (AGG_COUNT_STAR, -1, T_I64)]
SUM_COUNT = [(AGG_SUM, 1, T_I64), (AGG_COUNT_STAR, -1, T_I64)]
ROW_COUNTS = [1024, 1025, 4096 + 3, 16384]  # 1024 = the dense path's minimum
CONFIGS = [("max", MAX_COUNT, 1), ("max", MAX_COUNT, 2), ("max", MAX_COUNT, 3),
           ("max", MAX_COUNT, 8), ("sum", SUM_COUNT, 3)]


def gpu():
    import risingwave_amd

    return ffi.Lib(risingwave_amd.lib_path())


def key_patterns(rng, n, span_tiles):
    a, b, c = 10_000_000, 20_000_000, 30_000_000
    rows = np.arange(n)
    span = span_tiles * TILE
    span_edge = span if span < n else (n // 2) // TILE * TILE
    blip = np.full(n, a)
    blip[300:350] = c
    return {
        "one key": np.full(n, a),
        "change on a tile boundary": np.where(rows < 2 * TILE, a, b),
        "change mid-tile, other key after": np.where(rows < TILE + 100, a, b),
        "change mid-tile, same key after": blip,
        "change on a span boundary": np.where(rows < span_edge, a, b),
        "random keys from 5": rng.integers(0, 5, n) * a,
        "sorted runs of 1000": rows // 1000 * a,
    }


def rows_sorted(chunks):
    mats = []
    for c in chunks:
        cols = [c.ops.astype(np.int64)]
        for d, v in zip(c.cols, c.valids):
            cols.append(np.where(v != 0, d, 0).astype(np.int64))
            cols.append((v != 0).astype(np.int64))
        m = np.stack(cols, axis=1)
        if c.vis is not None:
            m = m[c.vis != 0]
        mats.append(m)
    m = np.concatenate(mats, axis=0)
    return m[np.lexsort(m.T[::-1])]


@pytest.mark.parametrize("n_rows", ROW_COUNTS)
@pytest.mark.parametrize("name,calls,span_tiles", CONFIGS,
                         ids=[f"{c[0]}-span{c[2]}" for c in CONFIGS])
def test_span_apply_matches_oracle(name, calls, span_tiles, n_rows):
    glib = gpu()
    L = glib.lib
    L.rw_agg_bench_preload.restype = ctypes.c_void_p
    L.rw_agg_bench_preload.argtypes = [ctypes.c_void_p,
                                       ctypes.POINTER(ffi.RwChunkC)]
    L.rw_agg_bench_apply.restype = ctypes.c_int
    L.rw_agg_bench_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.rw_agg_debug_set_span_tiles.restype = ctypes.c_int
    L.rw_agg_debug_set_span_tiles.argtypes = [ctypes.c_void_p, ctypes.c_uint32]

    rng = np.random.default_rng(1000 * span_tiles + n_rows)
    for what, keys in key_patterns(rng, n_rows, span_tiles).items():
        vals = rng.integers(1, 10**7, n_rows)
        chunk = ffi.Chunk([T_I64, T_I64], np.full(n_rows, OP_INSERT, np.uint8),
                          [keys, vals],
                          [np.ones(n_rows, np.uint8), np.ones(n_rows, np.uint8)])
        g = ffi.HashAgg(glib, [T_I64, T_I64], [0], calls, 1, append_only=True,
                        state_capacity_hint=1024)
        o = ffi.HashAgg(oracle(), [T_I64, T_I64], [0], calls, 1,
                        append_only=True)
        try:
            assert L.rw_agg_debug_set_span_tiles(g.h, span_tiles) == 0
            cc = chunk.to_c()
            h = L.rw_agg_bench_preload(g.h, ctypes.byref(cc))
            assert h, glib.last_error()
            # two launches into one epoch: the second meets existing groups
            for _ in range(2):
                assert L.rw_agg_bench_apply(g.h, h) == 0, glib.last_error()
                o.push(chunk)
            g.flush(1)
            o.flush(1)
            got = rows_sorted(g.poll_all())
            want = rows_sorted(o.poll_all())
            assert got.shape == want.shape and (got == want).all(), (
                f"{name} span_tiles={span_tiles} n={n_rows} [{what}]: GPU\n"
                f"{got[:6]}\nvs oracle\n{want[:6]}")
        finally:
            g.close()
            o.close()
