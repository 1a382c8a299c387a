"""Seeded insert/delete streams shared by the parity tests.

Each generator draws from the caller's numpy Generator in a fixed order, so
a test that passes its own seed and sizes gets the same stream every run.
`key_map` (optional) sends the drawn key index through a lookup table when
the chunk is built: the stream's shape stays, the keys land where the
caller wants them (tests/rwtest/slots.py).
"""
import numpy as np

from rwtest import ffi
from rwtest.ffi import T_I64


def retract_mix(rng, live, cols, p_delete):
    """Turn rows of freshly drawn `cols` (int arrays, edited in place) into
    deletes of earlier rows: with probability p_delete a row becomes the
    Delete of a random entry popped from `live`, else it stays an Insert
    and joins `live`. Returns the ops array."""
    n = len(cols[0])
    ops = np.zeros(n, np.uint8)
    for r in range(n):
        if live and rng.random() < p_delete:
            jx = int(rng.integers(0, len(live)))
            row = live.pop(jx)
            for c, v in zip(cols, row):
                c[r] = v
            ops[r] = ffi.OP_DELETE
        else:
            live.append(tuple(int(c[r]) for c in cols))
    return ops


def _mapped(col, key_map):
    if key_map is None:
        return col
    return np.asarray(key_map, np.int64)[np.asarray(col) % len(key_map)]


def join_mix_push(rng, live, pk0, n, key_space, p_delete, side=None,
                  key_map=None):
    """One (side, chunk) of a two-column (key, unique pk) join stream;
    deletes target rows of earlier pushes on the same side. `side` None
    draws it. live: {side: [(key, pk), ...]}."""
    if side is None:
        side = int(rng.integers(0, 2))
    keys = rng.integers(0, key_space, n)
    vals = np.arange(pk0, pk0 + n)
    ops = retract_mix(rng, live[side], [keys, vals], p_delete)
    n1 = np.ones(n, np.uint8)
    return side, ffi.Chunk([T_I64, T_I64], ops,
                           [_mapped(keys, key_map), vals], [n1, n1])


def topn_mix_chunk(rng, live, n, n_groups, ord_space, pk_space, p_delete,
                   key_map=None):
    """One (group, order value, pk) chunk of a GroupTopN stream with
    deletes of earlier rows."""
    gk = rng.integers(0, n_groups, n)
    ordv = rng.integers(0, ord_space, n)
    pk = rng.integers(0, pk_space, n)
    ops = retract_mix(rng, live, [gk, ordv, pk], p_delete)
    n1 = np.ones(n, np.uint8)
    return ffi.Chunk([T_I64, T_I64, T_I64], ops,
                     [_mapped(gk, key_map), ordv, pk], [n1, n1, n1])
