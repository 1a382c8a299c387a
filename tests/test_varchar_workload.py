"""The seeded q8-shaped varchar workload really contains what the GPU tests
(tests/test_varchar_join.py) claim to exercise. Runs only the generator and
the CPU oracle on surrogate ids (rwtest/varchar.py) — no GPU. These are
conditions on the fixed seed, not measurements.
"""
from collections import Counter

from rwtest import ffi
from rwtest import varchar as vc


def _run():
    epochs = vc.q8_workload()
    tl, tr = vc.schema_types(vc.Q8_LEFT), vc.schema_types(vc.Q8_RIGHT)
    outs, _, _ = vc.oracle_run(ffi.JOIN_INNER, tl, tr, vc.Q8_KW, epochs)
    return epochs, outs


def test_q8_workload_inputs_and_outputs():
    epochs, outs = _run()
    pushes = [p for chunks in epochs for p in chunks]
    assert len(pushes) == len(outs)

    # -- the plain multiset compare is valid on this stream: the oracle's
    # adjacent-no-op elimination (order dependent, so a parallel emitter
    # cannot reproduce it) removed nothing, and a row-at-a-time join on
    # the strings themselves agrees with the surrogate run
    assert outs == vc.naive_inner_join(epochs)

    # -- sizes the GPU tests promise
    per_side = Counter()
    for side, c in pushes:
        assert 64 <= c.n_rows <= 512
        per_side[side] += c.n_rows
    assert all(500 <= n <= 2500 for n in per_side.values()), per_side

    # -- deletes: hit a live row; some hit a row of the SAME chunk
    live = {0: Counter(), 1: Counter()}
    hits = same_chunk = 0
    for side, c in pushes:
        before = live[side].copy()
        for op, row in zip(c.ops, c.rows()):
            if op == ffi.OP_INSERT:
                live[side][row] += 1
            else:
                assert live[side][row] > 0, "delete of a row that is not live"
                live[side][row] -= 1
                hits += 1
                if before[row] == 0:
                    same_chunk += 1
    assert hits >= 50, hits
    assert same_chunk >= 1, same_chunk
    # both sides retract
    for s in (0, 1):
        assert any(op == ffi.OP_DELETE
                   for sd, c in pushes if sd == s for op in c.ops)

    # -- the all-insert batch: a probe row with >= 2 matches and one with 0
    gi = vc.Q8_ALL_INSERT[0]
    side, c = pushes[gi]
    assert side == ffi.SIDE_RIGHT
    assert all(op == ffi.OP_INSERT for op in c.ops)
    assert c.n_rows >= 64
    per_pk = Counter(row[-1] for _, row in outs[gi])  # auction pk is last
    in_pks = [row[2] for row in c.rows()]
    assert any(per_pk[pk] >= 2 for pk in in_pks), "no multi-match probe row"
    assert any(per_pk[pk] == 0 for pk in in_pks), "no zero-match probe row"

    # -- the string cases, in the INPUT ...
    in_names = [row[1] for sd, ch in pushes if sd == 0 for row in ch.rows()]
    for s in vc.SPECIALS:
        assert s in in_names, s
    assert len(vc.LONG) > 255 and vc.PREFIX_A[:64] == vc.PREFIX_B[:64]
    assert vc.UTF8.decode() and len(vc.UTF8) > len(vc.UTF8.decode())

    # -- ... and in the emitted OUTPUT (name is output column 1)
    out_rows = [row for o in outs for _, row in o]
    out_names = [row[1] for row in out_rows]
    for s in vc.SPECIALS:
        assert s in out_names, f"{s!r} never emitted"
    # two different person rows with equal (non-NULL) strings both emitted
    by_name = {}
    for row in out_rows:
        if row[1] is not None:
            by_name.setdefault(row[1], set()).add((row[0], row[2]))
    assert any(len(v) >= 2 for v in by_name.values())
    # retractions are emitted too (deletes carry the string)
    assert any(op == "-" and row[1] for o in outs for op, row in o)
