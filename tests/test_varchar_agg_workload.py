"""The seeded varchar group-by workload really contains what the GPU tests
(tests/test_varchar_agg.py) claim to exercise. Runs only the generator, the
CPU oracle on surrogate ids and a naive Python dict group-by on the strings
themselves (rwtest/varchar_agg.py) — no GPU. These are conditions on the
fixed seed, not measurements.
"""
import pytest

from rwtest import ffi
from rwtest import varchar as vc
from rwtest import varchar_agg as va


@pytest.fixture(scope="module")
def epochs():
    return va.make_workload()


def test_workload_shape(epochs):
    assert len(epochs) == 3 and all(len(ch) == 4 for ch in epochs)
    rows = [r for ch in epochs for c in ch for r in c.rows()]
    ops = [op for ch in epochs for c in ch for op in c.ops]
    for ch in epochs:
        for c in ch:
            assert c.n_rows in va.SIZES and c.types == va.TYPES
    n_del = sum(op == ffi.OP_DELETE for op in ops)
    assert 0.12 * len(ops) <= n_del <= 0.28 * len(ops), (n_del, len(ops))
    names = [r[va.COL_NAME] for r in rows]
    for s in vc.SPECIALS:
        assert s in names, s
    assert len(vc.LONG) > 255 and vc.PREFIX_A[:64] == vc.PREFIX_B[:64]
    assert any(r[va.COL_W] is None for r in rows)
    assert any(r[va.COL_W] is not None for r in rows)
    # every delete retracts a row that is live at that point
    live = []
    for ch in epochs:
        for c in ch:
            for op, row in zip(c.ops, c.rows()):
                if op == ffi.OP_INSERT:
                    live.append(row)
                else:
                    live.remove(row)


@pytest.mark.parametrize("group_key", [
    [va.COL_WINDOW, va.COL_NAME], [va.COL_NAME]], ids=["window_name", "name"])
def test_oracle_equals_naive_and_covers(epochs, group_key):
    run, _ = va.oracle_run(epochs, group_key)
    # the surrogate reference agrees with a group-by on the strings
    assert run.outs == va.naive_group_by(epochs, group_key)

    kw = len(group_key)
    npos = group_key.index(va.COL_NAME)
    n_delete = n_pairs = 0
    deleted, recreated = set(), set()
    keys_seen = set()
    for out in run.outs:
        toks = [op for op, _ in out]
        assert toks.count("U-") == toks.count("U+")
        n_pairs += toks.count("U-")
        n_delete += toks.count("-")
        for op, row in out:
            key = row[:kw]
            keys_seen.add(key)
            if op == "+" and key in deleted:
                recreated.add(key)
        # deletions take effect for the epochs AFTER this one
        deleted |= {row[:kw] for op, row in out if op == "-"}
    assert n_delete >= 20, n_delete
    assert n_pairs >= 20, n_pairs
    assert len(recreated) >= 5, len(recreated)
    names = {k[npos] for k in keys_seen}
    # a NULL-name group and an empty-string group, present and distinct
    assert None in names and b"" in names
    # both prefix strings as separate groups
    assert vc.PREFIX_A in names and vc.PREFIX_B in names
    assert vc.LONG in names and vc.UTF8 in names


def test_reencoded_drain_is_sorted_and_typed(epochs):
    """The re-encoded oracle drain the GPU spill test compares against:
    frames in key order, string keys decodable, DELETE frames present."""
    run, _ = va.oracle_run(epochs, [va.COL_WINDOW, va.COL_NAME])
    ot = va.out_types_of(va.TYPES, [va.COL_WINDOW, va.COL_NAME], va.CALLS)
    n_del = 0
    for buf in run.drains:
        frames = vc.decode_frames(buf)
        assert frames
        keys = [k for _, k, _ in frames]
        assert keys == sorted(keys)
        for put, key, val in frames:
            if put:
                row = vc.decode_row(val, ot)
                assert key == va.memcmp_i64(row[0]) + va.memcmp_str(row[1])
            else:
                n_del += 1
    assert n_del >= 20, n_del
