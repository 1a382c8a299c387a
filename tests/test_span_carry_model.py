"""Host-side model of the dense agg kernel's span mapping and carried run.

With SPAN, `agg_apply_dense4_body` (rw_amd.hip) gives each wave
`span_tiles` adjacent 256-row tiles. A tile whose 256 rows are all in range
and all carry the tile's first key is "uniform": it folds into the wave's
carried run (key, per-lane value partials, length) without touching the
table. The carry is committed when a uniform tile with another key or a
non-uniform tile arrives, and at the end of the span; a non-uniform tile
then goes through the segmented-scan path (one commit per run of the tile,
modelled lane for lane in test_dense_scan_model.py and restated here at run
level) and leaves the carry empty.

This file restates that control flow at commit-set level — per-lane
partials and the commit-time wave reduction included — and fuzzes it
against a direct per-key reduction. It validates the ALGORITHM; the binary
is validated on hardware by tests/test_agg_span_apply.py.
"""
import numpy as np
import pytest

RPL = 4
LANES = 64
TILE = LANES * RPL
I64_MIN = -(1 << 63)
MASK = (1 << 64) - 1


def wrap_add(a, b):
    """i64 wrapping add, as the kernel's integer add behaves."""
    s = (a + b) & MASK
    return s - (1 << 64) if s >> 63 else s


def span_tiles_for(rows, grid_blocks):
    """HashAgg::span_tiles_for: fewest tiles per wave that cover the rows."""
    tiles = (rows + TILE - 1) // TILE
    waves = grid_blocks * 4
    return (tiles + waves - 1) // waves


def tile_runs(keys, vals, lo, hi):
    """The scan path at run level: one (key, max, sum, count) commit per
    maximal run of equal keys among rows [lo, hi)."""
    out = []
    i = lo
    while i < hi:
        j = i
        mx, sm = I64_MIN, 0
        while j < hi and keys[j] == keys[i]:
            mx = max(mx, vals[j])
            sm = wrap_add(sm, vals[j])
            j += 1
        out.append((keys[i], mx, sm, j - i))
        i = j
    return out


def span_commits(keys, vals, span_tiles):
    """All commits of one launch: list of (key, max, sum, count)."""
    n = len(keys)
    total_tiles = (n + TILE - 1) // TILE
    n_waves = (total_tiles + span_tiles - 1) // span_tiles
    commits = []
    for wave in range(n_waves):
        first = wave * span_tiles
        iters = min(span_tiles, total_tiles - first)
        carry = None  # [key, per-lane max, per-lane sum, length]

        def commit_carry():
            key, lmax, lsum, length = carry
            mx, sm = I64_MIN, 0
            for lane in range(LANES):  # the commit-time wave reduction
                mx = max(mx, lmax[lane])
                sm = wrap_add(sm, lsum[lane])
            commits.append((key, mx, sm, length))

        for it in range(iters):
            lo = (first + it) * TILE
            hi = min(lo + TILE, n)
            k0 = keys[lo]
            uniform = hi - lo == TILE and all(
                keys[r] == k0 for r in range(lo, hi))
            if carry is not None and not (uniform and k0 == carry[0]):
                commit_carry()
                carry = None
            if uniform:
                if carry is None:
                    carry = [k0, [I64_MIN] * LANES, [0] * LANES, 0]
                for lane in range(LANES):
                    for r in range(RPL):
                        v = vals[lo + lane * RPL + r]
                        carry[1][lane] = max(carry[1][lane], v)
                        carry[2][lane] = wrap_add(carry[2][lane], v)
                carry[3] += TILE
                continue
            commits.extend(tile_runs(keys, vals, lo, hi))
        if carry is not None:
            commit_carry()
    return commits


def reduce_commits(commits):
    out = {}
    for k, mx, sm, n in commits:
        if k in out:
            o = out[k]
            out[k] = (max(o[0], mx), wrap_add(o[1], sm), o[2] + n)
        else:
            out[k] = (mx, sm, n)
    return out


def ground_truth(keys, vals):
    return reduce_commits((k, v, v, 1) for k, v in zip(keys, vals))


def make_keys(rng, style, n):
    if style == 0:  # q7: runs far longer than a tile
        return (np.arange(n) // int(rng.integers(600, 5000))).tolist()
    if style == 1:  # changes exactly on tile boundaries
        return (np.arange(n) // TILE // int(rng.integers(1, 4))).tolist()
    if style == 2:  # one-key stream with short foreign blips
        k = np.zeros(n, np.int64)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, n))
            k[at:at + int(rng.integers(1, 300))] = int(rng.integers(1, 3))
        return k.tolist()
    if style == 3:  # no uniform tile at all
        return rng.integers(0, 5, n).tolist()
    return (np.arange(n) // 1000).tolist()  # sorted runs of 1000


@pytest.mark.parametrize("seed", range(6))
def test_span_carry_model_fuzz(seed):
    rng = np.random.default_rng(seed)
    for trial in range(60):
        n = int(rng.choice([1024, 1025, 4096 + 3, 2048 + 255, 5000]))
        span_tiles = int(rng.choice([1, 2, 3, 8]))
        keys = make_keys(rng, trial % 5, n)
        vals = rng.integers(-(1 << 62), 1 << 62, n).tolist()
        got = reduce_commits(span_commits(keys, vals, span_tiles))
        assert got == ground_truth(keys, vals), (
            f"seed={seed} trial={trial} n={n} span_tiles={span_tiles}")


@pytest.mark.parametrize("span_tiles", [1, 2, 3, 8])
def test_one_key_span_commits_once(span_tiles):
    n = span_tiles * TILE  # exactly one wave's span, every tile uniform
    vals = list(range(n))
    commits = span_commits([7] * n, vals, span_tiles)
    assert commits == [(7, n - 1, sum(vals), n)]


def test_key_change_between_uniform_tiles_commits_per_run():
    keys = [1] * (2 * TILE) + [2] * TILE
    commits = span_commits(keys, [5] * len(keys), 8)
    assert [(c[0], c[3]) for c in commits] == [(1, 2 * TILE), (2, TILE)]


def test_span_policy_keeps_one_tile_per_wave_up_to_2m_rows():
    # the launch grid is capped at 2048 blocks of 4 waves
    def grid(rows):
        return min((rows // RPL + 255) // 256, 2048) or 1

    for rows in (1024, 1 << 20, 2 << 20):
        assert span_tiles_for(rows, grid(rows)) == 1
    assert span_tiles_for(16 << 20, grid(16 << 20)) == 8
