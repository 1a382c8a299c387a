"""numpy mirror of the device key hash (rw_amd.hip mix64 / hash_key) and of
the slot placement built on it, so tests can aim keys at chosen slots.

tests/test_slot_mirror.py pins the mirror to the library's exported
rw_debug_hash_key: if the hash changes that test fails, and the adversarial
key sets below do not silently turn into random ones.
"""
import numpy as np

_U = np.uint64
_GOLD = _U(0x9E3779B97F4A7C15)
_M1 = _U(0xBF58476D1CE4E5B9)
_M2 = _U(0x94D049BB133111EB)
_SEED = 0x20210401


def _u64(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64)


def mix64(x):
    """splitmix64 finalizer over a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x + _GOLD
        x = (x ^ (x >> _U(30))) * _M1
        x = (x ^ (x >> _U(27))) * _M2
        return x ^ (x >> _U(31))


def hash_key(words, nullmask=0):
    """Hash of keys given as a list of per-word int64 arrays (or scalars).
    nullmask: scalar or array, bit i = word i is NULL (its word is 0)."""
    words = [np.atleast_1d(_u64(w)) for w in words]
    nm = np.atleast_1d(np.asarray(nullmask, dtype=np.uint64))
    with np.errstate(over="ignore"):
        h = _U(_SEED) ^ (nm * _GOLD)
        h = np.broadcast_to(h, np.broadcast(h, words[0]).shape).copy()
        for w in words:
            h = mix64(h ^ w)
    return h


def _log2(cap):
    assert cap >= 1 and cap & (cap - 1) == 0, cap
    return cap.bit_length() - 1


def agg_home(h, cap):
    """HashAgg key table: low bits (table_find_or_insert)."""
    return h & _U(cap - 1)


def top_home(h, cap):
    """jslot_start: top bits. Join buckets, GroupTopN and the dedup tables."""
    assert cap >= 2
    return h >> _U(64 - _log2(cap))


def bloom_bit(h):
    """Index of the join bucket's bloom bit (jbloom_bit)."""
    return (h >> _U(32)) & _U(31)


def keys_with_home(home, cap, n, kind, fixed_prefix=(), nullmask=0,
                   start=1, avoid=()):
    """n distinct int64 values v, scanned upward from `start`, such that the
    key (*fixed_prefix, v) with `nullmask` has home slot `home` in a table
    of `cap` slots. kind: "agg" (low bits) or "top" (top bits)."""
    home_of = {"agg": agg_home, "top": top_home}[kind]
    avoid = set(int(a) for a in avoid)
    out = []
    lo = start
    block = min(max(4096, 4 * n * cap), 1 << 21)
    while len(out) < n:
        cand = np.arange(lo, lo + block, dtype=np.int64)
        words = [np.full(block, p, np.int64) for p in fixed_prefix] + [cand]
        hit = cand[home_of(hash_key(words, nullmask), cap) == _U(home)]
        out.extend(int(v) for v in hit if int(v) not in avoid)
        lo += block
        assert lo < start + (1 << 34), "no candidates found"
    return out[:n]
