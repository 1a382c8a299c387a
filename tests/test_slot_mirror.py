"""The numpy hash mirror (rwtest/slots.py) against the library's exported
rw_debug_hash_key — a pure host function, so this runs without a GPU."""
import ctypes as C

import numpy as np

from rwtest import slots

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _lib_hash():
    import risingwave_amd

    L = C.CDLL(risingwave_amd.lib_path())
    L.rw_debug_hash_key.restype = C.c_uint64
    L.rw_debug_hash_key.argtypes = [C.POINTER(C.c_int64), C.c_uint32, C.c_int]

    def h(words, nullmask):
        arr = (C.c_int64 * len(words))(*words)
        return L.rw_debug_hash_key(arr, nullmask, len(words))

    return h


def test_hash_mirror_matches_library():
    lib_hash = _lib_hash()
    rng = np.random.default_rng(2021)
    edge = [0, -1, I64_MIN, I64_MAX]
    cases = []
    for kw in (1, 2, 3, 4):
        for e in edge:  # every edge word at every position, every null mask
            for pos in range(kw):
                for nm in range(1 << kw):
                    w = [int(x) for x in rng.integers(I64_MIN, I64_MAX, kw)]
                    w[pos] = e
                    cases.append((w, nm))
        cases.extend(([e] * kw, 0) for e in edge)
        for _ in range(250):
            w = [int(x) for x in rng.integers(I64_MIN, I64_MAX, kw,
                                              endpoint=True)]
            cases.append((w, int(rng.integers(0, 1 << kw))))
    assert len(cases) >= 1000
    for kw in (1, 2, 3, 4):
        sel = [(w, nm) for w, nm in cases if len(w) == kw]
        cols = [np.array([w[i] for w, _ in sel], np.int64) for i in range(kw)]
        nms = np.array([nm for _, nm in sel], np.uint64)
        got = slots.hash_key(cols, nms)
        want = np.array([lib_hash(w, nm) for w, nm in sel], np.uint64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (
            f"KW={kw}: mirror != rw_debug_hash_key for {sel[int(bad[0])]}: "
            f"{int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}")


def test_keys_with_home_places_keys():
    lib_hash = _lib_hash()
    for kind, cap, home in [("agg", 64, 63), ("agg", 64, 0), ("top", 8, 7),
                            ("top", 2, 1), ("top", 65536, 65535)]:
        ks = slots.keys_with_home(home, cap, 5, kind)
        assert len(set(ks)) == 5
        for k in ks:
            h = lib_hash([k], 0)
            bits = cap.bit_length() - 1
            got = h & (cap - 1) if kind == "agg" else h >> (64 - bits)
            assert got == home
    ks = slots.keys_with_home(3, 8, 4, "top", fixed_prefix=(7,), nullmask=0)
    for k in ks:
        assert lib_hash([7, k], 0) >> 61 == 3
    assert int(slots.bloom_bit(slots.hash_key([np.int64(5)]))[0]) == \
        (lib_hash([5], 0) >> 32) & 31
