"""ctypes wrappers for the HashAgg key-table compaction entries
(include/rw_stream.h rw_hash_agg_compact / rw_hash_agg_state_stats; DESIGN.md
§19). The product library has them; the CPU oracle has no capacity and
needs no compaction call."""
import ctypes as C

RW_E_INVAL = -1


def compact_rc(lib, h):
    """(return code, slots given back) of rw_hash_agg_compact."""
    fn = lib.lib.rw_hash_agg_compact
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    got = C.c_uint64()
    rc = fn(h, C.byref(got))
    return rc, got.value


def compact(lib, h):
    """Give dead groups' slots back; returns their number."""
    rc, got = compact_rc(lib, h)
    if rc != 0:
        raise RuntimeError(f"rw_hash_agg_compact failed {rc}: "
                           f"{lib.last_error()}")
    return got


def state_stats(lib, h):
    """(slots_ready, groups_live, capacity); synchronises."""
    fn = lib.lib.rw_hash_agg_state_stats
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
    v = [C.c_uint64() for _ in range(3)]
    rc = fn(h, *[C.byref(x) for x in v])
    if rc != 0:
        raise RuntimeError(f"rw_hash_agg_state_stats failed {rc}: "
                           f"{lib.last_error()}")
    return tuple(x.value for x in v)


def ingest_mode(lib, h, on):
    fn = lib.lib.rw_hash_agg_ingest_mode
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int]
    rc = fn(h, 1 if on else 0)
    if rc != 0:
        raise RuntimeError(f"rw_hash_agg_ingest_mode failed {rc}: "
                           f"{lib.last_error()}")
