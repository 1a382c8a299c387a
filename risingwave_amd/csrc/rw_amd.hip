// rw_amd.hip — MI355X-native (gfx950) stream HashAgg + HashJoin executors.
//
// PRODUCT PATH. Implements the C-ABI of include/rw_stream.h with all state
// resident in HBM and all per-row work in HIP kernels. The
// reference semantics being implemented (cited per function below) are those
// of /root/reference/src/stream/src/executor/{aggregate/hash_agg.rs,
// hash_join.rs}; the DESIGN is MI355X-first: SoA layouts, coalesced loads,
// open-addressed HBM tables, wave-level pre-aggregation, atomic-cursor
// emission (epoch outputs are order-free row multisets, matching the
// reference's own nondeterminism bar).
//
// There is NO CPU fallback: every entry point requires a visible GPU and
// fails loudly otherwise (RW_E_NOGPU).
//
// Round-1 kernel scope: group keys / join keys of 1..4 i64
// words (i64/timestamp columns), agg calls count(*)/count/sum/sum0 (i64) and
// append-only min/max (i64); join types Inner (incl. append-only) with
// optional i64 comparison condition. Everything else returns RW_E_INVAL with
// a message — the oracle covers it until the kernels land.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "../../include/rw_chunkbuild.hpp"
#include "../../include/rw_codec.hpp"
#include "../../include/rw_stream.h"
#include "../../include/rw_varlen.hpp"
#include "../../include/rw_xpayload.hpp"
#include "rw_devmem.hpp"

#define WAVE 64

static thread_local std::string g_err;

#define FAIL(code, ...)                                  \
    do {                                                 \
        char _b[256];                                    \
        snprintf(_b, sizeof _b, __VA_ARGS__);            \
        g_err = _b;                                      \
        return code;                                     \
    } while (0)

#define HIP_TRY(x)                                                          \
    do {                                                                    \
        hipError_t _e = (x);                                                \
        if (_e != hipSuccess)                                               \
            FAIL(RW_E_INTERNAL, "HIP error %s at %s:%d", hipGetErrorString(_e), \
                 __FILE__, __LINE__);                                       \
    } while (0)

// An executor's staging batch (AggBatch / JoinBatchDev), re-made for `cap`
// rows of `val_bytes`-wide value cells: everything old is freed first, so
// the peak stays at one batch.
template <class Batch>
static int stage_regrow(DevOwner& mem, Batch& b, int n_cols, size_t cap,
                        size_t val_bytes) {
    for (int i = 0; i < n_cols; i++) {
        mem.release(&b.col_vals[i]);
        mem.release(&b.col_valid[i]);
    }
    mem.release(&b.ops);
    mem.release(&b.vis);
    for (int i = 0; i < n_cols; i++) {
        HIP_TRY(mem.alloc(&b.col_vals[i], cap * val_bytes));
        HIP_TRY(mem.alloc(&b.col_valid[i], cap));
    }
    HIP_TRY(mem.alloc(&b.ops, cap));
    HIP_TRY(mem.alloc(&b.vis, cap));
    return RW_OK;
}

// One host column's n values of `width` bytes (8, or 16 for decimals) and its
// valid bytes, to one slot of a staging batch.
static int upload_col(int64_t* d_vals, uint8_t* d_valid, const void* vals,
                      const uint8_t* valid, uint32_t n, size_t width,
                      hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(d_vals, vals, (size_t)n * width,
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_valid, valid, n, hipMemcpyHostToDevice, stream));
    return RW_OK;
}

// The tail of every chunk upload: ops, then vis (a null b.vis tells the
// kernels that every row is visible), then the row count. `b` is the caller's
// copy of its staging batch.
template <class Batch>
static int upload_ops_vis(Batch& b, const RwChunk* c, hipStream_t stream) {
    uint32_t n = c->n_rows;
    HIP_TRY(hipMemcpyAsync(b.ops, c->ops, n, hipMemcpyHostToDevice, stream));
    if (c->vis)
        HIP_TRY(hipMemcpyAsync(b.vis, c->vis, n, hipMemcpyHostToDevice, stream));
    else
        b.vis = nullptr;
    b.n_rows = n;
    return RW_OK;
}

// A caller-owned device batch (the bench preload handles): the
// kernel-argument struct, which is what the handle points at, and beside it
// the owner of the batch's buffers.
template <class Batch>
struct Owned : Batch {
    DevOwner mem;
};

static bool gpu_ok() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// 256-thread blocks for `work` items: at least 1, at most 2048 (G11: cap +
// grid-stride)
static int grid_for(uint32_t work) {
    uint32_t blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    return (int)(blocks ? blocks : 1);
}

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    // splitmix64 finalizer — internal hash placement only (free choice per
    // XxHash64 is cache placement, not output-visible)
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

__host__ __device__ __forceinline__ uint64_t hash_key(const int64_t* kw,
                                                      uint32_t nullmask,
                                                      int KW) {
    uint64_t h = 0x20210401u ^ (uint64_t)nullmask * 0x9e3779b97f4a7c15ULL;
    for (int i = 0; i < KW; i++) h = mix64(h ^ (uint64_t)kw[i]);
    return h;
}

__device__ __forceinline__ long long atomic_add_i64(long long* p, long long v) {
    return (long long)atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

__device__ __forceinline__ void atomic_min_i64(long long* p, long long v) {
    atomicMin(p, v);
}
__device__ __forceinline__ void atomic_max_i64(long long* p, long long v) {
    atomicMax(p, v);
}

// ---- decimal (device mirror of the exact-domain restatement in
// oracle/common.hpp; rust_decimal 1.40.0 layout — see include/rw_chunk.h
// RW_T_DECIMAL and DESIGN.md §9). Sums accumulate as exact signed 256-bit
// integers at scale 28 via per-word atomics with cascading carries. ----
struct DecValD {
    int special; // 0 normal, 1 NaN, 2 +Inf, 3 -Inf
    bool neg;
    uint32_t scale;
    uint64_t lo;
    uint32_t hi;
};

__device__ __forceinline__ DecValD dec_parse_d(int64_t a, int64_t b) {
    DecValD v{};
    uint32_t flags = (uint32_t)a;
    uint8_t b0 = (uint8_t)flags;
    if (b0 == 1 || b0 == 2 || b0 == 3) {
        v.special = b0;
        return v;
    }
    v.neg = (flags >> 31) & 1;
    v.scale = (flags >> 16) & 0xFF;
    uint32_t lo32 = (uint32_t)((uint64_t)a >> 32);
    uint32_t mid = (uint32_t)b;
    v.hi = (uint32_t)((uint64_t)b >> 32);
    v.lo = ((uint64_t)mid << 32) | lo32;
    return v;
}

__device__ __forceinline__ void dec_serialize_d(const DecValD& v, long long* a,
                                                long long* b) {
    if (v.special) {
        *a = (long long)(uint32_t)v.special;
        *b = 0;
        return;
    }
    uint32_t flags = (v.scale << 16) | ((uint32_t)v.neg << 31);
    *a = (long long)(((uint64_t)(uint32_t)v.lo << 32) | flags);
    *b = (long long)(((uint64_t)v.hi << 32) | (uint32_t)(v.lo >> 32));
}

__device__ __forceinline__ uint64_t dec_pow10_d(int k) {
    uint64_t p = 1;
    while (k-- > 0) p *= 10;
    return p;
}

// addend words = sign * mantissa96 * 10^(28-scale) (two's complement i256)
__device__ __forceinline__ void dec_addend_d(const DecValD& v, uint64_t w[4]) {
    int k = 28 - (int)v.scale;
    uint64_t pa = dec_pow10_d(k / 2), pb = dec_pow10_d(k - k / 2);
    w[0] = v.lo;
    w[1] = v.hi;
    w[2] = w[3] = 0;
    for (int t = 0; t < 2; t++) {
        uint64_t p = t ? pb : pa;
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; i++) {
            unsigned __int128 x = (unsigned __int128)w[i] * p + c;
            w[i] = (uint64_t)x;
            c = x >> 64;
        }
    }
    if (v.neg) {
        unsigned __int128 c = 1;
        for (int i = 0; i < 4; i++) {
            unsigned __int128 x = (unsigned __int128)(~w[i]) + c;
            w[i] = (uint64_t)x;
            c = x >> 64;
        }
    }
}

// per-word atomic accumulation with cascading carries (mod 2^256 two's
// complement — negative addends just work)
__device__ __forceinline__ void dec_i256_atomic_add(
    unsigned long long* base, size_t cap, uint32_t slot, const uint64_t w[4]) {
    unsigned long long carry = 0;
    for (int k = 0; k < 4; k++) {
        unsigned long long add = (unsigned long long)w[k] + carry;
        carry = add < w[k] ? 1 : 0;
        if (add) {
            unsigned long long old = atomicAdd(&base[(size_t)k * cap + slot],
                                               add);
            if (old + add < add) carry += 1;
        }
    }
}

// exact conversion of the slot's i256 sum back to a decimal at out_scale;
// false when the mantissa exceeds 96 bits (the reference's order-dependent
// precision-loss rescale domain)
__device__ __forceinline__ bool dec_from_sum_d(const unsigned long long* base,
                                               size_t cap, uint32_t slot,
                                               uint32_t out_scale,
                                               DecValD* out) {
    uint64_t a[4];
    for (int k = 0; k < 4; k++) a[k] = base[(size_t)k * cap + slot];
    bool neg = a[3] >> 63;
    if (neg) {
        unsigned __int128 c = 1;
        for (int k = 0; k < 4; k++) {
            unsigned __int128 x = (unsigned __int128)(~a[k]) + c;
            a[k] = (uint64_t)x;
            c = x >> 64;
        }
    }
    int k = 28 - (int)out_scale;
    for (int t = 0; t < 2; t++) {
        uint64_t p = t ? dec_pow10_d(k - k / 2) : dec_pow10_d(k / 2);
        if (p == 1) continue;
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; i--) {
            unsigned __int128 cur = (rem << 64) | a[i];
            a[i] = (uint64_t)(cur / p);
            rem = cur % p;
        }
        if (rem != 0) return false;
    }
    if (a[3] || a[2] || (a[1] >> 32)) return false;
    out->special = 0;
    out->neg = neg && (a[0] | a[1]);
    out->scale = out_scale;
    out->lo = a[0];
    out->hi = (uint32_t)a[1];
    return true;
}

// rust_decimal PartialEq compares VALUES (1.2 == 1.20)
__device__ __forceinline__ bool dec_value_eq_d(int64_t a0, int64_t a1,
                                               int64_t b0, int64_t b1) {
    DecValD x = dec_parse_d(a0, a1), y = dec_parse_d(b0, b1);
    if (x.special || y.special) return x.special == y.special;
    uint64_t wx[4], wy[4];
    dec_addend_d(x, wx);
    dec_addend_d(y, wy);
    return wx[0] == wy[0] && wx[1] == wy[1] && wx[2] == wy[2] &&
           wx[3] == wy[3];
}

// slot states
#define SLOT_EMPTY 0u
#define SLOT_CLAIMED 1u
#define SLOT_READY 2u

// All cross-lane-shared table words use relaxed AGENT-scope atomics (sc1:
// L1-bypassing, write-through to the coherent point) — the guide's R1/R2
// hand-off forms. The claim path is R1: sc1 key stores -> s_waitcnt vmcnt(0)
// drain -> sc1 READY store; readers use sc1 loads throughout, which per the
// microarch visibility table replace the acquire when the producer stored
// sc1. No acquire/release fences anywhere on the hot path.
#define RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ uint32_t ld_u32(const uint32_t* p) {
    return __hip_atomic_load((uint32_t*)p, RLX);
}
__device__ __forceinline__ void st_u32(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, RLX);
}
__device__ __forceinline__ int64_t ld_i64(const int64_t* p) {
    return (int64_t)__hip_atomic_load((unsigned long long*)p, RLX);
}
__device__ __forceinline__ void st_i64(int64_t* p, int64_t v) {
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)v, RLX);
}

// AggTableDev::counters: words, and the fused apply's arrival-ticket shards
#define AGG_FUSE_SHARDS 64u
#define AGG_CTR_SHARD0 32u
#define AGG_CTR_WORDS (AGG_CTR_SHARD0 + 32u * AGG_FUSE_SHARDS)

// Find-or-insert into an open-addressed key table (linear probe).
// key_nulls is a u32-per-slot null mask. Returns slot, or -1 on table-full.
__device__ __forceinline__ uint32_t table_find_or_insert(
    uint32_t* state, int64_t* keys, uint32_t* key_nulls, uint32_t cap_mask,
    const int64_t* kw, uint32_t nullmask, int KW) {
    uint32_t slot = (uint32_t)(hash_key(kw, nullmask, KW) & cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        uint32_t st = ld_u32(&state[slot]);
        if (st == SLOT_EMPTY) {
            uint32_t prev = atomicCAS(&state[slot], SLOT_EMPTY, SLOT_CLAIMED);
            if (prev == SLOT_EMPTY) {
                for (int i = 0; i < KW; i++) st_i64(&keys[(size_t)slot * KW + i], kw[i]);
                st_u32(&key_nulls[slot], nullmask);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // R1 drain
                st_u32(&state[slot], SLOT_READY);
                return slot;
            }
            st = prev;
        }
        while (st == SLOT_CLAIMED) {
            __builtin_amdgcn_s_sleep(1);
            st = ld_u32(&state[slot]);
        }
        // st == SLOT_READY
        bool eq = ld_u32(&key_nulls[slot]) == nullmask;
        for (int i = 0; eq && i < KW; i++)
            eq = ld_i64(&keys[(size_t)slot * KW + i]) == kw[i];
        if (eq) return slot;
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

// Find-only (no insert). Returns slot or -1.
__device__ __forceinline__ uint32_t table_find(const uint32_t* state,
                                               const int64_t* keys,
                                               const uint32_t* key_nulls,
                                               uint32_t cap_mask, const int64_t* kw,
                                               uint32_t nullmask, int KW) {
    uint32_t slot = (uint32_t)(hash_key(kw, nullmask, KW) & cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        uint32_t st = ld_u32(&state[slot]);
        if (st == SLOT_EMPTY) return (uint32_t)-1;
        if (st == SLOT_READY) {
            bool eq = ld_u32(&key_nulls[slot]) == nullmask;
            for (int i = 0; eq && i < KW; i++)
                eq = ld_i64(&keys[(size_t)slot * KW + i]) == kw[i];
            if (eq) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

// ---------------------------------------------------------------------------
// HashAgg
// ---------------------------------------------------------------------------

#define MAX_CALLS 8
#define MAX_KW 4

struct AggCallDev {
    uint8_t kind;
    int32_t arg;  // column index in the input BATCH (gk cols ∥ arg cols ∥ sk cols)
    uint8_t minput; // materialized-input state (retractable min/max)
    int8_t mord;    // ordinal among minput calls
    uint8_t decimal; // RW_T_DECIMAL sum/count argument (16-B datums)
    int8_t dord;     // ordinal among decimal calls
};

// Device-side batch of input rows (SoA), i64-widened values. `stride` (in
// elements) lets the batch view row-major buffers — e.g. the join's output
// block, where column c of row r sits at vals[r*n_out + c] — without a
// repack; `valid_inverted` views a null-flag array as validity.
struct AggBatch {
    int64_t* col_vals[MAX_KW + MAX_CALLS]; // group key cols then arg cols
    uint8_t* col_valid[MAX_KW + MAX_CALLS];
    uint8_t* ops;
    uint8_t* vis; // may be null
    uint32_t n_rows;
    uint32_t stride = 1;
    uint8_t valid_inverted = 0;
    uint8_t dense = 0; // all rows visible+Insert+non-null (checked at upload)
    // DISTINCT dedup visibility (aggregate/distinct.rs): per call, byte per
    // row (indexed by r*stride) — 1 = hidden duplicate; null = no dedup
    const uint8_t* call_hidden[MAX_CALLS] = {};
};

// AoS layouts: one 64-B line per key slot, one packed record per row —
// a random probe touches 1 table line + 1 record line instead of the 8–10
// lines the SoA arrays cost (DESIGN §8 lever).
struct alignas(64) JoinSlot {
    uint32_t state; // SLOT_EMPTY/CLAIMED/READY
    uint32_t head;  // chain head row index, UINT32_MAX = none
    uint32_t nulls; // key null mask
    uint32_t _pad;
    long long key[4];
};
static_assert(sizeof(JoinSlot) == 64, "one cache line per slot");

// row record header; vals[n_cols] i64 follow at offset 16
struct JoinRowHdr {
    uint32_t alive; // CAS-claimed tombstone
    uint32_t next;
    uint32_t validbits; // bit c = column c non-NULL
    uint32_t degree;    // matches on the other side (outer/semi/anti types)
};

// host view of one row record copied off the device (the checkpoint drains)
struct HostRow {
    const uint8_t* rec;
    const JoinRowHdr& hdr() const { return *(const JoinRowHdr*)rec; }
    const int64_t* words() const {
        return (const int64_t*)(rec + sizeof(JoinRowHdr));
    }
    bool null(int c) const { return !((hdr().validbits >> c) & 1); }
    rwcodec::DatumC datum(uint8_t type, int c) const {
        return rwcodec::datum_of_word(type, null(c), words()[c]);
    }
};

struct JoinSideDev {
    JoinSlot* slots;     // 64-B AoS slots (GroupTopN tables)
    uint64_t* slots8;    // compact 8-B slots (join executor tables; see below)
    uint32_t cap_mask;
    uint8_t* rows;       // packed records, row_stride bytes each (16-B aligned)
    uint32_t row_stride;  // 16 + 8*n_cols
    uint32_t* row_cursor; // single counter
    uint32_t row_cap;
    // checkpoint-delta tracking (§8f-2): rows killed by deletes this epoch
    // (null for executors without spill, e.g. GroupTopN this round)
    uint32_t* killed;
    uint32_t* killed_cursor;
    uint32_t killed_cap;
    // degree-table delta tracking (§8f-2): pre-epoch rows whose degree
    // changed this epoch (null when the join type needs no degree here)
    uint32_t* deg_dirty_flag;
    uint32_t* deg_dirty_list;
    uint32_t* deg_dirty_n;
    // byte arena of the side's RW_T_VARCHAR cells (rw_varlen.hpp words
    // index it; null for sides without varchar columns). Last field: the
    // probe kernels never read it.
    uint8_t* arena;
};

__device__ __forceinline__ JoinRowHdr* jrow(const JoinSideDev& s, uint32_t r) {
    return (JoinRowHdr*)(s.rows + (size_t)r * s.row_stride);
}
__device__ __forceinline__ long long* jvals(JoinRowHdr* h) {
    return (long long*)((uint8_t*)h + 16);
}

// First slot for a join-table probe: TOP bits of the hash, so the slot index
// is monotone in h and a hash prefix maps to a CONTIGUOUS slot region.
// Distribution-equivalent to h & cap_mask; table layout depends on it.
__device__ __forceinline__ uint32_t jslot_start(uint64_t h, uint32_t cap_mask) {
    return (uint32_t)(h >> (64 - __popc(cap_mask)));
}

// ---- compact 8-B join slots: CHAINED buckets with bloom tags ----------
// The join executor's slot table packs {head u32 (high), bloom u32 (low)}
// into one u64; bloom==0 means empty. The KEY WORDS live only in the row
// records, and a bucket CHAINS every row whose hash lands on the slot —
// chained hashing, not open addressing. Rationale (round-2 roofline work):
// the round-1 64-B open-addressed slots made every probe/insert touch
// 1–3 random HBM lines (PMC: 500–1000 B/row vs the 128-B model), and even
// compact open addressing needs a verify read of the head record per
// insert. With buckets:
//  - INSERT = one 64-bit CAS on the slot (8-B table, 128–256 MB at q8
//    capacity -> Infinity-Cache-resident) — no probing, no verify read.
//  - MISS   = one slot load: the bloom bit (bit (h>>32)&31, set by every
//    insert, never cleared) rejects absent keys with ~k/32 false-positive
//    walks for a k-key bucket.
//  - MATCH  = walk the chain and filter by FULL key from the records the
//    match reads anyway (no tag-identity assumption anywhere).
// A bucket may mix keys (same-slot hash collisions), so every chain walk
// carries the key filter; deletes/cleans kill records individually.

__device__ __forceinline__ uint32_t jbloom_bit(uint64_t h) {
    return 1u << ((uint32_t)(h >> 32) & 31);
}
__device__ __forceinline__ uint32_t jhead_of(uint64_t packed) {
    return (uint32_t)(packed >> 32);
}
// head row of the bucket for hash h, or UINT32_MAX if the bloom rejects.
// sc1: coherent slot load (the side is mutated during this launch).
__device__ __forceinline__ uint32_t jbucket_head(const JoinSideDev& sd,
                                                 uint64_t h, bool sc1) {
    uint32_t slot = jslot_start(h, sd.cap_mask);
    uint64_t packed = sc1 ? __hip_atomic_load(&sd.slots8[slot], RLX)
                          : sd.slots8[slot];
    if (!((uint32_t)packed & jbloom_bit(h))) return UINT32_MAX;
    return jhead_of(packed);
}
// push row onto its bucket: record payload fully written by the caller
// (drained to the coherence point before the CAS lands, so a walker that
// sees the new head fetches real bytes). sc1_next: the launch has
// same-side walkers (mixed-op chunks) — store `next` coherently.
__device__ __forceinline__ void jbucket_insert(const JoinSideDev& sd,
                                               uint64_t h, uint32_t row,
                                               bool sc1_next) {
    uint32_t slot = jslot_start(h, sd.cap_mask);
    JoinRowHdr* hd = jrow(sd, row);
    uint64_t old = __hip_atomic_load(&sd.slots8[slot], RLX);
    for (;;) {
        uint32_t old_head =
            (uint32_t)old ? jhead_of(old) : UINT32_MAX; // bloom 0 = empty
        if (sc1_next) {
            st_u32(&hd->next, old_head);
            // R1 drain: same-launch walkers (mixed-op chunks) must fetch
            // real payload bytes once they see the new head. All-Insert
            // launches have NO same-side walkers — their visibility comes
            // from the inter-dispatch flush, so the pipeline-stalling
            // drain is skipped (sc1_next == false).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            hd->next = old_head;
        }
        uint64_t want =
            ((uint64_t)row << 32) | ((uint32_t)old | jbloom_bit(h));
        uint64_t prev = atomicCAS((unsigned long long*)&sd.slots8[slot], old,
                                  want);
        if (prev == old) return;
        old = prev;
    }
}

// key filter for chain walks given the record header pointer (buckets mix
// keys; every walk filters by full key)
__device__ __forceinline__ bool jhdr_key_eq(JoinRowHdr* hd,
                                            const uint8_t* key_cols, int KW,
                                            const int64_t* kw,
                                            uint32_t nullmask, bool sc1) {
    uint32_t vb = sc1 ? ld_u32(&hd->validbits) : hd->validbits;
    const long long* hv = (const long long*)((const uint8_t*)hd + 16);
    for (int i = 0; i < KW; i++) {
        uint8_t col = key_cols[i];
        bool valid = (vb >> col) & 1;
        if (valid == (bool)((nullmask >> i) & 1)) return false;
        if (valid) {
            long long v = sc1 ? ld_i64((const int64_t*)&hv[col]) : hv[col];
            if (v != kw[i]) return false;
        }
    }
    return true;
}

// own-side find-or-insert. The probe walk uses PLAIN cached loads: a slot's
// state and keys share one 64-B line, and the claim protocol drains the sc1
// key stores to the coherence point BEFORE the sc1 READY store — so any
// line fill that observes READY also contains the keys (same-line, written
// earlier at the coherence point), and a stale cached line can only show
// the older EMPTY/CLAIMED state, which funnels into the coherent CAS/spin
// path below. Keys never change once READY. This removes the per-visit sc1
// word loads that dominated the insert path (~0.45 ms/1M inserts measured).
__device__ __forceinline__ uint32_t jslot_find_or_insert(JoinSlot* slots,
                                                         uint32_t cap_mask,
                                                         const int64_t* kw,
                                                         uint32_t nullmask,
                                                         int KW) {
    uint32_t slot = jslot_start(hash_key(kw, nullmask, KW), cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        JoinSlot* sl = &slots[slot];
        uint32_t st = sl->state; // plain (fast path)
        if (st == SLOT_READY) {
            bool eq = sl->nulls == nullmask;
            for (int i = 0; eq && i < KW; i++) eq = sl->key[i] == kw[i];
            if (eq) return slot;
        } else {
            if (st == SLOT_EMPTY) {
                uint32_t prev = atomicCAS(&sl->state, SLOT_EMPTY, SLOT_CLAIMED);
                if (prev == SLOT_EMPTY) {
                    for (int i = 0; i < KW; i++)
                        st_i64((int64_t*)&sl->key[i], kw[i]);
                    st_u32(&sl->nulls, nullmask);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // R1 drain
                    st_u32(&sl->state, SLOT_READY);
                    return slot;
                }
                st = prev;
            } else {
                st = ld_u32(&sl->state); // sc1 refresh of a stale CLAIMED
            }
            while (st == SLOT_CLAIMED) {
                __builtin_amdgcn_s_sleep(1);
                st = ld_u32(&sl->state);
            }
            // coherent compare (the plain line may be stale here)
            bool eq = ld_u32(&sl->nulls) == nullmask;
            for (int i = 0; eq && i < KW; i++)
                eq = ld_i64((const int64_t*)&sl->key[i]) == kw[i];
            if (eq) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

// match-side find with plain cached loads (immutable during the launch)
__device__ __forceinline__ uint32_t jslot_find_cached(const JoinSlot* slots,
                                                      uint32_t cap_mask,
                                                      const int64_t* kw,
                                                      uint32_t nullmask, int KW) {
    uint32_t slot = jslot_start(hash_key(kw, nullmask, KW), cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        const JoinSlot* sl = &slots[slot];
        uint32_t st = sl->state;
        if (st == SLOT_EMPTY) return (uint32_t)-1;
        if (st == SLOT_READY) {
            bool eq = sl->nulls == nullmask;
            for (int i = 0; eq && i < KW; i++) eq = sl->key[i] == kw[i];
            if (eq) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

// sc1 variant of the find (append-only path mutates the match side)
__device__ __forceinline__ uint32_t jslot_find_sc1(const JoinSlot* slots,
                                                   uint32_t cap_mask,
                                                   const int64_t* kw,
                                                   uint32_t nullmask, int KW) {
    uint32_t slot = jslot_start(hash_key(kw, nullmask, KW), cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        const JoinSlot* sl = &slots[slot];
        uint32_t st = ld_u32(&sl->state);
        if (st == SLOT_EMPTY) return (uint32_t)-1;
        if (st == SLOT_READY) {
            bool eq = ld_u32(&sl->nulls) == nullmask;
            for (int i = 0; eq && i < KW; i++)
                eq = ld_i64((const int64_t*)&sl->key[i]) == kw[i];
            if (eq) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

__global__ void jslot_init_kernel(JoinSlot* slots, size_t cap) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        slots[i].state = SLOT_EMPTY;
        slots[i].head = UINT32_MAX;
    }
}

// DISTINCT dedup pass (aggregate/distinct.rs:131-158): per (group key,
// datum) a counter slot (JoinSlot layout; `head` is the count, initialized
// 0). An insert is visible iff the count rises 0→1, a delete iff it falls
// 1→0 — transition ownership via the atomic's return value, so concurrent
// duplicates resolve to the same net visibility multiset as the
// reference's sequential pass (the accumulators only see the net).
__global__ void dedup_init_kernel(JoinSlot* slots, size_t cap) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        slots[i].state = SLOT_EMPTY;
        slots[i].head = 0; // count
    }
}

__global__ void agg_dedup_kernel(AggBatch b, JoinSlot* slots,
                                 uint32_t cap_mask, int KW, int dslot,
                                 uint8_t* hidden, uint32_t* err,
                                 uint32_t* dirty_flag, uint32_t* dirty_list,
                                 uint32_t* dirty_n) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < b.n_rows;
         r += stride) {
        size_t rs = (size_t)r * b.stride;
        if (b.vis && !b.vis[r]) continue;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < KW; i++) {
            bool valid = b.col_valid[i][rs] ^ b.valid_inverted;
            kw[i] = valid ? b.col_vals[i][rs] : 0;
            nullmask |= (!valid) << i;
        }
        bool dvalid = b.col_valid[dslot][rs] ^ b.valid_inverted;
        kw[KW] = dvalid ? b.col_vals[dslot][rs] : 0;
        nullmask |= (!dvalid) << KW;
        uint32_t slot =
            jslot_find_or_insert(slots, cap_mask, kw, nullmask, KW + 1);
        if (slot == UINT32_MAX) {
            atomicExch(err, 4u); // dedup table full
            continue;
        }
        uint8_t op = b.ops[r];
        bool retract = (op == RW_OP_DELETE || op == RW_OP_UPDATE_DELETE);
        uint32_t old = retract ? atomicSub(&slots[slot].head, 1u)
                               : atomicAdd(&slots[slot].head, 1u);
        hidden[rs] = retract ? (old != 1) : (old != 0);
        // §8f-2 spill: record each (group, datum) touched this epoch, once
        // (the reference writes an update per touched datum at dedup(),
        // distinct.rs:158-185; the per-epoch drain nets those to one)
        if (ld_u32(&dirty_flag[slot]) == 0 &&
            atomicCAS(&dirty_flag[slot], 0u, 1u) == 0u) {
            uint32_t i = atomicAdd(dirty_n, 1u);
            dirty_list[i] = slot;
        }
    }
}

// Dedup-table checkpoint gather: pack the dirty slots' (key, count) into a
// compact buffer for one D2H copy, clearing the dirty flags on the way.
struct DedupDirtyRec {
    long long key[MAX_KW]; // group key words ++ datum (KW+1 used)
    uint32_t nulls;
    uint32_t count;
};
__global__ void dedup_gather_kernel(const JoinSlot* slots,
                                    uint32_t* dirty_flag,
                                    const uint32_t* dirty_list,
                                    const uint32_t* dirty_n,
                                    DedupDirtyRec* out) {
    uint32_t n = *dirty_n;
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        uint32_t s = dirty_list[i];
        const JoinSlot* sl = &slots[s];
        for (int w = 0; w < MAX_KW; w++) out[i].key[w] = sl->key[w];
        out[i].nulls = sl->nulls;
        out[i].count = sl->head;
        dirty_flag[s] = 0;
    }
}

// §8f-5 recovery: seed dedup counter slots from a netted spill replay.
// Keys in the netted map are unique, so each lane owns its slot; the slot
// index is reported back so the host can mark it persisted (the next drain
// must emit DELETE, not silence, when a restored count dies).
__global__ void dedup_restore_kernel(const long long* keys,
                                     const uint32_t* nulls,
                                     const uint32_t* counts, uint32_t n,
                                     int KW1, JoinSlot* slots,
                                     uint32_t cap_mask, uint32_t* out_slots,
                                     uint32_t* err) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        int64_t kw[MAX_KW];
        for (int i = 0; i < KW1; i++) kw[i] = keys[(size_t)r * KW1 + i];
        uint32_t slot =
            jslot_find_or_insert(slots, cap_mask, kw, nulls[r], KW1);
        if (slot == UINT32_MAX) {
            atomicExch(err, 4u);
            continue;
        }
        slots[slot].head = counts[r];
        out_slots[r] = slot;
    }
}

struct AggTableDev {
    uint32_t* state;
    int64_t* keys;      // [cap * KW]
    uint32_t* key_nulls; // [cap]
    long long* acc;     // [n_calls][cap]
    uint8_t* has;       // [n_calls][cap] — any non-null input applied
    long long* prev;    // [n_calls][cap]
    uint8_t* prev_null; // [n_calls][cap]
    uint8_t* has_prev;  // [cap]
    uint32_t* dirty_flag;
    uint32_t* dirty_list;
    // [0]=dirty_count [1]=out_cursor [2]=overflow flag [3]=flush-kernel ticket
    // [4]=fused-apply arrival ticket [5]=largest dirty count a flush has seen
    // [AGG_CTR_SHARD0 + 32 s]=arrival ticket of shard s, one 128-B line each
    uint32_t* counters;
                        // [3]=flush arrival ticket (0 outside a flush)
    // flush output buffers (records of width gk+calls)
    long long* out_vals;
    uint8_t* out_nulls;
    uint8_t* out_ops;
    uint32_t out_capacity;
    uint32_t cap_mask;
    // materialized-input state (retractable min/max, aggregate/minput.rs):
    // shared row store + per-(minput call, slot) chain heads; rows carry
    // (arg value, stream key) and a CAS-claimed alive flag, mirroring the
    // state-table rows keyed [group, value, stream key]
    uint32_t* mheads;   // [n_minput][cap], UINT32_MAX = empty
    long long* mval;    // [mrow_cap]
    uint8_t* mval_null; // [mrow_cap]
    long long* msk;     // [n_sk][mrow_cap]
    uint8_t* msk_null;  // [n_sk][mrow_cap]
    uint32_t* mnext;
    uint32_t* malive;
    uint32_t* mcursor; // single counter
    uint32_t mrow_cap;
    int n_sk;
    // minput-table spill bookkeeping (§8f-2 round 2): owner of each mrow
    // + per-epoch kill list (deletes of pre-drain rows)
    uint32_t* mslot;          // [mrow_cap] owning group slot
    uint8_t* mcall;           // [mrow_cap] minput ordinal
    uint32_t* mkilled;        // [mkilled_cap]
    uint32_t* mkilled_cursor; // single counter
    uint32_t mkilled_cap;
    // decimal-sum state (exact i256 at scale 28):
    unsigned long long* dsum; // [n_dec][4][cap]
    uint32_t* dscl;           // [n_dec][cap] running max input scale
    long long* dspec;         // [n_dec][3][cap] NaN/+Inf/-Inf counts
    long long* out_vals2;     // [out_capacity][width] decimal high halves
    long long* prev2;         // [n_calls][cap] decimal high halves
    int n_dec;
};

// agg_apply: HashAggExecutor::apply_chunk (hash_agg.rs:332-409) as one
// grid-stride pass over a multi-chunk batch. Per row: group lookup
// (get_group_visibilities/touch_agg_groups collapse to find-or-insert),
// then AggregateFunction::update per call (general.rs:18-41,154-162) via
// atomics — order-free for count/sum/min/max over the epoch's row multiset.
// Wave-level segmented pre-aggregation: q7 input is date_time-monotone, so
// consecutive rows (= consecutive lanes) share the window slot. Each
// contiguous equal-slot run inside a wave is reduced with shuffles and its
// TAIL lane issues ONE atomic per call — cutting hot-slot atomics by up to
// 64× (the unsorted case degrades to runs of 1 = plain per-lane atomics,
// still correct). count/sum combine by +, min/max by min/max, null-presence
// by OR; all order-free, so the result is exactly the reference's.
template <int KW, int n_calls, bool DENSE>
__global__ void agg_apply_kernel(AggBatch b, AggTableDev t, AggCallDev c0,
                                 AggCallDev c1, AggCallDev c2, AggCallDev c3,
                                 uint32_t r0, uint32_t r1) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t iters = (r1 - r0 + stride - 1) / stride;
    int lane = threadIdx.x & 63;
    size_t cap = (size_t)t.cap_mask + 1;
    const uint32_t SLOT_NONE = (uint32_t)-1;

    // per-lane probe memo: with sorted input a head's key rarely changes
    // between grid-stride iterations — skip the (fabric-bound) table probe
    // and dirty re-check when it doesn't
    int64_t memo_kw[KW];
    for (int i = 0; i < KW; i++) memo_kw[i] = 0;
    uint32_t memo_null = 0;
    uint32_t memo_slot = (uint32_t)-1;
    bool memo_dirtied = false;

    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = r0 + it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = DENSE ? (r < r1) : ((r < r1) && !(b.vis && !b.vis[r]));
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < KW; i++) kw[i] = 0;
        size_t rs = (size_t)r * b.stride;
        if (active) {
            for (int i = 0; i < KW; i++) {
                bool valid = DENSE || (b.col_valid[i][rs] ^ b.valid_inverted);
                kw[i] = valid ? b.col_vals[i][rs] : 0;
                nullmask |= (!valid) << i;
            }
        }
        // run-head detection by neighbor key compare: only one lane per
        // contiguous equal-key run probes the table (q7 input is
        // window-sorted, so runs are long; unsorted degrades to per-lane)
        uint64_t act_b = __ballot(active);
        bool same = true;
        for (int i = 0; i < KW; i++) {
            int64_t pk = __shfl_up(kw[i], 1);
            same = same && (pk == kw[i]);
        }
        uint32_t pn = (uint32_t)__shfl_up((int)nullmask, 1);
        same = same && (pn == nullmask);
        bool prev_active = lane > 0 && ((act_b >> (lane - 1)) & 1);
        bool head = active && !(same && prev_active);
        uint32_t slot = SLOT_NONE;
        if (head) {
            bool memo_hit = memo_slot != SLOT_NONE && nullmask == memo_null;
            for (int i = 0; i < KW; i++) memo_hit = memo_hit && kw[i] == memo_kw[i];
            if (memo_hit) {
                slot = memo_slot;
            } else {
                slot = table_find_or_insert(t.state, t.keys, t.key_nulls,
                                            t.cap_mask, kw, nullmask, KW);
                if (slot == SLOT_NONE) atomicExch(&t.counters[2], 1u); // full
                memo_slot = slot;
                memo_null = nullmask;
                for (int i = 0; i < KW; i++) memo_kw[i] = kw[i];
                memo_dirtied = false;
            }
            // dirty tracking moved to the head (it owns the memo); exactly-
            // once overall is still the CAS's job
            if (slot != SLOT_NONE && !memo_dirtied) {
                if (ld_u32(&t.dirty_flag[slot]) == 0 &&
                    atomicCAS(&t.dirty_flag[slot], 0u, 1u) == 0u) {
                    uint32_t i = atomicAdd(&t.counters[0], 1u);
                    t.dirty_list[i] = slot;
                }
                memo_dirtied = true;
            }
        }
        uint64_t heads_b = __ballot(head);
        uint64_t le_mask = heads_b & (~0ULL >> (63 - lane));
        int run_start = 63 - __clzll(le_mask | 1ULL);
        // the shuffle MUST be executed by all lanes: ds_bpermute returns
        // undefined data when the SOURCE lane (the head) is exec-masked off,
        // so a divergent `if (!head) slot = shfl(...)` reads garbage
        uint32_t bcast_slot = (uint32_t)__shfl((int)slot, run_start);
        if (active && !head) slot = bcast_slot;
        int run_pos = lane - run_start;

        // per-lane contributions (identity when inactive / NULL arg)
        uint8_t op = (!DENSE && active && slot != SLOT_NONE) ? b.ops[r]
                                                             : RW_OP_INSERT;
        long long sign =
            (op == RW_OP_DELETE || op == RW_OP_UPDATE_DELETE) ? -1 : 1;
        bool contributing = active && slot != SLOT_NONE;
        long long v[4];
        uint8_t hasmask = 0;
        for (int ci = 0; ci < n_calls; ci++) {
            const AggCallDev& c = calls[ci];
            int col = KW + ci;
            bool arg_valid =
                contributing &&
                (DENSE || (b.col_valid[col][rs] ^ b.valid_inverted));
            if (c.minput) {
                // materialized-input ops are exact per-row chain mutations
                // (minput.rs apply_batch): no wave aggregation
                v[ci] = 0;
                if (contributing) {
                    uint32_t* headp = t.mheads + (size_t)c.mord * cap + slot;
                    bool valid = b.col_valid[col][rs] ^ b.valid_inverted;
                    long long val = valid ? b.col_vals[col][rs] : 0;
                    if (sign > 0) {
                        uint32_t row = atomicAdd(t.mcursor, 1u);
                        if (row >= t.mrow_cap) {
                            atomicExch(&t.counters[2], 3u); // minput store full
                        } else {
                            st_u32(&t.mslot[row], slot);
                            t.mcall[row] = (uint8_t)c.mord;
                            st_i64((int64_t*)&t.mval[row], val);
                            t.mval_null[row] = !valid;
                            for (int k = 0; k < t.n_sk; k++) {
                                int skc = KW + n_calls + k;
                                bool skv = b.col_valid[skc][rs] ^ b.valid_inverted;
                                st_i64((int64_t*)&t.msk[(size_t)k * t.mrow_cap + row],
                                       skv ? b.col_vals[skc][rs] : 0);
                                t.msk_null[(size_t)k * t.mrow_cap + row] = !skv;
                            }
                            st_u32(&t.malive[row], 1);
                            uint32_t old_head = ld_u32(headp);
                            for (;;) {
                                st_u32(&t.mnext[row], old_head);
                                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                                uint32_t prev = atomicCAS(headp, old_head, row);
                                if (prev == old_head) break;
                                old_head = prev;
                            }
                        }
                    } else {
                        // delete: CAS-kill one matching (value, stream key)
                        uint32_t row = ld_u32(headp);
                        while (row != UINT32_MAX) {
                            if (ld_u32(&t.malive[row])) {
                                bool eq = (t.mval_null[row] == (uint8_t)!valid) &&
                                          (!valid || ld_i64((const int64_t*)&t.mval[row]) == val);
                                for (int k = 0; eq && k < t.n_sk; k++) {
                                    int skc = KW + n_calls + k;
                                    uint8_t va = b.col_valid[skc][rs] ^ b.valid_inverted;
                                    uint8_t vb = !t.msk_null[(size_t)k * t.mrow_cap + row];
                                    eq = (va == vb) &&
                                         (!va || b.col_vals[skc][rs] ==
                                                     ld_i64((const int64_t*)&t.msk[(size_t)k * t.mrow_cap + row]));
                                }
                                if (eq && atomicCAS(&t.malive[row], 1u, 0u) == 1u) {
                                    uint32_t ki =
                                        atomicAdd(t.mkilled_cursor, 1u);
                                    if (ki < t.mkilled_cap)
                                        t.mkilled[ki] = row;
                                    else
                                        atomicExch(&t.counters[2], 3u);
                                    break;
                                }
                            }
                            row = ld_u32(&t.mnext[row]);
                        }
                    }
                }
                continue;
            }
            if (c.decimal) {
                // exact decimal sum (device restatement above): per-lane
                // atomics, no wave pre-reduction
                v[ci] = 0;
                if (contributing &&
                    (DENSE || (b.col_valid[col][rs] ^ b.valid_inverted))) {
                    const int64_t* dp = b.col_vals[col]; // 2 words/row
                    DecValD dv = dec_parse_d(dp[2 * rs], dp[2 * rs + 1]);
                    size_t dcap = cap;
                    if (dv.special) {
                        atomic_add_i64(
                            &t.dspec[((size_t)c.dord * 3 + (dv.special - 1)) *
                                         dcap +
                                     slot],
                            sign);
                    } else {
                        uint64_t w[4];
                        dec_addend_d(dv, w);
                        if (sign < 0) {
                            unsigned __int128 cc = 1;
                            for (int k = 0; k < 4; k++) {
                                unsigned __int128 x =
                                    (unsigned __int128)(~w[k]) + cc;
                                w[k] = (uint64_t)x;
                                cc = x >> 64;
                            }
                        }
                        dec_i256_atomic_add(
                            t.dsum + (size_t)c.dord * 4 * dcap, dcap, slot, w);
                        atomicMax(&t.dscl[(size_t)c.dord * dcap + slot],
                                  dv.scale);
                    }
                    t.has[(size_t)ci * cap + slot] = 1;
                }
                continue;
            }
            bool shown = contributing &&
                         !(b.call_hidden[ci] && b.call_hidden[ci][rs]);
            arg_valid = arg_valid && shown;
            switch (c.kind) {
                case RW_AGG_COUNT_STAR: v[ci] = shown ? sign : 0; break;
                case RW_AGG_COUNT: v[ci] = arg_valid ? sign : 0; break;
                case RW_AGG_SUM:
                case RW_AGG_SUM0:
                    v[ci] = arg_valid ? sign * b.col_vals[col][rs] : 0;
                    if (arg_valid) hasmask |= 1 << ci;
                    break;
                case RW_AGG_MIN:
                    v[ci] = arg_valid ? b.col_vals[col][rs] : INT64_MAX;
                    if (arg_valid) hasmask |= 1 << ci;
                    break;
                case RW_AGG_MAX:
                    v[ci] = arg_valid ? b.col_vals[col][rs] : INT64_MIN;
                    if (arg_valid) hasmask |= 1 << ci;
                    break;
            }
        }
        // segmented inclusive reduction over the runs; the run TAIL issues
        // one atomic per call (order-free combines: +, min, max, OR)
        for (int d = 1; d < 64; d <<= 1) {
            long long ov[4];
            uint8_t ohas;
            for (int ci = 0; ci < n_calls; ci++) ov[ci] = __shfl_up(v[ci], d);
            // hasmask must ALWAYS be shuffled: even in a DENSE batch the
            // per-lane masks differ when DISTINCT dedup hides rows (a
            // dense own-mask shortcut dropped the run's sum/min/max here
            // whenever the tail lane's own row was a hidden duplicate)
            ohas = (uint8_t)__shfl_up((int)hasmask, d);
            if (run_pos >= d) {
                for (int ci = 0; ci < n_calls; ci++) {
                    switch (calls[ci].kind) {
                        case RW_AGG_MIN: v[ci] = v[ci] < ov[ci] ? v[ci] : ov[ci]; break;
                        case RW_AGG_MAX: v[ci] = v[ci] > ov[ci] ? v[ci] : ov[ci]; break;
                        default: v[ci] += ov[ci];
                    }
                }
                hasmask |= ohas;
            }
        }
        // a run ends before a head, before a non-contributing lane, or at 63
        uint64_t cont_b = __ballot(contributing);
        uint64_t ends_after = (heads_b | ~cont_b) >> 1 | (1ULL << 63);
        bool tail = contributing && ((ends_after >> lane) & 1);
        if (tail) {
            for (int ci = 0; ci < n_calls; ci++) {
                if (calls[ci].minput || calls[ci].decimal) continue;
                long long* acc = t.acc + (size_t)ci * cap;
                uint8_t* has = t.has + (size_t)ci * cap;
                switch (calls[ci].kind) {
                    case RW_AGG_COUNT_STAR:
                    case RW_AGG_COUNT:
                        if (v[ci]) atomic_add_i64(&acc[slot], v[ci]);
                        break;
                    case RW_AGG_SUM:
                    case RW_AGG_SUM0:
                        if (hasmask & (1 << ci)) {
                            atomic_add_i64(&acc[slot], v[ci]);
                            if (!has[slot]) has[slot] = 1; // benign race
                        }
                        break;
                    case RW_AGG_MIN:
                        if (hasmask & (1 << ci)) {
                            atomic_min_i64(&acc[slot], v[ci]);
                            if (!has[slot]) has[slot] = 1;
                        }
                        break;
                    case RW_AGG_MAX:
                        if (hasmask & (1 << ci)) {
                            atomic_max_i64(&acc[slot], v[ci]);
                            if (!has[slot]) has[slot] = 1;
                        }
                        break;
                }
            }
        }
    }
}


// ---- dense 4-rows-per-lane apply (q7 fast path) ----
// Specialization for dense (all-visible/Insert/non-null), KW==1, unit-stride
// batches: each lane owns 4 consecutive rows loaded as 16-B pairs, combines
// lane-local equal-key segments, and the wave closes cross-lane runs with a
// segmented scan over lane suffixes — one table probe + one atomic set per
// committed run. Verified against a host-side lane simulation (30k random
// patterns) before hardware.

__device__ __forceinline__ long long agg4_unit(uint8_t kind, long long v) {
    switch (kind) {
        case RW_AGG_COUNT_STAR:
        case RW_AGG_COUNT: return 1;
        default: return v;
    }
}
__device__ __forceinline__ long long agg4_identity(uint8_t kind) {
    switch (kind) {
        case RW_AGG_MIN: return INT64_MAX;
        case RW_AGG_MAX: return INT64_MIN;
        default: return 0;
    }
}
__device__ __forceinline__ long long agg4_comb(uint8_t kind, long long a,
                                               long long b) {
    switch (kind) {
        case RW_AGG_MIN: return a < b ? a : b;
        case RW_AGG_MAX: return a > b ? a : b;
        default: return a + b;
    }
}

// Rows per lane. Measured on MI355X at q7 sizes: 4 → 37.8 G rows/s,
// 8 → 28.9, 16 → 23.0 — the VGPR cost of wider per-lane tiles outweighs
// the deeper load pipeline.
constexpr int RPL = 4;

template <int n_calls, int CS>
__device__ __forceinline__ void dense_load(const AggBatch& b,
                                           const AggCallDev* calls,
                                           uint32_t rb, uint32_t r1, bool* act,
                                           long long* k,
                                           long long (*cv)[n_calls]) {
    bool all_in = rb + RPL - 1 < r1;
    if (all_in) {
        // back-to-back b128 loads: RPL/2 per column, all in flight at once
        const ulonglong2* kp = (const ulonglong2*)(b.col_vals[0] + rb);
#pragma unroll
        for (int h = 0; h < RPL / 2; h++) {
            ulonglong2 kk = kp[h];
            k[2 * h] = (long long)kk.x;
            k[2 * h + 1] = (long long)kk.y;
        }
#pragma unroll
        for (int r = 0; r < RPL; r++) act[r] = true;
        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
            if (ci == CS) continue; // count-star carried as run length
            if (calls[ci].arg < 0) {
#pragma unroll
                for (int r = 0; r < RPL; r++) cv[r][ci] = 1;
                continue;
            }
            const ulonglong2* vp = (const ulonglong2*)(b.col_vals[1 + ci] + rb);
#pragma unroll
            for (int h = 0; h < RPL / 2; h++) {
                ulonglong2 vv = vp[h];
                cv[2 * h][ci] = agg4_unit(calls[ci].kind, (long long)vv.x);
                cv[2 * h + 1][ci] = agg4_unit(calls[ci].kind, (long long)vv.y);
            }
        }
    } else {
        for (int r = 0; r < RPL; r++) {
            act[r] = rb + r < r1;
            k[r] = act[r] ? b.col_vals[0][rb + r] : 0;
            _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                if (ci == CS) continue;
                cv[r][ci] = act[r]
                                ? agg4_unit(calls[ci].kind,
                                            calls[ci].arg < 0
                                                ? 1
                                                : b.col_vals[1 + ci][rb + r])
                                : 0;
            }
        }
    }
}

// CS >= 0 names a count-star call (arg < 0): its per-row contribution is
// the constant 1, so the run's value is the run LENGTH — carried as one
// u32 beside the scan instead of an i64 inside it (halves the scan's
// cross-lane traffic for q7's [max, count] shape and frees the VGPRs the
// count column held). CS == -1 is the generic path, unchanged.
//
// SPAN: each wave owns `span_tiles` ADJACENT 64xRPL-row tiles instead of
// grid-stride ones, and carries an open run across them. q7 keys arrive in
// runs far longer than a tile, so nearly every tile holds one key: such a
// uniform tile (every row in range, every key equal to the tile's first —
// RPL compares and one vote) folds into per-lane partials in registers
// with no scan, no table probe and no atomics. The carry is wave-reduced
// and committed (by lane 0, through the same `commit`) only when a tile
// with another key or a non-uniform tile arrives, or the span ends; a
// non-uniform tile then takes the segmented-scan path unchanged. All
// combiners are commutative and associative on i64 (wrapping add
// included), so the table state after the launch is bit-identical.
//
// PUBLISH (the fused-flush span kernel only, see its tail): `commit`'s two
// plain stores, the dirty_list entry and the has byte, become write-through
// agent-scope stores, so that the launch's last-arriving block can read them
// behind one acquire with no release fence in any producer.
template <int n_calls, int CS = -1, bool SPAN = false, bool PUBLISH = false>
__device__ __forceinline__ void agg_apply_dense4_body(
        const AggBatch& b, const AggTableDev& t, AggCallDev c0, AggCallDev c1,
        AggCallDev c2, AggCallDev c3, uint32_t r0, uint32_t r1,
        uint32_t span_tiles = 0) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    int lane = threadIdx.x & 63;
    size_t cap = (size_t)t.cap_mask + 1;
    const uint32_t SLOT_NONE = (uint32_t)-1;
    uint32_t stride_rows = (gridDim.x * blockDim.x) * RPL;
    uint32_t iters = (r1 - r0 + stride_rows - 1) / stride_rows;

    long long memo_key = 0;
    uint32_t memo_slot = SLOT_NONE;
    bool memo_dirtied = false;

    auto commit = [&](long long key, const long long* vals, uint32_t cnt) {
        (void)cnt;
        uint32_t slot;
        if (memo_slot != SLOT_NONE && key == memo_key) {
            slot = memo_slot;
        } else {
            int64_t kw1[1] = {key};
            slot = table_find_or_insert(t.state, t.keys, t.key_nulls, t.cap_mask,
                                        kw1, 0, 1);
            if (slot == SLOT_NONE) {
                atomicExch(&t.counters[2], 1u);
                return;
            }
            memo_slot = slot;
            memo_key = key;
            memo_dirtied = false;
        }
        if (!memo_dirtied) {
            if (ld_u32(&t.dirty_flag[slot]) == 0 &&
                atomicCAS(&t.dirty_flag[slot], 0u, 1u) == 0u) {
                uint32_t i = atomicAdd(&t.counters[0], 1u);
                if (PUBLISH) st_u32(&t.dirty_list[i], slot);
                else t.dirty_list[i] = slot;
            }
            memo_dirtied = true;
        }
        auto set_has = [&](uint8_t* has) {
            if (has[slot]) return;
            if (PUBLISH) __hip_atomic_store(&has[slot], (uint8_t)1, RLX);
            else has[slot] = 1;
        };
        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
            long long* acc = t.acc + (size_t)ci * cap;
            uint8_t* has = t.has + (size_t)ci * cap;
            if (ci == CS) {
                atomic_add_i64(&acc[slot], (long long)cnt);
                continue;
            }
            switch (calls[ci].kind) {
                case RW_AGG_MIN:
                    atomic_min_i64(&acc[slot], vals[ci]);
                    set_has(has);
                    break;
                case RW_AGG_MAX:
                    atomic_max_i64(&acc[slot], vals[ci]);
                    set_has(has);
                    break;
                case RW_AGG_SUM:
                case RW_AGG_SUM0:
                    atomic_add_i64(&acc[slot], vals[ci]);
                    set_has(has);
                    break;
                default:
                    atomic_add_i64(&acc[slot], vals[ci]);
            }
        }
    };

    uint32_t base = r0 + (blockIdx.x * blockDim.x + threadIdx.x) * RPL;
    if (SPAN) {
        // wave-uniform: this wave's tiles are [first, first + iters)
        const uint32_t tile_rows = 64 * RPL;
        uint32_t total_tiles = (r1 - r0 + tile_rows - 1) / tile_rows;
        uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)(threadIdx.x >> 6));
        uint32_t first = (blockIdx.x * (blockDim.x >> 6) + wave) * span_tiles;
        iters = first >= total_tiles ? 0
                : total_tiles - first < span_tiles ? total_tiles - first
                                                   : span_tiles;
        base = r0 + first * tile_rows + lane * RPL;
        stride_rows = tile_rows;
    }
    // the carried run (SPAN): key and length are wave-uniform, the value
    // calls are per-lane partials until the commit reduces them
    bool have_carry = false;
    long long carry_key = 0;
    uint32_t carry_n = 0;
    long long carry_v[n_calls];
    bool act[RPL];
    long long k[RPL];
    long long cv[RPL][n_calls]; // [row][call]
    // SPAN runs one extra, data-less trip that commits the last carry, so
    // the carry commit is inlined once
    for (uint32_t it = 0; it < iters + (SPAN ? 1u : 0u); it++) {
        uint32_t rb = base + it * stride_rows;
        if (SPAN) {
            const bool last = it == iters;
            bool uni = false;
            long long k0 = 0;
            if (!last) {
                dense_load<n_calls, CS>(b, calls, rb, r1, act, k, cv);
                // lane 0's first key, held in scalar registers
                k0 = (long long)(((unsigned long long)(uint32_t)
                                      __builtin_amdgcn_readfirstlane(
                                          (int)((unsigned long long)k[0] >> 32))
                                  << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane(
                                     (int)(unsigned long long)k[0]));
                bool mine = true;
#pragma unroll
                for (int r = 0; r < RPL; r++) mine = mine && act[r] && k[r] == k0;
                uni = __ballot(mine) == ~0ULL;
            }
            if (have_carry && !(uni && k0 == carry_key)) {
                long long tot[n_calls];
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
                    long long v = carry_v[ci];
                    for (int d = 32; d >= 1; d >>= 1)
                        v = agg4_comb(calls[ci].kind, v, __shfl_xor(v, d));
                    tot[ci] = v;
                }
                if (lane == 0) commit(carry_key, tot, carry_n);
                have_carry = false;
            }
            if (last) break;
            if (uni) {
                if (!have_carry) {
                    have_carry = true;
                    carry_key = k0;
                    carry_n = 0;
                    _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                        if (ci == CS) continue;
                        carry_v[ci] = agg4_identity(calls[ci].kind);
                    }
                }
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
#pragma unroll
                    for (int r = 0; r < RPL; r++)
                        carry_v[ci] =
                            agg4_comb(calls[ci].kind, carry_v[ci], cv[r][ci]);
                }
                carry_n += 64 * RPL;
                continue;
            }
        } else {
            dense_load<n_calls, CS>(b, calls, rb, r1, act, k, cv);
        }
        // lane-local segments over the RPL rows (inactive rows break runs)
        long long last_key = 0;
        bool any = false, has_bnd = false;
        long long cur_key = 0;
        long long cur[n_calls];
        uint32_t cur_n = 0, pre_n = 0;
        bool have_cur = false, have_pre = false;
        long long preq[n_calls];
        long long pre_key = 0;
        for (int r = 0; r < RPL; r++) {
            if (!act[r]) {
                if (have_cur) {
                    if (!have_pre) {
                        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                            if (ci == CS) continue;
                            preq[ci] = cur[ci];
                        }
                        pre_key = cur_key;
                        pre_n = cur_n;
                        have_pre = true;
                    } else {
                        commit(cur_key, cur, cur_n); // interior complete run
                    }
                    has_bnd = true;
                    have_cur = false;
                }
                continue;
            }
            any = true;
            if (have_cur && k[r] == cur_key) {
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
                    cur[ci] = agg4_comb(calls[ci].kind, cur[ci], cv[r][ci]);
                }
                cur_n++;
            } else {
                if (have_cur) {
                    if (!have_pre) {
                        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                            if (ci == CS) continue;
                            preq[ci] = cur[ci];
                        }
                        pre_key = cur_key;
                        pre_n = cur_n;
                        have_pre = true;
                    } else {
                        commit(cur_key, cur, cur_n);
                    }
                    has_bnd = true;
                }
                cur_key = k[r];
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
                    cur[ci] = cv[r][ci];
                }
                cur_n = 1;
                have_cur = true;
            }
        }
        // after the loop: `cur` (if live) is the open suffix run; `preq`
        // holds the first closed run (prefix). Gaps between same-key runs
        // are irrelevant: every partition of a key's rows commits correctly
        // under commutative combines.
        long long sufv[n_calls];
        bool have_suf = have_cur;
        long long suf_key = cur_key;
        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
            if (ci == CS) continue;
            sufv[ci] = have_cur ? cur[ci] : agg4_identity(calls[ci].kind);
        }
        uint32_t suf_n = have_cur ? cur_n : 0;
        last_key = have_suf ? suf_key : (have_pre ? pre_key : 0);
        bool lane_any = any;
        bool lane_has_bnd = has_bnd || (have_pre && have_suf);

        // inter-lane continuity
        long long prev_last = __shfl_up(last_key, 1);
        uint64_t act_b = __ballot(lane_any);
        bool prev_any = lane > 0 && ((act_b >> (lane - 1)) & 1);
        long long my_first = any ? (have_pre ? pre_key : suf_key) : 0;
        bool first_at_row0 = any && act[0] && k[0] == my_first;
        bool cont = lane_any && prev_any && first_at_row0 &&
                    my_first == prev_last;

        // scan over suffix values
        bool scan_head = !lane_any || lane_has_bnd || !cont;
        uint64_t heads_b = __ballot(scan_head);
        uint64_t le_mask = heads_b & (~0ULL >> (63 - lane));
        int run_start = 63 - __clzll(le_mask | 1ULL);
        int run_pos = lane - run_start;
        long long incl[n_calls];
        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
            if (ci == CS) continue;
            incl[ci] = sufv[ci];
        }
        uint32_t incl_n = suf_n;
        for (int d = 1; d < 64; d <<= 1) {
            long long ov[n_calls];
            _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                if (ci == CS) continue;
                ov[ci] = __shfl_up(incl[ci], d);
            }
            uint32_t ov_n = CS >= 0 ? __shfl_up(incl_n, d) : 0u;
            if (run_pos >= d) {
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
                    incl[ci] = agg4_comb(calls[ci].kind, incl[ci], ov[ci]);
                }
                if (CS >= 0) incl_n += ov_n;
            }
        }
        long long incoming[n_calls];
        _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
            if (ci == CS) continue;
            incoming[ci] = __shfl_up(incl[ci], 1);
        }
        uint32_t incoming_n = CS >= 0 ? __shfl_up(incl_n, 1) : 0u;

        uint64_t cont_b = __ballot(cont);
        uint64_t bnd_b = __ballot(lane_has_bnd);
        bool next_cont = lane < 63 && ((cont_b >> (lane + 1)) & 1);
        bool next_closes = next_cont && ((bnd_b >> (lane + 1)) & 1);

        if (lane_any) {
            if (cont && lane_has_bnd) {
                // closer: commit the incoming run + own prefix
                long long tot[n_calls];
                _Pragma("unroll") for (int ci = 0; ci < n_calls; ci++) {
                    if (ci == CS) continue;
                    tot[ci] = agg4_comb(calls[ci].kind, incoming[ci], preq[ci]);
                }
                commit(pre_key, tot, incoming_n + pre_n);
            } else if (!cont && lane_has_bnd && have_pre) {
                commit(pre_key, preq, pre_n);
            }
            bool run_continues = next_cont;
            if (have_suf && !run_continues) {
                commit(suf_key, incl, incl_n);
            } else if (have_suf && next_closes) {
                // the next lane commits incoming (== this incl) + its prefix
            }
        }
    }
}

// Generic shapes (no count-star carried as run length): grid-stride tiles,
// no register cap — capping these at 64 VGPRs spilled 8 for +2.5%.
template <int n_calls>
__global__ void agg_apply_dense4_kernel(AggBatch b, AggTableDev t, AggCallDev c0,
                                        AggCallDev c1, AggCallDev c2,
                                        AggCallDev c3, uint32_t r0, uint32_t r1) {
    agg_apply_dense4_body<n_calls>(b, t, c0, c1, c2, c3, r0, r1);
}

// Count-star shapes, grid-stride: cap the register budget at 64 VGPRs so 8
// waves/SIMD are resident instead of the unbounded build's 7 — more
// latency-hiding on a latency-structured kernel. Measured 160.3 vs 135.0
// G rows/s over the unbounded CS build (the launch-bounds contract also
// changes scheduling, not just the register cap).
template <int n_calls, int CS>
__global__ __launch_bounds__(256, 8) void agg_apply_dense4_kernel_w8(
        AggBatch b, AggTableDev t, AggCallDev c0, AggCallDev c1, AggCallDev c2,
        AggCallDev c3, uint32_t r0, uint32_t r1) {
    agg_apply_dense4_body<n_calls, CS>(b, t, c0, c1, c2, c3, r0, r1);
}

// The same with the run-carrying span mapping (see agg_apply_dense4_body):
// the launch gives each wave `span_tiles` adjacent tiles.
//
// FUSE: the launch also runs the epoch's checkpoint flush, so an epoch step
// is one launch and one boundary. `fuse_arg` packs the call
// kinds (one per byte, bits 0-15) and row_count_index (bits 16-23); FUSE =
// false ignores it and is the kernel as it was.
//  - publish: `commit` stores the dirty_list entry and the has byte
//    write-through (PUBLISH above); the table words and the accumulators
//    are agent-scope atomics already. No fence in any producer.
//  - arrival: every wave drains its memory operations, the block meets at a
//    barrier, thread 0 draws a ticket (relaxed, agent scope) on its shard
//    word, the shard's last arriver one on counters[4].
//  - the block drawing the last top ticket is the flusher: thread 0 takes one
//    agent acquire and waits for it, the block learns "last" through one
//    LDS word behind the barrier, then runs agg_flush_fast_pass over every
//    dirty slot with stride 256 (right for any count, only slow for a large
//    one: HashAgg::fuse_allowed keeps those on the flush kernel).
//  - reset: the flusher zeroes counters[0], [1] and the ticket behind its
//    last pass; counters[2] stays sticky.
// Nothing waits on another block, and no step depends on where blocks run.
template <int KW, int NC, bool PRELOADED = false>
__device__ __forceinline__ void agg_flush_fast_pass(
        const AggTableDev& t, int row_count_index, uint32_t kinds, size_t cap,
        int lane, uint32_t i, uint32_t n_dirty, uint32_t slot = 0);

// The tail reads the table descriptor from the kernel-argument segment
// again (scalar loads) instead of keeping its ~30 further pointer SGPRs live
// across the main loop, whose register allocation it must leave alone. The
// descriptor is the kernel's second argument, behind the AggBatch.
__device__ __forceinline__ AggTableDev span_tail_table() {
    constexpr size_t off = (sizeof(AggBatch) + alignof(AggTableDev) - 1) /
                           alignof(AggTableDev) * alignof(AggTableDev);
    using kptr = const __attribute__((address_space(4))) char*;
    uint64_t a = (uint64_t)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + off);
    asm volatile("" : "+s"(a)); // not the main loop's copy of the same bytes
    // the asm's result counts as divergent; back to scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    auto* p = (const __attribute__((address_space(4))) AggTableDev*)(
        ((uint64_t)hi << 32) | lo);
    AggTableDev tt;
    __builtin_memcpy(&tt, p, sizeof(tt));
    return tt;
}

template <int n_calls, int CS, bool FUSE = false>
__global__ __launch_bounds__(256, 8) void agg_apply_dense4_kernel_span(
        AggBatch b, AggTableDev t, AggCallDev c0, AggCallDev c1, AggCallDev c2,
        AggCallDev c3, uint32_t r0, uint32_t r1, uint32_t span_tiles,
        uint32_t fuse_arg) {
    // the tail rebuilds its thread index from this scalar and the lane
    // number, so that no VGPR of the main loop has to carry threadIdx.x
    const uint32_t wave_id =
        FUSE ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
             : 0u;
    agg_apply_dense4_body<n_calls, CS, true, FUSE>(b, t, c0, c1, c2, c3, r0,
                                                   r1, span_tiles);
    if constexpr (FUSE) {
        __shared__ uint32_t s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const AggTableDev tt = span_tail_table();
        const uint32_t lane = __lane_id();
        const uint32_t tid = wave_id * 64u + lane;
        if (tid == 0) {
            // a launch's blocks end together, and one word takes about 88
            // returning atomics per microsecond: 2048 tickets on one word
            // measured 13 us per launch. Blocks draw on one of AGG_FUSE_SHARDS words, each
            // on a line of its own; a shard's last arriver zeroes it and
            // draws on the top word.
            const uint32_t sh = blockIdx.x % AGG_FUSE_SHARDS;
            const uint32_t members = gridDim.x / AGG_FUSE_SHARDS +
                                     (sh < gridDim.x % AGG_FUSE_SHARDS ? 1u : 0u);
            const uint32_t shards =
                gridDim.x < AGG_FUSE_SHARDS ? gridDim.x : AGG_FUSE_SHARDS;
            uint32_t* shard = &tt.counters[AGG_CTR_SHARD0 + 32u * sh];
            bool last = false;
            if (__hip_atomic_fetch_add(shard, 1u, RLX) == members - 1) {
                st_u32(shard, 0u);
                last = __hip_atomic_fetch_add(&tt.counters[4], 1u, RLX) ==
                       shards - 1;
            }
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            s_last = last;
        }
        __syncthreads();
        if (!s_last) return;
        const uint32_t n_dirty = ld_u32(&tt.counters[0]);
        const uint32_t kinds = fuse_arg & 0xffffu;
        const int rci = (int)((fuse_arg >> 16) & 0xffu);
        const size_t cap = (size_t)tt.cap_mask + 1;
        // four passes' dirty_list loads go out together (a q7 checkpoint has
        // at most 1024 dirty slots); the state loads of the four passes
        // together do not fit the kernel's 64 VGPRs
        for (uint32_t i0 = 0; i0 < n_dirty; i0 += 1024u) {
            uint32_t slot[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const uint32_t i = i0 + p * 256u + tid;
                slot[p] = i < n_dirty ? tt.dirty_list[i] : 0u;
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (i0 + p * 256u >= n_dirty) break; // block-uniform
                agg_flush_fast_pass<1, n_calls, true>(
                    tt, rci, kinds, cap, (int)lane, i0 + p * 256u + tid,
                    n_dirty, slot[p]);
            }
        }
        __syncthreads();
        if (tid == 0) {
            atomicMax(&tt.counters[5], n_dirty); // high-water mark
            atomicExch(&tt.counters[0], 0u);     // dirty count
            atomicExch(&tt.counters[1], 0u);     // out cursor
            atomicExch(&tt.counters[4], 0u);     // arrival ticket
        }
    }
}

// agg_flush: flush_data's emit-on-update branch (hash_agg.rs:475-501) +
// OnlyOutputIfHasInput::infer_change_type (agg_group.rs:131-165) +
// reset-at-zero (agg_group.rs:431-445). One thread per dirty slot; Update
// writes the U−/U+ pair into consecutive reserved rows (pair adjacency).
__global__ void agg_flush_kernel(AggTableDev t, int KW, int n_calls,
                                 int row_count_index, AggCallDev c0, AggCallDev c1,
                                 AggCallDev c2, AggCallDev c3) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    uint32_t n_dirty = t.counters[0];
    uint32_t stride = gridDim.x * blockDim.x;
    size_t cap = (size_t)t.cap_mask + 1;
    int width = KW + n_calls;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_dirty;
         i += stride) {
        uint32_t slot = t.dirty_list[i];
        t.dirty_flag[slot] = 0;
        // current outputs (get_outputs, agg_group.rs:431-467)
        long long rc = t.acc[(size_t)row_count_index * cap + slot];
        if (rc < 0) rc = 0; // row_count_of clamp (agg_group.rs:63-75)
        long long curr[MAX_CALLS];
        long long curr2[MAX_CALLS];
        uint8_t curr_null[MAX_CALLS];
        for (int ci = 0; ci < n_calls; ci++) {
            const AggCallDev& c = calls[ci];
            long long* acc = t.acc + (size_t)ci * cap;
            uint8_t* has = t.has + (size_t)ci * cap;
            curr2[ci] = 0;
            if (rc == 0) {
                // reset value states (agg_state.rs:149-155)
                switch (c.kind) {
                    case RW_AGG_MIN: acc[slot] = INT64_MAX; break;
                    case RW_AGG_MAX: acc[slot] = INT64_MIN; break;
                    default: acc[slot] = 0;
                }
                has[slot] = 0;
                if (c.decimal) {
                    for (int k = 0; k < 4; k++)
                        t.dsum[((size_t)c.dord * 4 + k) * cap + slot] = 0;
                    t.dscl[(size_t)c.dord * cap + slot] = 0;
                    for (int k = 0; k < 3; k++)
                        t.dspec[((size_t)c.dord * 3 + k) * cap + slot] = 0;
                }
            }
            if (c.decimal) {
                // exact decimal sum output (specials per decimal.rs:259-276)
                if (!has[slot]) {
                    curr[ci] = 0;
                    curr_null[ci] = 1;
                    continue;
                }
                long long nan = t.dspec[((size_t)c.dord * 3 + 0) * cap + slot];
                long long pinf = t.dspec[((size_t)c.dord * 3 + 1) * cap + slot];
                long long ninf = t.dspec[((size_t)c.dord * 3 + 2) * cap + slot];
                DecValD r2{};
                if (nan > 0 || (pinf > 0 && ninf > 0)) {
                    r2.special = 1;
                } else if (pinf > 0) {
                    r2.special = 2;
                } else if (ninf > 0) {
                    r2.special = 3;
                } else if (!dec_from_sum_d(
                               t.dsum + (size_t)c.dord * 4 * cap, cap, slot,
                               t.dscl[(size_t)c.dord * cap + slot], &r2)) {
                    atomicExch(&t.counters[2], 5u); // outside exact domain
                    curr[ci] = 0;
                    curr_null[ci] = 1;
                    continue;
                }
                dec_serialize_d(r2, &curr[ci], &curr2[ci]);
                curr_null[ci] = 0;
                continue;
            }
            if (c.minput) {
                // output_first over the materialized rows (minput.rs:236-241):
                // min = value ASC NULLS LAST → smallest non-null, NULL if all
                // null; max = value DESC NULLS FIRST → NULL if any NULL row
                // (the reference's order types, test_utils/agg_executor.rs:
                // 96-99 + sort_util.rs NullsAre::Largest)
                uint32_t row = t.mheads[(size_t)c.mord * cap + slot];
                bool any = false, any_null = false;
                long long best = 0;
                while (row != UINT32_MAX) {
                    if (t.malive[row]) {
                        if (t.mval_null[row]) {
                            any_null = true;
                        } else {
                            long long v = t.mval[row];
                            if (!any) best = v;
                            else if (c.kind == RW_AGG_MIN) best = v < best ? v : best;
                            else best = v > best ? v : best;
                            any = true;
                        }
                    }
                    row = t.mnext[row];
                }
                if (c.kind == RW_AGG_MAX && any_null) {
                    curr[ci] = 0;
                    curr_null[ci] = 1;
                } else {
                    curr[ci] = best;
                    curr_null[ci] = !any;
                }
                continue;
            }
            switch (c.kind) {
                case RW_AGG_COUNT_STAR:
                case RW_AGG_COUNT:
                case RW_AGG_SUM0:
                    curr[ci] = acc[slot];
                    curr_null[ci] = 0;
                    break;
                default:
                    curr[ci] = acc[slot];
                    curr_null[ci] = !has[slot];
            }
        }
        uint8_t hp = t.has_prev[slot];
        long long prev_rc = 0;
        if (hp) {
            long long p = t.prev[(size_t)row_count_index * cap + slot];
            prev_rc = p < 0 ? 0 : p;
        }
        // infer_change_type (agg_group.rs:138-163)
        int change; // 0 none, 1 insert, 2 delete, 3 update
        if (prev_rc == 0 && rc == 0) change = 0;
        else if (prev_rc == 0) change = 1;
        else if (rc == 0) change = 2;
        else {
            bool eq = true;
            for (int ci = 0; eq && ci < n_calls; ci++) {
                uint8_t pn = t.prev_null[(size_t)ci * cap + slot];
                if (calls[ci].decimal) {
                    // rust_decimal Eq compares VALUES (1.2 == 1.20)
                    eq = (pn == curr_null[ci]) &&
                         (pn ||
                          dec_value_eq_d(t.prev[(size_t)ci * cap + slot],
                                         t.prev2[(size_t)ci * cap + slot],
                                         curr[ci], curr2[ci]));
                } else {
                    eq = (pn == curr_null[ci]) &&
                         (pn || t.prev[(size_t)ci * cap + slot] == curr[ci]);
                }
            }
            change = eq ? 0 : 3;
        }
        if (change == 0) continue;
        int n_out_rows = (change == 3) ? 2 : 1;
        uint32_t base = atomicAdd(&t.counters[1], (uint32_t)n_out_rows);
        if (base + n_out_rows > t.out_capacity) {
            atomicExch(&t.counters[2], 2u); // output overflow
            continue;
        }
        auto write_row = [&](uint32_t orow, uint8_t op, const long long* vals,
                             const uint8_t* nulls, const long long* vals2) {
            t.out_ops[orow] = op;
            for (int k = 0; k < KW; k++) {
                t.out_vals[(size_t)orow * width + k] = t.keys[(size_t)slot * KW + k];
                t.out_nulls[(size_t)orow * width + k] =
                    (t.key_nulls[slot] >> k) & 1;
            }
            for (int ci = 0; ci < n_calls; ci++) {
                t.out_vals[(size_t)orow * width + KW + ci] = vals[ci];
                t.out_nulls[(size_t)orow * width + KW + ci] = nulls[ci];
                if (t.out_vals2)
                    t.out_vals2[(size_t)orow * width + KW + ci] = vals2[ci];
            }
        };
        long long prevv[MAX_CALLS];
        long long prevv2[MAX_CALLS];
        uint8_t prevn[MAX_CALLS];
        for (int ci = 0; ci < n_calls; ci++) {
            prevv[ci] = t.prev[(size_t)ci * cap + slot];
            prevv2[ci] = t.prev2 ? t.prev2[(size_t)ci * cap + slot] : 0;
            prevn[ci] = t.prev_null[(size_t)ci * cap + slot];
        }
        if (change == 1) {
            write_row(base, RW_OP_INSERT, curr, curr_null, curr2);
        } else if (change == 2) {
            write_row(base, RW_OP_DELETE, prevv, prevn, prevv2);
        } else {
            write_row(base, RW_OP_UPDATE_DELETE, prevv, prevn, prevv2);
            write_row(base + 1, RW_OP_UPDATE_INSERT, curr, curr_null, curr2);
        }
        // prev := curr (or cleared on delete) — agg_group.rs:571-607
        if (change == 2) {
            t.has_prev[slot] = 0;
        } else {
            t.has_prev[slot] = 1;
            for (int ci = 0; ci < n_calls; ci++) {
                t.prev[(size_t)ci * cap + slot] = curr[ci];
                if (t.prev2) t.prev2[(size_t)ci * cap + slot] = curr2[ci];
                t.prev_null[(size_t)ci * cap + slot] = curr_null[ci];
            }
        }
    }
}

// agg_flush_fast: agg_flush_kernel for executors whose calls all keep plain
// value states (no decimal, no materialized-input call) — q7, q7pipe, q3.
// Same semantics, restructured around what the generic kernel pays for at
// a ~1K-slot flush:
//  - <KW, NC> are compile-time and the call kinds arrive packed one per
//    byte, so every per-slot array is fully unrolled into registers (no
//    scratch; the generic kernel indexes its arrays at run time);
//  - all of a slot's state loads are issued together after the dirty_list
//    load and the decision is taken afterwards (dirty_list → state → stores:
//    three dependent round trips);
//  - one cursor atomic per wave: lanes count their 0/1/2 rows, ballots give
//    the prefix, lane 0 reserves the wave's rows, a U−/U+ pair stays
//    adjacent;
//  - a block without work leaves after reading the dirty count;
//  - fused_reset: the stream-ordered flush needs counters[0..1] zeroed
//    after the last slot is handled. Every block that had work draws an
//    arrival ticket (counters[3]) after its loop; the block drawing the last
//    one writes the zeros, the ticket included. A block reads the dirty
//    count before it draws, so the zeros cannot land before a working
//    block has read it; a block that reads 0 afterwards had no work anyway.
//    Nothing waits on another block. counters[2] (overflow) stays sticky.
//  - block 0 records the largest dirty count seen in counters[5].
//
// One pass of the fast flush for thread `i` of `n_dirty`; PRELOADED: the
// caller has read `slot` = dirty_list[i] already. The whole wave calls it
// together (ballots), threads past the dirty count included. Shared by agg_flush_fast_kernel and the fused tail
// of agg_apply_dense4_kernel_span.
template <int KW, int NC, bool PRELOADED>
__device__ __forceinline__ void agg_flush_fast_pass(
        const AggTableDev& t, int row_count_index, uint32_t kinds, size_t cap,
        int lane, uint32_t i, uint32_t n_dirty, uint32_t slot) {
    constexpr int width = KW + NC;
    const uint64_t lanes_below = (1ull << lane) - 1;
    long long curr[NC], prevv[NC];
    uint8_t curr_null[NC], prevn[NC];
    int64_t key[KW];
    uint32_t knull = 0;
    int change = 0; // 0 none, 1 insert, 2 delete, 3 update
    if (i < n_dirty) {
        if (!PRELOADED) slot = t.dirty_list[i];
        long long a[NC];
        uint8_t h[NC];
#pragma unroll
        for (int ci = 0; ci < NC; ci++) {
            a[ci] = t.acc[(size_t)ci * cap + slot];
            h[ci] = t.has[(size_t)ci * cap + slot];
            prevv[ci] = t.prev[(size_t)ci * cap + slot];
            prevn[ci] = t.prev_null[(size_t)ci * cap + slot];
        }
        const uint8_t hp = t.has_prev[slot];
#pragma unroll
        for (int k = 0; k < KW; k++) key[k] = t.keys[(size_t)slot * KW + k];
        knull = t.key_nulls[slot];
        // row_count_of clamp (agg_group.rs:63-75); prev/prev_null hold
        // no meaningful value until has_prev is set
        long long rc = 0, prc = 0;
#pragma unroll
        for (int ci = 0; ci < NC; ci++)
            if (ci == row_count_index) {
                rc = a[ci];
                prc = prevv[ci];
            }
        if (rc < 0) rc = 0;
        const long long prev_rc = (hp && prc > 0) ? prc : 0;
        bool eq = true;
#pragma unroll
        for (int ci = 0; ci < NC; ci++) {
            const uint32_t kind = (kinds >> (8 * ci)) & 0xffu;
            const bool never_null = kind == RW_AGG_COUNT_STAR ||
                                    kind == RW_AGG_COUNT ||
                                    kind == RW_AGG_SUM0;
            curr[ci] = a[ci];
            curr_null[ci] = never_null ? 0 : !h[ci];
            eq = eq && prevn[ci] == curr_null[ci] &&
                 (prevn[ci] || prevv[ci] == curr[ci]);
        }
        // infer_change_type (agg_group.rs:138-163)
        if (prev_rc == 0 && rc == 0) change = 0;
        else if (prev_rc == 0) change = 1;
        else if (rc == 0) change = 2;
        else change = eq ? 0 : 3;
        if (rc == 0) {
            // reset value states (agg_state.rs:149-155)
#pragma unroll
            for (int ci = 0; ci < NC; ci++) {
                const uint32_t kind = (kinds >> (8 * ci)) & 0xffu;
                t.acc[(size_t)ci * cap + slot] =
                    kind == RW_AGG_MIN ? INT64_MAX
                    : kind == RW_AGG_MAX ? INT64_MIN : 0;
                t.has[(size_t)ci * cap + slot] = 0;
            }
        }
        t.dirty_flag[slot] = 0;
    }
    const int n_out = change == 3 ? 2 : (change ? 1 : 0);
    const uint64_t b1 = __ballot(n_out >= 1);
    const uint64_t b2 = __ballot(n_out == 2);
    const uint32_t wave_rows = __popcll(b1) + __popcll(b2);
    if (wave_rows) { // wave-uniform
        uint32_t wbase = 0;
        if (lane == 0) wbase = atomicAdd(&t.counters[1], wave_rows);
        wbase = __shfl(wbase, 0);
        const uint32_t orow = wbase + __popcll(b1 & lanes_below) +
                              __popcll(b2 & lanes_below);
        if (n_out && orow + n_out > t.out_capacity) {
            atomicExch(&t.counters[2], 2u); // output overflow
        } else if (n_out) {
            auto write_row = [&](uint32_t r, uint8_t op,
                                 const long long (&vals)[NC],
                                 const uint8_t (&nulls)[NC]) {
                t.out_ops[r] = op;
                long long* ov = t.out_vals + (size_t)r * width;
                uint8_t* on = t.out_nulls + (size_t)r * width;
#pragma unroll
                for (int k = 0; k < KW; k++) {
                    ov[k] = key[k];
                    on[k] = (knull >> k) & 1;
                }
#pragma unroll
                for (int ci = 0; ci < NC; ci++) {
                    ov[KW + ci] = vals[ci];
                    on[KW + ci] = nulls[ci];
                }
            };
            if (change == 1) {
                write_row(orow, RW_OP_INSERT, curr, curr_null);
            } else if (change == 2) {
                write_row(orow, RW_OP_DELETE, prevv, prevn);
            } else {
                write_row(orow, RW_OP_UPDATE_DELETE, prevv, prevn);
                write_row(orow + 1, RW_OP_UPDATE_INSERT, curr, curr_null);
            }
            // prev := curr (or cleared on delete) — agg_group.rs:571-607
            if (change == 2) {
                t.has_prev[slot] = 0;
            } else {
                t.has_prev[slot] = 1;
#pragma unroll
                for (int ci = 0; ci < NC; ci++) {
                    t.prev[(size_t)ci * cap + slot] = curr[ci];
                    t.prev_null[(size_t)ci * cap + slot] = curr_null[ci];
                }
            }
        }
    }
}

template <int KW, int NC>
__global__ __launch_bounds__(256) void agg_flush_fast_kernel(
        AggTableDev t, int row_count_index, uint32_t kinds, int fused_reset) {
    const uint32_t n_dirty = __atomic_load_n(&t.counters[0], __ATOMIC_RELAXED);
    const uint32_t block0 = blockIdx.x * blockDim.x;
    if (block0 >= n_dirty) return;
    const uint32_t stride = gridDim.x * blockDim.x;
    const size_t cap = (size_t)t.cap_mask + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&t.counters[5], n_dirty);
    for (uint32_t i0 = block0; i0 < n_dirty; i0 += stride) {
        agg_flush_fast_pass<KW, NC>(t, row_count_index, kinds, cap,
                                    threadIdx.x & 63, i0 + threadIdx.x,
                                    n_dirty);
    }
    if (fused_reset) {
        __syncthreads(); // block-uniform: every thread ran the same trip count
        if (threadIdx.x == 0) {
            uint32_t working = (n_dirty + blockDim.x - 1) / blockDim.x;
            if (working > gridDim.x) working = gridDim.x;
            if (atomicAdd(&t.counters[3], 1u) == working - 1) {
                atomicExch(&t.counters[0], 0u); // dirty count
                atomicExch(&t.counters[1], 0u); // out cursor
                atomicExch(&t.counters[3], 0u); // ticket
            }
        }
    }
}

// init kernel: min/max identities
__global__ void agg_init_kernel(AggTableDev t, int n_calls, AggCallDev c0,
                                AggCallDev c1, AggCallDev c2, AggCallDev c3) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    size_t cap = (size_t)t.cap_mask + 1;
    size_t total = cap * n_calls;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int ci = (int)(i / cap);
        long long init = 0;
        if (calls[ci].kind == RW_AGG_MIN) init = INT64_MAX;
        if (calls[ci].kind == RW_AGG_MAX) init = INT64_MIN;
        t.acc[i] = init;
    }
}

__global__ void agg_eowc_close_kernel(AggTableDev t, int KW, int n_calls,
                                      int row_count_index, long long wm,
                                      AggCallDev c0, AggCallDev c1,
                                      AggCallDev c2, AggCallDev c3);

__global__ void agg_eowc_dump_kernel(AggTableDev t, int KW, int n_calls,
                                     int row_count_index, AggCallDev c0,
                                     AggCallDev c1, AggCallDev c2,
                                     AggCallDev c3);

extern "C" __global__ void agg_counters_reset_kernel(uint32_t* counters);

// state restore (rw_stream.h contract): seed value states + prev outputs
// from decoded state rows. err code 1 = table full.
__global__ void agg_restore_kernel(AggTableDev t, int KW, int n_calls,
                                   const int64_t* keys,
                                   const uint32_t* knulls,
                                   const long long* vals,
                                   const uint8_t* vnulls,
                                   const long long* vals2, uint32_t n,
                                   int set_prev, AggCallDev c0, AggCallDev c1,
                                   AggCallDev c2, AggCallDev c3) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    size_t cap = (size_t)t.cap_mask + 1;
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t kw[MAX_KW];
        for (int k = 0; k < KW; k++) kw[k] = keys[(size_t)i * KW + k];
        uint32_t slot = table_find_or_insert(t.state, t.keys, t.key_nulls,
                                             t.cap_mask, kw, knulls[i], KW);
        if (slot == UINT32_MAX) {
            atomicExch(&t.counters[2], 1u);
            continue;
        }
        for (int ci = 0; ci < n_calls; ci++) {
            if (calls[ci].decimal) {
                // seed the exact-sum state from the stored decimal output
                // (sum == output in the exact domain; oracle restore does
                // the same)
                long long w0 = vals[(size_t)ci * n + i];
                long long w1 = vals2 ? vals2[(size_t)ci * n + i] : 0;
                uint8_t nu = vnulls[(size_t)ci * n + i];
                int dord = calls[ci].dord;
                t.has[(size_t)ci * cap + slot] = !nu;
                if (!nu) {
                    DecValD dv = dec_parse_d(w0, w1);
                    if (dv.special) {
                        t.dspec[((size_t)dord * 3 + (dv.special - 1)) * cap +
                                slot] = 1;
                    } else {
                        uint64_t w[4];
                        dec_addend_d(dv, w);
                        for (int k = 0; k < 4; k++)
                            t.dsum[((size_t)dord * 4 + k) * cap + slot] =
                                w[k];
                        t.dscl[(size_t)dord * cap + slot] = dv.scale;
                    }
                }
                if (set_prev) {
                    t.prev[(size_t)ci * cap + slot] = w0;
                    if (t.prev2) t.prev2[(size_t)ci * cap + slot] = w1;
                    t.prev_null[(size_t)ci * cap + slot] = nu;
                }
                continue;
            }
            if (calls[ci].minput) {
                // prev output = first entry of the (already restored)
                // minput chain (output_first, minput.rs:236-241; see
                // agg_flush_kernel's identical walk)
                const AggCallDev& c = calls[ci];
                uint32_t row = t.mheads[(size_t)c.mord * cap + slot];
                bool any = false, any_null = false;
                long long best = 0;
                while (row != UINT32_MAX) {
                    if (t.malive[row]) {
                        if (t.mval_null[row]) {
                            any_null = true;
                        } else {
                            long long v2 = t.mval[row];
                            if (!any) best = v2;
                            else if (c.kind == RW_AGG_MIN)
                                best = v2 < best ? v2 : best;
                            else
                                best = v2 > best ? v2 : best;
                            any = true;
                        }
                    }
                    row = t.mnext[row];
                }
                long long pv;
                uint8_t pn;
                if (c.kind == RW_AGG_MAX && any_null) {
                    pv = 0;
                    pn = 1;
                } else {
                    pv = best;
                    pn = !any;
                }
                if (set_prev) {
                    t.prev[(size_t)ci * cap + slot] = pv;
                    t.prev_null[(size_t)ci * cap + slot] = pn;
                }
                continue;
            }
            long long v = vals[(size_t)ci * n + i];
            uint8_t nu = vnulls[(size_t)ci * n + i];
            long long init = 0;
            if (calls[ci].kind == RW_AGG_MIN) init = INT64_MAX;
            if (calls[ci].kind == RW_AGG_MAX) init = INT64_MIN;
            t.acc[(size_t)ci * cap + slot] = nu ? init : v;
            t.has[(size_t)ci * cap + slot] = !nu;
            if (set_prev) {
                t.prev[(size_t)ci * cap + slot] = v;
                t.prev_null[(size_t)ci * cap + slot] = nu;
            }
        }
        if (set_prev) t.has_prev[slot] = 1;
    }
}

// minput-table restore: rebuild the materialized-input chains from decoded
// rows (rw_stream.h restore contract)
__global__ void agg_minput_restore_kernel(AggTableDev t, int KW, int mord,
                                          const int64_t* gkeys,
                                          const uint32_t* gnulls,
                                          const long long* vals,
                                          const uint8_t* vnulls,
                                          const long long* sks,
                                          const uint8_t* sknulls, uint32_t n) {
    size_t cap = (size_t)t.cap_mask + 1;
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t kw[MAX_KW];
        for (int k = 0; k < KW; k++) kw[k] = gkeys[(size_t)i * KW + k];
        uint32_t slot = table_find_or_insert(t.state, t.keys, t.key_nulls,
                                             t.cap_mask, kw, gnulls[i], KW);
        if (slot == UINT32_MAX) {
            atomicExch(&t.counters[2], 1u);
            continue;
        }
        uint32_t row = atomicAdd(t.mcursor, 1u);
        if (row >= t.mrow_cap) {
            atomicExch(&t.counters[2], 3u);
            continue;
        }
        st_u32(&t.mslot[row], slot);
        t.mcall[row] = (uint8_t)mord;
        st_i64((int64_t*)&t.mval[row], vals[i]);
        t.mval_null[row] = vnulls[i];
        for (int k = 0; k < t.n_sk; k++) {
            st_i64((int64_t*)&t.msk[(size_t)k * t.mrow_cap + row],
                   sks[(size_t)k * n + i]);
            t.msk_null[(size_t)k * t.mrow_cap + row] =
                sknulls[(size_t)k * n + i];
        }
        st_u32(&t.malive[row], 1);
        uint32_t* headp = t.mheads + (size_t)mord * cap + slot;
        uint32_t old_head = ld_u32(headp);
        for (;;) {
            st_u32(&t.mnext[row], old_head);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            uint32_t prev = atomicCAS(headp, old_head, row);
            if (prev == old_head) break;
            old_head = prev;
        }
    }
}

// ============ varchar: the string materialiser both executors share ======

// n reference words, word i at words[i * stride] (stride in 8-byte units:
// 1 for a columnar block, row_stride / 8 for a column of packed records).
// Optional masks yield the zero word (length 0): nulls[i] != 0 (the join
// output block's NULL flags) and ops[i] == 0xFF for i < sparse_n (the inner
// probe's pre-assigned sparse region — those slots hold unwritten words).
struct VarlenView {
    const uint64_t* words;
    uint32_t stride;
    const uint8_t* nulls;
    const uint8_t* ops;
    uint32_t sparse_n;
};

// Materialises the strings a view's words reference into one packed host
// byte buffer (length kernel -> rocPRIM exclusive scan -> copy kernel ->
// D2H), with the device scratch that sequence needs. One per executor
// (HashJoin's emit/drain/compaction, HashAgg's flush/spill/watermark); the
// methods are defined beside the kernels.
struct VarlenFetch {
    uint64_t* d_vlens = nullptr;
    uint64_t* d_voffs = nullptr;
    uint32_t d_vcap = 0;
    uint8_t* d_vbytes = nullptr;
    uint64_t d_vbytes_cap = 0;
    void* d_scan_tmp = nullptr;
    size_t d_scan_tmp_cap = 0;
    hipEvent_t vev0 = nullptr, vev1 = nullptr, vev2 = nullptr;
    double vemit_ms = 0, vcopy_ms = 0; // whole materialise / copy kernel
    uint64_t vemit_bytes = 0, vemit_launches = 0;

    DevOwner mem;

    int ensure_vscratch(uint32_t n);
    int ensure_scan_tmp(size_t tmp); // rocPRIM scan temporary storage
    int fetch(const VarlenView& v, const uint8_t* arena, uint32_t n,
              std::vector<uint64_t>& offs, std::vector<uint8_t>& bytes,
              bool timed, hipStream_t stream);
    ~VarlenFetch();
};

// ============ HashAgg varchar group keys: string interning ===
//
// A varchar group-key cell is a reference word (rw_varlen.hpp). The agg
// kernels key on words, so before the apply launch every word of the batch
// is made CANONICAL: equal strings carry equal words, and the tuned
// apply / flush / clean / restore kernels run as they do for i64 keys.
//
// The table is open-addressed, one 8-byte canonical word per slot, 0 =
// empty. Visibility rule (guide G16, and the comment above
// table_find_or_insert): a lane may not read BYTES another lane wrote in
// the same launch without a release/acquire pair. So every byte a lane
// hashes or compares was written before its launch began — arena bytes by
// an earlier launch, staging bytes by the push's host-to-device copy — and
// only slot WORDS are exchanged in-launch, through relaxed agent-scope
// atomics. That takes three launch-separated kernels per push:
//   lookup : CAS the row's provisional (staging) word into an empty slot,
//            or compare bytes with the word found there; record the slot
//   commit : one lane per CAS winner appends its string to the arena and
//            stores the final word into the slot
//   resolve: every row reloads slot[its recorded index] into the batch
// No CLAIMED state, no fences.
struct InternDev {
    uint64_t* slots;
    uint32_t cap_mask;
    uint8_t* arena;
    uint64_t arena_cap;
    const uint8_t* stg;       // this push's staged bytes
    unsigned long long* tail; // arena append cursor (bytes)
    uint32_t* ctr;            // [0] winners of this push, [1] table entries
    uint32_t* winners;        // slot indices claimed by this push
    uint32_t* rowslot;        // per (vcol, row): slot, UINT32_MAX = none
    uint32_t* err;            // &AggTableDev::counters[2]
};

// the words to intern: varchar column j of row r at words[j][r * stride];
// word 0 (NULL) and invisible rows are skipped
struct InternCols {
    int64_t* words[MAX_KW];
    const uint8_t* vis; // may be null
    uint32_t n_rows, nv, stride;
};

#define AGG_ERR_INTERN 6u // counters[2] code: intern table / arena full

__device__ __forceinline__ uint64_t intern_hash(const uint8_t* p,
                                                uint32_t len) {
    uint64_t h = 0xcbf29ce484222325ULL ^ len; // FNV-1a, then the finalizer
    for (uint32_t k = 0; k < len; k++) h = (h ^ p[k]) * 0x100000001b3ULL;
    return mix64(h);
}

__global__ __launch_bounds__(256) void agg_intern_lookup_kernel(InternDev d,
                                                                InternCols c) {
    uint32_t total = c.n_rows * c.nv;
    uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gstride) {
        uint32_t j = i / c.n_rows, r = i - j * c.n_rows;
        uint64_t w = (uint64_t)c.words[j][(size_t)r * c.stride];
        uint32_t found = UINT32_MAX;
        if (w != 0 && !(c.vis && !c.vis[r])) {
            uint32_t len = rwvarlen::word_len(w);
            const uint8_t* p =
                d.stg + (rwvarlen::word_off(w) & ~rwvarlen::PROV_BIT);
            uint32_t slot = (uint32_t)intern_hash(p, len) & d.cap_mask;
            for (uint32_t probes = 0; probes <= d.cap_mask; probes++) {
                uint64_t cur = __hip_atomic_load(&d.slots[slot], RLX);
                if (cur == 0) {
                    cur = atomicCAS((unsigned long long*)&d.slots[slot], 0ULL,
                                    (unsigned long long)w);
                    if (cur == 0) { // this row's staged copy is the candidate
                        d.winners[atomicAdd(&d.ctr[0], 1u)] = slot;
                        found = slot;
                        break;
                    }
                }
                // a final word references the arena, a provisional one this
                // push's staging: both written before this launch
                if (rwvarlen::word_len(cur) == len) {
                    uint64_t off = rwvarlen::word_off(cur);
                    const uint8_t* q = (off & rwvarlen::PROV_BIT)
                                           ? d.stg + (off & ~rwvarlen::PROV_BIT)
                                           : d.arena + off;
                    bool eq = true;
                    for (uint32_t k = 0; eq && k < len; k++) eq = p[k] == q[k];
                    if (eq) {
                        found = slot;
                        break;
                    }
                }
                slot = (slot + 1) & d.cap_mask;
            }
            if (found == UINT32_MAX) st_u32(d.err, AGG_ERR_INTERN); // wrapped
        }
        d.rowslot[i] = found;
    }
}

__global__ __launch_bounds__(256) void agg_intern_commit_kernel(InternDev d) {
    uint32_t nw = d.ctr[0]; // final since the lookup launch ended
    uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nw;
         k += gstride) {
        uint32_t slot = d.winners[k];
        uint64_t w = d.slots[slot];
        uint32_t len = rwvarlen::word_len(w);
        uint64_t off = atomicAdd(d.tail, (unsigned long long)len);
        if (off + len > d.arena_cap) { // host bound violated: never write
            st_u32(d.err, AGG_ERR_INTERN);
            continue;
        }
        const uint8_t* src =
            d.stg + (rwvarlen::word_off(w) & ~rwvarlen::PROV_BIT);
        uint8_t* dst = d.arena + off;
        for (uint32_t b = 0; b < len; b++) dst[b] = src[b];
        __hip_atomic_store(&d.slots[slot], rwvarlen::pack(off, len), RLX);
        atomicAdd(&d.ctr[1], 1u);
    }
}

__global__ __launch_bounds__(256) void agg_intern_resolve_kernel(
    InternDev d, InternCols c) {
    uint32_t total = c.n_rows * c.nv;
    uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gstride) {
        uint32_t j = i / c.n_rows, r = i - j * c.n_rows;
        uint32_t s = d.rowslot[i];
        c.words[j][(size_t)r * c.stride] =
            s == UINT32_MAX ? 0 : (int64_t)d.slots[s];
    }
}

// table growth: every entry is distinct, so CAS-on-empty with no compares;
// the bytes hashed were written by earlier launches
__global__ __launch_bounds__(256) void agg_intern_rehash_kernel(
    const uint64_t* old_slots, uint32_t old_cap, uint64_t* slots,
    uint32_t cap_mask, const uint8_t* arena) {
    uint32_t gstride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < old_cap;
         s += gstride) {
        uint64_t w = old_slots[s];
        if (w == 0) continue;
        uint32_t slot = (uint32_t)intern_hash(arena + rwvarlen::word_off(w),
                                              rwvarlen::word_len(w)) &
                        cap_mask;
        for (uint32_t probes = 0; probes <= cap_mask; probes++) {
            if (__hip_atomic_load(&slots[slot], RLX) == 0 &&
                atomicCAS((unsigned long long*)&slots[slot], 0ULL,
                          (unsigned long long)w) == 0)
                break;
            slot = (slot + 1) & cap_mask;
        }
    }
}

// ============ HashAgg key-table compaction ====================
//
// The clean / EOWC-close / vnode-rescope kernels and the flush's delete
// branch reset a group in place and leave its slot READY, which keeps probe
// clusters intact inside an epoch. Between epochs rw_hash_agg_compact gives
// those slots back: live groups are packed into a temporary sized by their
// number, the table is cleared to its as-created state, and the packed
// groups are inserted again.
//
// A slot is LIVE when it is READY and has a persisted row (has_prev), a
// pending change (dirty_flag) or a positive row count. The last term keeps
// what an EOWC restore leaves: state with neither flag set.
__device__ __forceinline__ bool agg_slot_live(const AggTableDev& t, size_t cap,
                                              int row_count_index,
                                              uint32_t slot) {
    return t.has_prev[slot] || t.dirty_flag[slot] ||
           t.acc[(size_t)row_count_index * cap + slot] > 0;
}

// out[0] = READY slots, out[1] = live ones; one atomic pair per wave
__global__ __launch_bounds__(256) void agg_compact_count_kernel(
    AggTableDev t, int row_count_index, unsigned long long* out) {
    const size_t cap = (size_t)t.cap_mask + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    uint32_t ready = 0, live = 0;
    // wave-uniform trip count: the ballots below need every lane
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < cap;
         base += stride) {
        size_t slot = base + threadIdx.x;
        bool r = slot < cap && t.state[slot] == SLOT_READY;
        bool l = r && agg_slot_live(t, cap, row_count_index, (uint32_t)slot);
        ready += __popcll(__ballot(r));
        live += __popcll(__ballot(l));
    }
    if (lane == 0 && ready) {
        atomicAdd(&out[0], (unsigned long long)ready);
        atomicAdd(&out[1], (unsigned long long)live);
    }
}

// the packed temporary: n records, columns laid out as the table's are with
// n in place of the capacity
struct AggPackDev {
    int64_t* keys;       // [n * KW]
    uint32_t* key_nulls; // [n]
    long long* acc;      // [n_calls][n]
    uint8_t* has;        // [n_calls][n]
    long long* prev;     // [n_calls][n]
    uint8_t* prev_null;  // [n_calls][n]
    long long* prev2;    // [n_calls][n], decimal executors
    uint8_t* has_prev;   // [n]
    unsigned long long* dsum; // [n_dec][4][n]
    uint32_t* dscl;           // [n_dec][n]
    long long* dspec;         // [n_dec][3][n]
    uint32_t* mheads;    // [n_minput][n]
    uint32_t* old_slot;  // [n]
    uint32_t* new_slot;  // [n], minput executors
    uint32_t* cursor;    // records packed so far
    uint32_t* err;       // 1 = more live slots than counted, 2 = table full
    uint32_t n;
    int n_minput;
};

__global__ __launch_bounds__(256) void agg_compact_pack_kernel(
    AggTableDev t, AggPackDev p, int KW, int n_calls, int row_count_index) {
    const size_t cap = (size_t)t.cap_mask + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    const uint64_t lanes_below = (1ull << lane) - 1;
    const size_t n = p.n;
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < cap;
         base += stride) {
        size_t slot = base + threadIdx.x;
        bool live = slot < cap && t.state[slot] == SLOT_READY &&
                    agg_slot_live(t, cap, row_count_index, (uint32_t)slot);
        const uint64_t b = __ballot(live);
        if (!b) continue; // wave-uniform
        uint32_t wbase = 0;
        if (lane == 0) wbase = atomicAdd(p.cursor, (uint32_t)__popcll(b));
        wbase = __shfl(wbase, 0);
        if (!live) continue;
        size_t r = (size_t)wbase + __popcll(b & lanes_below);
        if (r >= n) { // the count said otherwise: never write
            atomicExch(p.err, 1u);
            continue;
        }
        for (int k = 0; k < KW; k++) p.keys[r * KW + k] = t.keys[slot * KW + k];
        p.key_nulls[r] = t.key_nulls[slot];
        p.has_prev[r] = t.has_prev[slot];
        p.old_slot[r] = (uint32_t)slot;
        for (int ci = 0; ci < n_calls; ci++) {
            p.acc[ci * n + r] = t.acc[ci * cap + slot];
            p.has[ci * n + r] = t.has[ci * cap + slot];
            p.prev[ci * n + r] = t.prev[ci * cap + slot];
            p.prev_null[ci * n + r] = t.prev_null[ci * cap + slot];
            if (t.prev2) p.prev2[ci * n + r] = t.prev2[ci * cap + slot];
        }
        for (int d = 0; d < t.n_dec; d++) {
            for (int k = 0; k < 4; k++)
                p.dsum[((size_t)d * 4 + k) * n + r] =
                    t.dsum[((size_t)d * 4 + k) * cap + slot];
            p.dscl[d * n + r] = t.dscl[d * cap + slot];
            for (int k = 0; k < 3; k++)
                p.dspec[((size_t)d * 3 + k) * n + r] =
                    t.dspec[((size_t)d * 3 + k) * cap + slot];
        }
        for (int m = 0; m < p.n_minput; m++)
            p.mheads[m * n + r] = t.mheads[m * cap + slot];
    }
}

// varchar key words of the packed block -> provisional words over the OLD
// arena (same offset, same length); word 0 (NULL) stays
__global__ __launch_bounds__(256) void agg_compact_prov_kernel(
    AggPackDev p, int KW, uint32_t vc_mask) {
    const size_t total = (size_t)p.n * KW;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        if (!((vc_mask >> (i % KW)) & 1)) continue;
        uint64_t w = (uint64_t)p.keys[i];
        if (w)
            p.keys[i] = (int64_t)rwvarlen::pack(
                rwvarlen::PROV_BIT | rwvarlen::word_off(w),
                rwvarlen::word_len(w));
    }
}

// one lane per packed record, into the cleared table; the keys are distinct
// and no more than the capacity, so a full table is an internal error
__global__ __launch_bounds__(256) void agg_compact_reinsert_kernel(
    AggTableDev t, AggPackDev p, int KW, int n_calls) {
    const size_t cap = (size_t)t.cap_mask + 1;
    const size_t n = p.n;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        int64_t kw[MAX_KW];
        for (int k = 0; k < KW; k++) kw[k] = p.keys[r * KW + k];
        uint32_t slot = table_find_or_insert(t.state, t.keys, t.key_nulls,
                                             t.cap_mask, kw, p.key_nulls[r],
                                             KW);
        if (p.new_slot) p.new_slot[r] = slot;
        if (slot == UINT32_MAX) {
            atomicExch(p.err, 2u);
            continue;
        }
        t.has_prev[slot] = p.has_prev[r];
        t.dirty_flag[slot] = 0;
        for (int ci = 0; ci < n_calls; ci++) {
            t.acc[ci * cap + slot] = p.acc[ci * n + r];
            t.has[ci * cap + slot] = p.has[ci * n + r];
            t.prev[ci * cap + slot] = p.prev[ci * n + r];
            t.prev_null[ci * cap + slot] = p.prev_null[ci * n + r];
            if (t.prev2) t.prev2[ci * cap + slot] = p.prev2[ci * n + r];
        }
        for (int d = 0; d < t.n_dec; d++) {
            for (int k = 0; k < 4; k++)
                t.dsum[((size_t)d * 4 + k) * cap + slot] =
                    p.dsum[((size_t)d * 4 + k) * n + r];
            t.dscl[d * cap + slot] = p.dscl[d * n + r];
            for (int k = 0; k < 3; k++)
                t.dspec[((size_t)d * 3 + k) * cap + slot] =
                    p.dspec[((size_t)d * 3 + k) * n + r];
        }
        for (int m = 0; m < p.n_minput; m++)
            t.mheads[m * cap + slot] = p.mheads[m * n + r];
    }
}

// materialized-input rows follow their group: one lane per (minput call,
// packed record) walks the chain it moved and writes the new owner. The
// store holds live rows only here (minput_compact ran first), and a chain
// belongs to exactly one record, so no row is written twice.
__global__ __launch_bounds__(256) void agg_compact_mslot_kernel(AggTableDev t,
                                                                AggPackDev p) {
    const size_t total = (size_t)p.n * p.n_minput;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        uint32_t slot = p.new_slot[i % p.n];
        if (slot == UINT32_MAX) continue;
        uint32_t row = p.mheads[i];
        // a chain cannot be longer than the store: the bound ends a walk
        // over a malformed chain
        for (uint32_t steps = 0; row < t.mrow_cap && steps < t.mrow_cap;
             steps++) {
            t.mslot[row] = slot;
            row = t.mnext[row];
        }
    }
}

struct HashAgg {
    RwHashAggDesc desc;
    std::vector<uint8_t> input_types;
    std::vector<uint32_t> group_key;
    std::vector<RwAggCall> calls;
    int KW, n_calls, out_width;
    std::vector<uint8_t> out_types;
    hipStream_t stream = nullptr;
    // every device buffer of this executor (rw_devmem.hpp); the destructor
    // frees them after the stream has drained and before it is destroyed
    DevOwner mem;
    AggTableDev t{};
    uint32_t capacity;
    // staging (host-pinned mirrors reused per push)
    AggBatch stage{};
    uint32_t stage_cap = 0;
    // kernel timing (HIP events on this executor's own stream)
    EventRing ring; // ring.ms_total: apply kernel time
    uint64_t apply_launches = 0, apply_rows = 0;
    // pending outputs
    rwchunk::ChunkQueue outq;
    // checkpoint spill buffer (§8f-2): state-table KV deltas, accumulated at
    // flush, drained by rw_agg_checkpoint_drain
    std::vector<uint8_t> spill;
    uint8_t* d_vnode_bitmap = nullptr; // rescale scope (update_vnode_bitmap)
    uint16_t* d_vnode_hop = nullptr;   // q7-pipeline exchange-hop vnodes
    uint32_t d_vnode_hop_cap = 0;
    bool eowc = false; // emit-on-window-close (hash_agg.rs:421-474)
    bool has_pending_wm = false;
    int64_t pending_wm = 0;
    int n_minput = 0;   // materialized-input (retractable min/max) calls
    std::vector<uint8_t> call_decimal;
    int n_dec = 0;      // decimal-sum calls (exact i256 state)
    std::vector<uint8_t> call_minput;
    std::vector<uint32_t> stream_key;
    // DISTINCT dedup state (aggregate/distinct.rs)
    std::vector<int> distinct_slots;  // batch slot per dedup table
    std::vector<int> call_dedup_idx;  // per call: dedup table index or -1
    std::vector<JoinSlot*> dedup_slots;
    uint32_t dedup_cap_mask = 0;
    std::vector<uint8_t*> hidden_bufs; // device, per dedup table
    uint32_t hidden_cap = 0;
    // §8f-2 dedup-table spill: per table, device dirty tracking + a host
    // persisted bitmap (was the row in the table at the last checkpoint?)
    std::vector<uint8_t> distinct_col_types; // datum col type per table
    std::vector<uint32_t*> ddirty_flag, ddirty_list, ddirty_n;
    std::vector<std::vector<uint8_t>> dedup_persisted;

    // ----- varchar group keys: interning state -----
    uint32_t vc_mask = 0; // bit i: group-key position i is varchar
    int nv = 0;           // number of varchar key positions
    int vpos[MAX_KW] = {};
    bool has_vc() const { return vc_mask != 0; }
    static constexpr uint64_t IN_ARENA_DEFAULT = 1ull << 20;
    static constexpr uint32_t IN_STRINGS_DEFAULT = 1u << 15;
    InternDev in{};
    bool in_ready = false;
    uint8_t* in_stg = nullptr;
    uint64_t in_stg_cap = 0;
    uint32_t in_row_cap = 0;
    uint64_t in_reserve_arena = 0, in_reserve_strings = 0;
    // The host learns the arena tail and the entry count exactly wherever
    // it synchronises anyway (flush); between those points it bounds them
    // by the bytes / rows pushed since.
    uint64_t in_tail_known = rwvarlen::AGG_ARENA_HEADER, in_tail_pending = 0;
    uint64_t in_n_known = 0, in_n_pending = 0;
    // host staging of a batch's provisional words; lives until the next
    // upload so the async H2D copy never outlives its source
    std::vector<int64_t> vwords[MAX_KW];
    // flush / clean materialisation: per key position, n + 1 offsets and
    // the packed bytes of the rows being emitted or spilled
    VarlenFetch vf;
    std::vector<uint64_t> vk_offs[MAX_KW];
    std::vector<uint8_t> vk_bytes[MAX_KW];

    int intern_init() {
        if (in_ready) return RW_OK;
        uint64_t acap = in_reserve_arena ? in_reserve_arena : IN_ARENA_DEFAULT;
        if (acap < rwvarlen::AGG_ARENA_HEADER) acap = rwvarlen::AGG_ARENA_HEADER;
        uint64_t want = 2 * (in_reserve_strings ? in_reserve_strings
                                                : IN_STRINGS_DEFAULT);
        uint32_t tcap = 2;
        while (tcap < want && tcap < (1u << 31)) tcap <<= 1;
        HIP_TRY(mem.alloc(&in.arena, acap));
        HIP_TRY(hipMemset(in.arena, 0, rwvarlen::AGG_ARENA_HEADER));
        in.arena_cap = acap;
        HIP_TRY(mem.alloc(&in.slots, (size_t)tcap * 8));
        HIP_TRY(hipMemset(in.slots, 0, (size_t)tcap * 8));
        in.cap_mask = tcap - 1;
        HIP_TRY(mem.alloc(&in.tail, 8));
        unsigned long long t0 = rwvarlen::AGG_ARENA_HEADER;
        HIP_TRY(hipMemcpy(in.tail, &t0, 8, hipMemcpyHostToDevice));
        HIP_TRY(mem.alloc(&in.ctr, 8));
        HIP_TRY(hipMemset(in.ctr, 0, 8));
        in.err = &t.counters[2];
        in_ready = true;
        return RW_OK;
    }

    // exact tail and entry count; the caller has work pending on the stream
    // or not — either way this drains it
    int intern_sync_counts() {
        if (!in_ready) return RW_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        unsigned long long tl = 0;
        uint32_t c[2] = {0, 0};
        HIP_TRY(hipMemcpy(&tl, in.tail, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c, in.ctr, 8, hipMemcpyDeviceToHost));
        in_tail_known = tl;
        in_tail_pending = 0;
        in_n_known = c[1];
        in_n_pending = 0;
        return RW_OK;
    }

    // room for `extra` more arena bytes: reallocate + one D2D copy between
    // launches (words are offsets, so none is rewritten)
    int intern_arena_ensure(uint64_t extra) {
        if (in_tail_known + in_tail_pending + extra <= in.arena_cap)
            return RW_OK;
        int rc = intern_sync_counts(); // also: launches may read the old one
        if (rc != RW_OK) return rc;
        uint64_t need = in_tail_known + extra;
        if (need > rwvarlen::AGG_ARENA_MAX)
            FAIL(RW_E_INVAL, "varchar group-key arena would exceed 2^39 bytes");
        if (need > in.arena_cap) {
            uint64_t cap = in.arena_cap;
            while (cap < need) cap *= 2;
            HIP_TRY(mem.regrow(&in.arena, cap, in_tail_known));
            in.arena_cap = cap;
        }
        return RW_OK;
    }

    // room for `add` more entries: the bound may pass 0.7 of the capacity
    // only after an exact count, and past half the table doubles (rehash)
    int intern_table_ensure(uint64_t add) {
        uint64_t tcap = (uint64_t)in.cap_mask + 1;
        if ((in_n_known + in_n_pending + add) * 10 <= tcap * 7) return RW_OK;
        int rc = intern_sync_counts();
        if (rc != RW_OK) return rc;
        uint64_t ncap = tcap;
        while ((in_n_known + add) * 2 > ncap) ncap <<= 1;
        if (ncap > (1ull << 31))
            FAIL(RW_E_INVAL, "varchar group-key intern table > 2^31 slots");
        if (ncap != tcap) {
            uint64_t* ns = nullptr;
            HIP_TRY(mem.alloc(&ns, ncap * 8));
            HIP_TRY(hipMemsetAsync(ns, 0, ncap * 8, stream));
            agg_intern_rehash_kernel<<<grid_for((uint32_t)tcap), 256, 0,
                                       stream>>>(in.slots, (uint32_t)tcap, ns,
                                                 (uint32_t)(ncap - 1),
                                                 in.arena);
            HIP_TRY(hipStreamSynchronize(stream));
            mem.release(&in.slots);
            in.slots = ns;
            in.cap_mask = (uint32_t)(ncap - 1);
        }
        return RW_OK;
    }

    // size everything one pre-pass over `cells` (row, varchar column) cells
    // holding `bytes` string bytes needs; the stream is idle between pushes
    // (push_chunk ends synchronised), so scratch is reallocated freely
    int intern_prepare(uint64_t cells, uint64_t bytes) {
        int rc = intern_init();
        if (rc != RW_OK) return rc;
        if (bytes >= rwvarlen::PROV_BIT || cells > UINT32_MAX)
            FAIL(RW_E_INVAL, "varchar group-key batch too large");
        if (in_stg_cap < bytes + 1) {
            HIP_TRY(hipStreamSynchronize(stream));
            in_stg_cap = 0;
            uint64_t cap = 1ull << 16;
            while (cap < bytes + 1) cap <<= 1;
            HIP_TRY(mem.regrow(&in_stg, cap));
            in_stg_cap = cap;
        }
        in.stg = in_stg;
        if (in_row_cap < cells) {
            HIP_TRY(hipStreamSynchronize(stream));
            mem.release(&in.rowslot);
            mem.release(&in.winners);
            in_row_cap = 0;
            uint64_t cap = 4096;
            while (cap < cells) cap <<= 1;
            HIP_TRY(mem.alloc(&in.rowslot, cap * 4));
            HIP_TRY(mem.alloc(&in.winners, cap * 4));
            in_row_cap = (uint32_t)(cap > UINT32_MAX ? UINT32_MAX : cap);
        }
        rc = intern_arena_ensure(bytes);
        if (rc != RW_OK) return rc;
        rc = intern_table_ensure(cells);
        if (rc != RW_OK) return rc;
        // only now: either ensure may have taken exact counts, which zeroes
        // the pending bounds, and this batch's launches come after both
        in_tail_pending += bytes;
        in_n_pending += cells;
        return RW_OK;
    }

    // the pre-pass: lookup -> commit -> resolve, launch-separated
    int intern_run(const InternCols& c) {
        uint32_t cells = c.n_rows * c.nv;
        if (!cells) return RW_OK;
        HIP_TRY(hipMemsetAsync(in.ctr, 0, 4, stream)); // winners of this push
        int grid = grid_for(cells);
        if (in_timing && !in_ev[0])
            for (auto& ev : in_ev) HIP_TRY(hipEventCreate(&ev));
        if (in_timing) HIP_TRY(hipEventRecord(in_ev[0], stream));
        agg_intern_lookup_kernel<<<grid, 256, 0, stream>>>(in, c);
        if (in_timing) HIP_TRY(hipEventRecord(in_ev[1], stream));
        agg_intern_commit_kernel<<<grid < 256 ? grid : 256, 256, 0, stream>>>(in);
        if (in_timing) HIP_TRY(hipEventRecord(in_ev[2], stream));
        agg_intern_resolve_kernel<<<grid, 256, 0, stream>>>(in, c);
        if (in_timing) {
            HIP_TRY(hipEventRecord(in_ev[3], stream));
            in_ev_pending = true;
        }
        return RW_OK;
    }

    // RW_AGG_INTERN_TIMING=1 (read at create; tests/bench_varchar_agg.py):
    // an event around each pre-pass kernel, read back where the push has
    // synchronised anyway
    bool in_timing = false, in_ev_pending = false;
    hipEvent_t in_ev[4] = {};
    double in_ms[3] = {0, 0, 0};
    uint64_t in_timed_launches = 0;
    int intern_harvest() {
        if (!in_ev_pending) return RW_OK;
        in_ev_pending = false;
        HIP_TRY(hipEventSynchronize(in_ev[3]));
        for (int k = 0; k < 3; k++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, in_ev[k], in_ev[k + 1]));
            in_ms[k] += ms;
        }
        in_timed_launches++;
        return RW_OK;
    }

    // validate a chunk's varchar key columns; reads offsets only
    int intern_validate(const RwChunk* c, uint64_t* total_bytes) {
        uint64_t total = 0;
        for (int j = 0; j < nv; j++) {
            uint32_t ci = group_key[vpos[j]];
            if (c->cols[ci].type != RW_T_VARCHAR)
                FAIL(RW_E_INVAL, "column %u: expected a varchar column", ci);
            if (const char* why = rwvarlen::check_column(c->cols[ci], c->n_rows))
                FAIL(RW_E_INVAL, "varchar column %u: %s", ci, why);
            total += ((const RwVarlenData*)c->cols[ci].data)->offsets[c->n_rows];
        }
        *total_bytes = total;
        return RW_OK;
    }

    // flush / clean: fetch the strings of n rows of key words, key position
    // k of row i at base[i * stride + k], into vk_offs / vk_bytes. A NULL
    // key's word is 0, so it yields length 0 without a null mask.
    int fetch_key_strings(const uint64_t* base, uint32_t stride, uint32_t n) {
        for (int j = 0; j < nv; j++) {
            int k = vpos[j];
            VarlenView v{base + k, stride, nullptr, nullptr, 0};
            int rc = vf.fetch(v, in.arena, n, vk_offs[k], vk_bytes[k],
                              in_timing, stream);
            if (rc != RW_OK) return rc;
        }
        return RW_OK;
    }

    // one key datum of emitted / spilled row r into a memcomparable key or
    // a value row
    void encode_key_datum(std::vector<uint8_t>& buf, bool memcmp_key, int k,
                          uint32_t r, bool null, long long word) const {
        if ((vc_mask >> k) & 1) {
            uint64_t o = vk_offs[k][r];
            uint32_t len = (uint32_t)(vk_offs[k][r + 1] - o);
            const uint8_t* s = vk_bytes[k].data() + o;
            if (memcmp_key) rwcodec::memcmp_encode_str(buf, null, s, len);
            else rwcodec::value_encode_str(buf, null, s, len);
            return;
        }
        rwcodec::DatumC d{null, word, 0};
        if (memcmp_key) rwcodec::memcmp_encode_datum(buf, out_types[k], d, {});
        else rwcodec::value_encode_datum(buf, out_types[k], d);
    }

    // Tiles (256 rows) per wave for the dense kernel's span mapping: the
    // fewest with which the capped grid covers the rows. Launches of up to
    // 2M rows keep one tile per wave, and with it all their parallelism;
    // a 16.7M-row epoch at the 2048-block cap gets 8.
    static uint32_t span_tiles_for(uint32_t rows, int grid) {
        uint32_t tiles = (rows + 255) / 256;
        uint32_t waves = (uint32_t)grid * 4;
        return (tiles + waves - 1) / waves;
    }
    uint32_t span_tiles_override = 0; // rw_agg_debug_set_span_tiles

    // Fused checkpoint flush (rw_agg_apply_flush_launch): the
    // span kernel's last-arriving block runs the flush. ONE block moves a
    // slot's scattered lines at ~70 GB/s, and on the MI355X that lost to the
    // flush launch at every dirty count measured (64 groups: +1.4 %, 1024:
    // +66 %), so the path is OFF unless RW_AGG_FUSE_FLUSH=1 asks for it
    // (read when the executor is created). Enabled, the dirty-count policy
    // guards it: the host cannot read the count on the asynchronous path;
    // every flush records the largest count it has seen in counters[5],
    // check_overflow() copies it at every sync, and fusion is allowed only
    // once a sync has shown it at most FUSE_MAX. The mark never falls: one
    // large flush turns fusion off for good.
    static constexpr uint32_t FUSE_MAX = 64;
    bool fuse_env = false; // RW_AGG_FUSE_FLUSH=1
    int fuse_mode = 0; // rw_agg_debug_set_fuse: 0 policy, 1 always, 2 never
    bool dirty_hwm_known = false;
    uint32_t dirty_hwm = 0;
    uint64_t fused_launches = 0; // rw_agg_debug_fused_launches

    static bool flush_fast_enabled() {
        static int en = [] {
            const char* e = getenv("RW_AGG_FLUSH_FAST");
            return !(e && *e == '0');
        }();
        return en;
    }
    bool fuse_allowed() const {
        if (fuse_mode == 2) return false;
        if (!flush_fast_enabled() || n_dec || n_minput || eowc) return false;
        if (fuse_mode == 1) return true;
        return fuse_env && dirty_hwm_known && dirty_hwm <= FUSE_MAX;
    }

    // apply_range's HIP event pair costs ~5 us of a ~62 us epoch step on
    // this runtime: it is recorded on one launch in
    // 16, the first after a stats reset included, and only recorded
    // launches count in apply_launches / apply_rows / ring.ms_total, so the
    // averages stay averages (A/B via RW_AGG_EVENT_EVERY=1).
    static uint32_t ev_every() {
        static uint32_t n = [] {
            const char* e = getenv("RW_AGG_EVENT_EVERY");
            int v = e ? atoi(e) : 0;
            return (uint32_t)(v > 0 ? v : 16);
        }();
        return n;
    }
    uint32_t ev_seq = 0;

    AggCallDev cd(int i) const {
        if (i < n_calls) {
            int8_t mord = 0, dord = 0;
            for (int j = 0; j < i; j++) {
                mord += call_minput[j];
                dord += call_decimal[j];
            }
            return AggCallDev{calls[i].kind, calls[i].arg, call_minput[i],
                              mord, call_decimal[i], dord};
        }
        return AggCallDev{0, -1, 0, 0, 0, 0};
    }

    int init(const RwHashAggDesc* d) {
        if (!gpu_ok()) FAIL(RW_E_NOGPU, "risingwave_amd: no GPU visible (product path has no CPU fallback)");
        desc = *d;
        eowc = d->emit_on_window_close != 0;
        if (const char* e = getenv("RW_AGG_FUSE_FLUSH")) fuse_env = *e == '1';
        if (const char* e = getenv("RW_AGG_INTERN_TIMING")) in_timing = *e == '1';
        input_types.assign(d->input_types, d->input_types + d->n_input_cols);
        group_key.assign(d->group_key_indices, d->group_key_indices + d->n_group_key);
        calls.assign(d->calls, d->calls + d->n_calls);
        KW = (int)group_key.size();
        n_calls = (int)calls.size();
        if (KW < 1 || KW > MAX_KW) FAIL(RW_E_INVAL, "group key width %d unsupported (1..%d)", KW, MAX_KW);
        if (n_calls < 1 || n_calls > 4) FAIL(RW_E_INVAL, "n_calls %d unsupported (1..4 in round-1 kernels)", n_calls);
        for (int i = 0; i < KW; i++) {
            uint8_t ty = input_types[group_key[i]];
            if (ty == RW_T_VARCHAR) {
                vc_mask |= 1u << i;
                vpos[nv++] = i;
            } else if (ty != RW_T_I64 && ty != RW_T_TS) {
                FAIL(RW_E_INVAL, "group key type %d unsupported on GPU (i64/ts/varchar only)", ty);
            }
        }
        if (has_vc()) {
            // scope of varchar group keys (rw_stream.h)
            if (eowc)
                FAIL(RW_E_INVAL, "varchar group key + emit_on_window_close unsupported");
            for (auto& c : calls) {
                if (c.distinct)
                    FAIL(RW_E_INVAL, "varchar group key + DISTINCT call unsupported");
                if ((c.kind == RW_AGG_MIN || c.kind == RW_AGG_MAX) &&
                    !d->append_only)
                    FAIL(RW_E_INVAL,
                         "varchar group key + materialized-input min/max "
                         "unsupported (append-only min/max is)");
            }
        }
        stream_key.assign(d->stream_key, d->stream_key + d->n_stream_key);
        for (auto& c : calls) {
            if (c.kind > RW_AGG_MAX) FAIL(RW_E_INVAL, "agg kind %d", c.kind);
            bool minput = (c.kind == RW_AGG_MIN || c.kind == RW_AGG_MAX) &&
                          !d->append_only;
            call_minput.push_back(minput);
            n_minput += minput;
            bool dec = false;
            if (c.arg >= 0) {
                uint8_t ty = input_types[c.arg];
                if (ty == RW_T_DECIMAL) {
                    // decimal scope: non-DISTINCT sum/count
                    // arguments, non-EOWC executors
                    if (c.distinct ||
                        !(c.kind == RW_AGG_SUM || c.kind == RW_AGG_SUM0 ||
                          c.kind == RW_AGG_COUNT))
                        FAIL(RW_E_INVAL,
                             "decimal supported as non-DISTINCT sum/count "
                             "arguments only");
                    if (eowc)
                        FAIL(RW_E_INVAL, "decimal + EOWC unsupported");
                    dec = c.kind != RW_AGG_COUNT; // count needs only validity
                } else if (ty != RW_T_I64 && ty != RW_T_TS) {
                    FAIL(RW_E_INVAL, "agg arg type %d unsupported on GPU (i64/ts only)", ty);
                }
            }
            call_decimal.push_back(dec);
            n_dec += dec;
        }
        for (auto k : stream_key)
            if (input_types[k] == RW_T_DECIMAL)
                FAIL(RW_E_INVAL, "decimal stream keys unsupported");
        // DISTINCT dedup (aggregate/distinct.rs): one counter table per
        // distinct column. min/max DISTINCT ≡ min/max — the frontend strips
        // it — so distinct over a materialized-input call is rejected.
        call_dedup_idx.assign(calls.size(), -1);
        for (size_t ci = 0; ci < calls.size(); ci++) {
            if (!calls[ci].distinct || calls[ci].arg < 0) continue;
            if (call_minput[ci])
                FAIL(RW_E_INVAL,
                     "DISTINCT min/max is min/max — plan should strip it");
            if (KW + 1 > MAX_KW)
                FAIL(RW_E_INVAL, "group key too wide for DISTINCT dedup");
            int slot = KW + (int)ci; // arg column's batch slot
            size_t di = 0;
            for (; di < distinct_slots.size(); di++)
                if (distinct_slots[di] == slot) break;
            // distinct calls on the same arg COLUMN may use different batch
            // slots (args are duplicated per call) — dedupe by source col
            for (size_t cj = 0; cj < ci; cj++)
                if (call_dedup_idx[cj] >= 0 && calls[cj].arg == calls[ci].arg) {
                    di = (size_t)call_dedup_idx[cj];
                    break;
                }
            if (di == distinct_slots.size()) {
                distinct_slots.push_back(slot);
                distinct_col_types.push_back(input_types[calls[ci].arg]);
            }
            call_dedup_idx[ci] = (int)di;
        }
        if (n_minput) {
            if (stream_key.size() > 2)
                FAIL(RW_E_INVAL, "stream key wider than 2 unsupported for GPU minput state");
            for (auto sk : stream_key) {
                uint8_t ty = input_types[sk];
                if (ty != RW_T_I64 && ty != RW_T_TS)
                    FAIL(RW_E_INVAL, "stream key type %d unsupported on GPU", ty);
            }
        }
        out_width = KW + n_calls;
        for (auto k : group_key) out_types.push_back(input_types[k]);
        for (auto& c : calls) out_types.push_back(c.ret_type);
        capacity = 1u << 20;
        if (desc.state_capacity_hint) {
            capacity = 1;
            while (capacity < desc.state_capacity_hint) capacity <<= 1;
        }
        HIP_TRY(hipStreamCreate(&stream));
        size_t cap = capacity;
        t.cap_mask = capacity - 1;
        HIP_TRY(mem.alloc(&t.state, cap * 4));
        HIP_TRY(hipMemset(t.state, 0, cap * 4));
        HIP_TRY(mem.alloc(&t.keys, cap * KW * 8));
        HIP_TRY(mem.alloc(&t.key_nulls, cap * 4));
        HIP_TRY(mem.alloc(&t.acc, cap * n_calls * 8));
        HIP_TRY(mem.alloc(&t.has, cap * n_calls));
        HIP_TRY(hipMemset(t.has, 0, cap * n_calls));
        HIP_TRY(mem.alloc(&t.prev, cap * n_calls * 8));
        HIP_TRY(mem.alloc(&t.prev_null, cap * n_calls));
        HIP_TRY(mem.alloc(&t.has_prev, cap));
        HIP_TRY(hipMemset(t.has_prev, 0, cap));
        HIP_TRY(mem.alloc(&t.dirty_flag, cap * 4));
        HIP_TRY(hipMemset(t.dirty_flag, 0, cap * 4));
        HIP_TRY(mem.alloc(&t.dirty_list, cap * 4));
        HIP_TRY(mem.alloc(&t.counters, AGG_CTR_WORDS * 4));
        HIP_TRY(hipMemset(t.counters, 0, AGG_CTR_WORDS * 4));
        t.out_capacity = 1u << 22;
        HIP_TRY(mem.alloc(&t.out_vals, (size_t)t.out_capacity * out_width * 8));
        HIP_TRY(mem.alloc(&t.out_nulls, (size_t)t.out_capacity * out_width));
        HIP_TRY(mem.alloc(&t.out_ops, t.out_capacity));
        t.n_dec = n_dec;
        if (n_dec) {
            HIP_TRY(mem.alloc(&t.dsum, (size_t)n_dec * 4 * cap * 8));
            HIP_TRY(hipMemset(t.dsum, 0, (size_t)n_dec * 4 * cap * 8));
            HIP_TRY(mem.alloc(&t.dscl, (size_t)n_dec * cap * 4));
            HIP_TRY(hipMemset(t.dscl, 0, (size_t)n_dec * cap * 4));
            HIP_TRY(mem.alloc(&t.dspec, (size_t)n_dec * 3 * cap * 8));
            HIP_TRY(hipMemset(t.dspec, 0, (size_t)n_dec * 3 * cap * 8));
            HIP_TRY(mem.alloc(&t.out_vals2,
                              (size_t)t.out_capacity * out_width * 8));
            HIP_TRY(mem.alloc(&t.prev2, (size_t)n_calls * cap * 8));
            HIP_TRY(hipMemset(t.prev2, 0, (size_t)n_calls * cap * 8));
        }
        t.n_sk = (int)stream_key.size();
        if (n_minput) {
            t.mrow_cap = 1u << 22;
            if (desc.state_capacity_hint) {
                uint64_t want = desc.state_capacity_hint * 8;
                t.mrow_cap = 1;
                while (t.mrow_cap < want && t.mrow_cap < (1u << 28)) t.mrow_cap <<= 1;
            }
            HIP_TRY(mem.alloc(&t.mheads, (size_t)n_minput * cap * 4));
            HIP_TRY(hipMemset(t.mheads, 0xFF, (size_t)n_minput * cap * 4));
            HIP_TRY(mem.alloc(&t.mval, (size_t)t.mrow_cap * 8));
            HIP_TRY(mem.alloc(&t.mval_null, t.mrow_cap));
            size_t nsk = t.n_sk ? t.n_sk : 1;
            HIP_TRY(mem.alloc(&t.msk, nsk * t.mrow_cap * 8));
            HIP_TRY(mem.alloc(&t.msk_null, nsk * t.mrow_cap));
            HIP_TRY(mem.alloc(&t.mnext, (size_t)t.mrow_cap * 4));
            HIP_TRY(mem.alloc(&t.malive, (size_t)t.mrow_cap * 4));
            HIP_TRY(mem.alloc(&t.mcursor, 4));
            HIP_TRY(hipMemset(t.mcursor, 0, 4));
            HIP_TRY(mem.alloc(&t.mslot, (size_t)t.mrow_cap * 4));
            HIP_TRY(mem.alloc(&t.mcall, t.mrow_cap));
            t.mkilled_cap = 1u << 22;
            HIP_TRY(mem.alloc(&t.mkilled, (size_t)t.mkilled_cap * 4));
            HIP_TRY(mem.alloc(&t.mkilled_cursor, 4));
            HIP_TRY(hipMemset(t.mkilled_cursor, 0, 4));
        }
        agg_init_kernel<<<2048, 256, 0, stream>>>(t, n_calls, cd(0), cd(1), cd(2),
                                                  cd(3));
        HIP_TRY(hipStreamSynchronize(stream));
        return RW_OK;
    }

    int n_batch_slots() const { return KW + n_calls + (n_minput ? (int)stream_key.size() : 0); }

    int ensure_stage(uint32_t n_rows) {
        if (stage_cap >= n_rows) return RW_OK;
        stage_cap = 0;
        uint32_t cap = 4096;
        while (cap < n_rows) cap <<= 1;
        // 16 B/row so decimal slots (2 words/row) fit
        int rc = stage_regrow(mem, stage, n_batch_slots(), cap, 16);
        if (rc != RW_OK) return rc;
        stage_cap = cap;
        return RW_OK;
    }

    // upload one host chunk into a device AggBatch (batch cols = group key
    // cols then per-call arg cols, i64)
    int upload(const RwChunk* c, AggBatch* out, bool use_stage) {
        uint32_t n = c->n_rows;
        AggBatch b{};
        // varchar key columns: validate every offsets array BEFORE any copy
        // or state change, then size the interning state for this chunk
        uint64_t vbytes_total = 0;
        if (has_vc()) {
            if (!use_stage)
                FAIL(RW_E_INVAL, "varchar group keys: device-resident batches unsupported");
            int rc = intern_validate(c, &vbytes_total);
            if (rc != RW_OK) return rc;
            rc = intern_prepare((uint64_t)n * nv, vbytes_total);
            if (rc != RW_OK) return rc;
        }
        if (use_stage) {
            int rc = ensure_stage(n);
            if (rc != RW_OK) return rc;
            b = stage;
        }
        uint64_t vbase = 0; // staging offset of the next varchar column
        auto upcol = [&](int bi, uint32_t col_idx) -> int {
            const RwColumn& col = c->cols[col_idx];
            if (bi < KW && ((vc_mask >> bi) & 1)) {
                // bytes go to the STAGING buffer (not the arena); the words
                // staged where i64 values go are provisional
                auto* vd = (const RwVarlenData*)col.data;
                uint64_t total = n ? vd->offsets[n] : 0;
                if (total)
                    HIP_TRY(hipMemcpyAsync(in_stg + vbase, vd->bytes, total,
                                           hipMemcpyHostToDevice, stream));
                rwvarlen::ref_words(vd, col.valid, n, vbase, rwvarlen::PROV_BIT,
                                    vwords[bi]);
                vbase += total;
                return upload_col(b.col_vals[bi], b.col_valid[bi],
                                  vwords[bi].data(), col.valid, n, 8, stream);
            }
            size_t w = 8;
            if (col.type == RW_T_DECIMAL) w = 16; // 2 words/row
            else if (col.type != RW_T_I64 && col.type != RW_T_TS)
                FAIL(RW_E_INVAL, "column type %d unsupported on GPU", col.type);
            return upload_col(b.col_vals[bi], b.col_valid[bi], col.data,
                              col.valid, n, w, stream);
        };
        for (int i = 0; i < KW; i++) {
            int rc = upcol(i, group_key[i]);
            if (rc != RW_OK) return rc;
        }
        for (int ci = 0; ci < n_calls; ci++) {
            if (calls[ci].arg >= 0) {
                int rc = upcol(KW + ci, (uint32_t)calls[ci].arg);
                if (rc != RW_OK) return rc;
            } else {
                HIP_TRY(hipMemsetAsync(b.col_valid[KW + ci], 1, n, stream));
            }
        }
        if (n_minput) {
            for (size_t j = 0; j < stream_key.size(); j++) {
                int rc = upcol(KW + n_calls + (int)j, stream_key[j]);
                if (rc != RW_OK) return rc;
            }
        }
        int rc = upload_ops_vis(b, c, stream);
        if (rc != RW_OK) return rc;
        // dense fast path: every row visible, Insert, and non-null in every
        // referenced column — the kernel then skips the three byte streams
        b.dense = (c->vis == nullptr);
        for (uint32_t r = 0; b.dense && r < n; r++) b.dense = c->ops[r] == 0;
        auto col_all_valid = [&](uint32_t col_idx) {
            const uint8_t* v = c->cols[col_idx].valid;
            for (uint32_t r = 0; r < n; r++)
                if (!v[r]) return false;
            return true;
        };
        for (int i = 0; b.dense && i < KW; i++)
            b.dense = col_all_valid(group_key[i]);
        for (int ci = 0; b.dense && ci < n_calls; ci++)
            if (calls[ci].arg >= 0) b.dense = col_all_valid((uint32_t)calls[ci].arg);
        if (n_minput)
            for (size_t jx = 0; b.dense && jx < stream_key.size(); jx++)
                b.dense = col_all_valid(stream_key[jx]);
        *out = b;
        return RW_OK;
    }

    // `fuse`: carry the checkpoint flush in the launch where the launch is
    // a span one; returns whether it did.
    bool launch_apply(const AggBatch& b, uint32_t r0, uint32_t r1,
                      bool fuse = false) {
        auto a0 = cd(0), a1 = cd(1), a2 = cd(2), a3 = cd(3);
        if (b.dense && KW == 1 && b.stride == 1 && n_minput == 0 &&
            n_dec == 0 && distinct_slots.empty() &&
            ((uintptr_t)(b.col_vals[0] + r0) & 31) == 0 &&
            (r1 - r0) >= 1024) {
            int grid = grid_for((r1 - r0 + RPL - 1) / RPL);
            // CS: count-star carried as run length beside the scan instead
            // of an i64 inside it
            int cs = -1;
            for (int ci = 0; ci < n_calls && cs < 0; ci++)
                if (cd(ci).arg < 0 && cd(ci).kind == RW_AGG_COUNT_STAR) cs = ci;
            // SPAN: contiguous per-wave spans with a carried run
            // (A/B via RW_AGG_SPAN=0: the grid-stride mapping)
            static int span_en = [] {
                const char* e = getenv("RW_AGG_SPAN");
                return !(e && *e == '0');
            }();
            uint32_t tiles = (r1 - r0 + 64 * RPL - 1) / (64 * RPL);
            uint32_t st = span_tiles_override ? span_tiles_override
                                              : span_tiles_for(r1 - r0, grid);
            uint32_t waves = (tiles + st - 1) / st;
            int sgrid = (int)((waves + 3) / 4);
            // the fused tail's flush arguments: call kinds one per byte,
            // row_count_index above them
            uint32_t farg = (uint32_t)desc.row_count_index << 16;
            for (int ci = 0; ci < n_calls && ci < 2; ci++)
                farg |= (uint32_t)calls[ci].kind << (8 * ci);
            #define RW_DCS(nc, csv)                                           \
                do {                                                          \
                    if (span_en && fuse)                                      \
                        agg_apply_dense4_kernel_span<nc, csv, true>           \
                            <<<sgrid, 256, 0, stream>>>(b, t, a0, a1, a2, a3, \
                                                        r0, r1, st, farg);    \
                    else if (span_en)                                         \
                        agg_apply_dense4_kernel_span<nc, csv>                 \
                            <<<sgrid, 256, 0, stream>>>(b, t, a0, a1, a2, a3, \
                                                        r0, r1, st, 0u);      \
                    else                                                      \
                        agg_apply_dense4_kernel_w8<nc, csv>                   \
                            <<<grid, 256, 0, stream>>>(b, t, a0, a1, a2, a3,  \
                                                       r0, r1);               \
                } while (0)
            #define RW_DENSE(nc)                                              \
                agg_apply_dense4_kernel<nc><<<grid, 256, 0, stream>>>(        \
                    b, t, a0, a1, a2, a3, r0, r1)
            // the count-star shapes of q7 ([count], [max|sum, count] either
            // way round) have the CS kernels; every other shape, count-star
            // with 3 or 4 calls included, takes the generic one
            switch (cs < 0 ? -1 : n_calls * 8 + cs) {
                case 1 * 8 + 0: RW_DCS(1, 0); return span_en && fuse;
                case 2 * 8 + 0: RW_DCS(2, 0); return span_en && fuse;
                case 2 * 8 + 1: RW_DCS(2, 1); return span_en && fuse;
            }
            switch (n_calls) {
                case 1: RW_DENSE(1); return false;
                case 2: RW_DENSE(2); return false;
                case 3: RW_DENSE(3); return false;
                case 4: RW_DENSE(4); return false;
            }
            #undef RW_DCS
            #undef RW_DENSE
        }
        int grid = grid_for(r1 - r0);
        #define RW_LAUNCH(kw, nc)                                             \
            do {                                                              \
                if (b.dense)                                                  \
                    agg_apply_kernel<kw, nc, true><<<grid, 256, 0, stream>>>( \
                        b, t, a0, a1, a2, a3, r0, r1);                        \
                else                                                          \
                    agg_apply_kernel<kw, nc, false><<<grid, 256, 0, stream>>>(\
                        b, t, a0, a1, a2, a3, r0, r1);                        \
            } while (0)
        switch (KW * 8 + n_calls) {
            case 1 * 8 + 1: RW_LAUNCH(1, 1); break;
            case 1 * 8 + 2: RW_LAUNCH(1, 2); break;
            case 1 * 8 + 3: RW_LAUNCH(1, 3); break;
            case 1 * 8 + 4: RW_LAUNCH(1, 4); break;
            case 2 * 8 + 1: RW_LAUNCH(2, 1); break;
            case 2 * 8 + 2: RW_LAUNCH(2, 2); break;
            case 2 * 8 + 3: RW_LAUNCH(2, 3); break;
            case 2 * 8 + 4: RW_LAUNCH(2, 4); break;
            case 3 * 8 + 1: RW_LAUNCH(3, 1); break;
            case 3 * 8 + 2: RW_LAUNCH(3, 2); break;
            case 3 * 8 + 3: RW_LAUNCH(3, 3); break;
            case 3 * 8 + 4: RW_LAUNCH(3, 4); break;
            case 4 * 8 + 1: RW_LAUNCH(4, 1); break;
            case 4 * 8 + 2: RW_LAUNCH(4, 2); break;
            case 4 * 8 + 3: RW_LAUNCH(4, 3); break;
            case 4 * 8 + 4: RW_LAUNCH(4, 4); break;
        }
        #undef RW_LAUNCH
        return false;
    }

    int apply(const AggBatch& b, bool timed,
              const std::vector<uint32_t>& seg_bounds = {}) {
        int slot = -1;
        if (timed) {
            slot = ring.begin(stream);
            if (slot < 0) FAIL(RW_E_INTERNAL, "HIP event error (apply timing)");
        }
        uint32_t start = 0;
        for (uint32_t bnd : seg_bounds) {
            if (bnd > start) launch_apply(b, start, bnd);
            start = bnd;
        }
        if (start < b.n_rows) launch_apply(b, start, b.n_rows);
        if (timed) {
            HIP_TRY(ring.end(slot, stream));
            apply_launches++;
            apply_rows += b.n_rows;
        }
        return RW_OK;
    }

    // apply a sub-range of a device batch as one launch (epoch-granular
    // ingestion: chunks buffered within an epoch are applied together)
    // `fuse`/`fused`: as launch_apply's flag and result.
    int apply_range(const AggBatch& b, uint32_t r0, uint32_t r1, bool timed,
                    bool fuse = false, bool* fused = nullptr) {
        int slot = -1;
        timed = timed && ev_seq++ % ev_every() == 0;
        if (timed) {
            slot = ring.begin(stream);
            if (slot < 0) FAIL(RW_E_INTERNAL, "HIP event error (apply timing)");
        }
        bool did = launch_apply(b, r0, r1, fuse);
        if (fused) *fused = did;
        fused_launches += did;
        if (timed) {
            HIP_TRY(ring.end(slot, stream));
            apply_launches++;
            apply_rows += r1 - r0;
        }
        return RW_OK;
    }

    // A minput DELETE targeting a row INSERTed earlier in the same chunk
    // must observe that insert (the reference applies rows in order,
    // hash_agg.rs:332-398); the parallel kernel keeps that only across
    // launches, so such deletes run in their own single-row segments.
    std::vector<uint32_t> minput_conflict_segments(const RwChunk* c) {
        std::vector<uint32_t> bounds;
        if (!n_minput) return bounds;
        bool any_delete = false;
        for (uint32_t r = 0; r < c->n_rows && !any_delete; r++)
            any_delete = c->ops[r] == RW_OP_DELETE || c->ops[r] == RW_OP_UPDATE_DELETE;
        if (!any_delete) return bounds;
        auto row_key = [&](uint32_t r) {
            // (group key, per-minput arg, stream key) — conservative match
            std::string k;
            auto add = [&](uint32_t col) {
                uint8_t valid = c->cols[col].valid[r];
                k.push_back((char)valid);
                int64_t v = valid ? ((const int64_t*)c->cols[col].data)[r] : 0;
                k.append((const char*)&v, 8);
            };
            for (auto g : group_key) add(g);
            for (int ci = 0; ci < n_calls; ci++)
                if (call_minput[ci] && calls[ci].arg >= 0) add((uint32_t)calls[ci].arg);
            for (auto sk : stream_key) add(sk);
            return k;
        };
        std::unordered_multiset<std::string> inserts;
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            if (c->ops[r] == RW_OP_INSERT || c->ops[r] == RW_OP_UPDATE_INSERT)
                inserts.insert(row_key(r));
        }
        if (inserts.empty()) return bounds;
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            if ((c->ops[r] == RW_OP_DELETE || c->ops[r] == RW_OP_UPDATE_DELETE) &&
                inserts.count(row_key(r))) {
                bounds.push_back(r);
                bounds.push_back(r + 1);
            }
        }
        return bounds;
    }

    int ensure_dedup(uint32_t n) {
        if (dedup_slots.empty()) {
            size_t cap = 1;
            size_t hint = (size_t)capacity * 4;
            if (hint < (1u << 16)) hint = 1u << 16;
            while (cap < hint) cap <<= 1;
            dedup_cap_mask = (uint32_t)(cap - 1);
            for (size_t di = 0; di < distinct_slots.size(); di++) {
                JoinSlot* sl = nullptr;
                HIP_TRY(mem.alloc(&sl, cap * sizeof(JoinSlot)));
                dedup_init_kernel<<<2048, 256, 0, stream>>>(sl, cap);
                dedup_slots.push_back(sl);
                uint32_t *df = nullptr, *dl = nullptr, *dn = nullptr;
                HIP_TRY(mem.alloc(&df, cap * 4));
                HIP_TRY(hipMemset(df, 0, cap * 4));
                HIP_TRY(mem.alloc(&dl, cap * 4));
                HIP_TRY(mem.alloc(&dn, 4));
                HIP_TRY(hipMemset(dn, 0, 4));
                ddirty_flag.push_back(df);
                ddirty_list.push_back(dl);
                ddirty_n.push_back(dn);
                dedup_persisted.emplace_back(cap, 0);
            }
        }
        if (hidden_cap < n) {
            hidden_cap = 0;
            for (auto*& hb : hidden_bufs) mem.release(&hb);
            hidden_bufs.assign(distinct_slots.size(), nullptr);
            for (size_t di = 0; di < distinct_slots.size(); di++)
                HIP_TRY(mem.alloc(&hidden_bufs[di], n));
            hidden_cap = n;
        }
        return RW_OK;
    }

    // ----- product-reachable epoch-batched ingestion (VERDICT r01 item
    // 7): with ingest mode ON, push_chunk STAGES the chunk into a growing
    // device epoch buffer (H2D + D2D append; no apply launch), and the
    // barrier flush applies the whole epoch as ONE kernel launch — the
    // same one-launch-per-epoch shape as the bench's preloaded path, but
    // reachable from the INTEGRATION.md binding. Legal because
    // sum/count/min/max value states are order-free over the epoch's row
    // multiset; rejected for materialized-input or DISTINCT
    // aggregates (their per-chunk passes are order-sensitive). -----
    bool epoch_ingest = false;
    AggBatch ebuf{};
    uint64_t ecap = 0, erows = 0;
    bool edense = true;

    int ensure_epoch(uint64_t need) {
        if (ecap >= need) return RW_OK;
        uint64_t cap = ecap ? ecap : (1ull << 21);
        while (cap < need) cap <<= 1;
        // the last epoch's apply launch may still read the old buffers
        HIP_TRY(hipStreamSynchronize(stream));
        ecap = 0;
        int slots = n_batch_slots();
        for (int i = 0; i < slots; i++) {
            HIP_TRY(mem.regrow(&ebuf.col_vals[i], cap * 8, erows * 8, stream,
                               true));
            HIP_TRY(mem.regrow(&ebuf.col_valid[i], cap, erows, stream, true));
        }
        HIP_TRY(mem.regrow(&ebuf.ops, cap, erows, stream, true));
        ecap = cap;
        return RW_OK;
    }

    int epoch_append(const RwChunk* c) {
        if (c->vis)
            FAIL(RW_E_INVAL,
                 "epoch-batched ingest requires visibility-compacted chunks");
        AggBatch b;
        int rc = upload(c, &b, true); // H2D into the pinned-staged buffers
        if (rc != RW_OK) return rc;
        uint32_t n = c->n_rows;
        rc = ensure_epoch(erows + n);
        if (rc != RW_OK) return rc;
        int slots = n_batch_slots();
        for (int i = 0; i < slots; i++) {
            HIP_TRY(hipMemcpyAsync(ebuf.col_vals[i] + erows, b.col_vals[i],
                                   (size_t)n * 8, hipMemcpyDeviceToDevice,
                                   stream));
            HIP_TRY(hipMemcpyAsync(ebuf.col_valid[i] + erows, b.col_valid[i],
                                   n, hipMemcpyDeviceToDevice, stream));
        }
        HIP_TRY(hipMemcpyAsync(ebuf.ops + erows, b.ops, n,
                               hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream)); // staging buffer reuse
        edense = edense && b.dense;
        erows += n;
        return RW_OK;
    }

    // apply the staged epoch as one launch (called from flush)
    int epoch_apply() {
        if (!erows) return RW_OK;
        AggBatch b = ebuf;
        b.vis = nullptr;
        b.n_rows = (uint32_t)erows;
        b.dense = edense ? 1 : 0;
        int rc = apply(b, true);
        if (rc != RW_OK) return rc;
        erows = 0;
        edense = true;
        return RW_OK;
    }

    int push_chunk(const RwChunk* c) {
        if (epoch_ingest) return epoch_append(c);
        AggBatch b;
        int rc = upload(c, &b, true);
        if (rc != RW_OK) return rc;
        if (has_vc()) {
            // make the batch's varchar key words canonical;
            // from here on the batch is an i64 batch
            InternCols ic{};
            for (int j = 0; j < nv; j++) ic.words[j] = b.col_vals[vpos[j]];
            ic.vis = b.vis;
            ic.n_rows = b.n_rows;
            ic.nv = (uint32_t)nv;
            ic.stride = 1;
            rc = intern_run(ic);
            if (rc != RW_OK) return rc;
        }
        if (!distinct_slots.empty()) {
            rc = ensure_dedup(c->n_rows);
            if (rc != RW_OK) return rc;
            int grid = grid_for(c->n_rows);
            for (size_t di = 0; di < distinct_slots.size(); di++)
                agg_dedup_kernel<<<grid, 256, 0, stream>>>(
                    b, dedup_slots[di], dedup_cap_mask, KW, distinct_slots[di],
                    hidden_bufs[di], &t.counters[2], ddirty_flag[di],
                    ddirty_list[di], ddirty_n[di]);
            for (size_t ci = 0; ci < calls.size(); ci++)
                if (call_dedup_idx[ci] >= 0)
                    b.call_hidden[ci] = hidden_bufs[call_dedup_idx[ci]];
        }
        rc = apply(b, true, minput_conflict_segments(c));
        if (rc != RW_OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream)); // staging buffer reuse
        if (in_ev_pending && intern_harvest() != RW_OK) return RW_E_INTERNAL;
        return check_overflow();
    }

    int check_overflow() {
        uint32_t ctr[6];
        HIP_TRY(hipMemcpy(ctr, t.counters, 24, hipMemcpyDeviceToHost));
        dirty_hwm = ctr[5]; // fuse_allowed()
        dirty_hwm_known = true;
        if (ctr[2] == 1) FAIL(RW_E_INTERNAL, "agg state table full (capacity %u)", capacity);
        if (ctr[2] == 2) FAIL(RW_E_INTERNAL, "agg output buffer overflow");
        if (ctr[2] == 3) FAIL(RW_E_INTERNAL, "agg minput row store full");
        if (ctr[2] == 4) FAIL(RW_E_INTERNAL, "agg distinct dedup table full");
        if (ctr[2] == AGG_ERR_INTERN)
            FAIL(RW_E_INTERNAL, "agg varchar group-key intern table or arena full");
        if (ctr[2] == 5)
            FAIL(RW_E_OVERFLOW,
                 "decimal sum outside the exact 96-bit domain (the "
                 "reference's order-dependent rescale path; unsupported)");
        return RW_OK;
    }

    // Grow the flush output buffers to hold `need` rows. Called on the sync
    // flush paths BEFORE launching the flush kernel (the kernel clears dirty
    // flags and updates prev as it emits, so an overflowed launch is not
    // retryable): large dirty sets — e.g. q3's 512k-order windows × 16-step
    // epochs — emit up to 2 rows per dirty group.
    int ensure_out_capacity(uint64_t need) {
        if (need <= t.out_capacity) return RW_OK;
        uint64_t cap = t.out_capacity;
        while (cap < need) cap <<= 1;
        if (cap > UINT32_MAX) FAIL(RW_E_INVAL, "flush output > 4G rows");
        mem.release(&t.out_vals);
        mem.release(&t.out_nulls);
        mem.release(&t.out_ops);
        HIP_TRY(mem.alloc(&t.out_vals, (size_t)cap * out_width * 8));
        HIP_TRY(mem.alloc(&t.out_nulls, (size_t)cap * out_width));
        HIP_TRY(mem.alloc(&t.out_ops, cap));
        if (n_dec)
            HIP_TRY(mem.regrow(&t.out_vals2, (size_t)cap * out_width * 8));
        t.out_capacity = (uint32_t)cap;
        return RW_OK;
    }

    // sync the stream, read the dirty count, and size the output buffers for
    // the worst case (2 rows per dirty group) ahead of the flush launch
    int presize_flush_out(uint32_t* n_dirty = nullptr) {
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t nd = 0;
        HIP_TRY(hipMemcpy(&nd, t.counters, 4, hipMemcpyDeviceToHost));
        if (n_dirty) *n_dirty = nd;
        return ensure_out_capacity((uint64_t)nd * 2);
    }

    // The one place the change-inference flush is launched from.
    // `n_dirty` is the exact dirty count where the caller has just read it
    // (the host-synchronous paths), or -1 on the stream-ordered path, which
    // also wants counters[0..1] zeroed behind the flush (`stream_reset`).
    // Value-state executors take agg_flush_fast_kernel: the grid is sized
    // to the count when it is known; unknown, 2048 one-wave blocks cover
    // 128K slots per grid-stride pass, blocks past the dirty count exit on
    // their first load, and at most 2048 blocks ever draw a reset ticket. Decimal and
    // materialized-input executors, or RW_AGG_FLUSH_FAST=0 (A/B), keep the
    // generic kernel at its fixed grid with the separate reset launch.
    void launch_flush(long long n_dirty, bool stream_reset) {
        if (flush_fast_enabled() && n_dec == 0 && n_minput == 0) {
            if (n_dirty == 0) return; // counters already read back as idle
            // One-wave blocks: a slot's state is a dozen scattered lines, and
            // one CU moves only ~70 GB/s of those (a 256-slot block takes
            // ~8 us), so a q7 checkpoint's 1024 slots go to 16
            // CUs instead of 4. Thread counts are as with 256-thread blocks
            // (A/B via RW_AGG_FLUSH_BLOCK=256).
            static int bs = [] {
                const char* e = getenv("RW_AGG_FLUSH_BLOCK");
                return e && atoi(e) == 256 ? 256 : 64;
            }();
            int grid = (n_dirty < 0 ? 512 : grid_for((uint32_t)n_dirty)) *
                       (256 / bs);
            uint32_t kinds = 0;
            for (int ci = 0; ci < n_calls; ci++)
                kinds |= (uint32_t)calls[ci].kind << (8 * ci);
            #define RW_FF(kw, nc)                                              \
                case kw * 8 + nc:                                              \
                    agg_flush_fast_kernel<kw, nc><<<grid, bs, 0, stream>>>(    \
                        t, (int)desc.row_count_index, kinds,                   \
                        stream_reset ? 1 : 0);                                 \
                    return;
            switch (KW * 8 + n_calls) {
                RW_FF(1, 1) RW_FF(1, 2) RW_FF(1, 3) RW_FF(1, 4)
                RW_FF(2, 1) RW_FF(2, 2) RW_FF(2, 3) RW_FF(2, 4)
                RW_FF(3, 1) RW_FF(3, 2) RW_FF(3, 3) RW_FF(3, 4)
                RW_FF(4, 1) RW_FF(4, 2) RW_FF(4, 3) RW_FF(4, 4)
            }
            #undef RW_FF
        }
        agg_flush_kernel<<<2048, 256, 0, stream>>>(
            t, KW, n_calls, (int)desc.row_count_index, cd(0), cd(1), cd(2),
            cd(3));
        if (stream_reset)
            agg_counters_reset_kernel<<<1, 1, 0, stream>>>(t.counters);
    }

    int flush(uint64_t) {
        if (epoch_ingest) {
            int rce = epoch_apply();
            if (rce != RW_OK) return rce;
        }
        uint32_t n_dirty = 0;
        int rcp = presize_flush_out(&n_dirty);
        if (rcp != RW_OK) return rcp;
        if (has_vc()) { // the stream is drained: exact tail / entry count
            rcp = intern_sync_counts();
            if (rcp != RW_OK) return rcp;
        }
        if (eowc) {
            // EOWC barrier (hash_agg.rs:429-474): nothing is EMITTED until a
            // watermark closes windows, but the dirty groups' current states
            // still upsert into the intermediate table (mid-window PUTs,
            // :429-460); state accumulates across epochs
            agg_eowc_dump_kernel<<<2048, 256, 0, stream>>>(
                t, KW, n_calls, (int)desc.row_count_index, cd(0), cd(1), cd(2),
                cd(3));
            HIP_TRY(hipStreamSynchronize(stream));
            int rcd = check_overflow();
            if (rcd != RW_OK) return rcd;
            uint32_t ctrd[3];
            HIP_TRY(hipMemcpy(ctrd, t.counters, 12, hipMemcpyDeviceToHost));
            if (uint32_t n_put = ctrd[1]) {
                std::vector<long long> vals((size_t)n_put * out_width);
                std::vector<uint8_t> nulls((size_t)n_put * out_width);
                HIP_TRY(hipMemcpy(vals.data(), t.out_vals, vals.size() * 8,
                                  hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(nulls.data(), t.out_nulls, nulls.size(),
                                  hipMemcpyDeviceToHost));
                std::vector<uint8_t> put_ops(n_put, RW_OP_INSERT);
                spill_records(vals, nulls, put_ops, n_put);
            }
            HIP_TRY(hipMemset(t.counters, 0, 12));
            if (!has_pending_wm) return RW_OK;
            has_pending_wm = false;
            agg_eowc_close_kernel<<<2048, 256, 0, stream>>>(
                t, KW, n_calls, (int)desc.row_count_index, pending_wm, cd(0),
                cd(1), cd(2), cd(3));
            HIP_TRY(hipStreamSynchronize(stream));
            int rc2 = check_overflow();
            if (rc2 != RW_OK) return rc2;
            uint32_t ctr2[3];
            HIP_TRY(hipMemcpy(ctr2, t.counters, 12, hipMemcpyDeviceToHost));
            uint32_t n_out = ctr2[1];
            if (n_out) {
                std::vector<long long> vals((size_t)n_out * out_width);
                std::vector<uint8_t> nulls((size_t)n_out * out_width);
                std::vector<uint8_t> ops(n_out);
                HIP_TRY(hipMemcpy(vals.data(), t.out_vals, vals.size() * 8,
                                  hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(nulls.data(), t.out_nulls, nulls.size(),
                                  hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(ops.data(), t.out_ops, n_out,
                                  hipMemcpyDeviceToHost));
                // group-key-sorted emission (SortBuffer::consume order)
                std::vector<uint32_t> order(n_out);
                for (uint32_t i = 0; i < n_out; i++) order[i] = i;
                std::sort(order.begin(), order.end(),
                          [&](uint32_t a, uint32_t b) {
                              for (int k = 0; k < KW; k++) {
                                  bool na = nulls[(size_t)a * out_width + k];
                                  bool nb = nulls[(size_t)b * out_width + k];
                                  if (na != nb) return nb; // NULLs largest
                                  if (na) continue;
                                  long long va = vals[(size_t)a * out_width + k];
                                  long long vb = vals[(size_t)b * out_width + k];
                                  if (va != vb) return va < vb;
                              }
                              return false;
                          });
                std::vector<long long> sv((size_t)n_out * out_width);
                std::vector<uint8_t> sn((size_t)n_out * out_width);
                std::vector<uint8_t> so(n_out);
                for (uint32_t i = 0; i < n_out; i++) {
                    memcpy(&sv[(size_t)i * out_width],
                           &vals[(size_t)order[i] * out_width],
                           (size_t)out_width * 8);
                    memcpy(&sn[(size_t)i * out_width],
                           &nulls[(size_t)order[i] * out_width], out_width);
                    so[i] = ops[order[i]];
                }
                // spill: every closed window leaves the state table (the
                // reference deletes all intermediate rows < wm) — DELETE
                // records for all rows, incl. the rc==0 marker rows, which
                // are then filtered out of emission
                spill_records_eowc(sv, sn, n_out);
                uint32_t m = 0;
                for (uint32_t i = 0; i < n_out; i++) {
                    if (so[i] != RW_OP_INSERT) continue;
                    if (m != i) {
                        memcpy(&sv[(size_t)m * out_width],
                               &sv[(size_t)i * out_width],
                               (size_t)out_width * 8);
                        memcpy(&sn[(size_t)m * out_width],
                               &sn[(size_t)i * out_width], out_width);
                    }
                    so[m] = RW_OP_INSERT;
                    m++;
                }
                int rcs = slice_outputs(sv, sn, so, m);
                if (rcs != RW_OK) return rcs;
            }
            HIP_TRY(hipMemset(t.counters, 0, 12));
            return RW_OK;
        }
        launch_flush(n_dirty, false);
        HIP_TRY(hipStreamSynchronize(stream));
        int rc = check_overflow();
        if (rc != RW_OK) return rc;
        uint32_t ctr[3];
        HIP_TRY(hipMemcpy(ctr, t.counters, 12, hipMemcpyDeviceToHost));
        uint32_t n_out = ctr[1];
        if (n_out) {
            std::vector<long long> vals((size_t)n_out * out_width);
            std::vector<uint8_t> nulls((size_t)n_out * out_width);
            std::vector<uint8_t> ops(n_out);
            std::vector<long long> vals2;
            if (has_vc()) { // strings of the emitted varchar key columns
                int rcv = fetch_key_strings((const uint64_t*)t.out_vals,
                                            (uint32_t)out_width, n_out);
                if (rcv != RW_OK) return rcv;
            }
            HIP_TRY(hipMemcpy(vals.data(), t.out_vals, vals.size() * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(nulls.data(), t.out_nulls, nulls.size(),
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ops.data(), t.out_ops, n_out, hipMemcpyDeviceToHost));
            if (n_dec) {
                vals2.resize(vals.size());
                HIP_TRY(hipMemcpy(vals2.data(), t.out_vals2,
                                  vals2.size() * 8, hipMemcpyDeviceToHost));
            }
            spill_records(vals, nulls, ops, n_out, vals2);
            int rcs = slice_outputs(vals, nulls, ops, n_out, vals2);
            if (rcs != RW_OK) return rcs;
        }
        HIP_TRY(hipMemset(t.counters, 0, 12));
        return RW_OK;
    }

    // EOWC close spill: one DELETE per closed (emitted) window. Paired
    // with agg_eowc_dump_kernel's per-barrier mid-window PUTs of the
    // dirty groups' current states (hash_agg.rs:429-460), the stream is
    // the full state-table view — an EOWC executor restores from it
    // (tests/test_restore.py::test_agg_eowc_restore_*).
    void spill_records_eowc(const std::vector<long long>& vals,
                            const std::vector<uint8_t>& nulls,
                            uint32_t n_out) {
        std::vector<uint8_t> k;
        for (uint32_t r = 0; r < n_out; r++) {
            k.clear();
            for (int i = 0; i < KW; i++) {
                rwcodec::DatumC d{nulls[(size_t)r * out_width + i] != 0,
                                  vals[(size_t)r * out_width + i], 0};
                rwcodec::memcmp_encode_datum(k, out_types[i], d, {});
            }
            rwcodec::put_frame(spill, 0, k);
        }
    }

    // Append state-table KV deltas for the flushed records (the spill
    // boundary of StateTable::commit, state_table.rs:1718): PUT for
    // Insert/U+, DELETE for Delete; U− rows carry no delta of their own.
    // Keys are memcomparable (ASC NULLS LAST per group-key column); values
    // are value-encoded rows of group key ++ encoded states (materialized-
    // input states encode None, agg_group.rs:417-421).
    void spill_records(const std::vector<long long>& vals,
                       const std::vector<uint8_t>& nulls,
                       const std::vector<uint8_t>& ops, uint32_t n_out,
                       const std::vector<long long>& vals2 = {}) {
        std::vector<uint8_t> k, v;
        for (uint32_t r = 0; r < n_out; r++) {
            uint8_t op = ops[r];
            if (op == RW_OP_UPDATE_DELETE) continue;
            uint8_t put = op != RW_OP_DELETE;
            k.clear();
            v.clear();
            for (int i = 0; i < KW; i++)
                encode_key_datum(k, true, i, r,
                                 nulls[(size_t)r * out_width + i] != 0,
                                 vals[(size_t)r * out_width + i]);
            if (put) {
                for (int i = 0; i < KW; i++)
                    encode_key_datum(v, false, i, r,
                                     nulls[(size_t)r * out_width + i] != 0,
                                     vals[(size_t)r * out_width + i]);
                for (int ci = 0; ci < n_calls; ci++) {
                    if (call_minput[ci]) {
                        rwcodec::value_encode_datum(v, calls[ci].ret_type,
                                                    {true, 0, 0});
                    } else {
                        size_t ix = (size_t)r * out_width + KW + ci;
                        rwcodec::DatumC d = rwcodec::datum_of_word(
                            calls[ci].ret_type, nulls[ix] != 0, vals[ix],
                            vals2.empty() ? 0 : vals2[ix]);
                        rwcodec::value_encode_datum(v, calls[ci].ret_type, d);
                    }
                }
            }
            rwcodec::put_frame(spill, put, k, v);
        }
    }

    // §8f-2 drain for one DISTINCT dedup table (its own state table in the
    // reference, one per distinct column: pk = group key ∥ datum, value =
    // full row ++ one i64 count per call distincting on the column,
    // distinct.rs:89-93,158-185; DELETE when the count drops to 0, nothing
    // when a row created this epoch also dies in it — mem-table netting,
    // as the join/topn drains). Records sorted by memcomparable pk: the
    // reference iterates a HashMap (nondeterministic), so sorted order is
    // the canonical form both this and the oracle emit.
    int dedup_drain(int di, std::vector<uint8_t>& out) {
        if (di < 0 || (size_t)di >= distinct_slots.size())
            FAIL(RW_E_INVAL, "dedup table index %d (have %zu)", di,
                 distinct_slots.size());
        if ((size_t)di >= dedup_slots.size()) return RW_OK; // nothing pushed
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t n = 0;
        HIP_TRY(hipMemcpy(&n, ddirty_n[di], 4, hipMemcpyDeviceToHost));
        if (!n) return RW_OK;
        std::vector<uint32_t> slots_h(n);
        HIP_TRY(hipMemcpy(slots_h.data(), ddirty_list[di], (size_t)n * 4,
                          hipMemcpyDeviceToHost));
        DevOwner tmp;
        DedupDirtyRec* d_out = nullptr;
        HIP_TRY(tmp.alloc(&d_out, (size_t)n * sizeof(DedupDirtyRec)));
        dedup_gather_kernel<<<grid_for(n), 256, 0, stream>>>(
            dedup_slots[di], ddirty_flag[di], ddirty_list[di], ddirty_n[di],
            d_out);
        std::vector<DedupDirtyRec> recs(n);
        int rc_cp = hipMemcpy(recs.data(), d_out,
                              (size_t)n * sizeof(DedupDirtyRec),
                              hipMemcpyDeviceToHost);
        tmp.release(&d_out);
        if (rc_cp != hipSuccess) FAIL(RW_E_INTERNAL, "dedup gather copy");
        HIP_TRY(hipMemset(ddirty_n[di], 0, 4));
        std::vector<uint8_t> key_types(out_types.begin(),
                                       out_types.begin() + KW);
        key_types.push_back(distinct_col_types[di]);
        auto& persisted = dedup_persisted[di];
        std::vector<rwcodec::FrameRec> rs;
        rs.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            const DedupDirtyRec& r = recs[i];
            uint32_t slot = slots_h[i];
            rwcodec::FrameRec e;
            // signed view: a retract of a never-inserted datum wraps the u32
            // below 0 — match the oracle's signed-count semantics (the
            // reference's count is i64; inconsistent input tolerance)
            if ((int32_t)r.count > 0) {
                e.put = 1;
                persisted[slot] = 1;
            } else {
                if (!persisted[slot]) continue; // created+died this epoch
                e.put = 0;
                persisted[slot] = 0;
            }
            for (int c = 0; c <= KW; c++) {
                rwcodec::DatumC d = rwcodec::datum_of_word(
                    key_types[c], ((r.nulls >> c) & 1) != 0, r.key[c]);
                rwcodec::memcmp_encode_datum(e.k, key_types[c], d, {});
            }
            if (e.put) {
                for (int c = 0; c <= KW; c++) {
                    rwcodec::DatumC d = rwcodec::datum_of_word(
                        key_types[c], ((r.nulls >> c) & 1) != 0, r.key[c]);
                    rwcodec::value_encode_datum(e.v, key_types[c], d);
                }
                for (int ci = 0; ci < n_calls; ci++)
                    if (call_dedup_idx[ci] == di)
                        rwcodec::value_encode_datum(
                            e.v, RW_T_I64, {false, (long long)r.count, 0});
            }
            rs.push_back(std::move(e));
        }
        // keys are distinct here: one slot is one (group, datum)
        rwcodec::write_sorted(out, rs);
        return RW_OK;
    }

    // §8f-5 recovery for one DISTINCT dedup table: replay concatenated
    // dedup_drain streams (PUT last-write-wins / DELETE removes), decode
    // the surviving (group ∥ datum, count) records and seed the counter
    // slots; restored slots are marked persisted so a later 1→0 drop
    // drains as DELETE exactly as in an uninterrupted run.
    int dedup_restore(int di, const uint8_t* buf, uint64_t len) {
        if (di < 0 || (size_t)di >= distinct_slots.size())
            FAIL(RW_E_INVAL, "dedup table index %d (have %zu)", di,
                 distinct_slots.size());
        int rc = ensure_dedup(1);
        if (rc != RW_OK) return rc;
        rwcodec::FrameMap merged;
        if (!rwcodec::merge_frames(buf, len, merged))
            FAIL(RW_E_INVAL, "malformed spill stream");
        uint32_t n = (uint32_t)merged.size();
        if (!n) return RW_OK;
        int KW1 = KW + 1;
        std::vector<uint8_t> key_types(out_types.begin(),
                                       out_types.begin() + KW);
        key_types.push_back(distinct_col_types[di]);
        std::vector<long long> keys((size_t)n * KW1);
        std::vector<uint32_t> nulls(n, 0), counts(n);
        uint32_t i = 0;
        for (auto& [kbytes, val] : merged) {
            (void)kbytes;
            rwcodec::RowReader rd{val.data(), val.size()};
            rwcodec::DatumC d;
            for (int c = 0; c < KW1; c++) {
                if (!rd.datum(key_types[c], &d))
                    FAIL(RW_E_INVAL, "dedup restore: bad key datum");
                keys[(size_t)i * KW1 + c] =
                    d.null ? 0 : rwcodec::word_of_datum(key_types[c], d);
                nulls[i] |= (uint32_t)(d.null != 0) << c;
            }
            if (!rd.datum(RW_T_I64, &d) || d.null)
                FAIL(RW_E_INVAL, "dedup restore: bad count datum");
            counts[i] = (uint32_t)d.i;
            i++;
        }
        long long* dkeys = nullptr;
        uint32_t *dnulls = nullptr, *dcounts = nullptr, *dslots_out = nullptr,
                 *derr = nullptr;
        DevOwner tmp;
        HIP_TRY(tmp.upload(&dkeys, keys));
        HIP_TRY(tmp.upload(&dnulls, nulls));
        HIP_TRY(tmp.upload(&dcounts, counts));
        HIP_TRY(tmp.alloc(&dslots_out, (size_t)n * 4));
        HIP_TRY(tmp.alloc(&derr, 4));
        HIP_TRY(hipMemset(derr, 0, 4));
        dedup_restore_kernel<<<grid_for(n), 256, 0, stream>>>(
            dkeys, dnulls, dcounts, n, KW1, dedup_slots[di], dedup_cap_mask,
            dslots_out, derr);
        std::vector<uint32_t> slots_h(n);
        uint32_t errv = 0;
        int rc_s = hipStreamSynchronize(stream) == hipSuccess ? RW_OK
                                                              : RW_E_INTERNAL;
        if (rc_s == RW_OK) {
            hipMemcpy(slots_h.data(), dslots_out, (size_t)n * 4,
                      hipMemcpyDeviceToHost);
            hipMemcpy(&errv, derr, 4, hipMemcpyDeviceToHost);
        }
        tmp.release_all();
        if (rc_s != RW_OK) FAIL(RW_E_INTERNAL, "dedup restore sync failed");
        if (errv) FAIL(RW_E_INTERNAL, "dedup restore overflow (code %u)", errv);
        auto& persisted = dedup_persisted[di];
        for (uint32_t r = 0; r < n; r++) persisted[slots_h[r]] = 1;
        return RW_OK;
    }

    // ----- §8f-2 round 2: materialized-input state-TABLE spill. One
    // table per retractable min/max call (AggStateStorage::
    // MaterializedInput, test_utils/agg_executor.rs:63-121): pk =
    // [group ASC ∥ value ASC(min)/DESC(max) ∥ stream key ASC], NULLs
    // largest; value = the full row. Per-epoch deltas with mem-table
    // netting: fresh alive rows → PUT, pre-drain rows killed this epoch →
    // DELETE, created+died nets away. The drain copies the row arrays up
    // to the cursor (host-marshal path; cost noted). -----
    std::vector<uint32_t> mflush_mark, mkill_mark;

    int minput_drain(int mi, std::vector<uint8_t>& out) {
        if (mi < 0 || mi >= n_minput) FAIL(RW_E_INVAL, "minput table %d", mi);
        HIP_TRY(hipStreamSynchronize(stream));
        if ((int)mflush_mark.size() < n_minput) {
            mflush_mark.assign(n_minput, 0);
            mkill_mark.assign(n_minput, 0);
        }
        uint32_t cur = 0, kcur = 0;
        HIP_TRY(hipMemcpy(&cur, t.mcursor, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&kcur, t.mkilled_cursor, 4, hipMemcpyDeviceToHost));
        if (kcur > t.mkilled_cap)
            FAIL(RW_E_INTERNAL, "minput kill list overflow (lost deltas)");
        if (cur > t.mrow_cap) cur = t.mrow_cap;
        size_t cap = (size_t)t.cap_mask + 1;
        std::vector<long long> mval(cur);
        std::vector<uint8_t> mnull(cur), mc(cur), alive4(cur * 4);
        std::vector<uint32_t> mslot_h(cur), alive(cur);
        std::vector<long long> sk((size_t)t.n_sk * cur);
        std::vector<uint8_t> skn((size_t)t.n_sk * cur);
        if (cur) {
            HIP_TRY(hipMemcpy(mval.data(), t.mval, (size_t)cur * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mnull.data(), t.mval_null, cur,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mc.data(), t.mcall, cur, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mslot_h.data(), t.mslot, (size_t)cur * 4,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(alive.data(), t.malive, (size_t)cur * 4,
                              hipMemcpyDeviceToHost));
            for (int k = 0; k < t.n_sk; k++) {
                HIP_TRY(hipMemcpy(sk.data() + (size_t)k * cur,
                                  t.msk + (size_t)k * t.mrow_cap,
                                  (size_t)cur * 8, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(skn.data() + (size_t)k * cur,
                                  t.msk_null + (size_t)k * t.mrow_cap, cur,
                                  hipMemcpyDeviceToHost));
            }
        }
        std::vector<uint32_t> kills(kcur);
        if (kcur)
            HIP_TRY(hipMemcpy(kills.data(), t.mkilled, (size_t)kcur * 4,
                              hipMemcpyDeviceToHost));
        std::vector<int64_t> gkeys(cap * KW);
        std::vector<uint32_t> gnulls(cap);
        HIP_TRY(hipMemcpy(gkeys.data(), t.keys, cap * KW * 8,
                          hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(gnulls.data(), t.key_nulls, cap * 4,
                          hipMemcpyDeviceToHost));
        // ordinal -> (call index)
        int ci = -1, o = -1;
        for (size_t j = 0; j < calls.size(); j++) {
            if (call_minput[j]) o++;
            if (o == mi) {
                ci = (int)j;
                break;
            }
        }
        auto encode = [&](uint32_t row, std::vector<uint8_t>& kb,
                          std::vector<uint8_t>* v) {
            uint32_t slot = mslot_h[row];
            for (int i2 = 0; i2 < KW; i2++) {
                rwcodec::DatumC d{((gnulls[slot] >> i2) & 1) != 0,
                                  gkeys[(size_t)slot * KW + i2], 0};
                rwcodec::memcmp_encode_datum(kb, out_types[i2], d, {});
            }
            rwcodec::DatumC dv = rwcodec::datum_of_word(
                input_types[calls[ci].arg], mnull[row] != 0, mval[row]);
            rwcodec::memcmp_encode_datum(
                kb, input_types[calls[ci].arg], dv,
                {calls[ci].kind == RW_AGG_MAX, true});
            for (int k2 = 0; k2 < t.n_sk; k2++) {
                rwcodec::DatumC d{skn[(size_t)k2 * cur + row] != 0,
                                  sk[(size_t)k2 * cur + row], 0};
                rwcodec::memcmp_encode_datum(
                    kb, input_types[stream_key[k2]], d, {});
            }
            if (v) {
                for (int i2 = 0; i2 < KW; i2++) {
                    rwcodec::DatumC d{((gnulls[slot] >> i2) & 1) != 0,
                                      gkeys[(size_t)slot * KW + i2], 0};
                    rwcodec::value_encode_datum(*v, out_types[i2], d);
                }
                rwcodec::DatumC dv2 = rwcodec::datum_of_word(
                    input_types[calls[ci].arg], mnull[row] != 0, mval[row]);
                rwcodec::value_encode_datum(*v, input_types[calls[ci].arg],
                                            dv2);
                for (int k2 = 0; k2 < t.n_sk; k2++) {
                    rwcodec::DatumC d{skn[(size_t)k2 * cur + row] != 0,
                                      sk[(size_t)k2 * cur + row], 0};
                    rwcodec::value_encode_datum(
                        *v, input_types[stream_key[k2]], d);
                }
            }
        };
        std::vector<rwcodec::FrameRec> rs;
        for (uint32_t row = mflush_mark[mi]; row < cur; row++) {
            if (mc[row] != (uint8_t)mi || !alive[row]) continue;
            rwcodec::FrameRec e{1, {}, {}};
            encode(row, e.k, &e.v);
            rs.push_back(std::move(e));
        }
        for (uint32_t i2 = mkill_mark[mi]; i2 < kcur; i2++) {
            uint32_t row = kills[i2];
            if (row >= cur || mc[row] != (uint8_t)mi) continue;
            if (row >= mflush_mark[mi]) continue; // created+died this epoch
            rwcodec::FrameRec e{0, {}, {}};
            encode(row, e.k, nullptr);
            rs.push_back(std::move(e));
        }
        // a PUT and a DELETE can share a key here: the stable order keeps
        // the PUT first
        rwcodec::write_sorted(out, rs);
        mflush_mark[mi] = cur;
        mkill_mark[mi] = kcur;
        return RW_OK;
    }

    // §8f-4 memory reclamation for the materialized-input row store:
    // retractions retire rows in place (malive=0) and the store would
    // otherwise grow without bound. Host-marshalled pack (maintenance
    // cadence, same copy costs as a drain): alive rows compact down,
    // chains rebuild host-side, heads re-upload. Requires drained minput
    // tables (flush marks at the cursor, kill list consumed).
    int minput_compact(uint64_t* reclaimed) {
        if (!n_minput) {
            if (reclaimed) *reclaimed = 0;
            return RW_OK;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t cur = 0, kcur = 0;
        HIP_TRY(hipMemcpy(&cur, t.mcursor, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&kcur, t.mkilled_cursor, 4,
                          hipMemcpyDeviceToHost));
        if ((int)mflush_mark.size() < n_minput) {
            mflush_mark.assign(n_minput, 0);
            mkill_mark.assign(n_minput, 0);
        }
        for (int mi = 0; mi < n_minput; mi++)
            if (mflush_mark[mi] != cur || mkill_mark[mi] != kcur)
                FAIL(RW_E_INVAL, "minput compact requires drained tables "
                                 "(table %d has undrained deltas)", mi);
        if (cur > t.mrow_cap) cur = t.mrow_cap;
        size_t cap = (size_t)t.cap_mask + 1;
        std::vector<long long> mval(cur), sk((size_t)t.n_sk * cur);
        std::vector<uint8_t> mnull(cur), skn((size_t)t.n_sk * cur),
            mc(cur);
        std::vector<uint32_t> mslot_h(cur), alive(cur);
        if (cur) {
            HIP_TRY(hipMemcpy(mval.data(), t.mval, (size_t)cur * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mnull.data(), t.mval_null, cur,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mc.data(), t.mcall, cur,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(mslot_h.data(), t.mslot, (size_t)cur * 4,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(alive.data(), t.malive, (size_t)cur * 4,
                              hipMemcpyDeviceToHost));
            for (int k = 0; k < t.n_sk; k++) {
                HIP_TRY(hipMemcpy(sk.data() + (size_t)k * cur,
                                  t.msk + (size_t)k * t.mrow_cap,
                                  (size_t)cur * 8, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(skn.data() + (size_t)k * cur,
                                  t.msk_null + (size_t)k * t.mrow_cap,
                                  (size_t)cur, hipMemcpyDeviceToHost));
            }
        }
        uint32_t n_alive = 0;
        std::vector<uint32_t> mnext_h;
        std::vector<uint32_t> heads((size_t)n_minput * cap, UINT32_MAX);
        for (uint32_t r = 0; r < cur; r++) {
            if (!alive[r]) continue;
            uint32_t nr = n_alive++;
            mval[nr] = mval[r];
            mnull[nr] = mnull[r];
            mc[nr] = mc[r];
            mslot_h[nr] = mslot_h[r];
            for (int k = 0; k < t.n_sk; k++) {
                sk[(size_t)k * cur + nr] = sk[(size_t)k * cur + r];
                skn[(size_t)k * cur + nr] = skn[(size_t)k * cur + r];
            }
            size_t hi = (size_t)mc[nr] * cap + mslot_h[nr];
            mnext_h.push_back(heads[hi]);
            heads[hi] = nr;
        }
        if (n_alive) {
            HIP_TRY(hipMemcpy(t.mval, mval.data(), (size_t)n_alive * 8,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.mval_null, mnull.data(), n_alive,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.mcall, mc.data(), n_alive,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.mslot, mslot_h.data(), (size_t)n_alive * 4,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.mnext, mnext_h.data(), (size_t)n_alive * 4,
                              hipMemcpyHostToDevice));
            std::vector<uint32_t> ones(n_alive, 1);
            HIP_TRY(hipMemcpy(t.malive, ones.data(), (size_t)n_alive * 4,
                              hipMemcpyHostToDevice));
            for (int k = 0; k < t.n_sk; k++) {
                HIP_TRY(hipMemcpy(t.msk + (size_t)k * t.mrow_cap,
                                  sk.data() + (size_t)k * cur,
                                  (size_t)n_alive * 8,
                                  hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(t.msk_null + (size_t)k * t.mrow_cap,
                                  skn.data() + (size_t)k * cur,
                                  (size_t)n_alive, hipMemcpyHostToDevice));
            }
        }
        HIP_TRY(hipMemcpy(t.mheads, heads.data(), heads.size() * 4,
                          hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.mcursor, &n_alive, 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(t.mkilled_cursor, 0, 4));
        for (int mi = 0; mi < n_minput; mi++) {
            mflush_mark[mi] = n_alive;
            mkill_mark[mi] = 0;
        }
        if (reclaimed)
            *reclaimed = (uint64_t)(cur - n_alive) * (8 + 1 + 9 * t.n_sk);
        return RW_OK;
    }

    int minput_restore(int mi, const uint8_t* buf, uint64_t len) {
        if (mi < 0 || mi >= n_minput) FAIL(RW_E_INVAL, "minput table %d", mi);
        int ci = -1, o = -1;
        for (size_t j = 0; j < calls.size(); j++) {
            if (call_minput[j]) o++;
            if (o == mi) {
                ci = (int)j;
                break;
            }
        }
        rwcodec::FrameMap merged;
        if (!rwcodec::merge_frames(buf, len, merged))
            FAIL(RW_E_INVAL, "malformed minput spill stream");
        uint32_t n = (uint32_t)merged.size();
        if (!n) return RW_OK;
        std::vector<int64_t> gk((size_t)n * KW);
        std::vector<uint32_t> gn(n, 0);
        std::vector<long long> mv(n);
        std::vector<uint8_t> mn(n);
        std::vector<long long> sks((size_t)t.n_sk * n, 0);
        std::vector<uint8_t> skns((size_t)t.n_sk * n, 0);
        uint32_t i2 = 0;
        for (auto& [kb, val] : merged) {
            (void)kb;
            rwcodec::RowReader row{val.data(), val.size()};
            auto rd = [&](uint8_t ty, long long* vv, uint8_t* nn) -> bool {
                rwcodec::DatumC d;
                if (!row.datum(ty, &d)) return false;
                *vv = d.null ? 0 : rwcodec::word_of_datum(ty, d);
                *nn = d.null;
                return true;
            };
            long long vv;
            uint8_t nn;
            for (int k2 = 0; k2 < KW; k2++) {
                if (!rd(out_types[k2], &vv, &nn))
                    FAIL(RW_E_INVAL, "minput restore: bad group datum");
                gk[(size_t)i2 * KW + k2] = vv;
                gn[i2] |= (uint32_t)(nn != 0) << k2;
            }
            if (!rd(input_types[calls[ci].arg], &mv[i2], &mn[i2]))
                FAIL(RW_E_INVAL, "minput restore: bad value datum");
            for (int k2 = 0; k2 < t.n_sk; k2++) {
                if (!rd(input_types[stream_key[k2]], &vv, &nn))
                    FAIL(RW_E_INVAL, "minput restore: bad stream-key datum");
                sks[(size_t)k2 * n + i2] = vv;
                skns[(size_t)k2 * n + i2] = nn;
            }
            i2++;
        }
        int64_t* dgk = nullptr;
        uint32_t* dgn = nullptr;
        long long* dmv = nullptr;
        uint8_t* dmn = nullptr;
        long long* dsk = nullptr; // the two stay null without stream keys
        uint8_t* dskn = nullptr;
        DevOwner tmp;
        HIP_TRY(tmp.upload(&dgk, gk));
        HIP_TRY(tmp.upload(&dgn, gn));
        HIP_TRY(tmp.upload(&dmv, mv));
        HIP_TRY(tmp.upload(&dmn, mn));
        HIP_TRY(tmp.upload(&dsk, sks));
        HIP_TRY(tmp.upload(&dskn, skns));
        agg_minput_restore_kernel<<<grid_for(n), 256, 0, stream>>>(
            t, KW, mi, dgk, dgn, dmv, dmn, dsk, dskn, n);
        int rc2 = hipStreamSynchronize(stream) == hipSuccess ? RW_OK
                                                             : RW_E_INTERNAL;
        tmp.release_all();
        if (rc2 != RW_OK) FAIL(RW_E_INTERNAL, "minput restore sync failed");
        int rc3 = check_overflow();
        if (rc3 != RW_OK) return rc3;
        // restored rows predate the epoch
        if ((int)mflush_mark.size() < n_minput) {
            mflush_mark.assign(n_minput, 0);
            mkill_mark.assign(n_minput, 0);
        }
        uint32_t cur = 0;
        HIP_TRY(hipMemcpy(&cur, t.mcursor, 4, hipMemcpyDeviceToHost));
        for (int j = 0; j < n_minput; j++) mflush_mark[j] = cur;
        return RW_OK;
    }

    // §8f-5 recovery of the result table. minput-bearing executors:
    // minput_restore must run for every minput table BEFORE this call (prev
    // outputs are recomputed from the hydrated chains, mirroring
    // agg_group.rs:219-221)
    int restore(const uint8_t* buf, uint64_t len) {
        rwcodec::FrameMap merged;
        if (!rwcodec::merge_frames(buf, len, merged))
            FAIL(RW_E_INVAL, "malformed spill stream");
        uint32_t n = (uint32_t)merged.size();
        if (!n) return RW_OK;
        int nc = n_calls;
        std::vector<int64_t> keys((size_t)n * KW);
        std::vector<uint32_t> knulls(n, 0);
        std::vector<long long> vals((size_t)nc * n);
        std::vector<uint8_t> vnulls((size_t)nc * n);
        std::vector<long long> vals2;
        if (n_dec) vals2.assign((size_t)nc * n, 0);
        // varchar group keys: the decoded strings are packed into one host
        // buffer and take the same staging + intern path a pushed chunk does
        std::vector<uint8_t> sbytes;
        uint32_t i = 0;
        for (auto& [kbytes, val] : merged) {
            (void)kbytes;
            rwcodec::RowReader rd{val.data(), val.size()};
            for (int c = 0; c < KW + nc; c++) {
                uint8_t ty = out_types[c];
                if (c < KW && ((vc_mask >> c) & 1)) {
                    bool null = false;
                    const uint8_t* s = nullptr;
                    uint32_t slen = 0;
                    if (!rd.str(&null, &s, &slen) || slen > rwvarlen::MAX_LEN)
                        FAIL(RW_E_INVAL, "restore: bad varchar key datum");
                    keys[(size_t)i * KW + c] =
                        null ? 0
                             : (int64_t)rwvarlen::pack(
                                   rwvarlen::PROV_BIT | (uint64_t)sbytes.size(),
                                   slen);
                    knulls[i] |= (uint32_t)null << c;
                    if (!null) sbytes.insert(sbytes.end(), s, s + slen);
                    continue;
                }
                rwcodec::DatumC d;
                if (!rd.datum(ty, &d))
                    FAIL(RW_E_INVAL, "restore: bad state datum");
                if (c < KW) {
                    keys[(size_t)i * KW + c] = d.null ? 0 : d.i;
                    knulls[i] |= (uint32_t)(d.null != 0) << c;
                } else {
                    vals[(size_t)(c - KW) * n + i] =
                        rwcodec::word_of_datum(ty, d);
                    vnulls[(size_t)(c - KW) * n + i] = d.null;
                    if (n_dec) vals2[(size_t)(c - KW) * n + i] = d.i2;
                }
            }
            i++;
        }
        int64_t* dkeys = nullptr;
        uint32_t* dknulls = nullptr;
        long long* dvals = nullptr;
        uint8_t* dvnulls = nullptr;
        long long* dvals2 = nullptr; // stays null without decimal calls
        DevOwner tmp;
        HIP_TRY(tmp.upload(&dkeys, keys));
        HIP_TRY(tmp.upload(&dknulls, knulls));
        HIP_TRY(tmp.upload(&dvals, vals));
        HIP_TRY(tmp.upload(&dvnulls, vnulls));
        HIP_TRY(tmp.upload(&dvals2, vals2));
        if (has_vc()) {
            int rcv = intern_prepare((uint64_t)n * nv, sbytes.size());
            if (rcv == RW_OK && !sbytes.empty() &&
                hipMemcpy(in_stg, sbytes.data(), sbytes.size(),
                          hipMemcpyHostToDevice) != hipSuccess) {
                g_err = "restore: staging copy failed";
                rcv = RW_E_INTERNAL;
            }
            if (rcv == RW_OK) {
                InternCols ic{};
                for (int j = 0; j < nv; j++) ic.words[j] = dkeys + vpos[j];
                ic.vis = nullptr;
                ic.n_rows = n;
                ic.nv = (uint32_t)nv;
                ic.stride = (uint32_t)KW;
                rcv = intern_run(ic);
            }
            if (rcv != RW_OK) return rcv;
        }
        agg_restore_kernel<<<grid_for(n), 256, 0, stream>>>(
            t, KW, nc, dkeys, dknulls, dvals, dvnulls, dvals2, n,
            eowc ? 0 : 1, cd(0), cd(1), cd(2), cd(3));
        int rc = hipStreamSynchronize(stream) == hipSuccess ? RW_OK
                                                            : RW_E_INTERNAL;
        tmp.release_all();
        if (rc != RW_OK) FAIL(RW_E_INTERNAL, "restore sync failed");
        return check_overflow();
    }

    // ----- key-table compaction -----

    // READY slots and the live groups among them; drains the stream
    int state_counts(uint64_t* ready, uint64_t* live) {
        DevOwner tmp;
        unsigned long long* d = nullptr;
        HIP_TRY(tmp.alloc(&d, 16));
        HIP_TRY(hipMemsetAsync(d, 0, 16, stream));
        agg_compact_count_kernel<<<grid_for(capacity), 256, 0, stream>>>(
            t, (int)desc.row_count_index, d);
        unsigned long long h[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *ready = h[0];
        *live = h[1];
        return RW_OK;
    }

    // what a compaction must not run over: it would drop or reorder work
    // the caller has not finished
    int compact_refusals() {
        if (erows)
            FAIL(RW_E_INVAL, "agg compact: ingest-mode rows are staged but "
                             "not applied (flush first)");
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t nd = 0;
        HIP_TRY(hipMemcpy(&nd, t.counters, 4, hipMemcpyDeviceToHost));
        if (nd)
            FAIL(RW_E_INVAL, "agg compact: %u dirty groups are not flushed "
                             "(call between epochs, after the flush)", nd);
        if (n_minput) { // minput_compact's own check, before anything moves
            uint32_t cur = 0, kcur = 0;
            HIP_TRY(hipMemcpy(&cur, t.mcursor, 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&kcur, t.mkilled_cursor, 4,
                              hipMemcpyDeviceToHost));
            for (int mi = 0; mi < n_minput; mi++) {
                uint32_t fm = mi < (int)mflush_mark.size() ? mflush_mark[mi] : 0;
                uint32_t km = mi < (int)mkill_mark.size() ? mkill_mark[mi] : 0;
                if (fm != cur || km != kcur)
                    FAIL(RW_E_INVAL, "agg compact requires drained minput "
                                     "tables (table %d has undrained deltas)",
                         mi);
            }
        }
        return RW_OK;
    }

    // the table's per-slot arrays back to what init() leaves
    int compact_clear() {
        size_t cap = capacity;
        HIP_TRY(hipMemsetAsync(t.state, 0, cap * 4, stream));
        HIP_TRY(hipMemsetAsync(t.keys, 0, cap * KW * 8, stream));
        HIP_TRY(hipMemsetAsync(t.key_nulls, 0, cap * 4, stream));
        HIP_TRY(hipMemsetAsync(t.has, 0, cap * n_calls, stream));
        HIP_TRY(hipMemsetAsync(t.prev, 0, cap * n_calls * 8, stream));
        HIP_TRY(hipMemsetAsync(t.prev_null, 0, cap * n_calls, stream));
        HIP_TRY(hipMemsetAsync(t.has_prev, 0, cap, stream));
        HIP_TRY(hipMemsetAsync(t.dirty_flag, 0, cap * 4, stream));
        if (n_dec) {
            HIP_TRY(hipMemsetAsync(t.dsum, 0, (size_t)n_dec * 4 * cap * 8, stream));
            HIP_TRY(hipMemsetAsync(t.dscl, 0, (size_t)n_dec * cap * 4, stream));
            HIP_TRY(hipMemsetAsync(t.dspec, 0, (size_t)n_dec * 3 * cap * 8, stream));
            HIP_TRY(hipMemsetAsync(t.prev2, 0, (size_t)n_calls * cap * 8, stream));
        }
        if (n_minput)
            HIP_TRY(hipMemsetAsync(t.mheads, 0xFF, (size_t)n_minput * cap * 4,
                                   stream));
        // acc: the min / max identities
        agg_init_kernel<<<2048, 256, 0, stream>>>(t, n_calls, cd(0), cd(1),
                                                  cd(2), cd(3));
        return RW_OK;
    }

    // Strings of dead groups: re-intern the packed block's varchar words
    // into a fresh arena and table, reading the bytes from the old arena as
    // a push reads them from its staging buffer (§17.2's rule holds: every
    // byte hashed or compared was written before these launches).
    int compact_reintern(const AggPackDev& p) {
        uint64_t cells = (uint64_t)p.n * nv;
        if (in_row_cap < cells) {
            mem.release(&in.rowslot);
            mem.release(&in.winners);
            in_row_cap = 0;
            uint64_t cap = 4096;
            while (cap < cells) cap <<= 1;
            HIP_TRY(mem.alloc(&in.rowslot, cap * 4));
            HIP_TRY(mem.alloc(&in.winners, cap * 4));
            in_row_cap = (uint32_t)(cap > UINT32_MAX ? UINT32_MAX : cap);
        }
        uint8_t* old_arena = in.arena;
        uint64_t* old_slots = in.slots;
        uint8_t* arena = nullptr;
        uint64_t* slots = nullptr;
        size_t tbytes = ((size_t)in.cap_mask + 1) * 8;
        HIP_TRY(mem.alloc(&arena, in.arena_cap));
        if (mem.alloc(&slots, tbytes) != hipSuccess) {
            mem.release(&arena);
            FAIL(RW_E_INTERNAL, "agg compact: intern table allocation failed");
        }
        // from here on the executor owns the new pair; the old pair is
        // only read, as staging, until the stream drains
        in.arena = arena;
        in.slots = slots;
        in.stg = old_arena;
        unsigned long long t0 = rwvarlen::AGG_ARENA_HEADER;
        HIP_TRY(hipMemsetAsync(arena, 0, rwvarlen::AGG_ARENA_HEADER, stream));
        HIP_TRY(hipMemsetAsync(slots, 0, tbytes, stream));
        HIP_TRY(hipMemcpy(in.tail, &t0, 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(in.ctr, 0, 8, stream));
        agg_compact_prov_kernel<<<grid_for(p.n * (uint32_t)KW), 256, 0,
                                  stream>>>(p, KW, vc_mask);
        InternCols ic{};
        for (int j = 0; j < nv; j++) ic.words[j] = p.keys + vpos[j];
        ic.vis = nullptr;
        ic.n_rows = p.n;
        ic.nv = (uint32_t)nv;
        ic.stride = (uint32_t)KW;
        int rc = intern_run(ic);
        if (rc != RW_OK) return rc;
        HIP_TRY(hipStreamSynchronize(stream)); // the old pair is done with
        in.stg = in_stg;
        mem.release(&old_arena);
        mem.release(&old_slots);
        return intern_sync_counts(); // exact tail / entries, pending bounds 0
    }

    int compact(uint64_t* reclaimed) {
        if (reclaimed) *reclaimed = 0;
        int rc = compact_refusals();
        if (rc != RW_OK) return rc;
        uint64_t ready = 0, live = 0;
        rc = state_counts(&ready, &live);
        if (rc != RW_OK) return rc;
        if (live == ready) return RW_OK; // no dead group: nothing moves
        if (n_minput) { // only live rows remain, heads rebuilt by owner
            rc = minput_compact(nullptr);
            if (rc != RW_OK) return rc;
        }
        // transient memory: the live groups' records, not the capacity
        DevOwner tmp;
        AggPackDev p{};
        p.n = (uint32_t)live;
        p.n_minput = n_minput;
        size_t n = live ? live : 1, nc = n_calls;
        HIP_TRY(tmp.alloc(&p.keys, n * KW * 8));
        HIP_TRY(tmp.alloc(&p.key_nulls, n * 4));
        HIP_TRY(tmp.alloc(&p.acc, nc * n * 8));
        HIP_TRY(tmp.alloc(&p.has, nc * n));
        HIP_TRY(tmp.alloc(&p.prev, nc * n * 8));
        HIP_TRY(tmp.alloc(&p.prev_null, nc * n));
        HIP_TRY(tmp.alloc(&p.has_prev, n));
        HIP_TRY(tmp.alloc(&p.old_slot, n * 4));
        if (n_dec) {
            HIP_TRY(tmp.alloc(&p.prev2, nc * n * 8));
            HIP_TRY(tmp.alloc(&p.dsum, (size_t)n_dec * 4 * n * 8));
            HIP_TRY(tmp.alloc(&p.dscl, (size_t)n_dec * n * 4));
            HIP_TRY(tmp.alloc(&p.dspec, (size_t)n_dec * 3 * n * 8));
        }
        if (n_minput) {
            HIP_TRY(tmp.alloc(&p.mheads, (size_t)n_minput * n * 4));
            HIP_TRY(tmp.alloc(&p.new_slot, n * 4));
        }
        HIP_TRY(tmp.alloc(&p.cursor, 8));
        p.err = p.cursor + 1;
        HIP_TRY(hipMemsetAsync(p.cursor, 0, 8, stream));
        agg_compact_pack_kernel<<<grid_for(capacity), 256, 0, stream>>>(
            t, p, KW, n_calls, (int)desc.row_count_index);
        uint32_t ce[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(ce, p.cursor, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (ce[1] || ce[0] != p.n) // nothing has been changed yet
            FAIL(RW_E_INTERNAL, "agg compact: packed %u of %u live groups",
                 ce[0], p.n);
        rc = compact_clear();
        if (rc != RW_OK) return rc;
        if (has_vc() && in_ready) {
            rc = compact_reintern(p);
            if (rc != RW_OK) return rc;
        }
        if (p.n) {
            agg_compact_reinsert_kernel<<<grid_for(p.n), 256, 0, stream>>>(
                t, p, KW, n_calls);
            if (n_minput)
                agg_compact_mslot_kernel<<<grid_for(p.n * (uint32_t)n_minput),
                                           256, 0, stream>>>(t, p);
        }
        HIP_TRY(hipMemcpyAsync(ce, p.cursor, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (ce[1])
            FAIL(RW_E_INTERNAL, "agg compact: reinsert found the table full");
        rc = check_overflow(); // the intern pre-pass reports through counters[2]
        if (rc != RW_OK) return rc;
        if (reclaimed) *reclaimed = ready - live;
        return RW_OK;
    }

    // Cuts the row-major output block into chunks of chunk_size rows (0 =
    // 1024) under the U-pair rule and queues them.
    int slice_outputs(const std::vector<long long>& vals,
                      const std::vector<uint8_t>& nulls,
                      const std::vector<uint8_t>& ops, uint32_t n_out,
                      const std::vector<long long>& vals2 = {}) {
        uint32_t max_rows = desc.chunk_size ? desc.chunk_size : 1024;
        for (auto [start, n] : rwchunk::slice_ranges(n_out, max_rows, ops.data())) {
            rwchunk::Builder cb(n, (uint32_t)out_width);
            for (int ci = 0; ci < out_width; ci++) {
                size_t ix = (size_t)start * out_width + ci;
                auto valid = rwchunk::from_nulls(&nulls[ix], out_width);
                auto* v = (const int64_t*)&vals[ix];
                if (out_types[ci] == RW_T_DECIMAL && !vals2.empty())
                    cb.decimal(v, (const int64_t*)&vals2[ix], out_width, valid);
                else if (ci < KW && ((vc_mask >> ci) & 1)) {
                    // a varchar key column: the strings fetch_key_strings
                    // left in vk_offs / vk_bytes, in block row order
                    if (!cb.varchar(&vk_offs[ci][start], vk_bytes[ci].data(),
                                    nullptr, valid))
                        FAIL(RW_E_INTERNAL, "output chunk strings exceed 4 GiB; "
                                            "lower chunk_size");
                } else
                    cb.fixed(out_types[ci], v, out_width, valid);
            }
            cb.ops(&ops[start]);
            outq.push(cb.release());
        }
        return RW_OK;
    }

    RwChunk* poll() { return outq.poll(); }

    ~HashAgg() {
        for (auto ev : in_ev)
            if (ev) hipEventDestroy(ev);
        mem.release_all(); // device memory goes before the stream
        if (stream) hipStreamDestroy(stream);
    }
};

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

// Shared checked export for the drain functions: copies a host spill buffer
// into a malloc'd block the caller frees with rw_spill_free. Fails loudly on
// allocation failure instead of crashing in memcpy.
static int spill_export(const std::vector<uint8_t>& sp, uint8_t** buf,
                        uint64_t* len) {
    *len = sp.size();
    *buf = (uint8_t*)malloc(sp.size() ? sp.size() : 1);
    if (!*buf) FAIL(RW_E_INTERNAL, "spill export: host alloc of %zu bytes failed",
                    sp.size());
    memcpy(*buf, sp.data(), sp.size());
    return RW_OK;
}

extern "C" {

const char* rw_last_error(void) { return g_err.c_str(); }

void rw_chunk_free(RwChunk* ch) { rwchunk::free_chunk(ch); }

void* rw_hash_agg_create(const RwHashAggDesc* d) {
    auto* h = new HashAgg();
    if (h->init(d) != RW_OK) {
        delete h;
        return nullptr;
    }
    return h;
}
int rw_hash_agg_push_chunk(void* h, const RwChunk* c) {
    return ((HashAgg*)h)->push_chunk(c);
}
int rw_hash_agg_flush(void* h, uint64_t epoch) { return ((HashAgg*)h)->flush(epoch); }

// the epoch-staging, device-batch and device-hop entry points move 8-byte
// words with no arena behind them (rw_stream.h: varchar group keys)
#define AGG_NO_VARCHAR(agg, what)                                         \
    do {                                                                  \
        if ((agg)->has_vc())                                              \
            FAIL(RW_E_INVAL, what " is not supported on a HashAgg with "  \
                                  "varchar group keys");                  \
    } while (0)

int rw_hash_agg_varlen_reserve(void* h, uint64_t arena_bytes,
                               uint64_t n_strings) {
    auto* agg = (HashAgg*)h;
    if (!agg->has_vc())
        FAIL(RW_E_INVAL, "rw_hash_agg_varlen_reserve: no varchar group key");
    if (agg->in_ready)
        FAIL(RW_E_INVAL, "rw_hash_agg_varlen_reserve: call before the first "
                         "push or restore");
    if (arena_bytes > rwvarlen::AGG_ARENA_MAX || n_strings > (1ull << 30))
        FAIL(RW_E_INVAL, "rw_hash_agg_varlen_reserve: size out of range");
    agg->in_reserve_arena = arena_bytes;
    agg->in_reserve_strings = n_strings;
    return RW_OK;
}

int rw_hash_agg_varlen_stats(void* h, uint64_t* arena_used,
                             uint64_t* arena_cap, uint64_t* n_strings,
                             uint64_t* table_cap) {
    auto* agg = (HashAgg*)h;
    int rc = agg->intern_sync_counts(); // exact values; no-op when unused
    if (rc != RW_OK) return rc;
    bool on = agg->in_ready;
    if (arena_used) *arena_used = on ? agg->in_tail_known : 0;
    if (arena_cap) *arena_cap = on ? agg->in.arena_cap : 0;
    if (n_strings) *n_strings = on ? agg->in_n_known : 0;
    if (table_cap) *table_cap = on ? (uint64_t)agg->in.cap_mask + 1 : 0;
    return RW_OK;
}

int rw_hash_agg_varlen_intern_stats(void* h, double* kernel_ms,
                                    double* fetch_ms, uint64_t* launches) {
    auto* agg = (HashAgg*)h;
    if (kernel_ms)
        for (int k = 0; k < 3; k++) kernel_ms[k] = agg->in_ms[k];
    if (fetch_ms) *fetch_ms = agg->vf.vemit_ms;
    if (launches) *launches = agg->in_timed_launches;
    return RW_OK;
}

// epoch-batched ingest mode (rw_stream.h): push_chunk stages, flush applies
int rw_hash_agg_ingest_mode(void* h, int epoch_batched) {
    auto* agg = (HashAgg*)h;
    if (epoch_batched) AGG_NO_VARCHAR(agg, "epoch-batched ingest");
    if (epoch_batched && agg->n_dec)
        FAIL(RW_E_INVAL, "epoch-batched ingest + decimal not yet supported");
    if (epoch_batched && (agg->n_minput > 0 || !agg->distinct_slots.empty()))
        FAIL(RW_E_INVAL,
             "epoch-batched ingest needs order-free value states "
             "(no materialized-input or DISTINCT aggregates)");
    if (!epoch_batched && agg->erows)
        FAIL(RW_E_INVAL, "staged epoch pending; flush before disabling");
    agg->epoch_ingest = epoch_batched != 0;
    return RW_OK;
}
RwChunk* rw_hash_agg_poll(void* h) { return ((HashAgg*)h)->poll(); }
void rw_hash_agg_destroy(void* h) { delete (HashAgg*)h; }

// --- bench support: device-resident batches + kernel stats ---

void* rw_agg_bench_preload(void* h, const RwChunk* c) {
    auto* agg = (HashAgg*)h;
    if (agg->has_vc()) {
        g_err = "rw_agg_bench_preload is not supported on a HashAgg with "
                "varchar group keys";
        return nullptr;
    }
    auto b = std::make_unique<Owned<AggBatch>>();
    uint32_t n = c->n_rows;
    for (int i = 0; i < agg->n_batch_slots(); i++) {
        // 16 B/row so decimal slots (2 words/row) fit
        if (b->mem.alloc(&b->col_vals[i], (size_t)n * 16) != hipSuccess) return nullptr;
        if (b->mem.alloc(&b->col_valid[i], n) != hipSuccess) return nullptr;
    }
    if (b->mem.alloc(&b->ops, n) != hipSuccess) return nullptr;
    b->vis = nullptr;
    b->n_rows = n;
    AggBatch stage_save = agg->stage;
    uint32_t cap_save = agg->stage_cap;
    agg->stage = *b;
    agg->stage_cap = n;
    AggBatch out;
    int rc = agg->upload(c, &out, true);
    agg->stage = stage_save;
    agg->stage_cap = cap_save;
    if (rc != RW_OK) return nullptr;
    (AggBatch&)*b = out; // keep the computed fields (n_rows, dense, vis)
    hipStreamSynchronize(agg->stream);
    return static_cast<AggBatch*>(b.release());
}

int rw_agg_bench_apply(void* h, void* batch) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_agg_bench_apply");
    return agg->apply(*(AggBatch*)batch, true);
}

int rw_agg_flush_launch(void* h, uint64_t epoch); // defined below
int rw_agg_apply_flush_launch(void* h, void* batch, uint32_t r0, uint32_t r1,
                              uint64_t epoch); // defined below

// C-side step loop: the Python interpreter costs ~15-20 us per step at q7
// sizes (ctypes + loop bookkeeping), which exceeds the 16 us apply kernel
// and makes the host the bottleneck. One call runs `steps` applies with the
// periodic stream-ordered checkpoint flush; everything stays async.
int rw_agg_bench_run(void* h, void** batches, int n_batches, int steps,
                     int barrier_every, int step0) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_agg_bench_run");
    for (int i = 0; i < steps; i++) {
        int rc = agg->apply(*(AggBatch*)batches[(step0 + i) % n_batches], true);
        if (rc != RW_OK) return rc;
        if (barrier_every > 0 && (step0 + i + 1) % barrier_every == 0) {
            rc = rw_agg_flush_launch(h, (uint64_t)(step0 + i));
            if (rc != RW_OK) return rc;
        }
    }
    return RW_OK;
}

// Epoch-granular step loop over one contiguous preloaded region: the
// engine buffers an epoch's chunks and applies them as ONE launch before
// the checkpoint flush (order-free value states) — a
// barrier_every×1M-row launch pipelines HBM loads far better than
// barrier_every separate 1M-row launches. `giant` holds n_slots logical
// steps of rows_per_step rows each; step s reads slot s % n_slots.
// Requires barrier_every | n_slots so every epoch is a contiguous range.
int rw_agg_bench_run_epochs(void* h, void* giant, uint64_t rows_per_step,
                            int n_slots, int steps, int barrier_every,
                            int step0) {
    AGG_NO_VARCHAR((HashAgg*)h, "rw_agg_bench_run_epochs");
    if (barrier_every <= 0 || n_slots % barrier_every ||
        step0 % barrier_every)
        FAIL(RW_E_INVAL, "epoch run needs barrier_every | n_slots, aligned step0");
    for (int s = 0; s < steps; s += barrier_every) {
        int width = steps - s < barrier_every ? steps - s : barrier_every;
        uint32_t r0 = (uint32_t)(((step0 + s) % n_slots) * rows_per_step);
        uint32_t r1 = r0 + (uint32_t)(width * rows_per_step);
        int rc = rw_agg_apply_flush_launch(h, giant, r0, r1,
                                           (uint64_t)(step0 + s));
        if (rc != RW_OK) return rc;
    }
    return RW_OK;
}

int rw_agg_sync(void* h) {
    auto* agg = (HashAgg*)h;
    if (hipStreamSynchronize(agg->stream) != hipSuccess)
        FAIL(RW_E_INTERNAL, "sync failed");
    return agg->check_overflow();
}

typedef struct {
    uint64_t launches;
    double total_ms;
    uint64_t rows;
} RwKernelStats;

int rw_agg_n_batch_slots(void* h) { return ((HashAgg*)h)->n_batch_slots(); }

// expose a preloaded batch's device pointers (for the exchange path)
int rw_agg_batch_ptrs(void* batch, const int64_t** vals, const uint8_t** valids,
                      const uint8_t** ops, uint32_t* n_rows) {
    auto* b = (AggBatch*)batch;
    for (int i = 0; i < MAX_KW + MAX_CALLS; i++) {
        vals[i] = b->col_vals[i];
        valids[i] = b->col_valid[i];
    }
    *ops = b->ops;
    *n_rows = b->n_rows;
    return RW_OK;
}

// apply an exchange payload (device-resident; per-block layout
// vals[col][npad]*8 ∥ valid[col][n] ∥ ops[n] with npad = n rounded up to 4
// so every column base is 32-B aligned; cols in the executor's batch slot
// order: group key cols then call args) — one apply launch per block.
// `dense` asserts every payload row is a visible non-NULL Insert (the
// SENDER knows: its source batches carried the dense flag) and routes the
// receiver through the vectorized dense kernel.
int rw_agg_apply_payload(void* h, const uint8_t* payload,
                         const uint64_t* block_rows, int n_blocks, int n_cols,
                         int dense) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_agg_apply_payload");
    if (agg->n_dec)
        FAIL(RW_E_INVAL, "decimal columns not yet carried by the exchange");
    if (n_cols != agg->KW + agg->n_calls)
        FAIL(RW_E_INVAL, "payload n_cols %d != %d", n_cols, agg->KW + agg->n_calls);
    uint64_t off = 0;
    for (int bi = 0; bi < n_blocks; bi++) {
        uint64_t n = block_rows[bi];
        if (!n) continue;
        uint64_t npad = (n + 3) & ~3ull;
        AggBatch b{};
        for (int c = 0; c < n_cols; c++) {
            b.col_vals[c] = (int64_t*)(payload + off + (uint64_t)c * npad * 8);
            b.col_valid[c] =
                (uint8_t*)(payload + off + (uint64_t)n_cols * npad * 8 +
                           (uint64_t)c * n);
        }
        b.ops = (uint8_t*)(payload + off + (uint64_t)n_cols * npad * 8 +
                           (uint64_t)n_cols * n);
        b.vis = nullptr;
        b.n_rows = (uint32_t)n;
        b.dense = dense ? 1 : 0;
        int rc = agg->apply(b, true);
        if (rc != RW_OK) return rc;
        off += ((uint64_t)n_cols * npad * 8 + (uint64_t)n_cols * n + n + 31) &
               ~31ull;
    }
    return RW_OK;
}

// bench sink: run the flush (change inference + prev update) but leave the
// emitted records in HBM for the device-resident downstream — returns the
// emitted row count, resets the cursor. The host-marshalling path
// (rw_hash_agg_flush + poll) remains the parity-test surface.
long long rw_agg_flush_device(void* h, uint64_t epoch) {
    auto* agg = (HashAgg*)h;
    (void)epoch;
    uint32_t n_dirty = 0;
    if (agg->presize_flush_out(&n_dirty) != RW_OK) return -1;
    agg->launch_flush(n_dirty, false);
    if (hipStreamSynchronize(agg->stream) != hipSuccess) return -1;
    uint32_t ctr[3];
    if (hipMemcpy(ctr, agg->t.counters, 12, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (ctr[2] != 0) {
        g_err = "agg overflow (code " + std::to_string(ctr[2]) + ")";
        return -(long long)ctr[2] - 1;
    }
    long long n = ctr[1];
    if (hipMemset(agg->t.counters, 0, 12) != hipSuccess) return -1;
    return n;
}

__global__ void agg_counters_reset_kernel(uint32_t* counters) {
    counters[0] = 0; // dirty count
    counters[1] = 0; // out cursor
}

// fully async flush: change inference and the counter reset run
// stream-ordered with no host round-trip (one launch for value-state
// executors, whose flush kernel resets the counters itself; see
// HashAgg::launch_flush); the overflow flag (counters[2]) is left set and
// surfaces at the next rw_agg_sync. The emitted rows are device-resident
// for the downstream, as with rw_agg_flush_device.
int rw_agg_flush_launch(void* h, uint64_t epoch) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_agg_flush_launch");
    (void)epoch;
    agg->launch_flush(-1, true);
    return RW_OK;
}

// one epoch, fully async: apply rows [r0, r1) of a preloaded batch and run
// the checkpoint flush behind it. Leaves the executor as apply_range +
// rw_agg_flush_launch leave it; where HashAgg::fuse_allowed and the launch
// shape permit, the flush runs in the apply launch's last-arriving block
// instead of a launch of its own (only with RW_AGG_FUSE_FLUSH=1: measured
// slower than two launches on the MI355X).
int rw_agg_apply_flush_launch(void* h, void* batch, uint32_t r0, uint32_t r1,
                              uint64_t epoch) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_agg_apply_flush_launch");
    auto* b = (AggBatch*)batch;
    if (r0 > r1 || r1 > b->n_rows)
        FAIL(RW_E_INVAL, "apply range [%u, %u) outside the batch's %u rows", r0,
             r1, b->n_rows);
    bool fused = false;
    int rc = agg->apply_range(*b, r0, r1, true, agg->fuse_allowed(), &fused);
    if (rc != RW_OK) return rc;
    return fused ? RW_OK : rw_agg_flush_launch(h, epoch);
}

int rw_agg_kernel_stats(void* h, RwKernelStats* out) {
    auto* agg = (HashAgg*)h;
    if (!agg->ring.harvest_all())
        FAIL(RW_E_INTERNAL, "event harvest failed");
    out->launches = agg->apply_launches;
    out->total_ms = agg->ring.ms_total;
    out->rows = agg->apply_rows;
    return RW_OK;
}

// debug: scan the device table for duplicate READY keys and report counts
typedef struct {
    uint64_t ready_slots;
    uint64_t dup_keys;
    uint64_t dirty_count;
    uint64_t out_cursor;
} RwAggDebug;

// debug: fix the dense span kernel's tiles-per-wave for this executor (0 =
// the launch policy, HashAgg::span_tiles_for) — lets tests reach multi-tile
// spans at small row counts
int rw_agg_debug_set_span_tiles(void* h, uint32_t n) {
    ((HashAgg*)h)->span_tiles_override = n;
    return RW_OK;
}

// debug: the fused checkpoint flush of rw_agg_apply_flush_launch: 0 = the
// dirty-count policy (HashAgg::fuse_allowed), 1 = always where the launch is
// eligible, 2 = never
int rw_agg_debug_set_fuse(void* h, int mode) {
    if (mode < 0 || mode > 2) FAIL(RW_E_INVAL, "fuse mode %d (0..2)", mode);
    ((HashAgg*)h)->fuse_mode = mode;
    return RW_OK;
}

// debug: would an eligible launch fuse right now; how many launches have
// carried the flush so far; the policy's dirty-count limit
int rw_agg_debug_fuse_allowed(void* h) {
    return ((HashAgg*)h)->fuse_allowed() ? 1 : 0;
}
long long rw_agg_debug_fused_launches(void* h) {
    return (long long)((HashAgg*)h)->fused_launches;
}
uint32_t rw_agg_debug_fuse_max(void) { return HashAgg::FUSE_MAX; }

// debug: the key hash every state table places by (table_find_or_insert,
// jslot_start, jbloom_bit), so tests can aim keys at chosen slots
uint64_t rw_debug_dev_bytes_live(void) { return g_dev_bytes_live.load(); }

uint64_t rw_debug_hash_key(const int64_t* kw, uint32_t nullmask, int n_words) {
    return hash_key(kw, nullmask, n_words);
}

int rw_agg_debug_scan(void* h, RwAggDebug* out) {
    auto* agg = (HashAgg*)h;
    size_t cap = (size_t)agg->t.cap_mask + 1;
    std::vector<uint32_t> state(cap);
    std::vector<int64_t> keys(cap * agg->KW);
    std::vector<uint32_t> knulls(cap);
    uint32_t ctr[3];
    hipDeviceSynchronize();
    HIP_TRY(hipMemcpy(state.data(), agg->t.state, cap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys.data(), agg->t.keys, cap * agg->KW * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(knulls.data(), agg->t.key_nulls, cap * 4,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ctr, agg->t.counters, 12, hipMemcpyDeviceToHost));
    std::unordered_multiset<std::string> seen;
    uint64_t ready = 0, dups = 0;
    for (size_t sl = 0; sl < cap; sl++) {
        if (state[sl] != SLOT_READY) continue;
        ready++;
        std::string k((const char*)&keys[sl * agg->KW], agg->KW * 8);
        k.append((const char*)&knulls[sl], 4);
        if (seen.count(k)) dups++;
        seen.insert(k);
    }
    out->ready_slots = ready;
    out->dup_keys = dups;
    out->dirty_count = ctr[0];
    out->out_cursor = ctr[1];
    return RW_OK;
}

int rw_agg_checkpoint_drain(void* h, uint8_t** buf, uint64_t* len) {
    auto* agg = (HashAgg*)h;
    // memcmp-key order, as the join/topn/dedup drains (rw_stream.h's ordering
    // guarantee): the flush kernel's atomic-cursor emission order is
    // nondeterministic, so the canonical sorted form is what both this and
    // the oracle emit — enabling byte-compare parity.
    rwcodec::sort_spill_frames(agg->spill);
    int rc = spill_export(agg->spill, buf, len);
    if (rc != RW_OK) return rc;
    agg->spill.clear();
    return RW_OK;
}

int rw_hash_agg_restore(void* h, const uint8_t* buf, uint64_t len) {
    return ((HashAgg*)h)->restore(buf, len);
}

int rw_agg_n_minput_tables(void* h) { return ((HashAgg*)h)->n_minput; }
int rw_agg_minput_drain(void* h, int mi, uint8_t** buf, uint64_t* len) {
    auto* agg = (HashAgg*)h;
    std::vector<uint8_t> sp;
    int rc = agg->minput_drain(mi, sp);
    if (rc != RW_OK) return rc;
    return spill_export(sp, buf, len);
}
int rw_agg_minput_restore(void* h, int mi, const uint8_t* buf, uint64_t len) {
    return ((HashAgg*)h)->minput_restore(mi, buf, len);
}

int rw_agg_minput_compact(void* h, uint64_t* reclaimed) {
    return ((HashAgg*)h)->minput_compact(reclaimed);
}

int rw_hash_agg_compact(void* h, uint64_t* reclaimed) {
    return ((HashAgg*)h)->compact(reclaimed);
}

int rw_hash_agg_state_stats(void* h, uint64_t* slots_ready,
                            uint64_t* groups_live, uint64_t* capacity) {
    auto* agg = (HashAgg*)h;
    uint64_t ready = 0, live = 0;
    int rc = agg->state_counts(&ready, &live);
    if (rc != RW_OK) return rc;
    if (slots_ready) *slots_ready = ready;
    if (groups_live) *groups_live = live;
    if (capacity) *capacity = agg->capacity;
    return RW_OK;
}

int rw_agg_n_dedup_tables(void* h) {
    return (int)((HashAgg*)h)->distinct_slots.size();
}

int rw_agg_dedup_drain(void* h, int di, uint8_t** buf, uint64_t* len) {
    auto* agg = (HashAgg*)h;
    std::vector<uint8_t> sp;
    int rc = agg->dedup_drain(di, sp);
    if (rc != RW_OK) return rc;
    return spill_export(sp, buf, len);
}

int rw_agg_dedup_restore(void* h, int di, const uint8_t* buf, uint64_t len) {
    return ((HashAgg*)h)->dedup_restore(di, buf, len);
}

void rw_spill_free(uint8_t* buf) { free(buf); }

int rw_agg_stats_reset(void* h) {
    auto* agg = (HashAgg*)h;
    agg->ring.harvest_all();
    agg->apply_launches = 0;
    agg->ring.ms_total = 0;
    agg->apply_rows = 0;
    agg->ev_seq = 0;
    return RW_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------
// Vnode hashing (VirtualNode::compute_chunk, consistent_hash/vnode.rs:146-181)
// ---------------------------------------------------------------------------
// vnode = IEEE CRC-32 (crc32fast) of the row's dist-key datums fed exactly
// as hash_datum does (native-endian primitive bytes; NULL = u32 0xfffffff0,
// array/mod.rs:99) mod vnode_count. Oracle counterpart:
// oracle/oracle_dispatch.cpp; pinned against zlib.crc32 in tests.
// A non-NULL varchar datum feeds its bytes followed by one 0xFF byte:
// hash_datum on a &str is `impl Hash for str`, i.e. Hasher::write_str, whose
// default is write(bytes) then write_u8(0xff), and crc32fast::Hasher
// implements only write. So "" feeds the single byte 0xFF and differs from
// NULL (vnode_varlen_kernel below, include/rw_xpayload.hpp).

__device__ uint32_t g_crc_table[256];
static bool g_crc_table_init = false;

static int ensure_crc_table() {
    if (g_crc_table_init) return RW_OK;
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        tab[i] = c;
    }
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_crc_table), tab, sizeof tab) !=
        hipSuccess)
        return RW_E_INTERNAL;
    g_crc_table_init = true;
    return RW_OK;
}

// LDS-staged CRC: divergent indexing of __constant__ memory serializes
// (each distinct address replays); LDS banks handle it at full rate
__device__ __forceinline__ uint32_t crc32_bytes(const uint32_t* lut, uint32_t crc,
                                               const uint8_t* p, int n) {
    for (int i = 0; i < n; i++)
        crc = lut[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return crc;
}

__device__ __forceinline__ void stage_crc_lut(uint32_t* lut) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = g_crc_table[i];
    __syncthreads();
}

struct VnodeBatch {
    int64_t* col_vals[MAX_KW];
    uint8_t* col_valid[MAX_KW];
    uint8_t* col_types[1]; // unused placeholder alignment
    uint32_t n_rows;
};

__global__ void vnode_kernel(VnodeBatch b, int n_keys, uint32_t vnode_count,
                             uint16_t* out, uint8_t t0, uint8_t t1, uint8_t t2,
                             uint8_t t3) {
    __shared__ uint32_t lut[256];
    stage_crc_lut(lut);
    uint8_t types[4] = {t0, t1, t2, t3};
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < b.n_rows;
         r += stride) {
        uint32_t crc = 0xFFFFFFFFu;
        for (int k = 0; k < n_keys; k++) {
            if (!b.col_valid[k][r]) {
                uint32_t sentinel = 0xfffffff0u;
                crc = crc32_bytes(lut, crc, (const uint8_t*)&sentinel, 4);
            } else {
                int64_t v = b.col_vals[k][r];
                int nbytes = (types[k] == RW_T_I32) ? 4 : 8;
                if (types[k] == RW_T_I32) {
                    int32_t v32 = (int32_t)v;
                    crc = crc32_bytes(lut, crc, (const uint8_t*)&v32, 4);
                } else {
                    crc = crc32_bytes(lut, crc, (const uint8_t*)&v, 8);
                }
                (void)nbytes;
            }
        }
        out[r] = (uint16_t)((uint64_t)(crc ^ 0xFFFFFFFFu) % vnode_count);
    }
}

// Batches with a varchar dist key take this kernel; vnode_kernel above stays
// what rw_join_vnode_hop and every fixed-width call launch. The feed of a
// varchar datum: its bytes, then one 0xFF; NULL is the same
// 4-byte sentinel as for every type. Slicing-by-8 tables in LDS; T0 of them
// is the byte table the fixed-width datums go through, as in vnode_kernel.
__device__ uint32_t g_crc8_table[8 * 256];
static bool g_crc8_table_init = false;

static int ensure_crc8_table() {
    if (g_crc8_table_init) return RW_OK;
    static uint32_t tab[8 * 256];
    rwx::crc_build_tables(tab);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_crc8_table), tab, sizeof tab) !=
        hipSuccess)
        return RW_E_INTERNAL;
    g_crc8_table_init = true;
    return RW_OK;
}

struct VnodeVarlenBatch {
    const int64_t* col_vals[MAX_KW];   // fixed-width keys (widened to 8 B)
    const uint8_t* col_valid[MAX_KW];
    const uint32_t* col_offs[MAX_KW];  // varchar keys: n_rows + 1 offsets
    const uint8_t* col_bytes[MAX_KW];  // varchar keys: the byte buffer
    uint8_t types[MAX_KW];
    uint32_t n_rows;
};

__global__ void vnode_varlen_kernel(VnodeVarlenBatch b, int n_keys,
                                    uint32_t vnode_count, uint16_t* out) {
    __shared__ uint32_t lut[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += blockDim.x)
        lut[i] = g_crc8_table[i];
    __syncthreads();
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < b.n_rows;
         r += stride) {
        uint32_t crc = 0xFFFFFFFFu;
        for (int k = 0; k < n_keys; k++) {
            if (!b.col_valid[k][r]) {
                crc = rwx::crc_feed_u32(lut, crc, rwx::NULL_SENTINEL);
            } else if (b.types[k] == RW_T_VARCHAR) {
                uint32_t lo = b.col_offs[k][r], hi = b.col_offs[k][r + 1];
                crc = rwx::crc_feed_str(lut, crc, b.col_bytes[k] + lo, hi - lo);
            } else if (b.types[k] == RW_T_I32) { // as vnode_kernel
                crc = rwx::crc_feed_u32(lut, crc, (uint32_t)b.col_vals[k][r]);
            } else {
                crc = rwx::crc_feed_u64(lut, crc, (uint64_t)b.col_vals[k][r]);
            }
        }
        out[r] = (uint16_t)((crc ^ 0xFFFFFFFFu) % vnode_count);
    }
}

extern "C" {

typedef struct {
    uint32_t n_keys;
    const uint32_t* key_indices;
    uint32_t vnode_count;
} RwVnodeDesc;

// rw_vnode_compute for a key tuple with at least one varchar column, in any
// position and any mix with the fixed-width types. Every varchar key
// column's offsets are validated before the first device allocation.
static int vnode_compute_varlen(const RwVnodeDesc* d, const RwChunk* chunk,
                                uint16_t* out) {
    uint32_t n = chunk->n_rows;
    for (uint32_t k = 0; k < d->n_keys; k++) {
        const RwColumn& c = chunk->cols[d->key_indices[k]];
        if (c.type == RW_T_BOOL || c.type == RW_T_DECIMAL)
            FAIL(RW_E_INVAL, "vnode key type %d unsupported on GPU", c.type);
        if (c.type != RW_T_VARCHAR) continue;
        if (const char* why = rwvarlen::check_column(c, n))
            FAIL(RW_E_INVAL, "varchar vnode key (column %u): %s",
                 d->key_indices[k], why);
    }
    if (d->vnode_count < 1 || d->vnode_count > 65536)
        FAIL(RW_E_INVAL, "vnode_count %u (1..65536)", d->vnode_count);
    if (ensure_crc8_table() != RW_OK) FAIL(RW_E_INTERNAL, "crc table");
    if (n == 0) return RW_OK;
    DevOwner da;
    VnodeVarlenBatch b{};
    for (uint32_t k = 0; k < d->n_keys; k++) {
        const RwColumn& c = chunk->cols[d->key_indices[k]];
        b.types[k] = c.type;
        uint8_t* valid;
        HIP_TRY(da.alloc(&valid, n));
        HIP_TRY(hipMemcpy(valid, c.valid, n, hipMemcpyHostToDevice));
        b.col_valid[k] = valid;
        if (c.type == RW_T_VARCHAR) {
            auto* vd = (const RwVarlenData*)c.data;
            uint32_t* offs;
            uint8_t* bytes;
            HIP_TRY(da.alloc(&offs, ((size_t)n + 1) * 4));
            HIP_TRY(da.alloc(&bytes, vd->offsets[n] ? vd->offsets[n] : 1));
            HIP_TRY(hipMemcpy(offs, vd->offsets, ((size_t)n + 1) * 4,
                              hipMemcpyHostToDevice));
            if (vd->offsets[n])
                HIP_TRY(hipMemcpy(bytes, vd->bytes, vd->offsets[n],
                                  hipMemcpyHostToDevice));
            b.col_offs[k] = offs;
            b.col_bytes[k] = bytes;
        } else {
            int64_t* vals;
            HIP_TRY(da.alloc(&vals, (size_t)n * 8));
            if (c.type == RW_T_I32 || c.type == RW_T_F32) {
                std::vector<int64_t> tmp(n); // widen; hashed at native width
                for (uint32_t r = 0; r < n; r++)
                    tmp[r] = (int64_t)(uint32_t)((const uint32_t*)c.data)[r];
                HIP_TRY(hipMemcpy(vals, tmp.data(), (size_t)n * 8,
                                  hipMemcpyHostToDevice));
            } else {
                HIP_TRY(hipMemcpy(vals, c.data, (size_t)n * 8,
                                  hipMemcpyHostToDevice));
            }
            b.col_vals[k] = vals;
        }
    }
    b.n_rows = n;
    uint16_t* dout;
    HIP_TRY(da.alloc(&dout, (size_t)n * 2));
    vnode_varlen_kernel<<<grid_for(n), 256>>>(b, (int)d->n_keys,
                                              d->vnode_count, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 2, hipMemcpyDeviceToHost));
    return RW_OK;
}

int rw_vnode_compute(const RwVnodeDesc* d, const RwChunk* chunk, uint16_t* out) {
    if (!gpu_ok()) FAIL(RW_E_NOGPU, "no GPU visible");
    if (d->n_keys < 1 || d->n_keys > MAX_KW) FAIL(RW_E_INVAL, "n_keys");
    if (ensure_crc_table() != RW_OK) FAIL(RW_E_INTERNAL, "crc table");
    uint32_t n = chunk->n_rows;
    bool has_varchar = false;
    for (uint32_t k = 0; k < d->n_keys; k++)
        if (chunk->cols[d->key_indices[k]].type == RW_T_VARCHAR)
            has_varchar = true;
    if (has_varchar) return vnode_compute_varlen(d, chunk, out);
    DevOwner da;
    VnodeBatch b{};
    uint8_t types[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < d->n_keys; k++) {
        const RwColumn& c = chunk->cols[d->key_indices[k]];
        types[k] = c.type;
        if (c.type == RW_T_BOOL) FAIL(RW_E_INVAL, "bool vnode key unsupported on GPU");
        HIP_TRY(da.alloc(&b.col_vals[k], (size_t)n * 8));
        HIP_TRY(da.alloc(&b.col_valid[k], n));
        if (c.type == RW_T_I32 || c.type == RW_T_F32) {
            // widen to i64 storage but hash native width
            std::vector<int64_t> tmp(n);
            for (uint32_t r = 0; r < n; r++)
                tmp[r] = (int64_t)(uint32_t)((const uint32_t*)c.data)[r];
            HIP_TRY(hipMemcpy(b.col_vals[k], tmp.data(), (size_t)n * 8,
                              hipMemcpyHostToDevice));
        } else {
            HIP_TRY(hipMemcpy(b.col_vals[k], c.data, (size_t)n * 8,
                              hipMemcpyHostToDevice));
        }
        HIP_TRY(hipMemcpy(b.col_valid[k], c.valid, n, hipMemcpyHostToDevice));
    }
    b.n_rows = n;
    uint16_t* dout;
    HIP_TRY(da.alloc(&dout, (size_t)n * 2));
    vnode_kernel<<<grid_for(n), 256>>>(b, (int)d->n_keys, d->vnode_count, dout,
                                       types[0], types[1], types[2], types[3]);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 2, hipMemcpyDeviceToHost));
    return RW_OK;
}

typedef struct {
    RwVnodeDesc v;
    uint32_t n_outputs;
    const uint32_t* vnode_to_output;
} RwDispatchDesc;

// HashDataDispatcher::dispatch_data (dispatch.rs:949-1050): vnodes from the
// GPU kernel; the tiny per-row visibility/op rewrite is host-side (the
// device-side dense compaction lives in rw_exchange.hip's partition path).
// Varchar columns travel too: each output holds a fresh RwVarlenData (copy
// of offsets and bytes, NULL rows zero length) that rw_chunk_free releases.
// Every varchar column is validated before the first allocation, and an
// allocation failure after some outputs were built frees them.
int rw_dispatch_compute(const RwDispatchDesc* d, const RwChunk* chunk,
                        RwChunk** outs) {
    uint32_t n = chunk->n_rows;
    for (uint32_t c = 0; c < chunk->n_cols; c++) {
        if (chunk->cols[c].type != RW_T_VARCHAR) continue;
        if (const char* why = rwvarlen::check_column(chunk->cols[c], n))
            FAIL(RW_E_INVAL, "dispatch: varchar column %u: %s", c, why);
    }
    std::vector<uint16_t> vnodes(n);
    int rc = rw_vnode_compute(&d->v, chunk, vnodes.data());
    if (rc != RW_OK) return rc;

    std::vector<uint8_t> ops(chunk->ops, chunk->ops + n);
    auto visible = [&](uint32_t r) { return !chunk->vis || chunk->vis[r]; };
    auto datum_eq = [&](uint32_t col, uint32_t a, uint32_t b) {
        const RwColumn& c = chunk->cols[col];
        if (c.valid[a] != c.valid[b]) return false;
        if (!c.valid[a]) return true;
        switch (c.type) {
            case RW_T_I32: return ((const int32_t*)c.data)[a] == ((const int32_t*)c.data)[b];
            case RW_T_VARCHAR: { // validity, length, bytes
                auto* vd = (const RwVarlenData*)c.data;
                uint32_t la = vd->offsets[a + 1] - vd->offsets[a];
                uint32_t lb = vd->offsets[b + 1] - vd->offsets[b];
                return la == lb &&
                       (la == 0 || memcmp(vd->bytes + vd->offsets[a],
                                          vd->bytes + vd->offsets[b], la) == 0);
            }
            default: return ((const int64_t*)c.data)[a] == ((const int64_t*)c.data)[b];
        }
    };
    long last_ud = -1;
    for (uint32_t r = 0; r < n; r++) {
        if (!visible(r)) continue;
        if (ops[r] == RW_OP_UPDATE_DELETE) {
            last_ud = (long)r;
        } else if (ops[r] == RW_OP_UPDATE_INSERT && last_ud >= 0) {
            bool changed = false;
            for (uint32_t k = 0; k < d->v.n_keys && !changed; k++)
                changed = !datum_eq(d->v.key_indices[k], (uint32_t)last_ud, r);
            if (changed) {
                ops[last_ud] = RW_OP_DELETE;
                ops[r] = RW_OP_INSERT;
            }
            last_ud = -1;
        }
    }

    uint32_t built = 0;
    try {
        // a varchar column's output form, built once: NULL rows zero length
        std::vector<std::vector<uint64_t>> voffs(chunk->n_cols);
        std::vector<std::vector<uint8_t>> vbytes(chunk->n_cols);
        for (uint32_t c = 0; c < chunk->n_cols; c++) {
            if (chunk->cols[c].type != RW_T_VARCHAR) continue;
            auto* vd = (const RwVarlenData*)chunk->cols[c].data;
            voffs[c].assign((size_t)n + 1, 0);
            vbytes[c].reserve(vd->offsets[n]);
            for (uint32_t r = 0; r < n; r++) {
                if (chunk->cols[c].valid[r])
                    vbytes[c].insert(vbytes[c].end(),
                                     vd->bytes + vd->offsets[r],
                                     vd->bytes + vd->offsets[r + 1]);
                voffs[c][r + 1] = vbytes[c].size();
            }
        }
        std::vector<uint8_t> vis(n);
        for (uint32_t o = 0; o < d->n_outputs; o++) {
            rwchunk::Builder cb(n, chunk->n_cols);
            for (uint32_t c = 0; c < chunk->n_cols; c++) {
                const RwColumn& col = chunk->cols[c];
                auto valid = rwchunk::from_valid(col.valid);
                if (col.type == RW_T_VARCHAR)
                    // never refused: voffs[c][n] <= the input's 32-bit total
                    (void)cb.varchar(voffs[c].data(), vbytes[c].data(), nullptr,
                                     valid);
                else
                    cb.raw(col.type, col.data, valid);
            }
            cb.ops(ops.data());
            for (uint32_t r = 0; r < n; r++)
                vis[r] = visible(r) && d->vnode_to_output[vnodes[r]] == o ? 1 : 0;
            cb.vis(vis.data());
            outs[o] = cb.release();
            built = o + 1;
        }
    } catch (const std::bad_alloc&) {
        for (uint32_t o = 0; o < built; o++) {
            rw_chunk_free(outs[o]);
            outs[o] = nullptr;
        }
        FAIL(RW_E_INTERNAL, "dispatch: out of host memory");
    }
    return RW_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------
// HashJoin (round-1 kernels: Inner + append-only Inner)
// ---------------------------------------------------------------------------
//
// Implements eq_join_oneside for T=Inner (hash_join.rs:949-1075): per probe
// row, walk the other side's rows under the join key, evaluate the optional
// comparison condition (:1294-1302), emit one concatenated output row per
// match with the probe row's (downgraded) op, then apply the probe row to
// its own side's state (:1248-1259). The append-only optimize deletes the
// single matched row and skips the own-side insert (:1241-1245,1359-1364).
// Matched-row iteration order is a chain walk, not memcomparable pk order —
// valid because inner-join epoch outputs are compared as row multisets
// (the reference sorts its own snapshots).

#define MAX_COLS 8
#define MAX_OUT 16

// (JoinSlot/jslot helpers and the DISTINCT dedup kernels moved before
// HashAgg — shared by the agg dedup tables)


struct JoinMeta {
    int KW;
    int n_cols[2];
    int n_pk[2];
    uint8_t key_cols[2][MAX_KW];
    uint8_t pk_cols[2][MAX_KW];
    uint8_t null_safe_mask;
    int n_out;
    uint8_t out_src[MAX_OUT]; // 0 = left, 1 = right
    uint8_t out_col[MAX_OUT];
    uint8_t n_cond; // 0..2 conjuncts (AND)
    struct {
        uint8_t op, src_l, col_l, src_r, col_r;
        long long rconst; // added to the right operand
    } cond[2];
    uint8_t append_only;
    uint8_t join_type;    // RwJoinType
    uint8_t need_deg[2];  // need_left/right_degree (join/mod.rs:153-165)
    uint8_t vc_mask[2];   // bit c = column c of the side is RW_T_VARCHAR
};

struct JoinBatchDev {
    int64_t* col_vals[MAX_COLS];
    uint8_t* col_valid[MAX_COLS];
    uint8_t* ops;
    uint8_t* vis;
    uint32_t n_rows;
    // every visible row is an Insert: no same-launch thread walks the own
    // side, so record payloads may use plain cached stores (no sc1, no
    // vmcnt drain) — cross-launch visibility comes from the kernel boundary
    uint8_t all_insert;
    // every referenced cell non-NULL: the probe skips the ops/validity
    // byte streams entirely (checked at upload)
    uint8_t all_valid;
    // join keys are pairwise distinct within the batch (host-verified; true
    // by construction for agg-output inputs like Nexmark q8's): at most one
    // chain push per slot per launch, so the head publish needs no CAS
    uint8_t unique_keys;
    // no visible row is an Insert: the inner probe's pre-assigned layout
    // reserves no records for the batch, so a full row store still takes
    // the deletes that let rw_join_compact make room
    uint8_t no_insert;
};

struct JoinOutDev {
    // COLUMNAR output block: column c occupies vals[c*cap ..), so emit
    // stores are lane-coalesced and the q3 agg hop reads it as plain
    // columnar input (stride 1)
    int64_t* vals;   // [n_out][cap]
    uint8_t* nulls;  // [n_out][cap]
    uint8_t* ops;    // [cap]
    uint32_t* counters; // [0]=cursor [1]=overflow
    uint32_t cap;
};

// Find-only with PLAIN (cached) loads — valid only for a side that is not
// mutated during this launch: cross-launch visibility comes from the kernel
// boundary, and cached loads fetch whole lines once instead of per-word
// fabric transactions.
__device__ __forceinline__ uint32_t table_find_cached(
    const uint32_t* state, const int64_t* keys, const uint32_t* key_nulls,
    uint32_t cap_mask, const int64_t* kw, uint32_t nullmask, int KW) {
    uint32_t slot = (uint32_t)(hash_key(kw, nullmask, KW) & cap_mask);
    for (uint32_t probes = 0; probes <= cap_mask; probes++) {
        uint32_t st = state[slot];
        if (st == SLOT_EMPTY) return (uint32_t)-1;
        if (st == SLOT_READY) {
            bool eq = key_nulls[slot] == nullmask;
            for (int i = 0; eq && i < KW; i++)
                eq = keys[(size_t)slot * KW + i] == kw[i];
            if (eq) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return (uint32_t)-1;
}

// Select word `idx` of a register-resident record copy. Unrolled selects:
// a dynamic index into a private array would demote it to scratch, which
// defeats the point of the register walk.
__device__ __forceinline__ long long rec_sel(const long long* recv, int idx) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < 6; w++)
        if (w == idx) v = recv[w];
    return v;
}

// join_cond_ok over a register-resident match record (no memory re-reads)
__device__ __forceinline__ bool join_cond_ok_rec(const JoinMeta& m,
                                                 int probe_side,
                                                 const JoinBatchDev& b,
                                                 uint32_t r,
                                                 uint32_t validbits,
                                                 const long long* recv) {
    for (int ci = 0; ci < m.n_cond; ci++) {
        auto& cd = m.cond[ci];
        auto fetch = [&](uint8_t src, uint8_t col, int64_t* v) -> bool {
            if ((int)src == probe_side) {
                if (!b.col_valid[col][r]) return false;
                *v = b.col_vals[col][r];
            } else {
                if (!((validbits >> col) & 1)) return false;
                *v = rec_sel(recv, col);
            }
            return true;
        };
        int64_t a, c;
        if (!fetch(cd.src_l, cd.col_l, &a)) return false; // NULL ⇒ false
        if (!fetch(cd.src_r, cd.col_r, &c)) return false;
        c += cd.rconst;
        bool ok;
        switch (cd.op) {
            case RW_CMP_LT: ok = a < c; break;
            case RW_CMP_LE: ok = a <= c; break;
            case RW_CMP_GT: ok = a > c; break;
            case RW_CMP_GE: ok = a >= c; break;
            default: ok = false;
        }
        if (!ok) return false;
    }
    return true;
}

__device__ __forceinline__ bool join_cond_ok(const JoinMeta& m, int probe_side,
                                             const JoinBatchDev& b, uint32_t r,
                                             uint32_t validbits,
                                             const long long* mvals) {
    for (int ci = 0; ci < m.n_cond; ci++) {
        auto& cd = m.cond[ci];
        auto fetch = [&](uint8_t src, uint8_t col, int64_t* v) -> bool {
            if ((int)src == probe_side) {
                if (!b.col_valid[col][r]) return false;
                *v = b.col_vals[col][r];
            } else {
                if (!((validbits >> col) & 1)) return false;
                *v = mvals[col];
            }
            return true;
        };
        int64_t a, c;
        if (!fetch(cd.src_l, cd.col_l, &a)) return false; // NULL ⇒ false
        if (!fetch(cd.src_r, cd.col_r, &c)) return false;
        c += cd.rconst;
        bool ok;
        switch (cd.op) {
            case RW_CMP_LT: ok = a < c; break;
            case RW_CMP_LE: ok = a <= c; break;
            case RW_CMP_GT: ok = a > c; break;
            case RW_CMP_GE: ok = a >= c; break;
            default: ok = false;
        }
        if (!ok) return false;
    }
    return true;
}

// probe the match side + update own side, one thread per probe row.
// Emission reserves output rows with ONE wave-level atomicAdd per iteration;
// the match side is immutable during a non-append-only launch, so it is read
// with plain cached loads (one line per slot, one per record). The
// append-only path (in-launch kill-on-match) uses the sc1 protocol.

// ---- join-type predicates (join/mod.rs:120-165; oracle_join.cpp mirrors) ----
__host__ __device__ __forceinline__ bool j_is_semi(uint8_t t) {
    return t == RW_JOIN_LEFT_SEMI || t == RW_JOIN_RIGHT_SEMI;
}
__host__ __device__ __forceinline__ bool j_is_anti(uint8_t t) {
    return t == RW_JOIN_LEFT_ANTI || t == RW_JOIN_RIGHT_ANTI;
}
__host__ __device__ __forceinline__ bool j_is_outer_side(uint8_t t, int side) {
    return t == RW_JOIN_FULL_OUTER ||
           (t == RW_JOIN_LEFT_OUTER && side == RW_SIDE_LEFT) ||
           (t == RW_JOIN_RIGHT_OUTER && side == RW_SIDE_RIGHT);
}
__host__ __device__ __forceinline__ bool j_outer_side_null(uint8_t t, int side) {
    return t == RW_JOIN_FULL_OUTER ||
           (t == RW_JOIN_LEFT_OUTER && side == RW_SIDE_RIGHT) ||
           (t == RW_JOIN_RIGHT_OUTER && side == RW_SIDE_LEFT);
}
__host__ __device__ __forceinline__ bool j_forward_exactly_once(uint8_t t, int side) {
    return ((t == RW_JOIN_LEFT_SEMI || t == RW_JOIN_LEFT_ANTI) && side == RW_SIDE_LEFT) ||
           ((t == RW_JOIN_RIGHT_SEMI || t == RW_JOIN_RIGHT_ANTI) && side == RW_SIDE_RIGHT);
}
__host__ __device__ __forceinline__ bool j_only_forward_matched_side(uint8_t t, int side) {
    return ((t == RW_JOIN_LEFT_SEMI || t == RW_JOIN_LEFT_ANTI) && side == RW_SIDE_RIGHT) ||
           ((t == RW_JOIN_RIGHT_SEMI || t == RW_JOIN_RIGHT_ANTI) && side == RW_SIDE_LEFT);
}
__host__ __device__ __forceinline__ bool j_need_degree(uint8_t t, int side) {
    if (side == RW_SIDE_LEFT)
        return t == RW_JOIN_FULL_OUTER || t == RW_JOIN_LEFT_OUTER ||
               t == RW_JOIN_LEFT_ANTI || t == RW_JOIN_LEFT_SEMI;
    return t == RW_JOIN_FULL_OUTER || t == RW_JOIN_RIGHT_OUTER ||
           t == RW_JOIN_RIGHT_ANTI || t == RW_JOIN_RIGHT_SEMI;
}

template <bool NT, typename T>
__device__ __forceinline__ void jout_store(T* p, T v) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// The one output-row writer of the join: every emission stores its row
// through here. Writes row `orow`: probe-side cells from batch row r, match-side
// cells through the caller's accessor mval(col) — rec_sel over a
// register-resident record (a dynamic index into the private copy would
// demote it to scratch), a plain mv[col], or an sc1 load —
// validity from match_vb. form bit0 = include the probe side's columns,
// bit1 = include the matched record's columns; excluded sides are NULL
// (JoinOutBuilder append_row / _update / _matched, join/builder.rs:153-318).
// NT = nontemporal stores for ops, values and nulls alike: pre-assigned
// rows are written once and only read by later launches, and regular
// stores pay a read-for-ownership line fetch per partial write.
template <bool NT, typename MVal>
__device__ __forceinline__ void jwrite_row(JoinOutDev& out, const JoinMeta& m,
                                           int S, uint8_t op,
                                           const JoinBatchDev& b, uint32_t r,
                                           bool dense, uint32_t match_vb,
                                           MVal mval, int form,
                                           uint32_t orow) {
    jout_store<NT>(&out.ops[orow], op);
    for (int c = 0; c < m.n_out; c++) {
        bool from_probe = (int)m.out_src[c] == S;
        uint8_t col = m.out_col[c];
        int64_t v = 0;
        uint8_t valid = 0;
        if (from_probe && (form & 1)) {
            valid = dense || b.col_valid[col][r];
            v = b.col_vals[col][r];
        } else if (!from_probe && (form & 2)) {
            valid = (match_vb >> col) & 1;
            v = mval(col);
        }
        jout_store<NT>(&out.vals[(size_t)c * out.cap + orow],
                       valid ? v : (int64_t)0);
        jout_store<NT>(&out.nulls[(size_t)c * out.cap + orow],
                       (uint8_t)!valid);
    }
}

// emit one output row with per-emission reservation (plain stores); the
// match-side accessor is the caller's, as for jwrite_row
template <typename MVal>
__device__ __forceinline__ void jemit_row(JoinOutDev& out, const JoinMeta& m,
                                          int S, uint8_t op,
                                          const JoinBatchDev& b, uint32_t r,
                                          uint32_t match_vb, MVal mval,
                                          int form) {
    uint32_t orow = atomicAdd(&out.counters[0], 1u);
    if (orow >= out.cap) {
        atomicExch(&out.counters[1], 1u);
        return;
    }
    jwrite_row<false>(out, m, S, op, b, r, false, match_vb, mval, form, orow);
}

// own-side insert/delete (join/hash_join.rs:591-681 without the LRU tier)
__device__ __forceinline__ void jown_insert(JoinSideDev own, const JoinMeta& m,
                                            int S, const JoinBatchDev& b,
                                            uint32_t r, const int64_t* kw,
                                            uint32_t nullmask, JoinOutDev out,
                                            uint32_t init_deg) {
    // wave-aggregated row reservation: the single cursor sustains only
    // ~2.1 G same-line atomicAdds/s, so 1M per-lane adds cost ~0.47 ms per
    // launch (measured) — one leader add per wave instead
    uint64_t wmask = __ballot(true); // lanes currently inserting
    int lane = threadIdx.x & 63;
    int leader = 63 - __clzll(wmask);
    uint32_t base = 0;
    if (lane == leader)
        base = atomicAdd(own.row_cursor, (uint32_t)__popcll(wmask));
    base = (uint32_t)__shfl((int)base, leader);
    uint32_t row = base + (uint32_t)__popcll(wmask & ((1ULL << lane) - 1));
    if (row >= own.row_cap) {
        atomicExch(&out.counters[1], 3u); // row store full
        return;
    }
    uint64_t h64 = hash_key(kw, nullmask, m.KW);
    JoinRowHdr* h = jrow(own, row);
    uint32_t vb = 0;
    long long* hv = jvals(h);
    if (b.all_insert) {
        // plain cached stores: inserts never read records (chained
        // buckets), and all-Insert launches have no same-side walkers;
        // jbucket_insert drains to the coherence point before the CAS
        // publish so later foreign-key walks fetch real bytes.
        for (int c = 0; c < m.n_cols[S]; c++) {
            hv[c] = b.col_vals[c][r];
            vb |= (uint32_t)(b.col_valid[c][r] != 0) << c;
        }
        h->validbits = vb;
        h->degree = init_deg;
        h->alive = 1;
        jbucket_insert(own, h64, row, /*sc1_next=*/false);
    } else {
        for (int c = 0; c < m.n_cols[S]; c++) {
            st_i64((int64_t*)&hv[c], b.col_vals[c][r]);
            vb |= (uint32_t)(b.col_valid[c][r] != 0) << c;
        }
        st_u32(&h->validbits, vb);
        st_u32(&h->degree, init_deg);
        st_u32(&h->alive, 1);
        jbucket_insert(own, h64, row, /*sc1_next=*/true);
    }
}

__device__ __forceinline__ void jown_delete(JoinSideDev own, const JoinMeta& m,
                                            int S, const JoinBatchDev& b,
                                            uint32_t r, const int64_t* kw,
                                            uint32_t nullmask) {
    // delete own row: FULL-row compare + CAS claim; the
    // full-row compare subsumes the key filter (key cols are row cols)
    uint32_t row = jbucket_head(own, hash_key(kw, nullmask, m.KW), true);
    while (row != UINT32_MAX) {
        JoinRowHdr* h = jrow(own, row);
        if (ld_u32(&h->alive)) {
            uint32_t vb = ld_u32(&h->validbits);
            const long long* hv = jvals(h);
            bool eq = true;
            for (int c = 0; eq && c < m.n_cols[S]; c++) {
                uint8_t va = b.col_valid[c][r];
                uint8_t vbc = (vb >> c) & 1;
                eq = (va == vbc) &&
                     (!va || b.col_vals[c][r] == ld_i64((const int64_t*)&hv[c]));
            }
            if (eq && atomicCAS(&h->alive, 1u, 0u) == 1u) {
                if (own.killed) {
                    uint32_t kidx = atomicAdd(own.killed_cursor, 1u);
                    if (kidx < own.killed_cap) own.killed[kidx] = row;
                }
                break;
            }
        }
        row = ld_u32(&h->next);
    }
}

// one probe row of a non-inner join: eq_join_oneside for
// LeftOuter/RightOuter/FullOuter/Semi/Anti (hash_join.rs:949-1374 +
// with_match_on_insert/delete, join/builder.rs:173-318). Degree transitions
// use the matched record's atomic degree; the emitted transition rows are
// independent of which chunk row wins a concurrent transition, so the
// per-chunk output multiset matches the reference's sequential apply
// (mixed insert/delete chunks sharing a join key run in serial segments —
// conflict_segments).
__device__ void join_probe_row_noninner(const JoinBatchDev& b, JoinSideDev own,
                                        JoinSideDev match, const JoinMeta& m,
                                        int S, JoinOutDev out, uint32_t r,
                                        bool is_insert, uint8_t op,
                                        const int64_t* kw, uint32_t nullmask,
                                        bool never_match) {
    uint8_t T = m.join_type;
    bool fwd_once = j_forward_exactly_once(T, S);
    bool anti = j_is_anti(T), semi = j_is_semi(T);
    bool outer_self = j_is_outer_side(T, S);
    bool only_fwd_m = j_only_forward_matched_side(T, S);
    bool outer_null = j_outer_side_null(T, S);
    // the probe row alone, match side NULL
    auto forward = [&]() {
        jemit_row(out, m, S, op, b, r, 0, [](int) { return 0LL; }, 1);
    };
    if (never_match) {
        // null-safe NeverMatch forwards for anti/outer (hash_join.rs:1143-1152)
        if ((anti && fwd_once) || outer_self)
            forward();
        return; // no state write
    }
    uint32_t mhead =
        jbucket_head(match, hash_key(kw, nullmask, m.KW), false);
    uint32_t my_deg = 0;
    {
        // REGISTER-RESIDENT walk for narrow aligned records (same refetch
        // pathology and fix as the inner probe's walk);
        // wide records keep the field walk. The degree update stays an
        // atomic on the record itself (other lanes observe it through the
        // atomic's return value, never through their register copies).
        const bool regw =
            match.row_stride <= 64 && !(match.row_stride & 15);
        const int nw16 = (int)(match.row_stride >> 4);
        long long rec[8];
        uint32_t row = mhead;
        while (row != UINT32_MAX) {
            JoinRowHdr* h = jrow(match, row);
            uint32_t alive, nxt, vb;
            if (regw) {
                const long long* rp = (const long long*)h;
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (w < nw16)
                        *(longlong2*)&rec[2 * w] =
                            *(const longlong2*)(rp + 2 * w);
                alive = (uint32_t)(uint64_t)rec[0];
                nxt = (uint32_t)((uint64_t)rec[0] >> 32);
                vb = (uint32_t)(uint64_t)rec[1];
            } else {
                alive = h->alive;
                nxt = h->next;
                vb = h->validbits;
            }
            bool eq = alive != 0;
            for (int i = 0; eq && i < m.KW; i++) {
                uint8_t col = m.key_cols[1 - S][i];
                bool valid = (vb >> col) & 1;
                if (valid == (bool)((nullmask >> i) & 1)) {
                    eq = false;
                } else if (valid) {
                    long long v =
                        regw ? rec_sel(rec + 2, col) : jvals(h)[col];
                    if (v != kw[i]) eq = false;
                }
            }
            if (eq && (regw ? join_cond_ok_rec(m, S, b, r, vb, rec + 2)
                            : join_cond_ok(m, S, b, r, vb, jvals(h)))) {
                my_deg++;
                bool zero = false;
                if (m.need_deg[1 - S]) {
                    // insert: emit BEFORE increment (zero == pre-value 0);
                    // delete: decrement BEFORE emit (zero == post-value 0)
                    // (hash_join.rs:1311-1342)
                    uint32_t old = atomicAdd(&h->degree,
                                             is_insert ? 1u : (uint32_t)-1);
                    zero = is_insert ? old == 0 : old == 1;
                    // §8f-2 degree-table delta: record the touched row once
                    if (match.deg_dirty_flag &&
                        ld_u32(&match.deg_dirty_flag[row]) == 0 &&
                        atomicCAS(&match.deg_dirty_flag[row], 0u, 1u) == 0u) {
                        uint32_t di = atomicAdd(match.deg_dirty_n, 1u);
                        match.deg_dirty_list[di] = row;
                    }
                }
                auto emit2 = [&](uint8_t op2, int form) {
                    if (regw)
                        jemit_row(out, m, S, op2, b, r, vb,
                                  [&](int col) { return rec_sel(rec + 2, col); },
                                  form);
                    else
                        jemit_row(out, m, S, op2, b, r, vb,
                                  [&](int col) { return jvals(h)[col]; },
                                  form);
                };
                if (is_insert) {
                    if (anti) {
                        if (zero && only_fwd_m) emit2(RW_OP_DELETE, 2);
                    } else if (semi) {
                        if (zero && only_fwd_m) emit2(RW_OP_INSERT, 2);
                    } else if (zero && outer_null) {
                        emit2(RW_OP_DELETE, 2);
                        emit2(RW_OP_INSERT, 3);
                    } else if (!fwd_once) {
                        emit2(RW_OP_INSERT, 3);
                    }
                } else {
                    if (anti) {
                        if (zero && only_fwd_m) emit2(RW_OP_INSERT, 2);
                    } else if (semi) {
                        if (zero && only_fwd_m) emit2(RW_OP_DELETE, 2);
                    } else if (zero && outer_null) {
                        emit2(RW_OP_DELETE, 3);
                        emit2(RW_OP_INSERT, 2);
                    } else if (!fwd_once) {
                        emit2(RW_OP_DELETE, 3);
                    }
                }
            }
            row = nxt;
        }
    }
    if (my_deg == 0) {
        // forward_if_not_matched (join/builder.rs:303-312)
        if ((anti && fwd_once) || outer_self)
            forward();
    } else if (semi && fwd_once) {
        // forward_exactly_once_if_matched (join/builder.rs:287-300)
        forward();
    }
    if (is_insert)
        jown_insert(own, m, S, b, r, kw, nullmask, out, my_deg);
    else
        jown_delete(own, m, S, b, r, kw, nullmask);
}

// Per-batch setup for the inner probe's PRE-ASSIGNED layout (see the
// kernel comment below): output region [0, n) is one sparse slot per
// probe row (ops sentinel 0xFF = empty; the emission cursor starts at n
// for >1-match overflow), and the batch's record rows are reserved as ONE
// cursor bump so the kernel needs no cross-lane reservation at all
// (n_records = n, or 0 for a batch without inserts).
__global__ void jprobe_setup_kernel(JoinOutDev out, uint32_t* row_cursor,
                                    uint32_t row_cap, uint32_t* row_base,
                                    uint32_t n, uint32_t n_records) {
    out.counters[0] = n; // overflow emissions append past the sparse region
    uint32_t base = atomicAdd(row_cursor, n_records);
    if ((uint64_t)base + n_records > row_cap)
        atomicExch(&out.counters[1], 3u);
    *row_base = base;
}

__global__ void join_count_emitted_kernel(const uint8_t* ops, uint32_t n,
                                          const uint32_t* counters,
                                          unsigned long long* out_count) {
    uint32_t stride = gridDim.x * blockDim.x;
    unsigned long long local = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride)
        local += ops[r] != 0xFF;
    if (local) atomicAdd(out_count, local);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(out_count, (unsigned long long)(counters[0] - n));
}

// non-inner probe (outer/semi/anti): one thread per row over the shared
// per-row prologue, then the matched-side walk + degree/emission tree in
// join_probe_row_noninner. Separate kernel so its wider live range
// (register-resident records + the emission decision tree) gets its own
// launch bounds instead of spilling the inner kernel.
__global__ __launch_bounds__(256, 4) void join_probe_noninner_kernel(
    JoinBatchDev b, JoinSideDev own, JoinSideDev match, JoinMeta m, int S,
    JoinOutDev out, uint32_t r0, uint32_t r1) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1;
         r += stride) {
        if (b.vis && !b.vis[r]) continue;
        uint8_t op_in = b.ops[r];
        bool is_insert = (op_in == RW_OP_INSERT || op_in == RW_OP_UPDATE_INSERT);
        uint8_t op = is_insert ? RW_OP_INSERT : RW_OP_DELETE;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.key_cols[S][i];
            bool valid = b.col_valid[col][r];
            kw[i] = valid ? b.col_vals[col][r] : 0;
            nullmask |= (!valid) << i;
        }
        bool never_match = (nullmask & ~(uint32_t)m.null_safe_mask) != 0;
        join_probe_row_noninner(b, own, match, m, S, out, r, is_insert, op,
                                kw, nullmask, never_match);
    }
}

__global__ __launch_bounds__(256, 6) void join_probe_kernel(
    JoinBatchDev b, JoinSideDev own, JoinSideDev match, JoinMeta m, int S,
    JoinOutDev out, uint32_t r0, uint32_t r1, const uint32_t* row_base) {
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t n = r1 - r0;
    uint32_t iters = (n + stride - 1) / stride;

    const bool dense = b.all_insert && b.all_valid && !b.vis;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = r0 + it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = dense ? (r < r1)
                            : ((r < r1) && !(b.vis && !b.vis[r]));
        uint8_t op_in =
            (active && !dense) ? b.ops[r] : RW_OP_INSERT;
        bool is_insert = (op_in == RW_OP_INSERT || op_in == RW_OP_UPDATE_INSERT);
        uint8_t op = is_insert ? RW_OP_INSERT : RW_OP_DELETE;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        bool never_match = false;
        if (active) {
            for (int i = 0; i < m.KW; i++) {
                uint8_t col = m.key_cols[S][i];
                bool valid = dense || b.col_valid[col][r];
                kw[i] = valid ? b.col_vals[col][r] : 0;
                nullmask |= (!valid) << i;
            }
            // null-safe NeverMatch (hash_join.rs:1004-1016)
            if (nullmask & ~(uint32_t)m.null_safe_mask) never_match = true;
        }

        // non-inner types run in join_probe_noninner_kernel (own launch
        // bounds: its register walk + emission tree would spill this
        // kernel's budget)
        if (never_match) active = false;

        uint32_t mhead = UINT32_MAX;
        uint32_t my_n = 0;
        uint32_t matched_row = UINT32_MAX;
        uint64_t h64 = 0;
        // register-resident copy of the last record the walk loaded, and
        // whether it is the (single) match — lets the emit below run with
        // zero record re-reads in the dominant unique-key case
        long long rec[8];
        bool rec_match = false;
        if (active) {
            h64 = hash_key(kw, nullmask, m.KW);
            mhead = jbucket_head(match, h64, m.append_only != 0);
            if (mhead != UINT32_MAX && !m.append_only) {
                uint32_t row = mhead;
                // REGISTER-RESIDENT walk (narrow records, 16-B-aligned
                // stride): each record is fetched ONCE as wide b128 loads
                // into registers and evaluated from there. The serialized
                // field-by-field walk refetches its line from HBM 2-3x —
                // with ~2048 lanes in flight per CU the 32-KB vL0 (and the
                // 4-MB XCD L2) evict a line between a record's `alive`
                // check and its key loads; PMC measured ~323 B fetched per
                // 64-B record (gpurun_out/pmcW67.txt) vs the one-line 128-B
                // model. Records wider than 64 B keep the field walk.
                if (match.row_stride <= 64 && !(match.row_stride & 15)) {
                    int nw16 = (int)(match.row_stride >> 4);
                    while (row != UINT32_MAX) {
                        const long long* rp =
                            (const long long*)jrow(match, row);
#pragma unroll
                        for (int w = 0; w < 4; w++)
                            if (w < nw16)
                                *(longlong2*)&rec[2 * w] =
                                    *(const longlong2*)(rp + 2 * w);
                        rec_match = false; // rec just overwritten
                        uint32_t alive = (uint32_t)(uint64_t)rec[0];
                        uint32_t nxt = (uint32_t)((uint64_t)rec[0] >> 32);
                        uint32_t vb = (uint32_t)(uint64_t)rec[1];
                        bool eq = alive != 0;
                        for (int i = 0; eq && i < m.KW; i++) {
                            uint8_t col = m.key_cols[1 - S][i];
                            bool valid = (vb >> col) & 1;
                            if (valid == (bool)((nullmask >> i) & 1))
                                eq = false;
                            else if (valid &&
                                     rec_sel(rec + 2, col) != kw[i])
                                eq = false;
                        }
                        if (eq &&
                            join_cond_ok_rec(m, S, b, r, vb, rec + 2)) {
                            my_n++;
                            matched_row = row;
                            rec_match = true; // match is register-resident
                        }
                        row = nxt;
                    }
                } else {
                    while (row != UINT32_MAX) {
                        JoinRowHdr* h = jrow(match, row);
                        if (h->alive &&
                            jhdr_key_eq(h, m.key_cols[1 - S], m.KW, kw,
                                        nullmask, false) &&
                            join_cond_ok(m, S, b, r, h->validbits,
                                         jvals(h))) {
                            my_n++;
                            matched_row = row;
                        }
                        row = h->next;
                    }
                }
            }
        }

        if (!m.append_only) {
            // PRE-ASSIGNED sparse emission: match 0 of probe row r goes to
            // output slot r (ops sentinel 0xFF marks empty slots; the host
            // compacts at drain); matches 2..k append past n via a
            // PER-LANE atomic on the rare multi-match lanes. NO cross-lane
            // ops: the q8-shape ladder measured ANY
            // wave-convergent reservation (ballot or shuffle scan) at
            // +135-155 us per 1M
            // rows — the convergence stalls the wave on its slowest lane's
            // dependent loads — while the pre-assigned form runs at the
            // random-access ceiling (profiles/r02_membw_probes.json).
            uint32_t my_base = r;
            uint32_t extra_base = 0;
            if (my_n > 1) {
                extra_base = atomicAdd(&out.counters[0], my_n - 1);
                if (extra_base + my_n - 1 > out.cap)
                    atomicExch(&out.counters[1], 1u); // overflow
            }
            // All three branches store NONTEMPORAL through jwrite_row.
            // (Measured store-policy A/B on the single-match emit: full NT
            // 0.251 ms/step against 0.255 both fully cached and with only
            // the values NT — a narrow win; the dense orow=r layout
            // coalesces well under every policy.)
            if (my_n == 1 && rec_match) {
                // SINGLE-PASS emission from the REGISTER-RESIDENT match
                // (the walk's last-loaded record): zero record re-reads.
                jwrite_row<true>(
                    out, m, S, op, b, r, dense, (uint32_t)(uint64_t)rec[1],
                    [&](int col) { return rec_sel(rec + 2, col); }, 3,
                    my_base);
            } else if (my_n == 1) {
                // SINGLE-PASS emission for the dominant <=1-match case:
                // the count walk already identified the row — no re-walk
                JoinRowHdr* h = jrow(match, matched_row);
                const long long* mv = jvals(h);
                jwrite_row<true>(
                    out, m, S, op, b, r, dense, h->validbits,
                    [&](int col) { return mv[col]; }, 3, my_base);
            } else if (my_n && !(extra_base + my_n - 1 > out.cap)) {
                // second walk: emit (JoinStreamChunkBuilder::append_row)
                uint32_t row = mhead;
                uint32_t k = 0;
                while (row != UINT32_MAX && k < my_n) {
                    JoinRowHdr* h = jrow(match, row);
                    if (h->alive &&
                        jhdr_key_eq(h, m.key_cols[1 - S], m.KW, kw, nullmask,
                                    false) &&
                        join_cond_ok(m, S, b, r, h->validbits, jvals(h))) {
                        const long long* mv = jvals(h);
                        jwrite_row<true>(
                            out, m, S, op, b, r, dense, h->validbits,
                            [&](int col) { return mv[col]; }, 3,
                            k == 0 ? my_base : extra_base + k - 1);
                        k++;
                    }
                    row = h->next;
                }
            }
        } else if (active && mhead != UINT32_MAX) {
            // append-only path: <=1 match; sc1 reads, per-match atomics,
            // plain stores
            uint32_t row = mhead;
            while (row != UINT32_MAX) {
                JoinRowHdr* h = jrow(match, row);
                uint32_t vb = ld_u32(&h->validbits);
                if (ld_u32(&h->alive) &&
                    jhdr_key_eq(h, m.key_cols[1 - S], m.KW, kw, nullmask,
                                true) &&
                    join_cond_ok(m, S, b, r, vb, jvals(h))) {
                    const long long* mv = jvals(h);
                    jemit_row(out, m, S, op, b, r, vb,
                              [&](int col) {
                                  return ld_i64((const int64_t*)&mv[col]);
                              },
                              3);
                    matched_row = row;
                }
                row = ld_u32(&h->next);
            }
        }

        if (!m.append_only) {
            // PRE-ASSIGNED record slot (row_base + r): inserting rows write
            // their record and link the bucket; every other row marks its
            // slot dead (walks and drains skip by `alive`). No cross-lane
            // cursor — see the emission comment above.
            if (r < r1) {
                uint32_t myrow = *row_base + r;
                bool do_insert = active && is_insert;
                // (a batch without inserts reserved no records)
                if (!b.no_insert && myrow < own.row_cap) {
                    JoinRowHdr* hd2 = jrow(own, myrow);
                    if (do_insert) {
                        long long* hv2 = jvals(hd2);
                        uint32_t vb2 = 0;
                        // (Measured dead end: nontemporal record-insert
                        // stores — both 8-B fields and register-assembled
                        // b128s — ran 0.320 vs 0.248 ms/step on q8. The
                        // 64-B lane stride means no single instruction
                        // covers a full line, so NT partial-line writes
                        // reach HBM unmerged, while the cached path's RFO
                        // is amortized by L2 byte-granular write merge.)
                        if (dense) {
                            for (int c = 0; c < m.n_cols[S]; c++)
                                hv2[c] = b.col_vals[c][r];
                            vb2 = (1u << m.n_cols[S]) - 1;
                            hd2->validbits = vb2;
                            hd2->degree = 0;
                            hd2->alive = 1;
                        } else if (b.all_insert) {
                            for (int c = 0; c < m.n_cols[S]; c++) {
                                hv2[c] = b.col_vals[c][r];
                                vb2 |= (uint32_t)(b.col_valid[c][r] != 0) << c;
                            }
                            hd2->validbits = vb2;
                            hd2->degree = 0;
                            hd2->alive = 1;
                        } else {
                            // sc1 payload: same-launch delete walkers read it
                            for (int c = 0; c < m.n_cols[S]; c++) {
                                st_i64((int64_t*)&hv2[c], b.col_vals[c][r]);
                                vb2 |= (uint32_t)(b.col_valid[c][r] != 0) << c;
                            }
                            st_u32(&hd2->validbits, vb2);
                            st_u32(&hd2->degree, 0);
                            st_u32(&hd2->alive, 1);
                        }
                        jbucket_insert(own, h64, myrow, !b.all_insert);
                    } else {
                        hd2->alive = 0;
                    }
                }
                if (active && !is_insert)
                    jown_delete(own, m, S, b, r, kw, nullmask);
            }
            continue;
        }
        if (!active) continue;

        if (m.append_only && is_insert && matched_row != UINT32_MAX) {
            // append-only optimize (hash_join.rs:1241-1245)
            st_u32(&jrow(match, matched_row)->alive, 0);
            if (match.killed) {
                uint32_t kidx = atomicAdd(match.killed_cursor, 1u);
                if (kidx < match.killed_cap) match.killed[kidx] = matched_row;
            }
            continue;
        }

        // own-side state update (join/hash_join.rs:591-681 without LRU tier)
        if (is_insert)
            jown_insert(own, m, S, b, r, kw, nullmask, out, 0);
        else
            jown_delete(own, m, S, b, r, kw, nullmask);
    }
}

// join state restore: append decoded state rows + bucket links + degrees
// (rw_stream.h contract). err: 3 = row store full.
__global__ void join_restore_kernel(JoinBatchDev b, JoinSideDev sd,
                                    JoinMeta m, int S,
                                    const uint32_t* degrees, uint32_t* err) {
    uint32_t stride = gridDim.x * blockDim.x;
    int lane = threadIdx.x & 63;
    uint32_t n = b.n_rows;
    uint32_t iters = (n + stride - 1) / stride;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r < n;
        uint64_t wmask = __ballot(active);
        if (!active) continue;
        int leader = 63 - __clzll(wmask);
        uint32_t base = 0;
        if (lane == leader)
            base = atomicAdd(sd.row_cursor, (uint32_t)__popcll(wmask));
        base = (uint32_t)__shfl((int)base, leader);
        uint32_t row = base + (uint32_t)__popcll(wmask & ((1ULL << lane) - 1));
        if (row >= sd.row_cap) {
            atomicExch(err, 3u);
            continue;
        }
        JoinRowHdr* hd = jrow(sd, row);
        long long* hv = jvals(hd);
        uint32_t vb = 0;
        for (int c = 0; c < m.n_cols[S]; c++) {
            hv[c] = b.col_vals[c][r];
            vb |= (uint32_t)(b.col_valid[c][r] != 0) << c;
        }
        hd->validbits = vb;
        hd->degree = degrees ? degrees[r] : 0;
        hd->alive = 1;
        int64_t kw[MAX_KW];
        uint32_t nm = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.key_cols[S][i];
            bool valid = (vb >> col) & 1;
            kw[i] = valid ? hv[col] : 0;
            nm |= (uint32_t)(!valid) << i;
        }
        jbucket_insert(sd, hash_key(kw, nm, m.KW), row, false);
    }
}

// Batched record gather for the checkpoint drains: one kernel + one D2H
// instead of a hipMemcpy per referenced row (~10 us each dominated drain
// time once kill/degree lists grew past a few hundred rows).
__global__ void jgather_rows_kernel(JoinSideDev sd, const uint32_t* ids,
                                    uint32_t n, uint8_t* out) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const uint8_t* src = sd.rows + (size_t)ids[i] * sd.row_stride;
        uint8_t* dst = out + (size_t)i * sd.row_stride;
        for (uint32_t w = 0; w < sd.row_stride; w += 8)
            *(long long*)(dst + w) = *(const long long*)(src + w);
    }
}

// §8f-4 memory reclamation: rebuild one join side's record store without
// its dead records (retractions and watermark sweeps retire rows in
// place; the reference's LSM compaction reclaims them at the store —
// here a periodic maintenance pass does, between epochs). Pass 1 packs
// alive records into a fresh store (next rebuilt later); pass 2 relinks
// the cleared buckets. Runs only on a DRAINED table (kill list and
// degree deltas consumed, flush mark at the cursor), so row ids are not
// referenced by any pending delta tracking.
__global__ void jcompact_copy_kernel(JoinSideDev oldsd, uint8_t* nrows,
                                     uint32_t* ncursor, uint32_t old_n) {
    uint32_t stride = gridDim.x * blockDim.x;
    int lane = threadIdx.x & 63;
    uint32_t iters = (old_n + stride - 1) / stride;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool alive = r < old_n && jrow(oldsd, r)->alive;
        uint64_t wmask = __ballot(alive);
        if (!alive) continue;
        int leader = 63 - __clzll(wmask);
        uint32_t base = 0;
        if (lane == leader)
            base = atomicAdd(ncursor, (uint32_t)__popcll(wmask));
        base = (uint32_t)__shfl((int)base, leader);
        uint32_t nr = base + (uint32_t)__popcll(wmask & ((1ULL << lane) - 1));
        const uint8_t* src = oldsd.rows + (size_t)r * oldsd.row_stride;
        uint8_t* dst = nrows + (size_t)nr * oldsd.row_stride;
        for (uint32_t wq = 0; wq < oldsd.row_stride; wq += 8)
            *(long long*)(dst + wq) = *(const long long*)(src + wq);
        ((JoinRowHdr*)dst)->next = UINT32_MAX;
    }
}

__global__ void jcompact_link_kernel(JoinSideDev sd, JoinMeta m, int S,
                                     uint32_t n) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        JoinRowHdr* h = jrow(sd, r);
        int64_t kw[MAX_KW];
        uint32_t nm = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.key_cols[S][i];
            bool valid = (h->validbits >> col) & 1;
            kw[i] = valid ? jvals(h)[col] : 0;
            nm |= (uint32_t)(!valid) << i;
        }
        jbucket_insert(sd, hash_key(kw, nm, m.KW), r, false);
    }
}

// watermark TTL sweeps (state_table watermark cleaning):
// rows/groups whose watermarked key column sorts below the value are
// retired in place (slots stay READY so linear probing is undisturbed;
// memory reclamation is compaction work for a later round)
__global__ void join_clean_kernel(JoinSideDev sd, int kcol, long long wm,
                                  int KW) {
    // kcol = RECORD column of the watermarked key position. Buckets mix
    // keys, so the watermark predicate runs PER RECORD; rows below the
    // watermark are retired in place (slot entries stay — probes skip dead
    // records by the alive flag).
    (void)KW;
    size_t cap = (size_t)sd.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        uint64_t packed = __hip_atomic_load(&sd.slots8[slot], RLX);
        if ((uint32_t)packed == 0) continue; // bloom 0 = empty
        uint32_t row = jhead_of(packed);
        while (row != UINT32_MAX) {
            JoinRowHdr* h = jrow(sd, row);
            if (ld_u32(&h->alive) &&
                ((ld_u32(&h->validbits) >> kcol) & 1) && // NULLs largest
                ld_i64((const int64_t*)&jvals(h)[kcol]) < wm) {
                st_u32(&h->alive, 0);
                // §8f-2 state-cleaning spill deltas (the reference's
                // commit applies the watermark as a range delete on the
                // store, state_table.rs:1707): route retired rows
                // through the kill list so the next drain nets them to
                // DELETE frames — a restore replay must not resurrect
                // them
                if (sd.killed) {
                    uint32_t kidx = atomicAdd(sd.killed_cursor, 1u);
                    if (kidx < sd.killed_cap) sd.killed[kidx] = row;
                }
            }
            row = ld_u32(&h->next);
        }
    }
}

// crecs/crec_n/crec_cap/cover: capture the cleaned PERSISTED groups'
// keys so the host can append DELETE spill frames — the reference's
// commit applies the watermark as a range delete on the store
// (state_table.rs:1707), so the spill stream must net cleaned rows out
// or a restore replay resurrects them. On capture overflow the slot is
// LEFT UNCLEANED (cover set); the host grows the buffer and reruns —
// already-cleaned slots skip via the has_prev they cleared.
__global__ void agg_clean_kernel(AggTableDev t, int kpos, long long wm, int KW,
                                 int n_calls, AggCallDev c0, AggCallDev c1,
                                 AggCallDev c2, AggCallDev c3,
                                 DedupDirtyRec* crecs, uint32_t* crec_n,
                                 uint32_t crec_cap, uint32_t* cover) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    size_t cap = (size_t)t.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        if (ld_u32(&t.state[(uint32_t)slot]) != SLOT_READY) continue;
        if ((ld_u32(&t.key_nulls[(uint32_t)slot]) >> kpos) & 1) continue;
        if (ld_i64((const int64_t*)&t.keys[slot * KW + kpos]) >= wm) continue;
        if (t.has_prev[(uint32_t)slot]) {
            uint32_t ci2 = atomicAdd(crec_n, 1u);
            if (ci2 >= crec_cap) {
                atomicExch(cover, 1u);
                continue; // retried after the host grows the buffer
            }
            for (int w = 0; w < KW; w++)
                crecs[ci2].key[w] = t.keys[slot * KW + w];
            crecs[ci2].nulls = t.key_nulls[(uint32_t)slot];
            crecs[ci2].count = 0;
        }
        // reset the group as if freshly created (late rows restart it)
        for (int ci = 0; ci < n_calls; ci++) {
            long long init = 0;
            if (calls[ci].kind == RW_AGG_MIN) init = INT64_MAX;
            if (calls[ci].kind == RW_AGG_MAX) init = INT64_MIN;
            t.acc[(size_t)ci * cap + slot] = init;
            t.has[(size_t)ci * cap + slot] = 0;
            if (calls[ci].minput) {
                uint32_t row = t.mheads[(size_t)calls[ci].mord * cap + slot];
                while (row != UINT32_MAX) {
                    st_u32(&t.malive[row], 0);
                    // minput state-table deltas for the cleaned rows
                    // (netted to DELETE by minput_drain, as apply-path
                    // retractions are)
                    if (t.mkilled) {
                        uint32_t ki = atomicAdd(t.mkilled_cursor, 1u);
                        if (ki < t.mkilled_cap) t.mkilled[ki] = row;
                    }
                    row = ld_u32(&t.mnext[row]);
                }
                t.mheads[(size_t)calls[ci].mord * cap + slot] = UINT32_MAX;
            }
        }
        t.has_prev[(uint32_t)slot] = 0;
        t.dirty_flag[(uint32_t)slot] = 0;
    }
}

// DISTINCT dedup-table state cleaning (the same watermark applies to the
// dedup tables' group-key prefix in the reference): reset counts below
// the watermark and mark the slot dirty so the next dedup drain nets a
// DELETE for persisted rows — and so LATE rows restart visibility
// transitions from 0, as the reference's freshly-deleted state row would.
__global__ void dedup_clean_kernel(JoinSlot* slots, size_t cap, int kpos,
                                   long long wm, uint32_t* dirty_flag,
                                   uint32_t* dirty_list, uint32_t* dirty_n) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        if (slots[slot].state != SLOT_READY) continue;
        if ((slots[slot].nulls >> kpos) & 1) continue;
        if (slots[slot].key[kpos] >= wm) continue;
        if (slots[slot].head == 0) continue; // nothing live to clean
        slots[slot].head = 0;
        if (ld_u32(&dirty_flag[slot]) == 0 &&
            atomicCAS(&dirty_flag[slot], 0u, 1u) == 0u)
            dirty_list[atomicAdd(dirty_n, 1u)] = (uint32_t)slot;
    }
}

// EOWC close (hash_agg.rs:429-474): windows with group-key[0] below the
// watermark emit their FINAL row once (Insert; row_count 0 emits nothing)
// and are reset in place (slot stays READY so linear probing is
// undisturbed; a late row would restart the window). Emission order is
// fixed up host-side (rows sorted by group key, as SortBuffer::consume
// iterates ordered).
// EOWC mid-window state PUTs (hash_agg.rs:429-460): at every barrier the
// dirty groups' CURRENT states upsert into the intermediate table even
// though nothing is emitted until a watermark closes the window. One
// thread per dirty slot; rows carry op=Insert (PUT) and are encoded
// host-side by spill_records (materialized-input states encode None
// there, as in the non-EOWC spill).
__global__ void agg_eowc_dump_kernel(AggTableDev t, int KW, int n_calls,
                                     int row_count_index, AggCallDev c0,
                                     AggCallDev c1, AggCallDev c2,
                                     AggCallDev c3) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    uint32_t n_dirty = t.counters[0];
    uint32_t stride = gridDim.x * blockDim.x;
    size_t cap = (size_t)t.cap_mask + 1;
    int width = KW + n_calls;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_dirty;
         i += stride) {
        uint32_t slot = t.dirty_list[i];
        t.dirty_flag[slot] = 0;
        uint32_t orow = atomicAdd(&t.counters[1], 1u);
        if (orow + 1 > t.out_capacity) {
            atomicExch(&t.counters[2], 2u);
            continue;
        }
        long long rc = t.acc[(size_t)row_count_index * cap + slot];
        if (rc < 0) rc = 0;
        t.out_ops[orow] = RW_OP_INSERT;
        // the window now has a persisted intermediate-table row; the close
        // kernel emits its DELETE marker only for persisted windows (and
        // clears the flag), so re-scanned already-closed slots stay silent
        t.has_prev[slot] = 1;
        for (int k = 0; k < KW; k++) {
            t.out_vals[(size_t)orow * width + k] = t.keys[(size_t)slot * KW + k];
            t.out_nulls[(size_t)orow * width + k] =
                (t.key_nulls[slot] >> k) & 1;
        }
        for (int ci = 0; ci < n_calls; ci++) {
            const AggCallDev& c = calls[ci];
            long long* acc = t.acc + (size_t)ci * cap;
            uint8_t* has = t.has + (size_t)ci * cap;
            if (rc == 0 && !c.minput) {
                // reset value states (agg_state.rs:149-155), as the flush
                // kernel and the oracle's get_outputs do
                switch (c.kind) {
                    case RW_AGG_MIN: acc[slot] = INT64_MAX; break;
                    case RW_AGG_MAX: acc[slot] = INT64_MIN; break;
                    default: acc[slot] = 0;
                }
                has[slot] = 0;
            }
            long long v;
            uint8_t nl;
            if (c.minput) {
                v = 0;
                nl = 1; // spill_records encodes None for minput states
            } else {
                switch (c.kind) {
                    case RW_AGG_COUNT_STAR:
                    case RW_AGG_COUNT:
                    case RW_AGG_SUM0:
                        v = acc[slot];
                        nl = 0;
                        break;
                    default:
                        v = acc[slot];
                        nl = !has[slot];
                }
            }
            t.out_vals[(size_t)orow * width + KW + ci] = v;
            t.out_nulls[(size_t)orow * width + KW + ci] = nl;
        }
    }
}

__global__ void agg_eowc_close_kernel(AggTableDev t, int KW, int n_calls,
                                      int row_count_index, long long wm,
                                      AggCallDev c0, AggCallDev c1,
                                      AggCallDev c2, AggCallDev c3) {
    AggCallDev calls[4] = {c0, c1, c2, c3};
    size_t cap = (size_t)t.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    int width = KW + n_calls;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        if (ld_u32(&t.state[(uint32_t)slot]) != SLOT_READY) continue;
        if ((ld_u32(&t.key_nulls[(uint32_t)slot]) >> 0) & 1) continue;
        if (ld_i64((const int64_t*)&t.keys[slot * KW]) >= wm) continue;
        long long rc = t.acc[(size_t)row_count_index * cap + slot];
        if (rc < 0) rc = 0;
        if (rc > 0) {
            // final outputs (get_outputs, agg_group.rs:431-467)
            long long curr[MAX_CALLS];
            uint8_t curr_null[MAX_CALLS];
            for (int ci = 0; ci < n_calls; ci++) {
                const AggCallDev& c = calls[ci];
                long long* acc = t.acc + (size_t)ci * cap;
                uint8_t* has = t.has + (size_t)ci * cap;
                if (c.minput) {
                    uint32_t row = t.mheads[(size_t)c.mord * cap + slot];
                    bool any = false, any_null = false;
                    long long best = 0;
                    while (row != UINT32_MAX) {
                        if (t.malive[row]) {
                            if (t.mval_null[row]) {
                                any_null = true;
                            } else {
                                long long v = t.mval[row];
                                if (!any) best = v;
                                else if (c.kind == RW_AGG_MIN)
                                    best = v < best ? v : best;
                                else
                                    best = v > best ? v : best;
                                any = true;
                            }
                        }
                        row = t.mnext[row];
                    }
                    if (c.kind == RW_AGG_MAX && any_null) {
                        curr[ci] = 0;
                        curr_null[ci] = 1;
                    } else {
                        curr[ci] = best;
                        curr_null[ci] = !any;
                    }
                    continue;
                }
                switch (c.kind) {
                    case RW_AGG_COUNT_STAR:
                    case RW_AGG_COUNT:
                    case RW_AGG_SUM0:
                        curr[ci] = acc[slot];
                        curr_null[ci] = 0;
                        break;
                    default:
                        curr[ci] = acc[slot];
                        curr_null[ci] = !has[slot];
                }
            }
            uint32_t orow = atomicAdd(&t.counters[1], 1u);
            if (orow + 1 > t.out_capacity) {
                atomicExch(&t.counters[2], 2u);
            } else {
                t.out_ops[orow] = RW_OP_INSERT;
                for (int k = 0; k < KW; k++) {
                    t.out_vals[(size_t)orow * width + k] =
                        t.keys[slot * KW + k];
                    t.out_nulls[(size_t)orow * width + k] =
                        (t.key_nulls[(uint32_t)slot] >> k) & 1;
                }
                for (int ci = 0; ci < n_calls; ci++) {
                    t.out_vals[(size_t)orow * width + KW + ci] = curr[ci];
                    t.out_nulls[(size_t)orow * width + KW + ci] = curr_null[ci];
                }
            }
        } else if (t.has_prev[(uint32_t)slot]) {
            // closed window with row_count 0 but a persisted row: nothing
            // is emitted (OnlyOutputIfHasInput) but the reference still
            // deletes its intermediate-table row — a DELETE-marker row,
            // spilled but filtered out of emission host-side. Slots with
            // no persisted row (already-closed residue) stay silent.
            uint32_t orow = atomicAdd(&t.counters[1], 1u);
            if (orow + 1 > t.out_capacity) {
                atomicExch(&t.counters[2], 2u);
            } else {
                t.out_ops[orow] = RW_OP_DELETE;
                for (int k = 0; k < KW; k++) {
                    t.out_vals[(size_t)orow * width + k] =
                        t.keys[slot * KW + k];
                    t.out_nulls[(size_t)orow * width + k] =
                        (t.key_nulls[(uint32_t)slot] >> k) & 1;
                }
                for (int ci = 0; ci < n_calls; ci++) {
                    t.out_vals[(size_t)orow * width + KW + ci] = 0;
                    t.out_nulls[(size_t)orow * width + KW + ci] = 1;
                }
            }
        }
        // reset the window in place (as agg_clean_kernel does)
        for (int ci = 0; ci < n_calls; ci++) {
            long long init = 0;
            if (calls[ci].kind == RW_AGG_MIN) init = INT64_MAX;
            if (calls[ci].kind == RW_AGG_MAX) init = INT64_MIN;
            t.acc[(size_t)ci * cap + slot] = init;
            t.has[(size_t)ci * cap + slot] = 0;
            if (calls[ci].minput) {
                uint32_t row = t.mheads[(size_t)calls[ci].mord * cap + slot];
                while (row != UINT32_MAX) {
                    st_u32(&t.malive[row], 0);
                    row = ld_u32(&t.mnext[row]);
                }
                t.mheads[(size_t)calls[ci].mord * cap + slot] = UINT32_MAX;
            }
        }
        t.has_prev[(uint32_t)slot] = 0;
        t.dirty_flag[(uint32_t)slot] = 0;
    }
}

// Rescale re-scoping (update_vnode_bitmap, state_table.rs + executor cache
// eviction): state whose distribution-key vnode is no longer owned is
// dropped WITHOUT emitting retractions — the new owner holds it. Dist key =
// group key (agg) / join key (join). CRC feed identical to vnode_kernel.
__device__ __forceinline__ uint32_t crc_key_words(const uint32_t* lut,
                                                  const int64_t* kw,
                                                  uint32_t nulls, int KW,
                                                  const uint8_t* types) {
    uint32_t crc = 0xFFFFFFFFu;
    for (int k = 0; k < KW; k++) {
        if ((nulls >> k) & 1) {
            uint32_t sentinel = 0xfffffff0u;
            crc = crc32_bytes(lut, crc, (const uint8_t*)&sentinel, 4);
        } else if (types[k] == RW_T_I32) {
            int32_t v = (int32_t)kw[k];
            crc = crc32_bytes(lut, crc, (const uint8_t*)&v, 4);
        } else if (types[k] == RW_T_BOOL) {
            uint8_t v = (uint8_t)kw[k];
            crc = crc32_bytes(lut, crc, &v, 1);
        } else {
            int64_t v = kw[k];
            crc = crc32_bytes(lut, crc, (const uint8_t*)&v, 8);
        }
    }
    return crc ^ 0xFFFFFFFFu;
}

__global__ void agg_vnode_scope_kernel(AggTableDev t, int KW, int n_calls,
                                       AggCallDev c0, AggCallDev c1,
                                       AggCallDev c2, AggCallDev c3,
                                       const uint8_t* bitmap,
                                       uint32_t vnode_count, uint8_t t0,
                                       uint8_t t1, uint8_t t2, uint8_t t3) {
    __shared__ uint32_t lut[256];
    stage_crc_lut(lut);
    AggCallDev calls[4] = {c0, c1, c2, c3};
    uint8_t types[4] = {t0, t1, t2, t3};
    size_t cap = (size_t)t.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        if (ld_u32(&t.state[(uint32_t)slot]) != SLOT_READY) continue;
        uint32_t vn = crc_key_words(lut, &t.keys[slot * KW],
                                    ld_u32(&t.key_nulls[(uint32_t)slot]), KW,
                                    types) %
                      vnode_count;
        if ((bitmap[vn >> 3] >> (vn & 7)) & 1) continue; // still owned
        for (int ci = 0; ci < n_calls; ci++) {
            long long init = 0;
            if (calls[ci].kind == RW_AGG_MIN) init = INT64_MAX;
            if (calls[ci].kind == RW_AGG_MAX) init = INT64_MIN;
            t.acc[(size_t)ci * cap + slot] = init;
            t.has[(size_t)ci * cap + slot] = 0;
            if (calls[ci].minput) {
                uint32_t row = t.mheads[(size_t)calls[ci].mord * cap + slot];
                while (row != UINT32_MAX) {
                    st_u32(&t.malive[row], 0);
                    row = ld_u32(&t.mnext[row]);
                }
                t.mheads[(size_t)calls[ci].mord * cap + slot] = UINT32_MAX;
            }
        }
        t.has_prev[(uint32_t)slot] = 0;
        t.dirty_flag[(uint32_t)slot] = 0;
    }
}

__global__ void join_vnode_scope_kernel(JoinSideDev sd, int KW,
                                        const uint8_t* bitmap,
                                        uint32_t vnode_count, uint8_t t0,
                                        uint8_t t1, uint8_t t2, uint8_t t3,
                                        uint8_t k0, uint8_t k1, uint8_t k2,
                                        uint8_t k3) {
    __shared__ uint32_t lut[256];
    stage_crc_lut(lut);
    uint8_t types[4] = {t0, t1, t2, t3};
    uint8_t kcols[4] = {k0, k1, k2, k3};
    size_t cap = (size_t)sd.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        uint64_t packed = __hip_atomic_load(&sd.slots8[slot], RLX);
        if ((uint32_t)packed == 0) continue; // bloom 0 = empty
        uint32_t row = jhead_of(packed);
        while (row != UINT32_MAX) { // buckets mix keys: vnode PER RECORD
            JoinRowHdr* h = jrow(sd, row);
            if (ld_u32(&h->alive)) {
                uint32_t vb = ld_u32(&h->validbits);
                const long long* hv = jvals(h);
                int64_t kw[4];
                uint32_t nulls = 0;
                for (int k = 0; k < KW; k++) {
                    bool valid = (vb >> kcols[k]) & 1;
                    kw[k] = valid ? ld_i64((const int64_t*)&hv[kcols[k]]) : 0;
                    nulls |= (uint32_t)(!valid) << k;
                }
                uint32_t vn =
                    crc_key_words(lut, kw, nulls, KW, types) % vnode_count;
                if (!((bitmap[vn >> 3] >> (vn & 7)) & 1))
                    st_u32(&h->alive, 0);
            }
            row = ld_u32(&h->next);
        }
    }
}

// ============ varchar payload columns ============
//
// A varchar cell is an 8-byte reference word (rw_varlen.hpp) into its
// side's byte arena, so the probe kernels above move it like an i64. The
// kernels here are everything that has to look THROUGH a word: resolving
// retractions by string content, materialising strings for emit / drain,
// and rebuilding the arena at compaction.

// (VarlenView and the VarlenFetch materialiser both executors share are
// declared ahead of HashAgg.)

__device__ __forceinline__ uint64_t varlen_view_word(const VarlenView& v,
                                                     uint32_t i) {
    if (v.ops && i < v.sparse_n && v.ops[i] == 0xFF) return 0;
    if (v.nulls && v.nulls[i]) return 0;
    return v.words[(size_t)i * v.stride];
}

// lens[i] = byte length of cell i for i < n; lens[n] = 0 so an exclusive
// scan over n + 1 entries leaves the total at offs[n]
__global__ void varlen_len_kernel(VarlenView v, uint32_t n, uint64_t* lens) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n;
         i += stride)
        lens[i] = i < n ? rwvarlen::word_len(varlen_view_word(v, i)) : 0;
}

// OUTPUT-CENTRIC copy: each lane owns one aligned W-byte unit (a dword or
// 16 bytes) of the packed buffer, finds the string holding its first byte
// by binary search over the scanned offsets (the search's top levels hit
// the same few lines for every lane of a wave), gathers its <= W source
// bytes (they may span several short strings) and stores the unit
// coalesced. `out` holds (total + W - 1) / W whole units.
template <int W>
__global__ __launch_bounds__(256) void varlen_copy_out_kernel(
    VarlenView v, const uint8_t* __restrict__ arena,
    const uint64_t* __restrict__ offs, uint32_t n, uint64_t total,
    uint8_t* __restrict__ out) {
    static_assert(W == 4 || W == 16, "unit is a dword or four");
    uint64_t units = (total + W - 1) / W;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         t < units; t += stride) {
        uint64_t p = t * W;
        // largest i with offs[i] <= p; offs[0] = 0 <= p < total = offs[n],
        // so offs[i + 1] > p: string i is non-empty and holds byte p
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            uint32_t mid = lo + (hi - lo) / 2;
            if (offs[mid] <= p) lo = mid;
            else hi = mid;
        }
        uint32_t i = lo;
        uint64_t beg = offs[i], end = offs[i + 1];
        const uint8_t* src = arena + rwvarlen::word_off(varlen_view_word(v, i));
        uint32_t dw[W / 4] = {};
#pragma unroll
        for (int k = 0; k < W; k++) {
            uint64_t q = p + k;
            if (q < total) {
                while (q >= end) { // q < offs[n]: i + 1 <= n stays in range
                    i++;
                    beg = end;
                    end = offs[i + 1];
                    src = arena +
                          rwvarlen::word_off(varlen_view_word(v, i));
                }
                dw[k >> 2] |= (uint32_t)src[q - beg] << (8 * (k & 3));
            }
        }
        if (W == 4)
            ((uint32_t*)out)[t] = dw[0];
        else
            ((uint4*)out)[t] = make_uint4(dw[0], dw[W / 4 > 1 ? 1 : 0],
                                          dw[W / 4 > 2 ? 2 : 0],
                                          dw[W / 4 > 3 ? 3 : 0]);
    }
}

// the obvious form, and the one in use: one string per lane, byte loop.
// Neighbouring lanes write neighbouring short strings, so the stores of a
// wave still land in a few adjacent lines.
__global__ __launch_bounds__(256) void varlen_copy_lane_kernel(
    VarlenView v, const uint8_t* __restrict__ arena,
    const uint64_t* __restrict__ offs, uint32_t n,
    uint8_t* __restrict__ out) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        uint64_t w = varlen_view_word(v, i);
        uint32_t len = rwvarlen::word_len(w);
        const uint8_t* src = arena + rwvarlen::word_off(w);
        uint8_t* dst = out + offs[i];
        for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
    }
}

// bytes the copy may store past `total`: out buffers are padded to this
#define VARLEN_COPY_PAD 16

static void varlen_copy_launch(const VarlenView& v, const uint8_t* arena,
                               const uint64_t* offs, uint32_t n,
                               uint64_t total, uint8_t* out,
                               hipStream_t stream) {
    // Default = the measured winner on the q8 emit shape:
    // the per-string lane loop, 72 us per 1M names of 8-32 bytes, against
    // 135 us (dword units) and 240 us (16-byte units) for the
    // output-centric form, whose serial per-lane walk across string
    // boundaries costs more than its coalesced stores save.
    // RW_VARLEN_COPY=dword|b16 selects those for the A/B in
    // tests/bench_varchar_emit.py.
    const char* e = getenv("RW_VARLEN_COPY");
    const bool out_centric = e && (!strcmp(e, "dword") || !strcmp(e, "b16"));
    if (!out_centric) {
        uint32_t blocks = (n + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        varlen_copy_lane_kernel<<<blocks, 256, 0, stream>>>(v, arena, offs, n,
                                                            out);
        return;
    }
    const int W = !strcmp(e, "dword") ? 4 : 16;
    uint64_t units = (total + W - 1) / W;
    uint64_t blocks = (units + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (W == 4)
        varlen_copy_out_kernel<4><<<(uint32_t)blocks, 256, 0, stream>>>(
            v, arena, offs, n, total, out);
    else
        varlen_copy_out_kernel<16><<<(uint32_t)blocks, 256, 0, stream>>>(
            v, arena, offs, n, total, out);
}

// Retraction pre-pass (cold path; runs before a probe launch whose range
// holds delete rows, only for sides with varchar columns). jown_delete
// matches a delete row against the stored record by 8-byte word compare,
// but the delete row's string was appended at a different arena offset
// than the stored one. For each delete row this kernel walks the own-side
// bucket chain for the live record that equals the row on every
// fixed-width column (a superset of join key ∥ pk) and, by arena BYTES, on
// every varchar column; on a hit it rewrites the batch row's varchar
// word(s) to the stored record's, after which the probe kernel's compare
// works unchanged. ASSUMPTION: a side's live rows are unique by pk (the
// reference's JoinRowSet is keyed by pk), so at most one record qualifies;
// with duplicate live rows two same-launch deletes could resolve to the
// same record. No hit leaves the words alone: the delete then finds
// nothing, exactly like a non-matching i64 delete. The own side is not
// mutated during this launch, so plain loads suffice.
__global__ void join_varlen_resolve_kernel(JoinBatchDev b, JoinSideDev own,
                                           JoinMeta m, int S, uint32_t r0,
                                           uint32_t r1) {
    uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t vcm = m.vc_mask[S];
    for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1;
         r += stride) {
        if (b.vis && !b.vis[r]) continue;
        uint8_t op = b.ops[r];
        if (op == RW_OP_INSERT || op == RW_OP_UPDATE_INSERT) continue;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.key_cols[S][i];
            bool valid = b.col_valid[col][r];
            kw[i] = valid ? b.col_vals[col][r] : 0;
            nullmask |= (!valid) << i;
        }
        if (nullmask & ~(uint32_t)m.null_safe_mask) continue; // never stored
        uint32_t row = jbucket_head(own, hash_key(kw, nullmask, m.KW), false);
        while (row != UINT32_MAX) {
            JoinRowHdr* h = jrow(own, row);
            if (h->alive) {
                uint32_t vb = h->validbits;
                const long long* hv = jvals(h);
                bool eq = true;
                for (int c = 0; eq && c < m.n_cols[S]; c++) {
                    bool va = b.col_valid[c][r] != 0;
                    if (va != (bool)((vb >> c) & 1)) {
                        eq = false;
                    } else if (va && !((vcm >> c) & 1)) {
                        eq = b.col_vals[c][r] == hv[c];
                    } else if (va) {
                        uint64_t wa = (uint64_t)b.col_vals[c][r];
                        uint64_t wr = (uint64_t)hv[c];
                        uint32_t len = rwvarlen::word_len(wa);
                        if (len != rwvarlen::word_len(wr)) {
                            eq = false;
                        } else if (wa != wr) {
                            const uint8_t* pa =
                                own.arena + rwvarlen::word_off(wa);
                            const uint8_t* pr =
                                own.arena + rwvarlen::word_off(wr);
                            for (uint32_t k = 0; eq && k < len; k++)
                                eq = pa[k] == pr[k];
                        }
                    }
                }
                if (eq) {
                    for (int c = 0; c < m.n_cols[S]; c++)
                        if (((vcm >> c) & 1) && ((vb >> c) & 1))
                            b.col_vals[c][r] = hv[c];
                    break;
                }
            }
            row = h->next;
        }
    }
}

// compaction: point every live record's varchar word at its string's new
// home (new_base + offs[i]); NULL cells keep word 0
__global__ void varlen_rewrite_kernel(JoinSideDev sd, int col, uint32_t n,
                                      const uint64_t* offs,
                                      uint64_t new_base) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        JoinRowHdr* h = jrow(sd, i);
        long long* hv = jvals(h);
        bool valid = (h->validbits >> col) & 1;
        hv[col] = valid ? (long long)rwvarlen::pack(
                              new_base + offs[i],
                              rwvarlen::word_len((uint64_t)hv[col]))
                        : 0;
    }
}

int VarlenFetch::ensure_scan_tmp(size_t tmp) {
    if (tmp <= d_scan_tmp_cap) return RW_OK;
    d_scan_tmp_cap = 0;
    HIP_TRY(mem.regrow(&d_scan_tmp, tmp));
    d_scan_tmp_cap = tmp;
    return RW_OK;
}

int VarlenFetch::ensure_vscratch(uint32_t n) {
    if (d_vcap >= n + 1) return RW_OK;
    mem.release(&d_vlens);
    mem.release(&d_voffs);
    d_vcap = 0;
    uint32_t cap = 4096;
    while (cap < n + 1) cap <<= 1;
    HIP_TRY(mem.alloc(&d_vlens, (size_t)cap * 8));
    HIP_TRY(mem.alloc(&d_voffs, (size_t)cap * 8));
    d_vcap = cap;
    return RW_OK;
}

// Materialise the strings a view's words reference into ONE packed
// host byte buffer: length kernel -> exclusive scan -> copy kernel ->
// D2H. offs gets n + 1 entries (offs[n] = total bytes).
int VarlenFetch::fetch(const VarlenView& v, const uint8_t* arena, uint32_t n,
                       std::vector<uint64_t>& offs,
                       std::vector<uint8_t>& bytes, bool timed,
                       hipStream_t stream) {
    offs.assign((size_t)n + 1, 0);
    bytes.clear();
    if (!n) return RW_OK;
    int rc = ensure_vscratch(n);
    if (rc != RW_OK) return rc;
    if (timed && !vev0) {
        HIP_TRY(hipEventCreate(&vev0));
        HIP_TRY(hipEventCreate(&vev1));
        HIP_TRY(hipEventCreate(&vev2));
    }
    if (timed) HIP_TRY(hipEventRecord(vev0, stream));
    uint32_t blocks = (n + 1 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    varlen_len_kernel<<<blocks, 256, 0, stream>>>(v, n, d_vlens);
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, d_vlens, d_voffs,
                                    (uint64_t)0, (size_t)n + 1,
                                    rocprim::plus<uint64_t>(), stream));
    rc = ensure_scan_tmp(tmp);
    if (rc != RW_OK) return rc;
    HIP_TRY(rocprim::exclusive_scan(d_scan_tmp, tmp, d_vlens, d_voffs,
                                    (uint64_t)0, (size_t)n + 1,
                                    rocprim::plus<uint64_t>(), stream));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_voffs + n, 8, hipMemcpyDeviceToHost,
                           stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total) {
        uint64_t padded = total + VARLEN_COPY_PAD; // whole copy units
        if (d_vbytes_cap < padded) {
            d_vbytes_cap = 0;
            uint64_t cap = 1ull << 16;
            while (cap < padded) cap <<= 1;
            HIP_TRY(mem.regrow(&d_vbytes, cap));
            d_vbytes_cap = cap;
        }
        if (timed) HIP_TRY(hipEventRecord(vev2, stream));
        varlen_copy_launch(v, arena, d_voffs, n, total, d_vbytes, stream);
    }
    if (timed) {
        HIP_TRY(hipEventRecord(vev1, stream));
        HIP_TRY(hipEventSynchronize(vev1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, vev0, vev1));
        vemit_ms += ms;
        if (total) {
            HIP_TRY(hipEventElapsedTime(&ms, vev2, vev1));
            vcopy_ms += ms;
        }
        vemit_bytes += total;
        vemit_launches++;
    }
    HIP_TRY(hipMemcpy(offs.data(), d_voffs, ((size_t)n + 1) * 8,
                      hipMemcpyDeviceToHost));
    bytes.resize(total);
    if (total)
        HIP_TRY(hipMemcpy(bytes.data(), d_vbytes, total,
                          hipMemcpyDeviceToHost));
    return RW_OK;
}

VarlenFetch::~VarlenFetch() {
    if (vev0) {
        hipEventDestroy(vev0);
        hipEventDestroy(vev1);
        if (vev2) hipEventDestroy(vev2);
    }
}

struct HashJoin {
    RwHashJoinDesc desc;
    JoinMeta m{};
    JoinSideDev side[2]{};
    JoinOutDev out{};
    hipStream_t stream = nullptr;
    DevOwner mem; // every device buffer of this executor (rw_devmem.hpp)
    std::vector<uint8_t> out_types;
    std::vector<uint8_t> types[2];
    // staging
    JoinBatchDev stage[2]{};
    uint32_t stage_cap[2] = {0, 0};
    rwchunk::ChunkQueue outq;
    uint8_t* zeros = nullptr; // all-zero null flags for pipeline dummy cols
    uint8_t* d_vnode_bitmap = nullptr; // rescale scope (update_vnode_bitmap)
    uint16_t* d_vnode_hop = nullptr;   // q7-pipeline exchange-hop vnodes
    uint32_t d_vnode_hop_cap = 0;
    // join-key watermark buffering (hash_join.rs:826-867)
    struct Wm { bool has = false; int64_t val = 0; };
    std::vector<uint32_t> wm_pos;
    std::vector<uint8_t> wm_clean;
    std::vector<Wm> wm_side0, wm_side1, wm_out;
    // inequality-pair watermarks (hash_join.rs:869-914): buffered per
    // pair; the min across sides emits for the LARGER side's output
    // columns and (clean flag) sweeps that side's rows by the pair's
    // value column
    std::vector<uint32_t> ineq_col[2]; // [pair] per side
    std::vector<uint8_t> ineq_larger, ineq_do_clean;
    std::vector<Wm> ineq_wm[2], ineq_out;
    // lazy event ring (same rationale as HashAgg: no per-step host sync)
    EventRing ring; // ring.ms_total: probe kernel time
    uint64_t probe_launches = 0, probe_rows = 0;

    int init(const RwHashJoinDesc* d) {
        if (!gpu_ok()) FAIL(RW_E_NOGPU, "risingwave_amd: no GPU visible (product path has no CPU fallback)");
        desc = *d;
        if (d->join_type > RW_JOIN_RIGHT_ANTI)
            FAIL(RW_E_INVAL, "unknown join type %d", d->join_type);
        if (d->append_only && d->join_type != RW_JOIN_INNER)
            FAIL(RW_E_INVAL, "append-only optimize kernel is inner-only this round");
        if (d->n_key < 1 || d->n_key > MAX_KW) FAIL(RW_E_INVAL, "n_key %u", d->n_key);
        if (d->n_cols_l > MAX_COLS || d->n_cols_r > MAX_COLS)
            FAIL(RW_E_INVAL, "too many columns for round-1 kernels");
        if (d->n_output > MAX_OUT) FAIL(RW_E_INVAL, "too many output columns");
        m.KW = (int)d->n_key;
        m.n_cols[0] = (int)d->n_cols_l;
        m.n_cols[1] = (int)d->n_cols_r;
        m.n_pk[0] = (int)d->n_pk_l;
        m.n_pk[1] = (int)d->n_pk_r;
        types[0].assign(d->types_l, d->types_l + d->n_cols_l);
        types[1].assign(d->types_r, d->types_r + d->n_cols_r);
        for (int s = 0; s < 2; s++)
            for (size_t c = 0; c < types[s].size(); c++) {
                uint8_t t = types[s][c];
                if (t == RW_T_VARCHAR)
                    m.vc_mask[s] |= (uint8_t)(1u << c);
                else if (t != RW_T_I64 && t != RW_T_TS)
                    FAIL(RW_E_INVAL, "column type %d unsupported on GPU "
                                     "(i64/ts, varchar payload only)", t);
            }
        // varchar is a PAYLOAD type: every column the kernels compare or
        // hash as an 8-byte scalar must be fixed width (rw_stream.h)
        {
            const char* sn[2] = {"left", "right"};
            auto is_vc = [&](int s, uint32_t col) {
                return col < types[s].size() && types[s][col] == RW_T_VARCHAR;
            };
            auto is_vc_cat = [&](uint32_t idx) {
                return idx < d->n_cols_l ? is_vc(0, idx)
                                         : is_vc(1, idx - d->n_cols_l);
            };
            for (uint32_t i = 0; i < d->n_key; i++) {
                if (is_vc(0, d->key_l[i]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be a join key",
                         sn[0], d->key_l[i]);
                if (is_vc(1, d->key_r[i]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be a join key",
                         sn[1], d->key_r[i]);
            }
            for (uint32_t i = 0; i < d->n_pk_l; i++)
                if (is_vc(0, d->pk_l[i]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be a pk column",
                         sn[0], d->pk_l[i]);
            for (uint32_t i = 0; i < d->n_pk_r; i++)
                if (is_vc(1, d->pk_r[i]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be a pk column",
                         sn[1], d->pk_r[i]);
            if (d->has_cond && (is_vc_cat(d->cond_l) || is_vc_cat(d->cond_r)))
                FAIL(RW_E_INVAL, "varchar column %u cannot be a condition operand",
                     is_vc_cat(d->cond_l) ? d->cond_l : d->cond_r);
            if (d->has_cond && d->has_cond2 &&
                (is_vc_cat(d->cond2_l) || is_vc_cat(d->cond2_r)))
                FAIL(RW_E_INVAL, "varchar column %u cannot be a condition operand",
                     is_vc_cat(d->cond2_l) ? d->cond2_l : d->cond2_r);
            for (uint32_t p = 0; p < d->n_ineq; p++) {
                if (is_vc(0, d->ineq_left_col[p]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be an "
                                     "inequality/watermark column",
                         sn[0], d->ineq_left_col[p]);
                if (is_vc(1, d->ineq_right_col[p]))
                    FAIL(RW_E_INVAL, "varchar %s column %u cannot be an "
                                     "inequality/watermark column",
                         sn[1], d->ineq_right_col[p]);
            }
        }
        for (uint32_t i = 0; i < d->n_key; i++) {
            m.key_cols[0][i] = (uint8_t)d->key_l[i];
            m.key_cols[1][i] = (uint8_t)d->key_r[i];
            if (d->null_safe[i]) m.null_safe_mask |= 1 << i;
        }
        if (d->n_pk_l > MAX_KW || d->n_pk_r > MAX_KW) FAIL(RW_E_INVAL, "pk too wide");
        for (uint32_t i = 0; i < d->n_pk_l; i++) m.pk_cols[0][i] = (uint8_t)d->pk_l[i];
        for (uint32_t i = 0; i < d->n_pk_r; i++) m.pk_cols[1][i] = (uint8_t)d->pk_r[i];
        m.n_out = (int)d->n_output;
        for (uint32_t i = 0; i < d->n_output; i++) {
            uint32_t idx = d->output_indices[i];
            if (idx < d->n_cols_l) {
                m.out_src[i] = 0;
                m.out_col[i] = (uint8_t)idx;
                out_types.push_back(types[0][idx]);
            } else {
                m.out_src[i] = 1;
                m.out_col[i] = (uint8_t)(idx - d->n_cols_l);
                out_types.push_back(types[1][idx - d->n_cols_l]);
            }
        }
        auto split = [&](uint32_t idx, uint8_t* src, uint8_t* col) {
            if (idx < d->n_cols_l) {
                *src = 0;
                *col = (uint8_t)idx;
            } else {
                *src = 1;
                *col = (uint8_t)(idx - d->n_cols_l);
            }
        };
        m.n_cond = 0;
        if (d->has_cond) {
            m.cond[0].op = d->cond_op;
            split(d->cond_l, &m.cond[0].src_l, &m.cond[0].col_l);
            split(d->cond_r, &m.cond[0].src_r, &m.cond[0].col_r);
            m.cond[0].rconst = d->cond_rconst;
            m.n_cond = 1;
            if (d->has_cond2) {
                m.cond[1].op = d->cond2_op;
                split(d->cond2_l, &m.cond[1].src_l, &m.cond[1].col_l);
                split(d->cond2_r, &m.cond[1].src_r, &m.cond[1].col_r);
                m.cond[1].rconst = d->cond2_rconst;
                m.n_cond = 2;
            }
        }
        m.append_only = d->append_only;
        m.join_type = d->join_type;
        m.need_deg[0] = j_need_degree(d->join_type, RW_SIDE_LEFT);
        m.need_deg[1] = j_need_degree(d->join_type, RW_SIDE_RIGHT);
        if (d->n_wm_jk) {
            wm_pos.assign(d->wm_jk_pos, d->wm_jk_pos + d->n_wm_jk);
            wm_clean.assign(d->wm_jk_clean, d->wm_jk_clean + d->n_wm_jk);
        }
        wm_side0.resize(d->n_key);
        wm_side1.resize(d->n_key);
        wm_out.resize(d->n_key);
        if (d->n_ineq) {
            ineq_col[0].assign(d->ineq_left_col,
                               d->ineq_left_col + d->n_ineq);
            ineq_col[1].assign(d->ineq_right_col,
                               d->ineq_right_col + d->n_ineq);
            ineq_larger.assign(d->ineq_left_larger,
                               d->ineq_left_larger + d->n_ineq);
            ineq_do_clean.assign(d->ineq_clean, d->ineq_clean + d->n_ineq);
            ineq_wm[0].resize(d->n_ineq);
            ineq_wm[1].resize(d->n_ineq);
            ineq_out.resize(d->n_ineq);
        }

        HIP_TRY(hipStreamCreate(&stream));
        uint64_t key_cap = d->state_capacity_hint ? d->state_capacity_hint : (1u << 20);
        uint64_t row_cap = d->row_capacity_hint ? d->row_capacity_hint : (1u << 22);
        for (int s = 0; s < 2; s++) {
            uint32_t cap = 1;
            while (cap < key_cap * 2) cap <<= 1; // ≤50% load factor
            JoinSideDev& js = side[s];
            js.cap_mask = cap - 1;
            js.slots = nullptr; // join tables use compact 8-B slots
            HIP_TRY(mem.alloc(&js.slots8, (size_t)cap * 8));
            HIP_TRY(hipMemsetAsync(js.slots8, 0, (size_t)cap * 8, stream));
            js.row_cap = (uint32_t)row_cap;
            uint32_t rs = 16 + 8 * (uint32_t)m.n_cols[s];
            // line-align records: a stride of 16/32/64 never straddles a
            // 64-B line, so the random record reads of probe/verify fetch
            // exactly ONE line (a 48-B stride fetched ~1.5 lines/record)
            if (rs > 32 && rs <= 64) rs = 64;
            else if (rs > 64) rs = (rs + 31) & ~31u;
            js.row_stride = rs;
            HIP_TRY(mem.alloc(&js.rows, (size_t)row_cap * js.row_stride));
            HIP_TRY(mem.alloc(&js.row_cursor, 4));
            HIP_TRY(hipMemset(js.row_cursor, 0, 4));
            // checkpoint-delta tracking (§8f-2)
            js.killed_cap = 1u << 22;
            HIP_TRY(mem.alloc(&js.killed, (size_t)js.killed_cap * 4));
            HIP_TRY(mem.alloc(&js.killed_cursor, 4));
            HIP_TRY(hipMemset(js.killed_cursor, 0, 4));
            js.deg_dirty_flag = nullptr;
            js.deg_dirty_list = nullptr;
            js.deg_dirty_n = nullptr;
            if (m.need_deg[s]) {
                HIP_TRY(mem.alloc(&js.deg_dirty_flag, (size_t)row_cap * 4));
                HIP_TRY(hipMemset(js.deg_dirty_flag, 0, (size_t)row_cap * 4));
                HIP_TRY(mem.alloc(&js.deg_dirty_list, (size_t)row_cap * 4));
                HIP_TRY(mem.alloc(&js.deg_dirty_n, 4));
                HIP_TRY(hipMemset(js.deg_dirty_n, 0, 4));
            }
        }
        HIP_TRY(hipStreamSynchronize(stream));
        out.cap = 1u << 22;
        HIP_TRY(mem.alloc(&out.vals, (size_t)out.cap * m.n_out * 8));
        HIP_TRY(mem.alloc(&out.nulls, (size_t)out.cap * m.n_out));
        HIP_TRY(mem.alloc(&out.ops, out.cap));
        HIP_TRY(mem.alloc(&out.counters, 8));
        HIP_TRY(hipMemset(out.counters, 0, 8));
        return RW_OK;
    }

    int ensure_stage(int s, uint32_t n) {
        if (stage_cap[s] >= n) return RW_OK;
        stage_cap[s] = 0;
        uint32_t cap = 4096;
        while (cap < n) cap <<= 1;
        int rc = stage_regrow(mem, stage[s], m.n_cols[s], cap, 8);
        if (rc != RW_OK) return rc;
        stage_cap[s] = cap;
        return RW_OK;
    }

    // ----- varchar payload columns: per-side byte arena -----
    static constexpr uint64_t ARENA_DEFAULT = 1ull << 20;
    uint64_t arena_used[2] = {0, 0};
    uint64_t arena_cap[2] = {0, 0};     // allocated bytes
    uint64_t arena_reserve[2] = {0, 0}; // requested initial capacity
    bool seen_input = false;            // any push or restore happened
    // host staging of a batch's reference words; lives until the next
    // upload so the async H2D copy never outlives its source
    std::vector<int64_t> vwords[2][MAX_COLS];
    // emit-path materialisation scratch + stats (shared with HashAgg)
    VarlenFetch vf;

    bool has_varchar() const { return (m.vc_mask[0] | m.vc_mask[1]) != 0; }

    // make room for `extra` more bytes: reallocate + D2D copy between
    // launches (words are offsets, so none is rewritten)
    int arena_ensure(int s, uint64_t extra) {
        uint64_t need = arena_used[s] + extra;
        if (need > rwvarlen::MAX_OFF)
            FAIL(RW_E_INVAL, "varchar arena would exceed 2^40-1 bytes");
        if (side[s].arena && need <= arena_cap[s]) return RW_OK;
        uint64_t cap = arena_cap[s] ? arena_cap[s]
                       : arena_reserve[s] ? arena_reserve[s] : ARENA_DEFAULT;
        while (cap < need) cap *= 2;
        // in-flight launches may still read the old buffer
        if (side[s].arena) HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(mem.regrow(&side[s].arena, cap, arena_used[s]));
        arena_cap[s] = cap;
        return RW_OK;
    }

    int ensure_vscratch(uint32_t n) { return vf.ensure_vscratch(n); }
    int varlen_fetch(const VarlenView& v, const uint8_t* arena, uint32_t n,
                     std::vector<uint64_t>& offs, std::vector<uint8_t>& bytes,
                     bool timed) {
        return vf.fetch(v, arena, n, offs, bytes, timed, stream);
    }

    int upload(int s, const RwChunk* c, JoinBatchDev* bout) {
        uint32_t n = c->n_rows;
        // varchar columns: validate every offsets array BEFORE any copy
        for (int ci = 0; m.vc_mask[s] && ci < m.n_cols[s]; ci++) {
            if (!((m.vc_mask[s] >> ci) & 1)) continue;
            if (c->cols[ci].type != RW_T_VARCHAR)
                FAIL(RW_E_INVAL, "column %d: expected a varchar column", ci);
            if (const char* why = rwvarlen::check_column(c->cols[ci], n))
                FAIL(RW_E_INVAL, "varchar column %d: %s", ci, why);
        }
        seen_input = true;
        int rc = ensure_stage(s, n);
        if (rc != RW_OK) return rc;
        JoinBatchDev b = stage[s];
        for (int ci = 0; ci < m.n_cols[s]; ci++) {
            const void* vals = c->cols[ci].data;
            if ((m.vc_mask[s] >> ci) & 1) {
                // append the chunk's bytes at the arena tail (one H2D copy)
                // and stage reference words where i64 values go
                auto* vd = (const RwVarlenData*)c->cols[ci].data;
                uint64_t total = n ? vd->offsets[n] : 0;
                rc = arena_ensure(s, total);
                if (rc != RW_OK) return rc;
                uint64_t base = arena_used[s];
                if (total)
                    HIP_TRY(hipMemcpyAsync(side[s].arena + base, vd->bytes,
                                           total, hipMemcpyHostToDevice,
                                           stream));
                arena_used[s] += total;
                rwvarlen::ref_words(vd, c->cols[ci].valid, n, base, 0,
                                    vwords[s][ci]);
                vals = vwords[s][ci].data();
            }
            rc = upload_col(b.col_vals[ci], b.col_valid[ci], vals,
                            c->cols[ci].valid, n, 8, stream);
            if (rc != RW_OK) return rc;
        }
        rc = upload_ops_vis(b, c, stream);
        if (rc != RW_OK) return rc;
        b.all_insert = 1;
        for (uint32_t r = 0; r < n && b.all_insert; r++)
            if (!(c->vis && !c->vis[r]) && c->ops[r] != RW_OP_INSERT &&
                c->ops[r] != RW_OP_UPDATE_INSERT)
                b.all_insert = 0;
        b.no_insert = !b.all_insert;
        for (uint32_t r = 0; r < n && b.no_insert; r++)
            if (!(c->vis && !c->vis[r]) && (c->ops[r] == RW_OP_INSERT ||
                                            c->ops[r] == RW_OP_UPDATE_INSERT))
                b.no_insert = 0;
        b.all_valid = 1;
        for (int ci = 0; ci < m.n_cols[s] && b.all_valid; ci++)
            for (uint32_t r = 0; r < n && b.all_valid; r++)
                b.all_valid = c->cols[ci].valid[r];
        // chained buckets need no uniqueness pre-pass (round-1's plain
        // head-push lever is gone: inserts are single-CAS regardless)
        b.unique_keys = 0;
        *bout = b;
        return RW_OK;
    }

    // inner-probe pre-assigned layout bookkeeping (see jprobe_setup_kernel)
    uint32_t* d_probe_base = nullptr; // the batch's reserved record base
    unsigned long long* d_emit_count = nullptr;
    uint8_t* d_vis_scratch = nullptr;
    uint32_t d_vis_cap = 0;
    uint32_t last_sparse_rows = 0;
    bool sparse_out = false;

    int probe(int s, const JoinBatchDev& b, bool timed, uint32_t r0, uint32_t r1) {
        uint32_t blocks = (r1 - r0 + 255) / 256;
        // one row per lane up to 16K blocks: a grid-stride iteration
        // serializes its dependent walk behind the previous row's, while
        // fresh blocks give the scheduler independent work as waves
        // retire (measured on the q8 shape; 2048-cap was the G11 default)
        if (blocks > 16384) blocks = 16384;
        if (!blocks) blocks = 1;
        int slot = -1;
        if (timed) {
            slot = ring.begin(stream);
            if (slot < 0) FAIL(RW_E_INTERNAL, "HIP event error (probe timing)");
        }
        if (m.join_type == RW_JOIN_INNER && !m.append_only && r0 == 0) {
            // pre-assigned sparse output + one-bump record reservation
            if (!d_probe_base) {
                HIP_TRY(mem.alloc(&d_probe_base, 4));
                HIP_TRY(mem.alloc(&d_emit_count, 8));
            }
            if (b.n_rows > out.cap)
                FAIL(RW_E_INVAL, "probe batch larger than the output block");
            HIP_TRY(hipMemsetAsync(out.ops, 0xFF, b.n_rows, stream));
            jprobe_setup_kernel<<<1, 1, 0, stream>>>(
                out, side[s].row_cursor, side[s].row_cap, d_probe_base,
                b.n_rows, b.no_insert ? 0u : b.n_rows);
            last_sparse_rows = b.n_rows;
            sparse_out = true;
        }
        if (m.join_type != RW_JOIN_INNER) {
            join_probe_noninner_kernel<<<blocks, 256, 0, stream>>>(
                b, side[s], side[1 - s], m, s, out, r0, r1);
        } else {
            join_probe_kernel<<<blocks, 256, 0, stream>>>(
                b, side[s], side[1 - s], m, s, out, r0, r1, d_probe_base);
        }
        if (timed) {
            HIP_TRY(ring.end(slot, stream));
            probe_launches++;
            probe_rows += b.n_rows;
        }
        return RW_OK;
    }

    // §8f-2 checkpoint spill for the join state table: per side, the
    // epoch's KV deltas in the reference's encodings — key = memcomparable
    // (join key ∥ deduped input pk), value = value-encoded full row
    // (state_table.rs:1615-1727 via OrderedRowSerde; record framing matches
    // the agg spill: [put u8][klen u32 LE][k][vlen u32 LE][v], emitted in
    // memcmp key order). Deltas: rows appended since the last drain that
    // are still alive → PUT; rows killed this epoch that predate the last
    // drain → DELETE; kill-after-insert within the epoch nets away (the
    // record is dead, its PUT is skipped). Degree tables spill too (the
    // block below, drained via rw_join_degree_drain); watermark-TTL
    // cleanup is not spilled (the reference cleans via watermark hints).
    uint32_t flush_mark[2] = {0, 0};
    // rw_join_compact ping-pong stores (lazily allocated once per side;
    // a per-call hipMalloc of row_cap*stride dominates compaction cost)
    uint8_t* compact_scratch[2] = {nullptr, nullptr};
    int checkpoint_drain(int s, std::vector<uint8_t>& sp) {
        HIP_TRY(hipStreamSynchronize(stream));
        JoinSideDev& js = side[s];
        uint32_t cur = 0, kcur = 0;
        HIP_TRY(hipMemcpy(&cur, js.row_cursor, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&kcur, js.killed_cursor, 4, hipMemcpyDeviceToHost));
        if (kcur > js.killed_cap)
            FAIL(RW_E_INTERNAL, "join kill list overflow (lost deltas)");
        if (cur > js.row_cap) cur = js.row_cap;
        uint32_t mark = flush_mark[s];
        size_t stride = js.row_stride;
        std::vector<uint8_t> fresh((size_t)(cur - mark) * stride);
        if (cur > mark)
            HIP_TRY(hipMemcpy(fresh.data(), js.rows + (size_t)mark * stride,
                              fresh.size(), hipMemcpyDeviceToHost));
        std::vector<uint32_t> kills(kcur);
        if (kcur)
            HIP_TRY(hipMemcpy(kills.data(), js.killed, (size_t)kcur * 4,
                              hipMemcpyDeviceToHost));
        auto encode_key = [&](HostRow row) {
            std::vector<uint8_t> k;
            auto put_datum = [&](uint8_t col) {
                rwcodec::memcmp_encode_datum(
                    k, types[s][col], row.datum(types[s][col], col), {});
            };
            for (int i = 0; i < m.KW; i++) put_datum(m.key_cols[s][i]);
            for (int i = 0; i < m.n_pk[s]; i++) put_datum(m.pk_cols[s][i]);
            return k;
        };
        // varchar cells of the fresh records: fetch their strings with the
        // emit path's gather kernels (one strided view per column over the
        // uploaded copy of the fresh range; dead records and NULL cells
        // are masked to length 0 host-side before the upload)
        std::vector<std::vector<uint64_t>> voffs(m.n_cols[s]);
        std::vector<std::vector<uint8_t>> vbytes(m.n_cols[s]);
        if (m.vc_mask[s] && cur > mark) {
            uint32_t nf = cur - mark;
            std::vector<uint64_t> words(nf);
            DevOwner tmp;
            uint64_t* d_words = nullptr;
            HIP_TRY(tmp.alloc(&d_words, (size_t)nf * 8));
            for (int c = 0; c < m.n_cols[s]; c++) {
                if (!((m.vc_mask[s] >> c) & 1)) continue;
                for (uint32_t i = 0; i < nf; i++) {
                    HostRow row{fresh.data() + (size_t)i * stride};
                    bool live = row.hdr().alive && !row.null(c);
                    words[i] = live ? (uint64_t)row.words()[c] : 0;
                }
                if (hipMemcpy(d_words, words.data(), (size_t)nf * 8,
                              hipMemcpyHostToDevice) != hipSuccess)
                    FAIL(RW_E_INTERNAL, "drain string gather failed");
                VarlenView v{};
                v.words = d_words;
                v.stride = 1;
                int rcv = varlen_fetch(v, js.arena, nf, voffs[c], vbytes[c],
                                       false);
                if (rcv != RW_OK) return rcv;
            }
        }
        auto encode_val = [&](HostRow row) {
            std::vector<uint8_t> v;
            for (int c = 0; c < m.n_cols[s]; c++) {
                if ((m.vc_mask[s] >> c) & 1) {
                    // only fresh records are value-encoded (PUT frames)
                    size_t i = (size_t)(row.rec - fresh.data()) / stride;
                    uint64_t o0 = voffs[c][i], o1 = voffs[c][i + 1];
                    rwcodec::value_encode_str(v, row.null(c),
                                              vbytes[c].data() + o0,
                                              (uint32_t)(o1 - o0));
                    continue;
                }
                rwcodec::value_encode_datum(v, types[s][c],
                                            row.datum(types[s][c], c));
            }
            return v;
        };
        // batched gather of every pre-epoch record the kill and degree-
        // dirty lists reference (single kernel + one D2H copy)
        std::vector<uint32_t> dl;
        uint32_t dn = 0;
        if (m.need_deg[s]) {
            HIP_TRY(hipMemcpy(&dn, js.deg_dirty_n, 4,
                              hipMemcpyDeviceToHost));
            dl.resize(dn);
            if (dn)
                HIP_TRY(hipMemcpy(dl.data(), js.deg_dirty_list,
                                  (size_t)dn * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemset(js.deg_dirty_flag, 0, (size_t)js.row_cap * 4));
            HIP_TRY(hipMemset(js.deg_dirty_n, 0, 4));
        }
        std::vector<uint32_t> old_ids;
        for (uint32_t i = 0; i < kcur; i++)
            if (kills[i] < mark) old_ids.push_back(kills[i]);
        size_t n_kill_old = old_ids.size();
        for (uint32_t i = 0; i < dn; i++)
            if (dl[i] < mark) old_ids.push_back(dl[i]);
        std::vector<uint8_t> oldbuf(old_ids.size() * stride);
        if (!old_ids.empty()) {
            uint32_t* d_ids = nullptr;
            uint8_t* d_out = nullptr;
            DevOwner tmp;
            HIP_TRY(tmp.upload(&d_ids, old_ids));
            HIP_TRY(tmp.alloc(&d_out, oldbuf.size()));
            jgather_rows_kernel<<<grid_for((uint32_t)old_ids.size()), 256, 0,
                                  stream>>>(
                js, d_ids, (uint32_t)old_ids.size(), d_out);
            int rcg = hipMemcpy(oldbuf.data(), d_out, oldbuf.size(),
                                hipMemcpyDeviceToHost);
            tmp.release_all();
            if (rcg != hipSuccess)
                FAIL(RW_E_INTERNAL, "drain record gather failed");
        }
        rwcodec::KeyedDelta delta;
        for (size_t i = 0; i < n_kill_old; i++) // a later PUT overwrites = net
            delta.del(encode_key({oldbuf.data() + i * stride}));
        for (uint32_t i = mark; i < cur; i++) {
            HostRow row{fresh.data() + (size_t)(i - mark) * stride};
            if (!row.hdr().alive) continue; // dead: netted away
            delta.put(encode_key(row), encode_val(row));
        }
        delta.write(sp);
        // §8f-2 degree-table deltas (build_degree_row, join/row.rs:99-113:
        // pk = jk ∥ pk as the main table, value = order key ++ degree i64).
        // Keys mirror the main delta (a degree row exists iff its state row
        // does), plus pre-epoch rows whose degree changed during probes
        // (deg_dirty list). Serialized into deg_spill[s], returned by
        // rw_join_degree_drain after this drain.
        if (m.need_deg[s]) {
            auto encode_deg_val = [&](HostRow row) {
                std::vector<uint8_t> v;
                auto put_datum = [&](uint8_t col) {
                    rwcodec::value_encode_datum(
                        v, types[s][col], row.datum(types[s][col], col));
                };
                for (int i = 0; i < m.KW; i++) put_datum(m.key_cols[s][i]);
                for (int i = 0; i < m.n_pk[s]; i++) put_datum(m.pk_cols[s][i]);
                rwcodec::value_encode_datum(
                    v, RW_T_I64, {false, (long long)row.hdr().degree, 0});
                return v;
            };
            rwcodec::KeyedDelta dd;
            for (size_t i = 0; i < n_kill_old; i++)
                dd.del(encode_key({oldbuf.data() + i * stride}));
            for (uint32_t i = mark; i < cur; i++) {
                HostRow row{fresh.data() + (size_t)(i - mark) * stride};
                if (row.hdr().alive) dd.put(encode_key(row), encode_deg_val(row));
            }
            // pre-epoch rows whose degree changed (gathered above after
            // the kill entries); the killed among them are skipped
            for (size_t i = n_kill_old; i < old_ids.size(); i++) {
                HostRow row{oldbuf.data() + i * stride};
                if (row.hdr().alive) dd.put(encode_key(row), encode_deg_val(row));
            }
            dd.write(deg_spill[s]);
        }
        HIP_TRY(hipMemset(js.killed_cursor, 0, 4));
        flush_mark[s] = cur;
        return RW_OK;
    }
    std::vector<uint8_t> deg_spill[2];

    // §8f-5 recovery of side s from its concatenated drains, degrees from
    // the degree table's (optional) stream
    int restore(int s, const uint8_t* buf, uint64_t len,
                const uint8_t* deg_buf, uint64_t deg_len) {
        rwcodec::FrameMap merged;
        if (!rwcodec::merge_frames(buf, len, merged))
            FAIL(RW_E_INVAL, "malformed spill stream");
        // the degree is the row's last datum; a PUT without one is ignored
        std::map<std::string, uint32_t> degs;
        if (deg_buf && deg_len) {
            bool ok = rwcodec::for_each_frame(
                deg_buf, deg_len,
                [&](uint8_t put, const uint8_t* k, uint32_t klen,
                    const uint8_t* v, uint32_t vlen) {
                    std::string key((const char*)k, klen);
                    if (put && vlen >= 9 && v[vlen - 9] == 1) {
                        uint64_t d = 0;
                        for (int b = 0; b < 8; b++)
                            d |= (uint64_t)v[vlen - 8 + b] << (8 * b);
                        degs[key] = (uint32_t)d;
                    } else if (!put) {
                        degs.erase(key);
                    }
                });
            if (!ok) FAIL(RW_E_INVAL, "malformed degree spill stream");
        }
        uint32_t n = (uint32_t)merged.size();
        if (!n) return RW_OK;
        int ncols = m.n_cols[s];
        std::vector<std::vector<int64_t>> cols(ncols,
                                               std::vector<int64_t>(n));
        std::vector<std::vector<uint8_t>> valid(ncols,
                                                std::vector<uint8_t>(n));
        std::vector<uint32_t> degrees(n, 0);
        // varchar columns: decoded strings as bytes + offsets per column
        const uint32_t vcm = m.vc_mask[s];
        std::vector<std::vector<uint8_t>> sbytes(ncols);
        std::vector<std::vector<uint32_t>> soffs(ncols);
        for (int c = 0; c < ncols; c++)
            if ((vcm >> c) & 1) soffs[c].assign(1, 0);
        uint32_t i = 0;
        for (auto& [kbytes, val] : merged) {
            rwcodec::RowReader rd{val.data(), val.size()};
            for (int c = 0; c < ncols; c++) {
                if ((vcm >> c) & 1) {
                    bool null = false;
                    const uint8_t* sp = nullptr;
                    uint32_t slen = 0;
                    if (!rd.str(&null, &sp, &slen))
                        FAIL(RW_E_INVAL, "restore: bad varchar datum");
                    if (sbytes[c].size() + (uint64_t)slen > UINT32_MAX)
                        FAIL(RW_E_INVAL, "restore: column %d strings exceed "
                                         "4 GiB in one call", c);
                    sbytes[c].insert(sbytes[c].end(), sp, sp + slen);
                    soffs[c].push_back((uint32_t)sbytes[c].size());
                    valid[c][i] = !null;
                    continue;
                }
                rwcodec::DatumC d;
                if (!rd.datum(types[s][c], &d))
                    FAIL(RW_E_INVAL, "restore: bad row datum");
                cols[c][i] = d.null ? 0 : d.i;
                valid[c][i] = !d.null;
            }
            auto di = degs.find(kbytes);
            if (di != degs.end()) degrees[i] = di->second;
            i++;
        }
        seen_input = true;
        int rc;
        JoinBatchDev b;
        if (vcm) {
            // varchar side: the decoded rows go through the upload path,
            // which appends the strings to the arena and stages reference
            // words
            std::vector<RwVarlenData> vds(ncols);
            std::vector<RwColumn> rcols(ncols);
            std::vector<uint8_t> rops(n, RW_OP_INSERT);
            for (int c = 0; c < ncols; c++) {
                rcols[c].type = types[s][c];
                rcols[c].valid = valid[c].data();
                if ((vcm >> c) & 1) {
                    vds[c] = RwVarlenData{soffs[c].data(), sbytes[c].data()};
                    rcols[c].data = &vds[c];
                } else {
                    rcols[c].data = cols[c].data();
                }
            }
            RwChunk rch{};
            rch.n_rows = n;
            rch.n_cols = (uint32_t)ncols;
            rch.ops = rops.data();
            rch.vis = nullptr;
            rch.cols = rcols.data();
            rc = upload(s, &rch, &b);
            if (rc != RW_OK) return rc;
            // the staged host buffers die with this scope
            HIP_TRY(hipStreamSynchronize(stream));
        } else {
            rc = ensure_stage(s, n);
            if (rc != RW_OK) return rc;
            b = stage[s];
            for (int c = 0; c < ncols; c++) {
                HIP_TRY(hipMemcpy(b.col_vals[c], cols[c].data(),
                                  (size_t)n * 8, hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(b.col_valid[c], valid[c].data(), n,
                                  hipMemcpyHostToDevice));
            }
        }
        b.vis = nullptr;
        b.n_rows = n;
        DevOwner tmp;
        uint32_t* ddeg = nullptr;
        HIP_TRY(tmp.upload(&ddeg, degrees));
        join_restore_kernel<<<grid_for(n), 256, 0, stream>>>(
            b, side[s], m, s, ddeg, out.counters + 1);
        int rcs = hipStreamSynchronize(stream) == hipSuccess ? RW_OK
                                                             : RW_E_INTERNAL;
        tmp.release(&ddeg);
        if (rcs != RW_OK) FAIL(RW_E_INTERNAL, "restore sync failed");
        uint32_t ctr[2];
        HIP_TRY(hipMemcpy(ctr, out.counters, 8, hipMemcpyDeviceToHost));
        if (ctr[1]) FAIL(RW_E_INTERNAL, "restore overflow (code %u)", ctr[1]);
        // restored rows predate the epoch: the next drain must not re-PUT
        // them
        uint32_t cur = 0;
        HIP_TRY(hipMemcpy(&cur, side[s].row_cursor, 4, hipMemcpyDeviceToHost));
        flush_mark[s] = cur;
        return RW_OK;
    }

    int drain_output() {
        uint32_t ctr[2];
        HIP_TRY(hipMemcpy(ctr, out.counters, 8, hipMemcpyDeviceToHost));
        if (ctr[1] == 1) FAIL(RW_E_INTERNAL, "join output buffer overflow");
        if (ctr[1] == 2) FAIL(RW_E_INTERNAL, "join key table full");
        if (ctr[1] == 3) FAIL(RW_E_INTERNAL, "join row store full");
        uint32_t n_out = ctr[0];
        if (n_out) {
            // columnar device block: copy each column's first n_out entries
            std::vector<int64_t> vals((size_t)n_out * m.n_out); // [c][n]
            std::vector<uint8_t> nulls((size_t)n_out * m.n_out);
            std::vector<uint8_t> ops(n_out);
            for (int ci = 0; ci < m.n_out; ci++) {
                HIP_TRY(hipMemcpy(vals.data() + (size_t)ci * n_out,
                                  out.vals + (size_t)ci * out.cap,
                                  (size_t)n_out * 8, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(nulls.data() + (size_t)ci * n_out,
                                  out.nulls + (size_t)ci * out.cap, n_out,
                                  hipMemcpyDeviceToHost));
            }
            HIP_TRY(hipMemcpy(ops.data(), out.ops, n_out, hipMemcpyDeviceToHost));
            // varchar output columns: the words above reference the arena
            // of the side the column comes from — materialise the strings
            // on the device (over the UNCOMPACTED block: NULL cells and
            // sparse-region sentinel rows yield length 0)
            std::vector<std::vector<uint64_t>> voffs(m.n_out);
            std::vector<std::vector<uint8_t>> vbytes(m.n_out);
            for (int ci = 0; ci < m.n_out; ci++) {
                if (out_types[ci] != RW_T_VARCHAR) continue;
                VarlenView v{};
                v.words = (const uint64_t*)(out.vals + (size_t)ci * out.cap);
                v.stride = 1;
                v.nulls = out.nulls + (size_t)ci * out.cap;
                v.ops = sparse_out ? out.ops : nullptr;
                v.sparse_n = sparse_out ? last_sparse_rows : 0;
                int rcv = varlen_fetch(v, side[m.out_src[ci]].arena, n_out,
                                       voffs[ci], vbytes[ci], true);
                if (rcv != RW_OK) return rcv;
            }
            std::vector<uint32_t> src_idx; // compacted row -> block row
            if (sparse_out) {
                // compact the pre-assigned sparse region (sentinel 0xFF)
                std::vector<uint32_t> real;
                real.reserve(n_out);
                for (uint32_t r2 = 0; r2 < n_out; r2++)
                    if (!(r2 < last_sparse_rows && ops[r2] == 0xFF))
                        real.push_back(r2);
                uint32_t nc = (uint32_t)real.size();
                std::vector<int64_t> cv((size_t)nc * m.n_out);
                std::vector<uint8_t> cn((size_t)nc * m.n_out);
                std::vector<uint8_t> co(nc);
                for (uint32_t j2 = 0; j2 < nc; j2++) {
                    co[j2] = ops[real[j2]];
                    for (int ci = 0; ci < m.n_out; ci++) {
                        cv[(size_t)ci * nc + j2] =
                            vals[(size_t)ci * n_out + real[j2]];
                        cn[(size_t)ci * nc + j2] =
                            nulls[(size_t)ci * n_out + real[j2]];
                    }
                }
                vals.swap(cv);
                nulls.swap(cn);
                ops.swap(co);
                n_out = nc;
                sparse_out = false;
                src_idx.swap(real);
            }
            if (!n_out) {
                HIP_TRY(hipMemset(out.counters, 0, 8));
                return RW_OK;
            }
            // chunk_size rows each (0 = 1024, at least 2); join output has
            // no U-pair rule
            uint32_t max_rows = desc.chunk_size ? desc.chunk_size : 1024;
            if (max_rows < 2) max_rows = 2;
            for (auto [start, take] :
                 rwchunk::slice_ranges(n_out, max_rows, nullptr)) {
                rwchunk::Builder cb(take, (uint32_t)m.n_out);
                for (int ci = 0; ci < m.n_out; ci++) {
                    size_t ix = (size_t)ci * n_out + start;
                    auto valid = rwchunk::from_nulls(&nulls[ix], 1);
                    if (out_types[ci] != RW_T_VARCHAR) {
                        cb.fixed(out_types[ci], &vals[ix], 1, valid);
                        continue;
                    }
                    // the strings of this chunk's rows, found in the
                    // uncompacted block through src_idx
                    bool ok = src_idx.empty()
                                  ? cb.varchar(&voffs[ci][start],
                                               vbytes[ci].data(), nullptr, valid)
                                  : cb.varchar(voffs[ci].data(),
                                               vbytes[ci].data(),
                                               &src_idx[start], valid);
                    if (!ok)
                        FAIL(RW_E_INTERNAL, "output chunk strings exceed 4 GiB; "
                                            "lower chunk_size");
                }
                cb.ops(&ops[start]);
                outq.push(cb.release());
            }
        }
        HIP_TRY(hipMemset(out.counters, 0, 8));
        return RW_OK;
    }

    // The parallel kernel keeps the reference's sequential per-chunk
    // semantics except when a DELETE targets a row also INSERTed in the same
    // chunk (hash_join.rs processes rows in order, :993). Detect those rows
    // host-side and run each such delete in its own single-row segment, in
    // row order — stream ordering makes earlier segments' state visible.
    std::vector<uint32_t> conflict_segments(int s, const RwChunk* c) {
        std::vector<uint32_t> bounds; // segment start offsets (0 implied)
        bool any_delete = false;
        for (uint32_t r = 0; r < c->n_rows; r++) {
            uint8_t op = c->ops[r];
            if (op == RW_OP_DELETE || op == RW_OP_UPDATE_DELETE) {
                any_delete = true;
                break;
            }
        }
        if (!any_delete) return bounds;
        auto row_key = [&](uint32_t r) {
            std::string k;
            k.reserve(m.n_cols[s] * 9);
            for (int ci = 0; ci < m.n_cols[s]; ci++) {
                uint8_t valid = c->cols[ci].valid[r];
                k.push_back((char)valid);
                if ((m.vc_mask[s] >> ci) & 1) {
                    // row identity is the string's BYTES (length-prefixed
                    // so adjacent cells cannot alias)
                    auto* vd = (const RwVarlenData*)c->cols[ci].data;
                    uint32_t o0 = vd->offsets[r];
                    uint32_t len = valid ? vd->offsets[r + 1] - o0 : 0;
                    k.append((const char*)&len, 4);
                    if (len) k.append((const char*)vd->bytes + o0, len);
                    continue;
                }
                int64_t v = valid ? ((const int64_t*)c->cols[ci].data)[r] : 0;
                k.append((const char*)&v, 8);
            }
            return k;
        };
        auto join_key = [&](uint32_t r) {
            std::string k;
            for (int i = 0; i < m.KW; i++) {
                uint8_t ci = m.key_cols[s][i];
                uint8_t valid = c->cols[ci].valid[r];
                k.push_back((char)valid);
                int64_t v = valid ? ((const int64_t*)c->cols[ci].data)[r] : 0;
                k.append((const char*)&v, 8);
            }
            return k;
        };
        std::unordered_multiset<std::string> inserts;
        // degree-carrying types: a mixed insert/delete chunk sharing a JOIN
        // KEY races the matched rows' degree transitions — isolate all rows
        // of such keys (sequential semantics, hash_join.rs row order)
        bool deg = m.need_deg[0] || m.need_deg[1];
        std::unordered_map<std::string, int> jk_ops; // 1=ins 2=del bits
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            uint8_t op = c->ops[r];
            bool ins = (op == RW_OP_INSERT || op == RW_OP_UPDATE_INSERT);
            if (ins) inserts.insert(row_key(r));
            if (deg) jk_ops[join_key(r)] |= ins ? 1 : 2;
        }
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            uint8_t op = c->ops[r];
            bool is_del = (op == RW_OP_DELETE || op == RW_OP_UPDATE_DELETE);
            bool conflict =
                (is_del && !inserts.empty() && inserts.count(row_key(r))) ||
                (deg && jk_ops[join_key(r)] == 3);
            if (conflict) {
                bounds.push_back(r);     // segment ends before this row
                bounds.push_back(r + 1); // the row runs alone, in order
            }
        }
        return bounds;
    }

    // ----- epoch-batched ingestion (the agg's rw_hash_agg_ingest_mode
    // analogue): consecutive SAME-SIDE chunks merge into one staged host
    // batch applied as one launch at the next side switch / barrier /
    // watermark. Exactly order-equivalent: probes read only the MATCH
    // side (which a same-side run never mutates), own-side insert/delete
    // interleavings within the merged batch are the conflict-segment
    // pre-pass's existing job, and cross-SIDE boundaries always flush. -----
    bool epoch_ingest = false;
    int pend_side = -1;
    std::vector<uint8_t> pend_ops;
    std::vector<std::vector<int64_t>> pend_vals;  // per column (16-B decimal n/a)
    std::vector<std::vector<uint8_t>> pend_valid;

    int pending_flush() {
        if (pend_side < 0 || pend_ops.empty()) {
            pend_side = -1;
            return RW_OK;
        }
        int s2 = pend_side;
        uint32_t n = (uint32_t)pend_ops.size();
        std::vector<RwColumn> cols(m.n_cols[s2]);
        for (int c2 = 0; c2 < m.n_cols[s2]; c2++) {
            cols[c2].type = types[s2][c2];
            cols[c2].valid = pend_valid[c2].data();
            cols[c2].data = pend_vals[c2].data();
        }
        RwChunk ch{};
        ch.n_rows = n;
        ch.n_cols = (uint32_t)cols.size();
        ch.ops = pend_ops.data();
        ch.vis = nullptr;
        ch.cols = cols.data();
        pend_side = -1;
        int rc = push_chunk_now(s2, &ch);
        pend_ops.clear();
        for (auto& v : pend_vals) v.clear();
        for (auto& v : pend_valid) v.clear();
        return rc;
    }

    int push_chunk(int s, const RwChunk* c) {
        if (s != 0 && s != 1) FAIL(RW_E_INVAL, "bad side");
        if (epoch_ingest) {
            if (c->vis)
                FAIL(RW_E_INVAL,
                     "epoch-batched ingest requires visibility-compacted "
                     "chunks");
            if (pend_side >= 0 && pend_side != s) {
                int rc = pending_flush();
                if (rc != RW_OK) return rc;
            }
            if (pend_side < 0) {
                pend_side = s;
                pend_vals.assign(m.n_cols[s], {});
                pend_valid.assign(m.n_cols[s], {});
            }
            pend_ops.insert(pend_ops.end(), c->ops, c->ops + c->n_rows);
            for (int c2 = 0; c2 < m.n_cols[s]; c2++) {
                const int64_t* d = (const int64_t*)c->cols[c2].data;
                pend_vals[c2].insert(pend_vals[c2].end(), d, d + c->n_rows);
                pend_valid[c2].insert(pend_valid[c2].end(),
                                      c->cols[c2].valid,
                                      c->cols[c2].valid + c->n_rows);
            }
            return RW_OK;
        }
        return push_chunk_now(s, c);
    }

    int push_chunk_now(int s, const RwChunk* c) {
        JoinBatchDev b;
        int rc = upload(s, c, &b);
        if (rc != RW_OK) return rc;
        std::vector<uint32_t> bounds = conflict_segments(s, c);
        // varchar sides: delete rows resolve their strings against the
        // stored records before each segment's probe (see the kernel)
        std::vector<uint32_t> del_before; // deletes in rows [0, r)
        if (m.vc_mask[s] && !b.all_insert) {
            del_before.assign((size_t)b.n_rows + 1, 0);
            for (uint32_t r = 0; r < b.n_rows; r++) {
                bool vis = !(c->vis && !c->vis[r]);
                bool del = c->ops[r] == RW_OP_DELETE ||
                           c->ops[r] == RW_OP_UPDATE_DELETE;
                del_before[r + 1] = del_before[r] + (vis && del);
            }
        }
        auto run_segment = [&](uint32_t r0, uint32_t r1) -> int {
            if (!del_before.empty() && del_before[r1] != del_before[r0]) {
                join_varlen_resolve_kernel<<<grid_for(r1 - r0), 256, 0,
                                             stream>>>(b, side[s], m, s, r0, r1);
            }
            return probe(s, b, true, r0, r1);
        };
        uint32_t start = 0;
        for (uint32_t bnd : bounds) {
            if (bnd > start) {
                rc = run_segment(start, bnd);
                if (rc != RW_OK) return rc;
            }
            start = bnd;
        }
        if (start < b.n_rows) {
            rc = run_segment(start, b.n_rows);
            if (rc != RW_OK) return rc;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return drain_output();
    }

    int flush(uint64_t) {
        if (epoch_ingest) {
            int rc = pending_flush();
            if (rc != RW_OK) return rc;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return RW_OK;
    }

    int watermark(int s, uint32_t col_idx, int64_t val, uint32_t* out_cols,
                  int64_t* out_vals, int max_out, int* n_out_p) {
        if (epoch_ingest) {
            int rcp = pending_flush();
            if (rcp != RW_OK) return rcp;
        }
        int n_out = 0;
        auto& mine = s == 0 ? wm_side0 : wm_side1;
        for (uint32_t idx = 0; idx < (uint32_t)m.KW; idx++) {
            if (m.key_cols[s][idx] != col_idx) continue;
            mine[idx] = {true, val};
            if (!wm_side0[idx].has || !wm_side1[idx].has) continue;
            int64_t sel = std::min(wm_side0[idx].val, wm_side1[idx].val);
            if (wm_out[idx].has && sel <= wm_out[idx].val) continue;
            wm_out[idx] = {true, sel};
            bool clean = false;
            for (size_t w = 0; w < wm_pos.size(); w++)
                if (wm_pos[w] == idx && wm_clean[w]) clean = true;
            if (clean) {
                for (int sd = 0; sd < 2; sd++)
                    join_clean_kernel<<<2048, 256, 0, stream>>>(
                        side[sd], (int)m.key_cols[sd][idx], sel, m.KW);
                HIP_TRY(hipStreamSynchronize(stream));
            }
            // update side's output columns first, then the match side's
            for (int pass = 0; pass < 2; pass++) {
                int s2 = pass == 0 ? s : 1 - s;
                uint32_t src = m.key_cols[s2][idx] +
                               (s2 == 1 ? (uint32_t)m.n_cols[0] : 0);
                for (int oi = 0; oi < m.n_out; oi++) {
                    uint32_t osrc = (uint32_t)m.out_col[oi] +
                                    (m.out_src[oi] ? (uint32_t)m.n_cols[0] : 0);
                    if (osrc == src && n_out < max_out) {
                        out_cols[n_out] = (uint32_t)oi;
                        out_vals[n_out] = sel;
                        n_out++;
                    }
                }
            }
        }
        // inequality-pair watermarks (hash_join.rs:869-914): buffer per
        // side; the min across sides emits for the LARGER side's output
        // columns and (clean flag) sweeps that side's rows whose pair
        // column sorts below it — through the kill list, so the next
        // drain nets the cleaned rows to DELETE frames
        for (size_t p = 0; p < ineq_col[0].size(); p++) {
            if (ineq_col[s][p] != col_idx) continue;
            ineq_wm[s][p] = {true, val};
            if (!ineq_wm[0][p].has || !ineq_wm[1][p].has) continue;
            int64_t sel = std::min(ineq_wm[0][p].val, ineq_wm[1][p].val);
            if (ineq_out[p].has && sel <= ineq_out[p].val) continue;
            ineq_out[p] = {true, sel};
            int larger = ineq_larger[p] ? 0 : 1;
            if (ineq_do_clean[p]) {
                join_clean_kernel<<<2048, 256, 0, stream>>>(
                    side[larger], (int)ineq_col[larger][p], sel, m.KW);
                HIP_TRY(hipStreamSynchronize(stream));
            }
            uint32_t src = ineq_col[larger][p] +
                           (larger == 1 ? (uint32_t)m.n_cols[0] : 0);
            for (int oi = 0; oi < m.n_out; oi++) {
                uint32_t osrc = (uint32_t)m.out_col[oi] +
                                (m.out_src[oi] ? (uint32_t)m.n_cols[0] : 0);
                if (osrc == src && n_out < max_out) {
                    out_cols[n_out] = (uint32_t)oi;
                    out_vals[n_out] = sel;
                    n_out++;
                }
            }
        }
        *n_out_p = n_out;
        return RW_OK;
    }

    RwChunk* poll() { return outq.poll(); }

    ~HashJoin() {
        mem.release_all(); // device memory goes before the stream
        if (stream) hipStreamDestroy(stream);
    }
};

extern "C" {

void* rw_hash_join_create(const RwHashJoinDesc* d) {
    auto* h = new HashJoin();
    if (h->init(d) != RW_OK) {
        delete h;
        return nullptr;
    }
    return h;
}
int rw_hash_join_push_chunk(void* h, int side, const RwChunk* c) {
    return ((HashJoin*)h)->push_chunk(side, c);
}
int rw_hash_join_flush(void* h, uint64_t epoch) { return ((HashJoin*)h)->flush(epoch); }

// epoch-batched ingest mode (rw_stream.h): same-side chunk runs merge into
// one launch; barriers/watermarks/side switches flush the staged run
int rw_hash_join_ingest_mode(void* h, int epoch_batched) {
    auto* j = (HashJoin*)h;
    if (!epoch_batched && j->pend_side >= 0)
        FAIL(RW_E_INVAL, "staged chunks pending; flush before disabling");
    if (epoch_batched && j->has_varchar())
        FAIL(RW_E_INVAL, "epoch-batched ingest stages 8-byte columns only; "
                         "not supported with varchar columns");
    j->epoch_ingest = epoch_batched != 0;
    return RW_OK;
}

// the device-batch and device-hop entry points move 8-byte words without
// the arena behind them (rw_stream.h: varchar payload columns)
#define JOIN_NO_VARCHAR(j, what)                                          \
    do {                                                                  \
        if ((j)->has_varchar())                                           \
            FAIL(RW_E_INVAL, what " is not supported on a join with "     \
                                  "varchar columns");                     \
    } while (0)

int rw_hash_join_varlen_reserve(void* h, int side, uint64_t bytes) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    if (!j->m.vc_mask[side])
        FAIL(RW_E_INVAL, "side %d has no varchar column", side);
    if (j->seen_input)
        FAIL(RW_E_INVAL, "varlen_reserve is legal only before any input");
    if (!bytes || bytes > rwvarlen::MAX_OFF)
        FAIL(RW_E_INVAL, "varlen_reserve: bad capacity");
    j->mem.release(&j->side[side].arena);
    j->arena_cap[side] = 0;
    j->arena_reserve[side] = bytes;
    return j->arena_ensure(side, 0);
}

int rw_hash_join_varlen_stats(void* h, int side, uint64_t* used,
                              uint64_t* capacity) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    if (used) *used = j->arena_used[side];
    if (capacity) *capacity = j->arena_cap[side];
    return RW_OK;
}

int rw_hash_join_varlen_emit_stats(void* h, double* ms, double* copy_ms,
                                   uint64_t* bytes, uint64_t* launches) {
    auto* j = (HashJoin*)h;
    if (ms) *ms = j->vf.vemit_ms;
    if (copy_ms) *copy_ms = j->vf.vcopy_ms;
    if (bytes) *bytes = j->vf.vemit_bytes;
    if (launches) *launches = j->vf.vemit_launches;
    return RW_OK;
}

int rw_hash_join_watermark(void* h, int side, uint32_t col_idx, int64_t val,
                           uint32_t* out_cols, int64_t* out_vals, int max_out) {
    int n = 0;
    int rc = ((HashJoin*)h)->watermark(side, col_idx, val, out_cols, out_vals,
                                       max_out, &n);
    return rc == RW_OK ? n : rc;
}

int rw_hash_agg_watermark(void* h, uint32_t group_key_pos, int64_t val) {
    auto* agg = (HashAgg*)h;
    if (group_key_pos >= (uint32_t)agg->KW) FAIL(RW_E_INVAL, "bad group key pos");
    if ((agg->vc_mask >> group_key_pos) & 1)
        FAIL(RW_E_INVAL, "watermark on a varchar group key unsupported");
    if (agg->eowc) {
        // EOWC: buffer the window watermark; windows close at the next
        // barrier (hash_agg.rs:657-700)
        if (group_key_pos != 0) FAIL(RW_E_INVAL, "EOWC watermark must be on group key 0");
        if (!agg->has_pending_wm || val > agg->pending_wm)
            agg->pending_wm = val;
        agg->has_pending_wm = true;
        return RW_OK;
    }
    // clean + capture persisted cleaned groups for DELETE spill frames
    // (state-table watermark range delete, state_table.rs:1707)
    uint32_t crec_cap = 1u << 18;
    for (;;) {
        DevOwner tmp;
        DedupDirtyRec* crecs = nullptr;
        uint32_t* cmeta = nullptr; // [0]=n [1]=overflow
        HIP_TRY(tmp.alloc(&crecs, (size_t)crec_cap * sizeof(DedupDirtyRec)));
        HIP_TRY(tmp.alloc(&cmeta, 8));
        HIP_TRY(hipMemset(cmeta, 0, 8));
        agg_clean_kernel<<<2048, 256, 0, agg->stream>>>(
            agg->t, (int)group_key_pos, val, agg->KW, agg->n_calls,
            agg->cd(0), agg->cd(1), agg->cd(2), agg->cd(3), crecs, cmeta,
            crec_cap, cmeta + 1);
        int rcs = hipStreamSynchronize(agg->stream) == hipSuccess
                      ? RW_OK : RW_E_INTERNAL;
        uint32_t meta[2] = {0, 0};
        if (rcs == RW_OK)
            hipMemcpy(meta, cmeta, 8, hipMemcpyDeviceToHost);
        uint32_t n = meta[0] < crec_cap ? meta[0] : crec_cap;
        std::vector<DedupDirtyRec> recs(n);
        if (rcs == RW_OK && n)
            hipMemcpy(recs.data(), crecs, (size_t)n * sizeof(DedupDirtyRec),
                      hipMemcpyDeviceToHost);
        // varchar key columns: the captured words' strings, for the DELETE
        // frames' memcomparable keys
        static_assert(sizeof(DedupDirtyRec) % 8 == 0, "word-strided view");
        int rcv = RW_OK;
        if (rcs == RW_OK && n && agg->has_vc())
            rcv = agg->fetch_key_strings((const uint64_t*)crecs,
                                         sizeof(DedupDirtyRec) / 8, n);
        tmp.release_all();
        if (rcs != RW_OK) FAIL(RW_E_INTERNAL, "agg clean sync failed");
        if (rcv != RW_OK) return rcv;
        std::vector<uint8_t> k;
        for (uint32_t i = 0; i < n; i++) {
            k.clear();
            for (int w = 0; w < agg->KW; w++)
                agg->encode_key_datum(k, true, w, i,
                                      ((recs[i].nulls >> w) & 1) != 0,
                                      recs[i].key[w]);
            rwcodec::put_frame(agg->spill, 0, k); // DELETE
        }
        if (!meta[1]) break; // no overflow: every slot cleaned
        crec_cap *= 4;
    }
    // the same watermark cleans the DISTINCT dedup tables' group prefix
    for (size_t di = 0; di < agg->dedup_slots.size(); di++) {
        size_t dcap = (size_t)agg->dedup_cap_mask + 1;
        dedup_clean_kernel<<<2048, 256, 0, agg->stream>>>(
            agg->dedup_slots[di], dcap, (int)group_key_pos, val,
            agg->ddirty_flag[di], agg->ddirty_list[di], agg->ddirty_n[di]);
    }
    HIP_TRY(hipStreamSynchronize(agg->stream));
    return RW_OK;
}

// rescale re-scope (update_vnode_bitmap): drop state whose dist-key vnode
// (dist key = group key) is no longer owned; no retractions are emitted.
// `bitmap` is vnode_count/8 bytes, LSB-first per byte (common Bitmap layout).
int rw_hash_agg_update_vnode_bitmap(void* h, const uint8_t* bitmap,
                                    uint32_t vnode_count) {
    auto* agg = (HashAgg*)h;
    AGG_NO_VARCHAR(agg, "rw_hash_agg_update_vnode_bitmap");
    if (!vnode_count || vnode_count % 8 || vnode_count > 4096)
        FAIL(RW_E_INVAL, "vnode_count");
    if (ensure_crc_table() != RW_OK) FAIL(RW_E_INTERNAL, "crc table");
    if (!agg->d_vnode_bitmap)
        HIP_TRY(agg->mem.alloc(&agg->d_vnode_bitmap, 512));
    HIP_TRY(hipMemcpyAsync(agg->d_vnode_bitmap, bitmap, vnode_count / 8,
                           hipMemcpyHostToDevice, agg->stream));
    uint8_t ty[4] = {RW_T_I64, RW_T_I64, RW_T_I64, RW_T_I64};
    for (int k = 0; k < agg->KW && k < 4; k++) ty[k] = agg->out_types[k];
    agg_vnode_scope_kernel<<<2048, 256, 0, agg->stream>>>(
        agg->t, agg->KW, agg->n_calls, agg->cd(0), agg->cd(1), agg->cd(2),
        agg->cd(3), agg->d_vnode_bitmap, vnode_count, ty[0], ty[1], ty[2],
        ty[3]);
    HIP_TRY(hipStreamSynchronize(agg->stream));
    return RW_OK;
}

// join dist key = join key; both sides are re-scoped together
int rw_hash_join_update_vnode_bitmap(void* h, const uint8_t* bitmap,
                                     uint32_t vnode_count) {
    auto* j = (HashJoin*)h;
    if (!vnode_count || vnode_count % 8 || vnode_count > 4096)
        FAIL(RW_E_INVAL, "vnode_count");
    if (ensure_crc_table() != RW_OK) FAIL(RW_E_INTERNAL, "crc table");
    if (!j->d_vnode_bitmap) HIP_TRY(j->mem.alloc(&j->d_vnode_bitmap, 512));
    HIP_TRY(hipMemcpyAsync(j->d_vnode_bitmap, bitmap, vnode_count / 8,
                           hipMemcpyHostToDevice, j->stream));
    for (int s = 0; s < 2; s++) {
        uint8_t ty[4] = {RW_T_I64, RW_T_I64, RW_T_I64, RW_T_I64};
        uint8_t kc[4] = {0, 0, 0, 0};
        for (int k = 0; k < j->m.KW && k < 4; k++) {
            ty[k] = j->types[s][j->m.key_cols[s][k]];
            kc[k] = j->m.key_cols[s][k];
        }
        join_vnode_scope_kernel<<<2048, 256, 0, j->stream>>>(
            j->side[s], j->m.KW, j->d_vnode_bitmap, vnode_count, ty[0], ty[1],
            ty[2], ty[3], kc[0], kc[1], kc[2], kc[3]);
    }
    HIP_TRY(hipStreamSynchronize(j->stream));
    return RW_OK;
}
RwChunk* rw_hash_join_poll(void* h) { return ((HashJoin*)h)->poll(); }
void rw_hash_join_destroy(void* h) { delete (HashJoin*)h; }

// --- bench support: device-resident probe batches; outputs stay in HBM
// (the downstream operator is device-resident — DESIGN.md §5; the
// PCIe-inclusive ingest rate is reported separately) ---

void* rw_join_bench_preload(void* h, int side, const RwChunk* c) {
    auto* j = (HashJoin*)h;
    if (j->has_varchar()) {
        g_err = "rw_join_bench_preload is not supported on a join with "
                "varchar columns";
        return nullptr;
    }
    auto b = std::make_unique<Owned<JoinBatchDev>>();
    uint32_t n = c->n_rows;
    for (int ci = 0; ci < j->m.n_cols[side]; ci++) {
        if (b->mem.alloc(&b->col_vals[ci], (size_t)n * 8) != hipSuccess) return nullptr;
        if (b->mem.alloc(&b->col_valid[ci], n) != hipSuccess) return nullptr;
        hipMemcpy(b->col_vals[ci], c->cols[ci].data, (size_t)n * 8,
                  hipMemcpyHostToDevice);
        hipMemcpy(b->col_valid[ci], c->cols[ci].valid, n, hipMemcpyHostToDevice);
    }
    if (b->mem.alloc(&b->ops, n) != hipSuccess) return nullptr;
    hipMemcpy(b->ops, c->ops, n, hipMemcpyHostToDevice);
    b->vis = nullptr;
    b->n_rows = n;
    b->all_insert = 1;
    for (uint32_t r = 0; r < n && b->all_insert; r++)
        if (c->ops[r] != RW_OP_INSERT && c->ops[r] != RW_OP_UPDATE_INSERT)
            b->all_insert = 0;
    b->all_valid = 1;
    for (uint32_t ci2 = 0; ci2 < c->n_cols && b->all_valid; ci2++)
        for (uint32_t r = 0; r < n && b->all_valid; r++)
            b->all_valid = c->cols[ci2].valid[r];
    b->unique_keys = 0;
    return static_cast<JoinBatchDev*>(b.release());
}

// launch the probe for a preloaded batch; outputs accumulate in the device
// buffer until rw_join_bench_drain
int rw_join_bench_apply(void* h, int side, void* batch) {
    auto* j = (HashJoin*)h;
    JOIN_NO_VARCHAR(j, "rw_join_bench_apply");
    return j->probe(side, *(JoinBatchDev*)batch, true, 0,
                    ((JoinBatchDev*)batch)->n_rows);
}

// device-side drain: return match count, check errors, reset the cursor
__global__ void join_counters_reset_kernel(uint32_t* counters) {
    counters[0] = 0; // out cursor (overflow flag counters[1] persists)
}

// C-side q8 step loop: `steps` probe applies over a cycle of preloaded
// batches with a stream-ordered output-cursor reset after each step (the
// downstream consumes device-resident). No host round-trip per step — the
// Python-side drain cost ~0.15 ms/step of pure sync/copy overhead.
// Overflow flags surface at the next rw_join_bench_drain.
int rw_join_bench_run(void* h, int side, void** batches, int n_batches,
                      int steps) {
    auto* j = (HashJoin*)h;
    JOIN_NO_VARCHAR(j, "rw_join_bench_run");
    for (int i = 0; i < steps; i++) {
        // the inner probe's per-batch setup re-bases the output block, so
        // no per-step reset is needed; the last step's emissions survive
        // for the drain's count
        int rc = j->probe(side, *(JoinBatchDev*)batches[i % n_batches], true,
                          0, ((JoinBatchDev*)batches[i % n_batches])->n_rows);
        if (rc != RW_OK) return rc;
    }
    return RW_OK;
}

long long rw_join_bench_drain(void* h) {
    auto* j = (HashJoin*)h;
    if (hipStreamSynchronize(j->stream) != hipSuccess) return -1;
    uint32_t ctr[2];
    if (hipMemcpy(ctr, j->out.counters, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (ctr[1] != 0) {
        g_err = "join bench overflow/full (code " + std::to_string(ctr[1]) + ")";
        return -(long long)ctr[1] - 1;
    }
    long long emitted = (long long)ctr[0];
    if (j->sparse_out && j->d_emit_count) {
        // count the sparse region's real emissions (sentinel-aware)
        (void)hipMemset(j->d_emit_count, 0, 8);
        join_count_emitted_kernel<<<2048, 256, 0, j->stream>>>(
            j->out.ops, j->last_sparse_rows, j->out.counters,
            j->d_emit_count);
        unsigned long long cnt = 0;
        if (hipStreamSynchronize(j->stream) != hipSuccess) return -1;
        if (hipMemcpy(&cnt, j->d_emit_count, 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
            return -1;
        emitted = (long long)cnt;
        j->sparse_out = false;
    }
    hipMemset(j->out.counters, 0, 8);
    return emitted;
}

__global__ void join_out_vis_kernel(const uint8_t* ops, uint32_t sparse_n,
                                    uint32_t total, uint8_t* vis) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < total;
         r += stride)
        vis[r] = !(r < sparse_n && ops[r] == 0xFF);
}

// Device-side pipeline hop: apply the join's accumulated output buffer
// (row-major [row][n_out]) directly as agg input via a strided AggBatch
// view — the fragment edge agg(join(...)) of the TPC-H q3 MV without
// leaving HBM. The agg must have been created with the join's output
// schema as its input schema. Resets the join's output cursor.
// agg-output -> join-input transpose: the agg's flush output block is
// row-major [row][gk ++ calls]; the join consumes columnar batches. The
// map picks which record columns become join input columns.
struct AggOutColMap {
    uint8_t n;
    uint8_t map[MAX_COLS];
};
__global__ void aggout_to_join_kernel(const long long* avals,
                                      const uint8_t* anulls,
                                      const uint8_t* aops, uint32_t n,
                                      int width, AggOutColMap cm,
                                      JoinBatchDev b) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        for (int i = 0; i < cm.n; i++) {
            b.col_vals[i][r] = avals[(size_t)r * width + cm.map[i]];
            b.col_valid[i][r] = !anulls[(size_t)r * width + cm.map[i]];
        }
        b.ops[r] = aops[r];
    }
}

// Device-resident fragment edge agg -> join (the q7 plan's
// StreamHashJoin right input = the windowed max's change stream,
// nexmark.yaml q7): applies the agg's device-resident flush output
// (rw_agg_flush_device's emitted rows, still in HBM) as one join input
// batch on `side`. Safe without the host conflict pre-pass: a U-/Delete
// record's target row is always a PREVIOUS barrier's U+/Insert (the agg
// emits at most one change pair per group per barrier), so no delete
// targets a same-batch insert (DESIGN §3.2's only inner-join conflict).
int rw_join_apply_aggout(void* join_h, void* agg_h, int side,
                         const uint32_t* col_map, int n_map,
                         uint64_t n_rows) {
    auto* j = (HashJoin*)join_h;
    auto* agg = (HashAgg*)agg_h;
    JOIN_NO_VARCHAR(j, "rw_join_apply_aggout");
    AGG_NO_VARCHAR(agg, "rw_join_apply_aggout");
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    if (n_map != j->m.n_cols[side])
        FAIL(RW_E_INVAL, "col_map size %d != side cols %d", n_map,
             j->m.n_cols[side]);
    if (!n_rows) return RW_OK;
    if (n_rows > UINT32_MAX) FAIL(RW_E_INVAL, "batch too large");
    HIP_TRY(hipStreamSynchronize(agg->stream));
    int rc = j->ensure_stage(side, (uint32_t)n_rows);
    if (rc != RW_OK) return rc;
    AggOutColMap cm{};
    cm.n = (uint8_t)n_map;
    for (int i = 0; i < n_map; i++) {
        if (col_map[i] >= (uint32_t)agg->out_width)
            FAIL(RW_E_INVAL, "col_map[%d]=%u outside agg record", i,
                 col_map[i]);
        cm.map[i] = (uint8_t)col_map[i];
    }
    JoinBatchDev b = j->stage[side];
    b.vis = nullptr;
    b.n_rows = (uint32_t)n_rows;
    b.all_insert = 0; // change stream carries U-/U+ pairs
    b.unique_keys = 0;
    b.no_insert = 0;
    aggout_to_join_kernel<<<grid_for((uint32_t)n_rows), 256, 0, j->stream>>>(
        agg->t.out_vals, agg->t.out_nulls, agg->t.out_ops, (uint32_t)n_rows,
        agg->out_width, cm, b);
    return j->probe(side, b, true, 0, (uint32_t)n_rows);
}

// marshal the join's device-resident output buffer into host chunks on
// the poll queue (what push_chunk does after its probe) — for callers of
// rw_join_apply_aggout that want the emissions as chunks (parity tests)
int rw_join_marshal_output(void* join_h) {
    auto* j = (HashJoin*)join_h;
    JOIN_NO_VARCHAR(j, "rw_join_marshal_output");
    HIP_TRY(hipStreamSynchronize(j->stream));
    return j->drain_output();
}

// device-resident VirtualNode::compute_chunk (vnode.rs:146-181) over a
// preloaded join batch's columns, launched on the join's stream — the q7
// pipeline's exchange-hop vnode computation at R=1 (the reference computes
// vnodes in HashDataDispatcher even with one downstream; the N>1 payload
// exchange is librw_exchange's path)
int rw_join_vnode_hop(void* join_h, void* batch, uint32_t col, uint8_t type,
                      uint32_t vnode_count) {
    auto* j = (HashJoin*)join_h;
    auto* b = (JoinBatchDev*)batch;
    JOIN_NO_VARCHAR(j, "rw_join_vnode_hop");
    if (j->d_vnode_hop_cap < b->n_rows) {
        j->d_vnode_hop_cap = 0;
        HIP_TRY(j->mem.regrow(&j->d_vnode_hop, (size_t)b->n_rows * 2 + 2));
        j->d_vnode_hop_cap = b->n_rows;
    }
    VnodeBatch vb{};
    vb.col_vals[0] = b->col_vals[col];
    vb.col_valid[0] = b->col_valid[col];
    vb.n_rows = b->n_rows;
    uint32_t blocks = (b->n_rows + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    vnode_kernel<<<blocks, 256, 0, j->stream>>>(vb, 1, vnode_count,
                                                j->d_vnode_hop, type, 0, 0,
                                                0);
    return RW_OK;
}

int rw_agg_apply_joinout(void* agg_h, void* join_h) {
    auto* agg = (HashAgg*)agg_h;
    auto* j = (HashJoin*)join_h;
    JOIN_NO_VARCHAR(j, "rw_agg_apply_joinout");
    AGG_NO_VARCHAR(agg, "rw_agg_apply_joinout");
    if (agg->n_dec)
        FAIL(RW_E_INVAL, "decimal columns not yet in the join output block");
    if (hipStreamSynchronize(j->stream) != hipSuccess)
        FAIL(RW_E_INTERNAL, "join sync failed");
    uint32_t ctr[2];
    HIP_TRY(hipMemcpy(ctr, j->out.counters, 8, hipMemcpyDeviceToHost));
    if (ctr[1] != 0) FAIL(RW_E_INTERNAL, "join overflow %u before pipeline hop", ctr[1]);
    uint32_t n = ctr[0];
    if (!n) return RW_OK;
    if (!j->zeros) {
        HIP_TRY(j->mem.alloc(&j->zeros, (size_t)j->out.cap * j->m.n_out));
        HIP_TRY(hipMemset(j->zeros, 0, (size_t)j->out.cap * j->m.n_out));
    }
    AggBatch b{};
    b.stride = 1; // columnar output block: plain columnar agg input
    b.valid_inverted = 1;
    auto bind = [&](int slot, int src_col) {
        b.col_vals[slot] = j->out.vals + (size_t)src_col * j->out.cap;
        b.col_valid[slot] = j->out.nulls + (size_t)src_col * j->out.cap;
    };
    for (int i = 0; i < agg->KW; i++) {
        if ((int)agg->group_key[i] >= j->m.n_out)
            FAIL(RW_E_INVAL, "agg group key %u outside join output", agg->group_key[i]);
        bind(i, (int)agg->group_key[i]);
    }
    for (int ci = 0; ci < agg->n_calls; ci++) {
        if (agg->calls[ci].arg >= 0) {
            if (agg->calls[ci].arg >= j->m.n_out)
                FAIL(RW_E_INVAL, "agg arg outside join output");
            bind(agg->KW + ci, agg->calls[ci].arg);
        } else {
            b.col_vals[agg->KW + ci] = j->out.vals; // unread
            b.col_valid[agg->KW + ci] = j->zeros;   // inverted -> all valid
        }
    }
    if (agg->n_minput) {
        for (size_t k = 0; k < agg->stream_key.size(); k++) {
            if ((int)agg->stream_key[k] >= j->m.n_out)
                FAIL(RW_E_INVAL, "agg stream key outside join output");
            bind(agg->KW + agg->n_calls + (int)k, (int)agg->stream_key[k]);
        }
    }
    b.ops = j->out.ops;
    b.vis = nullptr;
    b.n_rows = n;
    if (j->sparse_out) {
        // pre-assigned sparse output: sentinel rows masked by visibility
        if (j->d_vis_cap < n) {
            j->d_vis_cap = 0;
            HIP_TRY(j->mem.regrow(&j->d_vis_scratch, n));
            j->d_vis_cap = n;
        }
        uint32_t blocks = (n + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        join_out_vis_kernel<<<blocks, 256, 0, agg->stream>>>(
            j->out.ops, j->last_sparse_rows, n, j->d_vis_scratch);
        b.vis = j->d_vis_scratch;
        b.dense = 0;
        j->sparse_out = false;
    }
    // run the agg on ITS stream after the join's work is drained (synced
    // above), then reset the join cursor
    int rc = agg->apply(b, true);
    if (rc != RW_OK) return rc;
    if (hipStreamSynchronize(agg->stream) != hipSuccess)
        FAIL(RW_E_INTERNAL, "agg sync failed");
    HIP_TRY(hipMemset(j->out.counters, 0, 8));
    return agg->check_overflow();
}

// C-side q7-pipeline step loop (the full q7 stream plan, bench.py
// bench_q7pipe): per step, two vnode exchange hops + the agg apply + the
// join-left probe; every barrier_every steps the agg flush's change
// stream feeds the join's right side device-resident. The Python
// interpreter costs ~30-40 us/step in ctypes dispatch — at a ~0.2 ms
// step that is 20% overhead, so the loop lives here.
int rw_q7pipe_bench_run(void* agg_h, void* join_h, void** agg_batches,
                        void** join_batches, int n_batches, int steps,
                        int barrier_every, const uint32_t* col_map,
                        int n_map, int step0) {
    auto* agg = (HashAgg*)agg_h;
    auto* j = (HashJoin*)join_h;
    JOIN_NO_VARCHAR(j, "rw_q7pipe_bench_run");
    AGG_NO_VARCHAR(agg, "rw_q7pipe_bench_run");
    // Long-run state maintenance: the agg change stream retires a right-
    // side record per replaced window max (U- then U+), so dead records
    // accumulate and lengthen the probe walks. Every RW_Q7PIPE_COMPACT
    // barriers (default 4; 0 disables) the loop runs the product cadence:
    // checkpoint-drain the right side (the barrier's commit), then
    // rw_join_compact reclaims the dead records. Costs stay inside the
    // timed region — they are part of running the plan.
    const char* ce = getenv("RW_Q7PIPE_COMPACT");
    int compact_every = ce ? atoi(ce) : 4;
    int barriers_done = 0;
    for (int i = 0; i < steps; i++) {
        int bi = (step0 + i) % n_batches;
        auto* jb = (JoinBatchDev*)join_batches[bi];
        int rc = rw_join_vnode_hop(join_h, jb, 3, RW_T_I64, 256);
        if (rc != RW_OK) return rc;
        rc = agg->apply(*(AggBatch*)agg_batches[bi], true);
        if (rc != RW_OK) return rc;
        rc = rw_join_vnode_hop(join_h, jb, 2, RW_T_I64, 256);
        if (rc != RW_OK) return rc;
        rc = j->probe(RW_SIDE_LEFT, *jb, true, 0, jb->n_rows);
        if (rc != RW_OK) return rc;
        if (barrier_every > 0 && (step0 + i + 1) % barrier_every == 0) {
            long long n = rw_agg_flush_device(agg_h, (uint64_t)(step0 + i));
            if (n < 0) return RW_E_INTERNAL;
            rc = rw_join_apply_aggout(join_h, agg_h, RW_SIDE_RIGHT, col_map,
                                      n_map, (uint64_t)n);
            if (rc != RW_OK) return rc;
            long long e = rw_join_bench_drain(join_h);
            if (e < 0) return RW_E_INTERNAL;
            barriers_done++;
            if (compact_every > 0 && barriers_done % compact_every == 0) {
                std::vector<uint8_t> sp;
                rc = j->checkpoint_drain(RW_SIDE_RIGHT, sp);
                if (rc != RW_OK) return rc;
                j->deg_spill[RW_SIDE_RIGHT].clear();
                rc = rw_join_compact(join_h, RW_SIDE_RIGHT, nullptr);
                if (rc != RW_OK) return rc;
            }
        }
    }
    return RW_OK;
}

int rw_join_kernel_stats(void* h, RwKernelStats* out) {
    auto* j = (HashJoin*)h;
    if (!j->ring.harvest_all())
        FAIL(RW_E_INTERNAL, "event harvest failed");
    out->launches = j->probe_launches;
    out->total_ms = j->ring.ms_total;
    out->rows = j->probe_rows;
    return RW_OK;
}

int rw_join_checkpoint_drain(void* h, int side, uint8_t** buf,
                             uint64_t* len) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    std::vector<uint8_t> sp;
    int rc = j->checkpoint_drain(side, sp);
    if (rc != RW_OK) return rc;
    return spill_export(sp, buf, len);
}

int rw_hash_join_restore(void* h, int side, const uint8_t* buf,
                         uint64_t len, const uint8_t* deg_buf,
                         uint64_t deg_len) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    return j->restore(side, buf, len, deg_buf, deg_len);
}

// §8f-4 memory reclamation: rebuild one side's record store and buckets
// without its dead records (the reference reclaims them in Hummock
// compaction; here a maintenance pass the embedder schedules between
// epochs, right after the checkpoint drains). Logical state is
// unchanged — subsequent drains, probes, and restores are unaffected.
int rw_join_compact(void* h, int side, uint64_t* reclaimed) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    int rcp = j->pending_flush();
    if (rcp != RW_OK) return rcp;
    HIP_TRY(hipStreamSynchronize(j->stream));
    auto& sd = j->side[side];
    uint32_t cur = 0, kcur = 0, dn = 0;
    HIP_TRY(hipMemcpy(&cur, sd.row_cursor, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&kcur, sd.killed_cursor, 4, hipMemcpyDeviceToHost));
    if (sd.deg_dirty_n)
        HIP_TRY(hipMemcpy(&dn, sd.deg_dirty_n, 4, hipMemcpyDeviceToHost));
    if (kcur || dn)
        FAIL(RW_E_INVAL,
             "compact requires drained deltas (checkpoint + degree drain "
             "first: %u kills, %u degree deltas pending)", kcur, dn);
    if (j->flush_mark[side] != cur)
        FAIL(RW_E_INVAL, "compact requires a drained state table "
                         "(%u undrained fresh rows)",
             cur - j->flush_mark[side]);
    if (cur > sd.row_cap) cur = sd.row_cap;
    if (!j->compact_scratch[side])
        HIP_TRY(j->mem.alloc(&j->compact_scratch[side],
                             (size_t)sd.row_cap * sd.row_stride));
    uint8_t* nrows = j->compact_scratch[side];
    DevOwner cur_mem;
    uint32_t* ncur = nullptr;
    HIP_TRY(cur_mem.alloc(&ncur, 4));
    HIP_TRY(hipMemsetAsync(ncur, 0, 4, j->stream));
    jcompact_copy_kernel<<<4096, 256, 0, j->stream>>>(sd, nrows, ncur, cur);
    HIP_TRY(hipMemsetAsync(sd.slots8, 0,
                           ((size_t)sd.cap_mask + 1) * 8, j->stream));
    int rcs = hipStreamSynchronize(j->stream) == hipSuccess ? RW_OK
                                                            : RW_E_INTERNAL;
    uint32_t n_alive = 0;
    if (rcs == RW_OK)
        hipMemcpy(&n_alive, ncur, 4, hipMemcpyDeviceToHost);
    cur_mem.release(&ncur);
    if (rcs != RW_OK) FAIL(RW_E_INTERNAL, "compact copy failed");
    // ping-pong: both buffers are the same size and stay owned by j->mem,
    // which tracks pointers, not slots — swapping the raw values needs no
    // bookkeeping
    j->compact_scratch[side] = sd.rows;
    sd.rows = nrows;
    HIP_TRY(hipMemcpy(sd.row_cursor, &n_alive, 4, hipMemcpyHostToDevice));
    jcompact_link_kernel<<<4096, 256, 0, j->stream>>>(sd, j->m, side,
                                                      n_alive);
    if (hipStreamSynchronize(j->stream) != hipSuccess)
        FAIL(RW_E_INTERNAL, "compact relink failed");
    j->flush_mark[side] = n_alive;
    // Rebuild the arena from the live records only (length, scan, copy,
    // word rewrite per varchar column). Until here the strings of
    // retracted / watermark-cleaned rows and the bytes appended for delete
    // rows are garbage that stays allocated.
    uint64_t arena_freed = 0;
    if (j->m.vc_mask[side] && sd.arena) {
        uint8_t* na = nullptr;
        HIP_TRY(j->mem.alloc(&na, j->arena_cap[side] +
                                  2 * VARLEN_COPY_PAD * MAX_COLS));
        uint64_t new_used = 0;
        int rcv = RW_OK;
        for (int c = 0; c < j->m.n_cols[side] && rcv == RW_OK && n_alive; c++) {
            if (!((j->m.vc_mask[side] >> c) & 1)) continue;
            rcv = j->ensure_vscratch(n_alive);
            if (rcv != RW_OK) break;
            VarlenView v{};
            v.words = (const uint64_t*)(sd.rows + 16) + c;
            v.stride = sd.row_stride / 8;
            uint32_t blocks = (n_alive + 1 + 255) / 256;
            if (blocks > 4096) blocks = 4096;
            varlen_len_kernel<<<blocks, 256, 0, j->stream>>>(v, n_alive,
                                                             j->vf.d_vlens);
            size_t tmp = 0;
            if (rocprim::exclusive_scan(nullptr, tmp, j->vf.d_vlens, j->vf.d_voffs,
                                        (uint64_t)0, (size_t)n_alive + 1,
                                        rocprim::plus<uint64_t>(),
                                        j->stream) != hipSuccess) {
                rcv = RW_E_INTERNAL;
                break;
            }
            if (j->vf.ensure_scan_tmp(tmp) != RW_OK) {
                rcv = RW_E_INTERNAL;
                break;
            }
            uint64_t total = 0;
            if (rocprim::exclusive_scan(j->vf.d_scan_tmp, tmp, j->vf.d_vlens,
                                        j->vf.d_voffs, (uint64_t)0,
                                        (size_t)n_alive + 1,
                                        rocprim::plus<uint64_t>(),
                                        j->stream) != hipSuccess ||
                hipMemcpyAsync(&total, j->vf.d_voffs + n_alive, 8,
                               hipMemcpyDeviceToHost, j->stream) != hipSuccess ||
                hipStreamSynchronize(j->stream) != hipSuccess) {
                rcv = RW_E_INTERNAL;
                break;
            }
            // every live cell owns its bytes in the old arena, so the live
            // total fits the old capacity; each column's region starts
            // unit-aligned (the copy stores whole units), which the
            // allocation's slack covers
            uint64_t base = (new_used + VARLEN_COPY_PAD - 1) &
                            ~(uint64_t)(VARLEN_COPY_PAD - 1);
            if (total)
                varlen_copy_launch(v, sd.arena, j->vf.d_voffs, n_alive, total,
                                   na + base, j->stream);
            uint32_t rblocks = (n_alive + 255) / 256;
            if (rblocks > 4096) rblocks = 4096;
            varlen_rewrite_kernel<<<rblocks, 256, 0, j->stream>>>(
                sd, c, n_alive, j->vf.d_voffs, base);
            if (hipStreamSynchronize(j->stream) != hipSuccess) {
                rcv = RW_E_INTERNAL;
                break;
            }
            new_used = base + total;
        }
        if (rcv != RW_OK) {
            j->mem.release(&na);
            FAIL(RW_E_INTERNAL, "compact: arena rebuild failed");
        }
        j->mem.release(&sd.arena);
        sd.arena = na;
        if (j->arena_used[side] > new_used)
            arena_freed = j->arena_used[side] - new_used;
        j->arena_used[side] = new_used;
    }
    if (reclaimed)
        *reclaimed = (uint64_t)(cur - n_alive) * sd.row_stride + arena_freed;
    return RW_OK;
}

int rw_join_degree_drain(void* h, int side, uint8_t** buf, uint64_t* len) {
    auto* j = (HashJoin*)h;
    if (side != 0 && side != 1) FAIL(RW_E_INVAL, "bad side");
    auto& sp = j->deg_spill[side];
    int rc = spill_export(sp, buf, len);
    if (rc != RW_OK) return rc;
    sp.clear();
    return RW_OK;
}

int rw_join_stats_reset(void* h) {
    auto* j = (HashJoin*)h;
    j->ring.harvest_all();
    j->probe_launches = 0;
    j->ring.ms_total = 0;
    j->probe_rows = 0;
    return RW_OK;
}

} // extern "C"

// ===================== GroupTopN =====================
//
// GPU restatement of stream/src/executor/top_n/group_top_n.rs (WITH_TIES =
// false). Per group the full row set lives in HBM (AoS slot + packed
// records, shared layout with the join side); the observable semantics are
// those of TopNCache<false> (top_n_cache.rs:293-520): the visible window is
// rows [offset, offset+limit) of the group in cache-key order, and each
// pushed chunk emits the ChangeBuffer-compacted window delta
// (change_buffer.rs:76-187: replace = U-pair, equal rows cancel).
//
// Kernel plan per push (stream-ordered):
//   1. touch    — find-or-insert group slots, collect the touched list
//   2. snapshot — per touched group, select the pre-chunk window (row ids)
//   3. apply    — inserts (upsert = kill old + append) / deletes; same-
//                 cache-key conflicts within the chunk run in single-row
//                 segments (host pre-pass, as in the agg/join executors)
//   4. emit     — per touched group, select the new window, merge-diff
//                 against the snapshot, reserve + write output rows
// Parallelism is across groups (2+4) and rows (1+3). Records are never
// overwritten in place, so snapshot row ids stay readable in step 4.

#define TOPN_MAX_CK 8
#define TOPN_MAX_WIN 128

struct TopMeta {
    int KW;     // group key width
    int n_cols; // input schema width
    uint8_t gk_cols[MAX_KW];
    uint8_t gk_float[MAX_KW]; // float group cols: canonicalize key words
                              // (-0.0 -> +0.0, NaN -> one pattern) so the
                              // raw-bit slot compare matches SQL equality
                              // (the reference's HashKey normalizes,
                              // common/src/hash/key.rs:517)
    int n_ck; // cache key = order_by then rest storage-key cols
    uint8_t ck_cols[TOPN_MAX_CK];
    uint8_t ck_desc[TOPN_MAX_CK];
    uint8_t ck_float[TOPN_MAX_CK];
    uint32_t offset, limit;
    uint8_t with_ties; // TopNCache<true>: window extends past limit while
                       // rows tie the limit-th row's order-by prefix
    int n_order;       // cache-key prefix length that defines a tie
};

// cache-key compare on packed records (ordered_cmp semantics: NULLs
// largest in value order, desc reverses, NaN largest among floats)
__device__ __forceinline__ int topn_cmp(const TopMeta& m, const long long* va,
                                        uint32_t nba, const long long* vb,
                                        uint32_t nbb, int ncols) {
    for (int i = 0; i < ncols; i++) {
        int c = m.ck_cols[i];
        bool na = !((nba >> c) & 1), nb = !((nbb >> c) & 1);
        int r;
        if (na || nb) {
            r = (na && nb) ? 0 : (na ? 1 : -1);
        } else if (m.ck_float[i]) {
            double da = __longlong_as_double(va[c]);
            double db = __longlong_as_double(vb[c]);
            bool an = isnan(da), bn = isnan(db);
            if (an || bn) r = an == bn ? 0 : (an ? 1 : -1);
            else r = da < db ? -1 : (da > db ? 1 : 0);
        } else {
            r = va[c] < vb[c] ? -1 : (va[c] > vb[c] ? 1 : 0);
        }
        if (m.ck_desc[i]) r = -r;
        if (r) return r;
    }
    return 0;
}

__device__ __forceinline__ bool topn_ck_eq_batch(const TopMeta& m,
                                                 const JoinBatchDev& b,
                                                 uint32_t r, const long long* v,
                                                 uint32_t nb) {
    for (int i = 0; i < m.n_ck; i++) {
        int c = m.ck_cols[i];
        bool bn = !b.col_valid[c][r];
        bool rn = !((nb >> c) & 1);
        if (bn != rn) return false;
        if (!bn && b.col_vals[c][r] != v[c]) return false;
    }
    return true;
}

// canonicalize a float group-key word: -0.0 -> +0.0, every NaN -> the
// canonical quiet pattern — SQL equality for the raw-bit slot compare
__device__ __forceinline__ int64_t fkey_canon(int64_t w) {
    double d = __longlong_as_double((long long)w);
    if (d == 0.0) return 0;
    if (d != d) return 0x7ff8000000000000LL;
    return w;
}

__device__ __forceinline__ int64_t topn_gkw(const TopMeta& m, int i,
                                            int64_t v) {
    return m.gk_float[i] ? fkey_canon(v) : v;
}

__global__ void topn_touch_kernel(JoinBatchDev b, JoinSideDev sd, TopMeta m,
                                  uint32_t* touched, uint32_t* touched_list,
                                  uint32_t* counters /*0=tcur 1=err*/) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < b.n_rows;
         r += stride) {
        if (b.vis && !b.vis[r]) continue;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.gk_cols[i];
            bool valid = b.col_valid[col][r];
            kw[i] = valid ? topn_gkw(m, i, b.col_vals[col][r]) : 0;
            nullmask |= (!valid) << i;
        }
        uint32_t slot =
            jslot_find_or_insert(sd.slots, sd.cap_mask, kw, nullmask, m.KW);
        if (slot == UINT32_MAX) {
            atomicExch(&counters[1], 2u);
            continue;
        }
        if (ld_u32(&touched[slot]) == 0 &&
            atomicCAS(&touched[slot], 0u, 1u) == 0u)
            touched_list[atomicAdd(&counters[0], 1u)] = slot;
    }
}

// select the first (offset+limit) rows of a chain in cache-key order;
// returns count. O(chain * K) insertion selection — the window is small.
__device__ int topn_select(const JoinSideDev& sd, const TopMeta& m,
                           uint32_t slot, uint32_t* sel, int K) {
    int n = 0;
    uint32_t row = sd.slots[slot].head;
    while (row != UINT32_MAX) {
        JoinRowHdr* h = jrow(sd, row);
        if (h->alive) {
            const long long* v = jvals(h);
            int pos = n;
            while (pos > 0) {
                JoinRowHdr* hp = jrow(sd, sel[pos - 1]);
                if (topn_cmp(m, jvals(hp), hp->validbits, v, h->validbits,
                             m.n_ck) <= 0)
                    break;
                pos--;
            }
            if (pos < K) {
                int last = n < K ? n : K - 1;
                for (int k = last; k > pos; k--) sel[k] = sel[k - 1];
                sel[pos] = row;
                if (n < K) n++;
            }
        }
        row = h->next;
    }
    return n;
}

// full visible window incl. WITH TIES extension (ties on the order-by
// prefix of the limit-th row, TopNCache<true>; offset == 0 with ties).
// Safe-overflow argument: sel is sorted by full cache key and the sort
// prefix is a key prefix, so prefixes are non-decreasing along sel and any
// row dropped by the bounded selection is ≥ the last kept row — once the
// tie trim stops before the buffer end, no dropped row can tie. Only a tie
// group consuming the ENTIRE buffer is unrepresentable → error 5.
__device__ int topn_window(const JoinSideDev& sd, const TopMeta& m,
                           uint32_t slot, uint32_t* sel, uint32_t* err) {
    if (!m.with_ties)
        return topn_select(sd, m, slot, sel, (int)(m.offset + m.limit));
    int n = topn_select(sd, m, slot, sel, TOPN_MAX_WIN);
    if (n <= (int)m.limit) return n;
    JoinRowHdr* hc = jrow(sd, sel[m.limit - 1]);
    int nw = (int)m.limit;
    while (nw < n) {
        JoinRowHdr* h = jrow(sd, sel[nw]);
        if (topn_cmp(m, jvals(h), h->validbits, jvals(hc), hc->validbits,
                     m.n_order) != 0)
            break;
        nw++;
    }
    if (nw == TOPN_MAX_WIN) atomicExch(err, 5u); // ties window overflow
    return nw;
}

__global__ void topn_snapshot_kernel(JoinSideDev sd, TopMeta m,
                                     const uint32_t* touched_list,
                                     const uint32_t* counters,
                                     uint32_t* old_win, uint32_t* old_n,
                                     uint32_t* err) {
    int K = m.with_ties ? TOPN_MAX_WIN : (int)(m.offset + m.limit);
    uint32_t nt = counters[0];
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt;
         t += stride) {
        uint32_t sel[TOPN_MAX_WIN];
        int n = topn_window(sd, m, touched_list[t], sel, err);
        // visible window = positions [offset, offset+limit) (+ ties)
        int w0 = n < (int)m.offset ? n : (int)m.offset;
        old_n[t] = (uint32_t)(n - w0);
        for (int i = w0; i < n; i++)
            old_win[(size_t)t * K + (i - w0)] = sel[i];
    }
}

__global__ void topn_apply_kernel(JoinBatchDev b, JoinSideDev sd, TopMeta m,
                                  uint32_t r0, uint32_t r1,
                                  uint32_t* counters /*1=err*/) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1;
         r += stride) {
        if (b.vis && !b.vis[r]) continue;
        int64_t kw[MAX_KW];
        uint32_t nullmask = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.gk_cols[i];
            bool valid = b.col_valid[col][r];
            kw[i] = valid ? topn_gkw(m, i, b.col_vals[col][r]) : 0;
            nullmask |= (!valid) << i;
        }
        uint32_t slot =
            jslot_find_cached(sd.slots, sd.cap_mask, kw, nullmask, m.KW);
        if (slot == UINT32_MAX) continue; // touch pass created it
        uint8_t op = b.ops[r];
        bool is_insert = (op == RW_OP_INSERT || op == RW_OP_UPDATE_INSERT);
        // find the alive row with this cache key (sc1 loads: the chain
        // mutates within this launch; same-ck rows run in their own
        // segments, so the kill/append below is race-free)
        uint32_t row = ld_u32(&sd.slots[slot].head);
        while (row != UINT32_MAX) {
            JoinRowHdr* h = jrow(sd, row);
            uint32_t vb = ld_u32(&h->validbits);
            if (ld_u32(&h->alive) &&
                topn_ck_eq_batch(m, b, r, jvals(h), vb)) {
                st_u32(&h->alive, 0); // upsert kills the old record
                if (sd.killed) {
                    uint32_t kidx = atomicAdd(sd.killed_cursor, 1u);
                    if (kidx < sd.killed_cap) sd.killed[kidx] = row;
                }
                break;
            }
            row = ld_u32(&h->next);
        }
        if (!is_insert) continue;
        // wave-aggregated reservation (single hot counter, see jown_insert)
        uint64_t wmask = __ballot(true);
        int lane = threadIdx.x & 63;
        int leader = 63 - __clzll(wmask);
        uint32_t base = 0;
        if (lane == leader)
            base = atomicAdd(sd.row_cursor, (uint32_t)__popcll(wmask));
        base = (uint32_t)__shfl((int)base, leader);
        uint32_t nrow = base + (uint32_t)__popcll(wmask & ((1ULL << lane) - 1));
        if (nrow >= sd.row_cap) {
            atomicExch(&counters[1], 3u);
            continue;
        }
        JoinRowHdr* h = jrow(sd, nrow);
        uint32_t vb = 0;
        long long* hv = jvals(h);
        for (int c = 0; c < m.n_cols; c++) {
            st_i64((int64_t*)&hv[c], b.col_vals[c][r]);
            vb |= (uint32_t)(b.col_valid[c][r] != 0) << c;
        }
        st_u32(&h->validbits, vb);
        st_u32(&h->alive, 1);
        uint32_t* headp = &sd.slots[slot].head;
        uint32_t old_head = ld_u32(headp);
        for (;;) {
            st_u32(&h->next, old_head);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // R1 drain
            uint32_t prev = atomicCAS(headp, old_head, nrow);
            if (prev == old_head) break;
            old_head = prev;
        }
    }
}

__global__ void topn_emit_kernel(JoinSideDev sd, TopMeta m,
                                 const uint32_t* touched_list,
                                 const uint32_t* tcounters, uint32_t* touched,
                                 const uint32_t* old_win,
                                 const uint32_t* old_n, JoinOutDev out,
                                 int n_cols, uint32_t* err) {
    int K = m.with_ties ? TOPN_MAX_WIN : (int)(m.offset + m.limit);
    uint32_t nt = tcounters[0];
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt;
         t += stride) {
        uint32_t slot = touched_list[t];
        touched[slot] = 0;
        uint32_t selbuf[TOPN_MAX_WIN];
        int nsel = topn_window(sd, m, slot, selbuf, err);
        // visible window = positions [offset, offset+limit)
        int w0 = nsel < (int)m.offset ? nsel : (int)m.offset;
        const uint32_t* neww = selbuf + w0;
        int nn = nsel - w0;
        const uint32_t* oldw = old_win + (size_t)t * K;
        int no = (int)old_n[t];
        // merge-diff into local delta lists: op + row id (+ paired old id)
        uint8_t dop[2 * TOPN_MAX_WIN];
        uint32_t drow[2 * TOPN_MAX_WIN];
        int nd = 0;
        int i = 0, j = 0;
        while (i < no || j < nn) {
            int c;
            if (i >= no) c = 1;
            else if (j >= nn) c = -1;
            else {
                JoinRowHdr* ho = jrow(sd, oldw[i]);
                JoinRowHdr* hn = jrow(sd, neww[j]);
                c = topn_cmp(m, jvals(ho), ho->validbits, jvals(hn),
                             hn->validbits, m.n_ck);
            }
            if (c == 0) {
                if (oldw[i] != neww[j]) {
                    // same cache key, different record: replaced. Equal
                    // rows cancel (ChangeBuffer no-op filter).
                    JoinRowHdr* ho = jrow(sd, oldw[i]);
                    JoinRowHdr* hn = jrow(sd, neww[j]);
                    bool eq = ho->validbits == hn->validbits;
                    const long long* vo = jvals(ho);
                    const long long* vn = jvals(hn);
                    for (int cc = 0; eq && cc < n_cols; cc++)
                        if (((ho->validbits >> cc) & 1) && vo[cc] != vn[cc])
                            eq = false;
                    if (!eq) {
                        dop[nd] = RW_OP_UPDATE_DELETE;
                        drow[nd++] = oldw[i];
                        dop[nd] = RW_OP_UPDATE_INSERT;
                        drow[nd++] = neww[j];
                    }
                }
                i++;
                j++;
            } else if (c < 0) {
                dop[nd] = RW_OP_DELETE;
                drow[nd++] = oldw[i];
                i++;
            } else {
                dop[nd] = RW_OP_INSERT;
                drow[nd++] = neww[j];
                j++;
            }
        }
        if (!nd) continue;
        uint32_t base = atomicAdd(&out.counters[0], (uint32_t)nd);
        if (base + nd > out.cap) {
            atomicExch(&out.counters[1], 1u);
            continue;
        }
        for (int k = 0; k < nd; k++) {
            uint32_t orow = base + k;
            JoinRowHdr* h = jrow(sd, drow[k]);
            const long long* v = jvals(h);
            out.ops[orow] = dop[k];
            for (int c = 0; c < n_cols; c++) {
                bool valid = (h->validbits >> c) & 1;
                out.vals[(size_t)orow * n_cols + c] = valid ? v[c] : 0;
                out.nulls[(size_t)orow * n_cols + c] = !valid;
            }
        }
    }
}

// GroupTopN watermark state cleaning (group_top_n.rs:266-273: a watermark
// on group_by[0] becomes a state-table watermark = range delete on the
// store). Rows of groups below the watermark are retired in place and
// routed through the kill list so the next drain nets them to DELETE
// frames (slots stay READY; a late row restarts the group).
__global__ void topn_clean_kernel(JoinSideDev sd, int kpos, long long wm) {
    size_t cap = (size_t)sd.cap_mask + 1;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cap;
         slot += stride) {
        if (sd.slots[slot].state != SLOT_READY) continue;
        if ((sd.slots[slot].nulls >> kpos) & 1) continue; // NULLs largest
        if (sd.slots[slot].key[kpos] >= wm) continue;
        uint32_t row = sd.slots[slot].head;
        while (row != UINT32_MAX) {
            JoinRowHdr* h = jrow(sd, row);
            if (h->alive) {
                h->alive = 0;
                if (sd.killed) {
                    uint32_t kidx = atomicAdd(sd.killed_cursor, 1u);
                    if (kidx < sd.killed_cap) sd.killed[kidx] = row;
                }
            }
            row = h->next;
        }
    }
}

// §8f-4 memory reclamation (TopN): relink packed records into freshly
// initialized group slots (jcompact_copy_kernel packs; this rebuilds the
// chains — netted keys need not be unique here, concurrent pushes on one
// group resolve by CAS).
__global__ void topn_relink_kernel(JoinSideDev sd, TopMeta m, uint32_t n,
                                   uint32_t* err) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        JoinRowHdr* h = jrow(sd, r);
        uint32_t vb = h->validbits;
        int64_t kw[MAX_KW];
        uint32_t nm = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.gk_cols[i];
            bool valid = (vb >> col) & 1;
            kw[i] = valid ? topn_gkw(m, i, jvals(h)[col]) : 0;
            nm |= (uint32_t)(!valid) << i;
        }
        uint32_t slot =
            jslot_find_or_insert(sd.slots, sd.cap_mask, kw, nm, m.KW);
        if (slot == UINT32_MAX) {
            atomicExch(err, 2u);
            continue;
        }
        uint32_t* headp = &sd.slots[slot].head;
        uint32_t old_head = ld_u32(headp);
        for (;;) {
            st_u32(&h->next, old_head);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // R1 drain
            uint32_t prev = atomicCAS(headp, old_head, r);
            if (prev == old_head) break;
            old_head = prev;
        }
    }
}

// §8f-5 recovery: rebuild the TopN state table from a netted spill replay.
// Each restored row is appended to the record store and chained onto its
// group's slot (cache keys in the netted map are unique, so no same-key
// conflicts; concurrent head pushes on one group resolve by CAS).
__global__ void topn_restore_kernel(JoinBatchDev b, JoinSideDev sd, TopMeta m,
                                    uint32_t* err) {
    uint32_t stride = gridDim.x * blockDim.x;
    int lane = threadIdx.x & 63;
    uint32_t n = b.n_rows;
    uint32_t iters = (n + stride - 1) / stride;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r < n;
        uint64_t wmask = __ballot(active);
        if (!active) continue;
        int leader = 63 - __clzll(wmask);
        uint32_t base = 0;
        if (lane == leader)
            base = atomicAdd(sd.row_cursor, (uint32_t)__popcll(wmask));
        base = (uint32_t)__shfl((int)base, leader);
        uint32_t row = base + (uint32_t)__popcll(wmask & ((1ULL << lane) - 1));
        if (row >= sd.row_cap) {
            atomicExch(err, 3u);
            continue;
        }
        JoinRowHdr* h = jrow(sd, row);
        long long* hv = jvals(h);
        uint32_t vb = 0;
        for (int c = 0; c < m.n_cols; c++) {
            hv[c] = b.col_vals[c][r];
            vb |= (uint32_t)(b.col_valid[c][r] != 0) << c;
        }
        h->validbits = vb;
        h->degree = 0;
        h->alive = 1;
        int64_t kw[MAX_KW];
        uint32_t nm = 0;
        for (int i = 0; i < m.KW; i++) {
            uint8_t col = m.gk_cols[i];
            bool valid = (vb >> col) & 1;
            kw[i] = valid ? topn_gkw(m, i, hv[col]) : 0;
            nm |= (uint32_t)(!valid) << i;
        }
        uint32_t slot =
            jslot_find_or_insert(sd.slots, sd.cap_mask, kw, nm, m.KW);
        if (slot == UINT32_MAX) {
            atomicExch(err, 2u);
            continue;
        }
        uint32_t* headp = &sd.slots[slot].head;
        uint32_t old_head = ld_u32(headp);
        for (;;) {
            st_u32(&h->next, old_head);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // R1 drain
            uint32_t prev = atomicCAS(headp, old_head, row);
            if (prev == old_head) break;
            old_head = prev;
        }
    }
}

struct GroupTopN {
    TopMeta m{};
    JoinSideDev sd{};
    JoinBatchDev stage{};
    uint32_t stage_cap = 0;
    JoinOutDev out{};
    uint32_t* touched = nullptr;     // [slot cap]
    uint32_t* touched_list = nullptr;
    uint32_t* tcounters = nullptr; // 0=tcursor 1=err
    uint32_t* old_win = nullptr;
    uint32_t* old_n = nullptr;
    uint32_t old_cap = 0; // touched capacity for old_win/old_n
    DevOwner mem; // every device buffer of this executor (rw_devmem.hpp)
    std::vector<uint8_t> types;
    std::vector<uint32_t> ck_col_idx;
    uint32_t chunk_size;
    hipStream_t stream = nullptr;
    rwchunk::ChunkQueue outq;

    int init(const RwGroupTopNDesc* d) {
        if (!gpu_ok())
            FAIL(RW_E_NOGPU,
                 "risingwave_amd: no GPU visible (product path has no CPU fallback)");
        if (!d->limit) FAIL(RW_E_INVAL, "limit must be > 0");
        if (d->offset + d->limit > TOPN_MAX_WIN)
            FAIL(RW_E_INVAL, "offset+limit > %d unsupported", TOPN_MAX_WIN);
        if (d->n_group_by > MAX_KW)
            FAIL(RW_E_INVAL, "group_by width 0..%d", MAX_KW);
        // n_group_by == 0 = the plain TopN executor (top_n_plain.rs): every
        // row lands in the single empty-key group
        if (d->n_order_by + d->n_rest > TOPN_MAX_CK)
            FAIL(RW_E_INVAL, "cache key width > %d", TOPN_MAX_CK);
        if (d->n_cols > MAX_COLS) FAIL(RW_E_INVAL, "n_cols > %d", MAX_COLS);
        types.assign(d->types, d->types + d->n_cols);
        for (auto t : types)
            if (t != RW_T_I64 && t != RW_T_TS && t != RW_T_F64)
                FAIL(RW_E_INVAL, "GroupTopN supports 8-byte datum columns");
        m.KW = (int)d->n_group_by;
        m.n_cols = (int)d->n_cols;
        for (uint32_t i = 0; i < d->n_group_by; i++) {
            m.gk_cols[i] = (uint8_t)d->group_by[i];
            m.gk_float[i] = types[d->group_by[i]] == RW_T_F64;
        }
        m.n_ck = (int)(d->n_order_by + d->n_rest);
        int k = 0;
        for (uint32_t i = 0; i < d->n_order_by; i++, k++) {
            m.ck_cols[k] = (uint8_t)d->order_cols[i];
            m.ck_desc[k] = d->order_desc[i];
            m.ck_float[k] = types[d->order_cols[i]] == RW_T_F64;
            ck_col_idx.push_back(d->order_cols[i]);
        }
        for (uint32_t i = 0; i < d->n_rest; i++, k++) {
            m.ck_cols[k] = (uint8_t)d->rest_cols[i];
            m.ck_desc[k] = d->rest_desc[i];
            m.ck_float[k] = types[d->rest_cols[i]] == RW_T_F64;
            ck_col_idx.push_back(d->rest_cols[i]);
        }
        m.offset = (uint32_t)d->offset;
        m.limit = (uint32_t)d->limit;
        m.with_ties = d->with_ties;
        m.n_order = (int)d->n_order_by;
        if (d->with_ties && d->offset)
            FAIL(RW_E_INVAL, "offset unsupported WITH TIES (as in the reference)");
        chunk_size = d->chunk_size ? d->chunk_size : 1024;

        uint64_t cap_hint = d->state_capacity_hint ? d->state_capacity_hint
                                                   : (1ull << 14);
        size_t cap = 1;
        while (cap < cap_hint * 2) cap <<= 1;
        sd.cap_mask = (uint32_t)(cap - 1);
        uint64_t row_cap = d->row_capacity_hint ? d->row_capacity_hint
                                                : (1ull << 20);
        sd.row_stride = 16 + 8u * (uint32_t)m.n_cols;
        sd.row_cap = (uint32_t)row_cap;
        HIP_TRY(hipStreamCreate(&stream));
        HIP_TRY(mem.alloc(&sd.slots, cap * sizeof(JoinSlot)));
        HIP_TRY(mem.alloc(&sd.rows, (size_t)row_cap * sd.row_stride));
        HIP_TRY(mem.alloc(&sd.row_cursor, 4));
        HIP_TRY(hipMemset(sd.row_cursor, 0, 4));
        sd.killed_cap = 1u << 22; // checkpoint-delta tracking (§8f-2)
        HIP_TRY(mem.alloc(&sd.killed, (size_t)sd.killed_cap * 4));
        HIP_TRY(mem.alloc(&sd.killed_cursor, 4));
        HIP_TRY(hipMemset(sd.killed_cursor, 0, 4));
        HIP_TRY(mem.alloc(&touched, cap * 4));
        HIP_TRY(hipMemset(touched, 0, cap * 4));
        HIP_TRY(mem.alloc(&tcounters, 8));
        jslot_init_kernel<<<2048, 256, 0, stream>>>(sd.slots, cap);
        uint32_t out_cap = 1 << 18;
        out.cap = out_cap;
        HIP_TRY(mem.alloc(&out.vals, (size_t)out_cap * m.n_cols * 8));
        HIP_TRY(mem.alloc(&out.nulls, (size_t)out_cap * m.n_cols));
        HIP_TRY(mem.alloc(&out.ops, out_cap));
        HIP_TRY(mem.alloc(&out.counters, 8));
        HIP_TRY(hipMemset(out.counters, 0, 8));
        HIP_TRY(hipStreamSynchronize(stream));
        return RW_OK;
    }

    ~GroupTopN() {
        mem.release_all(); // device memory goes before the stream
        if (stream) hipStreamDestroy(stream);
    }

    int ensure_caps(uint32_t n) {
        if (stage_cap < n) {
            stage_cap = 0;
            int rc = stage_regrow(mem, stage, m.n_cols, n, 8);
            if (rc != RW_OK) return rc;
            stage_cap = n;
        }
        if (old_cap < n) {
            old_cap = 0;
            mem.release(&touched_list);
            mem.release(&old_win);
            mem.release(&old_n);
            int K = m.with_ties ? TOPN_MAX_WIN : (int)(m.offset + m.limit);
            HIP_TRY(mem.alloc(&touched_list, (size_t)n * 4));
            HIP_TRY(mem.alloc(&old_win, (size_t)n * K * 4));
            HIP_TRY(mem.alloc(&old_n, (size_t)n * 4));
            old_cap = n;
        }
        return RW_OK;
    }

    // same-cache-key rows within one chunk run in their own single-row
    // segments (the reference applies rows in order, group_top_n.rs:168)
    std::vector<uint32_t> conflict_segments(const RwChunk* c) {
        std::vector<uint32_t> bounds;
        std::unordered_map<std::string, int> ck_count;
        auto ck_of = [&](uint32_t r) {
            std::string k;
            for (auto col : ck_col_idx) {
                uint8_t valid = c->cols[col].valid[r];
                k.push_back((char)valid);
                int64_t v = valid ? ((const int64_t*)c->cols[col].data)[r] : 0;
                k.append((const char*)&v, 8);
            }
            return k;
        };
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            ck_count[ck_of(r)]++;
        }
        bool any = false;
        for (auto& kv : ck_count)
            if (kv.second > 1) {
                any = true;
                break;
            }
        if (!any) return bounds;
        for (uint32_t r = 0; r < c->n_rows; r++) {
            if (c->vis && !c->vis[r]) continue;
            if (ck_count[ck_of(r)] > 1) {
                bounds.push_back(r);
                bounds.push_back(r + 1);
            }
        }
        return bounds;
    }

    int push_chunk(const RwChunk* c) {
        uint32_t n = c->n_rows;
        if (!n) return RW_OK;
        if (ensure_caps(n) != RW_OK) return RW_E_INTERNAL;
        JoinBatchDev b = stage;
        for (int i = 0; i < m.n_cols; i++) {
            int rc = upload_col(b.col_vals[i], b.col_valid[i], c->cols[i].data,
                                c->cols[i].valid, n, 8, stream);
            if (rc != RW_OK) return rc;
        }
        int rc = upload_ops_vis(b, c, stream);
        if (rc != RW_OK) return rc;
        HIP_TRY(hipMemsetAsync(tcounters, 0, 8, stream));

        topn_touch_kernel<<<grid_for(n), 256, 0, stream>>>(
            b, sd, m, touched, touched_list, tcounters);
        topn_snapshot_kernel<<<256, 256, 0, stream>>>(
            sd, m, touched_list, tcounters, old_win, old_n, tcounters + 1);
        auto segs = conflict_segments(c);
        uint32_t start = 0;
        auto launch_apply = [&](uint32_t a, uint32_t z) {
            if (z <= a) return;
            topn_apply_kernel<<<grid_for(z - a), 256, 0, stream>>>(b, sd, m, a, z,
                                                                   tcounters);
        };
        for (uint32_t bnd : segs) {
            launch_apply(start, bnd);
            start = bnd;
        }
        launch_apply(start, n);
        topn_emit_kernel<<<256, 256, 0, stream>>>(sd, m, touched_list,
                                                  tcounters, touched, old_win,
                                                  old_n, out, m.n_cols,
                                                  tcounters + 1);
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t tc[2];
        HIP_TRY(hipMemcpy(tc, tcounters, 8, hipMemcpyDeviceToHost));
        if (tc[1] == 2) FAIL(RW_E_INTERNAL, "group table full");
        if (tc[1] == 3) FAIL(RW_E_INTERNAL, "row store full");
        if (tc[1] == 5)
            FAIL(RW_E_INTERNAL, "WITH TIES window exceeds %d rows", TOPN_MAX_WIN);
        return drain_output();
    }

    int drain_output() {
        uint32_t ctr[2];
        HIP_TRY(hipMemcpy(ctr, out.counters, 8, hipMemcpyDeviceToHost));
        if (ctr[1] == 1) FAIL(RW_E_INTERNAL, "topn output overflow");
        uint32_t n_out = ctr[0];
        if (n_out) {
            std::vector<int64_t> vals((size_t)n_out * m.n_cols);
            std::vector<uint8_t> nulls((size_t)n_out * m.n_cols);
            std::vector<uint8_t> ops(n_out);
            HIP_TRY(hipMemcpy(vals.data(), out.vals, vals.size() * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(nulls.data(), out.nulls, nulls.size(),
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ops.data(), out.ops, n_out,
                              hipMemcpyDeviceToHost));
            // chunk_size rows each (at least 2), U-/U+ pairs kept together
            uint32_t max_rows = chunk_size < 2 ? 2 : chunk_size;
            for (auto [s, take] :
                 rwchunk::slice_ranges(n_out, max_rows, ops.data())) {
                rwchunk::Builder cb(take, (uint32_t)m.n_cols);
                for (int ci = 0; ci < m.n_cols; ci++) {
                    size_t ix = (size_t)s * m.n_cols + ci;
                    cb.fixed(types[ci], &vals[ix], m.n_cols,
                             rwchunk::from_nulls(&nulls[ix], m.n_cols));
                }
                cb.ops(&ops[s]);
                outq.push(cb.release());
            }
        }
        HIP_TRY(hipMemset(out.counters, 0, 8));
        return RW_OK;
    }

    // §8f-4 memory reclamation: pack alive records, reinit the slot
    // table, relink chains. Requires a drained table (kill list consumed,
    // flush mark at the cursor); logical state is unchanged.
    uint8_t* compact_scratch = nullptr;
    int compact(uint64_t* reclaimed) {
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t cur = 0, kcur = 0;
        HIP_TRY(hipMemcpy(&cur, sd.row_cursor, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&kcur, sd.killed_cursor, 4,
                          hipMemcpyDeviceToHost));
        if (kcur)
            FAIL(RW_E_INVAL,
                 "compact requires a drained kill list (%u pending)", kcur);
        if (flush_mark != cur)
            FAIL(RW_E_INVAL, "compact requires a drained state table "
                             "(%u undrained fresh rows)", cur - flush_mark);
        if (cur > sd.row_cap) cur = sd.row_cap;
        if (!compact_scratch)
            HIP_TRY(mem.alloc(&compact_scratch,
                              (size_t)sd.row_cap * sd.row_stride));
        DevOwner tmp;
        uint32_t* ncur = nullptr;
        HIP_TRY(tmp.alloc(&ncur, 4));
        HIP_TRY(hipMemsetAsync(ncur, 0, 4, stream));
        jcompact_copy_kernel<<<4096, 256, 0, stream>>>(sd, compact_scratch,
                                                       ncur, cur);
        jslot_init_kernel<<<2048, 256, 0, stream>>>(
            sd.slots, (size_t)sd.cap_mask + 1);
        int rcs = hipStreamSynchronize(stream) == hipSuccess
                      ? RW_OK : RW_E_INTERNAL;
        uint32_t n_alive = 0;
        if (rcs == RW_OK)
            hipMemcpy(&n_alive, ncur, 4, hipMemcpyDeviceToHost);
        tmp.release(&ncur);
        if (rcs != RW_OK) FAIL(RW_E_INTERNAL, "topn compact copy failed");
        // ping-pong: both stay owned by `mem`, which tracks pointers and
        // not slots, so swapping the raw values needs no bookkeeping
        std::swap(sd.rows, compact_scratch);
        HIP_TRY(hipMemcpy(sd.row_cursor, &n_alive, 4,
                          hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(tcounters, 0, 8, stream));
        topn_relink_kernel<<<grid_for(n_alive), 256, 0, stream>>>(
            sd, m, n_alive, tcounters + 1);
        if (hipStreamSynchronize(stream) != hipSuccess)
            FAIL(RW_E_INTERNAL, "topn compact relink failed");
        uint32_t tc[2];
        HIP_TRY(hipMemcpy(tc, tcounters, 8, hipMemcpyDeviceToHost));
        if (tc[1]) FAIL(RW_E_INTERNAL, "topn compact overflow (%u)", tc[1]);
        flush_mark = n_alive;
        if (reclaimed)
            *reclaimed = (uint64_t)(cur - n_alive) * sd.row_stride;
        return RW_OK;
    }

    // §8f-2 checkpoint spill: the TopN state table's per-epoch KV deltas —
    // key = memcomparable storage key (group cols ASC, then the cache-key
    // cols with their declared orders), value = value-encoded full row;
    // same kill-list netting and record framing as the join drain.
    uint32_t flush_mark = 0;
    std::vector<uint8_t> ck_desc_host;
    int checkpoint_drain(std::vector<uint8_t>& sp) {
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t cur = 0, kcur = 0;
        HIP_TRY(hipMemcpy(&cur, sd.row_cursor, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&kcur, sd.killed_cursor, 4, hipMemcpyDeviceToHost));
        if (kcur > sd.killed_cap)
            FAIL(RW_E_INTERNAL, "topn kill list overflow (lost deltas)");
        if (cur > sd.row_cap) cur = sd.row_cap;
        size_t stride = sd.row_stride;
        std::vector<uint8_t> fresh((size_t)(cur - flush_mark) * stride);
        if (cur > flush_mark)
            HIP_TRY(hipMemcpy(fresh.data(),
                              sd.rows + (size_t)flush_mark * stride,
                              fresh.size(), hipMemcpyDeviceToHost));
        std::vector<uint32_t> kills(kcur);
        if (kcur)
            HIP_TRY(hipMemcpy(kills.data(), sd.killed, (size_t)kcur * 4,
                              hipMemcpyDeviceToHost));
        auto encode_key = [&](HostRow row) {
            std::vector<uint8_t> k;
            for (int i = 0; i < m.KW; i++) {
                uint8_t col = m.gk_cols[i];
                rwcodec::memcmp_encode_datum(k, types[col],
                                             row.datum(types[col], col), {});
            }
            for (int i = 0; i < m.n_ck; i++) {
                uint8_t col = m.ck_cols[i];
                rwcodec::OrderType ot;
                ot.desc = m.ck_desc[i] != 0;
                rwcodec::memcmp_encode_datum(k, types[col],
                                             row.datum(types[col], col), ot);
            }
            return k;
        };
        auto encode_val = [&](HostRow row) {
            std::vector<uint8_t> v;
            for (int c = 0; c < m.n_cols; c++)
                rwcodec::value_encode_datum(v, types[c],
                                            row.datum(types[c], c));
            return v;
        };
        rwcodec::KeyedDelta delta;
        std::vector<uint8_t> oldrec(stride);
        for (uint32_t i = 0; i < kcur; i++) {
            if (kills[i] >= flush_mark) continue;
            HIP_TRY(hipMemcpy(oldrec.data(),
                              sd.rows + (size_t)kills[i] * stride, stride,
                              hipMemcpyDeviceToHost));
            delta.del(encode_key({oldrec.data()}));
        }
        for (uint32_t i = flush_mark; i < cur; i++) {
            HostRow row{fresh.data() + (size_t)(i - flush_mark) * stride};
            if (row.hdr().alive) delta.put(encode_key(row), encode_val(row));
        }
        delta.write(sp);
        HIP_TRY(hipMemset(sd.killed_cursor, 0, 4));
        flush_mark = cur;
        return RW_OK;
    }

    // §8f-5 recovery: replay one or more concatenated epoch drains into a
    // fresh executor. PUT/DELETE frames net host-side (last write wins, as a
    // KV store compaction would); the surviving rows rebuild the device
    // state and are marked persisted so the next drain does not re-PUT them.
    int restore(const uint8_t* buf, uint64_t len) {
        rwcodec::FrameMap merged;
        if (!rwcodec::merge_frames(buf, len, merged))
            FAIL(RW_E_INVAL, "malformed spill stream");
        uint32_t n = (uint32_t)merged.size();
        if (!n) return RW_OK;
        int ncols = m.n_cols;
        std::vector<std::vector<int64_t>> cols(ncols, std::vector<int64_t>(n));
        std::vector<std::vector<uint8_t>> valid(ncols, std::vector<uint8_t>(n));
        uint32_t i = 0;
        for (auto& [kbytes, val] : merged) {
            (void)kbytes;
            rwcodec::RowReader rd{val.data(), val.size()};
            for (int c = 0; c < ncols; c++) {
                rwcodec::DatumC d;
                if (!rd.datum(types[c], &d))
                    FAIL(RW_E_INVAL, "restore: bad row datum");
                cols[c][i] = d.null ? 0 : rwcodec::word_of_datum(types[c], d);
                valid[c][i] = !d.null;
            }
            i++;
        }
        int rc = ensure_caps(n);
        if (rc != RW_OK) return rc;
        JoinBatchDev b = stage;
        for (int c = 0; c < ncols; c++) {
            HIP_TRY(hipMemcpy(b.col_vals[c], cols[c].data(), (size_t)n * 8,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(b.col_valid[c], valid[c].data(), n,
                              hipMemcpyHostToDevice));
        }
        b.vis = nullptr;
        b.n_rows = n;
        HIP_TRY(hipMemset(tcounters, 0, 8));
        topn_restore_kernel<<<grid_for(n), 256, 0, stream>>>(b, sd, m,
                                                             tcounters + 1);
        if (hipStreamSynchronize(stream) != hipSuccess)
            FAIL(RW_E_INTERNAL, "restore sync failed");
        uint32_t tc[2];
        HIP_TRY(hipMemcpy(tc, tcounters, 8, hipMemcpyDeviceToHost));
        if (tc[1]) FAIL(RW_E_INTERNAL, "restore overflow (code %u)", tc[1]);
        uint32_t cur = 0;
        HIP_TRY(hipMemcpy(&cur, sd.row_cursor, 4, hipMemcpyDeviceToHost));
        flush_mark = cur;
        return RW_OK;
    }

    RwChunk* poll() { return outq.poll(); }
};

extern "C" {

int rw_topn_checkpoint_drain(void* h, uint8_t** buf, uint64_t* len) {
    std::vector<uint8_t> sp;
    int rc = ((GroupTopN*)h)->checkpoint_drain(sp);
    if (rc != RW_OK) return rc;
    return spill_export(sp, buf, len);
}

int rw_topn_restore(void* h, const uint8_t* buf, uint64_t len) {
    return ((GroupTopN*)h)->restore(buf, len);
}

void* rw_group_top_n_create(const RwGroupTopNDesc* d) {
    auto* t = new GroupTopN();
    if (t->init(d) != RW_OK) {
        delete t;
        return nullptr;
    }
    return t;
}

int rw_topn_compact(void* h, uint64_t* reclaimed) {
    return ((GroupTopN*)h)->compact(reclaimed);
}

// handle_watermark (group_top_n.rs:266-273): a watermark on the FIRST
// group-by column cleans the state table below it and is forwarded
// (returns 1); any other column's watermark is absorbed (returns 0).
int rw_group_top_n_watermark(void* h, uint32_t col_idx, int64_t val) {
    auto* t = (GroupTopN*)h;
    if (t->m.KW == 0 || t->m.gk_cols[0] != (uint8_t)col_idx) return 0;
    topn_clean_kernel<<<2048, 256, 0, t->stream>>>(t->sd, 0, val);
    if (hipStreamSynchronize(t->stream) != hipSuccess)
        FAIL(RW_E_INTERNAL, "topn clean sync failed");
    return 1;
}
int rw_group_top_n_push_chunk(void* h, const RwChunk* c) {
    return ((GroupTopN*)h)->push_chunk(c);
}
int rw_group_top_n_flush(void* h, uint64_t epoch) {
    (void)h;
    (void)epoch;
    return RW_OK; // emission is per push; checkpoint spill is a later row
}
RwChunk* rw_group_top_n_poll(void* h) { return ((GroupTopN*)h)->poll(); }
void rw_group_top_n_destroy(void* h) { delete (GroupTopN*)h; }

} // extern "C"

// ---------------------------------------------------------------------------
// HBM read-bandwidth probe: pins the "achievable" read rate the roofline
// `frac` is quoted against — the same b128 grid-stride load
// pattern as dense_load, reduced into a sink so nothing is eliminated.
// Measurement infrastructure, not a product path.
__global__ void membw_probe_kernel(const ulonglong2* __restrict__ p, size_t n,
                                   unsigned long long* sink) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned long long acc = 0;
    for (; i + 3 * stride < n; i += 4 * stride) {
        ulonglong2 a = p[i], b = p[i + stride], c = p[i + 2 * stride],
                   d = p[i + 3 * stride];
        acc += a.x + a.y + b.x + b.y + c.x + c.y + d.x + d.y;
    }
    for (; i < n; i += stride) acc += p[i].x + p[i].y;
    if (acc == 0xdeadbeefdeadbeefULL) *sink = acc; // never taken
}

// RANDOM-access ceiling probe: each lane chases splitmix-scattered 64-B
// lines over `bytes` of HBM — the achievable rate for the hash-join's
// probe/insert access pattern (one random line per touch), the honest
// denominator for q8's roofline discussion. Reads the first
// u64 of a random line per step; reported as GB/s of 64-B lines touched.
__global__ void membw_rand_probe_kernel(const unsigned long long* __restrict__ p,
                                        size_t n_lines, int steps_per_thread,
                                        unsigned long long* sink) {
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                     0x9e3779b97f4a7c15ULL +
                 0x243f6a8885a308d3ULL;
    unsigned long long acc = 0;
    for (int i = 0; i < steps_per_thread; i++) {
        x += 0x9e3779b97f4a7c15ULL;
        uint64_t h = x;
        h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ULL;
        h = (h ^ (h >> 27)) * 0x94d049bb133111ebULL;
        h ^= h >> 31;
        acc += p[(h % n_lines) * 8]; // 64-B line stride (8 u64)
    }
    if (acc == 0xdeadbeefdeadbeefULL) *sink = acc;
}

// random atomicAdd throughput (the insert path's slot-CAS analogue)
__global__ void membw_rand_atomic_kernel(unsigned long long* p, size_t n_lines,
                                         int steps_per_thread) {
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                     0x9e3779b97f4a7c15ULL +
                 0x243f6a8885a308d3ULL;
    for (int i = 0; i < steps_per_thread; i++) {
        x += 0x9e3779b97f4a7c15ULL;
        uint64_t h = x;
        h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ULL;
        h = (h ^ (h >> 27)) * 0x94d049bb133111ebULL;
        h ^= h >> 31;
        atomicAdd(&p[(h % n_lines) * 8], 1ull);
    }
}

// DEPENDENT random chase: each step's address depends on the previous
// load's value (the probe kernel's hash->slot->record chain shape);
// `mlp` independent chains per thread expose memory-level parallelism
__global__ void membw_rand_chase_kernel(const unsigned long long* __restrict__ p,
                                        size_t n_lines, int steps, int mlp,
                                        unsigned long long* sink) {
    uint64_t x[8];
    for (int j = 0; j < mlp && j < 8; j++)
        x[j] = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                   0x9e3779b97f4a7c15ULL +
               j * 0x94d049bb133111ebULL + 1;
    unsigned long long acc = 0;
    for (int i = 0; i < steps; i++) {
        for (int j = 0; j < mlp && j < 8; j++) {
            uint64_t h = x[j];
            h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ULL;
            h = (h ^ (h >> 27)) * 0x94d049bb133111ebULL;
            h ^= h >> 31;
            unsigned long long v = p[(h % n_lines) * 8];
            x[j] += v + 0x9e3779b97f4a7c15ULL; // DEPENDS on the load
            acc += v;
        }
    }
    if (acc == 0xdeadbeefdeadbeefULL) *sink = acc;
}

extern "C" int rw_membw_rand_atomic(uint64_t bytes, int steps_per_thread,
                                    double* gops_out) {
    size_t n_lines = bytes / 64;
    unsigned long long* p = nullptr;
    DevOwner tmp;
    if (tmp.alloc(&p, n_lines * 64) != hipSuccess) return RW_E_INTERNAL;
    (void)hipMemset(p, 0, n_lines * 64);
    int grid = 2048, blk = 256;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    membw_rand_atomic_kernel<<<grid, blk>>>(p, n_lines, steps_per_thread);
    (void)hipEventRecord(e0);
    membw_rand_atomic_kernel<<<grid, blk>>>(p, n_lines, steps_per_thread);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return RW_E_INTERNAL;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *gops_out = (double)grid * blk * steps_per_thread / (ms * 1e-3) / 1e9;
    tmp.release_all();
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return RW_OK;
}

extern "C" int rw_membw_rand_chase(uint64_t bytes, int steps, int mlp,
                                   double* glines_out) {
    size_t n_lines = bytes / 64;
    unsigned long long* p = nullptr;
    unsigned long long* sink = nullptr;
    DevOwner tmp;
    if (tmp.alloc(&p, n_lines * 64) != hipSuccess) return RW_E_INTERNAL;
    (void)tmp.alloc(&sink, 8);
    (void)hipMemset(p, 1, n_lines * 64);
    int grid = 2048, blk = 256;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    membw_rand_chase_kernel<<<grid, blk>>>(p, n_lines, steps, mlp, sink);
    (void)hipEventRecord(e0);
    membw_rand_chase_kernel<<<grid, blk>>>(p, n_lines, steps, mlp, sink);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return RW_E_INTERNAL;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *glines_out =
        (double)grid * blk * steps * mlp / (ms * 1e-3) / 1e9;
    tmp.release_all();
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return RW_OK;
}

extern "C" int rw_membw_rand_probe(uint64_t bytes, int steps_per_thread,
                                   double* glines_out, double* gbps_out) {
    size_t n_lines = bytes / 64;
    unsigned long long* p = nullptr;
    unsigned long long* sink = nullptr;
    DevOwner tmp;
    if (tmp.alloc(&p, n_lines * 64) != hipSuccess) return RW_E_INTERNAL;
    (void)tmp.alloc(&sink, 8);
    (void)hipMemset(p, 1, n_lines * 64);
    int grid = 2048, blk = 256;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    membw_rand_probe_kernel<<<grid, blk>>>(p, n_lines, steps_per_thread, sink);
    (void)hipEventRecord(e0);
    membw_rand_probe_kernel<<<grid, blk>>>(p, n_lines, steps_per_thread, sink);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return RW_E_INTERNAL;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    double touches = (double)grid * blk * steps_per_thread;
    *glines_out = touches / (ms * 1e-3) / 1e9;
    *gbps_out = touches * 64 / (ms * 1e-3) / 1e9;
    tmp.release_all();
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return RW_OK;
}

extern "C" int rw_membw_probe(uint64_t bytes, int iters, double* gbps_out) {
    size_t n = bytes / sizeof(ulonglong2);
    ulonglong2* p = nullptr;
    unsigned long long* sink = nullptr;
    DevOwner tmp;
    if (tmp.alloc(&p, n * sizeof(ulonglong2)) != hipSuccess) return RW_E_INTERNAL;
    (void)tmp.alloc(&sink, 8);
    (void)hipMemset(p, 1, n * sizeof(ulonglong2));
    int grid = 8192; // ≫256 workgroups: fills all 8 XCDs
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    membw_probe_kernel<<<grid, 256>>>(p, n, sink); // warmup
    (void)hipEventRecord(e0);
    for (int it = 0; it < iters; it++) membw_probe_kernel<<<grid, 256>>>(p, n, sink);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return RW_E_INTERNAL;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *gbps_out = (double)bytes * iters / (ms * 1e-3) / 1e9;
    tmp.release_all();
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return RW_OK;
}
