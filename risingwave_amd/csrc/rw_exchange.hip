// rw_exchange.hip — the vnode exchange/dispatch hop, MI355X-native.
//
// Replaces the reference's HashDataDispatcher → gRPC exchange → Merge chain
// (stream/src/executor/dispatch.rs:949-1050, exchange/input.rs:146,
// compute/src/rpc/service/stream_exchange_service.rs:45-160) for GPU↔GPU
// with: a device partition/compaction kernel (vnode = Crc32 row hash %
// vnode_count, consistent_hash/vnode.rs:146-181; vnode→rank = contiguous
// blocks) + RCCL all-to-all-v over xGMI. Dense per-destination
// row blocks are semantics-preserving: the reference's remote exchange also
// ships visibility-compacted chunks (stream_chunk.rs:238-247).
//
// Payload layout per destination: ops u8[n] ∥ per column (valid u8[n] ∥
// vals i64[n]) — one contiguous buffer per peer per batch.
//
// The typed entries (rw_exchange_partition, rw_exchange_run_typed) add
// varchar columns: the same block followed by one byte region, defined once
// in include/rw_xpayload.hpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rw_chunk.h"
#include "../../include/rw_xpayload.hpp"
#include "rw_devmem.hpp"

static thread_local std::string g_xerr;

#define XFAIL(code, ...)                               \
    do {                                               \
        char _b[256];                                  \
        snprintf(_b, sizeof _b, __VA_ARGS__);          \
        g_xerr = _b;                                   \
        return code;                                   \
    } while (0)

#define XHIP(x)                                                      \
    do {                                                             \
        hipError_t _e = (x);                                         \
        if (_e != hipSuccess) XFAIL(-5, "HIP: %s", hipGetErrorString(_e)); \
    } while (0)

#define XNCCL(x)                                                      \
    do {                                                              \
        ncclResult_t _r = (x);                                        \
        if (_r != ncclSuccess) XFAIL(-6, "RCCL: %s", ncclGetErrorString(_r)); \
    } while (0)

#define XMAX_COLS 8

// Slicing-by-8 CRC tables (T0 = the plain byte table): an 8-byte key is one
// XOR tree of 8 independent LDS lookups instead of an 8-deep dependent
// chain. Staged to LDS — divergent indexing of __constant__ memory
// serializes (each distinct address replays); LDS banks handle it at rate.
__device__ uint32_t gx_crc8_table[8 * 256];

__device__ __forceinline__ void stage_crc_lut(uint32_t* lut) {
    for (int i = threadIdx.x; i < 8 * 256; i += blockDim.x)
        lut[i] = gx_crc8_table[i];
    __syncthreads();
}

// feed one little-endian u64 (a non-null i64 key datum)
__device__ __forceinline__ uint32_t xcrc_u64(const uint32_t* lut, uint32_t crc,
                                             uint64_t v) {
    uint32_t lo = crc ^ (uint32_t)v;
    uint32_t hi = (uint32_t)(v >> 32);
    return lut[7 * 256 + (lo & 0xff)] ^ lut[6 * 256 + ((lo >> 8) & 0xff)] ^
           lut[5 * 256 + ((lo >> 16) & 0xff)] ^ lut[4 * 256 + (lo >> 24)] ^
           lut[3 * 256 + (hi & 0xff)] ^ lut[2 * 256 + ((hi >> 8) & 0xff)] ^
           lut[1 * 256 + ((hi >> 16) & 0xff)] ^ lut[0 * 256 + (hi >> 24)];
}

// feed one little-endian u32 (the NULL sentinel)
__device__ __forceinline__ uint32_t xcrc_u32(const uint32_t* lut, uint32_t crc,
                                             uint32_t w) {
    uint32_t t = crc ^ w;
    return lut[3 * 256 + (t & 0xff)] ^ lut[2 * 256 + ((t >> 8) & 0xff)] ^
           lut[1 * 256 + ((t >> 16) & 0xff)] ^ lut[0 * 256 + (t >> 24)];
}

struct XBatch {
    const int64_t* col_vals[XMAX_COLS];
    const uint8_t* col_valid[XMAX_COLS];
    const uint8_t* ops;
    uint32_t n_rows;
};

// pass 1: vnode per row → destination rank; count per destination
// pass 1: vnode per row → destination rank; per-(block, dest) counts.
// No global atomics: even wave-aggregated, 16k wave leaders on one global
// counter serialize at ~88 adds/us (~0.18 ms per 1M rows — measured as the
// dominant cost of the previous version). Each block accumulates its own
// counts in LDS and writes one row of block_counts[dest][block].
__global__ void x_count_kernel(XBatch b, int n_keys, uint32_t k0, uint32_t k1,
                               uint32_t k2, uint32_t k3, uint32_t vnode_count,
                               int n_ranks, uint32_t* dest_of_row,
                               uint32_t* block_counts /* [R][gridDim.x] */) {
    __shared__ uint32_t lut[8 * 256];
    __shared__ uint32_t lds_counts[64];
    if (threadIdx.x < 64) lds_counts[threadIdx.x] = 0;
    stage_crc_lut(lut); // includes the __syncthreads
    uint32_t keys[4] = {k0, k1, k2, k3};
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t iters = (b.n_rows + stride - 1) / stride;
    uint32_t per_rank = vnode_count / n_ranks; // contiguous vnode blocks
    int lane = threadIdx.x & 63;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r < b.n_rows;
        uint32_t dest = 0xFFFFFFFFu;
        if (active) {
            uint32_t crc = 0xFFFFFFFFu;
            for (int k = 0; k < n_keys; k++) {
                uint32_t col = keys[k];
                if (!b.col_valid[col][r])
                    crc = xcrc_u32(lut, crc, 0xfffffff0u); // NULL sentinel
                else
                    crc = xcrc_u64(lut, crc, (uint64_t)b.col_vals[col][r]);
            }
            // vnode_count is a power of 2 in practice (256 default):
            // mask/shift instead of the ~100-instruction u64 div pair
            uint32_t h = crc ^ 0xFFFFFFFFu;
            uint32_t vn = (vnode_count & (vnode_count - 1)) == 0
                              ? (h & (vnode_count - 1))
                              : (uint32_t)((uint64_t)h % vnode_count);
            dest = vn / per_rank;
            if (dest >= (uint32_t)n_ranks) dest = n_ranks - 1;
            dest_of_row[r] = dest;
        }
        // wave-aggregated LDS counting: one LDS atomic per (wave, dest)
        for (int d = 0; d < n_ranks; d++) {
            uint64_t mask = __ballot(dest == (uint32_t)d);
            if (mask && lane == (63 - __clzll(mask)))
                atomicAdd(&lds_counts[d], (uint32_t)__popcll(mask));
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)n_ranks)
        block_counts[threadIdx.x * gridDim.x + blockIdx.x] =
            lds_counts[threadIdx.x];
}

// pass 1.5: exclusive scan of block_counts per destination → per-(block,
// dest) base row indexes + per-destination totals. One block; the serial
// 256-partial scan is microseconds.
__global__ void x_scan_kernel(int n_ranks, int nblocks,
                              const uint32_t* block_counts,
                              uint32_t* block_bases,
                              unsigned long long* counts) {
    __shared__ uint32_t part[256];
    int t = threadIdx.x;
    int per = (nblocks + 255) / 256;
    for (int d = 0; d < n_ranks; d++) {
        const uint32_t* bc = block_counts + (size_t)d * nblocks;
        uint32_t* bb = block_bases + (size_t)d * nblocks;
        int lo = t * per, hi = lo + per < nblocks ? lo + per : nblocks;
        uint32_t s = 0;
        for (int i = lo; i < hi; i++) s += bc[i];
        part[t] = s;
        __syncthreads();
        if (t == 0) {
            uint32_t run = 0;
            for (int i = 0; i < 256; i++) {
                uint32_t c = part[i];
                part[i] = run;
                run += c;
            }
            counts[d] = run;
        }
        __syncthreads();
        uint32_t base = part[t];
        for (int i = lo; i < hi; i++) {
            uint32_t c = bc[i];
            bb[i] = base;
            base += c;
        }
        __syncthreads();
    }
}

// pass 2: scatter rows into dense per-destination blocks
__global__ void x_scatter_kernel(XBatch b, int n_cols, int n_ranks,
                                 const uint32_t* dest_of_row,
                                 const unsigned long long* offsets, // [n_ranks]
                                 const unsigned long long* counts,  // [n_ranks]
                                 const uint32_t* block_bases, // [R][gridDim.x]
                                 uint8_t* out /* packed payload */) {
    // per-block LDS cursors pre-based by the scan — zero global atomics
    __shared__ uint32_t cursors[64];
    if (threadIdx.x < (uint32_t)n_ranks)
        cursors[threadIdx.x] =
            block_bases[threadIdx.x * gridDim.x + blockIdx.x];
    __syncthreads();
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t iters = (b.n_rows + stride - 1) / stride;
    int lane = threadIdx.x & 63;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t r = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r < b.n_rows;
        uint32_t dest = active ? dest_of_row[r] : 0xFFFFFFFFu;
        // wave-aggregated reservation: one LDS atomic per (wave, dest);
        // same-dest lanes get consecutive slots (coalesced scatter writes)
        unsigned long long idx = 0;
        for (int d = 0; d < n_ranks; d++) {
            uint64_t mask = __ballot(dest == (uint32_t)d);
            if (!mask) continue;
            uint32_t base = 0;
            int leader = 63 - __clzll(mask);
            if (lane == leader)
                base = atomicAdd(&cursors[d], (uint32_t)__popcll(mask));
            base = (uint32_t)__shfl((int)base, leader);
            if (dest == (uint32_t)d)
                idx = base + (unsigned long long)__popcll(mask &
                                                          ((1ULL << lane) - 1));
        }
        if (!active) continue;
        unsigned long long base = offsets[dest]; // byte offset (32-aligned)
        unsigned long long n = counts[dest];
        unsigned long long npad = (n + 3) & ~3ull;
        // block layout: vals[col][npad]*8 ∥ valid[col][n] ∥ ops[n]
        for (int c = 0; c < n_cols; c++) {
            int64_t* vals =
                (int64_t*)(out + base + (unsigned long long)c * npad * 8);
            vals[idx] = b.col_valid[c][r] ? b.col_vals[c][r] : 0;
        }
        uint8_t* valids = out + base + (unsigned long long)n_cols * npad * 8;
        for (int c = 0; c < n_cols; c++) valids[(unsigned long long)c * n + idx] = b.col_valid[c][r];
        uint8_t* ops = valids + (unsigned long long)n_cols * n;
        ops[idx] = b.ops[r];
    }
}

// ---------------------------------------------------------------------------
// Typed columns with a byte payload. The three kernels above
// stay the all-i64 path; a batch with a varchar column runs the xv_* kernels
// below. Block layout: include/rw_xpayload.hpp.
// ---------------------------------------------------------------------------

struct XTBatch {
    const int64_t* col_vals[XMAX_COLS]; // type 7: rwvarlen words
    const uint8_t* col_valid[XMAX_COLS];
    const uint8_t* col_bytes[XMAX_COLS]; // type 7: base the words refer to
    const uint8_t* ops;
    uint32_t n_rows;
    uint32_t n_cols;
    uint32_t vmask; // bit c = column c is varchar
};

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned long long wave_incl_scan(
    unsigned long long v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        unsigned long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// varchar bytes a row contributes (NULL cells contribute none)
__device__ __forceinline__ unsigned long long xv_row_bytes(const XTBatch& b,
                                                           uint32_t r) {
    unsigned long long s = 0;
    for (uint32_t c = 0; c < b.n_cols; c++)
        if (((b.vmask >> c) & 1) && b.col_valid[c][r])
            s += rwvarlen::word_len((uint64_t)b.col_vals[c][r]);
    return s;
}

// pass 1 for a batch with varchar columns: x_count_kernel's row counts plus
// varchar bytes per (block, dest), accumulated the same way — wave-level
// reduction, one LDS add per (wave, dest), no global atomics. The byte
// counters are 64-bit from the LDS partial on. The destination loop peels
// the destinations present in the wave instead of walking 0..n_dests.
__global__ void xv_count_kernel(XTBatch b, int n_keys, uint32_t k0, uint32_t k1,
                                uint32_t k2, uint32_t k3, uint32_t vnode_count,
                                int n_dests, uint32_t* dest_of_row,
                                uint32_t* block_counts /* [D][gridDim.x] */,
                                unsigned long long* block_vbytes /* same */) {
    __shared__ uint32_t lut[8 * 256];
    __shared__ uint32_t lds_counts[64];
    __shared__ unsigned long long lds_vbytes[64];
    if (threadIdx.x < 64) {
        lds_counts[threadIdx.x] = 0;
        lds_vbytes[threadIdx.x] = 0;
    }
    stage_crc_lut(lut); // includes the __syncthreads
    uint32_t keys[4] = {k0, k1, k2, k3};
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t iters = (b.n_rows + stride - 1) / stride;
    int lane = threadIdx.x & 63;
    for (uint32_t it = 0; it < iters; it++) {
        // 64-bit: it * stride + ... may pass 2^32 on the last iteration
        unsigned long long r64 = (unsigned long long)it * stride +
                                 blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r64 < b.n_rows;
        uint32_t r = (uint32_t)r64;
        uint32_t dest = 0xFFFFFFFFu;
        unsigned long long nbytes = 0;
        if (active) {
            uint32_t crc = 0xFFFFFFFFu;
            for (int k = 0; k < n_keys; k++) {
                uint32_t col = keys[k];
                if (!b.col_valid[col][r]) {
                    crc = rwx::crc_feed_u32(lut, crc, rwx::NULL_SENTINEL);
                } else if ((b.vmask >> col) & 1) {
                    uint64_t w = (uint64_t)b.col_vals[col][r];
                    crc = rwx::crc_feed_str(
                        lut, crc, b.col_bytes[col] + rwvarlen::word_off(w),
                        rwvarlen::word_len(w));
                } else {
                    crc = rwx::crc_feed_u64(lut, crc,
                                            (uint64_t)b.col_vals[col][r]);
                }
            }
            uint32_t h = crc ^ 0xFFFFFFFFu;
            uint32_t vn = (vnode_count & (vnode_count - 1)) == 0
                              ? (h & (vnode_count - 1))
                              : h % vnode_count;
            dest = rwx::dest_of_vnode(vn, vnode_count, (uint32_t)n_dests);
            dest_of_row[r] = dest;
            nbytes = xv_row_bytes(b, r);
        }
        uint64_t todo = __ballot(active);
        while (todo) { // wave-uniform
            uint32_t d = (uint32_t)__shfl((int)dest, __ffsll((long long)todo) - 1);
            uint64_t mask = __ballot(dest == d);
            unsigned long long tot =
                wave_incl_scan(dest == d ? nbytes : 0ull, lane);
            if (lane == 63) {
                atomicAdd(&lds_counts[d], (uint32_t)__popcll(mask));
                atomicAdd(&lds_vbytes[d], tot);
            }
            todo &= ~mask;
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)n_dests) {
        block_counts[threadIdx.x * gridDim.x + blockIdx.x] =
            lds_counts[threadIdx.x];
        block_vbytes[threadIdx.x * gridDim.x + blockIdx.x] =
            lds_vbytes[threadIdx.x];
    }
}

// pass 1.5: x_scan_kernel with a second, 64-bit track for the byte counts
__global__ void xv_scan_kernel(int n_dests, int nblocks,
                               const uint32_t* block_counts,
                               const unsigned long long* block_vbytes,
                               uint32_t* block_bases,
                               unsigned long long* block_vbases,
                               unsigned long long* counts,
                               unsigned long long* vbytes) {
    __shared__ uint32_t part[256];
    __shared__ unsigned long long vpart[256];
    int t = threadIdx.x;
    int per = (nblocks + 255) / 256;
    for (int d = 0; d < n_dests; d++) {
        const uint32_t* bc = block_counts + (size_t)d * nblocks;
        const unsigned long long* vc = block_vbytes + (size_t)d * nblocks;
        uint32_t* bb = block_bases + (size_t)d * nblocks;
        unsigned long long* vb = block_vbases + (size_t)d * nblocks;
        int lo = t * per, hi = lo + per < nblocks ? lo + per : nblocks;
        uint32_t s = 0;
        unsigned long long vs = 0;
        for (int i = lo; i < hi; i++) {
            s += bc[i];
            vs += vc[i];
        }
        part[t] = s;
        vpart[t] = vs;
        __syncthreads();
        if (t == 0) {
            uint32_t run = 0;
            unsigned long long vrun = 0;
            for (int i = 0; i < 256; i++) {
                uint32_t c = part[i];
                unsigned long long v = vpart[i];
                part[i] = run;
                vpart[i] = vrun;
                run += c;
                vrun += v;
            }
            counts[d] = run;
            vbytes[d] = vrun;
        }
        __syncthreads();
        uint32_t base = part[t];
        unsigned long long vbase = vpart[t];
        for (int i = lo; i < hi; i++) {
            uint32_t c = bc[i];
            unsigned long long v = vc[i];
            bb[i] = base;
            vb[i] = vbase;
            base += c;
            vbase += v;
        }
        __syncthreads();
    }
}

// pass 2: scatter rows and reserve their byte ranges. One 64-bit LDS
// reservation per (wave, dest) hands out the row slots and the byte range
// together, so a row's slot and the ranges of all its varchar cells come
// from one atomic and can neither disagree nor overlap another row's:
//     bits  0..39  bytes reserved so far by this block for the destination
//     bits 40..63  rows  reserved so far by this block for the destination
// A block owns at most ceil(2^32 / (2048*256)) * 256 = 2^21 rows and the
// host refuses a destination with more than 2^40-1 varchar bytes (the word
// format's offset range), so neither field can carry into the other.
// Writes the record words; the bytes are copied by xv_copy_kernel, which
// finds its source row through slot_src.
__global__ void xv_scatter_kernel(XTBatch b, int n_dests,
                                  const uint32_t* dest_of_row,
                                  const unsigned long long* offsets, // [D]
                                  const unsigned long long* counts,  // [D]
                                  const unsigned long long* vbytes,  // [D]
                                  const unsigned long long* row_prefix, // [D]
                                  const uint32_t* block_bases,
                                  const unsigned long long* block_vbases,
                                  uint32_t* slot_src /* [n_rows] */,
                                  uint8_t* out) {
    __shared__ unsigned long long cursors[64];
    __shared__ uint32_t row_base[64];
    __shared__ unsigned long long byte_base[64];
    if (threadIdx.x < (uint32_t)n_dests) {
        cursors[threadIdx.x] = 0;
        row_base[threadIdx.x] =
            block_bases[threadIdx.x * gridDim.x + blockIdx.x];
        byte_base[threadIdx.x] =
            block_vbases[threadIdx.x * gridDim.x + blockIdx.x];
    }
    __syncthreads();
    uint32_t stride = gridDim.x * blockDim.x;
    uint32_t iters = (b.n_rows + stride - 1) / stride;
    int lane = threadIdx.x & 63;
    for (uint32_t it = 0; it < iters; it++) {
        unsigned long long r64 = (unsigned long long)it * stride +
                                 blockIdx.x * blockDim.x + threadIdx.x;
        bool active = r64 < b.n_rows;
        uint32_t r = (uint32_t)r64;
        uint32_t dest = active ? dest_of_row[r] : 0xFFFFFFFFu;
        unsigned long long nbytes = active ? xv_row_bytes(b, r) : 0ull;
        unsigned long long idx = 0, boff = 0;
        uint64_t todo = __ballot(active);
        while (todo) { // wave-uniform
            uint32_t d = (uint32_t)__shfl((int)dest, __ffsll((long long)todo) - 1);
            uint64_t mask = __ballot(dest == d);
            unsigned long long incl =
                wave_incl_scan(dest == d ? nbytes : 0ull, lane);
            unsigned long long got = 0;
            if (lane == 63)
                got = atomicAdd(&cursors[d],
                                ((unsigned long long)__popcll(mask)
                                 << rwvarlen::OFF_BITS) | incl);
            got = __shfl(got, 63, 64);
            if (dest == d) {
                idx = row_base[d] + (got >> rwvarlen::OFF_BITS) +
                      __popcll(mask & ((1ULL << lane) - 1));
                boff = byte_base[d] + (got & rwvarlen::MAX_OFF) + incl - nbytes;
            }
            todo &= ~mask;
        }
        if (!active) continue;
        rwx::BlockLayout L =
            rwx::block_layout(counts[dest], b.n_cols, vbytes[dest]);
        uint8_t* blk = out + offsets[dest];
        for (uint32_t c = 0; c < b.n_cols; c++) {
            int64_t* vals = (int64_t*)(blk + L.vals_off(c));
            uint8_t ok = b.col_valid[c][r];
            int64_t v = ok ? b.col_vals[c][r] : 0;
            if (ok && ((b.vmask >> c) & 1)) {
                uint32_t len = rwvarlen::word_len((uint64_t)v);
                v = (int64_t)rwvarlen::pack(boff, len);
                boff += len;
            }
            vals[idx] = v;
            blk[L.valid_off + (unsigned long long)c * L.n + idx] = ok;
        }
        blk[L.ops_off + idx] = b.ops[r];
        slot_src[row_prefix[dest] + idx] = r;
    }
}

// pass 3: copy the bytes, one string per lane in slot order (neighbouring
// lanes write neighbouring strings; §13.5 measured this loop 1.9-3.3x faster
// than output-centric copies at q8 name lengths).
__global__ void xv_copy_kernel(XTBatch b, const uint32_t* dest_of_row,
                               const unsigned long long* offsets,
                               const unsigned long long* counts,
                               const unsigned long long* vbytes,
                               const unsigned long long* row_prefix,
                               const uint32_t* slot_src, uint8_t* out) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (unsigned long long g = blockIdx.x * blockDim.x + threadIdx.x;
         g < b.n_rows; g += stride) {
        uint32_t r = slot_src[g];
        uint32_t dest = dest_of_row[r];
        unsigned long long idx = g - row_prefix[dest];
        rwx::BlockLayout L =
            rwx::block_layout(counts[dest], b.n_cols, vbytes[dest]);
        uint8_t* blk = out + offsets[dest];
        for (uint32_t c = 0; c < b.n_cols; c++) {
            if (!((b.vmask >> c) & 1) || !b.col_valid[c][r]) continue;
            uint64_t sw = (uint64_t)b.col_vals[c][r];
            uint64_t dw = (uint64_t)((const int64_t*)(blk + L.vals_off(c)))[idx];
            const uint8_t* src = b.col_bytes[c] + rwvarlen::word_off(sw);
            uint8_t* dst = blk + L.vbytes_off + rwvarlen::word_off(dw);
            uint32_t len = rwvarlen::word_len(sw);
            for (uint32_t i = 0; i < len; i++) dst[i] = src[i];
        }
    }
}

#define XMAX_DESTS 64

struct Exchange {
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr;
    DevOwner mem; // every device buffer of this context (rw_devmem.hpp)
    int rank = 0, n_ranks = 1;
    double exch_ms = 0;
    uint64_t exch_launches = 0;
    // persistent scratch (allocated on first run, grown as needed)
    uint32_t* d_dest = nullptr;
    uint32_t dest_cap = 0;
    unsigned long long *d_counts = nullptr, *d_offsets = nullptr,
                       *d_count_mat = nullptr;
    uint32_t *d_block_counts = nullptr, *d_block_bases = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // scratch of the typed entries (rw_exchange_partition / _run_typed),
    // sized for XMAX_DESTS destinations whatever the communicator size
    uint32_t *t_dest = nullptr, *t_slot_src = nullptr;
    uint32_t t_cap = 0;
    uint32_t *t_block_counts = nullptr, *t_block_bases = nullptr;
    unsigned long long *t_block_vbytes = nullptr, *t_block_vbases = nullptr;
    // [5][XMAX_DESTS]: counts, vbytes, offsets, row_prefix, recv pairs base
    unsigned long long* t_small = nullptr;
    unsigned long long *t_pair_send = nullptr, *t_pair_recv = nullptr;
    hipEvent_t t_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float t_phase_ms[4] = {0, 0, 0, 0};
};

extern "C" {

const char* rw_exchange_last_error(void) { return g_xerr.c_str(); }

int rw_exchange_unique_id_size(void) { return (int)sizeof(ncclUniqueId); }

int rw_exchange_get_unique_id(void* out) {
    ncclUniqueId id;
    XNCCL(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return 0;
}

void* rw_exchange_create(int n_ranks, int rank, const void* unique_id) {
    auto* x = new Exchange();
    x->rank = rank;
    x->n_ranks = n_ranks;
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    if (hipStreamCreate(&x->stream) != hipSuccess) {
        delete x;
        return nullptr;
    }
    if (ncclCommInitRank(&x->comm, n_ranks, id, rank) != ncclSuccess) {
        g_xerr = "ncclCommInitRank failed";
        delete x;
        return nullptr;
    }
    // slicing-by-8 CRC tables for the partition kernel:
    // T0 = plain byte table; Tk[i] = (Tk-1[i] >> 8) ^ T0[Tk-1[i] & 0xff]
    static uint32_t tab[8][256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        tab[0][i] = c;
    }
    for (int k = 1; k < 8; k++)
        for (int i = 0; i < 256; i++)
            tab[k][i] = (tab[k - 1][i] >> 8) ^ tab[0][tab[k - 1][i] & 0xff];
    hipMemcpyToSymbol(HIP_SYMBOL(gx_crc8_table), tab, sizeof tab);
    return x;
}

void rw_exchange_destroy(void* h) {
    auto* x = (Exchange*)h;
    if (!x) return;
    if (x->comm) ncclCommDestroy(x->comm);
    x->mem.release_all(); // device memory goes before the stream
    if (x->e0) hipEventDestroy(x->e0);
    if (x->e1) hipEventDestroy(x->e1);
    for (auto& e : x->t_ev)
        if (e) hipEventDestroy(e);
    if (x->stream) hipStreamDestroy(x->stream);
    delete x;
}

// Partition a device-resident batch by vnode and exchange: every rank
// contributes one batch; each receives the union of the rows routed to it.
// In/out buffers are device pointers. Returns received row count via
// *n_recv_rows; the received payload (same per-destination layout, blocks
// concatenated in rank order) lands in recv_buf (capacity recv_cap bytes).
// counts_out[n_ranks] reports per-peer sent rows (for stats).
int rw_exchange_run(void* h, const int64_t* const* col_vals,
                    const uint8_t* const* col_valid, const uint8_t* ops,
                    uint32_t n_rows, int n_cols, const uint32_t* key_cols,
                    int n_keys, uint32_t vnode_count, uint8_t* send_buf,
                    uint64_t send_cap, uint8_t* recv_buf, uint64_t recv_cap,
                    uint64_t* send_counts_out, uint64_t* recv_counts_out) {
    auto* x = (Exchange*)h;
    int R = x->n_ranks;
    if (n_cols > XMAX_COLS || n_keys > 4) XFAIL(-1, "too many cols/keys");
    XBatch b{};
    for (int c = 0; c < n_cols; c++) {
        b.col_vals[c] = col_vals[c];
        b.col_valid[c] = col_valid[c];
    }
    b.ops = ops;
    b.n_rows = n_rows;

    if (x->dest_cap < n_rows) {
        x->dest_cap = 0;
        XHIP(x->mem.regrow(&x->d_dest, (size_t)n_rows * 4));
        x->dest_cap = n_rows;
    }
    if (!x->d_counts) {
        XHIP(x->mem.alloc(&x->d_counts, R * 8));
        XHIP(x->mem.alloc(&x->d_offsets, R * 8));
        XHIP(x->mem.alloc(&x->d_count_mat, R * 8));
        XHIP(x->mem.alloc(&x->d_block_counts, (size_t)R * 2048 * 4));
        XHIP(x->mem.alloc(&x->d_block_bases, (size_t)R * 2048 * 4));
        XHIP(hipEventCreate(&x->e0));
        XHIP(hipEventCreate(&x->e1));
    }
    uint32_t* d_dest = x->d_dest;
    unsigned long long *d_counts = x->d_counts, *d_offsets = x->d_offsets;

    uint32_t blocks = (n_rows + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (!blocks) blocks = 1;
    uint32_t k[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_keys; i++) k[i] = key_cols[i];

    static int dbg = -1;
    if (dbg < 0) {
        const char* e = getenv("RW_EXCHANGE_DEBUG");
        dbg = e && *e == '1';
    }
    struct Phase {
        const char* name;
        double t;
    } phases[8];
    int np = 0;
    auto mark = [&](const char* name) {
        if (!dbg) return;
        hipStreamSynchronize(x->stream);
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        phases[np++] = {name, ts.tv_sec * 1e3 + ts.tv_nsec / 1e6};
    };
    mark("start");
    hipEvent_t e0 = x->e0, e1 = x->e1;
    XHIP(hipEventRecord(e0, x->stream));

    x_count_kernel<<<blocks, 256, 0, x->stream>>>(b, n_keys, k[0], k[1], k[2],
                                                  k[3], vnode_count, R, d_dest,
                                                  x->d_block_counts);
    x_scan_kernel<<<1, 256, 0, x->stream>>>(R, (int)blocks, x->d_block_counts,
                                            x->d_block_bases, d_counts);
    mark("count_kernel");
    unsigned long long counts[64];
    XHIP(hipMemcpyAsync(counts, d_counts, R * 8, hipMemcpyDeviceToHost,
                        x->stream));
    XHIP(hipStreamSynchronize(x->stream));
    mark("counts_d2h");

    // byte offsets of per-destination blocks in send_buf
    // per-destination block: vals[col][npad]*8 ∥ valid[col][n] ∥ ops[n],
    // npad = n rounded up to 4 so every vals[col] base is 32-B aligned
    // (the receiver's dense vectorized apply needs b128-aligned columns)
    auto block_bytes = [&](uint64_t nrows) {
        uint64_t npad = (nrows + 3) & ~3ull;
        return ((uint64_t)n_cols * npad * 8 + (uint64_t)n_cols * nrows + nrows +
                31) & ~31ull;
    };
    unsigned long long offsets[64];
    uint64_t off = 0;
    for (int d = 0; d < R; d++) {
        offsets[d] = off;
        off += block_bytes(counts[d]);
    }
    if (off > send_cap) XFAIL(-2, "send buffer too small (%llu)", (unsigned long long)off);
    XHIP(hipMemcpyAsync(d_offsets, offsets, R * 8, hipMemcpyHostToDevice,
                        x->stream));
    x_scatter_kernel<<<blocks, 256, 0, x->stream>>>(b, n_cols, R, d_dest,
                                                    d_offsets, d_counts,
                                                    x->d_block_bases, send_buf);
    mark("scatter");

    // exchange per-peer row counts, then the payload blocks (all-to-all-v)
    // over RCCL/xGMI. A single-rank communicator is a degenerate self-loop:
    // bypass RCCL with a device copy (semantics identical; RCCL's loopback
    // path costs ~25 ms per 28 MB on this stack). Set
    // RW_EXCHANGE_FORCE_NCCL=1 to exercise the collective at R=1.
    static int force_nccl = -1;
    if (force_nccl < 0) {
        const char* e = getenv("RW_EXCHANGE_FORCE_NCCL");
        force_nccl = e && *e == '1';
    }
    unsigned long long recv_counts[64];
    unsigned long long recv_offsets[64];
    if (R == 1 && !force_nccl) {
        recv_counts[0] = counts[0];
        recv_offsets[0] = 0;
        if (block_bytes(counts[0]) > recv_cap) XFAIL(-3, "recv buffer too small");
        XHIP(hipMemcpyAsync(recv_buf, send_buf, block_bytes(counts[0]),
                            hipMemcpyDeviceToDevice, x->stream));
    } else {
        unsigned long long* d_count_mat = x->d_count_mat;
        XNCCL(ncclGroupStart());
        for (int p = 0; p < R; p++) {
            XNCCL(ncclSend(d_counts + p, 1, ncclUint64, p, x->comm, x->stream));
            XNCCL(ncclRecv(d_count_mat + p, 1, ncclUint64, p, x->comm, x->stream));
        }
        XNCCL(ncclGroupEnd());
        XHIP(hipMemcpyAsync(recv_counts, d_count_mat, R * 8,
                            hipMemcpyDeviceToHost, x->stream));
        XHIP(hipStreamSynchronize(x->stream));

        uint64_t roff = 0;
        for (int p = 0; p < R; p++) {
            recv_offsets[p] = roff;
            roff += block_bytes(recv_counts[p]);
        }
        if (roff > recv_cap) XFAIL(-3, "recv buffer too small");

        XNCCL(ncclGroupStart());
        for (int p = 0; p < R; p++) {
            if (counts[p])
                XNCCL(ncclSend(send_buf + offsets[p], block_bytes(counts[p]),
                               ncclUint8, p, x->comm, x->stream));
            if (recv_counts[p])
                XNCCL(ncclRecv(recv_buf + recv_offsets[p],
                               block_bytes(recv_counts[p]), ncclUint8, p,
                               x->comm, x->stream));
        }
        XNCCL(ncclGroupEnd());
    }
    mark("exchange");
    XHIP(hipEventRecord(e1, x->stream));
    XHIP(hipStreamSynchronize(x->stream));
    if (dbg && x->exch_launches < 3) {
        for (int i = 1; i < np; i++)
            fprintf(stderr, "# exch %s: %.3f ms\n", phases[i].name,
                    phases[i].t - phases[i - 1].t);
    }
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    x->exch_ms += ms;
    x->exch_launches++;

    for (int p = 0; p < R; p++) {
        send_counts_out[p] = counts[p];
        recv_counts_out[p] = recv_counts[p];
    }
    return 0;
}

// ---- typed columns ----
//
// A column of a device-resident batch. `vals` holds n_rows 8-byte words: the
// value for RW_T_I64 / RW_T_TS / RW_T_F64, a rwvarlen::pack(off, len) word
// (include/rw_varlen.hpp) for RW_T_VARCHAR with `off` relative to `bytes`.
// The words and bytes of NULL rows are ignored. Other types are refused.
typedef struct RwXCol {
    uint8_t type;         // RwTypeId
    const int64_t* vals;  // device
    const uint8_t* valid; // device, 1 = non-NULL
    const uint8_t* bytes; // device; RW_T_VARCHAR only, else NULL
} RwXCol;

} // extern "C"

// count → scan → scatter (→ byte copy) into send_buf; fills rows / vbytes /
// offs for n_dests destinations. No communicator call.
static int partition_typed(Exchange* x, const RwXCol* cols, int n_cols,
                           const uint8_t* ops, uint32_t n_rows,
                           const uint32_t* key_cols, int n_keys,
                           uint32_t vnode_count, int n_dests, uint8_t* send_buf,
                           uint64_t send_cap, unsigned long long* rows,
                           unsigned long long* vbytes,
                           unsigned long long* offs) {
    if (n_cols < 1 || n_cols > XMAX_COLS || n_keys < 1 || n_keys > 4)
        XFAIL(-1, "n_cols %d (1..%d) / n_keys %d (1..4)", n_cols, XMAX_COLS,
              n_keys);
    if (n_dests < 1 || n_dests > XMAX_DESTS)
        XFAIL(-1, "n_dests %d out of range (1..%d)", n_dests, XMAX_DESTS);
    if (vnode_count < (uint32_t)n_dests || vnode_count > 65536)
        XFAIL(-1, "vnode_count %u (n_dests..65536)", vnode_count);
    XTBatch tb{};
    for (int c = 0; c < n_cols; c++) {
        uint8_t t = cols[c].type;
        if (t == RW_T_VARCHAR) {
            if (!cols[c].bytes) XFAIL(-1, "varchar column %d without bytes", c);
            tb.vmask |= 1u << c;
        } else if (t != RW_T_I64 && t != RW_T_TS && t != RW_T_F64) {
            XFAIL(-1, "column %d: type %d unsupported in the exchange", c, t);
        }
        tb.col_vals[c] = cols[c].vals;
        tb.col_valid[c] = cols[c].valid;
        tb.col_bytes[c] = cols[c].bytes;
    }
    uint32_t k[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_keys; i++) {
        if (key_cols[i] >= (uint32_t)n_cols) XFAIL(-1, "key column out of range");
        k[i] = key_cols[i];
    }
    tb.ops = ops;
    tb.n_rows = n_rows;
    tb.n_cols = (uint32_t)n_cols;

    const int D = XMAX_DESTS;
    if (!x->t_small) {
        XHIP(x->mem.alloc(&x->t_block_counts, (size_t)D * 2048 * 4));
        XHIP(x->mem.alloc(&x->t_block_bases, (size_t)D * 2048 * 4));
        XHIP(x->mem.alloc(&x->t_block_vbytes, (size_t)D * 2048 * 8));
        XHIP(x->mem.alloc(&x->t_block_vbases, (size_t)D * 2048 * 8));
        XHIP(x->mem.alloc(&x->t_pair_send, (size_t)D * 16));
        XHIP(x->mem.alloc(&x->t_pair_recv, (size_t)D * 16));
        for (auto& e : x->t_ev) XHIP(hipEventCreate(&e));
        XHIP(x->mem.alloc(&x->t_small, (size_t)4 * D * 8)); // last: the guard
    }
    if (x->t_cap < n_rows || !x->t_dest) {
        x->mem.release(&x->t_dest);
        x->mem.release(&x->t_slot_src);
        x->t_cap = 0;
        size_t cap = n_rows ? n_rows : 1;
        XHIP(x->mem.alloc(&x->t_dest, cap * 4));
        if (x->mem.alloc(&x->t_slot_src, cap * 4) != hipSuccess) {
            x->mem.release(&x->t_dest);
            XFAIL(-5, "HIP: out of memory (slot map)");
        }
        x->t_cap = (uint32_t)cap;
    }
    unsigned long long *d_counts = x->t_small, *d_vbytes = x->t_small + D,
                       *d_offsets = x->t_small + 2 * D,
                       *d_prefix = x->t_small + 3 * D;
    uint32_t blocks = (n_rows + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (!blocks) blocks = 1;
    hipStream_t s = x->stream;

    XHIP(hipEventRecord(x->t_ev[0], s));
    if (tb.vmask) {
        xv_count_kernel<<<blocks, 256, 0, s>>>(
            tb, n_keys, k[0], k[1], k[2], k[3], vnode_count, n_dests, x->t_dest,
            x->t_block_counts, x->t_block_vbytes);
        XHIP(hipEventRecord(x->t_ev[1], s));
        xv_scan_kernel<<<1, 256, 0, s>>>(n_dests, (int)blocks,
                                         x->t_block_counts, x->t_block_vbytes,
                                         x->t_block_bases, x->t_block_vbases,
                                         d_counts, d_vbytes);
    } else {
        // no varchar column: the all-i64 kernels, at this destination count
        XBatch b{};
        for (int c = 0; c < n_cols; c++) {
            b.col_vals[c] = cols[c].vals;
            b.col_valid[c] = cols[c].valid;
        }
        b.ops = ops;
        b.n_rows = n_rows;
        x_count_kernel<<<blocks, 256, 0, s>>>(b, n_keys, k[0], k[1], k[2], k[3],
                                              vnode_count, n_dests, x->t_dest,
                                              x->t_block_counts);
        XHIP(hipEventRecord(x->t_ev[1], s));
        x_scan_kernel<<<1, 256, 0, s>>>(n_dests, (int)blocks,
                                        x->t_block_counts, x->t_block_bases,
                                        d_counts);
        XHIP(hipMemsetAsync(d_vbytes, 0, (size_t)D * 8, s));
    }
    XHIP(hipEventRecord(x->t_ev[2], s));
    unsigned long long host[2 * XMAX_DESTS];
    XHIP(hipMemcpyAsync(host, x->t_small, (size_t)2 * D * 8,
                        hipMemcpyDeviceToHost, s));
    XHIP(hipStreamSynchronize(s));

    unsigned long long up[2 * XMAX_DESTS]; // offsets ∥ row_prefix
    uint64_t off = 0, pre = 0;
    for (int d = 0; d < n_dests; d++) {
        rows[d] = host[d];
        vbytes[d] = host[D + d];
        if (vbytes[d] > rwvarlen::MAX_OFF)
            XFAIL(-1, "destination %d: %llu varchar bytes exceed the word "
                      "format's 2^40-1", d, vbytes[d]);
        offs[d] = up[d] = off;
        up[D + d] = pre;
        off += rwx::block_bytes(rows[d], (uint64_t)n_cols, vbytes[d]);
        pre += rows[d];
    }
    if (pre != n_rows) XFAIL(-5, "partition count mismatch");
    if (off > send_cap)
        XFAIL(-2, "send buffer too small (%llu)", (unsigned long long)off);
    XHIP(hipMemcpyAsync(d_offsets, up, (size_t)2 * D * 8,
                        hipMemcpyHostToDevice, s));
    XHIP(hipEventRecord(x->t_ev[3], s));
    if (tb.vmask) {
        xv_scatter_kernel<<<blocks, 256, 0, s>>>(
            tb, n_dests, x->t_dest, d_offsets, d_counts, d_vbytes, d_prefix,
            x->t_block_bases, x->t_block_vbases, x->t_slot_src, send_buf);
        XHIP(hipEventRecord(x->t_ev[4], s));
        xv_copy_kernel<<<blocks, 256, 0, s>>>(tb, x->t_dest, d_offsets,
                                              d_counts, d_vbytes, d_prefix,
                                              x->t_slot_src, send_buf);
    } else {
        XBatch b{};
        for (int c = 0; c < n_cols; c++) {
            b.col_vals[c] = cols[c].vals;
            b.col_valid[c] = cols[c].valid;
        }
        b.ops = ops;
        b.n_rows = n_rows;
        x_scatter_kernel<<<blocks, 256, 0, s>>>(b, n_cols, n_dests, x->t_dest,
                                                d_offsets, d_counts,
                                                x->t_block_bases, send_buf);
        XHIP(hipEventRecord(x->t_ev[4], s));
    }
    XHIP(hipEventRecord(x->t_ev[5], s));
    XHIP(hipStreamSynchronize(s));
    XHIP(hipGetLastError());
    static const int ph[4] = {0, 1, 3, 4}; // count, scan, scatter, copy
    for (int i = 0; i < 4; i++)
        hipEventElapsedTime(&x->t_phase_ms[i], x->t_ev[ph[i]],
                            x->t_ev[ph[i] + 1]);
    return 0;
}

extern "C" {

// Partition only: route a device-resident typed batch into n_dests dense
// blocks in send_buf (layout: include/rw_xpayload.hpp) without touching the
// communicator. `h` supplies the stream and scratch. Destination of a vnode:
// min(vnode / (vnode_count / n_dests), n_dests - 1). n_dests is explicit
// (1..64, else -1), so one device can exercise every destination count.
// Per destination d the call reports rows_out[d], vbytes_out[d] and
// offs_out[d], the block's byte offset in send_buf (32-aligned). Returns 0,
// -1 (bad argument), -2 (send_cap too small; nothing past it is written) or
// -5 (HIP). The U-pair downgrade of HashDataDispatcher is not applied.
int rw_exchange_partition(void* h, const RwXCol* cols, int n_cols,
                          const uint8_t* ops, uint32_t n_rows,
                          const uint32_t* key_cols, int n_keys,
                          uint32_t vnode_count, int n_dests, uint8_t* send_buf,
                          uint64_t send_cap, uint64_t* rows_out,
                          uint64_t* vbytes_out, uint64_t* offs_out) {
    unsigned long long rows[XMAX_DESTS], vb[XMAX_DESTS], offs[XMAX_DESTS];
    int rc = partition_typed((Exchange*)h, cols, n_cols, ops, n_rows, key_cols,
                             n_keys, vnode_count, n_dests, send_buf, send_cap,
                             rows, vb, offs);
    if (rc) return rc;
    for (int d = 0; d < n_dests; d++) {
        rows_out[d] = rows[d];
        vbytes_out[d] = vb[d];
        offs_out[d] = offs[d];
    }
    return 0;
}

// Device time of the last partition's phases, ms: count, scan, scatter,
// byte copy (0 for a batch without varchar columns).
int rw_exchange_partition_phases(void* h, double* ms4) {
    auto* x = (Exchange*)h;
    for (int i = 0; i < 4; i++) ms4[i] = x->t_phase_ms[i];
    return 0;
}

// rw_exchange_run for typed columns: the partition above with n_dests =
// n_ranks, then the all-to-all-v. The per-peer count exchange carries two
// u64 per peer (rows, varchar bytes); a peer's block is
// rwx::block_bytes(rows, n_cols, vbytes) bytes. Received blocks land in
// recv_buf concatenated in rank order. send_*_out / recv_*_out [n_ranks]
// report per-peer rows and varchar bytes. A single-rank communicator
// bypasses RCCL with a device copy unless RW_EXCHANGE_FORCE_NCCL=1, as in
// rw_exchange_run. Returns 0, -1, -2 (send_cap), -3 (recv_cap), -5, -6.
int rw_exchange_run_typed(void* h, const RwXCol* cols, int n_cols,
                          const uint8_t* ops, uint32_t n_rows,
                          const uint32_t* key_cols, int n_keys,
                          uint32_t vnode_count, uint8_t* send_buf,
                          uint64_t send_cap, uint8_t* recv_buf,
                          uint64_t recv_cap, uint64_t* send_rows_out,
                          uint64_t* send_vbytes_out, uint64_t* recv_rows_out,
                          uint64_t* recv_vbytes_out) {
    auto* x = (Exchange*)h;
    int R = x->n_ranks;
    unsigned long long rows[XMAX_DESTS], vb[XMAX_DESTS], offs[XMAX_DESTS];
    int rc = partition_typed(x, cols, n_cols, ops, n_rows, key_cols, n_keys,
                             vnode_count, R, send_buf, send_cap, rows, vb, offs);
    if (rc) return rc;
    auto bbytes = [&](int p, const unsigned long long* r,
                      const unsigned long long* v) {
        return rwx::block_bytes(r[p], (uint64_t)n_cols, v[p]);
    };
    static int force_nccl = -1;
    if (force_nccl < 0) {
        const char* e = getenv("RW_EXCHANGE_FORCE_NCCL");
        force_nccl = e && *e == '1';
    }
    unsigned long long rrows[XMAX_DESTS], rvb[XMAX_DESTS];
    if (R == 1 && !force_nccl) {
        rrows[0] = rows[0];
        rvb[0] = vb[0];
        if (bbytes(0, rows, vb) > recv_cap)
            XFAIL(-3, "recv buffer too small (%llu)",
                  (unsigned long long)bbytes(0, rows, vb));
        XHIP(hipMemcpyAsync(recv_buf, send_buf, bbytes(0, rows, vb),
                            hipMemcpyDeviceToDevice, x->stream));
    } else {
        unsigned long long pair[2 * XMAX_DESTS];
        for (int p = 0; p < R; p++) {
            pair[2 * p] = rows[p];
            pair[2 * p + 1] = vb[p];
        }
        XHIP(hipMemcpyAsync(x->t_pair_send, pair, (size_t)R * 16,
                            hipMemcpyHostToDevice, x->stream));
        XNCCL(ncclGroupStart());
        for (int p = 0; p < R; p++) {
            XNCCL(ncclSend(x->t_pair_send + 2 * p, 2, ncclUint64, p, x->comm,
                           x->stream));
            XNCCL(ncclRecv(x->t_pair_recv + 2 * p, 2, ncclUint64, p, x->comm,
                           x->stream));
        }
        XNCCL(ncclGroupEnd());
        XHIP(hipMemcpyAsync(pair, x->t_pair_recv, (size_t)R * 16,
                            hipMemcpyDeviceToHost, x->stream));
        XHIP(hipStreamSynchronize(x->stream));
        unsigned long long roffs[XMAX_DESTS];
        uint64_t roff = 0;
        for (int p = 0; p < R; p++) {
            rrows[p] = pair[2 * p];
            rvb[p] = pair[2 * p + 1];
            roffs[p] = roff;
            roff += bbytes(p, rrows, rvb);
        }
        // every rank has finished the count exchange here, so failing now
        // leaves no peer waiting in the payload group
        if (roff > recv_cap)
            XFAIL(-3, "recv buffer too small (%llu)", (unsigned long long)roff);
        XNCCL(ncclGroupStart());
        for (int p = 0; p < R; p++) {
            if (rows[p])
                XNCCL(ncclSend(send_buf + offs[p], bbytes(p, rows, vb),
                               ncclUint8, p, x->comm, x->stream));
            if (rrows[p])
                XNCCL(ncclRecv(recv_buf + roffs[p], bbytes(p, rrows, rvb),
                               ncclUint8, p, x->comm, x->stream));
        }
        XNCCL(ncclGroupEnd());
    }
    XHIP(hipStreamSynchronize(x->stream));
    for (int p = 0; p < R; p++) {
        send_rows_out[p] = rows[p];
        send_vbytes_out[p] = vb[p];
        recv_rows_out[p] = rrows[p];
        recv_vbytes_out[p] = rvb[p];
    }
    return 0;
}

// Plain synchronous copies to and from rw_xbuf_alloc memory, so a caller
// can stage a batch and read a payload back without an executor.
int rw_xbuf_write(void* dev, const void* host, uint64_t bytes) {
    if (bytes) XHIP(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}
int rw_xbuf_read(void* host, const void* dev, uint64_t bytes) {
    if (bytes) XHIP(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// Caller-owned buffers share one process-wide owner, never destroyed (a
// static destructor would call into a HIP runtime that may be gone).
static std::mutex g_xbuf_mu;
static DevOwner& xbuf_mem() {
    static DevOwner* o = new DevOwner();
    return *o;
}
void* rw_xbuf_alloc(uint64_t bytes) {
    std::lock_guard<std::mutex> lk(g_xbuf_mu);
    void* p = nullptr;
    (void)xbuf_mem().alloc(&p, bytes);
    return p;
}
void rw_xbuf_free(void* p) {
    std::lock_guard<std::mutex> lk(g_xbuf_mu);
    xbuf_mem().release(&p);
}

// debug/test only: device bytes this library's owners hold right now
uint64_t rw_exchange_debug_dev_bytes_live(void) { return g_dev_bytes_live.load(); }

int rw_exchange_stats(void* h, double* total_ms, uint64_t* launches) {
    auto* x = (Exchange*)h;
    *total_ms = x->exch_ms;
    *launches = x->exch_launches;
    return 0;
}

} // extern "C"
