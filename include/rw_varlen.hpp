// rw_varlen.hpp — host/device helpers for RW_T_VARCHAR payload columns in
// the join executor.
//
// A varchar cell occupies the same 8-byte record word an i64 value does; the
// word is a REFERENCE into the owning side's device byte arena:
//
//     bits  0..39  byte offset into the arena   (arena <= 1 TiB)
//     bits 40..63  byte length                  (string <= 2^24-1 bytes)
//
// A NULL cell is word 0 with its validbit clear. Words hold offsets, not
// pointers, so growing the arena is a reallocate + copy: no word changes.
#pragma once
#include <cstdint>
#include <vector>

#include "rw_chunk.h"

#ifdef __HIPCC__
#define RW_VARLEN_HD __host__ __device__
#else
#define RW_VARLEN_HD
#endif

namespace rwvarlen {

constexpr uint64_t OFF_BITS = 40;
constexpr uint64_t MAX_OFF = (1ULL << OFF_BITS) - 1; // 2^40-1
constexpr uint32_t MAX_LEN = (1u << 24) - 1;         // 2^24-1

// HashAgg varchar group keys. A group-key word is CANONICAL:
// one word per distinct string, referencing the executor's interning arena.
// While a pushed batch is being interned its words are PROVISIONAL: offset
// bit 39 set, the remaining offset bits indexing the executor's staging
// buffer. The bit halves the offset range, so an interning arena (and a
// staged chunk) holds at most 2^39 bytes. The arena's first
// AGG_ARENA_HEADER bytes are reserved so that no canonical word is 0 (the
// NULL / empty-slot word); strings are packed at AGG_ARENA_ALIGN.
constexpr uint64_t PROV_BIT = 1ULL << 39;
constexpr uint64_t AGG_ARENA_MAX = PROV_BIT;
constexpr uint64_t AGG_ARENA_HEADER = 8;
constexpr uint64_t AGG_ARENA_ALIGN = 1;

RW_VARLEN_HD inline uint64_t pack(uint64_t off, uint32_t len) {
    return (off & MAX_OFF) | ((uint64_t)len << OFF_BITS);
}
RW_VARLEN_HD inline uint64_t word_off(uint64_t w) { return w & MAX_OFF; }
RW_VARLEN_HD inline uint32_t word_len(uint64_t w) {
    return (uint32_t)(w >> OFF_BITS);
}

// Offsets contract of RwVarlenData (rw_chunk.h): n_rows + 1 entries,
// offsets[0] == 0, non-decreasing, every string <= MAX_LEN bytes. Returns
// nullptr when the array is well formed, else a static description of the
// first violation. Reads only `offsets` (never the byte buffer).
inline const char* validate_offsets(const uint32_t* offsets, uint32_t n_rows) {
    if (!offsets) return "offsets is NULL";
    if (offsets[0] != 0) return "offsets[0] != 0";
    for (uint32_t r = 0; r < n_rows; r++) {
        if (offsets[r + 1] < offsets[r]) return "offsets decrease";
        if (offsets[r + 1] - offsets[r] > MAX_LEN)
            return "string longer than 2^24-1 bytes";
    }
    return nullptr;
}

// The input contract of one RW_T_VARCHAR column of n_rows rows: `data` set,
// well-formed offsets, and a byte buffer wherever there are bytes. Returns
// nullptr or the reason; the caller says which column. Every executor and
// entry point that accepts varchar columns checks them with this.
inline const char* check_column(const RwColumn& col, uint32_t n_rows) {
    auto* vd = (const RwVarlenData*)col.data;
    if (!vd) return "data is NULL";
    if (const char* why = validate_offsets(vd->offsets, n_rows)) return why;
    if (vd->offsets[n_rows] && !vd->bytes) return "bytes is NULL";
    return nullptr;
}

// Reference words of one uploaded varchar column whose bytes were placed at
// `base`: pack(flag | (base + offset), length) for a valid row, 0 for NULL.
// `flag` is 0 or PROV_BIT.
inline void ref_words(const RwVarlenData* vd, const uint8_t* valid, uint32_t n,
                      uint64_t base, uint64_t flag, std::vector<int64_t>& out) {
    out.resize(n);
    for (uint32_t r = 0; r < n; r++)
        out[r] = valid[r] ? (int64_t)pack(flag | (base + vd->offsets[r]),
                                          vd->offsets[r + 1] - vd->offsets[r])
                          : 0;
}

} // namespace rwvarlen
