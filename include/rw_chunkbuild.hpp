// rw_chunkbuild.hpp — the host side of every RwChunk the product hands out
// (DESIGN.md §21): the free routine, the builder whose allocations it undoes,
// the rule that cuts an output block into chunks, and the queue an executor
// keeps its unpolled chunks in. No HIP: tests/chunk_build_host_check.cpp
// builds it with the host compiler under ASan + UBSan.
//
// Allocation types, each freed by free_chunk with the matching delete:
//     RwChunk          new RwChunk
//     cols             new RwColumn[n_cols]
//     ops, vis, valid  new uint8_t[n]
//     fixed data       new int64_t[words]   (every width; bytes round up)
//     varchar data     new RwVarlenData, offsets new uint32_t[n + 1],
//                      bytes new uint8_t[total, at least 1]
#pragma once
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <utility>
#include <vector>

#include "rw_chunk.h"
#include "rw_varlen.hpp"

namespace rwchunk {

// Frees a chunk in any state the Builder leaves it in: n_cols counts the
// columns that were started, and a pointer is null until it is set.
inline void free_chunk(RwChunk* ch) {
    if (!ch) return;
    for (uint32_t c = 0; c < ch->n_cols; c++) {
        delete[] ch->cols[c].valid;
        if (ch->cols[c].type == RW_T_VARCHAR) {
            auto* vd = (const RwVarlenData*)ch->cols[c].data;
            if (vd) {
                delete[] vd->offsets;
                delete[] vd->bytes;
                delete vd;
            }
        } else {
            delete[] (int64_t*)ch->cols[c].data;
        }
    }
    delete[] ch->cols;
    delete[] ch->ops;
    delete[] ch->vis;
    delete ch;
}
struct ChunkFree {
    void operator()(RwChunk* c) const { free_chunk(c); }
};
typedef std::unique_ptr<RwChunk, ChunkFree> ChunkPtr;

// Where a column's valid bytes come from: a strided block of null flags
// (valid = !null) or another column's valid bytes, copied as they are.
struct ValidSrc {
    const uint8_t* p;
    size_t stride;
    bool negate;
};
inline ValidSrc from_nulls(const uint8_t* p, size_t stride) {
    return {p, stride, true};
}
inline ValidSrc from_valid(const uint8_t* p) { return {p, 1, false}; }

// One chunk of n rows under construction. Columns are added in order, each by
// one filler; the sources point at the chunk's FIRST row, so a row-major
// block is (&block[start * width + c], width) and a column-major one
// (&block[c * rows + start], 1). The chunk is freed unless release() hands it
// out, also when an allocation throws half way through a column.
class Builder {
    ChunkPtr ch_;
    RwColumn* cols_;
    uint32_t n_;

    RwColumn& start_col(uint8_t type, ValidSrc v) {
        RwColumn& c = cols_[ch_->n_cols];
        c.type = type;
        ch_->n_cols++;
        auto* valid = new uint8_t[n_];
        c.valid = valid;
        for (uint32_t r = 0; r < n_; r++)
            valid[r] = v.negate ? !v.p[r * v.stride] : v.p[r * v.stride];
        return c;
    }
    static uint8_t* copy_bytes(const uint8_t* src, uint32_t n) {
        auto* p = new uint8_t[n];
        if (n) memcpy(p, src, n);
        return p;
    }

public:
    Builder(uint32_t n, uint32_t n_cols) : ch_(new RwChunk()), n_(n) {
        ch_->n_rows = n;
        ch_->cols = cols_ = new RwColumn[n_cols]();
    }

    // 8-byte values, row r at vals[r * stride]
    void fixed(uint8_t type, const int64_t* vals, size_t stride, ValidSrc v) {
        RwColumn& c = start_col(type, v);
        auto* data = new int64_t[n_];
        c.data = data;
        for (uint32_t r = 0; r < n_; r++) data[r] = vals[r * stride];
    }

    // 16-byte decimals from their two words
    void decimal(const int64_t* lo, const int64_t* hi, size_t stride,
                 ValidSrc v) {
        RwColumn& c = start_col(RW_T_DECIMAL, v);
        auto* data = new int64_t[(size_t)2 * n_];
        c.data = data;
        for (uint32_t r = 0; r < n_; r++) {
            data[2 * r] = lo[r * stride];
            data[2 * r + 1] = hi[r * stride];
        }
    }

    // a fixed-width column of any type, copied as it is
    void raw(uint8_t type, const void* src, ValidSrc v) {
        RwColumn& c = start_col(type, v);
        size_t bytes = (size_t)n_ * rw_type_size(type);
        auto* data = new int64_t[(bytes + 7) / 8];
        c.data = data;
        if (bytes) memcpy(data, src, bytes);
    }

    // Varchar: row r is src[offs[i]..offs[i + 1]) with i = map ? map[r] : r,
    // so without a map offs has n + 1 entries and the rows are contiguous.
    // Offsets are rebased to 0; the bytes allocation is never null. Returns
    // false, with no column added, when the rows total more than UINT32_MAX
    // bytes: the sum is taken from the offsets before anything is allocated.
    bool varchar(const uint64_t* offs, const uint8_t* src, const uint32_t* map,
                 ValidSrc v) {
        uint64_t total = map ? 0 : offs[n_] - offs[0];
        for (uint32_t r = 0; map && r < n_; r++)
            total += offs[map[r] + 1] - offs[map[r]];
        if (total > UINT32_MAX) return false;
        RwColumn& c = start_col(RW_T_VARCHAR, v);
        auto* vd = new RwVarlenData{nullptr, nullptr};
        c.data = vd;
        auto* o = new uint32_t[(size_t)n_ + 1];
        vd->offsets = o;
        auto* bytes = new uint8_t[total ? total : 1];
        vd->bytes = bytes;
        uint32_t at = 0;
        for (uint32_t r = 0; r < n_; r++) {
            uint32_t i = map ? map[r] : r;
            uint32_t len = (uint32_t)(offs[i + 1] - offs[i]);
            o[r] = at;
            if (map && len) memcpy(bytes + at, src + offs[i], len);
            at += len;
        }
        o[n_] = at;
        if (!map && at) memcpy(bytes, src + offs[0], at);
        return true;
    }

    void ops(const uint8_t* src) { ch_->ops = copy_bytes(src, n_); }
    void vis(const uint8_t* src) { ch_->vis = copy_bytes(src, n_); }

    RwChunk* release() { return ch_.release(); }
};

// Cuts n_out output rows into consecutive (start, take) ranges of at most
// max_rows rows. With `ops` the U-/U+ pair rule holds
// (stream_chunk_builder.rs:188-218): a range that would end on an
// UpdateDelete with rows still to come takes the UpdateInsert too. Without
// `ops` every range but the last has exactly max_rows rows.
typedef std::pair<uint32_t, uint32_t> Range;
inline std::vector<Range> slice_ranges(uint32_t n_out, uint32_t max_rows,
                                       const uint8_t* ops) {
    std::vector<Range> out;
    if (!max_rows) max_rows = 1;
    for (uint32_t s = 0; s < n_out;) {
        uint32_t take = n_out - s < max_rows ? n_out - s : max_rows;
        if (ops && s + take < n_out && ops[s + take - 1] == RW_OP_UPDATE_DELETE)
            take++;
        out.push_back({s, take});
        s += take;
    }
    return out;
}

// An executor's unpolled output chunks: FIFO; what is never polled is freed
// with the queue.
class ChunkQueue {
    std::deque<ChunkPtr> q_;

public:
    void push(RwChunk* c) { q_.emplace_back(c); }
    RwChunk* poll() { // null when empty
        if (q_.empty()) return nullptr;
        RwChunk* c = q_.front().release();
        q_.pop_front();
        return c;
    }
};

} // namespace rwchunk
