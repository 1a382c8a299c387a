// rw_xpayload.hpp — the exchange hop's per-destination block layout and the
// vnode CRC feed of a varchar datum. Usable from host code
// without HIP; rw_exchange.hip and rw_amd.hip include it for the device side.
//
// One block per destination, n rows, C columns, V varchar bytes:
//
//     vals[C][npad] i64   npad = n rounded up to 4 (every vals[c] 32-B aligned)
//     valid[C][n]   u8
//     ops[n]        u8
//     pad to 32
//     vbytes[V]     u8    one byte region, shared by all varchar columns
//     pad to 32
//
// With V == 0 the size and every offset equal the all-i64 layout of
// rw_exchange_run. A varchar column's vals entry is a rwvarlen::pack(off,
// len) word with `off` relative to the block's vbytes region; a NULL cell is
// word 0 with its valid byte 0 and owns no bytes. The live words' ranges are
// pairwise disjoint, in bounds and cover vbytes exactly; their order, like
// the row order inside a block, is unspecified.
#pragma once
#include <cstdint>

#include "rw_varlen.hpp"

namespace rwx {

RW_VARLEN_HD inline uint64_t pad32(uint64_t x) { return (x + 31) & ~31ull; }

struct BlockLayout {
    uint64_t n, npad, n_cols;
    uint64_t valid_off;  // valid[c] at valid_off + c * n
    uint64_t ops_off;
    uint64_t vbytes_off; // 32-aligned
    uint64_t total;      // 32-aligned
    RW_VARLEN_HD uint64_t vals_off(uint64_t c) const { return c * npad * 8; }
};

RW_VARLEN_HD inline BlockLayout block_layout(uint64_t n, uint64_t n_cols,
                                             uint64_t vbytes) {
    BlockLayout L;
    L.n = n;
    L.n_cols = n_cols;
    L.npad = (n + 3) & ~3ull;
    L.valid_off = n_cols * L.npad * 8;
    L.ops_off = L.valid_off + n_cols * n;
    L.vbytes_off = pad32(L.ops_off + n);
    L.total = L.vbytes_off + pad32(vbytes);
    return L;
}

RW_VARLEN_HD inline uint64_t block_bytes(uint64_t n, uint64_t n_cols,
                                         uint64_t vbytes) {
    return block_layout(n, n_cols, vbytes).total;
}

// ---- the vnode CRC feed (VirtualNode::compute_chunk → hash_datum into a
// crc32fast::Hasher, which implements only Hasher::write) ----
//   non-NULL i64/ts   8 little-endian bytes
//   NULL              u32 0xfffffff0, little-endian
//   non-NULL varchar  the bytes, then one 0xFF (impl Hash for str →
//                     Hasher::write_str, whose default is write(bytes)
//                     followed by write_u8(0xff)); "" feeds the single 0xFF
// The tables are slicing-by-8: T0 the plain byte table, Tk[i] = (Tk-1[i] >>
// 8) ^ T0[Tk-1[i] & 0xff]. `lut` below is those 8 * 256 words, in LDS on the
// device.

constexpr uint32_t NULL_SENTINEL = 0xfffffff0u;

inline void crc_build_tables(uint32_t tab[8 * 256]) {
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        tab[i] = c;
    }
    for (int k = 1; k < 8; k++)
        for (int i = 0; i < 256; i++) {
            uint32_t p = tab[(k - 1) * 256 + i];
            tab[k * 256 + i] = (p >> 8) ^ tab[p & 0xff];
        }
}

RW_VARLEN_HD inline uint32_t crc_feed_u8(const uint32_t* lut, uint32_t crc,
                                         uint8_t b) {
    return lut[(crc ^ b) & 0xff] ^ (crc >> 8);
}

RW_VARLEN_HD inline uint32_t crc_feed_u32(const uint32_t* lut, uint32_t crc,
                                          uint32_t w) {
    uint32_t t = crc ^ w;
    return lut[3 * 256 + (t & 0xff)] ^ lut[2 * 256 + ((t >> 8) & 0xff)] ^
           lut[1 * 256 + ((t >> 16) & 0xff)] ^ lut[0 * 256 + (t >> 24)];
}

RW_VARLEN_HD inline uint32_t crc_feed_u64(const uint32_t* lut, uint32_t crc,
                                          uint64_t v) {
    uint32_t lo = crc ^ (uint32_t)v;
    uint32_t hi = (uint32_t)(v >> 32);
    return lut[7 * 256 + (lo & 0xff)] ^ lut[6 * 256 + ((lo >> 8) & 0xff)] ^
           lut[5 * 256 + ((lo >> 16) & 0xff)] ^ lut[4 * 256 + (lo >> 24)] ^
           lut[3 * 256 + (hi & 0xff)] ^ lut[2 * 256 + ((hi >> 8) & 0xff)] ^
           lut[1 * 256 + ((hi >> 16) & 0xff)] ^ lut[0 * 256 + (hi >> 24)];
}

// A non-NULL varchar datum. Strings sit at arbitrary byte addresses: the
// bytes before the first 8-aligned address go through the byte table (CRC is
// sequential, so this is the same feed), then whole aligned 8-byte groups
// through slicing-by-8, then the tail bytes, then the 0xFF.
RW_VARLEN_HD inline uint32_t crc_feed_str(const uint32_t* lut, uint32_t crc,
                                          const uint8_t* p, uint32_t len) {
    const uint8_t* end = p + len;
    while (p < end && ((uintptr_t)p & 7)) crc = crc_feed_u8(lut, crc, *p++);
    while (end - p >= 8) {
        uint64_t v; // one aligned 8-byte load
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8);
        crc = crc_feed_u64(lut, crc, v);
        p += 8;
    }
    while (p < end) crc = crc_feed_u8(lut, crc, *p++);
    return crc_feed_u8(lut, crc, 0xff);
}

// vnode → destination: contiguous vnode blocks, the last one absorbing the
// remainder of a non-dividing count
RW_VARLEN_HD inline uint32_t dest_of_vnode(uint32_t vnode, uint32_t vnode_count,
                                           uint32_t n_dests) {
    uint32_t per = vnode_count / n_dests;
    uint32_t d = per ? vnode / per : n_dests - 1;
    return d < n_dests ? d : n_dests - 1;
}

} // namespace rwx
