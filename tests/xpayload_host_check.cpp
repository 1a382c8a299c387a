// Stand-alone host check of include/rw_xpayload.hpp: the per-destination
// block layout and the host version of the vnode CRC feed. Built and run by
// tests/test_xpayload_host.py, once plain and once under
// -fsanitize=address,undefined. Exit 0 = all passed.
//
// argv[1] names a vector file the Python test wrote with zlib as reference:
// one case per line, "<crc32 hex> <datum> <datum> ...", a datum being
//   i<decimal>   non-NULL i64
//   n            NULL
//   s<hex>       non-NULL varchar ("s" alone = the empty string)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/rw_xpayload.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

// rw_exchange_run's private block_bytes lambda, verbatim
static uint64_t old_block_bytes(uint64_t n_cols, uint64_t nrows) {
    uint64_t npad = (nrows + 3) & ~3ull;
    return ((uint64_t)n_cols * npad * 8 + (uint64_t)n_cols * nrows + nrows +
            31) & ~31ull;
}

static void check_layout() {
    const uint64_t ns[] = {0, 1, 3, 4, 5, 255, 256, 257};
    for (uint64_t n : ns)
        for (uint64_t C = 1; C <= 8; C++) {
            rwx::BlockLayout L = rwx::block_layout(n, C, 0);
            uint64_t npad = (n + 3) & ~3ull;
            CHECK(L.total == old_block_bytes(C, n));
            CHECK(rwx::block_bytes(n, C, 0) == old_block_bytes(C, n));
            // the old scatter kernel's offsets
            for (uint64_t c = 0; c < C; c++) {
                CHECK(L.vals_off(c) == c * npad * 8);
                CHECK(L.vals_off(c) % 32 == 0);
            }
            CHECK(L.valid_off == C * npad * 8);
            CHECK(L.ops_off == C * npad * 8 + C * n);
            CHECK(L.vbytes_off == L.total);
            const uint64_t vs[] = {1, 31, 32, 33, 70000};
            for (uint64_t V : vs) {
                rwx::BlockLayout W = rwx::block_layout(n, C, V);
                CHECK(W.valid_off == L.valid_off && W.ops_off == L.ops_off);
                CHECK(W.vbytes_off == L.total);
                CHECK(W.vbytes_off % 32 == 0 && W.total % 32 == 0);
                CHECK(W.total >= W.vbytes_off + V);
                CHECK(W.total - (W.vbytes_off + V) < 32);
            }
        }
    CHECK(rwx::dest_of_vnode(0, 256, 1) == 0);
    CHECK(rwx::dest_of_vnode(255, 256, 1) == 0);
    CHECK(rwx::dest_of_vnode(255, 256, 3) == 2); // 85 per dest, clamp
    CHECK(rwx::dest_of_vnode(254, 256, 3) == 2);
    CHECK(rwx::dest_of_vnode(84, 256, 3) == 0);
    CHECK(rwx::dest_of_vnode(85, 256, 3) == 1);
    CHECK(rwx::dest_of_vnode(99, 100, 64) == 63);
}

static int check_vectors(const char* path) {
    static uint32_t lut[8 * 256];
    rwx::crc_build_tables(lut);
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", path);
        return 0;
    }
    int cases = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        ss >> tok;
        uint32_t want = (uint32_t)strtoul(tok.c_str(), nullptr, 16);
        std::vector<std::string> datums;
        while (ss >> tok) datums.push_back(tok);
        // every alignment of the string start: the head / aligned-group /
        // tail split must not change the feed
        for (size_t shift = 0; shift < 8; shift++) {
            uint32_t crc = 0xFFFFFFFFu;
            for (const std::string& d : datums) {
                if (d[0] == 'n') {
                    crc = rwx::crc_feed_u32(lut, crc, rwx::NULL_SENTINEL);
                } else if (d[0] == 'i') {
                    crc = rwx::crc_feed_u64(
                        lut, crc, (uint64_t)strtoll(d.c_str() + 1, nullptr, 10));
                } else {
                    size_t len = (d.size() - 1) / 2;
                    // exact-size heap buffer: an over-read trips ASan
                    std::vector<uint8_t> heap(shift + len);
                    for (size_t i = 0; i < len; i++)
                        heap[shift + i] = (uint8_t)strtoul(
                            d.substr(1 + 2 * i, 2).c_str(), nullptr, 16);
                    crc = rwx::crc_feed_str(lut, crc, heap.data() + shift,
                                            (uint32_t)len);
                }
            }
            CHECK((crc ^ 0xFFFFFFFFu) == want);
        }
        cases++;
    }
    return cases;
}

int main(int argc, char** argv) {
    check_layout();
    if (argc < 2) {
        fprintf(stderr, "usage: %s <vector file>\n", argv[0]);
        return 2;
    }
    int cases = check_vectors(argv[1]);
    CHECK(cases > 0);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("xpayload host check ok (%d crc vectors)\n", cases);
    return 0;
}
