// Stand-alone host check of the varchar codec and word helpers
// (include/rw_codec.hpp value_encode_str / value_decode_str,
// include/rw_varlen.hpp). Built and run by tests/test_varchar_host.py, once
// plain and once under -fsanitize=address,undefined. Exit 0 = all passed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rw_codec.hpp"
#include "../include/rw_varlen.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

static std::vector<uint8_t> enc(bool null, const std::string& s) {
    std::vector<uint8_t> b;
    rwcodec::value_encode_str(b, null, (const uint8_t*)s.data(),
                              (uint32_t)s.size());
    return b;
}

static void check_roundtrip(bool null, const std::string& s) {
    std::vector<uint8_t> b = enc(null, s);
    // exact-size heap copy: an over-read trips AddressSanitizer
    std::vector<uint8_t> heap(b.begin(), b.end());
    bool dn = !null;
    const uint8_t* p = nullptr;
    uint32_t len = 12345;
    size_t got = rwcodec::value_decode_str(heap.data(), heap.size(), &dn, &p,
                                           &len);
    CHECK(got == b.size());
    CHECK(dn == null);
    if (null) {
        CHECK(len == 0);
    } else {
        CHECK(len == s.size());
        CHECK(len == 0 || memcmp(p, s.data(), len) == 0);
    }
    // every truncated prefix must report 0 (and read nothing past it)
    for (size_t cut = 0; cut < b.size(); cut++) {
        std::vector<uint8_t> pre(b.begin(), b.begin() + cut);
        bool n2 = false;
        const uint8_t* p2 = nullptr;
        uint32_t l2 = 0;
        CHECK(rwcodec::value_decode_str(pre.data(), pre.size(), &n2, &p2,
                                        &l2) == 0);
    }
}

int main() {
    // golden bytes (serialize_str: presence, u32 LE length, bytes)
    const std::vector<uint8_t> hello = {0x01, 0x05, 0x00, 0x00, 0x00,
                                        0x68, 0x65, 0x6c, 0x6c, 0x6f};
    CHECK(enc(false, "hello") == hello);
    CHECK(enc(false, "") == (std::vector<uint8_t>{0x01, 0, 0, 0, 0}));
    CHECK(enc(true, "ignored") == (std::vector<uint8_t>{0x00}));

    check_roundtrip(false, "hello");
    check_roundtrip(false, "");
    check_roundtrip(true, "");
    check_roundtrip(false, std::string(300, 'x') + std::string("\0\xff", 2));
    // a datum followed by more row bytes decodes only itself
    {
        std::vector<uint8_t> b = enc(false, "ab");
        b.push_back(0x01);
        bool n = true;
        const uint8_t* p = nullptr;
        uint32_t l = 0;
        CHECK(rwcodec::value_decode_str(b.data(), b.size(), &n, &p, &l) == 7);
        CHECK(!n && l == 2 && p[0] == 'a' && p[1] == 'b');
    }
    // a length field claiming more than is there (incl. near-u32-max)
    {
        std::vector<uint8_t> b = {0x01, 0xff, 0xff, 0xff, 0xff, 'a'};
        bool n = false;
        const uint8_t* p = nullptr;
        uint32_t l = 0;
        CHECK(rwcodec::value_decode_str(b.data(), b.size(), &n, &p, &l) == 0);
    }

    // reference words: offset bits 0..39, length bits 40..63
    using namespace rwvarlen;
    CHECK(MAX_OFF == (1ULL << 40) - 1);
    CHECK(MAX_LEN == (1u << 24) - 1);
    {
        uint64_t w = pack(MAX_OFF, MAX_LEN);
        CHECK(w == ~0ULL);
        CHECK(word_off(w) == MAX_OFF && word_len(w) == MAX_LEN);
        w = pack(MAX_OFF, 0);
        CHECK(word_off(w) == MAX_OFF && word_len(w) == 0);
        w = pack(0, MAX_LEN);
        CHECK(word_off(w) == 0 && word_len(w) == MAX_LEN);
        w = pack(123456789012ULL, 77);
        CHECK(word_off(w) == 123456789012ULL && word_len(w) == 77);
        CHECK(pack(0, 0) == 0);
    }

    // offsets validation
    {
        const uint32_t ok[] = {0, 0, 5, 5, 9};
        CHECK(validate_offsets(ok, 4) == nullptr);
        const uint32_t empty[] = {0};
        CHECK(validate_offsets(empty, 0) == nullptr);
        const uint32_t nonzero0[] = {1, 2, 3};
        CHECK(validate_offsets(nonzero0, 2) != nullptr);
        const uint32_t nonmono[] = {0, 5, 4, 9};
        CHECK(validate_offsets(nonmono, 3) != nullptr);
        const uint32_t toolong[] = {0, 1u << 24};
        CHECK(validate_offsets(toolong, 1) != nullptr);
        const uint32_t maxlen[] = {0, (1u << 24) - 1};
        CHECK(validate_offsets(maxlen, 1) == nullptr);
        CHECK(validate_offsets(nullptr, 0) != nullptr);
    }

    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("varchar host check ok\n");
    return 0;
}
