// Stand-alone host check of the pieces HashAgg's varchar group keys add to
// the spill codec (include/rw_codec.hpp memcmp_encode_str, and
// value_encode_str / value_decode_str inside a multi-column row). Built and
// run by tests/test_varchar_agg_host.py, once plain and once under
// -fsanitize=address,undefined. Exit 0 = all passed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
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

typedef std::vector<uint8_t> Bytes;

static Bytes enc(bool null, const std::string& s) {
    // exact-size heap copy of the input: an over-read trips AddressSanitizer
    Bytes in(s.begin(), s.end());
    Bytes b;
    rwcodec::memcmp_encode_str(b, null, in.data(), (uint32_t)in.size());
    return b;
}

static Bytes hex(std::initializer_list<int> xs) {
    Bytes b;
    for (int x : xs) b.push_back((uint8_t)x);
    return b;
}

static void check_pinned() {
    CHECK(enc(false, "") == hex({0x00, 0x00}));
    CHECK(enc(false, "abc") == hex({0x00, 0x01, 0x61, 0x62, 0x63, 0, 0, 0, 0,
                                    0, 0x03}));
    CHECK(enc(false, "abcdefgh") == hex({0x00, 0x01, 0x61, 0x62, 0x63, 0x64,
                                         0x65, 0x66, 0x67, 0x68, 0x08}));
    CHECK(enc(false, "abcdefghi") ==
          hex({0x00, 0x01, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
               0x09, 0x69, 0, 0, 0, 0, 0, 0, 0, 0x01}));
    CHECK(enc(true, "") == hex({0x01}));
    CHECK(enc(true, "ignored") == hex({0x01}));
    // ASC NULLS LAST: NULL sorts after every string
    CHECK(enc(false, std::string(40, '\xff')) < enc(true, ""));
}

// byte-string order (std::string compares as unsigned bytes, shorter prefix
// first) must equal encoding order, and distinct strings must encode apart
static void check_order_and_injective() {
    std::vector<std::string> ss = {
        "", std::string(1, '\0'), std::string(8, '\0'), std::string(9, '\0'),
        "abcdefg", "abcdefgh", "abcdefghi", "abcdefghijklmnop",
        std::string(64, 'p') + "A", std::string(64, 'p') + "B",
        std::string(64, 'p'), std::string(7, '\0'), std::string(16, '\0'),
        "\x01", std::string("a\0", 2), "a", std::string("a\0b", 3),
        "\xff", "\xff\xff\xff\xff\xff\xff\xff\xff",
        "\xff\xff\xff\xff\xff\xff\xff\xff\xff"};
    uint64_t x = 0x9e3779b97f4a7c15ULL; // seeded xorshift
    auto next = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int i = 0; i < 4000; i++) {
        uint32_t len = (uint32_t)(next() % 20);
        std::string s;
        // small alphabet incl. 0x00 and 0xff: many shared prefixes and ties
        static const char alpha[] = {'\0', '\x01', 'a', 'b', '\xff'};
        for (uint32_t k = 0; k < len; k++) s.push_back(alpha[next() % 5]);
        ss.push_back(s);
    }
    std::sort(ss.begin(), ss.end(), [](const std::string& a,
                                       const std::string& b) {
        size_t n = std::min(a.size(), b.size());
        int c = n ? memcmp(a.data(), b.data(), n) : 0;
        return c ? c < 0 : a.size() < b.size();
    });
    ss.erase(std::unique(ss.begin(), ss.end()), ss.end());
    CHECK(ss.size() > 3000);
    for (size_t i = 0; i + 1 < ss.size(); i++) {
        Bytes a = enc(false, ss[i]), b = enc(false, ss[i + 1]);
        CHECK(a < b); // strict: order preserved AND injective
        // length law: tag + marker + 9 bytes per started group of 8
        CHECK(a.size() == (ss[i].empty() ? 2 : 2 + 9 * ((ss[i].size() + 7) / 8)));
    }
    // a few random non-adjacent pairs as well
    for (int i = 0; i < 4000; i++) {
        const std::string& p = ss[next() % ss.size()];
        const std::string& q = ss[next() % ss.size()];
        bool lt = std::lexicographical_compare(
            (const uint8_t*)p.data(), (const uint8_t*)p.data() + p.size(),
            (const uint8_t*)q.data(), (const uint8_t*)q.data() + q.size());
        CHECK((enc(false, p) < enc(false, q)) == lt);
    }
}

// (i64, varchar, NULL varchar, varchar "", i64 NULL, varchar) as one value
// row: encode, decode in order, and every cut of the row must be refused
static void check_value_row() {
    std::string s1 = "name-\xc3\xa9", s3 = "", s5(300, 'z');
    Bytes row;
    rwcodec::value_encode_datum(row, RW_T_I64, {false, -42, 0});
    rwcodec::value_encode_str(row, false, (const uint8_t*)s1.data(),
                              (uint32_t)s1.size());
    rwcodec::value_encode_str(row, true, nullptr, 0);
    rwcodec::value_encode_str(row, false, (const uint8_t*)s3.data(), 0);
    rwcodec::value_encode_datum(row, RW_T_I64, {true, 0, 0});
    rwcodec::value_encode_str(row, false, (const uint8_t*)s5.data(),
                              (uint32_t)s5.size());
    auto decode = [&](const Bytes& heap, std::vector<std::string>* out) {
        size_t off = 0;
        rwcodec::DatumC d;
        size_t got = rwcodec::value_decode_datum(heap.data() + off,
                                                 heap.size() - off, RW_T_I64,
                                                 &d);
        if (!got) return false;
        off += got;
        out->push_back(d.null ? "NULL" : std::to_string(d.i));
        for (int k = 0; k < 5; k++) {
            if (k == 3) {
                got = rwcodec::value_decode_datum(heap.data() + off,
                                                  heap.size() - off, RW_T_I64,
                                                  &d);
                if (!got) return false;
                off += got;
                out->push_back(d.null ? "NULL" : std::to_string(d.i));
                continue;
            }
            bool null = false;
            const uint8_t* p = nullptr;
            uint32_t len = 0;
            got = rwcodec::value_decode_str(heap.data() + off,
                                            heap.size() - off, &null, &p, &len);
            if (!got) return false;
            off += got;
            out->push_back(null ? "NULL" : "s:" + std::string((const char*)p, len));
        }
        return off == heap.size();
    };
    std::vector<std::string> got;
    CHECK(decode(Bytes(row.begin(), row.end()), &got));
    std::vector<std::string> want = {"-42", "s:" + s1, "NULL", "s:", "NULL",
                                     "s:" + s5};
    CHECK(got == want);
    for (size_t cut = 0; cut < row.size(); cut++) {
        std::vector<std::string> g;
        Bytes heap(row.begin(), row.begin() + cut); // exact-size: ASan guard
        CHECK(!decode(heap, &g));
    }
}

int main() {
    check_pinned();
    check_order_and_injective();
    check_value_row();
    // the provisional bit lives inside the offset field and leaves the
    // length alone
    uint64_t w = rwvarlen::pack(rwvarlen::PROV_BIT | 12345, 77);
    CHECK(rwvarlen::word_len(w) == 77);
    CHECK((rwvarlen::word_off(w) & ~rwvarlen::PROV_BIT) == 12345);
    CHECK(rwvarlen::pack(rwvarlen::AGG_ARENA_HEADER, 0) != 0);
    CHECK(rwvarlen::pack(rwvarlen::PROV_BIT, 0) != 0);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("agg varchar host check ok\n");
    return 0;
}
