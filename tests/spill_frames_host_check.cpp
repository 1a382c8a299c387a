// Stand-alone host check of the checkpoint spill framing in
// include/rw_codec.hpp: put_frame / for_each_frame / merge_frames, the
// KeyedDelta and write_sorted writers and the RowReader cursor. Built and run
// by tests/test_spill_frames_host.py, once plain and once under
// -fsanitize=address,undefined. Every buffer handed to a reader is a heap
// block of exactly its length, so an over-read trips AddressSanitizer.
// Exit 0 = all passed.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../include/rw_codec.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

using rwcodec::Bytes;

struct Frame {
    uint8_t put;
    Bytes k, v;
    bool operator==(const Frame& o) const {
        return put == o.put && k == o.k && v == o.v;
    }
};

static Bytes B(const std::string& s) { return Bytes(s.begin(), s.end()); }

// exact-size heap copy of the first n bytes
static std::unique_ptr<uint8_t[]> heap_copy(const Bytes& s, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n) memcpy(p.get(), s.data(), n);
    return p;
}

static bool read_frames(const Bytes& s, size_t n, std::vector<Frame>* out) {
    auto p = heap_copy(s, n);
    return rwcodec::for_each_frame(
        p.get(), n,
        [&](uint8_t put, const uint8_t* k, uint32_t klen, const uint8_t* v,
            uint32_t vlen) {
            out->push_back({put, Bytes(k, k + klen), Bytes(v, v + vlen)});
        });
}

static bool merge(const Bytes& s, size_t n, rwcodec::FrameMap* m) {
    auto p = heap_copy(s, n);
    return rwcodec::merge_frames(p.get(), n, *m);
}

static Bytes write_frames(const std::vector<Frame>& fs) {
    Bytes out;
    for (auto& f : fs) rwcodec::put_frame(out, f.put, f.k, f.v);
    return out;
}

static void check_round_trip() {
    std::vector<Frame> fs = {
        {1, {}, B("value of the empty key")},
        {1, B("empty value"), {}},
        {0, B("deleted"), {}},
        {1, {0x00, 0xff, 0x00, 0x00, 0xff, 0xff, 0x61}, {0xff, 0x00}},
        {0, {0x00}, {}},
        {1, {}, {}},
    };
    uint64_t x = 0x2545f4914f6cdd1dULL; // seeded xorshift
    auto next = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int i = 0; i < 40; i++) {
        Frame f;
        f.put = (uint8_t)(next() % 3 != 0);
        for (uint64_t n = next() % 40; n; n--) f.k.push_back((uint8_t)next());
        if (f.put)
            for (uint64_t n = next() % 300; n; n--)
                f.v.push_back((uint8_t)next());
        fs.push_back(f);
    }
    Bytes s = write_frames(fs);
    std::vector<Frame> got;
    CHECK(read_frames(s, s.size(), &got));
    CHECK(got == fs);
    // the pointer form writes the same bytes; a DELETE takes no value
    Bytes s2;
    for (auto& f : fs) {
        if (f.put)
            rwcodec::put_frame(s2, 1, f.k.data(), f.k.size(), f.v.data(),
                               f.v.size());
        else
            rwcodec::put_frame(s2, 0, f.k);
    }
    CHECK(s2 == s);
    got.clear();
    CHECK(read_frames(Bytes(), 0, &got) && got.empty()); // the empty stream
}

// [put u8][klen u32 LE][key][vlen u32 LE][value], written out by hand
static void check_pinned_layout() {
    Bytes s;
    rwcodec::put_frame(s, 1, B("ab"), {0x01, 0x02, 0x03});
    rwcodec::put_frame(s, 0, B("abc"));
    Bytes want = {0x01, 0x02, 0x00, 0x00, 0x00, 0x61, 0x62,
                  0x03, 0x00, 0x00, 0x00, 0x01, 0x02, 0x03,
                  0x00, 0x03, 0x00, 0x00, 0x00, 0x61, 0x62, 0x63,
                  0x00, 0x00, 0x00, 0x00};
    CHECK(s == want);
    Bytes big;
    rwcodec::put_frame(big, 1, Bytes(0x0102, 0x6b), Bytes(0x010203, 0x76));
    CHECK(big.size() == 1 + 4 + 0x0102 + 4 + 0x010203);
    CHECK(big[1] == 0x02 && big[2] == 0x01 && big[3] == 0 && big[4] == 0);
    size_t vo = 5 + 0x0102;
    CHECK(big[vo] == 0x03 && big[vo + 1] == 0x02 && big[vo + 2] == 0x01 &&
          big[vo + 3] == 0);
}

static void check_truncation() {
    std::vector<Frame> fs = {{1, B("k1"), B("first value")},
                             {0, B("key-two"), {}},
                             {1, B("k3"), {0x00, 0xff, 0x7f}}};
    Bytes s = write_frames(fs);
    std::vector<size_t> starts; // frame boundaries, incl. 0 and the end
    size_t off = 0;
    for (auto& f : fs) {
        starts.push_back(off);
        off += 9 + f.k.size() + f.v.size();
    }
    starts.push_back(off);
    CHECK(off == s.size());
    for (size_t cut = 0; cut <= s.size(); cut++) {
        size_t whole = 0; // frames that end at or before the cut
        bool boundary = false;
        for (size_t b = 0; b < starts.size(); b++) {
            if (starts[b] == cut) boundary = true;
            if (b && starts[b] <= cut) whole = b;
        }
        std::vector<Frame> got;
        CHECK(read_frames(s, cut, &got) == boundary);
        CHECK(got.size() <= whole);
        rwcodec::FrameMap m;
        CHECK(merge(s, cut, &m) == boundary);
    }
    // each length field in turn claims more than the stream holds
    for (size_t f = 0; f < fs.size(); f++) {
        size_t fields[2] = {starts[f] + 1, starts[f] + 5 + fs[f].k.size()};
        for (size_t field : fields) {
            uint32_t past = (uint32_t)(s.size() - (field + 4)) + 1;
            for (uint32_t bad : {past, past + 4, 0x7fffffffu, 0xffffffffu}) {
                Bytes t = s;
                for (int b = 0; b < 4; b++)
                    t[field + b] = (uint8_t)(bad >> (8 * b));
                std::vector<Frame> got;
                CHECK(!read_frames(t, t.size(), &got));
                CHECK(got.size() <= f);
                rwcodec::FrameMap m;
                CHECK(!merge(t, t.size(), &m));
            }
        }
    }
}

static void check_merge() {
    Bytes v1 = B("one"), v2 = B("two");
    rwcodec::FrameMap m;
    Bytes s = write_frames({{1, B("k"), v1}, {0, B("k"), {}}});
    CHECK(merge(s, s.size(), &m) && m.empty()); // PUT then DELETE
    s = write_frames({{0, B("k"), {}}, {1, B("k"), v1}});
    CHECK(merge(s, s.size(), &m) && m.size() == 1 && m["k"] == v1);
    m.clear();
    s = write_frames({{1, B("k"), v1}, {1, B("k"), v2}});
    CHECK(merge(s, s.size(), &m) && m.size() == 1 && m["k"] == v2);
    m.clear();
    // a DELETE of a key that was never put, and a key with 0x00 / 0xff
    std::string odd("\x00\xff\x00", 3);
    s = write_frames({{0, B("absent"), {}}, {1, B(odd), v1}});
    CHECK(merge(s, s.size(), &m) && m.size() == 1 && m[odd] == v1);
    m.clear();
    // two drains, concatenated or merged one after the other
    Bytes d1 = write_frames({{1, B("a"), v1}, {1, B("b"), v1}, {1, B("c"), v1}});
    Bytes d2 = write_frames({{0, B("a"), {}}, {1, B("b"), v2}, {1, B("d"), v2}});
    Bytes both = d1;
    both.insert(both.end(), d2.begin(), d2.end());
    rwcodec::FrameMap one, two;
    CHECK(merge(both, both.size(), &one));
    CHECK(merge(d1, d1.size(), &two) && merge(d2, d2.size(), &two));
    CHECK(one == two);
    rwcodec::FrameMap want = {{"b", v2}, {"c", v1}, {"d", v2}};
    CHECK(one == want);
}

static void check_writers() {
    Bytes v = B("v");
    rwcodec::KeyedDelta d;
    d.del(B("k"));
    d.put(B("k"), v);
    Bytes out;
    d.write(out);
    CHECK(out == write_frames({{1, B("k"), v}}));

    rwcodec::KeyedDelta e;
    e.put(B("k"), v);
    e.del(B("k"));
    out.clear();
    e.write(out);
    CHECK(out == write_frames({{0, B("k"), {}}}));

    // bytewise key order: unsigned bytes, a prefix before its extensions
    rwcodec::KeyedDelta o;
    o.put({0xff}, v);
    o.put({0x7f, 0x00}, v);
    o.del({0x80});
    o.put({0x7f}, {});
    o.put({}, v);
    o.del({0x00, 0xff});
    out.clear();
    o.write(out);
    CHECK(out == write_frames({{1, {}, v},
                               {0, {0x00, 0xff}, {}},
                               {1, {0x7f}, {}},
                               {1, {0x7f, 0x00}, v},
                               {0, {0x80}, {}},
                               {1, {0xff}, v}}));

    // collected records: ordered by key, equal keys keep their order
    std::vector<rwcodec::FrameRec> rs = {{1, {0x80}, B("p80")},
                                         {1, B("k"), B("put first")},
                                         {0, {0x80}, {}},
                                         {0, B("k"), {}},
                                         {1, {0x01}, v},
                                         {1, B("k"), B("put last")}};
    out.clear();
    rwcodec::write_sorted(out, rs);
    CHECK(out == write_frames({{1, {0x01}, v},
                               {1, B("k"), B("put first")},
                               {0, B("k"), {}},
                               {1, B("k"), B("put last")},
                               {1, {0x80}, B("p80")},
                               {0, {0x80}, {}}}));
}

// sort_spill_frames: stable, bytewise key order (a prefix before its
// extensions), a malformed stream left as it was
static void check_sort_frames() {
    Bytes s = write_frames({{1, {0x80}, B("p80")},
                            {1, B("k"), B("mid-window put")},
                            {1, {0x7f, 0x00}, B("ext")},
                            {0, B("k"), {}},
                            {1, {0x7f}, B("prefix")},
                            {0, {0x80}, {}},
                            {1, {}, B("empty key")}});
    Bytes sorted = write_frames({{1, {}, B("empty key")},
                                 {1, B("k"), B("mid-window put")},
                                 {0, B("k"), {}},
                                 {1, {0x7f}, B("prefix")},
                                 {1, {0x7f, 0x00}, B("ext")},
                                 {1, {0x80}, B("p80")},
                                 {0, {0x80}, {}}});
    Bytes got = s;
    got.shrink_to_fit();
    rwcodec::sort_spill_frames(got);
    CHECK(got == sorted);
    rwcodec::sort_spill_frames(got); // sorted already: unchanged
    CHECK(got == sorted);
    // the other order under one key stays the other order
    Bytes dp = write_frames({{0, B("k"), {}}, {1, B("k"), B("v")}, {1, {}, {}}});
    rwcodec::sort_spill_frames(dp);
    CHECK(dp == write_frames({{1, {}, {}}, {0, B("k"), {}}, {1, B("k"), B("v")}}));
    // a malformed tail, at every cut of the last frame and with stray bytes
    // after it: the buffer is left as it was
    for (size_t cut = 1; cut < 5 + 1 + 4 + 3; cut++) {
        Bytes bad(s.begin(), s.end() - cut);
        Bytes before = bad;
        rwcodec::sort_spill_frames(bad);
        CHECK(bad == before);
    }
    for (size_t extra = 1; extra <= 4; extra++) {
        Bytes bad = s;
        bad.insert(bad.end(), extra, 0x01);
        Bytes before = bad;
        rwcodec::sort_spill_frames(bad);
        CHECK(bad == before);
    }
    Bytes huge = s; // a key length that runs past the end
    huge[1] = huge[2] = huge[3] = huge[4] = 0xff;
    Bytes before = huge;
    rwcodec::sort_spill_frames(huge);
    CHECK(huge == before);
    Bytes none;
    rwcodec::sort_spill_frames(none);
    CHECK(none.empty());
}

static void check_row_reader() {
    const long long dec_lo = 0x0123456789abcdefLL, dec_hi = -7;
    const double f = -1234.5e-3;
    const std::string str("st\x00\xff\x00", 5);
    Bytes row;
    std::vector<size_t> ends; // end offset of each datum
    rwcodec::value_encode_datum(row, RW_T_I64, {false, -42, 0});
    ends.push_back(row.size());
    rwcodec::value_encode_datum(row, RW_T_I64, {true, 0, 0});
    ends.push_back(row.size());
    rwcodec::value_encode_datum(row, RW_T_DECIMAL,
                                {false, dec_lo, 0, dec_hi});
    ends.push_back(row.size());
    rwcodec::value_encode_datum(row, RW_T_F64,
                                rwcodec::DatumC{false, 0, f});
    ends.push_back(row.size());
    rwcodec::value_encode_str(row, false, (const uint8_t*)str.data(),
                              (uint32_t)str.size());
    ends.push_back(row.size());
    CHECK(ends == (std::vector<size_t>{9, 10, 27, 36, 41 + str.size()}));

    // reads datums until one fails; returns how many came back
    auto decode = [&](size_t n, bool check_values) {
        auto p = heap_copy(row, n);
        rwcodec::RowReader rd{p.get(), n};
        rwcodec::DatumC d;
        int got = 0;
        if (!rd.datum(RW_T_I64, &d)) return got;
        if (check_values) CHECK(!d.null && d.i == -42);
        got++;
        if (!rd.datum(RW_T_I64, &d)) return got;
        if (check_values) CHECK(d.null);
        got++;
        if (!rd.datum(RW_T_DECIMAL, &d)) return got;
        if (check_values) CHECK(!d.null && d.i == dec_lo && d.i2 == dec_hi);
        got++;
        if (!rd.datum(RW_T_F64, &d)) return got;
        if (check_values) CHECK(!d.null && d.d == f);
        got++;
        bool null = true;
        const uint8_t* s = nullptr;
        uint32_t len = 0;
        if (!rd.str(&null, &s, &len)) return got;
        if (check_values)
            CHECK(!null && std::string((const char*)s, len) == str);
        got++;
        CHECK(rd.off == n);
        // the row is used up: nothing more comes back
        CHECK(!rd.datum(RW_T_I64, &d));
        CHECK(!rd.str(&null, &s, &len));
        return got;
    };
    CHECK(decode(row.size(), true) == 5);
    for (size_t cut = 0; cut < row.size(); cut++) {
        int whole = 0; // datums that end at or before the cut
        while (ends[whole] <= cut) whole++;
        CHECK(decode(cut, true) == whole);
    }
    // an unknown type tag is refused, not skipped
    {
        auto p = heap_copy(row, row.size());
        rwcodec::RowReader rd{p.get(), row.size()};
        rwcodec::DatumC d;
        CHECK(!rd.datum(0xee, &d));
        CHECK(rd.off == 0);
    }
    // a string whose length field runs past the row
    {
        Bytes bad = {1, 0xff, 0xff, 0xff, 0xff, 'x'};
        auto p = heap_copy(bad, bad.size());
        rwcodec::RowReader rd{p.get(), bad.size()};
        bool null = false;
        const uint8_t* s = nullptr;
        uint32_t len = 0;
        CHECK(!rd.str(&null, &s, &len));
    }
}

int main() {
    check_round_trip();
    check_pinned_layout();
    check_truncation();
    check_merge();
    check_writers();
    check_sort_frames();
    check_row_reader();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("spill frames host check ok\n");
    return 0;
}
