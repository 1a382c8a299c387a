// Stand-alone host check of include/rw_chunkbuild.hpp (free_chunk, Builder,
// slice_ranges, ChunkQueue) and of the varchar column check and the
// reference-word loop in include/rw_varlen.hpp. Built and run by
// tests/test_chunk_build_host.py, once plain and once under
// -fsanitize=address,undefined. Every chunk built here is freed by
// free_chunk, directly or through the Builder / ChunkQueue destructors, so
// ASan's alloc-dealloc-mismatch check and LeakSanitizer cover every path.
// Source blocks are heap blocks of exactly their length, so an over-read
// trips AddressSanitizer. Exit 0 = all passed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rw_chunkbuild.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

using rwchunk::Builder;
using rwchunk::from_nulls;
using rwchunk::from_valid;
using rwchunk::Range;
typedef std::vector<uint8_t> U8;
typedef std::vector<int64_t> I64;

static I64 col_i64(const RwChunk* ch, uint32_t c, size_t words) {
    auto* p = (const int64_t*)ch->cols[c].data;
    return I64(p, p + words);
}
static U8 col_valid(const RwChunk* ch, uint32_t c) {
    return U8(ch->cols[c].valid, ch->cols[c].valid + ch->n_rows);
}

// ---- fixed columns: a 5 x 3 block, row-major and column-major ----
// column 0: 10..14, no NULLs; column 1: 20..24, rows 1 and 4 NULL;
// column 2: decimal low words 30..34 with high words 40..44, row 2 NULL
static const int64_t V[5][3] = {
    {10, 20, 30}, {11, 21, 31}, {12, 22, 32}, {13, 23, 33}, {14, 24, 34}};
static const int64_t HI[5] = {40, 41, 42, 43, 44};
static const uint8_t NUL[5][3] = {
    {0, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}, {0, 1, 0}};

static void check_fixed() {
    const uint32_t R = 5, W = 3;
    for (int colmajor = 0; colmajor < 2; colmajor++) {
        I64 vals(R * W), hi(R * W, -1);
        U8 nulls(R * W);
        auto at = [&](uint32_t r, uint32_t c) {
            return colmajor ? (size_t)c * R + r : (size_t)r * W + c;
        };
        for (uint32_t r = 0; r < R; r++)
            for (uint32_t c = 0; c < W; c++) {
                vals[at(r, c)] = V[r][c];
                nulls[at(r, c)] = NUL[r][c];
            }
        for (uint32_t r = 0; r < R; r++) hi[at(r, 2)] = HI[r];
        size_t stride = colmajor ? 1 : W;
        const uint32_t slices[3][2] = {{0, 2}, {2, 3}, {0, 5}};
        for (auto& sl : slices) {
            uint32_t s = sl[0], n = sl[1];
            U8 ops(R, RW_OP_INSERT);
            ops[2] = RW_OP_DELETE;
            Builder b(n, W);
            b.fixed(RW_T_I64, &vals[at(s, 0)], stride,
                    from_nulls(&nulls[at(s, 0)], stride));
            b.fixed(RW_T_TS, &vals[at(s, 1)], stride,
                    from_nulls(&nulls[at(s, 1)], stride));
            b.decimal(&vals[at(s, 2)], &hi[at(s, 2)], stride,
                      from_nulls(&nulls[at(s, 2)], stride));
            b.ops(&ops[s]);
            RwChunk* ch = b.release();
            CHECK(ch->n_rows == n && ch->n_cols == W && ch->vis == nullptr);
            CHECK(ch->cols[0].type == RW_T_I64 && ch->cols[1].type == RW_T_TS &&
                  ch->cols[2].type == RW_T_DECIMAL);
            I64 e0, e1, e2;
            U8 v0, v1, v2, eo;
            for (uint32_t r = s; r < s + n; r++) {
                e0.push_back(V[r][0]);
                e1.push_back(V[r][1]);
                e2.push_back(V[r][2]);
                e2.push_back(HI[r]);
                v0.push_back(1);
                v1.push_back(r != 1 && r != 4);
                v2.push_back(r != 2);
                eo.push_back(r == 2 ? RW_OP_DELETE : RW_OP_INSERT);
            }
            CHECK(col_i64(ch, 0, n) == e0 && col_valid(ch, 0) == v0);
            CHECK(col_i64(ch, 1, n) == e1 && col_valid(ch, 1) == v1);
            CHECK(col_i64(ch, 2, 2 * n) == e2 && col_valid(ch, 2) == v2);
            CHECK(U8(ch->ops, ch->ops + n) == eo);
            rwchunk::free_chunk(ch);
        }
    }
    // hand-written: rows 2..4, whichever the layout
    {
        I64 vals = {10, 11, 12, 13, 14, 20, 21, 22, 23, 24}; // column-major
        U8 nulls = {0, 0, 0, 0, 0, 0, 1, 0, 0, 1};
        U8 ops(3, RW_OP_INSERT);
        Builder b(3, 1);
        b.fixed(RW_T_I64, &vals[5 + 2], 1, from_nulls(&nulls[5 + 2], 1));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        CHECK(col_i64(ch, 0, 3) == (I64{22, 23, 24}));
        CHECK(col_valid(ch, 0) == (U8{1, 1, 0}));
        rwchunk::free_chunk(ch);
    }
}

// ---- varchar ----
struct Str {
    std::vector<uint32_t> offs;
    std::string bytes;
};
static Str col_str(const RwChunk* ch, uint32_t c) {
    auto* vd = (const RwVarlenData*)ch->cols[c].data;
    Str s;
    s.offs.assign(vd->offsets, vd->offsets + ch->n_rows + 1);
    s.bytes.assign((const char*)vd->bytes, vd->offsets[ch->n_rows]);
    CHECK(vd->bytes != nullptr);
    return s;
}

static void check_varchar() {
    // six block rows: "ab", NULL (length 0), "cde", "" (valid), "f", "ghij"
    std::vector<uint64_t> offs = {0, 2, 2, 5, 5, 6, 10};
    U8 src = {'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', 'j'};
    U8 nulls = {0, 1, 0, 0, 0, 0};
    U8 ops(6, RW_OP_INSERT);
    { // identity, rows 0..3: NULL between two strings, then the empty one
        Builder b(4, 1);
        CHECK(b.varchar(&offs[0], src.data(), nullptr, from_nulls(&nulls[0], 1)));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        Str s = col_str(ch, 0);
        CHECK(s.offs == (std::vector<uint32_t>{0, 2, 2, 5, 5}));
        CHECK(s.bytes == "abcde");
        CHECK(col_valid(ch, 0) == (U8{1, 0, 1, 1}));
        rwchunk::free_chunk(ch);
    }
    { // identity, rows 2..5: offsets rebased to 0
        Builder b(4, 1);
        CHECK(b.varchar(&offs[2], src.data(), nullptr, from_nulls(&nulls[2], 1)));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        Str s = col_str(ch, 0);
        CHECK(s.offs == (std::vector<uint32_t>{0, 3, 3, 4, 8}));
        CHECK(s.bytes == "cdefghij");
        rwchunk::free_chunk(ch);
    }
    { // slices whose total is 0: the empty string alone, the NULL row alone
        Builder b(1, 2);
        CHECK(b.varchar(&offs[3], src.data(), nullptr, from_nulls(&nulls[3], 1)));
        CHECK(b.varchar(&offs[1], nullptr, nullptr, from_nulls(&nulls[1], 1)));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        for (uint32_t c = 0; c < 2; c++) {
            Str s = col_str(ch, c); // checks bytes != nullptr
            CHECK(s.offs == (std::vector<uint32_t>{0, 0}));
        }
        CHECK(col_valid(ch, 0) == (U8{1}) && col_valid(ch, 1) == (U8{0}));
        rwchunk::free_chunk(ch);
    }
    { // gapped row map: block rows 0, 2, 5 of 6; valid bytes are per OUTPUT row
        std::vector<uint32_t> map = {0, 2, 5};
        U8 out_nulls = {0, 0, 0};
        Builder b(3, 1);
        CHECK(b.varchar(offs.data(), src.data(), map.data(),
                        from_nulls(out_nulls.data(), 1)));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        Str s = col_str(ch, 0);
        CHECK(s.offs == (std::vector<uint32_t>{0, 2, 5, 9}));
        CHECK(s.bytes == "abcdeghij");
        rwchunk::free_chunk(ch);
    }
    { // gapped map over a NULL row and the empty string, from map + 1
        std::vector<uint32_t> map = {4, 0, 1, 3, 2};
        U8 out_nulls = {0, 1, 0, 0};
        Builder b(4, 1);
        CHECK(b.varchar(offs.data(), src.data(), &map[1],
                        from_nulls(out_nulls.data(), 1)));
        b.ops(ops.data());
        RwChunk* ch = b.release();
        Str s = col_str(ch, 0);
        CHECK(s.offs == (std::vector<uint32_t>{0, 2, 2, 2, 5}));
        CHECK(s.bytes == "abcde");
        CHECK(col_valid(ch, 0) == (U8{1, 0, 1, 1}));
        rwchunk::free_chunk(ch);
    }
}

// offsets that claim more than UINT32_MAX bytes with no buffer behind them:
// refused before anything is allocated or copied, and the builder then goes
// out of scope with what it had
static void check_overlong() {
    std::vector<uint64_t> offs = {0, 0x80000000ull, 0x100000000ull};
    U8 nulls = {0, 0};
    I64 vals = {1, 2};
    {
        Builder b(2, 2);
        b.fixed(RW_T_I64, vals.data(), 1, from_nulls(nulls.data(), 1));
        CHECK(!b.varchar(offs.data(), nullptr, nullptr,
                         from_nulls(nulls.data(), 1)));
    }
    {
        std::vector<uint32_t> map = {1, 0};
        Builder b(2, 1);
        CHECK(!b.varchar(offs.data(), nullptr, map.data(),
                         from_nulls(nulls.data(), 1)));
    }
}

// a builder abandoned after each filler in turn
static void check_abandon() {
    I64 vals = {1, 2, 3}, hi = {4, 5, 6};
    U8 nulls = {0, 1, 0}, valid = {1, 1, 0}, ops(3, RW_OP_INSERT), vis = {1, 0, 1};
    std::vector<uint64_t> offs = {0, 1, 1, 3};
    U8 src = {'x', 'y', 'z'};
    int32_t i32[3] = {7, 8, 9};
    for (int stop = 0; stop <= 7; stop++) {
        Builder b(3, 4);
        if (stop == 0) continue;
        b.fixed(RW_T_I64, vals.data(), 1, from_nulls(nulls.data(), 1));
        if (stop == 1) continue;
        b.decimal(vals.data(), hi.data(), 1, from_nulls(nulls.data(), 1));
        if (stop == 2) continue;
        CHECK(b.varchar(offs.data(), src.data(), nullptr,
                        from_nulls(nulls.data(), 1)));
        if (stop == 3) continue;
        b.raw(RW_T_I32, i32, from_valid(valid.data()));
        if (stop == 4) continue;
        b.ops(ops.data());
        if (stop == 5) continue;
        b.vis(vis.data());
        if (stop == 6) continue;
        RwChunk* ch = b.release();
        CHECK(ch->n_cols == 4);
        CHECK(U8(ch->vis, ch->vis + 3) == vis);
        rwchunk::free_chunk(ch);
    }
    rwchunk::free_chunk(nullptr);
    { // zero rows, zero columns
        Builder b(0, 0);
        b.ops(nullptr);
        rwchunk::free_chunk(b.release());
    }
}

// raw-copy columns narrower than a word: 12 and 3 bytes, freed as int64_t[]
static void check_raw() {
    std::unique_ptr<int32_t[]> i32(new int32_t[3]{-1, 2, 0x7fffffff});
    std::unique_ptr<uint8_t[]> bo(new uint8_t[3]{1, 0, 1});
    U8 valid = {1, 2, 0}, ops(3, RW_OP_INSERT);
    Builder b(3, 2);
    b.raw(RW_T_I32, i32.get(), from_valid(valid.data()));
    b.raw(RW_T_BOOL, bo.get(), from_valid(valid.data()));
    b.ops(ops.data());
    RwChunk* ch = b.release();
    CHECK(memcmp(ch->cols[0].data, i32.get(), 12) == 0);
    CHECK(memcmp(ch->cols[1].data, bo.get(), 3) == 0);
    // valid bytes are copied as they are, not normalised
    CHECK(col_valid(ch, 0) == valid && col_valid(ch, 1) == valid);
    rwchunk::free_chunk(ch);
}

// ---- slicer ----
static void check_slices(uint32_t n, uint32_t max, const U8* ops,
                         const std::vector<Range>& expect) {
    auto got = rwchunk::slice_ranges(n, max, ops ? ops->data() : nullptr);
    CHECK(got == expect);
    uint32_t at = 0;
    for (auto [s, take] : got) {
        CHECK(s == at && take > 0);
        CHECK(take <= max || (ops && take == max + 1));
        at += take;
        if (ops && at < n) CHECK((*ops)[at - 1] != RW_OP_UPDATE_DELETE);
    }
    CHECK(at == n);
}

static void check_slicer() {
    const uint8_t I = RW_OP_INSERT, UD = RW_OP_UPDATE_DELETE,
                  UI = RW_OP_UPDATE_INSERT;
    U8 a = {I, I, UD, UI, I, I, I};
    check_slices(7, 3, &a, {{0, 4}, {4, 3}});
    // U- as the very last row of the output: nothing past n_out
    U8 b = {I, I, I, I, I, UD};
    check_slices(6, 3, &b, {{0, 3}, {3, 3}});
    U8 b2 = {I, I, UD};
    check_slices(3, 3, &b2, {{0, 3}});
    // max = 1 with a pair at rows 0-1 (HashAgg's unclamped chunk_size 1)
    U8 c = {UD, UI, I};
    check_slices(3, 1, &c, {{0, 2}, {2, 1}});
    // the same ops with none passed: the pair is split (the join)
    check_slices(3, 1, nullptr, {{0, 1}, {1, 1}, {2, 1}});
    check_slices(7, 3, nullptr, {{0, 3}, {3, 3}, {6, 1}});
    // n_out a multiple of max
    U8 d(6, I);
    check_slices(6, 2, &d, {{0, 2}, {2, 2}, {4, 2}});
    check_slices(6, 6, &d, {{0, 6}});
    // back-to-back pairs: every range takes its U+ and the next starts clean
    U8 e = {I, UD, UI, UD, UI, UD, UI};
    check_slices(7, 2, &e, {{0, 3}, {3, 2}, {5, 2}});
    // nothing to cut
    check_slices(0, 3, &d, {});
    check_slices(0, 3, nullptr, {});
}

// ---- queue ----
static RwChunk* tiny_chunk(int64_t tag) {
    uint8_t null = 0, op = RW_OP_INSERT;
    Builder b(1, 1);
    b.fixed(RW_T_I64, &tag, 1, from_nulls(&null, 1));
    b.ops(&op);
    return b.release();
}
static int64_t tag_of(const RwChunk* ch) {
    return ((const int64_t*)ch->cols[0].data)[0];
}

static void check_queue() {
    rwchunk::ChunkQueue q;
    CHECK(q.poll() == nullptr);
    for (int64_t t = 1; t <= 3; t++) q.push(tiny_chunk(t));
    for (int64_t t = 1; t <= 3; t++) {
        RwChunk* ch = q.poll();
        CHECK(ch && tag_of(ch) == t);
        rwchunk::free_chunk(ch);
    }
    CHECK(q.poll() == nullptr);
    // two chunks left behind: the destructor frees both (LeakSanitizer)
    q.push(tiny_chunk(4));
    q.push(tiny_chunk(5));
}

// ---- column check ----
static void check_column_check() {
    using rwvarlen::check_column;
    U8 valid = {1, 1};
    U8 bytes = {'a', 'b', 'c'};
    auto col = [&](const RwVarlenData* vd) {
        return RwColumn{RW_T_VARCHAR, valid.data(), vd};
    };
    CHECK(check_column(col(nullptr), 2) != nullptr);
    std::vector<uint32_t> good = {0, 1, 3};
    RwVarlenData ok{good.data(), bytes.data()};
    CHECK(check_column(col(&ok), 2) == nullptr);
    RwVarlenData no_offs{nullptr, bytes.data()};
    CHECK(check_column(col(&no_offs), 2) != nullptr);
    std::vector<uint32_t> first = {1, 2, 3};
    RwVarlenData bad_first{first.data(), bytes.data()};
    CHECK(check_column(col(&bad_first), 2) != nullptr);
    std::vector<uint32_t> dec = {0, 2, 1};
    RwVarlenData bad_dec{dec.data(), bytes.data()};
    CHECK(check_column(col(&bad_dec), 2) != nullptr);
    std::vector<uint32_t> lng = {0, rwvarlen::MAX_LEN + 1};
    RwVarlenData bad_len{lng.data(), bytes.data()};
    CHECK(check_column(col(&bad_len), 1) != nullptr);
    RwVarlenData no_bytes{good.data(), nullptr};
    const char* why = check_column(col(&no_bytes), 2);
    CHECK(why && std::string(why).find("bytes") != std::string::npos);
    std::vector<uint32_t> zeros = {0, 0, 0};
    RwVarlenData empty{zeros.data(), nullptr};
    CHECK(check_column(col(&empty), 2) == nullptr);
    // n = 0: one offset, which must still be 0
    std::vector<uint32_t> one = {0}, one_bad = {5};
    RwVarlenData z{one.data(), nullptr}, zb{one_bad.data(), nullptr};
    CHECK(check_column(col(&z), 0) == nullptr);
    CHECK(check_column(col(&zb), 0) != nullptr);
}

// ---- reference words ----
static void check_ref_words() {
    using namespace rwvarlen;
    std::vector<uint32_t> offs = {0, 2, 2, 5, 5};
    RwVarlenData vd{offs.data(), nullptr}; // the loop never reads bytes
    U8 valid = {1, 0, 1, 1}; // row 1 NULL, row 3 a valid empty string
    std::vector<int64_t> w(9, -1);
    ref_words(&vd, valid.data(), 4, 100, 0, w);
    CHECK(w == (I64{(int64_t)pack(100, 2), 0, (int64_t)pack(102, 3),
                    (int64_t)pack(105, 0)}));
    CHECK(word_off((uint64_t)w[2]) == 102 && word_len((uint64_t)w[2]) == 3);
    CHECK(w[3] == 105); // empty string: nonzero only through base
    ref_words(&vd, valid.data(), 4, 100, PROV_BIT, w);
    CHECK(w == (I64{(int64_t)pack(PROV_BIT | 100, 2), 0,
                    (int64_t)pack(PROV_BIT | 102, 3),
                    (int64_t)pack(PROV_BIT | 105, 0)}));
    ref_words(&vd, valid.data(), 4, 0, 0, w);
    CHECK(w[0] == (int64_t)pack(0, 2) && w[1] == 0 && w[3] == 5);
    std::vector<uint32_t> z = {0, 0};
    RwVarlenData e{z.data(), nullptr};
    U8 v1 = {1};
    ref_words(&e, v1.data(), 1, 0, 0, w);
    CHECK(w == (I64{0})); // empty string at base 0 without a flag: word 0
    ref_words(&e, v1.data(), 1, 0, PROV_BIT, w);
    CHECK(w == (I64{(int64_t)PROV_BIT}));
    ref_words(&e, v1.data(), 0, 0, 0, w);
    CHECK(w.empty());
}

int main() {
    check_fixed();
    check_varchar();
    check_overlong();
    check_abandon();
    check_raw();
    check_slicer();
    check_queue();
    check_column_check();
    check_ref_words();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("chunk build host check ok\n");
    return 0;
}
