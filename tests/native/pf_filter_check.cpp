// pf_filter_check.cpp — host-only check of the row filter's planner and comparisons (no GPU, no HIP):
//   plan_filter (csrc/pf_plan.cpp) over every call error of pf_decode_row_group_filter, with bounds of 0, 1, 4095,
//   4096 and 4097 bytes, and the packed table's offsets;
//   the comparisons of csrc/pf_pred.h, the text the kernel compiles, on a fixed list of pairs.
// Built by tests/test_row_filter_cpu.py with g++ under AddressSanitizer + UBSan. Prints "checks N failures F".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pf_plan.h"
#include "pf_pred.h"

using namespace pf;

static int g_checks = 0, g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        g_checks++;                                                        \
        if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static pf_chunk_desc chunk(int ptype, int max_def, int max_rep, int type_length = 0) {
    pf_chunk_desc c{};
    c.physical_type = ptype;
    c.type_length = type_length;
    c.max_def = max_def;
    c.max_rep = max_rep;
    return c;
}

static pf_predicate pred(int chunk, int op, const uint8_t* lo, int lo_len, const uint8_t* hi, int hi_len) {
    pf_predicate p{};
    p.chunk = chunk; p.op = op; p.lo = lo; p.lo_len = lo_len; p.hi = hi; p.hi_len = hi_len;
    return p;
}

static int plan(const std::vector<pf_chunk_desc>& cds, const std::vector<pf_predicate>& ps, FilterPlan& f, int n_preds = -100) {
    const char* why = nullptr;
    const int n = n_preds == -100 ? int(ps.size()) : n_preds;
    const int rc = plan_filter(cds.data(), int(cds.size()), ps.empty() ? nullptr : ps.data(), n, f, &why);
    CHECK(why != nullptr);
    if (rc != PF_OK) CHECK(f.preds.empty() && f.blob.empty() && why[0] != 0);
    return rc;
}

static void check_plan() {
    // chunks: 0 BOOLEAN, 1 INT32, 2 INT64, 3 INT96, 4 FLOAT, 5 DOUBLE, 6 BYTE_ARRAY, 7 FLBA(5), 8 nested INT32, 9 nested BYTE_ARRAY
    std::vector<pf_chunk_desc> cds;
    for (int t = 0; t < 8; t++) cds.push_back(chunk(t, t & 1, 0, t == PF_FIXED_LEN_BYTE_ARRAY ? 5 : 0));
    cds.push_back(chunk(PF_INT32, 3, 1));
    cds.push_back(chunk(PF_BYTE_ARRAY, 3, 1));
    std::vector<uint8_t> buf(4097, 0x61);
    buf[0] = 1;
    const uint8_t* b = buf.data();
    FilterPlan f;

    // n_preds
    CHECK(plan(cds, {}, f, 0) == PF_OK && f.preds.empty());
    CHECK(plan(cds, {}, f, -1) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {}, f, 1) == PF_ERR_INVALID_ARG);   // NULL preds with n_preds > 0
    {
        std::vector<pf_predicate> many(PF_MAX_PREDICATES + 1, pred(1, PF_PRED_NOT_NULL, nullptr, 0, nullptr, 0));
        CHECK(plan(cds, many, f) == PF_ERR_INVALID_ARG);
        many.pop_back();
        CHECK(plan(cds, many, f) == PF_OK && int(f.preds.size()) == PF_MAX_PREDICATES);
    }
    // chunk index, op
    CHECK(plan(cds, {pred(-1, PF_PRED_NOT_NULL, nullptr, 0, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {pred(int(cds.size()), PF_PRED_NOT_NULL, nullptr, 0, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {pred(1, 3, nullptr, 0, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {pred(1, -1, nullptr, 0, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    // a bound on IS_NULL / NOT_NULL
    CHECK(plan(cds, {pred(1, PF_PRED_IS_NULL, b, 4, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {pred(1, PF_PRED_NOT_NULL, nullptr, 0, b, 4)}, f) == PF_ERR_INVALID_ARG);
    // repetition; ranges over INT96 / FLBA; IS_NULL / NOT_NULL take any flat type
    CHECK(plan(cds, {pred(8, PF_PRED_NOT_NULL, nullptr, 0, nullptr, 0)}, f) == PF_ERR_UNSUPPORTED_TYPE);
    CHECK(plan(cds, {pred(9, PF_PRED_RANGE, b, 1, nullptr, 0)}, f) == PF_ERR_UNSUPPORTED_TYPE);
    CHECK(plan(cds, {pred(3, PF_PRED_RANGE, b, 12, nullptr, 0)}, f) == PF_ERR_UNSUPPORTED_TYPE);
    CHECK(plan(cds, {pred(7, PF_PRED_RANGE, b, 5, nullptr, 0)}, f) == PF_ERR_UNSUPPORTED_TYPE);
    CHECK(plan(cds, {pred(3, PF_PRED_RANGE, nullptr, 0, nullptr, 0)}, f) == PF_ERR_UNSUPPORTED_TYPE);
    for (int t = 0; t < 8; t++) {
        CHECK(plan(cds, {pred(t, PF_PRED_IS_NULL, nullptr, 0, nullptr, 0), pred(t, PF_PRED_NOT_NULL, nullptr, 0, nullptr, 0)}, f) == PF_OK);
        CHECK(f.preds.size() == 2 && f.preds[0].chunk == t && f.preds[0].ptype == t && f.preds[1].op == PF_PRED_NOT_NULL);
    }
    // bound lengths: every fixed-width type takes its width alone; BYTE_ARRAY up to 4096
    const int lens[] = {0, 1, 4, 8, 4095, 4096, 4097};
    const int fixed[][2] = {{PF_BOOLEAN, 1}, {PF_INT32, 4}, {PF_INT64, 8}, {PF_FLOAT, 4}, {PF_DOUBLE, 8}};
    for (const auto& tw : fixed)
        for (int n : lens)
            for (int side = 0; side < 2; side++) {
                const pf_predicate p = side ? pred(tw[0], PF_PRED_RANGE, nullptr, 0, b, n) : pred(tw[0], PF_PRED_RANGE, b, n, nullptr, 0);
                const int rc = plan(cds, {p}, f);
                CHECK(rc == (n == tw[1] ? PF_OK : PF_ERR_INVALID_ARG));
                if (rc == PF_OK) CHECK(f.preds.size() == 1 && f.preds[0].flags == (side ? PRED_HAS_HI : PRED_HAS_LO) && f.blob.empty());
            }
    CHECK(plan(cds, {pred(PF_INT32, PF_PRED_RANGE, b, -4, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    for (int n : lens) {
        const int rc = plan(cds, {pred(PF_BYTE_ARRAY, PF_PRED_RANGE, b, n, b + 1, n > 0 ? n - 1 : 0)}, f);
        CHECK(rc == (n <= 4096 ? PF_OK : PF_ERR_INVALID_ARG));
        if (rc == PF_OK) {
            const DevPred& d = f.preds[0];
            CHECK(d.flags == (PRED_HAS_LO | PRED_HAS_HI) && int(d.lo_len) == n && int(d.hi_len) == (n > 0 ? n - 1 : 0));
            CHECK(size_t(d.lo_off) + d.lo_len <= f.blob.size() && size_t(d.hi_off) + d.hi_len <= f.blob.size());
            CHECK(f.blob.size() == size_t(d.lo_len) + d.hi_len);
            if (d.lo_len) CHECK(std::memcmp(f.blob.data() + d.lo_off, b, d.lo_len) == 0);
            if (d.hi_len) CHECK(std::memcmp(f.blob.data() + d.hi_off, b + 1, d.hi_len) == 0);
        }
    }
    CHECK(plan(cds, {pred(PF_BYTE_ARRAY, PF_PRED_RANGE, nullptr, 0, b, 4097)}, f) == PF_ERR_INVALID_ARG);
    CHECK(plan(cds, {pred(PF_BYTE_ARRAY, PF_PRED_RANGE, b, -1, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
    // BOOLEAN bounds are 0 or 1
    {
        const uint8_t two = 2, one = 1, zero = 0;
        CHECK(plan(cds, {pred(PF_BOOLEAN, PF_PRED_RANGE, &two, 1, nullptr, 0)}, f) == PF_ERR_INVALID_ARG);
        CHECK(plan(cds, {pred(PF_BOOLEAN, PF_PRED_RANGE, &zero, 1, &one, 1)}, f) == PF_OK && f.preds[0].lo_i == 0 && f.preds[0].hi_i == 1);
    }
    // PF_MAX_PREDICATES BYTE_ARRAY predicates with both bounds at 4096: every offset stays inside the blob
    {
        std::vector<pf_predicate> ps(PF_MAX_PREDICATES, pred(PF_BYTE_ARRAY, PF_PRED_RANGE, b, 4096, b + 1, 4096));
        CHECK(plan(cds, ps, f) == PF_OK && f.blob.size() == size_t(PF_MAX_PREDICATES) * 8192);
        size_t at = 0;
        for (const DevPred& d : f.preds) {
            CHECK(d.lo_off == at && d.hi_off == at + 4096 && size_t(d.hi_off) + d.hi_len <= f.blob.size());
            at += 8192;
        }
    }
    // the values of fixed-width bounds: little-endian, sign-extended, FLOAT widened exactly
    {
        const int32_t i32 = std::numeric_limits<int32_t>::min();
        const int64_t i64 = std::numeric_limits<int64_t>::max();
        const float f32 = -0.1f;
        const double f64 = -std::numeric_limits<double>::infinity();
        uint8_t a[4], c[8], d[4], e[8];
        std::memcpy(a, &i32, 4); std::memcpy(c, &i64, 8); std::memcpy(d, &f32, 4); std::memcpy(e, &f64, 8);
        CHECK(plan(cds, {pred(PF_INT32, PF_PRED_RANGE, a, 4, a, 4), pred(PF_INT64, PF_PRED_RANGE, nullptr, 0, c, 8),
                         pred(PF_FLOAT, PF_PRED_RANGE, d, 4, nullptr, 0), pred(PF_DOUBLE, PF_PRED_RANGE, e, 8, e, 8)}, f) == PF_OK);
        CHECK(f.preds[0].lo_i == i32 && f.preds[0].hi_i == i32 && f.preds[1].hi_i == i64 && f.preds[1].flags == PRED_HAS_HI);
        CHECK(f.preds[2].lo_f == double(f32) && f.preds[3].lo_f == f64 && f.preds[3].hi_f == f64);
    }
}

static int sgn(int x) { return (x > 0) - (x < 0); }
static int cmp(const std::string& a, const std::string& b) {
    return sgn(pred_cmp_bytes(reinterpret_cast<const uint8_t*>(a.data()), uint32_t(a.size()), reinterpret_cast<const uint8_t*>(b.data()),
                              uint32_t(b.size())));
}

static void check_compare() {
    using S = std::string;
    // (a, b, sign of a ? b): prefix first, bytes unsigned, 0x00 and 0xFF, the empty string
    const struct { S a, b; int want; } pairs[] = {
        {S(""), S(""), 0}, {S(""), S("a"), -1}, {S(""), S("\0", 1), -1}, {S("a"), S("a"), 0}, {S("a"), S("a\0", 2), -1},
        {S("a\0", 2), S("a\0\0", 3), -1}, {S("a"), S("b"), -1}, {S("ab"), S("b"), -1}, {S("a\xff"), S("b"), -1},
        {S("\x7f"), S("\x80"), -1}, {S("\xff"), S("\x01"), 1}, {S("\xff\xff"), S("\xff"), 1}, {S("\xff"), S("\xff\0", 2), -1},
        {S("\0", 1), S("\xff"), -1}, {S("abc"), S("abd"), -1}, {S("abc"), S("ab"), 1}, {S(300, 'x'), S(299, 'x') + "y", -1},
    };
    for (const auto& p : pairs) {
        CHECK(cmp(p.a, p.b) == p.want);
        CHECK(cmp(p.b, p.a) == -p.want);
    }
    const uint8_t* e = nullptr;
    CHECK(pred_cmp_bytes(e, 0, e, 0) == 0);
    auto in = [](const S& v, const S* lo, const S* hi) {
        auto u = [](const S& s) { return reinterpret_cast<const uint8_t*>(s.data()); };
        return pred_range_bytes(u(v), uint32_t(v.size()), lo != nullptr, lo ? u(*lo) : nullptr, lo ? uint32_t(lo->size()) : 0, hi != nullptr,
                                hi ? u(*hi) : nullptr, hi ? uint32_t(hi->size()) : 0);
    };
    const S a("a"), a0("a\0", 2), b("b"), empty;
    CHECK(in(a, &a, &a) && !in(a0, &a, &a) && in(a0, &a, &b) && !in(empty, &a, nullptr) && in(empty, nullptr, &a) && in(empty, &empty, &empty));
    CHECK(in(b, nullptr, nullptr) && !in(b, nullptr, &a0));
    // integers
    const int64_t mn = std::numeric_limits<int64_t>::min(), mx = std::numeric_limits<int64_t>::max();
    CHECK(pred_range_int(mn, true, mn, true, mn) && pred_range_int(mx, true, mx, true, mx));
    CHECK(!pred_range_int(mn, true, mn + 1, false, 0) && !pred_range_int(mx, false, 0, true, mx - 1));
    CHECK(pred_range_int(0, true, mn, true, mx) && pred_range_int(-1, false, 0, true, 0) && !pred_range_int(1, false, 0, true, 0));
    CHECK(pred_range_int(5, false, 0, false, 0) && !pred_range_int(5, true, 6, true, 4) && pred_range_int(-5, true, -5, true, -5));
    // reals: NaN, signed zeros, infinities
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    CHECK(!pred_range_real(nan, true, -inf, true, inf) && !pred_range_real(nan, true, -inf, false, 0) && !pred_range_real(nan, false, 0, true, inf));
    CHECK(pred_range_real(nan, false, 0, false, 0));   // both bounds missing: every present row
    CHECK(!pred_range_real(1.0, true, nan, false, 0) && !pred_range_real(1.0, false, 0, true, nan) && !pred_range_real(nan, true, nan, true, nan));
    CHECK(pred_range_real(-0.0, true, 0.0, true, 0.0) && pred_range_real(0.0, true, -0.0, true, -0.0));
    CHECK(pred_range_real(inf, true, inf, true, inf) && pred_range_real(-inf, true, -inf, true, -inf) && !pred_range_real(inf, false, 0, true, 1e308));
    CHECK(pred_range_real(-inf, false, 0, true, -1e308) && pred_range_real(1.5, true, -inf, true, inf));
    CHECK(pred_range_real(double(0.1f), true, double(0.1f), true, double(0.1f)) && !pred_range_real(double(0.1f), false, 0, true, 0.1));
}

int main() {
    check_plan();
    check_compare();
    std::printf("checks %d failures %d\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
