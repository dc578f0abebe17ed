// Invariant checks of the write path's host planner (csrc/pf_enc_plan.cpp) without a GPU: every call error
// with its code and text, and over one grid of columns the page plan, the delta / statistics / page-index
// tables, the arena layout and binding, the sections of every route at sizes from 0 to the reserved worst
// case, the compression layout, and the assembled chunk read back by pf_meta.cpp's page walk with its CRCs
// recomputed bytewise. The planner never reads values or chars, so those are made-up addresses.
// Built with -fsanitize=address,undefined by tests/test_enc_plan_cpu.py.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pf_crc.h"
#include "pf_enc_plan.h"
#include "pf_host.h"
#include "pfloor.h"

using namespace pf;

namespace {

int g_failures = 0;
long g_checks = 0, g_cases = 0;
std::string g_case;

void check(bool ok, const char* fmt, ...) {
    g_checks++;
    if (ok) return;
    if (++g_failures > 40) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "FAIL [%s] %s\n", g_case.c_str(), buf);
}

uint8_t* const ARENA = reinterpret_cast<uint8_t*>(0x7f0000000000ull);    // made-up device addresses
uint8_t* const SEC = reinterpret_cast<uint8_t*>(0x7e0000000000ull);
uint8_t* const OUT = reinterpret_cast<uint8_t*>(0x7d0000000000ull);
uint8_t* const CALLER = reinterpret_cast<uint8_t*>(0x7c0000000000ull);   // the caller's arrays (never read)
template <class T> uint64_t addr(T* q) { return reinterpret_cast<uintptr_t>(q); }
int width_of(int pt) { return pt == PF_BYTE_ARRAY ? 0 : pt == PF_BOOLEAN ? 1 : (pt == PF_INT32 || pt == PF_FLOAT) ? 4 : 8; }
uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; return x ^ (x >> 33); }

// ---------------------------------------------------------------- inputs
struct Input {
    std::vector<uint8_t> hval;
    std::vector<int32_t> hoff;
    pf_encode_column col{};
};

// def_mode 0: REQUIRED; 1: OPTIONAL with validity; 2: OPTIONAL, validity NULL. Validity: page 0 all present, page 1 all
// null (next to each other), then mixed; strings: lengths 0..4, so many are empty.
Input make_input(int pt, int def_mode, int64_t n, int page_rows) {
    Input in;
    pf_encode_column& c = in.col;
    c.physical_type = pt;
    c.max_def = def_mode ? 1 : 0;
    c.num_rows = n;
    c.page_rows = page_rows;
    const int64_t eff = ((page_rows > 0 ? page_rows : 20000) + 7) / 8 * 8;
    if (def_mode == 1) {
        in.hval.assign(size_t((n + 7) / 8) + 1, 0);   // (+1: never a null data pointer)
        for (int64_t r = 0; r < n; r++) {
            const int64_t pg = r / eff;
            const bool on = pg % 4 == 0 ? true : pg % 4 == 1 ? false : (mix(uint64_t(r)) & 3) != 0;
            if (on) in.hval[size_t(r >> 3)] |= uint8_t(1u << (r & 7));
        }
        in.hval.resize(size_t((n + 7) / 8));
        c.validity = in.hval.empty() ? CALLER : in.hval.data();
    }
    if (pt == PF_BYTE_ARRAY) {
        in.hoff.assign(size_t(n) + 1, 0);
        for (int64_t r = 0; r < n; r++) {
            const bool on = def_mode != 1 || ((in.hval[size_t(r >> 3)] >> (r & 7)) & 1);
            in.hoff[size_t(r) + 1] = in.hoff[size_t(r)] + (on ? int32_t(mix(uint64_t(r) + 77) % 5) : 0);
        }
        c.offsets = in.hoff.data();
        c.chars = CALLER + 4096;
        c.chars_len = in.hoff[size_t(n)];
    } else {
        c.values = CALLER;
    }
    c.codec = PF_CODEC_SNAPPY;
    return in;
}

// ---------------------------------------------------------------- rejections
// (the texts are the parent commit's pf_encode_chunk messages)
void expect_reject(const char* what, const Input& in, int code, const char* text) {
    g_case = std::string("reject ") + what;
    EncPlan p;
    const char* why = "";
    const int rc = plan_encode(&in.col, in.hval, in.hoff, p, &why);
    check(rc == code, "code %d, expected %d", rc, code);
    check(std::strcmp(why, text) == 0, "text '%s', expected '%s'", why, text);
    check(p.pp.empty() && p.n == 0 && p.m == 0 && p.dstreams.empty() && p.stiles.empty() && p.px_in.empty() && p.a_sz == 0,
          "a failed plan is not empty");
}
void expect_accept(const char* what, const Input& in, EncPlan& p) {
    g_case = std::string("accept ") + what;
    const char* why = "";
    const int rc = plan_encode(&in.col, in.hval, in.hoff, p, &why);
    check(rc == PF_OK, "code %d '%s'", rc, why);
}

void check_rejections() {
    const char* BLOOM = "encode: bloom_bytes must be a power of two in [32, 128 MiB]";
    const char* TRUNC = "encode: index_truncate must be 0, -1 or in [1, 2047]";
    const char* MISSING = "encode: missing input arrays";
    const char* OFFS = "encode: offsets out of order or outside chars";
    const char* SHAPE = "encode: bad shape";
    EncPlan p;
    Input in = make_input(PF_INT32, 0, 16, 0);
    for (int pt : {int(PF_INT96), int(PF_FIXED_LEN_BYTE_ARRAY), 8, -1}) {
        Input x = in; x.col.physical_type = pt;
        expect_reject("type", x, PF_ERR_UNSUPPORTED_TYPE, "encode: unsupported physical type");
    }
    { Input x = in; x.col.num_rows = -1; expect_reject("n < 0", x, PF_ERR_INVALID_ARG, SHAPE); }
    { Input x = in; x.col.num_rows = 0x7ffffff1ll; expect_reject("n large", x, PF_ERR_INVALID_ARG, SHAPE); }
    { Input x = in; x.col.max_def = 2; expect_reject("max_def 2", x, PF_ERR_INVALID_ARG, SHAPE); }
    for (int codec : {2, 3, 4, 5, 7, -1}) {
        Input x = in; x.col.codec = codec;
        expect_reject("codec", x, PF_ERR_UNSUPPORTED_CODEC, "encode: codec must be SNAPPY, ZSTD or UNCOMPRESSED");
    }
    for (int b : {-1, 31, 48, 256 << 20}) {
        Input x = in; x.col.bloom_bytes = b;
        expect_reject("bloom_bytes", x, PF_ERR_INVALID_ARG, BLOOM);
    }
    { Input x = make_input(PF_BOOLEAN, 0, 16, 0); x.col.bloom_bytes = 64; expect_accept("BOOLEAN bloom", x, p); check(p.bloom == 0, "BOOLEAN plans a filter"); }
    { Input x = in; x.col.bloom_bytes = 64; expect_accept("INT32 bloom", x, p); check(p.bloom == 64, "bloom %zu", p.bloom); }
    { Input x = make_input(PF_BOOLEAN, 0, 16, 0); x.col.bloom_bytes = 48; expect_reject("BOOLEAN bad bloom", x, PF_ERR_INVALID_ARG, BLOOM); }
    Input s = make_input(PF_BYTE_ARRAY, 0, 16, 0);
    for (int t : {-2, 2048}) {
        Input x = s; x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = t;
        expect_reject("index_truncate", x, PF_ERR_INVALID_ARG, TRUNC);
        x.col.dictionary = 0;
        expect_accept("index_truncate without the bit", x, p);
    }
    { Input x = in; x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = 5; expect_accept("index_truncate INT32", x, p); }
    { Input x = in; x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = 4000; expect_accept("index_truncate INT32 4000", x, p); }
    { Input x = s; x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = 2047; expect_accept("index_truncate 2047", x, p); check(p.px_trunc == 2047, "trunc"); }
    { Input x = s; x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = -1; expect_accept("index_truncate -1", x, p); check(p.px_trunc == PX_NO_TRUNC, "trunc"); }
    { Input x = in; x.col.values = nullptr; expect_reject("values", x, PF_ERR_INVALID_ARG, MISSING); }
    { Input x = s; x.col.offsets = nullptr; expect_reject("offsets", x, PF_ERR_INVALID_ARG, MISSING); }
    { Input x = s; x.col.chars = nullptr; expect_reject("chars", x, PF_ERR_INVALID_ARG, MISSING); }
    { Input x = s; x.col.chars_len = -1; expect_reject("chars_len < 0", x, PF_ERR_INVALID_ARG, MISSING); }
    { Input x = s; x.col.chars_len = 0x80000000ll; expect_reject("chars_len large", x, PF_ERR_INVALID_ARG, MISSING); }
    { Input x = in; x.col.num_rows = 0; x.col.values = nullptr; expect_accept("no rows, no arrays", x, p); }
    { Input x = s; x.hoff[5] = x.hoff[4] - 1; x.col.offsets = x.hoff.data(); expect_reject("offsets decrease", x, PF_ERR_INVALID_ARG, OFFS); }
    { Input x = s; for (auto& o : x.hoff) o -= 1; x.col.offsets = x.hoff.data(); expect_reject("offsets negative", x, PF_ERR_INVALID_ARG, OFFS); }
    { Input x = s; x.col.offsets = x.hoff.data(); x.col.chars_len -= 1; expect_reject("offsets past chars", x, PF_ERR_INVALID_ARG, OFFS); }
    {   // page index values over 1 GiB: 2 x 2048 bytes for each of more than 2^18 pages
        Input x = make_input(PF_BYTE_ARRAY, 0, 8 * ((1 << 18) + 1), 8);
        x.col.dictionary = PF_ENCODE_PAGE_INDEX; x.col.index_truncate = -1;
        expect_reject("page index 1 GiB", x, PF_ERR_INVALID_ARG, "encode: page index values over 1 GiB (fewer pages or a shorter index_truncate)");
        x.col.index_truncate = 0;
        expect_accept("page index, 64-byte entries", x, p);
    }
    {   // a DELTA_BYTE_ARRAY page over 2 GiB: two rows, the lengths alone say so
        Input x = make_input(PF_BYTE_ARRAY, 0, 2, 0);
        x.hoff = {0, 0x40000000, 0x7fffffff};
        x.col.offsets = x.hoff.data(); x.col.chars_len = 0x7fffffff;
        x.col.dictionary = PF_ENCODE_DELTA_FALLBACK;
        expect_reject("delta page 2 GiB", x, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
        x.col.dictionary = 0;
        expect_accept("PLAIN page of 2 GiB", x, p);
    }
}

// ---------------------------------------------------------------- page plan, tables
void check_page_plan(const EncPlan& p, const Input& in) {
    const int64_t n = p.n;
    check(!p.pp.empty() && p.pp.front().r0 == 0 && p.pp.back().r1 == n, "pages do not span [0, n)");
    if (n == 0) check(p.pp.size() == 1 && p.pp[0].cnt == 0, "n == 0: not one empty page");
    uint64_t pop = 0;
    if (p.has_val) for (int64_t r = 0; r < n; r++) pop += (in.hval[size_t(r >> 3)] >> (r & 7)) & 1;
    else pop = uint64_t(n);
    uint32_t d0 = 0;
    for (size_t i = 0; i < p.pp.size(); i++) {
        const EncPagePlan& g = p.pp[i];
        if (i) check(g.r0 == p.pp[i - 1].r1, "page %zu does not start where %zu ends", i, i - 1);
        check(n == 0 || g.r1 > g.r0, "page %zu is empty", i);
        check(g.r1 - g.r0 <= p.page_rows && g.r0 % 8 == 0, "page %zu: rows %lld at %lld", i, (long long)(g.r1 - g.r0), (long long)g.r0);
        check(g.d0 == d0, "page %zu: d0 %u, prefix sum %u", i, g.d0, d0);
        uint32_t cnt = 0;
        uint64_t plain = 0;
        for (int64_t r = g.r0; r < g.r1; r++)
            if (!p.has_val || ((in.hval[size_t(r >> 3)] >> (r & 7)) & 1)) {
                cnt++;
                if (p.str) plain += 4 + uint64_t(in.hoff[size_t(r) + 1] - in.hoff[size_t(r)]);
            }
        if (!p.str) plain = p.pt == PF_BOOLEAN ? (cnt + 7) / 8 : uint64_t(cnt) * uint64_t(width_of(p.pt));
        check(g.cnt == cnt && g.plain == plain, "page %zu: cnt %u plain %llu, recomputed %u %llu", i, g.cnt, (unsigned long long)g.plain, cnt,
              (unsigned long long)plain);
        d0 += g.cnt;
    }
    check(d0 == p.m && p.m == pop, "sum cnt %u, m %u, popcount %llu", d0, p.m, (unsigned long long)pop);
    check(p.page_rows % 8 == 0, "page_rows %lld", (long long)p.page_rows);
}

void check_tables(const EncPlan& p) {
    const size_t np = p.pp.size();
    const bool delta_ok = (p.bits & PF_ENCODE_DELTA_FALLBACK) && (p.pt == PF_INT32 || p.pt == PF_INT64 || p.str);
    check(p.delta_bit == delta_ok, "delta_bit %d", int(p.delta_bit));
    if (p.delta_bit) {
        const uint32_t ns = p.str ? 2 : 1;
        check(p.dpages.size() == np && p.dstreams.size() == ns * np + 1, "delta: %zu pages, %zu streams", p.dpages.size(), p.dstreams.size());
        uint32_t item = 0;
        for (size_t s = 0; s + 1 < p.dstreams.size(); s++) {
            const DeltaStream& d = p.dstreams[s];
            const EncPagePlan& g = p.pp[s / ns];
            check(d.page == s / ns && d.cnt == g.cnt && d.item0 == item && d.ew == uint32_t(p.str ? 4 : p.w), "delta stream %zu", s);
            item += 1 + (g.cnt <= 1 ? 0 : (g.cnt - 1 + 127) / 128);
        }
        check(p.dstreams.back().item0 == item && p.n_items == item, "delta: sentinel %u, n_items %u, counted %u", p.dstreams.back().item0, p.n_items, item);
        for (size_t i = 0; i < p.dpages.size(); i++)
            check(p.dpages[i].s0 == ns * i && p.dpages[i].ns == ns && p.dpages[i].d0 == p.pp[i].d0 && p.dpages[i].cnt == p.pp[i].cnt, "delta page %zu", i);
    } else {
        check(p.dpages.empty() && p.dstreams.empty() && p.n_items == 0, "delta tables without the bit");
    }
    if (p.run_stats) {
        check(p.sptile.size() == np + 1 && p.sptile.back() == p.stiles.size() && p.n_se == np + 1, "ptile: %zu entries, last %u of %zu tiles", p.sptile.size(),
              p.sptile.empty() ? 0u : p.sptile.back(), p.stiles.size());
        for (size_t i = 0; i < np; i++) {
            check(p.sptile[i] <= p.sptile[i + 1], "ptile not monotone at %zu", i);
            uint32_t at = p.pp[i].d0;
            for (uint32_t t = p.sptile[i]; t < p.sptile[i + 1]; t++) {
                const StatTile& s = p.stiles[t];
                check(s.page == i && s.d0 == at && s.cnt > 0 && s.cnt <= ST_TILE && (s.cnt == ST_TILE || t + 1 == p.sptile[i + 1]), "tile %u of page %zu", t, i);
                at += s.cnt;
            }
            check(at == p.pp[i].d0 + p.pp[i].cnt, "page %zu: tiles end at %u", i, at);
        }
    } else {
        check(p.stiles.empty() && p.sptile.empty() && p.n_se == 0, "statistics tables without a bit");
    }
    if (p.want_index) {
        check(p.n_px == np && p.px_nc == sizeof(PgIndexHead) && p.px_nc + 8 * np <= p.px_off && p.px_off + 4 * (2 * np + 1) <= p.px_np &&
                  p.px_np + np <= p.px_val && p.px_val + p.px_cap == p.px_bytes, "page index sub-offsets");
        check(p.px_nc % 8 == 0 && p.px_off % 4 == 0, "page index alignment");
        check(p.px_in.size() == 2 * np, "px_in");
        for (size_t i = 0; i < np && p.px_in.size() == 2 * np; i++)
            check(p.px_in[i] == uint32_t(p.pp[i].r1 - p.pp[i].r0) && p.px_in[np + i] == p.pp[i].cnt, "px_in of page %zu", i);
    } else {
        check(p.n_px == 0 && p.px_bytes == 0 && p.px_in.empty(), "page index tables without the bit");
    }
    check(p.scan_elems == std::max(size_t(p.n) + 1, p.delta_bit ? size_t(p.n_items) + 1 : size_t(0)), "scan_elems %zu", p.scan_elems);
}

// ---------------------------------------------------------------- arena
bool region_used(const EncPlan& p, int r) {
    const bool ds = p.delta_bit && p.str;
    switch (r) {
    case R_IN: return !p.str && p.n > 0;
    case R_VL: return p.vbytes > 0;
    case R_OF: case R_DSRC: case R_DLEN: case R_VSZ: case R_VPRE: return p.str;
    case R_CH: return p.str && p.chars_len > 0;
    case R_DENSE: return !p.str && p.n > 0;
    case R_PFX: case R_SFX: case R_SPRE: return ds;
    case R_DSTR: case R_DPG: case R_DBY: case R_DOF: case R_DMIN: case R_DWD: case R_DTOT: return p.delta_bit;
    case R_HSTR: case R_HBY: return p.hyb;
    case R_STT: case R_SPART: return p.run_stats && !p.stiles.empty();
    case R_STP: case R_SOUT: return p.run_stats;
    case R_SWIN: return p.run_stats && p.str && !p.stiles.empty();
    case R_SBYTES: return p.run_stats && p.str;
    case R_XIN: case R_XNN: case R_XOUT: return p.want_index;
    case R_BLOOM: return p.bloom > 0;
    default: return true;
    }
}

struct Ptr { uint64_t a, bytes; int reg; const char* what; };

void check_arena(EncPlan& p, const Input& in) {
    const size_t temp = 4096 + 8 * p.scan_elems;   // (enc_scan_temp's answer is the device library's; any size must lay out)
    layout_encode(p, temp);
    std::vector<std::pair<size_t, int>> order;
    for (int r = 0; r < N_ENC_REGIONS; r++) {
        const Region& g = p.reg[r];
        if (r == R_BLOOM && !p.bloom) { check(g.size == 0, "a Bloom region without a filter"); continue; }
        check(g.off % 256 == 0, "region %d at %zu", r, g.off);
        check(g.size >= 1 && g.off + g.size <= p.a_sz, "region %d [%zu, +%zu) past a_sz %zu", r, g.off, g.size, p.a_sz);
        if (!region_used(p, r)) check(g.size == 1, "region %d unused, %zu bytes", r, g.size);
        order.push_back({g.off, r});
    }
    check(p.reg[R_TEMP].size == temp && (!p.bloom || p.reg[R_BLOOM].size == p.bloom) && p.reg[R_COL].size == 256, "temp / bloom / collide sizes");
    for (size_t i = 0; i + 1 < order.size(); i++) {   // today's order, and disjoint
        check(order[i].second < order[i + 1].second, "regions %d and %d out of order", order[i].second, order[i + 1].second);
        check(order[i].first + p.reg[order[i].second].size <= order[i + 1].first, "regions %d and %d overlap", order[i].second, order[i + 1].second);
    }
    for (int on_device = 0; on_device < 2; on_device++) {
        bind_encode(p, ARENA, &in.col, on_device != 0);
        const EncArgs& e = p.ea;
        const size_t N1 = size_t(p.n) + 1, n = size_t(p.n), w = size_t(p.w);
        check(e.ptype == p.pt && e.width == p.w && e.n == p.n, "EncArgs head");
        if (on_device) {
            check(e.values == in.col.values && e.offsets == in.col.offsets && e.chars == in.col.chars &&
                      e.validity == (p.has_val ? in.col.validity : nullptr), "on_device: the caller's arrays");
        } else {
            check(addr(e.values) == addr(ARENA) + p.reg[R_IN].off && addr(e.offsets) == addr(ARENA) + p.reg[R_OF].off &&
                      addr(e.chars) == addr(ARENA) + p.reg[R_CH].off && (p.has_val ? addr(e.validity) == addr(ARENA) + p.reg[R_VL].off : !e.validity),
                  "host inputs' regions");
            check(p.reg[R_IN].size >= (p.str ? 0 : n * w) && p.reg[R_VL].size >= p.vbytes && p.reg[R_OF].size >= (p.str ? 4 * N1 : 0) &&
                      p.reg[R_CH].size >= size_t(p.chars_len), "host inputs' sizes");
        }
        std::vector<Ptr> ptrs = {
            {addr(e.flag), 4 * N1, R_FLAG, "flag"}, {addr(e.pos), 4 * N1, R_POS, "pos"}, {addr(e.dense), n * w, R_DENSE, "dense"},
            {addr(e.key), 8 * N1, R_KEY, "key"}, {addr(e.skey), 8 * N1, R_SKEY, "skey"}, {addr(e.didx), 4 * N1, R_DIDX, "didx"},
            {addr(e.sidx), 4 * N1, R_SIDX, "sidx"}, {addr(e.headpos), 4 * N1, R_HP, "headpos"}, {addr(e.head), 4 * N1, R_HEAD, "head"},
            {addr(e.mark), 4 * N1, R_MARK, "mark"}, {addr(e.did), 4 * N1, R_DID, "did"}, {addr(e.dsz), 4 * N1, R_DSZ, "dsz"},
            {addr(e.doff), 4 * N1, R_DOFF, "doff"}, {addr(e.ids), 4 * N1, R_IDS, "ids"}, {addr(e.collide), 256, R_COL, "collide"},
            {addr(p.temp), temp, R_TEMP, "temp"}, {addr(p.ha.streams), sizeof(HybridStream) * p.n_hs_max, R_HSTR, "hybrid streams"},
            {addr(p.ha.bytes), 4 * p.n_hs_max, R_HBY, "hybrid bytes"}};
        if (p.str)
            for (Ptr q : {Ptr{addr(e.dsrc), 4 * N1, R_DSRC, "dsrc"}, Ptr{addr(e.dlen), 4 * N1, R_DLEN, "dlen"}, Ptr{addr(e.vsz), 4 * N1, R_VSZ, "vsz"},
                          Ptr{addr(e.vpre), 4 * N1, R_VPRE, "vpre"}})
                ptrs.push_back(q);
        if (p.bloom) ptrs.push_back({addr(p.d_bloom), p.bloom, R_BLOOM, "bloom"});
        if (p.delta_bit) {
            const DeltaArgs& d = p.da;
            const size_t NI1 = size_t(p.n_items) + 1;
            check(d.n_streams + 1 == p.dstreams.size() && d.n_pages == p.dpages.size() && d.n_items == p.n_items, "DeltaArgs counts");
            for (Ptr q : {Ptr{addr(d.streams), sizeof(DeltaStream) * p.dstreams.size(), R_DSTR, "delta streams"},
                          Ptr{addr(d.pages), sizeof(DeltaPage) * p.dpages.size(), R_DPG, "delta pages"}, Ptr{addr(d.bytes), 4 * NI1, R_DBY, "delta bytes"},
                          Ptr{addr(d.off), 4 * NI1, R_DOF, "delta off"}, Ptr{addr(d.minv), 8 * NI1, R_DMIN, "delta minv"},
                          Ptr{addr(d.widths), 4 * NI1, R_DWD, "delta widths"}, Ptr{addr(d.totals), 4 * p.dpages.size(), R_DTOT, "delta totals"}})
                ptrs.push_back(q);
            if (p.str)
                for (Ptr q : {Ptr{addr(d.pfx), 4 * N1, R_PFX, "pfx"}, Ptr{addr(d.sfx), 4 * N1, R_SFX, "sfx"}, Ptr{addr(d.spre), 4 * N1, R_SPRE, "spre"}})
                    ptrs.push_back(q);
            else check(!d.pfx && !d.sfx && !d.spre, "integer delta with string tables");
            for (size_t s = 0; s + 1 < p.dstreams.size(); s++) {
                const DeltaStream& ds = p.dstreams[s];
                const DeltaPage& g = p.dpages[ds.page];
                const int reg = !p.str ? R_DENSE : s - g.s0 == 0 ? R_PFX : R_SFX;
                const uint64_t base = addr(ARENA) + p.reg[reg].off, want = base + uint64_t(g.d0) * ds.ew;
                check(addr(ds.src) == want && want + uint64_t(ds.cnt) * ds.ew <= base + p.reg[reg].size, "delta stream %zu: src", s);
            }
        }
        if (p.run_stats) {
            const StatArgs& s = p.sa;
            const size_t nt = p.stiles.size();
            check(s.n_tiles == nt && s.n_pages == p.pp.size(), "StatArgs counts");
            for (Ptr q : {Ptr{addr(s.tiles), sizeof(StatTile) * nt, R_STT, "tiles"}, Ptr{addr(s.ptile), 4 * p.sptile.size(), R_STP, "ptile"},
                          Ptr{addr(s.part), sizeof(StatPart) * nt, R_SPART, "part"}, Ptr{addr(s.win), p.str ? 8 * nt : 0, R_SWIN, "win"},
                          Ptr{addr(s.out), sizeof(StatPart) * p.n_se, R_SOUT, "stat out"}, Ptr{addr(s.bytes), p.str ? size_t(ST_LIMIT) * p.n_se : 0, R_SBYTES, "stat bytes"}})
                ptrs.push_back(q);
        }
        if (p.want_index) {
            const PgIndexArgs& x = p.xa;
            const uint64_t xo = addr(ARENA) + p.reg[R_XOUT].off;
            check(x.pages == p.sa.out && x.n_pages == p.n_px && x.trunc == p.px_trunc && x.value_cap == p.px_cap, "PgIndexArgs head");
            check(addr(x.head) == xo && addr(x.null_counts) == xo + p.px_nc && addr(x.off) == xo + p.px_off && addr(x.null_pages) == xo + p.px_np &&
                      addr(x.values) == xo + p.px_val && p.reg[R_XOUT].size >= p.px_bytes, "PgIndexArgs block");
            check(x.cnt == x.rows + p.n_px, "PgIndexArgs cnt");
            ptrs.push_back({addr(x.rows), 8 * p.n_px, R_XIN, "index rows"});
            ptrs.push_back({addr(x.nn), 4 * p.n_px, R_XNN, "index nn"});
        }
        for (const Ptr& q : ptrs) {
            const uint64_t lo = addr(ARENA) + p.reg[q.reg].off;
            check(q.a == lo && q.bytes <= p.reg[q.reg].size, "%s: %llx (+%llu) not its region %d at %llx (+%zu)", q.what, (unsigned long long)q.a,
                  (unsigned long long)q.bytes, q.reg, (unsigned long long)lo, p.reg[q.reg].size);
        }
    }
    bind_encode(p, ARENA, &in.col, false);
}

// ---------------------------------------------------------------- values, sections
uint64_t delta_worst(const EncPlan& p, const EncPagePlan& g) {   // what plan_encode bounds by 2 GiB
    const uint64_t ns = p.str ? 2 : 1, blocks = g.cnt > 1 ? (g.cnt - 1 + 127) / 128 : 0;
    return ns * (25ull + blocks * 14ull + uint64_t(g.cnt) * (p.str ? 4 : p.w)) + (p.str ? g.plain : 0);
}

// Sizes for the size passes' results: fill 0: all 0; 1: the worst case; 2: mixed.
void feed_sizes(EncPlan& p, int fill) {
    for (size_t s = 0; s < p.hs.size(); s++) {
        const uint64_t worst = hybrid_worst(p.hs[s].cnt, p.hs[s].bw);
        p.hbytes[s] = uint32_t(fill == 0 ? 0 : fill == 1 ? worst : mix(s + 5) % (worst + 1));
    }
    p.htot.assign(p.delta ? p.pp.size() : 0, 0);
    for (size_t i = 0; i < p.htot.size(); i++) {
        const uint64_t worst = delta_worst(p, p.pp[i]);
        p.htot[i] = uint32_t(fill == 0 ? 0 : fill == 1 ? worst : mix(i + 9) % (worst + 1));
    }
}

void check_values(const EncPlan& p, uint32_t collide, uint32_t D, uint32_t dbytes) {
    const bool dict_bit = (p.bits & PF_ENCODE_DICTIONARY) != 0, boolean = p.pt == PF_BOOLEAN;
    const bool want = dict_bit && !boolean && p.m > 0;   // (4 m + chars < 4 GiB in every case here)
    int fb = 0;
    if (dict_bit && boolean) fb = 3;
    else if (want && collide) fb = 2;
    else if (want && (p.str ? int64_t(dbytes) : int64_t(D) * p.w) > p.dict_limit) fb = 1;
    check(p.want_dict == want && p.fallback == fb && p.dict == (want && fb == 0), "fallback %d (expected %d), dict %d", p.fallback, fb, int(p.dict));
    check(p.D == (p.dict ? D : 0) && p.dict_bytes == (p.dict ? (p.str ? dbytes : D * uint32_t(p.w)) : 0), "D %u, dict_bytes %u", p.D, p.dict_bytes);
    uint32_t bw = 0;
    while ((uint64_t(1) << bw) < p.D) bw++;   // bits of D - 1; at least 1, but parquet-mr's 0 for one entry under hybrid runs
    check(p.bw == (p.hyb && p.D == 1 ? 0u : std::max(bw, 1u)), "bw %u for D %u", p.bw, p.D);
    check(p.brle == (p.hyb && boolean) && p.delta == (p.delta_bit && !p.dict), "brle / delta");
    const int enc = p.dict ? PF_ENC_RLE_DICTIONARY : p.delta ? (p.str ? PF_ENC_DELTA_BYTE_ARRAY : PF_ENC_DELTA_BINARY_PACKED) : p.brle ? PF_ENC_RLE : PF_ENC_PLAIN;
    check(p.data_enc == enc, "data_enc %d, expected %d", p.data_enc, enc);
    size_t ns = 0;
    for (size_t i = 0; i < p.pp.size(); i++) {
        check((p.lv_of[i] >= 0) == (p.hyb && p.max_def == 1) && (p.vs_of[i] >= 0) == (p.hyb && (p.dict || p.brle)), "page %zu: streams", i);
        if (p.lv_of[i] >= 0) {
            const HybridStream& s = p.hs[size_t(p.lv_of[i])];
            check(s.kind == HY_VALIDITY && s.src == p.ea.validity && s.first == p.pp[i].r0 && s.cnt == p.pp[i].r1 - p.pp[i].r0 && s.bw == 1 &&
                      s.prefix == HY_PREFIX_NONE && s.page == i, "page %zu: level stream", i);
            ns++;
        }
        if (p.vs_of[i] >= 0) {
            const HybridStream& s = p.hs[size_t(p.vs_of[i])];
            check(s.first == p.pp[i].d0 && s.cnt == p.pp[i].cnt && s.page == i &&
                      (p.dict ? s.kind == HY_IDS && addr(s.src) == addr(p.ea.ids) && s.bw == p.bw && s.prefix == HY_PREFIX_WIDTH
                              : s.kind == HY_BOOL && s.src == p.ea.dense && s.bw == 1 && s.prefix == HY_PREFIX_LENGTH), "page %zu: value stream", i);
            ns++;
        }
    }
    check(p.hs.size() == ns && ns <= p.n_hs_max && p.hbytes.size() == ns && p.ha.n_streams == (p.hyb ? ns : p.ha.n_streams), "hybrid stream count %zu", p.hs.size());
}

void check_sections(const EncPlan& p) {
    const size_t np = p.pp.size();
    check(p.sections.size() == np + (p.dict ? 1 : 0), "%zu sections for %zu pages", p.sections.size(), np);
    uint64_t end = 0;
    for (size_t i = 0; i < p.sections.size(); i++) {   // in order, disjoint, aligned, inside vo
        check(p.sections[i].first % 256 == 0 && p.sections[i].first >= end && p.sections[i].first + p.sections[i].second <= p.vo, "section %zu [%llu, +%llu), vo %zu",
              i, (unsigned long long)p.sections[i].first, (unsigned long long)p.sections[i].second, p.vo);
        end = p.sections[i].first + std::max<uint64_t>(p.sections[i].second, 1);
    }
    if (p.dict) check(p.sections[0].first == p.o_dict && p.sections[0].second == p.dict_bytes, "dictionary section");
    const size_t b = p.dict ? 1 : 0;
    for (size_t i = 0; i < np && p.sections.size() == np + b; i++) {
        const auto& sct = p.sections[b + i];
        if (p.delta) {
            check(p.dpages[i].out_off == sct.first && sct.second == p.htot[i], "delta page %zu: section", i);
            continue;
        }
        check(p.ep[i].out_off == sct.first && p.ep[i].d0 == p.pp[i].d0 && p.ep[i].cnt == p.pp[i].cnt && p.ep[i].dict == (p.dict ? 1u : 0u) && p.ep[i].bw == p.bw,
              "EncPage %zu", i);
        if (p.vs_of[i] >= 0) {
            const uint64_t pre = p.dict ? 1 : 4;
            check(sct.second == pre + p.hbytes[size_t(p.vs_of[i])] && p.hs[size_t(p.vs_of[i])].out_off == sct.first + pre, "page %zu: hybrid values section", i);
        } else if (p.dict) {
            const uint64_t groups = (p.pp[i].cnt + 7) / 8;
            check(sct.second == (p.pp[i].cnt ? 1 + uvarint_len((groups << 1) | 1) + groups * p.bw : 1), "page %zu: ids section %llu", i, (unsigned long long)sct.second);
        } else {
            check(sct.second == p.pp[i].plain, "page %zu: PLAIN section", i);
        }
    }
    if (p.hyb) {   // levels behind every values section, the EncPage table behind them
        check(p.o_lv >= end && p.o_lv % 256 == 0 && p.o_lv + p.lv_total <= p.vo, "levels [%zu, +%zu), sections end %llu, vo %zu", p.o_lv, p.lv_total,
              (unsigned long long)end, p.vo);
        size_t at = 0;
        for (size_t i = 0; i < np; i++)
            if (p.lv_of[i] >= 0) {
                check(p.lv_off[i] == at && p.hs[size_t(p.lv_of[i])].out_off == p.o_lv + at, "page %zu: levels placement", i);
                at += p.hbytes[size_t(p.lv_of[i])];
            }
        check(at == p.lv_total, "lv_total %zu, summed %zu", p.lv_total, at);
        end = p.o_lv + std::max<size_t>(p.lv_total, 1);
    } else {
        check(p.lv_total == 0, "levels without hybrid runs");
    }
    if (!p.delta) check(p.o_pages >= end && p.o_pages % 256 == 0 && p.o_pages + sizeof(EncPage) * p.ep.size() <= p.vo, "EncPage table at %zu", p.o_pages);
    else check(p.ep.empty(), "EncPage entries on the delta route");
    if (p.hyb && !p.delta) check(p.vo <= p.ub, "vo %zu over the reserved %zu: d_enc_sec would move", p.vo, p.ub);
}

// ---------------------------------------------------------------- compression layout
void check_compress(const EncPlan& p, const CompressPlan& cp, size_t n_extra) {
    const bool zs = p.codec == PF_CODEC_ZSTD;
    const uint32_t JOB = zs ? ZC_BLOCK : SC_BLOCK, SLOT = zs ? ZC_SLOT : SC_SLOT;
    check(cp.JOB == JOB && cp.SLOT == SLOT && cp.range.size() == p.sections.size() && cp.src_off.size() == cp.jobs.size(), "compress plan head");
    size_t k = 0;
    for (size_t i = 0; i < p.sections.size(); i++) {
        check(cp.range[i].first == k, "section %zu: first job %zu, expected %zu", i, cp.range[i].first, k);
        uint64_t at = 0;
        for (; k < cp.range[i].second && k < cp.jobs.size(); k++) {
            const bool last_job = at + cp.jobs[k].len == p.sections[i].second;
            check(cp.src_off[k] == p.sections[i].first + at && cp.jobs[k].len > 0 && (cp.jobs[k].len == JOB || last_job), "job %zu of section %zu", k, i);
            check(cp.jobs[k].last == ((zs && last_job) ? 1u : 0u), "job %zu: last %u", k, cp.jobs[k].last);
            at += cp.jobs[k].len;
        }
        check(at == p.sections[i].second && (p.sections[i].second > 0 || cp.range[i].first == cp.range[i].second), "section %zu: jobs cover %llu of %llu", i,
              (unsigned long long)at, (unsigned long long)p.sections[i].second);
    }
    const size_t nj = cp.jobs.size();
    check(k == nj && cp.np == (p.want_crc ? nj + n_extra : 0), "jobs %zu, counted %zu; pieces %zu", nj, k, cp.np);
    const size_t sizes[4] = {sizeof(CompJob) * std::max<size_t>(nj, 1), cp.len_bytes, sizeof(CrcPiece) * std::max<size_t>(cp.np, 1), size_t(SLOT) * std::max<size_t>(nj, 1)};
    const size_t offs[4] = {cp.o_jobs, cp.o_len, cp.o_pieces, cp.o_slots};
    for (int i = 0; i < 4; i++) {
        check(offs[i] % 256 == 0 && offs[i] + sizes[i] <= cp.arena, "compress region %d", i);
        if (i) check(offs[i - 1] + sizes[i - 1] <= offs[i], "compress regions %d and %d overlap", i - 1, i);
    }
    // the one D2H of len_bytes from o_len covers the lengths and the CrcOut block
    check(4 * nj <= cp.o_crc_in_len && cp.o_crc_in_len % 16 == 0, "o_crc_in_len %zu", cp.o_crc_in_len);
    check(cp.np ? cp.o_crc_in_len + sizeof(CrcOut) * cp.np == cp.len_bytes : cp.len_bytes >= 4 * nj, "len_bytes %zu", cp.len_bytes);
    CompressPlan b = cp;
    bind_compress(b, SEC, OUT, &p.lv_pieces);
    for (size_t j = 0; j < nj; j++) {
        check(addr(b.jobs[j].src) == addr(SEC) + cp.src_off[j] && addr(b.jobs[j].dst) == addr(OUT) + cp.o_slots + j * SLOT, "job %zu: bound pointers", j);
        if (cp.np) check(b.pieces[j].ptr == b.jobs[j].dst && addr(b.pieces[j].len_ptr) == addr(OUT) + cp.o_len + 4 * j && b.pieces[j].cap == SLOT, "job %zu: CRC piece", j);
    }
    for (size_t j = nj; j < cp.np; j++) check(b.pieces[j].ptr == p.lv_pieces[j - nj].ptr && b.pieces[j].len == p.lv_pieces[j - nj].len && !b.pieces[j].len_ptr, "extra piece %zu", j);
}

// ---------------------------------------------------------------- assembly
CrcOut crc_of(const uint8_t* b, size_t n) { return CrcOut{crc_raw_bytes(0, b, n), uint32_t(n), crc_x8n(n, crc_x2n_host()), 0}; }
uint32_t crc32_of(const uint8_t* b, size_t n) { return crc_finish(crc_raw_bytes(0, b, n), n); }

struct Synth {
    std::vector<std::vector<uint8_t>> bodies;
    std::vector<uint8_t> hlv, hsb, px, bloom;
    std::vector<CrcOut> crcs;
    std::vector<StatPart> hst;
    size_t crc_first_lv = 0;
};

// Bodies as a device would leave them: per section stream_head and job outputs of chosen lengths (0, SLOT and
// lengths between), or the section's bytes themselves; CrcOuts of the pieces from those bytes.
void synthesize(EncPlan& p, const Input& in, Synth& s) {
    const size_t np = p.pp.size();
    uint64_t seed = 1;
    auto fill = [&](std::vector<uint8_t>& o, size_t n) { for (size_t i = 0; i < n; i++) o.push_back(uint8_t(mix(seed++) >> 7)); };
    plan_crc_levels(p, SEC);
    fill(s.hlv, p.lv_total);
    s.bodies.reserve(p.sections.size());
    if (p.compressed) {
        plan_compress(p.sections, p.codec, p.want_crc, p.lv_pieces.size(), p.comp);
        check_compress(p, p.comp, p.lv_pieces.size());
        const uint32_t lens[6] = {0, p.comp.SLOT, 1, 5, 300, 3};
        for (size_t i = 0; i < p.sections.size(); i++) {
            uint8_t head[12];
            std::vector<uint8_t> o(head, head + stream_head(p.codec, p.sections[i].second, head));
            for (size_t k = p.comp.range[i].first; k < p.comp.range[i].second; k++) {
                const size_t at = o.size(), len = lens[(k + i) % 6];
                fill(o, len);
                if (p.want_crc) s.crcs.push_back(crc_of(o.data() + at, len));
            }
            s.bodies.push_back(std::move(o));
        }
        s.crc_first_lv = p.comp.jobs.size();
    } else {
        for (const auto& sct : p.sections) {
            std::vector<uint8_t> o;
            fill(o, size_t(sct.second));
            if (p.want_crc) s.crcs.push_back(crc_of(o.data(), o.size()));
            s.bodies.push_back(std::move(o));
        }
        s.crc_first_lv = p.sections.size();
        const char* why = "";
        if (p.want_crc) check(plan_section_pieces(p, SEC, &why) == PF_OK && p.sec_pieces.size() == p.sections.size() + p.lv_pieces.size(), "section pieces");
    }
    for (size_t i = 0; i < np && p.want_crc; i++) {   // the level pieces, in lv_pieces' order
        if (p.lv_piece[i] >= 0) {
            check(size_t(p.lv_piece[i]) + s.crc_first_lv == s.crcs.size(), "page %zu: level piece index", i);
            check(addr(p.lv_pieces[size_t(p.lv_piece[i])].ptr) == addr(SEC) + p.o_lv + p.lv_off[i], "page %zu: level piece address", i);
            s.crcs.push_back(crc_of(s.hlv.data() + p.lv_off[i], p.hbytes[size_t(p.lv_of[i])]));
        } else if (p.vb_piece[i] >= 0) {
            const size_t nb = size_t(p.pp[i].r1 - p.pp[i].r0) / 8;
            check(size_t(p.vb_piece[i]) + s.crc_first_lv == s.crcs.size(), "page %zu: validity piece index", i);
            check(p.lv_pieces[size_t(p.vb_piece[i])].ptr == p.ea.validity + p.pp[i].r0 / 8 && p.lv_pieces[size_t(p.vb_piece[i])].len == nb, "page %zu: validity piece", i);
            s.crcs.push_back(crc_of(in.hval.data() + p.pp[i].r0 / 8, nb));
        }
        check((p.lv_piece[i] >= 0) == (p.lv_of[i] >= 0) && (p.vb_piece[i] >= 0) == (p.lv_of[i] < 0 && p.has_val && p.pp[i].r1 - p.pp[i].r0 >= 8), "page %zu: level form", i);
    }
    if (p.want_stats) {
        s.hst.assign(p.n_se, StatPart{});
        s.hsb.assign(p.str ? size_t(ST_LIMIT) * p.n_se : 1, 'a');
        for (size_t e = 0; e < p.n_se; e++) {
            s.hst[e].any = uint32_t(e % 3 == 2 ? 0 : 1);
            s.hst[e].mn = e; s.hst[e].mx = e + 7;
            s.hst[e].mnl = uint32_t(e % 4); s.hst[e].mxl = 3;
        }
    }
    s.px.assign(std::max<size_t>(p.px_bytes, sizeof(PgIndexHead)), 0);
    if (p.want_index) { PgIndexHead hd{1, 1, 0, 0}; std::memcpy(s.px.data(), &hd, sizeof hd); }
    s.bloom.assign(std::max<size_t>(p.bloom, 1), 0x5a);
}

struct Chunk {
    std::vector<uint8_t> bytes, stat;
    std::vector<int64_t> pgoff, pgrow;
    std::vector<int32_t> pgsize;
    pf_encoded_chunk out{};
};

int run_assemble(const EncPlan& p, const Input& in, const Synth& s, Chunk& c, const char** why) {
    AssembleIn a{};
    a.hval = &in.hval; a.bodies = &s.bodies; a.hlv = s.hlv.data(); a.crcs = s.crcs.data(); a.crc_first_lv = s.crc_first_lv;
    a.hst = p.want_stats ? s.hst.data() : nullptr; a.hsb = p.want_stats ? s.hsb.data() : nullptr;
    a.px = p.want_index ? s.px.data() : nullptr; a.bloom = p.bloom ? s.bloom.data() : nullptr;
    AssembledChunk ac{&c.bytes, &c.stat, &c.pgoff, &c.pgrow, &c.pgsize};
    return assemble_chunk(p, a, ac, &c.out, why);
}

// PageHeader.crc (field 4) of the header at h: fields 1..3 are i32, then 4 if present (Thrift compact, in field order).
bool header_crc(const uint8_t* h, size_t n, uint32_t& crc) {
    size_t k = 0;
    auto i32 = [&](uint32_t& v) {
        uint64_t z = 0;
        for (int sh = 0; k < n; sh += 7) { const uint8_t b = h[k++]; z |= uint64_t(b & 0x7f) << sh; if (!(b & 0x80)) break; }
        v = uint32_t((z >> 1) ^ (~(z & 1) + 1));
    };
    uint32_t v;
    for (int f = 0; f < 3; f++) { if (k >= n || h[k++] != 0x15) return false; i32(v); }
    if (k >= n || h[k++] != 0x15) return false;
    i32(crc);
    return true;
}

void check_assembly(EncPlan& p, const Input& in, bool wrong_piece) {
    Synth s;
    synthesize(p, in, s);
    Chunk c;
    const char* why = "";
    const int rc = run_assemble(p, in, s, c, &why);
    check(rc == PF_OK, "assemble_chunk: %d '%s'", rc, why);
    if (rc) return;
    const pf_encoded_chunk& o = c.out;
    const size_t np = p.pp.size(), b = p.dict ? 1 : 0;
    std::vector<pf_page_desc> pages;
    try {
        if (p.n > 0) {
            ChunkMeta m;
            m.num_values = p.n;
            FileMeta::walk_pages(c.bytes.data(), c.bytes.size(), m, pages);
        } else {   // (walk_pages stops at num_values: the one empty page is read by its reader)
            pf_page_desc d;
            d.offset = read_page_header(c.bytes.data(), c.bytes.size(), d);
            pages.push_back(d);
        }
    } catch (const MetaError& e) {
        check(false, "the page walk fails: %s", e.what());
        return;
    }
    check(pages.size() == np + b && o.n_data_pages == int32_t(np) && o.bytes == c.bytes.data() && o.size == int64_t(c.bytes.size()), "%zu pages walked, %zu planned", pages.size(), np + b);
    if (pages.size() != np + b) return;
    check(o.dictionary_page_offset == (p.dict ? 0 : -1) && o.num_values == p.n && o.dict_entries == int32_t(p.D) && o.data_encoding == p.data_enc &&
              o.fallback == p.fallback && o.codec == p.codec && o.bloom_len == int32_t(p.bloom) && (p.bloom ? o.bloom == s.bloom.data() : !o.bloom), "chunk fields");
    int64_t unc = 0, sin = 0, sout = 0;
    size_t prev_end = 0;
    for (size_t k = 0; k < pages.size(); k++) {
        const pf_page_desc& d = pages[k];
        const size_t hdr0 = prev_end, hdr_len = size_t(d.offset) - hdr0;
        const bool is_dict = p.dict && k == 0;
        const size_t i = k - b;
        unc += int64_t(hdr_len) + d.uncompressed_size;
        if (p.compressed) { sin += int64_t(p.sections[k].second); sout += int64_t(s.bodies[k].size()); }
        if (is_dict) {
            check(d.page_type == PF_PAGE_DICTIONARY && d.encoding == PF_ENC_PLAIN && d.num_values == int32_t(p.D) && d.uncompressed_size == p.dict_bytes &&
                      d.compressed_size == s.bodies[0].size(), "dictionary page header");
        } else {
            const EncPagePlan& g = p.pp[i];
            const int64_t rows = g.r1 - g.r0;
            size_t def = 0;
            if (p.lv_of[i] >= 0) def = p.hbytes[size_t(p.lv_of[i])];
            else if (p.max_def == 1 && rows > 0) def = uvarint_len(((uint64_t(rows + 7) / 8) << 1) | 1) + size_t(rows + 7) / 8;
            check(d.page_type == PF_PAGE_DATA_V2 && d.encoding == p.data_enc && d.num_values == rows && d.num_rows == rows && d.num_nulls == rows - g.cnt &&
                      d.def_bytes == int32_t(def) && d.rep_bytes == 0 && d.is_compressed == (p.compressed ? 1 : 0), "page %zu header", i);
            check(d.uncompressed_size == def + p.sections[k].second && d.compressed_size == def + s.bodies[k].size(), "page %zu sizes", i);
            if (i == 0) check(o.data_page_offset == int64_t(hdr0), "data_page_offset");
            if (p.want_index) check(c.pgoff[i] == int64_t(hdr0) && c.pgsize[i] == int32_t(hdr_len + d.compressed_size) && c.pgrow[i] == g.r0, "page %zu: OffsetIndex entry", i);
            if (def && p.lv_of[i] < 0) {   // the host's bit-packed run repeats the validity bits
                const uint8_t* lv = c.bytes.data() + d.offset + (def - size_t(rows + 7) / 8);
                bool same = true;
                for (int64_t r = 0; r < rows; r++) same &= ((lv[r >> 3] >> (r & 7)) & 1) == (p.has_val ? (in.hval[size_t((g.r0 + r) >> 3)] >> ((g.r0 + r) & 7)) & 1 : 1);
                check(same, "page %zu: level bits", i);
            }
        }
        uint32_t crc = 0;
        const bool has = header_crc(c.bytes.data() + hdr0, hdr_len, crc);
        check(has == p.want_crc, "page %zu: crc field %d", k, int(has));
        if (has) check(crc == crc32_of(c.bytes.data() + d.offset, d.compressed_size), "page %zu: crc %08x is not the stored bytes'", k, crc);
        prev_end = size_t(d.offset) + d.compressed_size;
    }
    check(prev_end == c.bytes.size() && o.total_uncompressed_size == unc && o.snappy_in == sin && o.snappy_out == sout, "chunk sizes: uncompressed %lld, summed %lld",
          (long long)o.total_uncompressed_size, (long long)unc);
    check(o.index_pages == int32_t(p.n_px) && (p.want_index ? o.page_offset == c.pgoff.data() && o.column_index == 1 && o.index_null_pages == s.px.data() + p.px_np
                                                            : !o.page_offset && !o.index_null_pages), "index fields");
    check(p.want_stats ? (o.stats_flags & PF_STATS_NULL_COUNT) && o.null_count == p.n - int64_t(p.m) : o.stats_flags == 0, "chunk statistics");
    if (wrong_piece && p.want_crc && !s.crcs.empty()) {   // a piece whose length is off by one: reported, not written
        const size_t which = p.codec == PF_CODEC_SNAPPY ? 0 : p.codec == PF_CODEC_ZSTD ? s.crcs.size() - 1 : s.crcs.size() / 2;
        s.crcs[which].len += 1;
        Chunk c2;
        const int rc2 = run_assemble(p, in, s, c2, &why);
        check(rc2 == PF_ERR_HIP && std::strcmp(why, "encode: the CRC pieces of a page do not add up to its size") == 0, "a wrong piece %zu: %d '%s'", which, rc2, why);
    }
}

// ---------------------------------------------------------------- the grid
// What a check reads decides where in the grid it runs in full: the page plan depends on the column alone, the
// tables and the sections on the column and the option bits, the arena also on the filter, the compression
// layout and the assembly also on the codec. At the other grid points the plan is compared with the checked one.
struct Checked {
    std::vector<EncPagePlan> pp;
    uint32_t m = 0, n_items = 0;
    size_t n_tiles = 0, px_bytes = 0;
};

bool same_pages(const std::vector<EncPagePlan>& a, const std::vector<EncPagePlan>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].r0 != b[i].r0 || a[i].r1 != b[i].r1 || a[i].d0 != b[i].d0 || a[i].cnt != b[i].cnt || a[i].plain != b[i].plain) return false;
    return true;
}

void run_case(const Input& base, int bits, int codec, int bloom, Checked& col_plan, Checked& bits_plan) {
    Input in = base;
    in.col.dictionary = bits; in.col.codec = codec; in.col.bloom_bytes = bloom;
    EncPlan p;
    const char* why = "";
    const int rc = plan_encode(&in.col, in.hval, in.hoff, p, &why);
    check(rc == PF_OK, "plan_encode: %d '%s'", rc, why);
    if (rc) return;
    g_cases++;
    check(p.bloom == (in.col.physical_type == PF_BOOLEAN ? 0u : unsigned(bloom)) && p.dict_limit == (1 << 20) && p.compressed == (codec != PF_CODEC_UNCOMPRESSED), "settings");
    const bool first_of_bits = codec == PF_CODEC_SNAPPY && bloom == 0;
    if (col_plan.pp.empty()) {
        check_page_plan(p, in);
        col_plan.pp = p.pp;
        col_plan.m = p.m;
    } else {
        check(same_pages(p.pp, col_plan.pp) && p.m == col_plan.m, "the page plan depends on more than the column");
    }
    if (first_of_bits) {
        check_tables(p);
        bits_plan.n_items = p.n_items; bits_plan.n_tiles = p.stiles.size(); bits_plan.px_bytes = p.px_bytes;
    } else {
        check(p.n_items == bits_plan.n_items && p.stiles.size() == bits_plan.n_tiles && p.px_bytes == bits_plan.px_bytes, "the tables depend on more than column and bits");
    }
    if (codec == PF_CODEC_SNAPPY) check_arena(p, in);
    else { layout_encode(p, 4096); bind_encode(p, ARENA, &in.col, false); }
    // the dictionary's answers: a small one / one entry / a collision / over the page limit
    const uint32_t Dsmall = std::min<uint32_t>(std::max<uint32_t>(p.m, 1), 5), D1 = 1;
    const uint32_t tries[4][3] = {{0, Dsmall, 4 * Dsmall + 9}, {0, D1, 4}, {1, Dsmall, 4 * Dsmall + 9}, {0, (1u << 20) / 4 + 1, (1u << 20) + 1}};
    for (int t = 0; t < (p.want_dict ? 4 : 1); t++) {
        plan_values(p, tries[t][0], tries[t][1], tries[t][2]);
        check_values(p, tries[t][0], tries[t][1], tries[t][2]);
        for (int fill = first_of_bits ? 0 : 2; fill < 3; fill++) {
            feed_sizes(p, fill);
            const int rs = plan_sections(p, &why);
            check(rs == PF_OK, "plan_sections: %d '%s'", rs, why);
            if (rs) continue;
            if (first_of_bits) check_sections(p);
            // the three codecs; with a filter only the first route, its off-by-one CRC piece included
            // (chunks of more than 64 pages, thousands of pages that are all alike: under the two combined bit sets and the
            // dictionary's first answer only, with a filter under all six bits only)
            const bool big = p.pp.size() > 64;
            const bool assemble = !big || (t == 0 && (bits == 63 || (bits == (1 | 2 | 4) && bloom == 0)));
            if (fill == 2 && t < 3 && (bloom == 0 || t == 0) && assemble) check_assembly(p, in, bloom != 0);
        }
    }
}

void check_hybrid_worst() {
    g_case = "hybrid_worst";
    for (uint64_t cnt : {0ull, 1ull, 7ull, 8ull, 9ull, 63ull * 8, 63ull * 8 + 1, 20000ull})
        for (uint32_t bw = 0; bw <= 32; bw++) {
            const uint64_t groups = (cnt + 7) / 8;
            const uint64_t packed = groups * bw + (groups + 62) / 63;                        // only bit-packed groups, 63 to a header
            const uint64_t rle = (cnt / 8) * (1 + (bw + 7) / 8) + (cnt % 8 ? 1 + bw : 0);   // only RLE runs of 8, and the last group
            check(hybrid_worst(cnt, bw) >= packed && hybrid_worst(cnt, bw) >= rle, "cnt %llu bw %u: %llu < max(%llu, %llu)", (unsigned long long)cnt, bw,
                  (unsigned long long)hybrid_worst(cnt, bw), (unsigned long long)packed, (unsigned long long)rle);
        }
}

}  // namespace

int main() {
    check_rejections();
    check_hybrid_worst();
    const int types[] = {PF_BOOLEAN, PF_INT32, PF_INT64, PF_FLOAT, PF_DOUBLE, PF_BYTE_ARRAY};
    const int64_t rows[] = {0, 1, 7, 8, 9, 17, 20000, 20001, 40007};
    const int page_rows[] = {8, 0, 13};
    const int bits[] = {1, 2, 4, 8, 16, 32, 1 | 2 | 4, 63};
    const int codecs[] = {PF_CODEC_SNAPPY, PF_CODEC_ZSTD, PF_CODEC_UNCOMPRESSED};
    for (int pt : types)
        for (int def_mode = 0; def_mode < 3; def_mode++)
            for (int64_t n : rows)
                for (int pr : page_rows) {
                    const Input base = make_input(pt, def_mode, n, pr);
                    Checked col_plan;
                    for (int b : bits) {
                        Checked bits_plan;
                        for (int codec : codecs)
                            for (int bloom : {0, 32}) {
                                char name[128];
                                std::snprintf(name, sizeof name, "type %d def %d rows %lld page_rows %d bits %d codec %d bloom %d", pt, def_mode, (long long)n, pr, b, codec, bloom);
                                g_case = name;
                                run_case(base, b, codec, bloom, col_plan, bits_plan);
                            }
                    }
                }
    std::printf("cases %ld checks %ld failures %d\n", g_cases, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
