// Checks of the decode's host-only result side (csrc/pf_result.cpp) without a GPU: the side-table layouts, the arena
// and rerun decisions, the merge of the decode's, the window's and the selection's view into pf_column_info, and the
// batch-copy layout with its pointer rebase. Every table is hand-made and every expected value is written out here;
// nothing is read through the made-up device addresses. Built with -fsanitize=address,undefined by
// tests/test_result_cpu.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pf_result.h"
#include "pfloor.h"

using namespace pf;

namespace {

int g_failures = 0;
long g_checks = 0;
std::string g_case;

void check(bool ok, const char* fmt, ...) {
    g_checks++;
    if (ok) return;
    if (++g_failures > 60) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "FAIL [%s] %s\n", g_case.c_str(), buf);
}
#define EQ(a, b) check((long long)(a) == (long long)(b), "%s = %lld, expected %lld (line %d)", #a, (long long)(a), (long long)(b), __LINE__)
#define PEQ(a, b) check((const void*)(a) == (const void*)(b), "%s = %p, expected %p (line %d)", #a, (const void*)(a), (const void*)(b), __LINE__)

// the sizes the hand-written offsets below rest on
static_assert(sizeof(DevChunkResult) == 40 && sizeof(DevChunk) == 184, "results block");
static_assert(sizeof(DevWin) == 24 && sizeof(DevWinRes) == 88, "window tables");
static_assert(sizeof(DevSelHead) == 24 && sizeof(DevSelChunk) == 104 && sizeof(DevPred) == 64, "filter tables");
static_assert(SEL_TILE == 1024 && WIN_TILE == 4096, "tiles");

// made-up device addresses: the twins lie below the decode arenas, so both deltas are negative and differ
constexpr uintptr_t OUT = 0x7f0000000000ull, BITS = 0x7e0000000000ull, CHARS = 0x7d0000000000ull;
constexpr uintptr_t WOUT = 0x7c0000000000ull, WBITS = 0x7b8000000000ull, WCHARS = 0x7a0000000000ull, SEL = 0x790000000000ull;
template <class T = uint8_t> T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }

// ---------------------------------------------------------------- res_layout, win_layout, win_grid
void test_layouts() {
    g_case = "res_layout";
    ResLayout r0 = res_layout(0);
    EQ(r0.res_bytes, 0); EQ(r0.chunks_off, 0); EQ(r0.chunks_bytes, 0); EQ(r0.total, 256);
    ResLayout r1 = res_layout(1);
    EQ(r1.res_bytes, 40); EQ(r1.chunks_off, 256); EQ(r1.chunks_bytes, 184); EQ(r1.total, 256 + 184 + 256);
    ResLayout r7 = res_layout(7);   // 280 bytes of results: the copies begin at 512
    EQ(r7.res_bytes, 280); EQ(r7.chunks_off, 512); EQ(r7.chunks_bytes, 1288); EQ(r7.total, 512 + 1288 + 256);

    g_case = "win_layout";
    WinLayout w1 = win_layout(1);
    EQ(w1.wins_bytes, 24); EQ(w1.res_off, 256); EQ(w1.res_bytes, 88); EQ(w1.total, 344);
    WinLayout w32 = win_layout(32);   // 32 * 24 = 768 = 3 * 256: no padding
    EQ(w32.wins_bytes, 768); EQ(w32.res_off, 768); EQ(w32.res_bytes, 2816); EQ(w32.total, 3584);
    WinLayout w11 = win_layout(11);   // 264 -> 512
    EQ(w11.res_off, 512); EQ(w11.total, 512 + 968);

    g_case = "win_grid";
    BatchPlan p;
    p.n_chunks = 4;
    p.chunks.assign(4, DevChunk{});
    p.chunks[0].width = 4; p.chunks[0].num_entries = 1 << 20;                            // flat INT32
    p.chunks[1].width = 8; p.chunks[1].num_entries = 40960; p.chunks[1].max_rep = 1;     // nested INT64
    p.chunks[2].width = 0; p.chunks[2].num_entries = 12288;                              // flat BYTE_ARRAY
    p.chunks[3].width = 8; p.chunks[3].num_entries = 1 << 22;                            // flat INT64
    EQ(win_grid(p, {}), 1);
    EQ(win_grid(p, {DevWin{0, 0, 5, 0}}), 8);                 // take 0: nothing but the + 8
    EQ(win_grid(p, {DevWin{0, 0, 5, 8192}}), 24);             // width 4 counts as 8: 8192 * 8 / 4096 + 8 (16 if it counted as 4)
    EQ(win_grid(p, {DevWin{0, 0, 5, -1}}), 512);              // to the end: 2^20 entries * 8 / 4096 + 8 = 2056, capped
    EQ(win_grid(p, {DevWin{1, 0, 0, 10}}), 88);               // nested: take ignored, 40960 * 8 / 4096 + 8
    EQ(win_grid(p, {DevWin{2, 0, 1, 4096}}), 16);             // width 0 counts as 8
    EQ(win_grid(p, {DevWin{2, 0, 1, -1}}), 32);               // 12288 * 8 / 4096 + 8
    EQ(win_grid(p, {DevWin{3, 0, 0, 258048}}), 512);          // 258048 * 8 / 4096 + 8 = 512: at the cap
    EQ(win_grid(p, {DevWin{3, 0, 0, 257536}}), 511);          // one tile less
    EQ(win_grid(p, {DevWin{3, 0, 0, 258560}}), 512);          // one more: capped
    EQ(win_grid(p, {DevWin{0, 0, 5, 8192}, DevWin{1, 0, 0, 10}, DevWin{2, 0, 1, 4096}}), 88);   // the largest
}

// ---------------------------------------------------------------- layout_filter, fill_filter, bind_sel
struct Region { const char* name; size_t off, bytes; };
std::vector<Region> regions(const SelLayout& l, size_t nc, size_t np, size_t blob) {
    const size_t t = l.tiles;
    return {{"head", l.o_head, 24}, {"sc", l.o_sc, 104 * nc}, {"preds", l.o_preds, 64 * np}, {"blob", l.o_blob, blob},
            {"win_of", l.o_winof, 4 * nc}, {"mask", l.o_mask, 8 * t * 16}, {"tile_count", l.o_tc, 4 * t}, {"tile_base", l.o_tb, 4 * t},
            {"rows", l.o_rows, 4 * t * 1024}, {"ba_sum", l.o_bs, 4 * t * nc}, {"ba_base", l.o_bb, 4 * t * nc}, {"ba_total", l.o_bt, 8 * nc}};
}
void check_sel_invariants(const SelLayout& l, size_t nc, size_t np, size_t blob) {
    const std::vector<Region> rs = regions(l, nc, np, blob);
    size_t end = 0;
    for (size_t i = 0; i < rs.size(); i++) {
        check(rs[i].off % 256 == 0, "%s at %zu is not 256-aligned", rs[i].name, rs[i].off);
        check(rs[i].off >= end, "%s at %zu begins below the end %zu of the region before it", rs[i].name, rs[i].off, end);
        end = rs[i].off + rs[i].bytes;
    }
    EQ(l.total, end);
    check(l.o_up % 256 == 0, "o_up %zu", l.o_up);
    check(l.o_head + 24 <= l.o_up && l.o_sc + 104 * nc <= l.o_up, "head / DevSelChunk[] reach into the uploaded part");
    for (int i = 2; i <= 4; i++)
        check(rs[size_t(i)].off >= l.o_up && rs[size_t(i)].off + rs[size_t(i)].bytes <= l.up_end, "%s outside [o_up, up_end)", rs[size_t(i)].name);
    check(l.o_mask >= l.up_end, "mask begins inside the uploaded part");
    EQ(l.win_of.size(), nc);
}

BatchPlan flat_plan(int nc, int64_t entries) {
    BatchPlan p;
    p.n_chunks = nc;
    p.chunks.assign(size_t(nc), DevChunk{});
    for (DevChunk& ck : p.chunks) { ck.ptype = PF_INT32; ck.width = 4; ck.num_entries = entries; }
    return p;
}
FilterPlan preds_on(std::vector<int> chunks, size_t blob) {
    FilterPlan f;
    for (int c : chunks) { DevPred d{}; d.chunk = c; d.op = 1 + c; f.preds.push_back(d); }
    f.blob.assign(blob, 0);
    for (size_t i = 0; i < blob; i++) f.blob[i] = uint8_t(0xa0 + i);
    return f;
}

void test_filter_layout() {
    g_case = "layout_filter: 3 chunks, 2 predicates, blob 5, 3000 rows";
    {
        const BatchPlan p = flat_plan(3, 3000);
        const FilterPlan f = preds_on({1, 2}, 5);
        const std::vector<DevWin> wins = {DevWin{2, 0, 7, -1}};
        const SelLayout l = layout_filter(p, f, wins);
        EQ(l.rows_cap, 3000); EQ(l.tiles, 3); EQ(l.grid, 3);
        EQ(l.o_head, 0); EQ(l.o_sc, 256);            // 3 * 104 = 312 -> ends at 568
        EQ(l.o_up, 768); EQ(l.o_preds, 768);         // 128 -> 896
        EQ(l.o_blob, 1024); EQ(l.o_winof, 1280); EQ(l.up_end, 1292);
        EQ(l.o_mask, 1536);                          // 3 * 16 words = 384 -> 1920
        EQ(l.o_tc, 2048); EQ(l.o_tb, 2304);
        EQ(l.o_rows, 2560);                          // 3 * 4096 = 12288 -> 14848
        EQ(l.o_bs, 14848); EQ(l.o_bb, 15104);        // 36 each
        EQ(l.o_bt, 15360); EQ(l.total, 15384);
        EQ(l.win_of[0], -1); EQ(l.win_of[1], -1); EQ(l.win_of[2], 0);
        check_sel_invariants(l, 3, 2, 5);

        std::vector<uint8_t> h(l.up_end, 0xee);
        fill_filter(l, f, h.data());
        for (size_t i = 0; i < l.o_up; i++) if (h[i]) { check(false, "mirror byte %zu below o_up is not zero", i); break; }
        check(std::memcmp(h.data() + l.o_preds, f.preds.data(), 128) == 0, "predicates in the mirror");
        check(std::memcmp(h.data() + l.o_blob, f.blob.data(), 5) == 0, "blob in the mirror");
        const int32_t wo[3] = {-1, -1, 0};
        check(std::memcmp(h.data() + l.o_winof, wo, 12) == 0, "win_of in the mirror");
        EQ(h[l.o_preds + 128], 0); EQ(h[l.o_blob + 5], 0);   // the padding is cleared

        const SelBufs s = bind_sel(l, f, SEL);
        PEQ(s.head, at(SEL)); PEQ(s.sc, at(SEL + 256)); PEQ(s.preds, at(SEL + 768)); PEQ(s.blob, at(SEL + 1024));
        PEQ(s.win_of, at(SEL + 1280)); PEQ(s.mask, at(SEL + 1536)); PEQ(s.tile_count, at(SEL + 2048));
        PEQ(s.tile_base, at(SEL + 2304)); PEQ(s.rows, at(SEL + 2560)); PEQ(s.ba_sum, at(SEL + 14848));
        PEQ(s.ba_base, at(SEL + 15104)); PEQ(s.ba_total, at(SEL + 15360));
        EQ(s.rows_cap, 3000); EQ(s.tiles_cap, 3); EQ(s.n_preds, 2);
    }
    g_case = "layout_filter: rows_cap from the first predicate chunk's window";
    {
        const BatchPlan p = flat_plan(2, 3000);
        const FilterPlan f = preds_on({1, 0}, 0);   // the first predicate is on chunk 1
        struct { int64_t take; int64_t cap; } cs[] = {{-1, 3000}, {0, 0}, {100, 100}, {2999, 2999}, {3000, 3000}, {5000, 3000}};
        for (auto c : cs) {
            const SelLayout l = layout_filter(p, f, {DevWin{1, 0, 3, c.take}});
            check(l.rows_cap == c.cap, "take %lld: rows_cap %lld, expected %lld", (long long)c.take, (long long)l.rows_cap, (long long)c.cap);
            EQ(l.win_of[0], -1); EQ(l.win_of[1], 0);
            check_sel_invariants(l, 2, 2, 0);
        }
        EQ(layout_filter(p, f, {DevWin{0, 0, 3, 10}}).rows_cap, 3000);   // a window on another chunk does not bound it
        EQ(layout_filter(p, f, {}).rows_cap, 3000);
    }
    g_case = "layout_filter: tiles and grid";
    {
        const FilterPlan f = preds_on({0}, 3);
        struct { int64_t rows; size_t tiles; int grid; } cs[] = {{0, 1, 1}, {1, 1, 1}, {1024, 1, 1}, {1025, 2, 2},
                                                                 {256 * 1024, 256, 256}, {256 * 1024 + 1, 257, 256}};
        for (auto c : cs) {
            const SelLayout l = layout_filter(flat_plan(1, c.rows), f, {});
            check(l.rows_cap == c.rows && l.tiles == c.tiles && l.grid == c.grid, "rows %lld: rows_cap %lld tiles %zu grid %d",
                  (long long)c.rows, (long long)l.rows_cap, l.tiles, l.grid);
            check_sel_invariants(l, 1, 1, 3);
            EQ(l.o_rows + 4 * 1024 * c.tiles, l.o_bs);   // (4096 bytes per tile: the next region follows at once)
        }
    }
    g_case = "layout_filter: empty blob";
    {
        const BatchPlan p = flat_plan(2, 10);
        const FilterPlan f = preds_on({0}, 0);
        const SelLayout l = layout_filter(p, f, {});
        EQ(l.o_preds, 512); EQ(l.o_blob, 768); EQ(l.o_winof, 768); EQ(l.up_end, 776);
        check_sel_invariants(l, 2, 1, 0);
        std::vector<uint8_t> h(l.up_end, 0xee);
        fill_filter(l, f, h.data());
        const int32_t wo[2] = {-1, -1};
        check(std::memcmp(h.data() + l.o_winof, wo, 8) == 0, "win_of in the mirror");
    }
}

// ---------------------------------------------------------------- arena_needs, arenas_grow, chars_overflow
void test_decisions() {
    g_case = "arena_needs";
    BatchPlan p;
    p.out_bytes = 1000; p.bits_bytes = 0; p.chars_hint = 100;
    ArenaNeeds n = arena_needs(p, 0, false);
    EQ(n.out, 1000); EQ(n.bits, 1); EQ(n.chars, 200 + (16 << 20));
    n = arena_needs(p, 0, true);
    EQ(n.bits, 9);
    p.bits_bytes = 77;
    EQ(arena_needs(p, 0, false).bits, 77); EQ(arena_needs(p, 0, true).bits, 85);
    EQ(arena_needs(p, 1ull << 30, false).chars, 1ull << 30);           // a rerun's exact need above the hint
    EQ(arena_needs(p, 1000, false).chars, 200 + (16 << 20));           // ... and below it
    p.out_bytes = 0;
    EQ(arena_needs(p, 0, false).out, 0);

    g_case = "arenas_grow";
    const ArenaNeeds need{1000, 85, 5000};
    check(!arenas_grow(need, ArenaCaps{1000, 85, 5000, 0, 0, 0}, false), "exact capacities, no twins: no growth");
    check(arenas_grow(need, ArenaCaps{999, 85, 5000, 0, 0, 0}, false), "out one byte short");
    check(arenas_grow(need, ArenaCaps{1000, 84, 5000, 0, 0, 0}, false), "bits one byte short");
    check(arenas_grow(need, ArenaCaps{1000, 85, 4999, 0, 0, 0}, false), "chars one byte short");
    check(!arenas_grow(need, ArenaCaps{2000, 90, 6000, 2000, 90, 6000}, true), "twins as large as their arenas");
    check(arenas_grow(need, ArenaCaps{2000, 90, 6000, 1999, 90, 6000}, true), "twin out below its arena");
    check(arenas_grow(need, ArenaCaps{2000, 90, 6000, 2000, 89, 6000}, true), "twin bits below its arena");
    check(arenas_grow(need, ArenaCaps{2000, 90, 6000, 2000, 90, 5999}, true), "twin chars below its arena");
    check(!arenas_grow(need, ArenaCaps{2000, 90, 6000, 0, 0, 0}, false), "small twins do not matter to a batch without them");

    g_case = "chars_overflow";
    BatchPlan q;
    q.n_chunks = 3;
    q.chunks.assign(3, DevChunk{});
    q.chunks[0].ptype = PF_INT32; q.chunks[1].ptype = PF_BYTE_ARRAY; q.chunks[2].ptype = PF_BYTE_ARRAY;
    auto res = [](int64_t a, int sa, int64_t b, int sb, int64_t c, int sc) {
        std::vector<DevChunkResult> r(3, DevChunkResult{});
        r[0].num_chars = a; r[0].status = sa; r[1].num_chars = b; r[1].status = sb; r[2].num_chars = c; r[2].status = sc;
        return r;
    };
    CharsOverflow o = chars_overflow(q, res(5000, PF_ERR_CAPACITY, 1, 0, 300, 0).data());
    check(!o.rerun, "a capacity status on an INT32 chunk asks for no rerun"); EQ(o.need, 256 + 512);
    o = chars_overflow(q, res(0, 0, 1, PF_ERR_CAPACITY, 300, 0).data());
    check(o.rerun, "a capacity status on a BYTE_ARRAY chunk"); EQ(o.need, 768);
    o = chars_overflow(q, res(0, 0, 0x7fffffff, PF_ERR_CAPACITY, 0, 0).data());
    check(o.rerun, "num_chars 0x7fffffff still reruns"); EQ(o.need, 0x80000000ll);
    o = chars_overflow(q, res(0, 0, 0x80000000ll, PF_ERR_CAPACITY, 0, 0).data());
    check(!o.rerun, "num_chars 0x80000000 does not"); EQ(o.need, 0x80000000ll);
    o = chars_overflow(q, res(0, 0, -5, PF_ERR_CAPACITY, 257, 0).data());
    check(o.rerun, "negative num_chars"); EQ(o.need, 512);   // -5 counts as 0
    o = chars_overflow(q, res(0, 0, 10, PF_ERR_CORRUPT_PAGE, 10, 0).data());
    check(!o.rerun, "another status asks for no rerun"); EQ(o.need, 512);
    BatchPlan e;
    o = chars_overflow(e, nullptr);
    check(!o.rerun, "no chunks"); EQ(o.need, 0);
}

// ---------------------------------------------------------------- assemble_info
// Chunk c of a hand-made batch: 0 INT32 with validity and def levels, 1 BYTE_ARRAY, 2 INT64 without validity.
struct Batch {
    BatchPlan p;
    std::vector<DevChunkResult> r;
    std::vector<DevChunk> dc;
    explicit Batch(int n) {
        p.n_chunks = n;
        p.chunks.assign(size_t(n), DevChunk{});
        r.assign(size_t(n), DevChunkResult{});
        dc.assign(size_t(n), DevChunk{});
        for (int c = 0; c < n; c++) {
            DevChunk& k = p.chunks[size_t(c)];
            const uintptr_t o = OUT + 0x1000u * unsigned(c), b = BITS + 0x100u * unsigned(c);
            k.num_entries = 100 + c;
            if (c == 0) { k.ptype = PF_INT32; k.width = 4; k.values = at(o); k.validity = at(b); k.def_levels = at(o + 0x800); }
            if (c == 1) { k.ptype = PF_BYTE_ARRAY; k.width = 0; k.offsets = at<int32_t>(o); k.validity = at(b); }
            if (c == 2) { k.ptype = PF_INT64; k.width = 8; k.values = at(o); }
            k.chars = at(0xdead00);   // (the host's copy: never reported; the device-written copy is)
            dc[size_t(c)].chars = c == 1 ? at(CHARS + 0x400) : nullptr;
            r[size_t(c)] = DevChunkResult{10 + c, 9 + c, 8 + c, 1000 + c, 0, -1};
        }
    }
};
// the decode's view of chunk c of a Batch, written out
pf_column_info decode_view(int c) {
    pf_column_info e{};
    e.num_entries = 100 + c; e.num_slots = 10 + c; e.num_values = 9 + c; e.num_rows = 8 + c;
    e.num_chars = c == 1 ? 1001 : 0;
    e.width = c == 0 ? 4 : c == 1 ? 0 : 8;
    const uintptr_t o = OUT + 0x1000u * unsigned(c), b = BITS + 0x100u * unsigned(c);
    if (c == 0) { e.d_values = at(o); e.d_validity = at(b); e.d_def_levels = at(o + 0x800); }
    if (c == 1) { e.d_offsets = at<int32_t>(o); e.d_validity = at(b); e.d_chars = at(CHARS + 0x400); }
    if (c == 2) { e.d_values = at(o); }
    return e;
}
DevWinRes win_res(int c) {
    DevWinRes w{};
    w.n_entries = 50 + c; w.n_slots = 40 + c; w.n_values = 30 + c; w.n_rows = 20 + c; w.n_chars = 500 + c;
    w.chars_dst = c == 1 ? at(WCHARS + 0x40) : nullptr;
    return w;
}
// the window's view of chunk c: the counts of win_res(c), the pointers at the same offsets in the twins
pf_column_info window_view(int c) {
    pf_column_info e{};
    e.num_entries = 50 + c; e.num_slots = 40 + c; e.num_values = 30 + c; e.num_rows = 20 + c;
    e.num_chars = c == 1 ? 501 : 0;
    e.width = c == 0 ? 4 : c == 1 ? 0 : 8;
    const uintptr_t o = WOUT + 0x1000u * unsigned(c), b = WBITS + 0x100u * unsigned(c);
    if (c == 0) { e.d_values = at(o); e.d_validity = at(b); e.d_def_levels = at(o + 0x800); }
    if (c == 1) { e.d_offsets = at<int32_t>(o); e.d_validity = at(b); e.d_chars = at(WCHARS + 0x40); }
    if (c == 2) { e.d_values = at(o); }
    return e;
}
void expect_info(const pf_column_info& g, const pf_column_info& e, int c) {
    const std::string keep = g_case;
    g_case += " chunk " + std::to_string(c);
    EQ(g.num_entries, e.num_entries); EQ(g.num_slots, e.num_slots); EQ(g.num_values, e.num_values); EQ(g.num_rows, e.num_rows);
    EQ(g.num_chars, e.num_chars); EQ(g.width, e.width); EQ(g.status, e.status);
    PEQ(g.d_values, e.d_values); PEQ(g.d_validity, e.d_validity); PEQ(g.d_offsets, e.d_offsets); PEQ(g.d_chars, e.d_chars);
    PEQ(g.d_list_offsets, e.d_list_offsets); PEQ(g.d_list_validity, e.d_list_validity);
    PEQ(g.d_def_levels, e.d_def_levels); PEQ(g.d_rep_levels, e.d_rep_levels);
    g_case = keep;
}
const TwinDelta TWIN{int64_t(WOUT) - int64_t(OUT), int64_t(WBITS) - int64_t(BITS)};
const pf_selection_info SENTINEL{-11, -12, at<const int32_t>(0x5e00), -13};
bool untouched(const pf_selection_info& s) {
    return s.rows_in == -11 && s.rows_selected == -12 && s.d_rows == SENTINEL.d_rows && s.status == -13;
}
BatchResults results_of(const Batch& b, const std::vector<DevWin>& wins, const std::vector<DevWinRes>& wres) {
    BatchResults br{};
    br.res = b.r.data(); br.dev_chunks = b.dc.data();
    br.wins = wins.data(); br.wres = wins.empty() ? nullptr : wres.data(); br.n_wins = wins.size();
    br.twin = TWIN;
    return br;
}

void test_assemble() {
    std::vector<DevWin> none;
    std::vector<DevWinRes> nores;
    g_case = "assemble: 0 chunks";
    {
        Batch b(0);
        pf_selection_info si = SENTINEL;
        DevSelHead sh{5, 4, 0, 0};
        BatchResults br = results_of(b, none, nores);
        FirstError fe = assemble_info(b.p, br, nullptr, &si);
        EQ(fe.code, PF_OK); check(fe.msg.empty(), "message '%s'", fe.msg.c_str());
        br.sel_head = &sh;   // a filter's head over no chunk: nothing is written
        fe = assemble_info(b.p, br, nullptr, &si);
        EQ(fe.code, PF_OK); check(untouched(si), "sel_info written for 0 chunks");
    }
    g_case = "assemble: 1 chunk";
    {
        Batch b(1);
        pf_column_info info[1];
        std::memset(info, 0x5a, sizeof info);   // (every field is written)
        pf_selection_info si = SENTINEL;
        FirstError fe = assemble_info(b.p, results_of(b, none, nores), info, &si);
        EQ(fe.code, PF_OK);
        expect_info(info[0], decode_view(0), 0);   // num_chars 0: the result's 1000 is not reported for INT32
        check(untouched(si), "sel_info written without a filter");
    }
    // windows on no chunk, the first, the last, all
    const std::vector<std::vector<int>> sets = {{}, {0}, {2}, {0, 1, 2}, {1}};
    for (const std::vector<int>& set : sets) {
        g_case = "assemble: 3 chunks, windows on {";
        for (int c : set) g_case += std::to_string(c);
        g_case += "}";
        Batch b(3);
        std::vector<DevWin> wins;
        std::vector<DevWinRes> wres;
        for (int c : set) { wins.push_back(DevWin{c, 0, 1, 2}); wres.push_back(win_res(c)); }
        pf_column_info info[3];
        std::memset(info, 0x5a, sizeof info);
        pf_selection_info si = SENTINEL;
        FirstError fe = assemble_info(b.p, results_of(b, wins, wres), info, &si);
        EQ(fe.code, PF_OK); check(fe.msg.empty(), "message '%s'", fe.msg.c_str());
        for (int c = 0; c < 3; c++) {
            bool in_set = false;
            for (int x : set) in_set |= x == c;
            expect_info(info[c], in_set ? window_view(c) : decode_view(c), c);
        }
        // (null pointers stayed null through the shift: chunk 2 has no validity, chunk 1 no values, none has lists)
        PEQ(info[2].d_validity, nullptr); PEQ(info[1].d_values, nullptr); PEQ(info[0].d_list_offsets, nullptr);
        PEQ(info[0].d_rep_levels, nullptr); PEQ(info[0].d_chars, nullptr);
        check(untouched(si), "sel_info written without a filter");
    }
    g_case = "assemble: identity window";
    {
        Batch b(3);
        std::vector<DevWin> wins = {DevWin{0, 0, 0, 1000}, DevWin{1, 0, 0, 1000}};
        std::vector<DevWinRes> wres = {win_res(0), win_res(1)};
        wres[1].identity = 1;
        pf_column_info info[3];
        FirstError fe = assemble_info(b.p, results_of(b, wins, wres), info, nullptr);
        EQ(fe.code, PF_OK);
        expect_info(info[0], window_view(0), 0);
        expect_info(info[1], decode_view(1), 1);   // counts and pointers stay the decode's
        expect_info(info[2], decode_view(2), 2);
    }
    g_case = "assemble: failed window under an OK decode";
    {
        Batch b(3);
        std::vector<DevWin> wins = {DevWin{1, 0, 0, 5}, DevWin{2, 0, 0, 5}};
        std::vector<DevWinRes> wres = {win_res(1), win_res(2)};
        wres[0].status = PF_ERR_INVALID_ARG;
        pf_column_info info[3];
        FirstError fe = assemble_info(b.p, results_of(b, wins, wres), info, nullptr);
        EQ(fe.code, PF_ERR_INVALID_ARG);
        check(fe.msg == "chunk 1: decode failed (status -1, page -1)", "message '%s'", fe.msg.c_str());
        pf_column_info e = decode_view(1);   // the view stays the decode's, the status is the window's
        e.status = PF_ERR_INVALID_ARG;
        expect_info(info[0], decode_view(0), 0);
        expect_info(info[1], e, 1);
        expect_info(info[2], window_view(2), 2);
    }
    g_case = "assemble: failed decode over an OK window";
    {
        Batch b(3);
        b.r[0].status = PF_ERR_CORRUPT_PAGE; b.r[0].err_page = 3;
        std::vector<DevWin> wins = {DevWin{0, 0, 0, 5}};
        std::vector<DevWinRes> wres = {win_res(0)};
        wres[0].status = PF_ERR_UNSUPPORTED_TYPE;   // (the decode's status stands even over a failed window)
        pf_column_info info[3];
        FirstError fe = assemble_info(b.p, results_of(b, wins, wres), info, nullptr);
        EQ(fe.code, PF_ERR_CORRUPT_PAGE);
        check(fe.msg == "chunk 0: decode failed (status -2, page 3)", "message '%s'", fe.msg.c_str());
        pf_column_info e = decode_view(0);
        e.status = PF_ERR_CORRUPT_PAGE;
        expect_info(info[0], e, 0);
        wres[0].status = 0;   // ... and over an OK one: still the decode's view
        fe = assemble_info(b.p, results_of(b, wins, wres), info, nullptr);
        EQ(fe.code, PF_ERR_CORRUPT_PAGE);
        expect_info(info[0], e, 0);
        expect_info(info[1], decode_view(1), 1);
    }
    g_case = "assemble: selection over windows";
    {
        Batch b(3);
        std::vector<DevWin> wins = {DevWin{0, 0, 0, 5}, DevWin{1, 0, 0, 5}};
        std::vector<DevWinRes> wres = {win_res(0), win_res(1)};
        DevSelHead sh{45, 7, 0, 0};
        std::vector<DevSelChunk> sc(3, DevSelChunk{});
        for (int c = 0; c < 3; c++) {
            sc[size_t(c)].o_values = c == 1 ? nullptr : at(OUT + 0x9000u + 0x100u * unsigned(c));
            sc[size_t(c)].o_validity = c == 2 ? nullptr : at(BITS + 0x900u + 0x10u * unsigned(c));
            sc[size_t(c)].o_offsets = c == 1 ? at<int32_t>(OUT + 0xa000u) : nullptr;
            sc[size_t(c)].o_chars = c == 1 ? at(CHARS + 0x7000u) : nullptr;
            sc[size_t(c)].n_values = 6 - c; sc[size_t(c)].n_chars = 60 + c;
        }
        sc[1].status = PF_ERR_UNSUPPORTED_TYPE;   // a selection status over chunk 1's OK window view
        BatchResults br = results_of(b, wins, wres);
        br.sel_head = &sh; br.sel_chunks = sc.data(); br.sel_rows = at<const int32_t>(SEL + 2560);
        pf_column_info info[3];
        pf_selection_info si = SENTINEL;
        FirstError fe = assemble_info(b.p, br, info, &si);
        EQ(fe.code, PF_ERR_UNSUPPORTED_TYPE);
        check(fe.msg == "chunk 1: decode failed (status -7, page -1)", "message '%s'", fe.msg.c_str());
        EQ(si.rows_in, 45); EQ(si.rows_selected, 7); PEQ(si.d_rows, at(SEL + 2560)); EQ(si.status, 0);
        // chunk 0: the selection's counts and arrays; the levels keep the window's (twin) address
        pf_column_info e0{};
        e0.num_entries = e0.num_slots = e0.num_rows = 7; e0.num_values = 6; e0.num_chars = 0; e0.width = 4;
        e0.d_values = at(OUT + 0x9000u); e0.d_validity = at(BITS + 0x900u); e0.d_def_levels = at(WOUT + 0x800);
        expect_info(info[0], e0, 0);
        pf_column_info e1 = window_view(1);   // the window's view with the selection's status
        e1.status = PF_ERR_UNSUPPORTED_TYPE;
        expect_info(info[1], e1, 1);
        pf_column_info e2{};                  // no window: the selection over the decode's view
        e2.num_entries = e2.num_slots = e2.num_rows = 7; e2.num_values = 4; e2.num_chars = 0; e2.width = 8;
        e2.d_values = at(OUT + 0x9200u);
        expect_info(info[2], e2, 2);

        sc[1].status = 0;                     // BYTE_ARRAY: the selection's chars are reported
        sh.status = PF_ERR_INVALID_ARG;       // (the head's status goes to sel_info as it is)
        si = SENTINEL;
        fe = assemble_info(b.p, br, info, &si);
        EQ(fe.code, PF_OK);
        EQ(si.status, PF_ERR_INVALID_ARG); EQ(si.rows_selected, 7);
        pf_column_info s1{};
        s1.num_entries = s1.num_slots = s1.num_rows = 7; s1.num_values = 5; s1.num_chars = 61; s1.width = 0;
        s1.d_validity = at(BITS + 0x910u); s1.d_offsets = at<int32_t>(OUT + 0xa000u); s1.d_chars = at(CHARS + 0x7000u);
        expect_info(info[1], s1, 1);

        b.r[2].status = PF_ERR_CORRUPT_PAGE; b.r[2].err_page = 9;   // a failed decode under the selection: its status and view stand
        fe = assemble_info(b.p, br, info, &si);
        EQ(fe.code, PF_ERR_CORRUPT_PAGE);
        pf_column_info d2 = decode_view(2);
        d2.status = PF_ERR_CORRUPT_PAGE;
        expect_info(info[2], d2, 2);
    }
    g_case = "assemble: selection over one chunk";
    {
        Batch b(1);
        DevSelHead sh{100, 0, 0, 0};
        DevSelChunk sc{};
        BatchResults br = results_of(b, none, nores);
        br.sel_head = &sh; br.sel_chunks = &sc; br.sel_rows = at<const int32_t>(SEL);
        pf_column_info info[1];
        pf_selection_info si = SENTINEL;
        FirstError fe = assemble_info(b.p, br, info, &si);
        EQ(fe.code, PF_OK);
        EQ(si.rows_in, 100); EQ(si.rows_selected, 0); PEQ(si.d_rows, at(SEL)); EQ(si.status, 0);
        pf_column_info e{};
        e.width = 4; e.d_def_levels = at(OUT + 0x800);
        expect_info(info[0], e, 0);
    }
    g_case = "assemble: chunks 1 and 2 both fail";
    {
        Batch b(3);
        b.r[1].status = PF_ERR_CORRUPT_PAGE; b.r[1].err_page = 5;
        b.r[2].status = PF_ERR_UNSUPPORTED_ENCODING; b.r[2].err_page = 7;
        pf_column_info info[3];
        FirstError fe = assemble_info(b.p, results_of(b, none, nores), info, nullptr);
        EQ(fe.code, PF_ERR_CORRUPT_PAGE);
        check(fe.msg == "chunk 1: decode failed (status -2, page 5)", "message '%s'", fe.msg.c_str());
        EQ(info[0].status, 0); EQ(info[1].status, PF_ERR_CORRUPT_PAGE); EQ(info[2].status, PF_ERR_UNSUPPORTED_ENCODING);
    }
}

// ---------------------------------------------------------------- batch_layout, rebase, copy_items
void test_batch_copy() {
    BatchPlan p;
    p.out_bytes = 1000; p.bits_bytes = 77;
    const ArenaPtrs arenas{at(OUT), at(BITS), at(CHARS)};
    uint8_t* const host = at(0x10000000);
    g_case = "batch_layout: no BYTE_ARRAY chunk";
    {
        std::vector<pf_column_info> info(2, pf_column_info{});
        info[1].d_chars = at(CHARS + 64);   // (a chars pointer with no chars counts for nothing)
        const BatchLayout b = batch_layout(p, info, at(CHARS));
        EQ(b.out, 1000); EQ(b.bits_off, 1024); EQ(b.bits, 77); EQ(b.chars_off, 1280); EQ(b.chars, 0); EQ(b.total, 1280);
        const BatchLayout b0 = batch_layout(p, {}, at(CHARS));
        EQ(b0.total, 1280); EQ(b0.chars, 0);
    }
    g_case = "batch_layout: two BYTE_ARRAY chunks in reverse order";
    {
        std::vector<pf_column_info> info(3, pf_column_info{});
        info[0].d_chars = at(CHARS + 512); info[0].num_chars = 100;
        info[2].d_chars = at(CHARS); info[2].num_chars = 300;
        BatchLayout b = batch_layout(p, info, at(CHARS));
        EQ(b.chars, 612);             // the used extent: the chunk placed last ends it
        EQ(b.total, 1280 + 768);      // the order-independent bound 256 + 512 is the larger
        info[0].d_chars = at(CHARS + 1024);
        b = batch_layout(p, info, at(CHARS));
        EQ(b.chars, 1124); EQ(b.total, 1280 + 1124);   // the extent is the larger

        g_case = "rebase";
        PEQ(rebase(b, arenas, host, nullptr), nullptr);
        PEQ(rebase(b, arenas, host, at(OUT)), host);
        PEQ(rebase(b, arenas, host, at(OUT + 999)), host + 999);
        PEQ(rebase(b, arenas, host, at(OUT + 1000)), host + 1000);       // exactly at the arena's end: still maps
        PEQ(rebase(b, arenas, host, at(OUT + 1001)), nullptr);
        PEQ(rebase(b, arenas, host, at(OUT - 1)), nullptr);
        PEQ(rebase(b, arenas, host, at(BITS)), host + 1024);
        PEQ(rebase(b, arenas, host, at(BITS + 77)), host + 1024 + 77);
        PEQ(rebase(b, arenas, host, at(BITS + 78)), nullptr);
        PEQ(rebase(b, arenas, host, at(CHARS + 1024)), host + 1280 + 1024);
        PEQ(rebase(b, arenas, host, at(CHARS + 1124)), host + 1280 + 1124);
        PEQ(rebase(b, arenas, host, at(CHARS + 1125)), nullptr);
        PEQ(rebase(b, arenas, host, at(WOUT + 8)), nullptr);             // outside every arena
        PEQ(rebase(b, arenas, host, at(0x1234)), nullptr);

        pf_column_info ci{};
        ci.num_entries = 1; ci.num_slots = 2; ci.num_values = 3; ci.num_rows = 4; ci.num_chars = 100; ci.width = 0; ci.status = 0;
        ci.d_validity = at(BITS + 16); ci.d_offsets = at<int32_t>(OUT + 64); ci.d_chars = at(CHARS + 1024);
        ci.d_list_offsets = at<int32_t>(OUT + 128); ci.d_list_validity = at(BITS + 32);
        ci.d_def_levels = at(OUT + 256); ci.d_rep_levels = at(WOUT + 256);   // (one pointer that lies in no arena)
        pf_column_info e = ci;
        e.d_values = nullptr; e.d_validity = host + 1024 + 16; e.d_offsets = reinterpret_cast<int32_t*>(host + 64);
        e.d_chars = host + 1280 + 1024; e.d_list_offsets = reinterpret_cast<int32_t*>(host + 128);
        e.d_list_validity = host + 1024 + 32; e.d_def_levels = host + 256; e.d_rep_levels = nullptr;
        g_case = "rebase_info";
        expect_info(rebase_info(b, arenas, host, ci), e, 0);
    }
    g_case = "copy_items";
    {
        pf_column_info ci{};
        ci.num_entries = 21; ci.num_slots = 13; ci.num_rows = 5; ci.num_chars = 99; ci.width = 4;
        ci.d_values = at(OUT); ci.d_validity = at(BITS); ci.d_chars = at(CHARS);
        ci.d_list_validity = at(BITS + 64); ci.d_def_levels = at(OUT + 512); ci.d_rep_levels = at(OUT + 768);
        pf_column_out o{};
        uint8_t buf[8];
        o.values = buf; o.values_cap = 1; o.validity = buf + 1; o.validity_cap = 2; o.offsets = reinterpret_cast<int32_t*>(buf + 4);
        o.offsets_cap = 3; o.chars_cap = 4; o.list_offsets_cap = 5; o.list_validity = buf + 2; o.list_validity_cap = 6;
        o.def_levels = buf + 3; o.def_levels_cap = 7; o.rep_levels_cap = 8;
        CopyItem it[8];
        copy_items(ci, o, it);
        const size_t n_absent[8] = {52, 2, 0, 99, 0, 1, 21, 21};   // 13 * 4; (13 + 7) / 8; no offsets; chars; no lists; (5 + 7) / 8
        const void* src[8] = {at(OUT), at(BITS), nullptr, at(CHARS), nullptr, at(BITS + 64), at(OUT + 512), at(OUT + 768)};
        const void* dst[8] = {buf, buf + 1, buf + 4, nullptr, nullptr, buf + 2, buf + 3, nullptr};
        const bool wanted[8] = {true, true, false, false, false, true, true, false};
        for (int k = 0; k < 8; k++) {
            check(it[k].n == n_absent[k], "item %d: n %zu, expected %zu", k, it[k].n, n_absent[k]);
            check(it[k].cap == size_t(k + 1), "item %d: cap %zu", k, it[k].cap);
            PEQ(it[k].src, src[k]); PEQ(it[k].dst, dst[k]);
            check(it[k].wanted() == wanted[k], "item %d: wanted", k);
        }
        ci.d_offsets = at<int32_t>(OUT + 1024); ci.d_list_offsets = at<int32_t>(OUT + 2048);
        copy_items(ci, o, it);
        EQ(it[2].n, 56); EQ(it[4].n, 24);   // 4 * (13 + 1), 4 * (5 + 1)
        ci.num_slots = 16; ci.num_rows = 0;
        copy_items(ci, o, it);
        EQ(it[1].n, 2); EQ(it[5].n, 0); EQ(it[2].n, 68); EQ(it[4].n, 4);
        ci.num_slots = 17;
        copy_items(ci, o, it);
        EQ(it[1].n, 3);
    }
}

}  // namespace

int main() {
    test_layouts();
    test_filter_layout();
    test_decisions();
    test_assemble();
    test_batch_copy();
    std::printf("checks %ld failures %d\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
