// pf_dict_filter_check — the host side of windows and predicates over kept dictionaries (csrc/pf_plan.cpp,
// csrc/pf_result.cpp, csrc/pf_pred.h; pf_decode_row_group_dict_filter), without a GPU: hand-made descriptors, made-up
// addresses. Built by tests/test_dict_filter_plan_cpu.py with g++ under AddressSanitizer + UBSan.
//  * identity of plans: with keep == NULL, or with no RANGE predicate on a kept chunk, the filter plan and
//    layout_filter are field for field those of a batch without the feature; the batch plan does not depend on windows
//    or predicates at all (plan_batch never sees them);
//  * bitmap regions: word counts and offsets at 0, 1, 63, 64, 65, 256, 257, 65536 and 65537 entries; the regions
//    overlap neither each other nor any other region of the stage's buffer; 8 predicates on 8 kept chunks fit;
//  * views: the index width reaches the window's and the selection's view in assemble_info for widths 1, 2 and 4;
//  * errors: plan_filter's call errors are what they are whatever the keep flags; RANGE on INT96 / FLBA is
//    PF_ERR_UNSUPPORTED_TYPE;
//  * entry matching: pred_range_at over dictionary entries against a brute-force loop, every RANGE-able type.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "pf_plan.h"
#include "pf_pred.h"
#include "pf_result.h"

using namespace pf;

namespace {
int g_fail = 0;
void check(bool ok, const char* fmt, ...) {
    if (ok) return;
    g_fail++;
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}

struct Chunk {
    pf_chunk_desc d{};
    std::vector<pf_page_desc> pages;
};
pf_page_desc page(int type, int enc, int nv, uint32_t bytes) {
    pf_page_desc d{};
    d.page_type = type; d.encoding = enc; d.def_encoding = PF_ENC_RLE; d.rep_encoding = PF_ENC_RLE;
    d.num_values = nv; d.compressed_size = bytes; d.uncompressed_size = bytes; d.num_nulls = -1; d.is_compressed = 1;
    return d;
}
// A chunk of `rows` rows: dictionary-encoded over n_dict entries (n_dict < 0: PLAIN, no dictionary).
Chunk make_chunk(int ptype, int max_def, int n_dict, int rows, int type_length = 0) {
    Chunk c;
    c.d.physical_type = ptype; c.d.max_def = max_def; c.d.codec = PF_CODEC_UNCOMPRESSED; c.d.type_length = type_length;
    const int w = type_width(ptype, type_length);
    if (n_dict >= 0) {
        c.pages.push_back(page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, n_dict, uint32_t(n_dict) * uint32_t(w > 0 ? w : 9)));
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_RLE_DICTIONARY, rows, uint32_t(rows) * 4 + 8));
    } else {
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, rows, uint32_t(rows) * uint32_t(w > 0 ? w : 9) + 8));
    }
    return c;
}
std::vector<pf_chunk_desc> layout(std::vector<Chunk>& cs, size_t& n_bytes) {
    std::vector<pf_chunk_desc> out;
    uint64_t off = 0;
    for (Chunk& c : cs) {
        uint64_t in = 0;
        for (pf_page_desc& pd : c.pages) { pd.offset = in + 40; in = pd.offset + pd.compressed_size; }
        c.d.n_pages = int(c.pages.size());
        c.d.pages = c.pages.data();
        c.d.chunk_offset = off;
        c.d.chunk_size = in;
        off += align_up(in, 256);
        out.push_back(c.d);
    }
    n_bytes = off;
    return out;
}

pf_predicate range(int chunk, const void* lo, int nlo, const void* hi, int nhi) {
    pf_predicate q{};
    q.chunk = chunk; q.op = PF_PRED_RANGE;
    q.lo = static_cast<const uint8_t*>(lo); q.lo_len = nlo;
    q.hi = static_cast<const uint8_t*>(hi); q.hi_len = nhi;
    return q;
}
pf_predicate null_pred(int chunk, int op) {
    pf_predicate q{};
    q.chunk = chunk; q.op = op;
    return q;
}

bool same_layout(const SelLayout& a, const SelLayout& b) {
    return a.o_head == b.o_head && a.o_sc == b.o_sc && a.o_up == b.o_up && a.o_preds == b.o_preds && a.o_blob == b.o_blob &&
           a.o_winof == b.o_winof && a.up_end == b.up_end && a.o_mask == b.o_mask && a.o_tc == b.o_tc && a.o_tb == b.o_tb &&
           a.o_rows == b.o_rows && a.o_bs == b.o_bs && a.o_bb == b.o_bb && a.o_bt == b.o_bt && a.total == b.total &&
           a.rows_cap == b.rows_cap && a.tiles == b.tiles && a.grid == b.grid && a.win_of == b.win_of;
}
bool same_preds(const FilterPlan& a, const FilterPlan& b) {
    return a.preds.size() == b.preds.size() && a.blob == b.blob &&
           (a.preds.empty() || std::memcmp(a.preds.data(), b.preds.data(), sizeof(DevPred) * a.preds.size()) == 0);
}

struct Region {
    size_t off, len;
    const char* what;
};

// ---- identity of plans ------------------------------------------------------------------------------------------------
void identity() {
    std::vector<Chunk> cs = {make_chunk(PF_INT32, 1, 300, 5000), make_chunk(PF_BYTE_ARRAY, 0, 7, 5000), make_chunk(PF_INT64, 0, -1, 5000),
                             make_chunk(PF_INT96, 1, 5, 5000)};
    size_t n_bytes = 0;
    const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
    const int32_t lo = 5;
    const std::vector<pf_predicate> on_kept = {range(0, &lo, 4, nullptr, 0), range(1, "ab", 2, "abc", 3)};
    const std::vector<pf_predicate> off_kept = {null_pred(0, PF_PRED_IS_NULL), null_pred(3, PF_PRED_NOT_NULL), range(2, nullptr, 0, nullptr, 0)};
    const std::vector<DevWin> wins = {DevWin{0, 0, 10, 100}, DevWin{1, 0, 10, 100}};
    const uint8_t all[4] = {1, 1, 1, 1}, none[4] = {0, 0, 0, 0};
    BatchPlan plain, kept, zero;
    plan_batch(cds.data(), 4, n_bytes, PfOpts{}, plain, nullptr);
    plan_batch(cds.data(), 4, n_bytes, PfOpts{}, kept, all);
    plan_batch(cds.data(), 4, n_bytes, PfOpts{}, zero, none);
    check(kept.keeps.size() == 3 && kept.keep_of[2] == -1, "identity: 3 of 4 chunks kept (%zu)", kept.keeps.size());
    const char* why = nullptr;
    for (const auto* ps : {&on_kept, &off_kept}) {
        FilterPlan base, f;
        check(plan_filter(cds.data(), 4, ps->data(), int(ps->size()), base, &why) == PF_OK, "identity: plan_filter: %s", why);
        check(plan_filter(cds.data(), 4, ps->data(), int(ps->size()), f, &why) == PF_OK, "identity: plan_filter: %s", why);
        const SelLayout l0 = layout_filter(plain, base, wins);
        // keep == NULL, keep all zero
        for (const BatchPlan* p : {&plain, &zero}) {
            plan_filter_dict(*p, f);
            check(f.dicts.empty() && f.dict_of.empty() && f.dict_words == 0 && same_preds(f, base), "identity: no keep flags, no records");
            const SelLayout l = layout_filter(*p, f, wins);
            check(same_layout(l, l0) && l.o_drec == 0 && l.o_dof == 0 && l.o_dbits == 0 && l.dict_tiles == 0,
                  "identity: the layout without keep flags");
            const SelDictBufs b = bind_sel_dict(l, f, 0x1000, nullptr, nullptr);
            check(b.n_recs == 0 && !b.recs && !b.dict_of && !b.bits && !b.keeps && !b.keep_of, "identity: nothing bound");
        }
        // keep flags set
        plan_filter_dict(kept, f);
        check(same_preds(f, base), "identity: DevPred and the blob do not change with keep flags");
        const SelLayout lk = layout_filter(kept, f, wins);
        if (ps == &off_kept) {
            check(f.dicts.empty() && f.dict_of.empty(), "identity: IS_NULL / NOT_NULL / a predicate on an expanded chunk get no record");
            // (rows_cap comes from the plan's entries, which keep flags do not change)
            check(same_layout(lk, l0) && lk.o_dbits == 0, "identity: the layout with no predicate on a kept chunk");
        } else {
            check(f.dicts.size() == 2 && f.dict_of.size() == 2 && f.dict_of[0] == 0 && f.dict_of[1] == 1, "identity: two records");
            check(lk.o_head == l0.o_head && lk.o_sc == l0.o_sc && lk.o_up == l0.o_up && lk.o_preds == l0.o_preds &&
                  lk.o_blob == l0.o_blob && lk.o_winof == l0.o_winof && lk.rows_cap == l0.rows_cap && lk.tiles == l0.tiles && lk.grid == l0.grid,
                  "identity: the existing tables lie where they lay");
            check(lk.o_drec >= lk.o_winof + 4 * 4 && lk.o_dof >= lk.o_drec + 2 * sizeof(DevSelDict) && lk.up_end >= lk.o_dof + 4 * 2,
                  "identity: the records lie behind win_of inside the uploaded part");
        }
    }
    // no windows and no predicates: the batch plan is that of plan_batch(..., keep) -- it takes neither
    BatchPlan again;
    plan_batch(cds.data(), 4, n_bytes, PfOpts{}, again, all);
    check(again.out_bytes == kept.out_bytes && again.bits_bytes == kept.bits_bytes && again.scratch_bytes == kept.scratch_bytes &&
          again.keep_of == kept.keep_of && again.lists[L_IDS] == kept.lists[L_IDS] && again.meta_bytes == kept.meta_bytes,
          "identity: the batch plan");
}

// ---- bitmap regions ---------------------------------------------------------------------------------------------------
void bitmaps() {
    const int sizes[] = {0, 1, 63, 64, 65, 256, 257, 65536};
    std::vector<Chunk> cs;
    for (int n : sizes) cs.push_back(make_chunk(PF_INT32, 1, n, 3000));
    size_t n_bytes = 0;
    const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
    std::vector<pf_predicate> ps;
    for (int c = 0; c < 8; c++) ps.push_back(range(c, nullptr, 0, nullptr, 0));
    const uint8_t all[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    BatchPlan p;
    plan_batch(cds.data(), 8, n_bytes, PfOpts{}, p, all);
    FilterPlan f;
    const char* why = nullptr;
    check(plan_filter(cds.data(), 8, ps.data(), 8, f, &why) == PF_OK, "bitmaps: plan_filter: %s", why);
    plan_filter_dict(p, f);
    check(f.dicts.size() == 8, "bitmaps: 8 predicates on 8 kept chunks fit (%zu)", f.dicts.size());
    uint64_t at = 0;
    for (size_t i = 0; i < f.dicts.size(); i++) {
        const DevSelDict& r = f.dicts[i];
        const uint64_t want = (uint64_t(sizes[i]) + 63) / 64;
        check(r.pred == int(i) && r.keep == p.keep_of[i] && r.n_entries == sizes[i], "bitmaps: record %zu names its predicate and dictionary", i);
        check(r.n_words == want && r.word_off == at, "bitmaps: %d entries: %llu words at %llu, expected %llu at %llu", sizes[i],
              (unsigned long long)r.n_words, (unsigned long long)r.word_off, (unsigned long long)want, (unsigned long long)at);
        at += want;
    }
    check(f.dict_words == at && f.dict_max_entries == 65536, "bitmaps: %llu words in all", (unsigned long long)f.dict_words);
    const std::vector<DevWin> no_wins;
    const SelLayout l = layout_filter(p, f, no_wins);
    check(l.dict_tiles == int(65536 / SELD_TILE), "bitmaps: %d entry tiles", l.dict_tiles);
    const size_t nc = 8, tiles = l.tiles;
    const std::vector<Region> rs = {{l.o_head, sizeof(DevSelHead), "head"}, {l.o_sc, sizeof(DevSelChunk) * nc, "sc"},
                                    {l.o_preds, sizeof(DevPred) * 8, "preds"}, {l.o_winof, 4 * nc, "win_of"},
                                    {l.o_drec, sizeof(DevSelDict) * 8, "records"}, {l.o_dof, 4 * 8, "dict_of"},
                                    {l.o_mask, 8 * tiles * (SEL_TILE / 64), "mask"}, {l.o_tc, 4 * tiles, "tile_count"},
                                    {l.o_tb, 4 * tiles, "tile_base"}, {l.o_rows, 4 * tiles * SEL_TILE, "rows"},
                                    {l.o_bs, 4 * tiles * nc, "ba_sum"}, {l.o_bb, 4 * tiles * nc, "ba_base"}, {l.o_bt, 8 * nc, "ba_total"}};
    std::vector<Region> all_r = rs;
    for (const DevSelDict& r : f.dicts) all_r.push_back({l.o_dbits + 8 * size_t(r.word_off), 8 * size_t(r.n_words), "bitmap"});
    for (size_t a = 0; a < all_r.size(); a++) {
        check(all_r[a].off + all_r[a].len <= l.total, "bitmaps: region %s outside the buffer", all_r[a].what);
        check(all_r[a].off % 8 == 0, "bitmaps: region %s misaligned", all_r[a].what);
        for (size_t b = a + 1; b < all_r.size(); b++)
            check(!all_r[a].len || !all_r[b].len || all_r[a].off + all_r[a].len <= all_r[b].off || all_r[b].off + all_r[b].len <= all_r[a].off,
                  "bitmaps: regions %zu (%s) and %zu (%s) overlap", a, all_r[a].what, b, all_r[b].what);
    }
    check(l.o_drec >= l.o_up && l.o_dof + 4 * 8 <= l.up_end && l.o_dbits >= l.up_end, "bitmaps: records go up, bitmaps stay on the device");
    // the upload mirror holds the records
    std::vector<uint8_t> h(l.up_end, 0xee);
    fill_filter(l, f, h.data());
    check(std::memcmp(h.data() + l.o_drec, f.dicts.data(), sizeof(DevSelDict) * 8) == 0 &&
          std::memcmp(h.data() + l.o_dof, f.dict_of.data(), 4 * 8) == 0, "bitmaps: fill_filter writes the records and dict_of");
    const DevKeep* keeps = reinterpret_cast<const DevKeep*>(uintptr_t(0x7000));
    const int32_t* keep_of = reinterpret_cast<const int32_t*>(uintptr_t(0x8000));
    const SelDictBufs b = bind_sel_dict(l, f, 0x100000, keeps, keep_of);
    check(b.n_recs == 8 && uintptr_t(b.recs) == 0x100000 + l.o_drec && uintptr_t(b.dict_of) == 0x100000 + l.o_dof &&
          uintptr_t(b.bits) == 0x100000 + l.o_dbits && b.keeps == keeps && b.keep_of == keep_of && b.tiles == l.dict_tiles, "bitmaps: bind_sel_dict");
    // 65537 entries: index width 4, 1025 words, 257 tiles; two predicates on the same chunk get a bitmap each
    std::vector<Chunk> one = {make_chunk(PF_DOUBLE, 0, 65537, 3000), make_chunk(PF_INT32, 0, -1, 3000)};
    const std::vector<pf_chunk_desc> cd1 = layout(one, n_bytes);
    const std::vector<pf_predicate> p1 = {range(0, nullptr, 0, nullptr, 0), range(1, nullptr, 0, nullptr, 0), range(0, nullptr, 0, nullptr, 0),
                                          null_pred(0, PF_PRED_NOT_NULL)};
    const uint8_t k1[2] = {1, 1};
    BatchPlan bp;
    plan_batch(cd1.data(), 2, n_bytes, PfOpts{}, bp, k1);
    FilterPlan f1;
    check(plan_filter(cd1.data(), 2, p1.data(), 4, f1, &why) == PF_OK, "bitmaps: plan_filter: %s", why);
    plan_filter_dict(bp, f1);
    check(bp.keeps.size() == 1 && bp.keeps[0].index_width == 4, "bitmaps: 65537 entries take 4-byte indices");
    check(f1.dicts.size() == 2 && f1.dict_of == std::vector<int32_t>({0, -1, 1, -1}), "bitmaps: kept and expanded predicates mixed");
    check(f1.dicts[0].n_words == 1025 && f1.dicts[1].word_off == 1025 && f1.dict_words == 2050, "bitmaps: 65537 entries are 1025 words");
    check(layout_filter(bp, f1, no_wins).dict_tiles == 257, "bitmaps: 65537 entries are 257 tiles");
}

// ---- views --------------------------------------------------------------------------------------------------------------
void views() {
    const int dict_n[3] = {200, 300, 70000};
    for (int k = 0; k < 3; k++) {
        for (int ptype : {PF_BYTE_ARRAY, PF_INT64}) {
            std::vector<Chunk> cs = {make_chunk(ptype, 1, dict_n[k], 4000)};
            size_t n_bytes = 0;
            const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
            const uint8_t keep[1] = {1};
            BatchPlan p;
            plan_batch(cds.data(), 1, n_bytes, PfOpts{}, p, keep);
            bind_batch(p, ArenaBases{0x10000000100ull, 0x20000000100ull, 0x30000000100ull, 0x40000000100ull, 0x50000000100ull, 0x60000000100ull});
            const int iw = 1 << k;
            DevChunkResult res{4000, 3000, 4000, 1234, 0, -1};   // (num_chars: the dictionary's, for the rerun's need)
            DevChunk dev = p.chunks[0];
            DevKeep dk = p.dkeeps[0];
            dk.d_chars = reinterpret_cast<uint8_t*>(uintptr_t(0x70000000));
            dk.num_chars = 1234;
            const DevWin win{0, 0, 10, 100};
            DevWinRes wr{};
            wr.e0 = 10; wr.n_entries = 100; wr.s0 = 10; wr.n_slots = 100; wr.n_values = 80; wr.n_rows = 100;
            BatchResults br{};
            br.res = &res; br.dev_chunks = &dev; br.wins = &win; br.wres = &wr; br.n_wins = 1; br.twin = TwinDelta{0x1000000, 0x2000000};
            br.keeps = &dk;
            pf_column_info ci{};
            pf_dict_info di{};
            pf_selection_info si{};
            assemble_info(p, br, &ci, &si, &di);
            check(ci.width == iw && ci.num_chars == 0 && !ci.d_offsets && !ci.d_chars && ci.num_slots == 100 && ci.num_values == 80 &&
                  ci.d_values == p.chunks[0].values + 0x1000000 && ci.d_validity == p.chunks[0].validity + 0x2000000,
                  "views: the window's view of a kept chunk, index width %d (got %d)", iw, ci.width);
            check(di.kept == 1 && di.index_width == iw && di.n_entries == dict_n[k] && di.d_values == dk.d_values && di.d_offsets == dk.d_offsets,
                  "views: the dictionary does not move under a window");
            DevSelHead head{100, 37, 0, 0};
            DevSelChunk sc{};
            sc.o_values = p.chunks[0].values; sc.o_validity = p.chunks[0].validity; sc.n_values = 30; sc.n_chars = 999;
            sc.o_offsets = reinterpret_cast<int32_t*>(uintptr_t(0x9000)); sc.o_chars = reinterpret_cast<uint8_t*>(uintptr_t(0xa000));
            br.sel_head = &head; br.sel_chunks = &sc; br.sel_rows = nullptr;
            assemble_info(p, br, &ci, &si, &di);
            check(ci.width == iw && ci.num_chars == 0 && !ci.d_offsets && !ci.d_chars && ci.num_slots == 37 && ci.num_rows == 37 &&
                  ci.num_entries == 37 && ci.num_values == 30 && ci.d_values == p.chunks[0].values,
                  "views: the selection's view of a kept chunk, index width %d", iw);
            check(di.kept == 1 && di.n_entries == dict_n[k] && (ptype != PF_BYTE_ARRAY || (di.num_chars == 1234 && di.d_chars == dk.d_chars)),
                  "views: the dictionary does not move under a filter");
        }
    }
}

// ---- errors -------------------------------------------------------------------------------------------------------------
void errors() {
    std::vector<Chunk> cs = {make_chunk(PF_INT96, 1, 5, 100), make_chunk(PF_FIXED_LEN_BYTE_ARRAY, 1, 5, 100, 16), make_chunk(PF_INT32, 0, 9, 100)};
    size_t n_bytes = 0;
    const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
    const uint8_t keep[3] = {1, 1, 1};
    BatchPlan p;
    plan_batch(cds.data(), 3, n_bytes, PfOpts{}, p, keep);
    check(p.keeps.size() == 3, "errors: INT96 and FLBA chunks are kept");
    FilterPlan f;
    const char* why = nullptr;
    const int32_t v = 1;
    const std::vector<uint8_t> big(PRED_BOUND_MAX + 1, 'x');
    struct Case { pf_predicate q; int n; int want; const char* what; };
    const std::vector<Case> bad = {
        {range(0, nullptr, 0, nullptr, 0), 1, PF_ERR_UNSUPPORTED_TYPE, "RANGE on INT96"},
        {range(1, nullptr, 0, nullptr, 0), 1, PF_ERR_UNSUPPORTED_TYPE, "RANGE on FLBA"},
        {range(3, nullptr, 0, nullptr, 0), 1, PF_ERR_INVALID_ARG, "chunk out of range"},
        {range(2, &v, 3, nullptr, 0), 1, PF_ERR_INVALID_ARG, "a bound of the wrong width"},
        {range(2, nullptr, 0, nullptr, 0), PF_MAX_PREDICATES + 1, PF_ERR_INVALID_ARG, "too many predicates"},
    };
    for (const Case& c : bad) {
        std::vector<pf_predicate> ps(size_t(c.n), c.q);
        const int rc = plan_filter(cds.data(), 3, ps.data(), c.n, f, &why);
        check(rc == c.want && f.preds.empty() && f.dicts.empty() && f.dict_of.empty() && f.dict_words == 0, "errors: %s gives %d (%s)", c.what, rc, why);
    }
    const std::vector<pf_predicate> ok = {null_pred(0, PF_PRED_IS_NULL), null_pred(1, PF_PRED_NOT_NULL), range(2, &v, 4, nullptr, 0)};
    check(plan_filter(cds.data(), 3, ok.data(), 3, f, &why) == PF_OK, "errors: IS_NULL / NOT_NULL stay legal on kept INT96 / FLBA: %s", why);
    plan_filter_dict(p, f);
    check(f.dicts.size() == 1 && f.dict_of == std::vector<int32_t>({-1, -1, 0}), "errors: only the RANGE gets a record");
    // a failed plan_filter after a good one leaves nothing of the records behind
    std::vector<pf_predicate> again(1, bad[0].q);
    plan_filter(cds.data(), 3, again.data(), 1, f, &why);
    check(f.dicts.empty() && f.dict_of.empty() && f.dict_words == 0 && f.dict_max_entries == 0, "errors: the records are cleared with the predicates");
}

// ---- entry matching -----------------------------------------------------------------------------------------------------
template <class T>
DevPred pred_of(int ptype, const T* lo, const T* hi) {
    DevPred d{};
    d.op = PF_PRED_RANGE; d.ptype = ptype;
    // (as plan_filter packs them: integers in lo_i / hi_i, reals widened in lo_f / hi_f)
    if (lo) { d.flags |= PRED_HAS_LO; if constexpr (std::is_integral<T>::value) d.lo_i = int64_t(*lo); else d.lo_f = double(*lo); }
    if (hi) { d.flags |= PRED_HAS_HI; if constexpr (std::is_integral<T>::value) d.hi_i = int64_t(*hi); else d.hi_f = double(*hi); }
    return d;
}
template <class T>
void match_fixed(int ptype, const std::vector<T>& entries, const std::vector<T>& bounds, const char* name) {
    int n = 0;
    for (int a = -1; a < int(bounds.size()); a++)
        for (int b = -1; b < int(bounds.size()); b++) {
            const T* lo = a < 0 ? nullptr : &bounds[size_t(a)];
            const T* hi = b < 0 ? nullptr : &bounds[size_t(b)];
            const DevPred d = pred_of<T>(ptype, lo, hi);
            for (size_t e = 0; e < entries.size(); e++) {
                const bool got = pred_range_at(d, reinterpret_cast<const uint8_t*>(entries.data()), nullptr, nullptr, int64_t(e), nullptr);
                const T v = entries[e];
                const bool want = (!lo || *lo <= v) && (!hi || v <= *hi);   // (IEEE comparisons: NaN fails, -0.0 == +0.0)
                check(got == want, "entry matching: %s entry %zu, bounds %d / %d: %d, expected %d", name, e, a, b, int(got), int(want));
                n++;
            }
        }
    std::printf("entry matching: %s, %d comparisons\n", name, n);
}
void matching() {
    const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
    const double dnan = std::numeric_limits<double>::quiet_NaN(), dinf = std::numeric_limits<double>::infinity();
    match_fixed<int32_t>(PF_INT32, {INT32_MIN, -1, 0, 1, INT32_MAX, 7}, {INT32_MIN, -1, 0, INT32_MAX, 8}, "INT32");
    match_fixed<int64_t>(PF_INT64, {INT64_MIN, -1, 0, 1, INT64_MAX, int64_t(1) << 31}, {INT64_MIN, 0, INT64_MAX, int64_t(1) << 31}, "INT64");
    match_fixed<float>(PF_FLOAT, {fnan, -fnan, -0.0f, 0.0f, finf, -finf, 1.5f, -1.5f, 3.4e38f}, {fnan, -0.0f, 0.0f, finf, -finf, 1.5f}, "FLOAT");
    match_fixed<double>(PF_DOUBLE, {dnan, -dnan, -0.0, 0.0, dinf, -dinf, 1.5, -1.5, 1e308}, {dnan, -0.0, 0.0, dinf, -dinf, 1.5}, "DOUBLE");
    // BYTE_ARRAY: the empty string, prefixes and extensions of the bounds, duplicates, bytes above 0x7f, a 4096-byte bound
    const std::vector<std::string> entries = {"", "a", "ab", "abc", "ab", std::string("ab\0", 3), "\xff", std::string(1, '\0'),
                                              std::string(4095, 'e'), std::string(4096, 'e'), std::string(5000, 'e'), "b"};
    const std::vector<std::string> bounds = {"", "ab", "abc", "\xff", std::string(4096, 'e'), std::string(1, '\0')};
    std::vector<int32_t> offs = {0};
    std::string chars;
    for (const std::string& s : entries) { chars += s; offs.push_back(int32_t(chars.size())); }
    int n = 0;
    for (int a = -1; a < int(bounds.size()); a++)
        for (int b = -1; b < int(bounds.size()); b++) {
            std::string blob;
            DevPred d{};
            d.op = PF_PRED_RANGE; d.ptype = PF_BYTE_ARRAY;
            if (a >= 0) { d.flags |= PRED_HAS_LO; d.lo_off = uint32_t(blob.size()); d.lo_len = uint32_t(bounds[size_t(a)].size()); blob += bounds[size_t(a)]; }
            if (b >= 0) { d.flags |= PRED_HAS_HI; d.hi_off = uint32_t(blob.size()); d.hi_len = uint32_t(bounds[size_t(b)].size()); blob += bounds[size_t(b)]; }
            blob += "pad";   // (so that an empty blob still has an address)
            for (size_t e = 0; e < entries.size(); e++) {
                const bool got = pred_range_at(d, nullptr, offs.data(), reinterpret_cast<const uint8_t*>(chars.data()), int64_t(e),
                                               reinterpret_cast<const uint8_t*>(blob.data()));
                auto less_eq = [](const std::string& x, const std::string& y) {   // unsigned bytewise, a proper prefix first
                    return std::lexicographical_compare(x.begin(), x.end(), y.begin(), y.end(),
                                                        [](char p, char q) { return uint8_t(p) < uint8_t(q); }) || x == y;
                };
                const bool want = (a < 0 || less_eq(bounds[size_t(a)], entries[e])) && (b < 0 || less_eq(entries[e], bounds[size_t(b)]));
                check(got == want, "entry matching: BYTE_ARRAY entry %zu, bounds %d / %d: %d, expected %d", e, a, b, int(got), int(want));
                n++;
            }
        }
    std::printf("entry matching: BYTE_ARRAY, %d comparisons\n", n);
}

}  // namespace

int main() {
    identity();
    bitmaps();
    views();
    errors();
    matching();
    std::printf("pf_dict_filter_check: failures %d\n", g_fail);
    return g_fail ? 1 : 0;
}
