// pf_dict_plan_check — the host planner (csrc/pf_plan.cpp) on kept-dictionary chunks (pf_decode_row_group_dict),
// without a GPU: hand-made descriptors, bound to made-up arena addresses. Built by tests/test_dict_plan_cpu.py with
// g++ under AddressSanitizer + UBSan.
//  * the eligibility rule case by case: each ineligible reason alone, a PLAIN page first, in the middle and last, a
//    dictionary page with no data page, PLAIN_DICTIONARY pages;
//  * index widths at 0, 1, 256, 257, 65536 and 65537 dictionary entries;
//  * the arena sizes of a kept chunk against the formula;
//  * no kept page on a list that would expand it, no unkept page on L_IDS, L_IDS = ceil(entries / FBLK) blocks a page;
//  * keep == NULL and keep all zero plan exactly as plan_batch without the parameter;
//  * the regions in scratch and in out never overlap and lie inside their arenas.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_plan.h"

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

const ArenaBases BASES{0x10000000100ull, 0x20000000100ull, 0x30000000100ull, 0x40000000100ull, 0x50000000100ull, 0x60000000100ull};

struct Chunk {
    pf_chunk_desc d{};
    std::vector<pf_page_desc> pages;
};
Chunk chunk(int ptype, int max_def, int codec = PF_CODEC_UNCOMPRESSED, int type_length = 0) {
    Chunk c;
    c.d.physical_type = ptype; c.d.max_def = max_def; c.d.codec = codec; c.d.type_length = type_length;
    return c;
}
pf_page_desc page(int type, int enc, int nv, uint32_t comp, uint32_t uncomp) {
    pf_page_desc d{};
    d.page_type = type; d.encoding = enc; d.def_encoding = PF_ENC_RLE; d.rep_encoding = PF_ENC_RLE;
    d.num_values = nv; d.compressed_size = comp; d.uncompressed_size = uncomp; d.num_nulls = -1; d.is_compressed = 1;
    return d;
}
pf_page_desc dict_page(int n, uint32_t bytes) { return page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, n, bytes, bytes); }
pf_page_desc data_page(int enc, int nv) { return page(PF_PAGE_DATA, enc, nv, uint32_t(nv) * 2 + 8, uint32_t(nv) * 2 + 8); }

// A dictionary chunk: n_dict entries of `ptype`, data pages of the given encodings and entry counts.
Chunk dict_chunk(int ptype, int max_def, int n_dict, const std::vector<int>& encs, const std::vector<int>& counts, int type_length = 0,
                 int codec = PF_CODEC_UNCOMPRESSED) {
    Chunk c = chunk(ptype, max_def, codec, type_length);
    const int w = type_width(ptype, type_length);
    c.pages.push_back(dict_page(n_dict, uint32_t(n_dict) * uint32_t(w > 0 ? w : 9)));
    for (size_t i = 0; i < encs.size(); i++) c.pages.push_back(data_page(encs[i], counts[i]));
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
void plan(std::vector<Chunk>& cs, const uint8_t* keep, BatchPlan& p, size_t& n_bytes, bool bind = true) {
    const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
    plan_batch(cds.data(), int(cds.size()), n_bytes, PfOpts{}, p, keep);
    if (bind) bind_batch(p, BASES);
}

struct Region {
    uint64_t off, len;
    const char* what;
};
void disjoint(const std::vector<Region>& rs, uint64_t arena, const char* name, const char* which) {
    for (size_t a = 0; a < rs.size(); a++) {
        check(rs[a].off + rs[a].len <= arena, "%s: %s region %zu (%s) outside the arena", name, which, a, rs[a].what);
        for (size_t b = a + 1; b < rs.size(); b++)
            check(rs[a].off + rs[a].len <= rs[b].off || rs[b].off + rs[b].len <= rs[a].off || !rs[a].len || !rs[b].len,
                  "%s: %s regions %zu (%s) and %zu (%s) overlap", name, which, a, rs[a].what, b, rs[b].what);
    }
}

bool on_list(const BatchPlan& p, ListId l, int v) { return std::find(p.lists[l].begin(), p.lists[l].end(), v) != p.lists[l].end(); }
bool on_pairs(const BatchPlan& p, ListId l, int page) {
    for (size_t k = 0; k + 1 < p.lists[l].size(); k += 2)
        if (p.lists[l][k] == page) return true;
    return false;
}

// Every invariant of a plan with kept chunks.
void check_plan(const BatchPlan& p, const char* name) {
    check(p.keep_of.size() == size_t(p.n_chunks), "%s: keep_of has %zu entries", name, p.keep_of.size());
    // regions
    std::vector<Region> sc, out, bits;
    for (size_t i = 0; i < p.pages.size(); i++) {
        const DevPage& pg = p.pages[i];
        const PagePlan& pp = p.pplan[i];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        const bool kept = p.keep_of[size_t(pg.chunk)] >= 0;
        if (pp.scratch_off != NO_OFF) sc.push_back(Region{pp.scratch_off, pg.body_len, "body"});
        if (pp.rt_off != NO_OFF) sc.push_back(Region{pp.rt_off, RT_BYTES, "run table"});
        if (pp.lt_off != NO_OFF) sc.push_back(Region{pp.lt_off, lvl_table_bytes(pg.num_values), "level table"});
        if (pp.aux_off != NO_OFF) {
            const uint64_t n = (pg.flags & PG_DICT) ? 8ull * (uint64_t(pg.num_values) + 1)
                                                    : (ck.ptype == PF_BYTE_ARRAY ? aux_chars_bytes(uint64_t(pg.num_values)) : 8ull * pg.num_values + 8);
            sc.push_back(Region{pp.aux_off, n, "aux"});
        }
        if (pg.flags & PG_DICT) continue;
        // lists
        if (kept) {
            check(pp.rt_off != NO_OFF && on_list(p, L_RUNS, int(i)), "%s: kept page %zu has no run table", name, i);
            check(pp.aux_off == NO_OFF, "%s: kept page %zu has aux words", name, i);
            check(!on_list(p, L_COUNT, int(i)) && !on_list(p, L_DECODE, int(i)) && !on_list(p, L_DELTA, int(i)) &&
                      !on_list(p, L_DLEN, int(i)) && !on_list(p, L_NEST, int(i)),
                  "%s: kept page %zu is on a page list that expands it", name, i);
            check(!on_pairs(p, L_FLAT, int(i)) && !on_pairs(p, L_CDICT, int(i)) && !on_pairs(p, L_NSEG, int(i)),
                  "%s: kept page %zu is on a block list that expands it", name, i);
            check((pp.lt_off != NO_OFF) == (ck.max_def > 0), "%s: kept page %zu: level table", name, i);
            check((pp.lt_off != NO_OFF) == on_list(p, L_LVL, int(i)), "%s: kept page %zu: L_LVL", name, i);
        } else {
            check(!on_pairs(p, L_IDS, int(i)), "%s: page %zu of a chunk that is not kept is on L_IDS", name, i);
            check(on_list(p, L_DECODE, int(i)), "%s: page %zu of a chunk that is not kept is not on L_DECODE", name, i);
        }
    }
    {   // L_IDS: per kept page its blocks 0 .. nb - 1, pages in order
        std::vector<int> want;
        for (size_t i = 0; i < p.pages.size(); i++) {
            const DevPage& pg = p.pages[i];
            if ((pg.flags & PG_DICT) || p.keep_of[size_t(pg.chunk)] < 0) continue;
            const int nb = std::max(1, int((int64_t(pg.num_values) + FBLK - 1) / FBLK));
            for (int b = 0; b < nb; b++) { want.push_back(int(i)); want.push_back(b); }
        }
        check(p.lists[L_IDS] == want, "%s: L_IDS is not the kept pages' blocks in order", name);
    }
    if (p.npub_bytes) sc.push_back(Region{p.off_npub, p.npub_bytes, "npub"});
    for (size_t b = 0; b < p.ba_bm.size(); b++)
        sc.push_back(Region{p.ba_bm[b], 4ull * (3ull * p.bajobs[b].n_tiles * (BA_TILE / 32) + p.bajobs[b].n_tiles), "ba bitmaps"});
    disjoint(sc, p.scratch_bytes, name, "scratch");
    size_t n_kept = 0;
    for (int c = 0; c < p.n_chunks; c++) {
        const DevChunk& ck = p.chunks[size_t(c)];
        const OutPlan& op = p.oplan[size_t(c)];
        const int k = p.keep_of[size_t(c)];
        const uint64_t e = uint64_t(ck.num_entries);
        if (k >= 0) {
            n_kept++;
            check(size_t(k) < p.keeps.size() && p.keeps[size_t(k)].chunk == c, "%s: keep_of[%d] points at another chunk", name, c);
            const KeepPlan& kp = p.keeps[size_t(k)];
            check(p.host_status[size_t(c)] == 0 && ck.needs_count == 0 && !on_list(p, L_SCAN, c), "%s: kept chunk %d is counted or failed", name, c);
            check(kp.index_width == dict_index_width(ck.dict_n) && kp.n_entries == ck.dict_n && kp.width == ck.width, "%s: chunk %d keep plan", name, c);
            check(op.values != NO_OFF && op.offsets == NO_OFF && op.list_offsets == NO_OFF && op.def == NO_OFF, "%s: kept chunk %d outputs", name, c);
            out.push_back(Region{op.values, e * uint64_t(kp.index_width), "indices"});
            check((kp.values != NO_OFF) == (ck.width > 0) && (kp.offsets != NO_OFF) == (ck.width == 0), "%s: chunk %d dictionary slot", name, c);
            if (kp.values != NO_OFF) out.push_back(Region{kp.values, uint64_t(kp.n_entries) * uint64_t(ck.width), "dictionary values"});
            if (kp.offsets != NO_OFF) out.push_back(Region{kp.offsets, 4ull * uint64_t(kp.n_entries + 1), "dictionary offsets"});
            check(kp.values == NO_OFF || kp.values % 256 == 0, "%s: chunk %d dictionary values not aligned", name, c);
            check(kp.offsets == NO_OFF || kp.offsets % 256 == 0, "%s: chunk %d dictionary offsets not aligned", name, c);
        } else {
            if (op.values != NO_OFF) out.push_back(Region{op.values, e * uint64_t(std::max(ck.width, 0)), "values"});
            if (op.offsets != NO_OFF) out.push_back(Region{op.offsets, 4 * (e + 1), "offsets"});
            if (op.list_offsets != NO_OFF) out.push_back(Region{op.list_offsets, 4 * (e + 1), "list offsets"});
            if (op.def != NO_OFF) out.push_back(Region{op.def, e, "def"});
            if (op.rep != NO_OFF) out.push_back(Region{op.rep, e, "rep"});
        }
        if (op.validity != NO_OFF) bits.push_back(Region{op.validity, (e + 7) / 8, "validity"});
        if (op.list_validity != NO_OFF) bits.push_back(Region{op.list_validity, (e + 7) / 8, "list validity"});
        check(op.values == NO_OFF || op.values % 256 == 0, "%s: chunk %d values not aligned", name, c);
    }
    check(n_kept == p.keeps.size(), "%s: %zu kept chunks, %zu keep plans", name, n_kept, p.keeps.size());
    disjoint(out, p.out_bytes, name, "out");
    disjoint(bits, p.bits_bytes, name, "bits");
    // metadata: the keep tables behind everything else, inside the block
    check(p.off_keeps % 256 == 0 && p.off_keeps >= p.off_ljobs + sizeof(Lz4Job) * p.ljobs.size(), "%s: keep table over the LZ4 jobs", name);
    check(p.off_keepof >= p.off_keeps + sizeof(DevKeep) * p.keeps.size(), "%s: keep_of over the keep table", name);
    check(p.off_keepof + (p.keeps.empty() ? 0 : 4 * size_t(p.n_chunks)) <= p.meta_bytes - 256, "%s: keep tables outside the metadata block", name);
    // bound pointers
    if (p.dkeeps.size() == p.keeps.size())
        for (size_t k = 0; k < p.keeps.size(); k++) {
            const KeepPlan& kp = p.keeps[k];
            const DevKeep& dk = p.dkeeps[k];
            const DevChunk& ck = p.chunks[size_t(kp.chunk)];
            check(dk.chunk == kp.chunk && dk.index_width == kp.index_width && dk.n_entries == kp.n_entries, "%s: DevKeep %zu", name, k);
            check(reinterpret_cast<uintptr_t>(ck.values) == BASES.out + p.oplan[size_t(kp.chunk)].values, "%s: kept chunk's indices pointer", name);
            check(ck.offsets == nullptr && ck.chars == nullptr, "%s: a kept chunk has offsets or chars", name);
            check(kp.values == NO_OFF ? dk.d_values == nullptr : reinterpret_cast<uintptr_t>(dk.d_values) == BASES.out + kp.values, "%s: d_values", name);
            check(kp.offsets == NO_OFF ? dk.d_offsets == nullptr : reinterpret_cast<uintptr_t>(dk.d_offsets) == BASES.out + kp.offsets, "%s: d_offsets", name);
            check(dk.d_chars == nullptr && dk.num_chars == 0, "%s: the device-written fields start zero", name);
        }
    else check(false, "%s: %zu DevKeep for %zu keep plans", name, p.dkeeps.size(), p.keeps.size());
}

// Two plans of the same descriptors, field by field (before binding: offsets only).
void same_plan(const BatchPlan& a, const BatchPlan& b, const char* name) {
    check(a.n_chunks == b.n_chunks && a.pages.size() == b.pages.size() && a.jobs.size() == b.jobs.size() && a.zjobs.size() == b.zjobs.size() &&
              a.ljobs.size() == b.ljobs.size() && a.bajobs.size() == b.bajobs.size() && a.ba_tiles.size() == b.ba_tiles.size(),
          "%s: table sizes", name);
    check(a.host_status == b.host_status, "%s: host_status", name);
    for (int l = 0; l < N_LISTS; l++) check(a.lists[l] == b.lists[l], "%s: list %d", name, l);
    check(std::memcmp(a.list_base, b.list_base, sizeof a.list_base) == 0, "%s: list_base", name);
    check(a.n_decode_first == b.n_decode_first && a.n_count_flat == b.n_count_flat && a.n_flat_fixed == b.n_flat_fixed &&
              a.n_flat_all == b.n_flat_all && a.n_null4 == b.n_null4 && a.n_null8 == b.n_null8 && a.n_ba_dict == b.n_ba_dict &&
              a.n_ba_dict_tiles == b.n_ba_dict_tiles && a.ba_short_dict == b.ba_short_dict && a.ba_short_data == b.ba_short_data &&
              a.max_nwin == b.max_nwin && a.max_dbp_nwin == b.max_dbp_nwin,
          "%s: grid lengths", name);
    check(a.null_caps.dcap == b.null_caps.dcap && a.null_caps.icap == b.null_caps.icap && a.null_caps.dlds == b.null_caps.dlds, "%s: null caps", name);
    check(a.scratch_bytes == b.scratch_bytes && a.out_bytes == b.out_bytes && a.bits_bytes == b.bits_bytes && a.off_npub == b.off_npub &&
              a.npub_bytes == b.npub_bytes && a.off_zlit == b.off_zlit && a.zlit_stride == b.zlit_stride && a.zstd_grid == b.zstd_grid &&
              a.chars_hint == b.chars_hint,
          "%s: arenas", name);
    check(a.off_chunks == b.off_chunks && a.off_pages == b.off_pages && a.off_jobs == b.off_jobs && a.off_lists == b.off_lists &&
              a.off_res == b.off_res && a.off_pieces == b.off_pieces && a.off_splits == b.off_splits && a.off_fallback == b.off_fallback &&
              a.off_wins == b.off_wins && a.off_bajobs == b.off_bajobs && a.off_batiles == b.off_batiles && a.off_nfbq == b.off_nfbq &&
              a.off_zjobs == b.off_zjobs && a.off_ljobs == b.off_ljobs && a.meta_bytes == b.meta_bytes,
          "%s: metadata layout", name);
    check(a.snap.tokmap_bytes == b.snap.tokmap_bytes && a.snap.n_splits == b.snap.n_splits && a.snap.wins.size() == b.snap.wins.size() &&
              a.snap.pieces.size() == b.snap.pieces.size(),
          "%s: Snappy tables", name);
    check(a.ba_bm == b.ba_bm, "%s: ba_bm", name);
    if (a.pages.size() != b.pages.size() || a.n_chunks != b.n_chunks) return;
    for (size_t i = 0; i < a.pages.size(); i++) {
        const PagePlan &x = a.pplan[i], &y = b.pplan[i];
        check(x.in_off == y.in_off && x.scratch_off == y.scratch_off && x.aux_off == y.aux_off && x.rt_off == y.rt_off && x.dx_off == y.dx_off &&
                  x.lt_off == y.lt_off && x.seg_off == y.seg_off && x.pub_off == y.pub_off && x.dbp_off == y.dbp_off && x.dbp_pub_off == y.dbp_pub_off,
              "%s: page %zu plan", name, i);
        const DevPage &g = a.pages[i], &h = b.pages[i];
        check(g.body_len == h.body_len && g.rep_len == h.rep_len && g.def_len == h.def_len && g.chunk == h.chunk && g.flags == h.flags &&
                  g.encoding == h.encoding && g.num_values == h.num_values && g.entry_start == h.entry_start && g.aux_cap == h.aux_cap &&
                  g.ba_job == h.ba_job && g.lvl_cap == h.lvl_cap && g.nseg == h.nseg && g.seg_len == h.seg_len && g.nwin == h.nwin &&
                  g.dbp_nwin == h.dbp_nwin && g.dbp_bcap == h.dbp_bcap,
              "%s: page %zu record", name, i);
    }
    for (int c = 0; c < a.n_chunks; c++) {
        const OutPlan &x = a.oplan[size_t(c)], &y = b.oplan[size_t(c)];
        check(x.values == y.values && x.validity == y.validity && x.offsets == y.offsets && x.list_offsets == y.list_offsets &&
                  x.list_validity == y.list_validity && x.def == y.def && x.rep == y.rep,
              "%s: chunk %d outputs", name, c);
        const DevChunk &g = a.chunks[size_t(c)], &h = b.chunks[size_t(c)];
        check(g.ptype == h.ptype && g.width == h.width && g.max_def == h.max_def && g.max_rep == h.max_rep && g.codec == h.codec &&
                  g.dict_page == h.dict_page && g.first_page == h.first_page && g.n_pages == h.n_pages && g.needs_count == h.needs_count &&
                  g.num_entries == h.num_entries && g.dict_n == h.dict_n,
              "%s: chunk %d record", name, c);
    }
}

const int RD = PF_ENC_RLE_DICTIONARY, PD = PF_ENC_PLAIN_DICTIONARY, PL = PF_ENC_PLAIN;

// One chunk planned alone with keep = 1: is it kept?
bool kept_alone(Chunk c, const char* name, long long want_status = 0) {
    std::vector<Chunk> cs{c};
    const uint8_t keep[1] = {1};
    BatchPlan p;
    size_t n = 0;
    plan(cs, keep, p, n);
    check(p.host_status[0] == want_status, "%s: status %lld", name, (long long)p.host_status[0]);
    check_plan(p, name);
    const bool rule = keep_eligible(cs[0].d);
    check((p.keep_of[0] >= 0) == (rule && p.host_status[0] == 0), "%s: the plan and keep_eligible disagree", name);
    return p.keep_of[0] >= 0;
}
}  // namespace

int main() {
    size_t n = 0;
    // ---- eligibility
    check(kept_alone(dict_chunk(PF_INT64, 1, 100, {RD, RD, RD}, {5000, 17, 9003}), "eligible"), "an eligible chunk is not kept");
    check(kept_alone(dict_chunk(PF_INT64, 0, 100, {PD, PD}, {5000, 17}), "PLAIN_DICTIONARY pages"), "PLAIN_DICTIONARY pages are not kept");
    check(kept_alone(dict_chunk(PF_INT32, 1, 7, {PD, RD}, {33, 4097}), "PLAIN_DICTIONARY then RLE_DICTIONARY"), "mixed dictionary encodings are not kept");
    check(kept_alone(dict_chunk(PF_BYTE_ARRAY, 1, 4, {RD}, {1}), "strings"), "a BYTE_ARRAY chunk is not kept");
    check(kept_alone(dict_chunk(PF_FIXED_LEN_BYTE_ARRAY, 0, 9, {RD}, {100}, 5), "FLBA(5)"), "an FLBA chunk is not kept");
    check(kept_alone(dict_chunk(PF_INT96, 0, 9, {RD}, {100}), "INT96"), "an INT96 chunk is not kept");
    {   // keep[i] == 0
        std::vector<Chunk> cs{dict_chunk(PF_INT64, 1, 100, {RD}, {5000})};
        const uint8_t keep[1] = {0};
        BatchPlan p;
        plan(cs, keep, p, n);
        check(p.keep_of[0] < 0 && p.keeps.empty() && p.lists[L_IDS].empty(), "keep = 0: kept");
        check_plan(p, "keep = 0");
    }
    {   // max_rep > 0
        Chunk c = dict_chunk(PF_INT64, 3, 100, {RD}, {5000});
        c.d.max_rep = 1; c.d.repeated_def = 2; c.d.list_null_def = 1;
        check(!kept_alone(c, "nested"), "a nested chunk is kept");
    }
    {   // BOOLEAN: no dictionary in any writer; with PLAIN pages it decodes as ever, with a dictionary page it fails as ever
        Chunk c = chunk(PF_BOOLEAN, 0);
        c.pages.push_back(data_page(PL, 1000));
        check(!kept_alone(c, "BOOLEAN"), "a BOOLEAN chunk is kept");
        Chunk d = dict_chunk(PF_BOOLEAN, 0, 2, {RD}, {1000});
        check(!kept_alone(d, "BOOLEAN with a dictionary page", PF_ERR_UNSUPPORTED_ENCODING), "a BOOLEAN chunk with a dictionary page is kept");
    }
    {   // no dictionary page
        Chunk c = chunk(PF_INT32, 0);
        c.pages.push_back(data_page(RD, 1000));
        check(!kept_alone(c, "no dictionary page"), "a chunk without a dictionary page is kept");
    }
    {   // a dictionary page and no data page
        Chunk c = chunk(PF_INT32, 0);
        c.pages.push_back(dict_page(10, 40));
        check(!kept_alone(c, "no data page"), "a chunk without a data page is kept");
    }
    check(!kept_alone(dict_chunk(PF_INT64, 1, 100, {PL, RD, RD}, {500, 17, 900}), "PLAIN first"), "PLAIN first: kept");
    check(!kept_alone(dict_chunk(PF_INT64, 1, 100, {RD, PL, RD}, {500, 17, 900}), "PLAIN in the middle"), "PLAIN in the middle: kept");
    check(!kept_alone(dict_chunk(PF_INT64, 1, 100, {RD, RD, PL}, {500, 17, 900}), "PLAIN last"), "PLAIN last: kept");
    check(!kept_alone(dict_chunk(PF_INT64, 0, 100, {RD, PF_ENC_DELTA_BINARY_PACKED}, {500, 17}), "DELTA page"), "a DELTA page: kept");
    check(!kept_alone(dict_chunk(PF_BYTE_ARRAY, 0, 100, {RD, PF_ENC_DELTA_BYTE_ARRAY}, {500, 17}), "DELTA_BYTE_ARRAY page"), "a DELTA_BYTE_ARRAY page: kept");
    {   // a chunk that fails validation is not kept and takes nothing with it
        Chunk bad = dict_chunk(PF_INT64, 1, 100, {RD}, {5000});
        bad.pages.push_back(page(PF_PAGE_DATA, RD, -5, 10, 10));
        std::vector<Chunk> cs{dict_chunk(PF_INT64, 1, 100, {RD}, {5000}), bad};
        const uint8_t keep[2] = {1, 1};
        BatchPlan p;
        plan(cs, keep, p, n);
        check(p.host_status[0] == 0 && p.host_status[1] == PF_ERR_CORRUPT_PAGE, "failed chunk: status");
        check(p.keep_of[0] == 0 && p.keep_of[1] < 0 && p.keeps.size() == 1, "failed chunk: kept");
        check_plan(p, "failed chunk");
    }
    // ---- index widths, arena sizes
    for (int nd : {0, 1, 256, 257, 65536, 65537}) {
        const int want = nd <= 256 ? 1 : (nd <= 65536 ? 2 : 4);
        check(dict_index_width(nd) == want, "dict_index_width(%d)", nd);
        for (int optional = 0; optional < 2; optional++) {
            const int64_t e = 5000 + 17 + 9003;
            std::vector<Chunk> cs{dict_chunk(PF_INT32, optional, nd, {RD, RD, RD}, {5000, 17, 9003})};
            const uint8_t keep[1] = {1};
            BatchPlan p, q;
            plan(cs, keep, p, n);
            plan(cs, nullptr, q, n);
            char name[64];
            std::snprintf(name, sizeof name, "width at %d entries, max_def %d", nd, optional);
            check(p.keep_of[0] == 0 && p.keeps.size() == 1 && p.keeps[0].index_width == want, "%s: index width", name);
            // out: the indices, then (256-byte aligned) the dictionary's values; bits: the validity words
            check(p.out_bytes == align_up(size_t(e) * size_t(want), 256) + size_t(nd) * 4, "%s: out arena %zu", name, p.out_bytes);
            check(q.out_bytes == size_t(e) * 4, "%s: expanding out arena %zu", name, q.out_bytes);
            check(p.bits_bytes == (optional ? align_up(size_t(e + 7) / 8, 4) : 0) && p.bits_bytes == q.bits_bytes, "%s: bits arena", name);
            check_plan(p, name);
            check_plan(q, name);
        }
    }
    {   // BYTE_ARRAY: indices + n + 1 offsets in out, no offsets of its own, no value positions in scratch
        const int64_t e = 33 + 4095 + 1;
        std::vector<Chunk> cs{dict_chunk(PF_BYTE_ARRAY, 1, 300, {RD, RD, RD}, {33, 4095, 1})};
        const uint8_t keep[1] = {1};
        BatchPlan p, q;
        plan(cs, keep, p, n);
        plan(cs, nullptr, q, n);
        check(p.keeps.size() == 1 && p.keeps[0].index_width == 2 && p.keeps[0].width == 0, "strings: keep plan");
        check(p.out_bytes == align_up(size_t(e) * 2, 256) + 4 * 301, "strings: out arena %zu", p.out_bytes);
        check(q.out_bytes == 4 * size_t(e + 1), "strings: expanding out arena %zu", q.out_bytes);
        check(p.chars_hint == cs[0].pages[0].uncompressed_size, "strings: only the dictionary's chars are hinted (%llu)", (unsigned long long)p.chars_hint);
        check(p.lists[L_SCAN].empty() && p.lists[L_COUNT].empty() && p.lists[L_CDICT].empty() && p.lists[L_FLAT].empty(), "strings: expanding lists");
        check(p.n_ba_dict == 1, "strings: the dictionary walk is still planned");
        check_plan(p, "strings");
    }
    // ---- keep == NULL and keep all zero are today's plan
    {
        Chunk nested = dict_chunk(PF_INT64, 3, 100, {RD}, {5000});
        nested.d.max_rep = 1; nested.d.repeated_def = 2; nested.d.list_null_def = 1;
        std::vector<Chunk> cs{dict_chunk(PF_INT64, 1, 100, {RD, RD}, {5000, 17}), dict_chunk(PF_BYTE_ARRAY, 1, 4, {RD, PL}, {9003, 100}),
                              dict_chunk(PF_INT32, 0, 70000, {RD}, {20000}, 0, PF_CODEC_SNAPPY), nested,
                              dict_chunk(PF_BYTE_ARRAY, 0, 300, {PD}, {4097}, 0, PF_CODEC_ZSTD)};
        const uint8_t zeros[5] = {0, 0, 0, 0, 0};
        BatchPlan a, b, c;
        const std::vector<pf_chunk_desc> cds = layout(cs, n);
        plan_batch(cds.data(), int(cds.size()), n, PfOpts{}, a);             // as every caller before the parameter
        plan_batch(cds.data(), int(cds.size()), n, PfOpts{}, b, nullptr);
        plan_batch(cds.data(), int(cds.size()), n, PfOpts{}, c, zeros);
        same_plan(a, b, "keep == NULL");
        same_plan(a, c, "keep all zero");
        for (const BatchPlan* p : {&a, &b, &c}) check(p->keeps.empty() && p->lists[L_IDS].empty() && p->off_keepof == p->off_keeps, "no keep: tables");
        // and a mixed batch: kept, not asked for, ineligible, nested
        const uint8_t mixed[5] = {1, 1, 0, 1, 1};
        BatchPlan m;
        plan_batch(cds.data(), int(cds.size()), n, PfOpts{}, m, mixed);
        bind_batch(m, BASES);
        check(m.keep_of[0] == 0 && m.keep_of[1] < 0 && m.keep_of[2] < 0 && m.keep_of[3] < 0 && m.keep_of[4] == 1, "mixed: kept chunks");
        check_plan(m, "mixed");
        bind_batch(a, BASES);
        check_plan(a, "no keep");
        // chunks that are not kept plan their pages as before (scratch offsets move, the lists' content per chunk does not)
        check(m.lists[L_SCAN] == std::vector<int>({1, 3}), "mixed: L_SCAN");
        check(m.out_bytes < a.out_bytes, "mixed: the out arena did not shrink (%zu, %zu)", m.out_bytes, a.out_bytes);
    }
    std::printf("dict plan check: failures %d\n", g_fail);
    return g_fail ? 1 : 0;
}
