// Invariant checks of the host batch planner (csrc/pf_plan.cpp) without a GPU: every golden file
// planned as one batch, and hand-made descriptor sets at the sizes where a routing decision flips.
// The planner never reads the input bytes, so the hand-made sets invent sizes and offsets.
// Built with -fsanitize=address,undefined by tests/test_plan_cpu.py.
//   pf_plan_check FILE...
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "pf_plan.h"
#include "pfloor.h"

using namespace pf;

namespace {

int g_failures = 0;
long g_checks = 0;
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

// made-up arena addresses, 256-byte aligned and 1 TiB apart
const ArenaBases BASES{0x10000000100ull, 0x20000000100ull, 0x30000000100ull, 0x40000000100ull, 0x50000000100ull, 0x60000000100ull};

struct Region {
    uint64_t off, len, align;
    const char* what;
    long idx;
};

// Regions of one arena: aligned, inside its size, pairwise disjoint.
void check_regions(const char* arena, std::vector<Region> r, uint64_t size) {
    for (const Region& x : r) {
        check(x.off % x.align == 0, "%s: %s %ld at %llu not %llu-aligned", arena, x.what, x.idx, (unsigned long long)x.off, (unsigned long long)x.align);
        check(x.off + x.len <= size, "%s: %s %ld [%llu, +%llu) past the arena's %llu bytes", arena, x.what, x.idx,
              (unsigned long long)x.off, (unsigned long long)x.len, (unsigned long long)size);
    }
    r.erase(std::remove_if(r.begin(), r.end(), [](const Region& x) { return x.len == 0; }), r.end());
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    for (size_t i = 0; i + 1 < r.size(); i++)
        check(r[i].off + r[i].len <= r[i + 1].off, "%s: %s %ld overlaps %s %ld", arena, r[i].what, r[i].idx, r[i + 1].what, r[i + 1].idx);
}

bool dict_enc(int e) { return e == PF_ENC_PLAIN_DICTIONARY || e == PF_ENC_RLE_DICTIONARY; }
bool in_list(const BatchPlan& p, ListId l, int v) { return std::count(p.lists[l].begin(), p.lists[l].end(), v) == 1; }
template <class T> uint64_t addr(T* q) { return reinterpret_cast<uintptr_t>(q); }

void check_arenas(const BatchPlan& p, size_t n_bytes) {
    std::vector<Region> S, O, B, M, T, PUB;
    for (size_t i = 0; i < p.pages.size(); i++) {
        const DevPage& pg = p.pages[i];
        const PagePlan& pp = p.pplan[i];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        const uint64_t nv = uint64_t(pg.num_values);
        const long I = long(i);
        check(pp.in_off + pg.rep_len + pg.def_len + ((pg.flags & PG_COMPRESSED) ? 0 : pg.body_len) <= n_bytes, "page %ld past the input", I);
        if (pg.flags & PG_COMPRESSED) {
            S.push_back({pp.scratch_off, pg.body_len, 16, "body", I});
            check(addr(pg.body) == BASES.scratch + pp.scratch_off, "page %ld body not at its scratch offset", I);
        } else {
            check(pp.scratch_off == NO_OFF, "page %ld: scratch body of an uncompressed page", I);
            check(addr(pg.body) == BASES.in + pp.in_off + pg.rep_len + pg.def_len, "page %ld body not in the input", I);
        }
        check((pg.lvl != nullptr) == bool(pg.flags & PG_V2) && (!pg.lvl || addr(pg.lvl) == BASES.in + pp.in_off), "page %ld lvl", I);
        if (pp.aux_off != NO_OFF) {
            const uint64_t len = (pg.flags & PG_DICT) ? 8 * (nv + 1)
                                 : ck.ptype == PF_BYTE_ARRAY ? 4 * nv + 16 + 8 * (nv / FBLK + 2)
                                 : ck.ptype == PF_FIXED_LEN_BYTE_ARRAY ? 4 * nv + 16 : 8 * nv + 8;   // (FLBA: DELTA_BYTE_ARRAY slot map)
            S.push_back({pp.aux_off, len, 256, "aux", I});
            check(pg.aux_cap == int64_t(nv), "page %ld aux_cap", I);
        }
        if (pp.rt_off != NO_OFF) S.push_back({pp.rt_off, RT_BYTES, 256, "runtab", I});
        if (pp.dx_off != NO_OFF) S.push_back({pp.dx_off, 8 * (3 * nv + 1), 256, "dx", I});
        if (pp.lt_off != NO_OFF) {
            S.push_back({pp.lt_off, 16 + 16ull * pg.lvl_cap + 4ull * LT_BT_WORDS * (nv / FBLK + 1), 256, "lvltab", I});
            check(pg.lvl_cap == lvl_table_cap(pg.num_values), "page %ld lvl_cap", I);
        }
        if (pp.seg_off != NO_OFF) {
            S.push_back({pp.seg_off, nest_seg_bytes(pg.nseg), 256, "seg", I});
            PUB.push_back({pp.pub_off, 2ull * uint64_t(pg.nwin) * sizeof(WinPub), 8, "npub", I});
            check(addr(pg.npub) == BASES.scratch + p.off_npub + pp.pub_off, "page %ld npub", I);
        }
        if (pp.dbp_off != NO_OFF) {
            S.push_back({pp.dbp_off, 12ull * pg.dbp_bcap + 16, 256, "dbp", I});
            PUB.push_back({pp.dbp_pub_off, uint64_t(pg.dbp_nwin) * sizeof(WinPub), 8, "dbp_pub", I});
            check(addr(pg.dbp_pub) == BASES.scratch + p.off_npub + pp.dbp_pub_off, "page %ld dbp_pub", I);
        }
        // bound pointers sit at their offsets (null where the page has no region)
        auto at = [&](uint64_t off) { return off == NO_OFF ? 0 : BASES.scratch + off; };
        check(addr(pg.aux) == at(pp.aux_off) && addr(pg.runtab) == at(pp.rt_off) && addr(pg.lvltab) == at(pp.lt_off) &&
                  addr(pg.dx) == at(pp.dx_off) && addr(pg.seg) == at(pp.seg_off) && addr(pg.dbp) == at(pp.dbp_off),
              "page %ld: a table pointer is not at its scratch offset", I);
    }
    for (size_t b = 0; b < p.bajobs.size(); b++) {
        const BaJob& J = p.bajobs[b];
        const uint64_t words = uint64_t(J.n_tiles) * (BA_TILE / 32);
        S.push_back({p.ba_bm[b], 4 * (3 * words + J.n_tiles), 256, "ba bitmaps", long(b)});
        check(addr(J.cand) == BASES.scratch + p.ba_bm[b] && J.link1 == J.cand + words && J.link2 == J.link1 + words &&
                  J.tile_cnt == J.link2 + words, "BaJob %zu bitmaps", b);
        check(uint64_t(J.n_tiles) * BA_TILE >= J.n_cap, "BaJob %zu: tiles do not cover its stream", b);
    }
    S.push_back({p.off_npub, p.npub_bytes, 256, "window hand-overs", 0});
    check_regions("scratch", S, p.scratch_bytes);
    check_regions("window hand-overs", PUB, p.npub_bytes);

    for (int c = 0; c < p.n_chunks; c++) {
        const DevChunk& ck = p.chunks[size_t(c)];
        const OutPlan& op = p.oplan[size_t(c)];
        const uint64_t e = uint64_t(ck.num_entries), vb = align_up((e + 7) / 8, 4);
        if (op.values != NO_OFF) O.push_back({op.values, e * uint64_t(ck.width), 256, "values", c});
        if (op.offsets != NO_OFF) O.push_back({op.offsets, 4 * (e + 1), 256, "offsets", c});
        if (op.list_offsets != NO_OFF) O.push_back({op.list_offsets, 4 * (e + 1), 256, "list offsets", c});
        if (op.def != NO_OFF) O.push_back({op.def, e, 256, "def levels", c});
        if (op.rep != NO_OFF) O.push_back({op.rep, e, 256, "rep levels", c});
        if (op.validity != NO_OFF) B.push_back({op.validity, vb, 256, "validity", c});
        if (op.list_validity != NO_OFF) B.push_back({op.list_validity, vb, 256, "list validity", c});
        auto at = [](uintptr_t base, uint64_t off) { return off == NO_OFF ? 0 : base + off; };
        check(addr(ck.values) == at(BASES.out, op.values) && addr(ck.offsets) == at(BASES.out, op.offsets) &&
                  addr(ck.list_offsets) == at(BASES.out, op.list_offsets) && addr(ck.def_levels) == at(BASES.out, op.def) &&
                  addr(ck.rep_levels) == at(BASES.out, op.rep) && addr(ck.validity) == at(BASES.bits, op.validity) &&
                  addr(ck.list_validity) == at(BASES.bits, op.list_validity), "chunk %d: an output pointer is not at its offset", c);
        if (p.host_status[size_t(c)] == 0) {
            check((op.values != NO_OFF) == (ck.width > 0) && (op.validity != NO_OFF) == (ck.max_def > 0) &&
                      (op.offsets != NO_OFF) == (ck.ptype == PF_BYTE_ARRAY) && (op.def != NO_OFF) == (ck.max_rep > 0),
                  "chunk %d: wrong set of output arrays", c);
            if (ck.dict_page >= 0) {
                const DevPage& dp = p.pages[size_t(ck.dict_page)];
                check(ck.dict_data == dp.body, "chunk %d dict_data", c);
                if (ck.ptype == PF_BYTE_ARRAY) check(ck.dict_pos == dp.aux && ck.dict_len == dp.aux + dp.num_values + 1, "chunk %d dict_pos", c);
            }
        }
    }
    check_regions("out", O, p.out_bytes);
    check_regions("bits", B, p.bits_bytes);

    const uint64_t nc = uint64_t(p.n_chunks);
    M.push_back({p.off_chunks, sizeof(DevChunk) * nc, 256, "chunks", 0});
    M.push_back({p.off_pages, sizeof(DevPage) * p.pages.size(), 256, "pages", 0});
    M.push_back({p.off_jobs, sizeof(SnappyJob) * p.jobs.size(), 256, "jobs", 0});
    for (int l = 0; l < N_LISTS; l++) M.push_back({p.off_lists + 4 * p.list_base[l], 4 * p.lists[l].size(), 4, "list", l});
    check(p.off_lists % 256 == 0 && p.list_base[0] == 0, "list array not 256-aligned");
    M.push_back({p.off_res, sizeof(DevChunkResult) * nc, 256, "results", 0});
    M.push_back({p.off_pieces, 8 * p.snap.pieces.size(), 256, "pieces", 0});
    M.push_back({p.off_splits, 4ull * p.snap.n_splits, 256, "splits", 0});
    M.push_back({p.off_fallback, 4 * p.jobs.size(), 256, "fallback flags", 0});
    M.push_back({p.off_wins, 8 * p.snap.wins.size(), 256, "wins", 0});
    M.push_back({p.off_bajobs, sizeof(BaJob) * p.bajobs.size(), 256, "bajobs", 0});
    M.push_back({p.off_batiles, 8 * p.ba_tiles.size(), 256, "ba tiles", 0});
    M.push_back({p.off_nfbq, 16 + 8ull * uint64_t(p.n_flat_fixed + p.n_null4 + p.n_null8), 16, "fallback queue", 0});
    check(p.meta_bytes >= 256 && p.meta_bytes % 256 == 0, "metadata size %zu", p.meta_bytes);
    M.push_back({p.meta_bytes - 256, 256, 256, "arena counter", 0});
    check_regions("meta", M, p.meta_bytes);

    uint64_t n_win = 0;
    for (const SnappyJob& jb : p.jobs) n_win += jb.n_win;
    T.push_back({0, n_win * SNAP_WWORDS * 4, 256, "token bitmaps", 0});
    T.push_back({p.snap.off_lane_out, n_win * 64 * 4, 256, "lane outs", 0});
    T.push_back({p.snap.off_win, n_win * sizeof(SnapWin), 256, "windows", 0});
    T.push_back({p.snap.off_ent, n_win * 64 * sizeof(SnapEnt), 256, "entry tables", 0});
    check_regions("tokmap", T, p.snap.tokmap_bytes);
    check(addr(p.snap.d_lane_out) == BASES.tokmap + p.snap.off_lane_out && addr(p.snap.d_win) == BASES.tokmap + p.snap.off_win &&
              addr(p.snap.d_ent) == BASES.tokmap + p.snap.off_ent, "tokmap table pointers");
    for (size_t j = 0; j < p.jobs.size(); j++) {
        const SnappyJob& jb = p.jobs[j];
        const DevPage& pg = p.pages[size_t(jb.page)];
        const PagePlan& pp = p.pplan[size_t(jb.page)];
        check(addr(jb.tokmap) == BASES.tokmap + uint64_t(jb.win_base) * SNAP_WWORDS * 4, "job %zu tokmap", j);
        check(addr(jb.src) == BASES.in + pp.in_off + pg.rep_len + pg.def_len && pp.in_off + pg.rep_len + pg.def_len + jb.src_len <= n_bytes,
              "job %zu src", j);
        check(jb.dst == pg.body && jb.dst_len == pg.body_len && (pg.flags & PG_COMPRESSED), "job %zu dst", j);
        check(addr(pg.jfb) == BASES.meta + p.off_fallback + 4 * j, "job %zu: its page's fallback flag", j);
    }
    for (size_t b = 0; b < p.bajobs.size(); b++) {
        const BaJob& J = p.bajobs[b];
        const DevPage& pg = p.pages[size_t(J.page)];
        if (int(b) < p.n_ba_dict)
            check(J.p == pg.body && J.n == pg.body_len && J.pos == p.chunks[size_t(J.chunk)].dict_pos &&
                      J.len == p.chunks[size_t(J.chunk)].dict_len && J.chars_out == nullptr, "dictionary BaJob %zu", b);
        else
            check(J.pos == pg.aux && pg.ba_job == int(b) && J.state == BA_SKIP &&
                      addr(J.chars_out) == BASES.meta + p.off_pages + sizeof(DevPage) * size_t(J.page) + offsetof(DevPage, n_chars),
                  "data BaJob %zu", b);
    }
}

void check_routing(const BatchPlan& p, const PfOpts& opts) {
    const int np = int(p.pages.size());
    // every page belongs to a chunk that planned, inside that chunk's page range
    for (int i = 0; i < np; i++) {
        const DevPage& pg = p.pages[size_t(i)];
        check(pg.chunk >= 0 && pg.chunk < p.n_chunks && p.host_status[size_t(pg.chunk)] == 0, "page %d of a failed chunk", i);
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        if (pg.flags & PG_DICT) check(ck.dict_page == i, "page %d: dictionary of chunk %d", i, pg.chunk);
        else check(i >= ck.first_page && i < ck.first_page + ck.n_pages, "page %d outside chunk %d's pages", i, pg.chunk);
    }
    // decode list: every data page once, the pages that will need k_decode first
    std::vector<int> seen(size_t(np), 0);
    const std::vector<int>& ld = p.lists[L_DECODE];
    for (size_t k = 0; k < ld.size(); k++) {
        const int i = ld[k];
        check(i >= 0 && i < np, "decode list entry %d", i);
        if (i < 0 || i >= np) continue;
        seen[size_t(i)]++;
        const DevPage& pg = p.pages[size_t(i)];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        const int e = pg.encoding;
        const bool first = ck.max_rep > 0 || ck.ptype == PF_BOOLEAN || !(e == PF_ENC_PLAIN || dict_enc(e) || e == PF_ENC_DELTA_BINARY_PACKED);
        check(first == (int(k) < p.n_decode_first), "page %d on the wrong side of n_decode_first", i);
    }
    for (int i = 0; i < np; i++) check(seen[size_t(i)] == ((p.pages[size_t(i)].flags & PG_DICT) ? 0 : 1), "page %d %d times in the decode list", i, seen[size_t(i)]);
    // count list: the pages of chunks that need counts, flat BYTE_ARRAY pages first
    const std::vector<int>& lc = p.lists[L_COUNT];
    size_t want_count = 0;
    for (int i = 0; i < np; i++) {
        const DevPage& pg = p.pages[size_t(i)];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        if ((pg.flags & PG_DICT) || !ck.needs_count) continue;
        want_count++;
        const auto it = std::find(lc.begin(), lc.end(), i);
        check(it != lc.end() && std::count(lc.begin(), lc.end(), i) == 1, "page %d not once in the count list", i);
        if (it != lc.end()) check((ck.ptype == PF_BYTE_ARRAY && ck.max_rep == 0) == (it - lc.begin() < p.n_count_flat), "page %d on the wrong side of n_count_flat", i);
    }
    check(lc.size() == want_count, "count list has %zu entries, %zu pages need counts", lc.size(), want_count);
    // the four flat grids
    const std::vector<int>& lf = p.lists[L_FLAT];
    const int glen[4] = {p.n_flat_fixed, p.n_flat_all, p.n_null4, p.n_null8};
    check(lf.size() == 2 * size_t(glen[0] + glen[1] + glen[2] + glen[3]), "flat list length");
    std::map<int, std::vector<int>> blocks;      // page -> blocks seen
    std::map<int, int> grid_of, shift_of;
    std::map<std::pair<int, int>, std::set<int>> labels;   // (grid, chunk) -> labels of its dictionary-encoded pages' blocks
    size_t base = 0;
    for (int g = 0; g < 4; g++) {
        check(glen[g] % 8 == 0, "grid %d length %d is no multiple of 8", g, glen[g]);
        for (int k = 0; k < glen[g] && 2 * (base + size_t(k)) + 1 < lf.size(); k++) {
            const int pgi = lf[2 * (base + size_t(k))], y = lf[2 * (base + size_t(k)) + 1];
            if (pgi < 0) { check(pgi == -1 && y == 0, "grid %d padding entry (%d, %d)", g, pgi, y); continue; }
            check(pgi < np, "grid %d entry page %d", g, pgi);
            if (pgi >= np) continue;
            check(!grid_of.count(pgi) || grid_of[pgi] == g, "page %d in grids %d and %d", pgi, grid_of.count(pgi) ? grid_of[pgi] : -1, g);
            const int sh = int(uint32_t(y) >> 28);
            check(!shift_of.count(pgi) || shift_of[pgi] == sh, "page %d: blocks of different sizes", pgi);
            grid_of[pgi] = g;
            shift_of[pgi] = sh;
            blocks[pgi].push_back(y & 0x0fffffff);
            if (dict_enc(p.pages[size_t(pgi)].encoding)) labels[{g, p.pages[size_t(pgi)].chunk}].insert(k % 8);
        }
        base += size_t(glen[g]);
    }
    for (int i = 0; i < np; i++) {
        const DevPage& pg = p.pages[size_t(i)];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        const bool flat = !(pg.flags & PG_DICT) && ck.max_rep == 0;
        check(flat == (blocks.count(i) == 1), "page %d: flat %d, in a flat grid %d", i, int(flat), int(blocks.count(i)));
        if (!flat || !blocks.count(i)) continue;
        std::vector<int> b = blocks[i];
        std::sort(b.begin(), b.end());
        const int64_t nb = int64_t(b.size()), bsz = int64_t(FBLK) << shift_of[i];
        for (int64_t k = 0; k < nb; k++) check(b[size_t(k)] == k, "page %d: block %lld missing or repeated", i, (long long)k);
        check(nb * bsz >= pg.num_values && (pg.num_values > (nb - 1) * bsz || (nb == 1 && pg.num_values == 0)),
              "page %d: %lld blocks of %lld for %d values", i, (long long)nb, (long long)bsz, pg.num_values);
        const bool fixed = ck.ptype != PF_BYTE_ARRAY, tab = pg.lvltab != nullptr;
        const int want = (tab && fixed && (dict_enc(pg.encoding) || pg.encoding == PF_ENC_PLAIN)) ? (ck.width == 4 ? 2 : ck.width == 8 ? 3 : 1)
                                                                                                : (fixed ? 0 : 1);
        check(grid_of[i] == want, "page %d in grid %d, expected %d", i, grid_of[i], want);
        check(shift_of[i] == ((fixed && !tab) ? opts.fix_shift : 0), "page %d: block shift %d", i, shift_of[i]);
        const bool big = ck.dict_page >= 0 && p.pages[size_t(ck.dict_page)].body_len > STICKY_DICT && dict_enc(pg.encoding);
        if (big) check(labels[{grid_of[i], pg.chunk}].size() == 1, "chunk %d: big dictionary, blocks on %zu labels", pg.chunk, labels[{grid_of[i], pg.chunk}].size());
    }
    // a page has a table exactly when it is in that table's list
    for (int i = 0; i < np; i++) {
        const DevPage& pg = p.pages[size_t(i)];
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        check((pg.lvltab != nullptr) == in_list(p, L_LVL, i), "page %d: level table / L_LVL", i);
        check((pg.runtab != nullptr) == in_list(p, L_RUNS, i), "page %d: run table / L_RUNS", i);
        check((pg.dx != nullptr) == in_list(p, L_DLEN, i), "page %d: dx / L_DLEN", i);
        check((pg.dx != nullptr && pg.encoding == PF_ENC_DELTA_BYTE_ARRAY) == in_list(p, L_DBA, i), "page %d: L_DBA", i);
        check((pg.seg != nullptr) == in_list(p, L_NEST, i), "page %d: seg / L_NEST", i);
        const bool dbp_page = !(pg.flags & PG_DICT) && pg.encoding == PF_ENC_DELTA_BINARY_PACKED && (ck.ptype == PF_INT32 || ck.ptype == PF_INT64);
        check(dbp_page == in_list(p, L_DELTA, i), "page %d: L_DELTA", i);
        check((pg.dbp != nullptr) == (dbp_page && pg.num_values >= DBP_PAR_MIN && opts.dbp_par), "page %d: dbp tables", i);
        check(!pg.dbp || (pg.dbp_nwin > 0 && pg.dbp_nwin <= p.max_dbp_nwin && uint64_t(pg.dbp_bcap) * 8 >= uint64_t(pg.num_values)), "page %d: dbp sizes", i);
        if (pg.seg) {
            check(pg.nseg >= 1 && pg.nseg <= int(NEST_MAX_SEGS) && int64_t(pg.nseg) * pg.seg_len >= pg.num_values &&
                      int64_t(pg.nseg - 1) * pg.seg_len < pg.num_values && pg.nwin > 0 && pg.nwin <= p.max_nwin, "page %d: %d segments of %d for %d", i, pg.nseg, pg.seg_len, pg.num_values);
        } else {
            check(pg.nseg == 0 && pg.seg_len == 0 && pg.npub == nullptr, "page %d: segment fields without segments", i);
        }
        const bool cdict = !(pg.flags & PG_DICT) && ck.ptype == PF_BYTE_ARRAY && ck.max_rep == 0 && pg.runtab && dict_enc(pg.encoding);
        const std::vector<int>& cd = p.lists[L_CDICT];
        int n = 0;
        for (size_t k = 0; k + 1 < cd.size(); k += 2) n += cd[k] == i;
        check(n == (cdict ? std::max(1, int((int64_t(pg.num_values) + FBLK - 1) / FBLK)) : 0), "page %d: %d k_count_dict blocks", i, n);
    }
    {   // L_NSEG: the segments of the L_NEST pages, in order
        std::vector<int> want;
        for (int i : p.lists[L_NEST])
            for (int k = 0; k < p.pages[size_t(i)].nseg; k++) { want.push_back(i); want.push_back(k); }
        check(want == p.lists[L_NSEG], "L_NSEG is not the segments of L_NEST");
    }
    {   // L_SCAN: the planned chunks that need counts
        std::vector<int> want;
        for (int c = 0; c < p.n_chunks; c++) if (p.host_status[size_t(c)] == 0 && p.chunks[size_t(c)].needs_count) want.push_back(c);
        check(want == p.lists[L_SCAN], "L_SCAN");
    }
    for (int l = 0; l < N_LISTS; l++) check(p.list_base[l + 1] == p.list_base[l] + p.lists[l].size(), "list_base[%d]", l + 1);
}

void check_snappy(const BatchPlan& p) {
    const SnappyPlan& sp = p.snap;
    std::set<std::pair<int, int>> pw, pp;
    uint32_t wb = 0, sb = 0;
    int max_win = 1;
    for (size_t j = 0; j < p.jobs.size(); j++) {
        const SnappyJob& jb = p.jobs[j];
        check(jb.n_win == std::max<uint64_t>(1, (uint64_t(jb.src_len) + SNAP_WIN - 1) / SNAP_WIN), "job %zu n_win", j);
        check(jb.n_pieces == std::max<uint64_t>(1, (uint64_t(jb.dst_len) + SNAP_BLOCK - 1) / SNAP_BLOCK), "job %zu n_pieces", j);
        check(jb.win_base == wb && jb.split_base == sb, "job %zu: bases are not the prefix sums", j);
        wb += jb.n_win;
        sb += jb.n_pieces;
        max_win = std::max(max_win, int(jb.n_win));
        const bool lit = (p.pages[size_t(jb.page)].flags & PG_DICT) || jb.src_len >= jb.dst_len;
        check(lit == in_list(p, L_DJOBS, int(j)) && lit == bool(jb.dflags & 2u), "job %zu: litcopy candidate", j);
    }
    check(sp.n_splits == sb && sp.pieces.size() == sb && sp.wins.size() == wb && sp.max_snap_win == max_win, "Snappy totals");
    for (const Int2& w : sp.wins) check(w.x >= 0 && size_t(w.x) < p.jobs.size() && w.y >= 0 && uint32_t(w.y) < p.jobs[size_t(w.x)].n_win && pw.insert({w.x, w.y}).second, "win (%d, %d)", w.x, w.y);
    for (const Int2& k : sp.pieces) check(k.x >= 0 && size_t(k.x) < p.jobs.size() && k.y >= 0 && uint32_t(k.y) < p.jobs[size_t(k.x)].n_pieces && pp.insert({k.x, k.y}).second, "piece (%d, %d)", k.x, k.y);
}

void check_failed(const BatchPlan& p) {
    for (int c = 0; c < p.n_chunks; c++) {
        if (p.host_status[size_t(c)] == 0) continue;
        const DevChunk& ck = p.chunks[size_t(c)];
        check(p.host_status[size_t(c)] < 0 && ck.n_pages == 0 && ck.dict_page == -1 && ck.num_entries == 0, "failed chunk %d keeps pages", c);
        for (const DevPage& pg : p.pages) check(pg.chunk != c, "a page of failed chunk %d", c);
        for (const SnappyJob& jb : p.jobs) check(jb.chunk != c, "a Snappy job of failed chunk %d", c);
        for (const BaJob& J : p.bajobs) check(J.chunk != c, "a BaJob of failed chunk %d", c);
        check(!in_list(p, L_SCAN, c), "failed chunk %d in L_SCAN", c);
        const OutPlan& op = p.oplan[size_t(c)];
        check(op.values == NO_OFF && op.validity == NO_OFF && op.offsets == NO_OFF && op.def == NO_OFF, "failed chunk %d has outputs", c);
    }
}

// Plans, binds and checks every invariant.
void plan_and_check(const char* name, const std::vector<pf_chunk_desc>& cds, size_t n_bytes, const PfOpts& opts, BatchPlan& p) {
    g_case = name;
    plan_batch(cds.data(), int(cds.size()), n_bytes, opts, p);
    bind_batch(p, BASES);
    check(p.pages.size() == p.pplan.size() && p.chunks.size() == cds.size() && p.oplan.size() == cds.size(), "table sizes");
    check_arenas(p, n_bytes);
    check_routing(p, opts);
    check_snappy(p);
    check_failed(p);
}

// ---- (a) golden files ----
int plan_golden(const char* path) {
    pf_file* f = nullptr;
    if (pf_file_open(path, &f) != PF_OK) { std::fprintf(stderr, "cannot open %s: %s\n", path, pf_file_last_error()); return 1; }
    int nrg = 0, nc = 0;
    pf_file_num_row_groups(f, &nrg);
    pf_file_num_columns(f, &nc);
    std::vector<pf_chunk_desc> cds;
    uint64_t off = 0;
    for (int rg = 0; rg < nrg; rg++)
        for (int c = 0; c < nc; c++) {
            pf_chunk_desc d;
            if (pf_file_chunk_desc(f, rg, c, off, &d) != PF_OK) { std::fprintf(stderr, "%s rg %d col %d: %s\n", path, rg, c, pf_file_last_error()); pf_file_close(f); return 1; }
            off += align_up(d.chunk_size, 256);
            cds.push_back(d);
        }
    BatchPlan p;
    plan_and_check(path, cds, off, PfOpts{}, p);
    for (size_t c = 0; c < cds.size(); c++) check(p.host_status[c] == 0, "chunk %zu of a golden file does not plan: %lld", c, (long long)p.host_status[c]);
    pf_file_close(f);
    return 0;
}

// ---- (b) hand-made descriptors ----
struct Chunk {
    pf_chunk_desc d{};
    std::vector<pf_page_desc> pages;
};
Chunk chunk(int ptype, int max_def, int max_rep, int codec) {
    Chunk c;
    c.d.physical_type = ptype;
    c.d.max_def = max_def;
    c.d.max_rep = max_rep;
    c.d.repeated_def = max_rep ? 1 : 0;
    c.d.list_null_def = max_rep ? 1 : 0;
    c.d.codec = codec;
    return c;
}
pf_page_desc page(int type, int enc, int nv, uint32_t comp, uint32_t uncomp, int nulls = -1) {
    pf_page_desc d{};
    d.page_type = type; d.encoding = enc; d.def_encoding = PF_ENC_RLE; d.rep_encoding = PF_ENC_RLE;
    d.num_values = nv; d.compressed_size = comp; d.uncompressed_size = uncomp; d.num_nulls = nulls; d.is_compressed = 1;
    return d;
}
// Lays the chunks out back to back (40 bytes of header before every page) and returns the descriptors.
std::vector<pf_chunk_desc> layout(std::vector<Chunk>& cs, size_t& n_bytes) {
    std::vector<pf_chunk_desc> out;
    uint64_t off = 0;
    for (Chunk& c : cs) {
        uint64_t in = 0;
        for (pf_page_desc& pd : c.pages) { pd.offset = in + 40; in = pd.offset + pd.compressed_size; }
        c.d.n_pages = int(c.pages.size());
        c.d.pages = c.pages.data();
        c.d.chunk_offset = off;
        if (c.d.chunk_size == 0) c.d.chunk_size = in;
        off += align_up(c.d.chunk_size, 256);
        out.push_back(c.d);
    }
    n_bytes = off;
    return out;
}
// Plans one chunk set; the plan stays in `p` for the caller's own assertions.
void run(const char* name, std::vector<Chunk> cs, const PfOpts& opts, BatchPlan& p) {
    size_t n = 0;
    const std::vector<pf_chunk_desc> cds = layout(cs, n);
    plan_and_check(name, cds, n, opts, p);
}
int blocks_of(const BatchPlan& p, int pg) {
    int n = 0;
    for (size_t k = 0; k + 1 < p.lists[L_FLAT].size(); k += 2) n += p.lists[L_FLAT][k] == pg;
    return n;
}
std::set<int> labels_of(const BatchPlan& p, int pg) {
    std::set<int> s;
    for (size_t k = 0; k + 1 < p.lists[L_FLAT].size(); k += 2) if (p.lists[L_FLAT][k] == pg) s.insert(int(k / 2) % 8);
    return s;
}

void hand_made() {
    BatchPlan p;
    char name[96];
    // 1. flat fixed-width pages around one and two blocks, 4096- and 8192-entry blocks
    for (int sh = 0; sh <= 1; sh++)
        for (int nv : {4096, 4097, 8192, 8193}) {
            PfOpts o; o.fix_shift = sh;
            Chunk c = chunk(PF_INT64, 0, 0, PF_CODEC_UNCOMPRESSED);
            c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, nv, 8u * uint32_t(nv), 8u * uint32_t(nv)));
            std::snprintf(name, sizeof name, "1 fixed %d values shift %d", nv, sh);
            run(name, {c}, o, p);
            const int bsz = 4096 << sh;
            check(blocks_of(p, 0) == (nv + bsz - 1) / bsz && p.n_flat_fixed == 8 && p.n_flat_all == 0, "blocks %d", blocks_of(p, 0));
            for (size_t k = 0; k + 1 < p.lists[L_FLAT].size(); k += 2)
                if (p.lists[L_FLAT][k] == 0) check((uint32_t(p.lists[L_FLAT][k + 1]) >> 28) == uint32_t(sh), "shift bits");
        }
    // 2. nullable dictionary pages: level table and null grid only when the page may hold nulls; the id run table
    // always (4095, 4096, 4097 entries: the edges of the tables' per-block parts)
    for (int pt : {PF_INT32, PF_INT64})
        for (int nulls : {-1, 0, 7})
            for (int nv : {5000, 4095, 4096, 4097}) {
                Chunk c = chunk(pt, 1, 0, PF_CODEC_UNCOMPRESSED);
                c.pages.push_back(page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, 100, 800, 800));
                c.pages.push_back(page(PF_PAGE_DATA_V2, PF_ENC_RLE_DICTIONARY, nv, 5000, 5000, nulls));
                c.pages[1].def_bytes = 700;
                std::snprintf(name, sizeof name, "2 nullable type %d nulls %d, %d values", pt, nulls, nv);
                run(name, {c}, PfOpts{}, p);
                const bool tab = nulls != 0;
                check((p.pages[1].lvltab != nullptr) == tab && p.lists[L_LVL].size() == size_t(tab) && p.pages[1].runtab != nullptr, "level table");
                check((pt == PF_INT32 ? p.n_null4 : p.n_null8) == (tab ? 8 : 0) && (pt == PF_INT32 ? p.n_null8 : p.n_null4) == 0 && p.n_flat_fixed == (tab ? 0 : 8), "null grid");
                check(blocks_of(p, 1) == (tab ? (nv + 4095) / 4096 : 1), "blocks");
                check((p.null_caps.dlds > 0) == tab && p.null_caps.dcap >= 16 && p.null_caps.dcap % 16 == 0 && p.null_caps.icap % 16 == 0 && p.null_caps.dcap <= NL_DST && p.null_caps.icap <= NL_IST, "null caps");
            }
    // 3. nested pages: segments
    struct N { int nv; bool set; int64_t seg; int nseg, seg_len; };
    for (const N& t : {N{2048, false, 0, 0, 0}, N{2049, false, 0, 2, 2048}, N{4095, false, 0, 2, 2048}, N{4096, false, 0, 2, 2048},
                       N{4097, false, 0, 3, 2048}, N{2048 * 1024 + 1, false, 0, 1024, 2049}, N{100, true, 64, 2, 64}, N{10, true, 64, 1, 64},
                       N{5000, true, 0, 0, 0}}) {
        PfOpts o; o.nest_seg_set = t.set; o.nest_seg = t.seg;
        Chunk c = chunk(PF_INT64, 2, 1, PF_CODEC_UNCOMPRESSED);
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, t.nv, 9u * uint32_t(t.nv), 9u * uint32_t(t.nv)));
        std::snprintf(name, sizeof name, "3 nested %d values seg %s%lld", t.nv, t.set ? "" : "default ", (long long)t.seg);
        run(name, {c}, o, p);
        check(p.pages[0].nseg == t.nseg && p.pages[0].seg_len == t.seg_len && p.lists[L_NEST].size() == size_t(t.nseg > 0) && p.lists[L_NSEG].size() == 2 * size_t(t.nseg),
              "segments %d of %d", p.pages[0].nseg, p.pages[0].seg_len);
        check(p.n_decode_first == 1 && blocks_of(p, 0) == 0, "nested page routing");
    }
    // 4. DELTA_BINARY_PACKED: block-parallel from 16384 entries
    for (int nv : {16383, 16384, 16385})
        for (bool par : {true, false}) {
            PfOpts o; o.dbp_par = par;
            Chunk c = chunk(PF_INT64, 0, 0, PF_CODEC_UNCOMPRESSED);
            c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_DELTA_BINARY_PACKED, nv, 20000, 20000));
            std::snprintf(name, sizeof name, "4 dbp %d values par %d", nv, int(par));
            run(name, {c}, o, p);
            check((p.pages[0].dbp != nullptr) == (nv >= 16384 && par) && p.lists[L_DELTA].size() == 1 && p.pages[0].aux != nullptr, "dbp tables");
            check((p.max_dbp_nwin > 0) == (nv >= 16384 && par), "max_dbp_nwin %d", p.max_dbp_nwin);
        }
    // 4b. DELTA_BYTE_ARRAY: BYTE_ARRAY and FIXED_LEN_BYTE_ARRAY pages get k_dlen's tables (FLBA also a slot map) and
    // k_dba_chars; no other type does (k_decode reports the page)
    // (4095, 4096, 4097 entries: the edges of the block chars behind a BYTE_ARRAY page's aux words)
    for (int pt : {PF_BYTE_ARRAY, PF_FIXED_LEN_BYTE_ARRAY, PF_INT32})
        for (int rep : {0, 1})
            for (int nv : {5000, 4095, 4096, 4097}) {
                Chunk c = chunk(pt, 1 + rep, rep, PF_CODEC_UNCOMPRESSED);
                c.d.type_length = pt == PF_FIXED_LEN_BYTE_ARRAY ? 7 : 0;
                c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_DELTA_BYTE_ARRAY, nv, 30000, 30000));
                std::snprintf(name, sizeof name, "4b delta byte array type %d rep %d, %d values", pt, rep, nv);
                run(name, {c}, PfOpts{}, p);
                const bool tabs = pt != PF_INT32;
                check((p.pages[0].dx != nullptr) == tabs && (p.pages[0].aux != nullptr) == tabs && p.lists[L_DLEN].size() == size_t(tabs) &&
                          p.lists[L_DBA].size() == size_t(tabs), "delta byte array tables");
                check(p.n_decode_first == 1 && p.pages[0].nseg == 0, "delta byte array routing");
            }
    // 5. BYTE_ARRAY dictionary at and above the sticky threshold
    for (uint32_t db : {65536u, 65537u}) {
        Chunk c = chunk(PF_BYTE_ARRAY, 0, 0, PF_CODEC_UNCOMPRESSED);
        c.pages.push_back(page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, 4000, db, db));
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_RLE_DICTIONARY, 5 * 4096, 30000, 30000));
        std::snprintf(name, sizeof name, "5 string dictionary %u bytes", db);
        run(name, {c}, PfOpts{}, p);
        check(blocks_of(p, 1) == 5 && labels_of(p, 1).size() == (db > 65536 ? 1u : 5u), "labels %zu", labels_of(p, 1).size());
        check(p.n_flat_all == (db > 65536 ? 40 : 8) && p.n_ba_dict == 1 && p.lists[L_CDICT].size() == 10, "grid %d", p.n_flat_all);
    }
    // 6. PLAIN BYTE_ARRAY: short values or not
    for (uint32_t per : {48u, 49u}) {
        Chunk c = chunk(PF_BYTE_ARRAY, 0, 0, PF_CODEC_UNCOMPRESSED);
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, 1000, per * 1000, per * 1000));
        Chunk d = chunk(PF_BYTE_ARRAY, 0, 0, PF_CODEC_UNCOMPRESSED);
        d.pages.push_back(page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, 100, per * 100, per * 100));
        d.pages.push_back(page(PF_PAGE_DATA, PF_ENC_RLE_DICTIONARY, 1000, 1200, 1200));
        std::snprintf(name, sizeof name, "6 strings of %u bytes", per);
        run(name, {c, d}, PfOpts{}, p);
        check(p.ba_short_data == (per == 48) && p.ba_short_dict == (per == 48), "ba_short %d %d", int(p.ba_short_dict), int(p.ba_short_data));
        check(p.bajobs.size() == 2 && p.n_ba_dict == 1 && p.bajobs[1].n_tiles == (per * 1000 + BA_TILE - 1) / BA_TILE && p.pages[0].ba_job == 1, "walk jobs");
    }
    // 7. Snappy windows and pieces
    for (uint32_t comp : {8192u, 8193u})
        for (uint32_t unc : {65536u, 65537u}) {
            Chunk c = chunk(PF_INT32, 0, 0, PF_CODEC_SNAPPY);
            c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, 16384, comp, unc));
            std::snprintf(name, sizeof name, "7 snappy %u -> %u", comp, unc);
            run(name, {c}, PfOpts{}, p);
            check(p.jobs.size() == 1 && p.snap.wins.size() == (comp > 8192 ? 2u : 1u) && p.snap.pieces.size() == (unc > 65536 ? 2u : 1u), "wins %zu pieces %zu", p.snap.wins.size(), p.snap.pieces.size());
            check(p.pages[0].body_len == unc && (p.pages[0].flags & PG_COMPRESSED), "compressed body");
        }
    // 8. v2 levels filling the page exactly, and one byte more
    for (int extra : {0, 1}) {
        Chunk c = chunk(PF_INT32, 1, 0, PF_CODEC_UNCOMPRESSED);
        c.pages.push_back(page(PF_PAGE_DATA_V2, PF_ENC_PLAIN, 100, 50, 50, 100));
        c.pages[0].def_bytes = 30 + extra;
        c.pages[0].rep_bytes = 20;
        std::snprintf(name, sizeof name, "8 v2 levels %d of 50 bytes", 50 + extra);
        run(name, {c}, PfOpts{}, p);
        check(p.host_status[0] == (extra ? PF_ERR_CORRUPT_PAGE : 0) && p.pages.size() == size_t(1 - extra), "status %lld", (long long)p.host_status[0]);
        if (!extra) check(p.pages[0].body_len == 0 && p.pages[0].def_len == 30 && p.pages[0].rep_len == 20, "empty values section");
    }
    // 9. one bad chunk between two good ones
    auto good_a = [] {
        Chunk c = chunk(PF_BYTE_ARRAY, 1, 0, PF_CODEC_SNAPPY);
        c.pages.push_back(page(PF_PAGE_DICTIONARY, PF_ENC_PLAIN, 300, 4000, 70000));
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_RLE_DICTIONARY, 9000, 3000, 12000));
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, 2000, 30000, 40000));
        return c;
    };
    auto good_b = [] {
        Chunk c = chunk(PF_INT64, 1, 1, PF_CODEC_SNAPPY);
        c.pages.push_back(page(PF_PAGE_DATA_V2, PF_ENC_DELTA_BINARY_PACKED, 20000, 9000, 20000, 5));
        c.pages[0].def_bytes = 600; c.pages[0].rep_bytes = 500;
        c.pages.push_back(page(PF_PAGE_DATA, PF_ENC_PLAIN, 5000, 9000, 41000));
        return c;
    };
    struct Bad { const char* what; int status; Chunk c; };
    std::vector<Bad> bad;
    {
        Chunk c = good_a(); c.d.codec = PF_CODEC_GZIP;
        bad.push_back({"unsupported codec", PF_ERR_UNSUPPORTED_CODEC, c});
        c = good_a(); c.d.chunk_size = 30000;   // the third page ends past it
        bad.push_back({"page past the chunk end", PF_ERR_CORRUPT_PAGE, c});
        c = good_a(); c.pages.insert(c.pages.begin() + 1, c.pages[0]);
        bad.push_back({"two dictionary pages", PF_ERR_CORRUPT_PAGE, c});
        c = good_a(); std::swap(c.pages[0], c.pages[1]);
        bad.push_back({"dictionary after a data page", PF_ERR_CORRUPT_PAGE, c});
        c = good_a(); c.pages[2].num_values = -1;
        bad.push_back({"negative num_values", PF_ERR_CORRUPT_PAGE, c});
        c = good_a(); c.pages[2].uncompressed_size = (1u << 29) + 1;
        bad.push_back({"uncompressed_size > 2^29", PF_ERR_CORRUPT_PAGE, c});
    }
    BatchPlan ref;
    run("9 good neighbours alone", {good_a(), good_b()}, PfOpts{}, ref);
    check(ref.host_status[0] == 0 && ref.host_status[1] == 0 && ref.pages.size() == 5 && ref.jobs.size() == 5, "the good chunks plan");
    for (const Bad& b : bad) {
        std::snprintf(name, sizeof name, "9 %s", b.what);
        run(name, {good_a(), b.c, good_b()}, PfOpts{}, p);
        check(p.host_status[0] == 0 && p.host_status[1] == b.status && p.host_status[2] == 0, "statuses %lld %lld %lld",
              (long long)p.host_status[0], (long long)p.host_status[1], (long long)p.host_status[2]);
        // the neighbours are routed as without the bad chunk: same pages and lists, chunk 2 for chunk 1
        auto rechunk = [](int c) { return c == 2 ? 1 : c; };
        check(p.pages.size() == ref.pages.size() && p.jobs.size() == ref.jobs.size() && p.bajobs.size() == ref.bajobs.size(), "table sizes differ");
        for (size_t i = 0; i < p.pages.size() && i < ref.pages.size(); i++) {
            const DevPage &x = p.pages[i], &y = ref.pages[i];
            check(rechunk(x.chunk) == y.chunk && x.flags == y.flags && x.encoding == y.encoding && x.num_values == y.num_values && x.body_len == y.body_len &&
                      x.entry_start == y.entry_start && x.ba_job == y.ba_job && x.nseg == y.nseg && x.seg_len == y.seg_len && x.nwin == y.nwin &&
                      x.dbp_nwin == y.dbp_nwin && x.dbp_bcap == y.dbp_bcap && x.lvl_cap == y.lvl_cap && x.aux_cap == y.aux_cap &&
                      (x.aux != nullptr) == (y.aux != nullptr) && (x.runtab != nullptr) == (y.runtab != nullptr) && (x.lvltab != nullptr) == (y.lvltab != nullptr) &&
                      (x.seg != nullptr) == (y.seg != nullptr) && (x.dbp != nullptr) == (y.dbp != nullptr), "page %zu differs", i);
        }
        for (int l = 0; l < N_LISTS; l++) {
            std::vector<int> v = p.lists[l];
            if (l == L_SCAN) for (int& c : v) c = rechunk(c);
            check(v == ref.lists[l], "list %d differs", l);
        }
        for (size_t j = 0; j < p.jobs.size() && j < ref.jobs.size(); j++)
            check(p.jobs[j].page == ref.jobs[j].page && rechunk(p.jobs[j].chunk) == ref.jobs[j].chunk && p.jobs[j].win_base == ref.jobs[j].win_base &&
                      p.jobs[j].split_base == ref.jobs[j].split_base && p.jobs[j].dflags == ref.jobs[j].dflags, "job %zu differs", j);
        check(p.n_decode_first == ref.n_decode_first && p.n_count_flat == ref.n_count_flat && p.n_flat_fixed == ref.n_flat_fixed && p.n_flat_all == ref.n_flat_all &&
                  p.n_null4 == ref.n_null4 && p.n_null8 == ref.n_null8 && p.n_ba_dict == ref.n_ba_dict && p.n_ba_dict_tiles == ref.n_ba_dict_tiles &&
                  p.max_nwin == ref.max_nwin && p.max_dbp_nwin == ref.max_dbp_nwin && p.snap.n_splits == ref.snap.n_splits && p.out_bytes == ref.out_bytes &&
                  p.bits_bytes == ref.bits_bytes, "counters differ");
        const bool same_pairs = p.snap.pieces.size() == ref.snap.pieces.size() &&
                                std::equal(p.snap.pieces.begin(), p.snap.pieces.end(), ref.snap.pieces.begin(), [](Int2 a, Int2 b) { return a.x == b.x && a.y == b.y; });
        check(same_pairs, "piece order differs");
    }
}

}  // namespace

int main(int argc, char** argv) {
    int files = 0;
    for (int i = 1; i < argc; i++) {
        if (plan_golden(argv[i])) return 2;
        files++;
    }
    hand_made();
    std::printf("files %d checks %ld failures %d\n", files, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
