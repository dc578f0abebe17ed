// pf_result.cpp — the result side of a decode batch on the host (pf_result.h): side-table layouts, the arena and
// rerun decisions, and the merge of the decode's, the window's and the selection's view into pf_column_info.
#include "pf_result.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>

namespace pf {

ResLayout res_layout(int n_chunks) {
    ResLayout l{};
    l.res_bytes = sizeof(DevChunkResult) * size_t(n_chunks);
    l.chunks_off = align_up(l.res_bytes, 256);
    l.chunks_bytes = sizeof(DevChunk) * size_t(n_chunks);
    l.total = l.chunks_off + l.chunks_bytes + 256;
    return l;
}

WinLayout win_layout(int n_wins) {
    WinLayout l{};
    l.wins_bytes = sizeof(DevWin) * size_t(n_wins);
    l.res_off = align_up(l.wins_bytes, 256);
    l.res_bytes = sizeof(DevWinRes) * size_t(n_wins);
    l.total = l.res_off + l.res_bytes;
    return l;
}

int win_grid(const BatchPlan& p, const std::vector<DevWin>& wins) {
    uint64_t tiles = 1;
    for (const DevWin& w : wins) {
        const DevChunk& ck = p.chunks[size_t(w.chunk)];
        const uint64_t n = ck.max_rep == 0 && w.take >= 0 ? uint64_t(w.take) : uint64_t(ck.num_entries);
        tiles = std::max<uint64_t>(tiles, n * uint64_t(std::max(ck.width, 8)) / WIN_TILE + 8);
    }
    return int(std::min<uint64_t>(tiles, 512));
}

SelLayout layout_filter(const BatchPlan& p, const FilterPlan& f, const std::vector<DevWin>& wins) {
    SelLayout l;
    const size_t nc = size_t(p.n_chunks), np = f.preds.size();
    l.win_of.assign(nc, -1);
    for (size_t i = 0; i < wins.size(); i++) l.win_of[size_t(wins[i].chunk)] = int32_t(i);
    // rows_in is the first predicate chunk's row count after its window: at most take rows, or the chunk's entries
    // (a predicate chunk is flat: rows = entries)
    const size_t c0 = size_t(f.preds[0].chunk);
    l.rows_cap = p.chunks[c0].num_entries;
    if (l.win_of[c0] >= 0 && wins[size_t(l.win_of[c0])].take >= 0)
        l.rows_cap = std::min<int64_t>(l.rows_cap, wins[size_t(l.win_of[c0])].take);
    l.rows_cap = std::max<int64_t>(l.rows_cap, 0);
    const size_t tiles = l.tiles = std::max<size_t>(1, (size_t(l.rows_cap) + SEL_TILE - 1) / SEL_TILE);
    l.grid = int(std::min<size_t>(tiles, 256));
    size_t m = 0;
    auto take = [&](size_t n) { const size_t o = align_up(m, 256); m = o + n; return o; };
    l.o_head = take(sizeof(DevSelHead));
    l.o_sc = take(sizeof(DevSelChunk) * nc);
    l.o_up = take(0);
    l.o_preds = take(sizeof(DevPred) * np);
    l.o_blob = take(f.blob.size());
    l.o_winof = take(4 * nc);
    const size_t nd = f.dicts.size();
    if (nd > 0) {   // (behind the existing tables, and only then: a batch without one keeps its layout)
        l.o_drec = take(sizeof(DevSelDict) * nd);
        l.o_dof = take(4 * np);
    }
    l.up_end = m;
    l.o_mask = take(8 * tiles * (SEL_TILE / 64));
    l.o_tc = take(4 * tiles);
    l.o_tb = take(4 * tiles);
    l.o_rows = take(4 * tiles * SEL_TILE);
    l.o_bs = take(4 * tiles * nc);
    l.o_bb = take(4 * tiles * nc);
    l.o_bt = take(8 * nc);
    if (nd > 0) {
        l.o_dbits = take(8 * size_t(f.dict_words));
        l.dict_tiles = int(std::max<int64_t>(1, (f.dict_max_entries + SELD_TILE - 1) / SELD_TILE));
    }
    l.total = m;
    return l;
}

void fill_filter(const SelLayout& l, const FilterPlan& f, uint8_t* h) {
    std::memset(h, 0, l.up_end);
    std::memcpy(h + l.o_preds, f.preds.data(), sizeof(DevPred) * f.preds.size());
    if (!f.blob.empty()) std::memcpy(h + l.o_blob, f.blob.data(), f.blob.size());
    if (!l.win_of.empty()) std::memcpy(h + l.o_winof, l.win_of.data(), 4 * l.win_of.size());
    if (!f.dicts.empty()) {
        std::memcpy(h + l.o_drec, f.dicts.data(), sizeof(DevSelDict) * f.dicts.size());
        std::memcpy(h + l.o_dof, f.dict_of.data(), 4 * f.dict_of.size());
    }
}

SelBufs bind_sel(const SelLayout& l, const FilterPlan& f, uintptr_t base) {
    uint8_t* d = reinterpret_cast<uint8_t*>(base);
    SelBufs s{};
    s.head = reinterpret_cast<DevSelHead*>(d + l.o_head);
    s.sc = reinterpret_cast<DevSelChunk*>(d + l.o_sc);
    s.preds = reinterpret_cast<const DevPred*>(d + l.o_preds);
    s.blob = d + l.o_blob;
    s.win_of = reinterpret_cast<const int32_t*>(d + l.o_winof);
    s.mask = reinterpret_cast<uint64_t*>(d + l.o_mask);
    s.tile_count = reinterpret_cast<uint32_t*>(d + l.o_tc);
    s.tile_base = reinterpret_cast<uint32_t*>(d + l.o_tb);
    s.rows = reinterpret_cast<int32_t*>(d + l.o_rows);
    s.ba_sum = reinterpret_cast<uint32_t*>(d + l.o_bs);
    s.ba_base = reinterpret_cast<uint32_t*>(d + l.o_bb);
    s.ba_total = reinterpret_cast<int64_t*>(d + l.o_bt);
    s.rows_cap = l.rows_cap;
    s.tiles_cap = int64_t(l.tiles);
    s.n_preds = int32_t(f.preds.size());
    return s;
}

SelDictBufs bind_sel_dict(const SelLayout& l, const FilterPlan& f, uintptr_t base, const DevKeep* keeps, const int32_t* keep_of) {
    SelDictBufs s{};
    s.keeps = keeps;   // (k_sel_prep sizes a kept payload chunk by them, whatever the predicates are on)
    s.keep_of = keep_of;
    if (f.dicts.empty()) return s;
    uint8_t* d = reinterpret_cast<uint8_t*>(base);
    s.recs = reinterpret_cast<const DevSelDict*>(d + l.o_drec);
    s.dict_of = reinterpret_cast<const int32_t*>(d + l.o_dof);
    s.bits = reinterpret_cast<uint64_t*>(d + l.o_dbits);
    s.n_recs = int32_t(f.dicts.size());
    s.tiles = l.dict_tiles;
    return s;
}

ArenaNeeds arena_needs(const BatchPlan& p, uint64_t chars_need, bool twins) {
    ArenaNeeds n{};
    n.out = p.out_bytes;
    // (the window kernels read validity bits in 8-byte words: room for the last one)
    n.bits = std::max<size_t>(p.bits_bytes, 1) + (twins ? 8 : 0);
    n.chars = std::max<size_t>(size_t(2 * p.chars_hint) + (16u << 20), size_t(chars_need));
    return n;
}

bool arenas_grow(const ArenaNeeds& n, const ArenaCaps& c, bool twins) {
    return n.out > c.out || n.bits > c.bits || n.chars > c.chars ||
           (twins && (c.out > c.wout || c.bits > c.wbits || c.chars > c.wchars));
}

CharsOverflow chars_overflow(const BatchPlan& p, const DevChunkResult* r) {
    CharsOverflow o{false, 0};
    for (int c = 0; c < p.n_chunks; c++) {
        if (p.chunks[size_t(c)].ptype != PF_BYTE_ARRAY) continue;
        o.need += align_up(uint64_t(std::max<int64_t>(r[c].num_chars, 0)), 256);
        if (r[c].status == PF_ERR_CAPACITY && r[c].num_chars <= 0x7fffffff) o.rerun = true;
    }
    return o;
}

namespace {
template <class T> T* shifted(T* q, int64_t d) {   // into the twin arena; nullptr stays
    return q ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(q) + uintptr_t(d)) : nullptr;
}
}  // namespace

FirstError assemble_info(const BatchPlan& p, const BatchResults& in, pf_column_info* info, pf_selection_info* sel_info,
                         pf_dict_info* dinfo) {
    FirstError err;
    const DevChunkResult* r = in.res;
    size_t wi = 0;
    if (in.sel_head && p.n_chunks > 0) {
        *sel_info = pf_selection_info{};
        sel_info->rows_in = in.sel_head->rows_in;
        sel_info->rows_selected = in.sel_head->rows_selected;
        sel_info->d_rows = in.sel_rows;
        sel_info->status = in.sel_head->status;
    }
    for (int c = 0; c < p.n_chunks; c++) {
        pf_column_info& ci = info[c];
        const DevChunk& ck = p.chunks[size_t(c)];
        const int32_t k = p.keep_of.empty() ? -1 : p.keep_of[size_t(c)];
        // (a kept chunk is a fixed-width column of index_width bytes in every view: no offsets, no chars)
        const bool ba = ck.ptype == PF_BYTE_ARRAY && k < 0;
        ci.num_entries = ck.num_entries;
        ci.num_slots = r[c].num_slots;
        ci.num_values = r[c].num_values;
        ci.num_rows = r[c].num_rows;
        ci.num_chars = ba ? r[c].num_chars : 0;
        ci.width = ck.width;
        ci.status = r[c].status;
        ci.d_values = ck.values;
        ci.d_validity = ck.validity;
        ci.d_offsets = ck.offsets;
        ci.d_chars = in.dev_chunks[c].chars;
        ci.d_list_offsets = ck.list_offsets;
        ci.d_list_validity = ck.list_validity;
        ci.d_def_levels = ck.def_levels;
        ci.d_rep_levels = ck.rep_levels;
        if (dinfo) dinfo[c] = pf_dict_info{};
        if (k >= 0) {   // kept dictionary: `values` are indices; the dictionary has the chars
            const KeepPlan& kp = p.keeps[size_t(k)];
            ci.width = kp.index_width;
            ci.num_chars = 0;
            ci.d_offsets = nullptr;
            ci.d_chars = nullptr;
            if (dinfo) {
                pf_dict_info& di = dinfo[c];
                di.kept = 1;
                di.index_width = kp.index_width;
                di.n_entries = kp.n_entries;
                di.width = kp.width;
                if (size_t(k) < p.dkeeps.size()) {
                    di.d_values = p.dkeeps[size_t(k)].d_values;
                    di.d_offsets = p.dkeeps[size_t(k)].d_offsets;
                }
                if (in.keeps && kp.width == 0) {
                    di.num_chars = std::max<int64_t>(in.keeps[k].num_chars, 0);
                    di.d_chars = in.keeps[k].d_chars;
                }
            }
        }
        if (wi < in.n_wins && in.wins[wi].chunk == c) {   // the window's view (chunks ascend in wins)
            const DevWinRes& w = in.wres[wi++];
            if (ci.status == 0 && w.status != 0) ci.status = w.status;
            else if (ci.status == 0 && !w.identity) {
                const int64_t od = in.twin.out, bd = in.twin.bits;
                ci.num_entries = w.n_entries;
                ci.num_slots = w.n_slots;
                ci.num_values = w.n_values;
                ci.num_rows = w.n_rows;
                ci.num_chars = ba ? w.n_chars : 0;
                ci.d_values = shifted(ck.values, od);
                ci.d_validity = shifted(ck.validity, bd);
                ci.d_offsets = k < 0 ? shifted(ck.offsets, od) : nullptr;
                ci.d_chars = k < 0 ? w.chars_dst : nullptr;
                ci.d_list_offsets = shifted(ck.list_offsets, od);
                ci.d_list_validity = shifted(ck.list_validity, bd);
                ci.d_def_levels = shifted(ck.def_levels, od);
                ci.d_rep_levels = shifted(ck.rep_levels, od);
            }
        }
        if (in.sel_head) {   // the selection's view
            const DevSelChunk& sc = in.sel_chunks[c];
            if (ci.status == 0 && sc.status != 0) ci.status = sc.status;   // (its own, or a predicate chunk's)
            else if (ci.status == 0) {
                ci.num_entries = ci.num_slots = ci.num_rows = in.sel_head->rows_selected;
                ci.num_values = sc.n_values;
                ci.num_chars = ba ? sc.n_chars : 0;
                ci.d_values = sc.o_values;
                ci.d_validity = sc.o_validity;
                ci.d_offsets = k < 0 ? sc.o_offsets : nullptr;
                ci.d_chars = k < 0 ? sc.o_chars : nullptr;
            }
        }
        if (ci.status != 0 && err.code == PF_OK) {
            err.code = ci.status;
            char buf[160];
            std::snprintf(buf, sizeof buf, "chunk %d: decode failed (status %d, page %d)", c, ci.status, r[c].err_page);
            err.msg = buf;
        }
    }
    return err;
}

BatchLayout batch_layout(const BatchPlan& p, const std::vector<pf_column_info>& info, const void* d_chars,
                         const std::vector<pf_dict_info>* dicts) {
    BatchLayout b{};
    b.out = p.out_bytes;
    b.bits_off = align_up(b.out, 256);
    b.bits = p.bits_bytes;
    b.chars_off = align_up(b.bits_off + b.bits, 256);
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(d_chars);
    size_t hi = 0, bound = 0;
    for (const pf_column_info& ci : info) {
        if (ci.d_chars && ci.num_chars > 0) {
            hi = std::max(hi, size_t(reinterpret_cast<uintptr_t>(ci.d_chars) - c0) + size_t(ci.num_chars));
            bound += align_up(size_t(ci.num_chars), 256);
        }
    }
    if (dicts)
        for (const pf_dict_info& di : *dicts)
            if (di.kept && di.d_chars && di.num_chars > 0) {
                hi = std::max(hi, size_t(reinterpret_cast<uintptr_t>(di.d_chars) - c0) + size_t(di.num_chars));
                bound += align_up(size_t(di.num_chars), 256);
            }
    b.chars = hi;   // bytes copied: the arena's used extent (depends on the order k_scan placed the chunks)
    // buffer size: an order-independent bound, so equal batches always need equal buffers
    b.total = b.chars_off + std::max(hi, bound);
    return b;
}

const void* rebase(const BatchLayout& b, const ArenaPtrs& a, const void* host, const void* q0) {
    if (!q0) return nullptr;
    const uintptr_t q = reinterpret_cast<uintptr_t>(q0), h = reinterpret_cast<uintptr_t>(host);
    const uintptr_t o = reinterpret_cast<uintptr_t>(a.out), v = reinterpret_cast<uintptr_t>(a.bits),
                    c = reinterpret_cast<uintptr_t>(a.chars);
    if (q >= o && q <= o + b.out) return reinterpret_cast<const void*>(h + (q - o));
    if (q >= v && q <= v + b.bits) return reinterpret_cast<const void*>(h + b.bits_off + (q - v));
    if (q >= c && q <= c + b.chars) return reinterpret_cast<const void*>(h + b.chars_off + (q - c));
    return nullptr;
}

pf_column_info rebase_info(const BatchLayout& b, const ArenaPtrs& a, const void* host, pf_column_info ci) {
    auto rb = [&](auto*& q) { q = static_cast<std::remove_reference_t<decltype(q)>>(rebase(b, a, host, q)); };
    rb(ci.d_values);
    rb(ci.d_validity);
    rb(ci.d_offsets);
    rb(ci.d_chars);
    rb(ci.d_list_offsets);
    rb(ci.d_list_validity);
    rb(ci.d_def_levels);
    rb(ci.d_rep_levels);
    return ci;
}

pf_dict_info rebase_dict(const BatchLayout& b, const ArenaPtrs& a, const void* host, pf_dict_info di) {
    di.d_values = rebase(b, a, host, di.d_values);
    di.d_offsets = static_cast<const int32_t*>(rebase(b, a, host, di.d_offsets));
    di.d_chars = static_cast<const uint8_t*>(rebase(b, a, host, di.d_chars));
    return di;
}

void dict_copy_items(const pf_dict_info& di, const pf_column_out& o, CopyItem it[3]) {
    it[0] = {o.values, o.values_cap, di.d_values, size_t(di.n_entries) * size_t(di.width)};
    it[1] = {o.offsets, o.offsets_cap, di.d_offsets, di.d_offsets ? 4 * size_t(di.n_entries + 1) : 0};
    it[2] = {o.chars, o.chars_cap, di.d_chars, size_t(di.num_chars)};
}

void copy_items(const pf_column_info& ci, const pf_column_out& o, CopyItem it[8]) {
    it[0] = {o.values, o.values_cap, ci.d_values, size_t(ci.num_slots) * size_t(ci.width)};
    it[1] = {o.validity, o.validity_cap, ci.d_validity, size_t((ci.num_slots + 7) / 8)};
    it[2] = {o.offsets, o.offsets_cap, ci.d_offsets, ci.d_offsets ? 4 * size_t(ci.num_slots + 1) : 0};
    it[3] = {o.chars, o.chars_cap, ci.d_chars, size_t(ci.num_chars)};
    it[4] = {o.list_offsets, o.list_offsets_cap, ci.d_list_offsets, ci.d_list_offsets ? 4 * size_t(ci.num_rows + 1) : 0};
    it[5] = {o.list_validity, o.list_validity_cap, ci.d_list_validity, size_t((ci.num_rows + 7) / 8)};
    it[6] = {o.def_levels, o.def_levels_cap, ci.d_def_levels, size_t(ci.num_entries)};
    it[7] = {o.rep_levels, o.rep_levels_cap, ci.d_rep_levels, size_t(ci.num_entries)};
}

}  // namespace pf
