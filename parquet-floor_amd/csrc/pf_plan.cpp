// pf_plan.cpp — host-only planning of one decode batch (pf_plan.h).
#include "pf_plan.h"

#include <algorithm>

namespace pf {

namespace {
size_t take(size_t& cursor, size_t n, size_t a = 256) {
    size_t o = align_up(cursor, a);
    cursor = o + n;
    return o;
}
bool dict_encoded(int e) { return e == PF_ENC_PLAIN_DICTIONARY || e == PF_ENC_RLE_DICTIONARY; }
bool int_type(int t) { return t == PF_INT32 || t == PF_INT64; }
}  // namespace

bool keep_eligible(const pf_chunk_desc& cd) {
    if (cd.max_rep != 0 || cd.physical_type == PF_BOOLEAN || cd.n_pages <= 0 || !cd.pages) return false;
    int n_dict = 0, n_data = 0;
    for (int i = 0; i < cd.n_pages; i++) {
        const pf_page_desc& pd = cd.pages[i];
        if (pd.page_type == PF_PAGE_DICTIONARY) { n_dict++; continue; }
        if (pd.page_type != PF_PAGE_DATA && pd.page_type != PF_PAGE_DATA_V2) continue;   // index pages
        if (!dict_encoded(pd.encoding)) return false;
        n_data++;
    }
    return n_dict > 0 && n_data > 0;
}

int type_width(int ptype, int type_length) {
    switch (ptype) {
    case PF_BOOLEAN: return 1;
    case PF_INT32: case PF_FLOAT: return 4;
    case PF_INT64: case PF_DOUBLE: return 8;
    case PF_INT96: return 12;
    case PF_BYTE_ARRAY: return 0;
    case PF_FIXED_LEN_BYTE_ARRAY: return type_length > 0 ? type_length : -1;
    default: return -1;
    }
}

void plan_snappy(std::vector<SnappyJob>& jobs, SnappyPlan& sp) {
    sp.n_splits = 0;
    sp.max_snap_win = 1;
    uint32_t n_win = 0;
    size_t tw = 0, tp = 0;
    for (SnappyJob& jb : jobs) {
        jb.n_win = std::max<uint32_t>(1u, uint32_t((uint64_t(jb.src_len) + SNAP_WIN - 1) / SNAP_WIN));
        sp.max_snap_win = std::max(sp.max_snap_win, int(std::min<uint32_t>(jb.n_win, 1u << 20)));
        jb.n_pieces = std::max<uint32_t>(1u, uint32_t((uint64_t(jb.dst_len) + SNAP_BLOCK - 1) / SNAP_BLOCK));
        tw += jb.n_win;
        tp += jb.n_pieces;
    }
    sp.wins.resize(tw);
    sp.pieces.resize(tp);
    // Dispatch the pieces with the most compressed bytes per 64 KiB of output first (more tokens per
    // piece -> more executor steps), so the longest pieces do not start last (k_snappy_exec alone
    // 1.50 -> 1.39 ms per launch on SF1).
    std::vector<uint64_t> keyed(tp);
    size_t wi = 0, pi = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        SnappyJob& jb = jobs[j];
        jb.win_base = n_win;
        for (uint32_t w = 0; w < jb.n_win; w++) sp.wins[wi++] = Int2{int(j), int(w)};
        n_win += jb.n_win;
        jb.split_base = sp.n_splits;
        sp.n_splits += jb.n_pieces;
        const uint64_t cost = uint64_t(jb.src_len) / jb.n_pieces;   // compressed bytes per piece
        for (uint32_t k = 0; k < jb.n_pieces; k++) {
            keyed[pi] = (std::min<uint64_t>(cost, 0xffffffffull) << 32) | uint64_t(pi);
            sp.pieces[pi++] = Int2{int(j), int(k)};
        }
    }
    {   // descending cost in 64-byte buckets (counting sort: O(pieces)), ties in page order
        constexpr uint32_t NB = 4096;
        std::vector<uint32_t> start(NB + 1, 0);
        auto bucket = [](uint64_t k) { return NB - 1 - uint32_t(std::min<uint64_t>((k >> 32) >> 6, NB - 1)); };
        for (size_t i = 0; i < tp; i++) start[bucket(keyed[i]) + 1]++;
        for (uint32_t b = 0; b < NB; b++) start[b + 1] += start[b];
        std::vector<Int2> sorted(tp);
        for (size_t i = 0; i < tp; i++) sorted[start[bucket(keyed[i])]++] = sp.pieces[size_t(uint32_t(keyed[i]))];
        sp.pieces.swap(sorted);
    }
    const size_t tok_bytes = size_t(n_win) * SNAP_WWORDS * 4, lo_bytes = size_t(n_win) * 64 * 4;
    const size_t win_bytes = align_up(size_t(n_win) * sizeof(SnapWin), 256), ent_bytes = size_t(n_win) * 64 * sizeof(SnapEnt);
    sp.off_lane_out = tok_bytes;
    sp.off_win = tok_bytes + lo_bytes;
    sp.off_ent = tok_bytes + lo_bytes + win_bytes;
    sp.tokmap_bytes = tok_bytes + lo_bytes + win_bytes + ent_bytes + 256;
}

void bind_snappy(std::vector<SnappyJob>& jobs, SnappyPlan& sp, uintptr_t tokmap) {
    sp.d_lane_out = reinterpret_cast<uint32_t*>(tokmap + sp.off_lane_out);
    sp.d_win = reinterpret_cast<SnapWin*>(tokmap + sp.off_win);
    sp.d_ent = reinterpret_cast<SnapEnt*>(tokmap + sp.off_ent);
    for (SnappyJob& jb : jobs) jb.tokmap = reinterpret_cast<uint32_t*>(tokmap + size_t(jb.win_base) * SNAP_WWORDS * 4);
}

namespace {

// The chunk's DevChunk, its pages, their scratch regions and Snappy jobs, its output arrays.
// A chunk that fails validation keeps its status and loses its pages and jobs.
void plan_chunk(const pf_chunk_desc& cd, int c, size_t n_bytes, const PfOpts& opts, BatchPlan& p, uint64_t& nest_pub,
                bool want_keep) {
    // nested pages: entries per segment (k_nest_*); PF_NEST_SEG=n (tests) sets it and sends every
    // eligible nested page, one segment or more, down the segment path (0: none)
    int64_t nest_seg_len = NEST_SEG;
    bool nest_seg_forced = false;
    if (opts.nest_seg_set) {
        nest_seg_len = opts.nest_seg;
        nest_seg_forced = nest_seg_len > 0;
        if (nest_seg_len <= 0) nest_seg_len = int64_t(1) << 40;   // every page stays on k_count / k_decode
    }
    DevChunk& ck = p.chunks[size_t(c)];
    ck.ptype = cd.physical_type; ck.type_length = cd.type_length;
    ck.width = type_width(cd.physical_type, cd.type_length);
    ck.max_def = cd.max_def; ck.max_rep = cd.max_rep; ck.repeated_def = cd.repeated_def;
    ck.list_null_def = cd.list_null_def; ck.codec = cd.codec;
    ck.dict_page = -1;
    ck.first_page = int(p.pages.size());
    int64_t& hs = p.host_status[size_t(c)];
    if (ck.width < 0) hs = PF_ERR_UNSUPPORTED_TYPE;
    else if (cd.codec != PF_CODEC_UNCOMPRESSED && cd.codec != PF_CODEC_SNAPPY && cd.codec != PF_CODEC_ZSTD &&
             cd.codec != PF_CODEC_LZ4_RAW)
        hs = PF_ERR_UNSUPPORTED_CODEC;
    else if (cd.max_def < 0 || cd.max_def > 255 || cd.max_rep < 0 || cd.max_rep > 255 || cd.n_pages < 0 ||
             (cd.n_pages > 0 && !cd.pages) || cd.chunk_offset + cd.chunk_size > n_bytes)
        hs = PF_ERR_INVALID_ARG;
    // kept dictionary: indices + dictionary instead of values (the rule reads the descriptors only; a chunk that
    // fails validation fails as ever)
    const bool kept = want_keep && hs == 0 && keep_eligible(cd);
    ck.needs_count = (!kept && (cd.physical_type == PF_BYTE_ARRAY || cd.max_rep > 0)) ? 1 : 0;
    int64_t entries = 0;
    int dict_global = -1;
    size_t& scratch = p.scratch_bytes;
    if (hs == 0) {
        for (int i = 0; i < cd.n_pages; i++) {
            const pf_page_desc& pd = cd.pages[i];
            if (pd.offset + pd.compressed_size > cd.chunk_size) { hs = PF_ERR_CORRUPT_PAGE; break; }
            if (pd.uncompressed_size > (1u << 29) || pd.compressed_size > (1u << 30)) { hs = PF_ERR_CORRUPT_PAGE; break; }
            bool is_dict = pd.page_type == PF_PAGE_DICTIONARY;
            bool v2 = pd.page_type == PF_PAGE_DATA_V2;
            if (!is_dict && pd.page_type != PF_PAGE_DATA && !v2) continue;   // index pages
            if (is_dict && (dict_global >= 0 || ck.n_pages > 0)) { hs = PF_ERR_CORRUPT_PAGE; break; }
            DevPage pg{};
            pg.chunk = c;
            pg.ba_job = -1;
            pg.encoding = pd.encoding; pg.def_enc = pd.def_encoding; pg.rep_enc = pd.rep_encoding;
            pg.num_values = pd.num_values;
            pg.flags = (v2 ? PG_V2 : 0) | (is_dict ? PG_DICT : 0);
            if (pd.num_values < 0) { hs = PF_ERR_CORRUPT_PAGE; break; }
            uint32_t lvl = v2 ? uint32_t(pd.rep_bytes) + uint32_t(pd.def_bytes) : 0;
            if (v2 && (pd.rep_bytes < 0 || pd.def_bytes < 0 || lvl > pd.compressed_size || lvl > pd.uncompressed_size)) {
                hs = PF_ERR_CORRUPT_PAGE; break;
            }
            bool compressed = cd.codec != PF_CODEC_UNCOMPRESSED && (!v2 || pd.is_compressed);
            PagePlan pp{cd.chunk_offset + pd.offset, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF};
            if (v2) { pg.rep_len = uint32_t(pd.rep_bytes); pg.def_len = uint32_t(pd.def_bytes); }
            if (compressed) {
                pp.scratch_off = take(scratch, pd.uncompressed_size - lvl, 16);
                pg.flags |= PG_COMPRESSED;
                pg.body_len = pd.uncompressed_size - lvl;
                if (cd.codec == PF_CODEC_ZSTD) {
                    ZstdJob j{};
                    j.src_len = pd.compressed_size - lvl; j.dst_len = pd.uncompressed_size - lvl;
                    j.page = int(p.pages.size()); j.chunk = c;
                    j.exact = 1;
                    p.zjobs.push_back(j);
                } else if (cd.codec == PF_CODEC_LZ4_RAW) {
                    Lz4Job j{};
                    j.src_len = pd.compressed_size - lvl; j.dst_len = pd.uncompressed_size - lvl;
                    j.page = int(p.pages.size()); j.chunk = c;
                    if (j.src_len || j.dst_len) p.ljobs.push_back(j);   // (an empty section stored as no bytes: nothing to do)
                } else {
                    SnappyJob j{};
                    j.src_len = pd.compressed_size - lvl; j.dst_len = pd.uncompressed_size - lvl;
                    j.page = int(p.pages.size()); j.chunk = c;
                    p.jobs.push_back(j);
                }
            } else {
                pg.body_len = pd.compressed_size - lvl;
            }
            if (is_dict) {
                dict_global = int(p.pages.size());
                ck.dict_page = dict_global;
                ck.dict_n = pd.num_values;
                if (pd.encoding != PF_ENC_PLAIN && pd.encoding != PF_ENC_PLAIN_DICTIONARY) { hs = PF_ERR_UNSUPPORTED_ENCODING; break; }
                if (cd.physical_type == PF_BOOLEAN) { hs = PF_ERR_UNSUPPORTED_ENCODING; break; }
                if (cd.physical_type == PF_BYTE_ARRAY) {   // pos + len of every entry
                    pp.aux_off = take(scratch, 8ull * (pd.num_values + 1), 256);
                    pg.aux_cap = pg.num_values;
                } else if (uint64_t(pd.num_values) * ck.width > pg.body_len) { hs = PF_ERR_CORRUPT_PAGE; break; }
            } else {
                pg.entry_start = entries;
                entries += pd.num_values;
                ck.n_pages++;
                // FIXED_LEN_BYTE_ARRAY in DELTA_BYTE_ARRAY (parquet-mr's v2 writer after a dictionary fallback)
                const bool flba_dba = cd.physical_type == PF_FIXED_LEN_BYTE_ARRAY && pd.encoding == PF_ENC_DELTA_BYTE_ARRAY;
                if (kept) {
                    // (k_flat_ids reads the id stream through k_runs' table: no value positions, no chars)
                } else if (cd.physical_type == PF_BYTE_ARRAY)   // value positions / ids + per-block chars (k_flat)
                    pp.aux_off = take(scratch, aux_chars_bytes(uint64_t(pd.num_values)), 256);
                else if (flba_dba)   // slot of every present value (decode_page -> k_dba_chars)
                    pp.aux_off = take(scratch, 4ull * pd.num_values + 16, 256);
                else if (pd.encoding == PF_ENC_DELTA_BINARY_PACKED && int_type(cd.physical_type)) {
                    pp.aux_off = take(scratch, 8ull * pd.num_values + 8, 256);
                    // block-parallel decode (k_dbp_*); PF_DBP_PAR=0: every page on the one-workgroup k_delta (tests)
                    if (pd.num_values >= DBP_PAR_MIN && opts.dbp_par) {
                        pg.dbp_bcap = uint32_t(pd.num_values / 8 + 2);
                        pp.dbp_off = take(scratch, dbp_bytes(pg.dbp_bcap), 256);
                        pg.dbp_nwin = int32_t((uint64_t(std::max(pd.uncompressed_size, pd.compressed_size)) + DBP_WIN - 1) / DBP_WIN + 1);
                        pp.dbp_pub_off = nest_pub;
                        nest_pub += uint64_t(pg.dbp_nwin) * sizeof(WinPub);
                    }
                }
                if (pp.aux_off != NO_OFF) pg.aux_cap = pg.num_values;
                if (cd.physical_type == PF_BYTE_ARRAY && !kept) p.chars_hint += pd.uncompressed_size;
                if (flba_dba || (cd.physical_type == PF_BYTE_ARRAY &&
                                 (pd.encoding == PF_ENC_DELTA_LENGTH_BYTE_ARRAY || pd.encoding == PF_ENC_DELTA_BYTE_ARRAY)))
                    pp.dx_off = take(scratch, dx_bytes(uint64_t(pd.num_values)), 256);   // k_dlen
                if (cd.max_rep == 0 && cd.physical_type != PF_BOOLEAN && dict_encoded(pd.encoding))
                    pp.rt_off = take(scratch, RT_BYTES, 256);   // k_runs table
                if (cd.max_rep == 0 && cd.max_def > 0 && cd.physical_type != PF_BOOLEAN &&
                    (cd.physical_type != PF_BYTE_ARRAY || kept) && pd.num_nulls != 0 &&   // v2 header / v1 page statistics say when no level is null (-1: unknown)
                    (pd.encoding == PF_ENC_PLAIN || dict_encoded(pd.encoding))) {
                    pp.lt_off = take(scratch, lvl_table_bytes(pg.num_values), 256);   // k_lvl tables
                    pg.lvl_cap = lvl_table_cap(pg.num_values);
                }
                {   // nested pages decoded in segments (k_nest_*): PLAIN fixed width, dictionary, DELTA_BINARY_PACKED ints
                    const int e = pd.encoding;
                    const bool enc_ok = (e == PF_ENC_PLAIN && cd.physical_type != PF_BYTE_ARRAY) || dict_encoded(e) ||
                                        (e == PF_ENC_DELTA_BINARY_PACKED && int_type(cd.physical_type));
                    if (cd.max_rep > 0 && cd.physical_type != PF_BOOLEAN && enc_ok && pd.num_values > 0) {
                        const int64_t sl = std::max<int64_t>(nest_seg_len, (int64_t(pd.num_values) + NEST_MAX_SEGS - 1) / NEST_MAX_SEGS);
                        const int64_t ns = (int64_t(pd.num_values) + sl - 1) / sl;
                        if (ns >= 2 || nest_seg_forced) {
                            pg.seg_len = int32_t(sl);
                            pg.nseg = int32_t(ns);
                            pp.seg_off = take(scratch, nest_seg_bytes(pg.nseg), 256);
                            // windows over the longer level stream (v2: its length is in the header; v1: the page bounds it)
                            const uint64_t lvl_bytes = v2 ? uint64_t(std::max(pd.rep_bytes, pd.def_bytes))
                                                          : uint64_t(std::max(pd.uncompressed_size, pd.compressed_size));
                            pg.nwin = int32_t((lvl_bytes + NEST_WIN - 1) / NEST_WIN + 1);
                            pp.pub_off = nest_pub;   // (the window hand-overs of all pages: one block, zeroed per batch)
                            nest_pub += 2ull * uint64_t(pg.nwin) * sizeof(WinPub);
                        }
                    }
                }
            }
            p.pplan.push_back(pp);
            p.pages.push_back(pg);
        }
    }
    if (hs != 0) {   // drop this chunk's pages and jobs
        while (int(p.pages.size()) > ck.first_page) { p.pages.pop_back(); p.pplan.pop_back(); }
        while (!p.jobs.empty() && p.jobs.back().chunk == c) p.jobs.pop_back();
        while (!p.zjobs.empty() && p.zjobs.back().chunk == c) p.zjobs.pop_back();
        while (!p.ljobs.empty() && p.ljobs.back().chunk == c) p.ljobs.pop_back();
        ck.n_pages = 0; ck.dict_page = -1; entries = 0;
    }
    if (ck.dict_page >= 0) ck.first_page = ck.dict_page + 1;
    ck.num_entries = entries;
    OutPlan& op = p.oplan[size_t(c)];
    op = OutPlan{NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF, NO_OFF};
    if (hs == 0 && kept) {   // indices, validity, and the dictionary's own arrays
        size_t &out = p.out_bytes, &bits = p.bits_bytes;
        KeepPlan kp{c, dict_index_width(ck.dict_n), ck.dict_n, ck.width, NO_OFF, NO_OFF};
        op.values = take(out, size_t(entries) * size_t(kp.index_width));
        if (cd.max_def > 0) op.validity = take(bits, align_up((entries + 7) / 8, 4), 256);
        if (ck.width > 0) kp.values = take(out, size_t(kp.n_entries) * size_t(ck.width));
        else {
            kp.offsets = take(out, 4 * size_t(kp.n_entries + 1));
            p.chars_hint += p.pages[size_t(ck.dict_page)].body_len;   // (the dictionary's chars are in the chars arena)
        }
        p.keep_of[size_t(c)] = int32_t(p.keeps.size());
        p.keeps.push_back(kp);
    } else if (hs == 0) {
        size_t &out = p.out_bytes, &bits = p.bits_bytes;
        if (ck.width > 0) op.values = take(out, size_t(entries) * ck.width);
        if (cd.max_def > 0) op.validity = take(bits, align_up((entries + 7) / 8, 4), 256);
        if (cd.physical_type == PF_BYTE_ARRAY) op.offsets = take(out, 4 * size_t(entries + 1));
        if (cd.max_rep == 1) {
            op.list_offsets = take(out, 4 * size_t(entries + 1));
            op.list_validity = take(bits, align_up((entries + 7) / 8, 4), 256);
        }
        if (cd.max_rep > 0) { op.def = take(out, entries); op.rep = take(out, entries); }
    }
}

// PLAIN BYTE_ARRAY walk jobs: dictionary pages first, then PLAIN data pages.
void plan_ba_walks(BatchPlan& p) {
    for (int pass = 0; pass < 2; pass++) {
        for (size_t i = 0; i < p.pages.size(); i++) {
            DevPage& pg = p.pages[i];
            const DevChunk& ck = p.chunks[size_t(pg.chunk)];
            if (ck.ptype != PF_BYTE_ARRAY || p.host_status[size_t(pg.chunk)] != 0) continue;
            const bool is_dict = pg.flags & PG_DICT;
            if (pass == 0 ? !is_dict : (is_dict || pg.encoding != PF_ENC_PLAIN)) continue;
            BaJob J{};
            J.n_cap = pg.body_len;
            J.n_tiles = std::max<uint32_t>(1u, (pg.body_len + BA_TILE - 1) / BA_TILE);
            J.chunk = pg.chunk;
            J.page = int32_t(i);
            J.state = BA_SKIP;
            if (pass == 0) {
                J.n = pg.body_len;
                J.count = ck.dict_n;
                J.state = ck.dict_n > 0 ? BA_OK : BA_SKIP;
            }   // (data pages: n, count, state by k_count)
            const size_t words = size_t(J.n_tiles) * (BA_TILE / 32);
            p.ba_bm.push_back(take(p.scratch_bytes, 4 * (3 * words + J.n_tiles), 256));
            const int rel = int(p.bajobs.size()) - (pass == 0 ? 0 : p.n_ba_dict);
            for (uint32_t t = 0; t < J.n_tiles; t++) p.ba_tiles.push_back(Int2{rel, int(t)});
            if (pass == 1) pg.ba_job = int32_t(p.bajobs.size());
            if (uint64_t(pg.body_len) > BA_SHORT * uint64_t(std::max<int64_t>(1, pg.num_values)))
                (pass == 0 ? p.ba_short_dict : p.ba_short_data) = false;
            p.bajobs.push_back(J);
        }
        if (pass == 0) { p.n_ba_dict = int(p.bajobs.size()); p.n_ba_dict_tiles = int(p.ba_tiles.size()); }
    }
}

// Per-page lists of the table kernels, and what k_flat_null's LDS stages have to hold.
void plan_page_tables(BatchPlan& p) {
    for (size_t i = 0; i < p.pages.size(); i++) {
        const DevPage& pg = p.pages[i];
        const PagePlan& pp = p.pplan[i];
        if (pp.rt_off != NO_OFF) p.lists[L_RUNS].push_back(int(i));
        if (pp.lt_off != NO_OFF) {
            p.lists[L_LVL].push_back(int(i));
            const DevChunk& lc = p.chunks[size_t(pg.chunk)];
            const uint64_t db = uint64_t(std::max<int64_t>(lc.dict_n, 0)) * uint64_t(std::max(lc.width, 0));
            if (lc.dict_page >= 0 && db > 0 && db <= NULL_DICT_LDS && p.keep_of[size_t(pg.chunk)] < 0)
                p.null_caps.dlds = std::max(p.null_caps.dlds, uint32_t(align_up(db, 256)));
            // level / id byte stages: FBLK values of the level width / the dictionary's id width
            // (bit width of its largest index, as writers choose it) + run headers
            auto bits = [](uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; };
            // hybrid worst case: bit-packed, FBLK * b / 8 bytes + headers; or RLE runs of
            // 8 repeats, a header byte + ceil(b / 8) value bytes per 8 entries (1-bit levels: 1 KiB)
            auto cap = [](int b, uint32_t most) {
                const uint64_t bp = uint64_t(FBLK) * uint64_t(b) / 8;
                const uint64_t rle = uint64_t(FBLK) / 8 * (1 + (uint64_t(b) + 7) / 8);
                return uint32_t(std::min<uint64_t>(most, align_up(std::max(bp, rle) + NL_SLACK, 16)));
            };
            p.null_caps.dcap = std::max(p.null_caps.dcap, cap(bits(uint64_t(std::max(lc.max_def, 0))), NL_DST));
            if (lc.dict_page >= 0)
                p.null_caps.icap = std::max(p.null_caps.icap, cap(bits(uint64_t(std::max<int64_t>(lc.dict_n, 1) - 1)), NL_IST));
        }
        if (pp.dbp_off != NO_OFF) p.max_dbp_nwin = std::max(p.max_dbp_nwin, pg.dbp_nwin);
        if (pp.seg_off != NO_OFF) {
            p.max_nwin = std::max(p.max_nwin, pg.nwin);
            p.lists[L_NEST].push_back(int(i));
            for (int k = 0; k < pg.nseg; k++) { p.lists[L_NSEG].push_back(int(i)); p.lists[L_NSEG].push_back(k); }
        }
        if (pp.dx_off != NO_OFF) {
            p.lists[L_DLEN].push_back(int(i));
            if (pg.encoding == PF_ENC_DELTA_BYTE_ARRAY) p.lists[L_DBA].push_back(int(i));
        }
    }
    for (int c = 0; c < p.n_chunks; c++)
        if (p.host_status[size_t(c)] == 0 && p.chunks[size_t(c)].needs_count) p.lists[L_SCAN].push_back(c);
}

// The page lists of k_delta, k_count and k_decode, and the (page, block) pairs of the flat kernels.
// A chunk with a large dictionary keeps all its blocks on one blockIdx % 8 label (the dispatcher's
// XCD group, MI355X_MICROARCH.md), so the dictionary is gathered through one XCD's L2 instead of
// all eight (config 4: 400 KB dictionaries); such chunks go to the least loaded label, all other
// blocks then fill the labels evenly. Labels are interleaved into the grid; short ones are padded
// with (-1, 0).
// Four such grids, one after the other in L_FLAT: fixed-width pages (k_flat_fixed), the other flat
// pages (k_flat_all), then the blocks of nullable 4- and 8-byte pages (k_flat_null<4> / <8>);
// k_flat_fixed and k_flat_null queue what they do not take for k_flat_all's last workgroups.
void plan_routes(const PfOpts& opts, BatchPlan& p) {
    const int n_chunks = p.n_chunks;
    std::vector<int> spread[4];
    std::vector<std::vector<int>> sticky[4];
    for (auto& v : sticky) v.resize(static_cast<size_t>(n_chunks));
    std::vector<int> decode_first, count_rest;
    std::vector<int>&l_count = p.lists[L_COUNT], &l_decode = p.lists[L_DECODE], &l_flat = p.lists[L_FLAT];
    for (size_t i = 0; i < p.pages.size(); i++) {
        const DevPage& pg = p.pages[i];
        const PagePlan& pp = p.pplan[i];
        if (pg.flags & PG_DICT) continue;
        const DevChunk& ck = p.chunks[size_t(pg.chunk)];
        if (p.keep_of[size_t(pg.chunk)] >= 0) {   // a kept chunk's pages reach k_flat_ids and nothing that expands them
            const int nb = std::max(1, int((int64_t(pg.num_values) + FBLK - 1) / FBLK));
            for (int b = 0; b < nb; b++) { p.lists[L_IDS].push_back(int(i)); p.lists[L_IDS].push_back(b); }
            continue;
        }
        const bool has_lvltab = pp.lt_off != NO_OFF;
        if (pg.encoding == PF_ENC_DELTA_BINARY_PACKED && pp.aux_off != NO_OFF && ck.ptype != PF_BYTE_ARRAY)
            p.lists[L_DELTA].push_back(int(i));
        if (ck.needs_count) (ck.ptype == PF_BYTE_ARRAY && ck.max_rep == 0 ? l_count : count_rest).push_back(int(i));
        if (ck.ptype == PF_BYTE_ARRAY && ck.max_rep == 0 && pp.rt_off != NO_OFF && dict_encoded(pg.encoding)) {
            const int nb = std::max(1, int((int64_t(pg.num_values) + FBLK - 1) / FBLK));
            for (int b = 0; b < nb; b++) { p.lists[L_CDICT].push_back(int(i)); p.lists[L_CDICT].push_back(b); }
        }
        if (ck.max_rep == 0) {   // (page, block) pairs
            // fixed-width pages without a level table (no nulls) take blocks of FBLK << fix_shift
            // entries (the block index carries the shift in bits 28..31): a block's metadata chain and
            // run-table load are paid once per 8192 entries instead of per 4096 (PF_FIX_BLK=4096|8192|16384)
            const int sh = (ck.ptype != PF_BYTE_ARRAY && !has_lvltab) ? opts.fix_shift : 0;
            const int64_t bsz = int64_t(FBLK) << sh;
            const int nb = std::max(1, int((int64_t(pg.num_values) + bsz - 1) / bsz));
            const bool dict_enc = dict_encoded(pg.encoding);
            const bool big_dict = ck.dict_page >= 0 && p.pages[size_t(ck.dict_page)].body_len > STICKY_DICT && dict_enc;
            const int grid = (has_lvltab && ck.ptype != PF_BYTE_ARRAY && (dict_enc || pg.encoding == PF_ENC_PLAIN))
                                 ? (ck.width == 4 ? 2 : (ck.width == 8 ? 3 : 1))
                                 : (ck.ptype != PF_BYTE_ARRAY ? 0 : 1);
            std::vector<int>& q = big_dict ? sticky[grid][size_t(pg.chunk)] : spread[grid];
            for (int b = 0; b < nb; b++) { q.push_back(int(i)); q.push_back(b | (sh << 28)); }
        }
        // k_decode does the pages the flat kernels do not take: nested pages and encodings other than
        // PLAIN / dictionary / DELTA_BINARY_PACKED go first (one block each), the rest are only checked
        const int e = pg.encoding;
        if (ck.max_rep > 0 || !(e == PF_ENC_PLAIN || dict_encoded(e) || e == PF_ENC_DELTA_BINARY_PACKED) || ck.ptype == PF_BOOLEAN)
            decode_first.push_back(int(i));
        else
            l_decode.push_back(int(i));
    }
    p.n_decode_first = int(decode_first.size());
    p.n_count_flat = int(l_count.size());
    l_count.insert(l_count.end(), count_rest.begin(), count_rest.end());
    l_decode.insert(l_decode.begin(), decode_first.begin(), decode_first.end());
    int n_grid[4] = {};
    for (int gi = 0; gi < 4; gi++) {
        std::vector<int> xq[8];
        size_t load[8] = {};
        std::vector<int> order(static_cast<size_t>(n_chunks));
        for (int c = 0; c < n_chunks; c++) order[size_t(c)] = c;
        const auto& sk = sticky[gi];
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sk[size_t(a)].size() > sk[size_t(b)].size(); });
        for (int c : order) {
            if (sk[size_t(c)].empty()) continue;
            const int x = int(std::min_element(load, load + 8) - load);
            xq[x].insert(xq[x].end(), sk[size_t(c)].begin(), sk[size_t(c)].end());
            load[x] += sk[size_t(c)].size() / 2;
        }
        const std::vector<int>& sp = spread[gi];
        for (size_t k = 0; k + 1 < sp.size(); k += 2) {
            const int x = int(std::min_element(load, load + 8) - load);
            xq[x].push_back(sp[k]);
            xq[x].push_back(sp[k + 1]);
            load[x]++;
        }
        const size_t longest = *std::max_element(load, load + 8);
        for (size_t k = 0; k < longest; k++)
            for (int x = 0; x < 8; x++) {
                const bool have = k < load[x];
                l_flat.push_back(have ? xq[x][2 * k] : -1);
                l_flat.push_back(have ? xq[x][2 * k + 1] : 0);
            }
        n_grid[gi] = int(8 * longest);
    }
    p.n_flat_fixed = n_grid[0];
    p.n_flat_all = n_grid[1];
    p.n_null4 = n_grid[2];
    p.n_null8 = n_grid[3];
    // k_snappy_litcopy candidates (k_snappy_head decides): dictionary pages, and data pages that did
    // not compress (a stream of literals only; one literal is read in place instead)
    for (size_t j = 0; j < p.jobs.size(); j++) {
        SnappyJob& jb = p.jobs[j];
        if ((p.pages[size_t(jb.page)].flags & PG_DICT) || jb.src_len >= jb.dst_len) {
            jb.dflags |= 2u;
            p.lists[L_DJOBS].push_back(int(j));
        }
    }
}

// ZSTD jobs: the dispatch order (the most compressed bytes first, so the longest pages do not start
// last; ties in page order) and one literal area per resident workgroup of k_zstd.
void plan_zstd(BatchPlan& p) {
    std::vector<int>& order = p.lists[L_ZSTD];
    uint32_t max_dst = 0;
    for (size_t j = 0; j < p.zjobs.size(); j++) {
        order.push_back(int(j));
        max_dst = std::max(max_dst, p.zjobs[j].dst_len);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.zjobs[size_t(a)].src_len > p.zjobs[size_t(b)].src_len; });
    p.zstd_grid = uint32_t(std::min<size_t>(p.zjobs.size(), size_t(ZSTD_GRID)));
    p.zlit_stride = p.zstd_grid ? zstd_lit_stride(max_dst) : 0;
    p.off_zlit = take(p.scratch_bytes, size_t(p.zstd_grid) * p.zlit_stride, 256);
}

// LZ4 jobs: the dispatch order, as for ZSTD (k_lz4 needs no area of its own).
void plan_lz4(BatchPlan& p) {
    std::vector<int>& order = p.lists[L_LZ4];
    for (size_t j = 0; j < p.ljobs.size(); j++) order.push_back(int(j));
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.ljobs[size_t(a)].src_len > p.ljobs[size_t(b)].src_len; });
}

void plan_meta(BatchPlan& p) {
    size_t m = 0;
    for (int l = 0; l < N_LISTS; l++) p.list_base[l + 1] = p.list_base[l] + p.lists[l].size();
    p.off_chunks = take(m, sizeof(DevChunk) * size_t(p.n_chunks));
    p.off_pages = take(m, sizeof(DevPage) * p.pages.size());
    p.off_jobs = take(m, sizeof(SnappyJob) * p.jobs.size());
    p.off_lists = take(m, sizeof(int) * p.list_base[N_LISTS]);
    p.off_res = take(m, sizeof(DevChunkResult) * size_t(p.n_chunks));
    p.off_pieces = take(m, sizeof(Int2) * p.snap.pieces.size());
    p.off_splits = take(m, sizeof(uint32_t) * p.snap.n_splits);
    p.off_fallback = take(m, sizeof(int) * p.jobs.size());
    p.off_wins = take(m, sizeof(Int2) * p.snap.wins.size());
    p.off_bajobs = take(m, sizeof(BaJob) * p.bajobs.size());
    p.off_batiles = take(m, sizeof(Int2) * p.ba_tiles.size());
    p.off_nfbq = take(m, 16 + sizeof(Int2) * size_t(p.n_flat_fixed + p.n_null4 + p.n_null8), 16);   // fallback queue
    p.off_zjobs = take(m, sizeof(ZstdJob) * p.zjobs.size());
    p.off_ljobs = take(m, sizeof(Lz4Job) * p.ljobs.size());
    p.off_keeps = take(m, sizeof(DevKeep) * p.keeps.size());
    p.off_keepof = take(m, p.keeps.empty() ? 0 : sizeof(int32_t) * size_t(p.n_chunks));
    p.meta_bytes = take(m, 256) + 256;   // arena counter lives in the last 256 bytes
}

}  // namespace

void plan_batch(const pf_chunk_desc* cds, int n_chunks, size_t n_bytes, const PfOpts& opts, BatchPlan& p, const uint8_t* keep) {
    p.n_chunks = n_chunks;
    p.chunks.assign(size_t(n_chunks), DevChunk{});
    p.host_status.assign(size_t(n_chunks), 0);
    p.oplan.resize(size_t(n_chunks));
    p.pages.clear(); p.pplan.clear(); p.jobs.clear(); p.zjobs.clear(); p.ljobs.clear();
    p.bajobs.clear(); p.ba_tiles.clear(); p.ba_bm.clear();
    p.keeps.clear(); p.dkeeps.clear();
    p.keep_of.assign(size_t(n_chunks), -1);
    for (auto& l : p.lists) l.clear();
    p.ba_short_dict = p.ba_short_data = true;
    p.max_nwin = p.max_dbp_nwin = 0;
    p.null_caps = NullCaps{16, 16, 0};
    p.scratch_bytes = p.out_bytes = p.bits_bytes = 0;
    p.chars_hint = 0;
    uint64_t nest_pub = 0;
    for (int c = 0; c < n_chunks; c++) plan_chunk(cds[c], c, n_bytes, opts, p, nest_pub, keep && keep[c]);
    plan_ba_walks(p);
    p.npub_bytes = size_t(nest_pub);
    p.off_npub = take(p.scratch_bytes, p.npub_bytes, 256);
    plan_page_tables(p);
    plan_routes(opts, p);
    plan_snappy(p.jobs, p.snap);
    plan_zstd(p);
    plan_lz4(p);
    plan_meta(p);
}

void bind_batch(BatchPlan& p, const ArenaBases& a) {
    auto at = [](uintptr_t base, uint64_t off) { return off == NO_OFF ? nullptr : reinterpret_cast<uint8_t*>(base + off); };
    auto words = [](uint8_t* b) { return reinterpret_cast<uint32_t*>(b); };
    const uintptr_t S = a.scratch;
    for (size_t i = 0; i < p.pages.size(); i++) {
        DevPage& pg = p.pages[i];
        const PagePlan& pp = p.pplan[i];
        const uint8_t* src = at(a.in, pp.in_off);
        if (pg.flags & PG_V2) pg.lvl = src;
        pg.body = (pg.flags & PG_COMPRESSED) ? at(S, pp.scratch_off) : src + pg.rep_len + pg.def_len;
        pg.aux = words(at(S, pp.aux_off));
        pg.runtab = reinterpret_cast<IdRunTab*>(at(S, pp.rt_off));
        pg.lvltab = reinterpret_cast<LvlHead*>(at(S, pp.lt_off));
        pg.dx = reinterpret_cast<uint64_t*>(at(S, pp.dx_off));
        pg.dbp = at(S, pp.dbp_off);
        pg.seg = at(S, pp.seg_off);
        if (pp.dbp_off != NO_OFF) pg.dbp_pub = reinterpret_cast<WinPub*>(at(S + p.off_npub, pp.dbp_pub_off));
        if (pp.seg_off != NO_OFF) pg.npub = reinterpret_cast<WinPub*>(at(S + p.off_npub, pp.pub_off));
        if (pg.flags & PG_DICT) {
            DevChunk& ck = p.chunks[size_t(pg.chunk)];
            ck.dict_data = pg.body;
            if (ck.ptype == PF_BYTE_ARRAY) {
                ck.dict_pos = pg.aux;
                ck.dict_len = ck.dict_pos + (pg.num_values + 1);
            }
        }
    }
    for (size_t j = 0; j < p.jobs.size(); j++) {
        SnappyJob& jb = p.jobs[j];
        DevPage& pg = p.pages[size_t(jb.page)];
        jb.src = at(a.in, p.pplan[size_t(jb.page)].in_off) + pg.rep_len + pg.def_len;
        jb.dst = at(S, p.pplan[size_t(jb.page)].scratch_off);
        // each Snappy data page reads its job's fallback flag (k_flat_fixed: were the values written direct?)
        pg.jfb = reinterpret_cast<const int*>(a.meta + p.off_fallback) + j;
    }
    bind_snappy(p.jobs, p.snap, a.tokmap);
    for (ZstdJob& jb : p.zjobs) {
        const DevPage& pg = p.pages[size_t(jb.page)];
        jb.src = at(a.in, p.pplan[size_t(jb.page)].in_off) + pg.rep_len + pg.def_len;
        jb.dst = at(S, p.pplan[size_t(jb.page)].scratch_off);
    }
    for (Lz4Job& jb : p.ljobs) {
        const DevPage& pg = p.pages[size_t(jb.page)];
        jb.src = at(a.in, p.pplan[size_t(jb.page)].in_off) + pg.rep_len + pg.def_len;
        jb.dst = at(S, p.pplan[size_t(jb.page)].scratch_off);
    }
    for (size_t b = 0; b < p.bajobs.size(); b++) {
        BaJob& J = p.bajobs[b];
        const size_t nw = size_t(J.n_tiles) * (BA_TILE / 32);
        J.cand = words(at(S, p.ba_bm[b]));
        J.link1 = J.cand + nw;
        J.link2 = J.link1 + nw;
        J.tile_cnt = J.link2 + nw;
        const DevPage& pg = p.pages[size_t(J.page)];
        if (int(b) < p.n_ba_dict) {
            const DevChunk& ck = p.chunks[size_t(J.chunk)];
            J.p = pg.body;
            J.pos = ck.dict_pos;
            J.len = ck.dict_len;
        } else {   // p: k_count; the walk reports its chars into the page record
            J.pos = pg.aux;
            J.chars_out = reinterpret_cast<int64_t*>(a.meta + p.off_pages + sizeof(DevPage) * size_t(J.page) + offsetof(DevPage, n_chars));
        }
    }
    for (int c = 0; c < p.n_chunks; c++) {
        DevChunk& ck = p.chunks[size_t(c)];
        const OutPlan& op = p.oplan[size_t(c)];
        ck.values = at(a.out, op.values);
        ck.validity = at(a.bits, op.validity);
        ck.offsets = reinterpret_cast<int32_t*>(at(a.out, op.offsets));
        ck.list_offsets = reinterpret_cast<int32_t*>(at(a.out, op.list_offsets));
        ck.list_validity = at(a.bits, op.list_validity);
        ck.def_levels = at(a.out, op.def);
        ck.rep_levels = at(a.out, op.rep);
    }
    p.dkeeps.clear();
    for (const KeepPlan& kp : p.keeps) {
        DevKeep k{};
        k.chunk = kp.chunk;
        k.index_width = kp.index_width;
        k.n_entries = kp.n_entries;
        k.d_values = at(a.out, kp.values);
        k.d_offsets = reinterpret_cast<int32_t*>(at(a.out, kp.offsets));
        p.dkeeps.push_back(k);
    }
}

// ---- row filters ---------------------------------------------------------------------------------------------------

int plan_filter(const pf_chunk_desc* cds, int n_chunks, const pf_predicate* preds, int n_preds, FilterPlan& f, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    auto reset = [&]() {
        f.preds.clear();
        f.blob.clear();
        f.dicts.clear();
        f.dict_of.clear();
        f.dict_words = 0;
        f.dict_max_entries = 0;
    };
    reset();
    auto bad = [&](int code, const char* text) {
        reset();
        *why = text;
        return code;
    };
    if (n_preds < 0 || n_preds > PF_MAX_PREDICATES) return bad(PF_ERR_INVALID_ARG, "predicates: n_preds outside [0, PF_MAX_PREDICATES]");
    if (n_preds > 0 && (!preds || !cds)) return bad(PF_ERR_INVALID_ARG, "predicates: null table");
    for (int i = 0; i < n_preds; i++) {
        const pf_predicate& q = preds[i];
        if (q.chunk < 0 || q.chunk >= n_chunks) return bad(PF_ERR_INVALID_ARG, "predicate: chunk index out of range");
        if (q.op != PF_PRED_RANGE && q.op != PF_PRED_IS_NULL && q.op != PF_PRED_NOT_NULL) return bad(PF_ERR_INVALID_ARG, "predicate: unknown op");
        const pf_chunk_desc& cd = cds[q.chunk];
        if (q.op != PF_PRED_RANGE && (q.lo || q.hi)) return bad(PF_ERR_INVALID_ARG, "predicate: IS_NULL / NOT_NULL take no bound");
        if (cd.max_rep > 0) return bad(PF_ERR_UNSUPPORTED_TYPE, "predicate: a column with repetition");
        DevPred d{};
        d.chunk = q.chunk;
        d.op = q.op;
        d.ptype = cd.physical_type;
        if (q.op == PF_PRED_RANGE) {
            const int pt = cd.physical_type;
            if (pt != PF_BOOLEAN && pt != PF_INT32 && pt != PF_INT64 && pt != PF_FLOAT && pt != PF_DOUBLE && pt != PF_BYTE_ARRAY)
                return bad(PF_ERR_UNSUPPORTED_TYPE, "predicate: a range over INT96, FIXED_LEN_BYTE_ARRAY or an unknown type");
            for (int side = 0; side < 2; side++) {
                const uint8_t* b = side ? q.hi : q.lo;
                const int32_t n = side ? q.hi_len : q.lo_len;
                if (!b) continue;
                d.flags |= side ? PRED_HAS_HI : PRED_HAS_LO;
                if (pt == PF_BYTE_ARRAY) {
                    if (n < 0 || n > PRED_BOUND_MAX) return bad(PF_ERR_INVALID_ARG, "predicate: a BYTE_ARRAY bound of more than 4096 bytes");
                    (side ? d.hi_off : d.lo_off) = uint32_t(f.blob.size());
                    (side ? d.hi_len : d.lo_len) = uint32_t(n);
                    f.blob.insert(f.blob.end(), b, b + n);
                    continue;
                }
                if (n != type_width(pt, 0)) return bad(PF_ERR_INVALID_ARG, "predicate: a bound whose length is not the type's width");
                uint64_t raw = 0;
                for (int k = 0; k < n; k++) raw |= uint64_t(b[k]) << (8 * k);   // little-endian
                int64_t iv = 0;
                double fv = 0;
                if (pt == PF_BOOLEAN) {
                    if (raw > 1) return bad(PF_ERR_INVALID_ARG, "predicate: a BOOLEAN bound is the byte 0 or 1");
                    iv = int64_t(raw);
                } else if (pt == PF_INT32) {
                    iv = int64_t(int32_t(uint32_t(raw)));
                } else if (pt == PF_INT64) {
                    iv = int64_t(raw);
                } else if (pt == PF_FLOAT) {
                    const uint32_t w = uint32_t(raw);
                    float x;
                    static_assert(sizeof x == sizeof w, "float is 32 bits");
                    __builtin_memcpy(&x, &w, 4);
                    fv = double(x);
                } else {
                    __builtin_memcpy(&fv, &raw, 8);
                }
                (side ? d.hi_i : d.lo_i) = iv;
                (side ? d.hi_f : d.lo_f) = fv;
            }
        }
        f.preds.push_back(d);
    }
    *why = "";
    return PF_OK;
}

void plan_filter_dict(const BatchPlan& p, FilterPlan& f) {
    f.dicts.clear();
    f.dict_of.clear();
    f.dict_words = 0;
    f.dict_max_entries = 0;
    if (p.keeps.empty()) return;
    for (size_t i = 0; i < f.preds.size(); i++) {
        const DevPred& d = f.preds[i];
        const int32_t k = d.op == PF_PRED_RANGE && size_t(d.chunk) < p.keep_of.size() ? p.keep_of[size_t(d.chunk)] : -1;
        if (k < 0) continue;
        if (f.dict_of.empty()) f.dict_of.assign(f.preds.size(), -1);
        DevSelDict r{};
        r.pred = int32_t(i);
        r.keep = k;
        r.n_entries = std::max<int64_t>(p.keeps[size_t(k)].n_entries, 0);
        r.word_off = f.dict_words;
        r.n_words = (uint64_t(r.n_entries) + 63) / 64;
        f.dict_words += r.n_words;
        f.dict_max_entries = std::max(f.dict_max_entries, r.n_entries);
        f.dict_of[i] = int32_t(f.dicts.size());
        f.dicts.push_back(r);
    }
}

}  // namespace pf
