// pf_enc_plan.cpp — host-only planning of one chunk's encode (pf_enc_plan.h). No HIP call.
#include "pf_enc_plan.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "pf_crc.h"
#include "pf_host.h"
#include "pf_xxh64.h"
#include "pf_zstd_enc_core.h"

namespace pf {

namespace {

int reject(const char** why, int code, const char* msg) {
    if (why) *why = msg;
    return code;
}

// (the arena's and the sections' cursor: 256-byte aligned regions of at least one byte)
size_t take(size_t& cur, size_t sz) {
    size_t o = align_up(cur, 256);
    cur = o + std::max<size_t>(sz, 1);
    return o;
}

int enc_width(int pt) { return pt == PF_BYTE_ARRAY ? 0 : pt == PF_BOOLEAN ? 1 : (pt == PF_INT32 || pt == PF_FLOAT) ? 4 : 8; }

}  // namespace

size_t uvarint_len(uint64_t v) { size_t k = 1; while (v >= 0x80) { v >>= 7; k++; } return k; }
void put_uvarint(std::vector<uint8_t>& o, uint64_t v) {
    while (v >= 0x80) { o.push_back(uint8_t(v | 0x80)); v >>= 7; }
    o.push_back(uint8_t(v));
}

size_t stream_head(int codec, uint64_t n, uint8_t* o /* 12 bytes */) {
    if (codec == PF_CODEC_ZSTD) {
        size_t k = zstd::frame_header_put(n, o);
        if (n == 0) { std::memcpy(o + k, zstd::ZE_EMPTY_BLOCK, 3); k += 3; }
        return k;
    }
    size_t k = 0;
    while (n >= 0x80) { o[k++] = uint8_t(n | 0x80); n >>= 7; }
    o[k++] = uint8_t(n);
    return k;
}

uint64_t hybrid_worst(uint64_t cnt, uint32_t bw) { return (cnt / 8 + 1) * std::max<uint64_t>(bw + 1, 5 + (bw + 7) / 8); }

// ---------------------------------------------------------------- plan_encode
int check_encode_args(const pf_encode_column* col, const char** why) {
    const int pt = col->physical_type;
    if (pt != PF_BOOLEAN && pt != PF_INT32 && pt != PF_INT64 && pt != PF_FLOAT && pt != PF_DOUBLE && pt != PF_BYTE_ARRAY)
        return reject(why, PF_ERR_UNSUPPORTED_TYPE, "encode: unsupported physical type");
    const int64_t n = col->num_rows;
    if (n < 0 || n > 0x7ffffff0 || (col->max_def != 0 && col->max_def != 1)) return reject(why, PF_ERR_INVALID_ARG, "encode: bad shape");
    if (col->codec != PF_CODEC_SNAPPY && col->codec != PF_CODEC_ZSTD && col->codec != PF_CODEC_UNCOMPRESSED)
        return reject(why, PF_ERR_UNSUPPORTED_CODEC, "encode: codec must be SNAPPY, ZSTD or UNCOMPRESSED");
    if (col->bloom_bytes != 0 && (col->bloom_bytes < 0 || !bloom_size_ok(uint64_t(col->bloom_bytes))))
        return reject(why, PF_ERR_INVALID_ARG, "encode: bloom_bytes must be a power of two in [32, 128 MiB]");
    const bool str = pt == PF_BYTE_ARRAY;
    if ((col->dictionary & PF_ENCODE_PAGE_INDEX) && str && col->index_truncate != 0 && col->index_truncate != -1 &&
        (col->index_truncate < 1 || col->index_truncate > 2047))
        return reject(why, PF_ERR_INVALID_ARG, "encode: index_truncate must be 0, -1 or in [1, 2047]");
    if (n > 0 && (str ? (!col->offsets || (!col->chars && col->chars_len > 0) || col->chars_len < 0 || col->chars_len > 0x7fffffff)
                      : !col->values))
        return reject(why, PF_ERR_INVALID_ARG, "encode: missing input arrays");
    return PF_OK;
}

namespace {

void plan_settings(const pf_encode_column* col, EncPlan& p) {
    p.pt = col->physical_type;
    p.str = p.pt == PF_BYTE_ARRAY;
    p.w = enc_width(p.pt);
    p.n = col->num_rows;
    p.max_def = col->max_def;
    p.codec = col->codec;
    p.bits = col->dictionary;
    p.chars_len = p.str ? col->chars_len : 0;
    p.compressed = col->codec != PF_CODEC_UNCOMPRESSED;
    p.bloom = p.pt == PF_BOOLEAN ? 0 : size_t(col->bloom_bytes);   // BOOLEAN: no filter (parquet-mr builds none)
    p.px_trunc = col->index_truncate == -1 ? PX_NO_TRUNC : col->index_truncate == 0 ? 64u : uint32_t(col->index_truncate);
    p.page_rows = col->page_rows > 0 ? col->page_rows : 20000;
    p.page_rows = (p.page_rows + 7) / 8 * 8;   // definition levels of a page start on a validity byte
    // dictionary page limit (parquet.dictionary.page.size, 1 MiB); capped so a dictionary that passes it
    // always fits the 32-bit offsets of the dictionary kernels
    p.dict_limit = std::min<int64_t>(col->dict_page_limit > 0 ? col->dict_page_limit : (1 << 20), 0x7fffffff);
    p.vbytes = size_t((p.n + 7) / 8);
    p.has_val = col->max_def == 1 && col->validity;
    p.dict_bit = (p.bits & PF_ENCODE_DICTIONARY) != 0;
    // DELTA_* fallback (PF_ENCODE_DELTA_FALLBACK): INT32, INT64 and BYTE_ARRAY; the other types stay PLAIN
    p.delta_bit = (p.bits & PF_ENCODE_DELTA_FALLBACK) && (p.pt == PF_INT32 || p.pt == PF_INT64 || p.str);
    p.hyb = (p.bits & PF_ENCODE_HYBRID_RUNS) != 0;
    p.want_stats = (p.bits & PF_ENCODE_STATISTICS) != 0;
    p.want_crc = (p.bits & PF_ENCODE_PAGE_CRC) != 0;
    p.want_index = (p.bits & PF_ENCODE_PAGE_INDEX) != 0;
    p.run_stats = p.want_stats || p.want_index;   // the page index is built from the statistics kernels' page results
}

// page plan: rows, present values, PLAIN byte sizes (the one pass over the rows)
void plan_pages(EncPlan& p, const std::vector<uint8_t>& hval, const std::vector<int32_t>& hoff) {
    const int64_t n = p.n;
    const bool has_val = p.has_val, str = p.str;
    const uint8_t* v = hval.data();
    const int32_t* off = hoff.data();
    uint32_t m = 0;
    for (int64_t r0 = 0; r0 < n || (n == 0 && p.pp.empty()); r0 += p.page_rows) {
        EncPagePlan g{r0, std::min(n, r0 + p.page_rows), m, 0, 0};
        const int64_t rows = g.r1 - g.r0;
        if (!has_val) {          // every row present: nothing to count (whatever the optimiser makes of a loop)
            g.cnt = uint32_t(rows);
            if (str && rows) g.plain = 4 * uint64_t(rows) + uint64_t(off[g.r1] - off[g.r0]);
        } else if (!str) {       // a page starts on a validity byte: whole bytes, then the last partial one
            const uint8_t* b = v + g.r0 / 8;
            for (int64_t k = 0; k < rows / 8; k++) g.cnt += uint32_t(__builtin_popcount(b[k]));
            if (rows & 7) g.cnt += uint32_t(__builtin_popcount(b[rows / 8] & ((1u << (rows & 7)) - 1u)));
        } else {                 // strings with nulls: the lengths of the present rows
            for (int64_t r = g.r0; r < g.r1; r++) {
                const uint32_t on = (v[r >> 3] >> (r & 7)) & 1u;
                g.cnt += on;
                g.plain += on * (4 + uint64_t(off[r + 1] - off[r]));
            }
        }
        if (!str) g.plain = p.pt == PF_BOOLEAN ? (g.cnt + 7) / 8 : uint64_t(g.cnt) * p.w;
        m += g.cnt;
        p.pp.push_back(g);
        if (n == 0) break;
    }
    p.m = m;
}

// DELTA_* tables: one stream per integer page, two (prefix lengths, suffix lengths) per string page; an item of
// the size table is a stream header or a 128-delta block
int plan_delta(EncPlan& p, const char** why) {
    const bool str = p.str;
    for (size_t i = 0; i < p.pp.size(); i++) {
        const EncPagePlan& g = p.pp[i];
        const uint32_t ns = str ? 2u : 1u, blocks = g.cnt > 1 ? (g.cnt - 1 + 127) / 128 : 0u;
        // worst case of the values section (every block: zigzag(min) + widths + full-width values)
        const uint64_t worst = ns * (25ull + blocks * 14ull + uint64_t(g.cnt) * (str ? 4 : p.w)) + (str ? g.plain : 0);
        if (worst > 0x7fffffffull) return reject(why, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
        p.dpages.push_back(DeltaPage{0, g.d0, g.cnt, uint32_t(p.dstreams.size()), ns});
        for (uint32_t k = 0; k < ns; k++) {
            p.dstreams.push_back(DeltaStream{nullptr, uint32_t(str ? 4 : p.w), g.cnt, uint32_t(i), p.n_items});
            p.n_items += 1 + blocks;
        }
    }
    p.dstreams.push_back(DeltaStream{nullptr, 0, 0, 0, p.n_items});
    return PF_OK;
}

// statistics (a workgroup per (page, tile of ST_TILE present values)) and the page index block:
// head | null_counts | offsets | null_pages | values (the worst case: every entry as long as it can get)
int plan_stats_index(EncPlan& p, const char** why) {
    if (p.run_stats) {
        for (size_t i = 0; i < p.pp.size(); i++) {
            p.sptile.push_back(uint32_t(p.stiles.size()));
            for (uint32_t o = 0; o < p.pp[i].cnt; o += ST_TILE)
                p.stiles.push_back(StatTile{uint32_t(i), p.pp[i].d0 + o, std::min(ST_TILE, p.pp[i].cnt - o), 0u});
        }
        p.sptile.push_back(uint32_t(p.stiles.size()));
    }
    p.n_se = p.run_stats ? p.pp.size() + 1 : 0;
    p.n_px = p.want_index ? p.pp.size() : 0;
    const uint64_t px_entry = !p.str ? uint64_t(p.w) : p.px_trunc == PX_NO_TRUNC ? uint64_t(ST_LIMIT) / 2 : uint64_t(p.px_trunc);
    p.px_cap = 2 * px_entry * p.n_px;
    if (p.px_cap > 0x40000000ull)
        return reject(why, PF_ERR_INVALID_ARG, "encode: page index values over 1 GiB (fewer pages or a shorter index_truncate)");
    p.px_nc = sizeof(PgIndexHead);
    p.px_off = p.px_nc + 8 * p.n_px;
    p.px_np = p.px_off + 4 * (2 * p.n_px + 1);
    p.px_val = p.px_np + p.n_px;
    p.px_bytes = p.want_index ? p.px_val + size_t(p.px_cap) : 0;
    p.px_in.resize(2 * p.n_px);
    for (size_t i = 0; i < p.n_px; i++) { p.px_in[i] = uint32_t(p.pp[i].r1 - p.pp[i].r0); p.px_in[p.n_px + i] = p.pp[i].cnt; }
    return PF_OK;
}

}  // namespace

int plan_encode(const pf_encode_column* col, const std::vector<uint8_t>& hval, const std::vector<int32_t>& hoff, EncPlan& p,
                const char** why) {
    p = EncPlan{};
    int rc = check_encode_args(col, why);
    if (rc) return rc;
    plan_settings(col, p);
    if (p.str && p.n > 0)
        for (int64_t r = 0; r < p.n; r++)
            if (hoff[size_t(r) + 1] < hoff[size_t(r)] || hoff[size_t(r)] < 0 || hoff[size_t(r) + 1] > col->chars_len) {
                p = EncPlan{};
                return reject(why, PF_ERR_INVALID_ARG, "encode: offsets out of order or outside chars");
            }
    plan_pages(p, hval, hoff);
    if (p.delta_bit) rc = plan_delta(p, why);
    // parquet-mr's hybrid runs: a page has a stream of levels (OPTIONAL) and one of ids or BOOLEAN values
    p.n_hs_max = p.hyb ? 2 * p.pp.size() : 0;
    if (!rc) rc = plan_stats_index(p, why);
    if (rc) { p = EncPlan{}; return rc; }
    // The device sums dictionary bytes in 32 bits: a BYTE_ARRAY column whose dictionary could reach 4 GiB
    // (all values distinct: 4 m + chars) is written PLAIN (conservative: such a dictionary is over any
    // page limit unless most values repeat; parity with parquet-mr's writer is unpinned).
    p.dict_fits32 = !p.str || 4ull * uint64_t(p.m) + uint64_t(col->chars_len) < (1ull << 32);
    p.want_dict = p.dict_bit && p.pt != PF_BOOLEAN && p.m > 0 && p.dict_fits32;
    // the scans over rows, dense values and delta items
    p.scan_elems = std::max(size_t(p.n) + 1, p.delta_bit ? size_t(p.n_items) + 1 : size_t(0));
    return PF_OK;
}

// ---------------------------------------------------------------- layout_encode / bind_encode
void layout_encode(EncPlan& p, size_t temp_bytes) {
    const bool str = p.str, ds = p.delta_bit && str;
    const size_t n = size_t(p.n), w = size_t(p.w), N1 = n + 1, S1 = str ? 4 * N1 : 0, D1 = ds ? 4 * N1 : 0;
    const size_t NI1 = p.delta_bit ? size_t(p.n_items) + 1 : 0, nt = p.stiles.size();
    p.temp_bytes = temp_bytes;
    // DELTA_* tables (only with the bit set): string prefix / suffix lengths and positions, streams, pages,
    // item bytes and offsets, block minima and widths, page totals
    const size_t size[N_ENC_REGIONS] = {
        /* R_IN */ str ? 0 : n * w, /* R_VL */ p.vbytes, /* R_OF */ S1, /* R_CH */ str ? size_t(p.chars_len) : 0,
        /* R_FLAG */ 4 * N1, /* R_POS */ 4 * N1, /* R_DENSE */ n * w, /* R_DSRC */ S1, /* R_DLEN */ S1, /* R_VSZ */ S1, /* R_VPRE */ S1,
        /* R_KEY */ 8 * N1, /* R_SKEY */ 8 * N1, /* R_DIDX */ 4 * N1, /* R_SIDX */ 4 * N1,
        /* R_HP */ 4 * N1, /* R_HEAD */ 4 * N1, /* R_MARK */ 4 * N1, /* R_DID */ 4 * N1,
        /* R_DSZ */ 4 * N1, /* R_DOFF */ 4 * N1, /* R_IDS */ 4 * N1, /* R_COL */ 256,
        /* R_PFX */ D1, /* R_SFX */ D1, /* R_SPRE */ D1,
        /* R_DSTR */ sizeof(DeltaStream) * p.dstreams.size(), /* R_DPG */ sizeof(DeltaPage) * p.dpages.size(),
        /* R_DBY */ 4 * NI1, /* R_DOF */ 4 * NI1, /* R_DMIN */ 8 * NI1, /* R_DWD */ 4 * NI1, /* R_DTOT */ 4 * p.dpages.size(),
        /* R_HSTR */ sizeof(HybridStream) * p.n_hs_max, /* R_HBY */ 4 * p.n_hs_max,
        /* R_STT */ sizeof(StatTile) * nt, /* R_STP */ 4 * p.sptile.size(), /* R_SPART */ sizeof(StatPart) * nt,
        /* R_SWIN */ str ? 8 * nt : 0, /* R_SOUT */ sizeof(StatPart) * p.n_se, /* R_SBYTES */ str ? size_t(ST_LIMIT) * p.n_se : 0,
        /* R_XIN */ 8 * p.n_px, /* R_XNN */ 4 * p.n_px, /* R_XOUT */ p.px_bytes,
        /* R_TEMP */ temp_bytes, /* R_BLOOM */ p.bloom};
    p.a_sz = 0;
    for (int r = 0; r < N_ENC_REGIONS; r++) {
        if (r == R_BLOOM && !p.bloom) { p.reg[r] = Region{}; continue; }
        p.reg[r].size = std::max<size_t>(size[r], 1);
        p.reg[r].off = take(p.a_sz, size[r]);
    }
}

void bind_encode(EncPlan& p, uint8_t* A, const pf_encode_column* col, bool on_device) {
    auto at = [&](EncRegion r) { return A + p.reg[r].off; };
    auto u32 = [&](EncRegion r) { return reinterpret_cast<uint32_t*>(A + p.reg[r].off); };
    EncArgs& ea = p.ea;
    ea.ptype = p.pt; ea.width = p.w; ea.n = p.n;
    if (on_device) {
        ea.values = static_cast<const uint8_t*>(col->values);
        ea.validity = p.has_val ? col->validity : nullptr;
        ea.offsets = col->offsets;
        ea.chars = col->chars;
    } else {
        ea.values = at(R_IN);
        ea.validity = p.has_val ? at(R_VL) : nullptr;
        ea.offsets = reinterpret_cast<const int32_t*>(at(R_OF));
        ea.chars = at(R_CH);
    }
    ea.flag = u32(R_FLAG); ea.pos = u32(R_POS);
    ea.dense = at(R_DENSE);
    ea.dsrc = u32(R_DSRC); ea.dlen = u32(R_DLEN);
    ea.vsz = u32(R_VSZ); ea.vpre = u32(R_VPRE);
    ea.key = reinterpret_cast<uint64_t*>(at(R_KEY)); ea.skey = reinterpret_cast<uint64_t*>(at(R_SKEY));
    ea.didx = u32(R_DIDX); ea.sidx = u32(R_SIDX);
    ea.headpos = u32(R_HP); ea.head = u32(R_HEAD);
    ea.mark = u32(R_MARK); ea.did = u32(R_DID);
    ea.dsz = u32(R_DSZ); ea.doff = u32(R_DOFF);
    ea.ids = u32(R_IDS); ea.collide = u32(R_COL);
    p.temp = at(R_TEMP);
    p.d_bloom = p.bloom ? at(R_BLOOM) : nullptr;
    p.ha.streams = reinterpret_cast<const HybridStream*>(at(R_HSTR));
    p.ha.bytes = u32(R_HBY);
    if (p.delta_bit) {
        DeltaArgs& da = p.da;
        da.streams = reinterpret_cast<const DeltaStream*>(at(R_DSTR));
        da.pages = reinterpret_cast<const DeltaPage*>(at(R_DPG));
        da.n_streams = uint32_t(p.dstreams.size() - 1); da.n_pages = uint32_t(p.dpages.size()); da.n_items = p.n_items;
        da.bytes = u32(R_DBY); da.off = u32(R_DOF);
        da.minv = reinterpret_cast<long long*>(at(R_DMIN)); da.widths = u32(R_DWD);
        da.totals = u32(R_DTOT);
        if (p.str) { da.pfx = u32(R_PFX); da.sfx = u32(R_SFX); da.spre = u32(R_SPRE); }
        for (size_t s = 0; s + 1 < p.dstreams.size(); s++) {
            const DeltaPage& g = p.dpages[p.dstreams[s].page];
            p.dstreams[s].src = !p.str ? ea.dense + uint64_t(g.d0) * uint32_t(p.w)
                                       : reinterpret_cast<const uint8_t*>((s - g.s0 == 0 ? da.pfx : da.sfx) + g.d0);
        }
    }
    if (p.run_stats) {
        StatArgs& sa = p.sa;
        sa.tiles = reinterpret_cast<const StatTile*>(at(R_STT)); sa.ptile = u32(R_STP);
        sa.n_tiles = uint32_t(p.stiles.size()); sa.n_pages = uint32_t(p.pp.size());
        sa.part = reinterpret_cast<StatPart*>(at(R_SPART)); sa.win = u32(R_SWIN);
        sa.out = reinterpret_cast<StatPart*>(at(R_SOUT)); sa.bytes = at(R_SBYTES);
    }
    if (p.want_index) {
        PgIndexArgs& xa = p.xa;
        uint8_t* x = at(R_XOUT);
        xa.pages = p.sa.out;
        xa.rows = u32(R_XIN); xa.cnt = xa.rows + p.n_px;
        xa.n_pages = uint32_t(p.n_px); xa.trunc = p.px_trunc; xa.value_cap = uint32_t(p.px_cap);
        xa.nn = u32(R_XNN);
        xa.head = reinterpret_cast<PgIndexHead*>(x);
        xa.null_counts = reinterpret_cast<long long*>(x + p.px_nc);
        xa.off = reinterpret_cast<uint32_t*>(x + p.px_off);
        xa.null_pages = x + p.px_np;
        xa.values = x + p.px_val;
    }
}

// ---------------------------------------------------------------- plan_values
void plan_values(EncPlan& p, uint32_t collide, uint32_t D, uint32_t dict_bytes_dev) {
    const bool str = p.str, not_bool = p.pt != PF_BOOLEAN;
    p.fallback = 0;
    if (p.dict_bit && !not_bool) p.fallback = 3;
    else if (p.want_dict && collide) p.fallback = 2;
    else if (p.dict_bit && not_bool && p.m > 0 && !p.dict_fits32) p.fallback = 1;
    else if (p.want_dict && (str ? int64_t(dict_bytes_dev) : int64_t(D) * p.w) > p.dict_limit) p.fallback = 1;   // fixed: D * w on the host
    p.dict = p.want_dict && p.fallback == 0;
    p.D = p.dict ? D : 0;
    p.dict_bytes = p.dict ? (str ? dict_bytes_dev : D * uint32_t(p.w)) : 0;
    p.bw = 1;
    while (p.D > 1 && (uint64_t(1) << p.bw) < p.D) p.bw++;
    if (p.hyb && p.D == 1) p.bw = 0;   // parquet-mr's getWidthFromMaxInt(D - 1)
    p.brle = p.hyb && !not_bool;       // parquet-mr v2 writes BOOLEAN with the RLE encoding
    p.delta = p.delta_bit && !p.dict;  // the chunk is not dictionary-encoded: DELTA_* pages
    p.data_enc = p.dict ? PF_ENC_RLE_DICTIONARY : p.delta ? (str ? PF_ENC_DELTA_BYTE_ARRAY : PF_ENC_DELTA_BINARY_PACKED)
                        : p.brle ? PF_ENC_RLE : PF_ENC_PLAIN;
    const size_t np = p.pp.size();
    p.hs.clear();
    p.lv_of.assign(np, -1);
    p.vs_of.assign(np, -1);
    p.ub = 0;
    if (!p.hyb) { p.hbytes.clear(); return; }
    for (size_t i = 0; i < np && p.max_def == 1; i++) {
        p.lv_of[i] = int(p.hs.size());
        p.hs.push_back(HybridStream{p.ea.validity, 0, HY_VALIDITY, uint32_t(p.pp[i].r0), uint32_t(p.pp[i].r1 - p.pp[i].r0), 1,
                                    HY_PREFIX_NONE, uint32_t(i)});
    }
    for (size_t i = 0; i < np && (p.dict || p.brle); i++) {
        p.vs_of[i] = int(p.hs.size());
        p.hs.push_back(p.dict ? HybridStream{reinterpret_cast<const uint8_t*>(p.ea.ids), 0, HY_IDS, p.pp[i].d0, p.pp[i].cnt, p.bw,
                                             HY_PREFIX_WIDTH, uint32_t(i)}
                              : HybridStream{p.ea.dense, 0, HY_BOOL, p.pp[i].d0, p.pp[i].cnt, 1, HY_PREFIX_LENGTH, uint32_t(i)});
    }
    p.ha.n_streams = uint32_t(p.hs.size());
    p.hbytes.assign(p.hs.size(), 0);
    if (p.delta) return;
    // The dictionary page and the ids are written before the size pass: room for the worst case of every section
    size_t vo = 0;
    p.o_dict = take(vo, p.dict_bytes);   // (plan_sections places it there again)
    p.ub = vo + 512 + sizeof(EncPage) * np;
    for (const EncPagePlan& g : p.pp)
        p.ub += 256 + size_t(p.dict ? 1 + hybrid_worst(g.cnt, p.bw) : p.brle ? 4 + hybrid_worst(g.cnt, 1) : g.plain) +
                size_t(p.max_def == 1 ? hybrid_worst(uint64_t(g.r1 - g.r0), 1) : 0);
}

// ---------------------------------------------------------------- plan_sections
int plan_sections(EncPlan& p, const char** why) {
    const size_t np = p.pp.size();
    p.sections.clear();
    p.ep.assign(p.delta ? 0 : np, EncPage{});
    p.lv_off.assign(np, 0);
    p.o_lv = p.lv_total = p.o_pages = 0;
    p.vo = 0;
    p.o_dict = take(p.vo, p.dict_bytes);
    if (p.dict) p.sections.push_back({p.o_dict, p.dict_bytes});
    for (size_t i = 0; i < np; i++) {
        const EncPagePlan& g = p.pp[i];
        if (p.delta) {
            if (p.htot[i] > 0x7fffffffu) return reject(why, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
            p.dpages[i].out_off = take(p.vo, p.htot[i]);
            p.sections.push_back({p.dpages[i].out_off, p.htot[i]});
            continue;
        }
        uint64_t bytes, pre = 0;
        if (p.vs_of[i] >= 0) {   // width byte or 4-byte length, then the stream
            pre = p.dict ? 1 : 4;
            bytes = pre + p.hbytes[size_t(p.vs_of[i])];
        } else if (p.dict) {     // one bit-packed run
            const uint64_t groups = (g.cnt + 7) / 8;
            bytes = g.cnt ? 1 + uvarint_len((groups << 1) | 1) + groups * p.bw : 1;
        } else {
            bytes = g.plain;
        }
        p.ep[i] = EncPage{0, g.d0, g.cnt, p.dict ? 1u : 0u, p.bw};
        p.ep[i].out_off = take(p.vo, bytes);
        if (p.vs_of[i] >= 0) p.hs[size_t(p.vs_of[i])].out_off = p.ep[i].out_off + pre;
        p.sections.push_back({p.ep[i].out_off, bytes});
    }
    if (p.hyb) {   // the pages' levels, back to back behind the values sections
        for (size_t i = 0; i < np; i++)
            if (p.lv_of[i] >= 0) { p.lv_off[i] = p.lv_total; p.lv_total += p.hbytes[size_t(p.lv_of[i])]; }
        p.o_lv = take(p.vo, p.lv_total);
        for (size_t i = 0; i < np; i++)
            if (p.lv_of[i] >= 0) p.hs[size_t(p.lv_of[i])].out_off = p.o_lv + p.lv_off[i];
    }
    if (!p.delta) p.o_pages = take(p.vo, sizeof(EncPage) * p.ep.size());
    return PF_OK;
}

// ---------------------------------------------------------------- CRC pieces, compression jobs
// Page CRCs (PF_ENCODE_PAGE_CRC): the pieces of the pages that lie in device memory -- the compression jobs'
// slots (SNAPPY, ZSTD; plan_compress lists them) or the sections themselves, and the levels: the stream the GPU
// encoded (hybrid runs), or the whole validity bytes of the page's rows, which the one bit-packed run repeats
// -- go through k_enc_crc; the results hold the jobs (SNAPPY, ZSTD) or sections first, then the levels.
void plan_crc_levels(EncPlan& p, const uint8_t* sec) {
    p.lv_pieces.clear();
    p.lv_piece.assign(p.pp.size(), -1);
    p.vb_piece.assign(p.pp.size(), -1);
    if (!p.want_crc) return;
    for (size_t i = 0; i < p.pp.size(); i++) {
        if (p.lv_of[i] >= 0) {
            const uint32_t nb = p.hbytes[size_t(p.lv_of[i])];
            p.lv_piece[i] = int(p.lv_pieces.size());
            p.lv_pieces.push_back(CrcPiece{sec + p.o_lv + p.lv_off[i], nullptr, nb, nb});
        } else if (p.has_val && p.pp[i].r1 - p.pp[i].r0 >= 8) {   // (pages start on a validity byte)
            const uint32_t nb = uint32_t((p.pp[i].r1 - p.pp[i].r0) / 8);
            p.vb_piece[i] = int(p.lv_pieces.size());
            p.lv_pieces.push_back(CrcPiece{p.ea.validity + p.pp[i].r0 / 8, nullptr, nb, nb});
        }
    }
}

int plan_section_pieces(EncPlan& p, const uint8_t* sec, const char** why) {
    p.sec_pieces.clear();
    for (const auto& sct : p.sections) {
        if (sct.second > 0xffffffffull) return reject(why, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
        p.sec_pieces.push_back(CrcPiece{sec + sct.first, nullptr, uint32_t(sct.second), uint32_t(sct.second)});
    }
    p.sec_pieces.insert(p.sec_pieces.end(), p.lv_pieces.begin(), p.lv_pieces.end());
    p.o_crc_res = align_up(sizeof(CrcPiece) * p.sec_pieces.size(), 256);
    return PF_OK;
}

void plan_compress(const std::vector<std::pair<uint64_t, uint64_t>>& sections, int codec, bool want_crc, size_t n_extra,
                   CompressPlan& cp) {
    const bool zs = codec == PF_CODEC_ZSTD;
    cp = CompressPlan{};
    cp.codec = codec;
    cp.JOB = zs ? ZC_BLOCK : SC_BLOCK;
    cp.SLOT = zs ? ZC_SLOT : SC_SLOT;
    cp.range.resize(sections.size());
    for (size_t i = 0; i < sections.size(); i++) {
        cp.range[i].first = cp.jobs.size();
        for (uint64_t o = 0; o < sections[i].second; o += cp.JOB) {
            CompJob j{};
            j.len = uint32_t(std::min<uint64_t>(cp.JOB, sections[i].second - o));
            j.last = zs && o + j.len == sections[i].second;
            cp.jobs.push_back(j);
            cp.src_off.push_back(sections[i].first + o);
        }
        cp.range[i].second = cp.jobs.size();
    }
    const size_t nj = cp.jobs.size();
    auto take0 = [](size_t& cur, size_t sz) { size_t o = align_up(cur, 256); cur = o + sz; return o; };
    cp.o_jobs = take0(cp.arena, sizeof(CompJob) * std::max<size_t>(nj, 1));
    // the jobs' lengths and, behind them, the pieces' CRCs: one D2H
    cp.np = want_crc ? nj + n_extra : 0;
    cp.o_crc_in_len = align_up(4 * nj, 16);
    cp.len_bytes = cp.np ? cp.o_crc_in_len + sizeof(CrcOut) * cp.np : 4 * std::max<size_t>(nj, 1);
    cp.o_len = take0(cp.arena, cp.len_bytes);
    cp.o_pieces = take0(cp.arena, sizeof(CrcPiece) * std::max<size_t>(cp.np, 1));
    cp.o_slots = take0(cp.arena, size_t(cp.SLOT) * std::max<size_t>(nj, 1));
}

void bind_compress(CompressPlan& cp, const uint8_t* base, uint8_t* d, const std::vector<CrcPiece>* extra) {
    const size_t nj = cp.jobs.size();
    for (size_t k = 0; k < nj; k++) {
        cp.jobs[k].src = base + cp.src_off[k];
        cp.jobs[k].dst = d + cp.o_slots + k * cp.SLOT;
    }
    cp.pieces.resize(cp.np);
    if (!cp.np) return;
    const uint32_t* d_len = reinterpret_cast<const uint32_t*>(d + cp.o_len);
    for (size_t k = 0; k < nj; k++) cp.pieces[k] = CrcPiece{cp.jobs[k].dst, d_len + k, 0u, cp.SLOT};
    for (size_t k = nj; k < cp.np; k++) cp.pieces[k] = (*extra)[k - nj];
}

// ---------------------------------------------------------------- assemble_chunk
namespace {

// CRC of a page: its pieces folded in stored order (pf_crc.h); the bytes the host generates itself (the
// length varint or the frame header, a bit-packed level run built from hval) are fed bytewise.
struct CrcFold {
    const EncPlan& p;
    const AssembleIn& in;
    size_t job = 0;     // SNAPPY, ZSTD: the next job in crcs
    bool bad = false;   // the pieces of some page are not the page

    uint32_t page(size_t sec, size_t pg, const std::vector<uint8_t>& def) {
        uint32_t raw = 0;
        uint64_t len = 0;
        auto piece = [&](const CrcOut& c) { raw = crc_combine_pow(raw, c.raw, c.x8len); len += c.len; };
        const std::vector<uint8_t>& body = (*in.bodies)[sec];
        if (pg != size_t(-1) && p.lv_piece[pg] >= 0) {
            piece(in.crcs[in.crc_first_lv + size_t(p.lv_piece[pg])]);
        } else if (pg != size_t(-1) && p.vb_piece[pg] >= 0) {   // run header ‖ whole validity bytes (device) ‖ last partial byte
            const CrcOut& c = in.crcs[in.crc_first_lv + size_t(p.vb_piece[pg])];
            const size_t groups = size_t(p.pp[pg].r1 - p.pp[pg].r0 + 7) / 8, hdr = def.size() - groups;
            raw = crc_raw_bytes(raw, def.data(), hdr);
            len += hdr;
            piece(c);
            if (c.len != size_t(p.pp[pg].r1 - p.pp[pg].r0) / 8) bad = true;   // (the host would fill what a short piece leaves)
            const size_t done = std::min<size_t>(hdr + c.len, def.size());
            raw = crc_raw_bytes(raw, def.data() + done, def.size() - done);
            len += def.size() - done;
        } else {
            raw = crc_raw_bytes(raw, def.data(), def.size());
            len += def.size();
        }
        if (p.compressed) {
            uint8_t head[12];
            const size_t vl = stream_head(p.codec, p.sections[sec].second, head);
            raw = crc_raw_bytes(raw, body.data(), vl);
            len += vl;
            const uint32_t JOB = p.codec == PF_CODEC_ZSTD ? ZC_BLOCK : SC_BLOCK;
            for (uint64_t o = 0; o < p.sections[sec].second; o += JOB) piece(in.crcs[job++]);
        } else {
            piece(in.crcs[sec]);
        }
        if (len != def.size() + body.size()) bad = true;
        return crc_finish(raw, len);
    }
};

// Statistics of entry e (a page, or pp.size(): the chunk) from the kernels' results
StatsOut stats_of(const EncPlan& p, const AssembleIn& in, size_t e, int64_t nulls) {
    StatsOut so;
    if (!p.want_stats || in.hst[e].any == 2) return so;   // over the size limit: no struct at all
    so.present = true;
    so.null_count = nulls;
    if (in.hst[e].any != 1) return so;
    so.has_min_max = true;
    if (p.str) {
        const char* b = reinterpret_cast<const char*>(in.hsb + e * size_t(ST_LIMIT));
        so.min.assign(b, in.hst[e].mnl);
        so.max.assign(b + in.hst[e].mnl, in.hst[e].mxl);
    } else {   // PLAIN: little-endian, w bytes (BOOLEAN: one byte)
        so.min.assign(reinterpret_cast<const char*>(&in.hst[e].mn), size_t(p.w));
        so.max.assign(reinterpret_cast<const char*>(&in.hst[e].mx), size_t(p.w));
    }
    so.legacy = !p.str || so.min == so.max;   // parquet-mr: the legacy fields only where the signed order is the type's
    return so;
}

// The definition levels of page i as stored: the stream the GPU encoded (hybrid runs), or one bit-packed run
// of the validity bits (RLE/bit-packed hybrid, bit width 1)
void page_levels(const EncPlan& p, const AssembleIn& in, size_t i, std::vector<uint8_t>& def) {
    const EncPagePlan& g = p.pp[i];
    const int64_t rows = g.r1 - g.r0;
    def.clear();
    if (p.lv_of[i] >= 0) {
        def.assign(in.hlv + p.lv_off[i], in.hlv + p.lv_off[i] + p.hbytes[size_t(p.lv_of[i])]);
    } else if (p.max_def == 1 && rows > 0) {
        const uint64_t groups = uint64_t(rows + 7) / 8;
        put_uvarint(def, (groups << 1) | 1);
        for (uint64_t k = 0; k < groups; k++) {
            uint8_t b = p.has_val ? (*in.hval)[size_t(g.r0 / 8 + int64_t(k))] : 0xff;
            const int64_t left = rows - int64_t(k) * 8;
            if (left < 8) b &= uint8_t((1u << left) - 1u);
            def.push_back(b);
        }
    }
}

void chunk_stats(const EncPlan& p, const AssembleIn& in, std::vector<uint8_t>& hb, pf_encoded_chunk* out) {
    out->stats_flags = 0;
    out->stat_min_len = out->stat_max_len = 0;
    out->null_count = 0;
    out->stat_min = out->stat_max = nullptr;
    if (!p.want_stats) return;
    const StatsOut so = stats_of(p, in, p.pp.size(), p.n - int64_t(p.m));
    hb.assign(so.min.begin(), so.min.end());
    hb.insert(hb.end(), so.max.begin(), so.max.end());
    hb.push_back(0);   // never empty: the pointers below are not null
    if (so.present) { out->stats_flags |= PF_STATS_NULL_COUNT; out->null_count = so.null_count; }
    if (so.has_min_max) {
        out->stats_flags |= PF_STATS_MIN_MAX;
        out->stat_min_len = int32_t(so.min.size());
        out->stat_max_len = int32_t(so.max.size());
        out->stat_min = hb.data();
        out->stat_max = hb.data() + so.min.size();
    }
}

int chunk_index(const EncPlan& p, const AssembleIn& in, const AssembledChunk& ac, pf_encoded_chunk* out, const char** why) {
    out->index_pages = 0;
    out->page_offset = nullptr; out->page_size = nullptr; out->page_first_row = nullptr;
    out->column_index = 0; out->boundary_order = 0;
    out->index_null_pages = nullptr; out->index_null_counts = nullptr;
    out->index_values = nullptr; out->index_value_off = nullptr;
    if (!p.want_index) return PF_OK;
    const uint8_t* h = in.px;
    const PgIndexHead* hd = reinterpret_cast<const PgIndexHead*>(h);
    if (hd->value_bytes > p.px_cap && hd->valid) return reject(why, PF_ERR_HIP, "encode: the page index values exceed their block");
    out->index_pages = int32_t(p.n_px);
    out->page_offset = ac.pgoff->data();
    out->page_size = ac.pgsize->data();
    out->page_first_row = ac.pgrow->data();
    out->column_index = hd->valid ? 1 : 0;
    out->boundary_order = hd->valid ? int32_t(hd->order) : 0;
    out->index_null_pages = h + p.px_np;
    out->index_null_counts = reinterpret_cast<const int64_t*>(h + p.px_nc);
    if (hd->valid) {
        out->index_values = h + p.px_val;
        out->index_value_off = reinterpret_cast<const uint32_t*>(h + p.px_off);
    }
    return PF_OK;
}

}  // namespace

int assemble_chunk(const EncPlan& p, const AssembleIn& in, AssembledChunk& ac, pf_encoded_chunk* out, const char** why) {
    std::vector<uint8_t>& o = *ac.bytes;
    const std::vector<std::vector<uint8_t>>& bodies = *in.bodies;
    o.clear();
    int64_t unc = 0;
    size_t bi = 0;
    CrcFold fold{p, in};
    out->dictionary_page_offset = -1;
    if (p.dict) {
        PageHeaderOut h;
        h.page_type = PF_PAGE_DICTIONARY;
        h.uncompressed_size = int32_t(p.dict_bytes);
        h.compressed_size = int32_t(bodies[0].size());
        h.num_values = int32_t(p.D);
        h.encoding = PF_ENC_PLAIN;   // parquet-mr PARQUET_2_0: dictionary page PLAIN, data pages RLE_DICTIONARY
        if (p.want_crc) { h.has_crc = true; h.crc = fold.page(0, size_t(-1), {}); }
        out->dictionary_page_offset = 0;
        const size_t h0 = o.size();
        write_page_header(o, h);
        unc += int64_t(o.size() - h0) + p.dict_bytes;
        o.insert(o.end(), bodies[0].begin(), bodies[0].end());
        bi = 1;
    }
    out->data_page_offset = int64_t(o.size());
    ac.pgoff->assign(p.n_px, 0);
    ac.pgrow->assign(p.n_px, 0);
    ac.pgsize->assign(p.n_px, 0);
    std::vector<uint8_t> def;
    for (size_t i = 0; i < p.pp.size(); i++, bi++) {
        const EncPagePlan& g = p.pp[i];
        const int64_t rows = g.r1 - g.r0;
        page_levels(p, in, i, def);
        PageHeaderOut h;
        h.page_type = PF_PAGE_DATA_V2;
        h.uncompressed_size = int32_t(def.size() + p.sections[bi].second);
        h.compressed_size = int32_t(def.size() + bodies[bi].size());
        h.num_values = int32_t(rows);
        h.num_nulls = int32_t(rows - g.cnt);
        h.num_rows = int32_t(rows);
        h.encoding = p.data_enc;
        h.def_bytes = int32_t(def.size());
        h.is_compressed = p.compressed;
        if (p.want_crc) { h.has_crc = true; h.crc = fold.page(bi, i, def); }
        h.stats = stats_of(p, in, i, rows - g.cnt);
        const size_t h0 = o.size();
        write_page_header(o, h);
        unc += int64_t(o.size() - h0) + h.uncompressed_size;
        o.insert(o.end(), def.begin(), def.end());
        o.insert(o.end(), bodies[bi].begin(), bodies[bi].end());
        if (p.want_index) {   // the OffsetIndex entry: the host knows where it put the page
            (*ac.pgoff)[i] = int64_t(h0);
            (*ac.pgsize)[i] = int32_t(o.size() - h0);
            (*ac.pgrow)[i] = g.r0;
        }
    }
    if (fold.bad) return reject(why, PF_ERR_HIP, "encode: the CRC pieces of a page do not add up to its size");
    chunk_stats(p, in, *ac.stat, out);
    out->bytes = o.data();
    out->size = int64_t(o.size());
    out->total_uncompressed_size = unc;
    out->num_values = p.n;
    out->n_data_pages = int32_t(p.pp.size());
    out->dict_entries = int32_t(p.D);
    out->data_encoding = p.data_enc;
    out->fallback = p.fallback;
    out->codec = p.codec;
    out->snappy_ms = out->encode_ms = out->bloom_ms = 0.f;
    out->bloom = p.bloom ? in.bloom : nullptr;
    out->bloom_len = int32_t(p.bloom);
    if (const int rc = chunk_index(p, in, ac, out, why)) return rc;
    out->snappy_in = 0;
    out->snappy_out = 0;
    if (p.compressed)
        for (size_t i = 0; i < p.sections.size(); i++) {
            out->snappy_in += int64_t(p.sections[i].second);
            out->snappy_out += int64_t(bodies[i].size());
        }
    return PF_OK;
}

}  // namespace pf
