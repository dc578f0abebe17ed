// pf_enc_runtime.hip — the write path behind include/pfloor.h: pf_encode_chunk, pf_snappy_compress, pf_zstd_compress.
//
// Every decision is the host planner's (pf_enc_plan.cpp, no HIP call): this file grows the arenas to the sizes it
// plans, uploads its tables, launches the kernels (pf_encode.hip, pf_enc_*.hip) and waits at the three places where
// the plan needs a word from the device -- the dictionary's result, the size pass's bytes, the compressed bodies.
// pf_encode_chunk reads top to bottom as that sequence; the context is pf_ctx.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pf_ctx.h"
#include "pf_enc_plan.h"
#include "pf_encode.h"
#include "pfloor.h"

using namespace pf;

namespace {

// The buffers of one compress_sections call that its caller reads afterwards.
struct Compressed {
    std::vector<std::vector<uint8_t>> streams;   // per section: Snappy: varint length + block outputs; ZSTD: frame header + the jobs' blocks
    const CrcOut* crcs = nullptr;                // cp.np results (in pinned staging, valid until the next call)
    float kernel_ms = 0.f, crc_ms = 0.f;
};

// Compress `sections` (device, each [off, off + len) of `base`) with cp.codec into the slots of independent jobs of
// SC_BLOCK / ZC_BLOCK bytes. With `want_crc` (PF_ENCODE_PAGE_CRC): k_enc_crc right behind the compressor over every
// job's slot, in job order, then over `extra`; the results come back in the copy that brings the jobs' lengths.
int compress_sections(pf_ctx* ctx, const uint8_t* base, const std::vector<std::pair<uint64_t, uint64_t>>& sections, int codec,
                      bool want_crc, const std::vector<CrcPiece>* extra, CompressPlan& cp, Compressed& res) {
    hipStream_t st = ctx->stream;
    const bool zs = codec == PF_CODEC_ZSTD;
    plan_compress(sections, codec, want_crc, extra ? extra->size() : 0, cp);
    const size_t nj = cp.jobs.size(), np = cp.np;
    const uint32_t SLOT = cp.SLOT;
    HIPCHK(ctx, ctx->d_enc_out.ensure(cp.arena));
    uint8_t* d = static_cast<uint8_t*>(ctx->d_enc_out.p);
    bind_compress(cp, base, d, extra);
    // compressed lengths + slots come back into the context's pinned staging (no zero-fill, DMA speed)
    HIPCHK(ctx, ctx->h_enc_slots.ensure(align_up(cp.len_bytes, 256) + nj * size_t(SLOT)));
    uint32_t* lens = static_cast<uint32_t*>(ctx->h_enc_slots.p);
    uint8_t* slots = static_cast<uint8_t*>(ctx->h_enc_slots.p) + align_up(cp.len_bytes, 256);
    if (nj) {
        HIPCHK(ctx, hipMemcpyAsync(d + cp.o_jobs, cp.jobs.data(), sizeof(CompJob) * nj, hipMemcpyHostToDevice, st));
        EVREC(ctx, ctx->ev[0], st);
        (zs ? launch_zstd_compress : launch_snappy_compress)(reinterpret_cast<const CompJob*>(d + cp.o_jobs), int(nj),
                                                              reinterpret_cast<uint32_t*>(d + cp.o_len), st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev[1], st);
    }
    if (np) {
        HIPCHK(ctx, hipMemcpyAsync(d + cp.o_pieces, cp.pieces.data(), sizeof(CrcPiece) * np, hipMemcpyHostToDevice, st));
        EVREC(ctx, ctx->ev[8], st);
        launch_enc_crc(reinterpret_cast<const CrcPiece*>(d + cp.o_pieces), int(np), reinterpret_cast<CrcOut*>(d + cp.o_len + cp.o_crc_in_len), st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev[9], st);
    }
    if (nj || np) HIPCHK(ctx, hipMemcpyAsync(lens, d + cp.o_len, np ? cp.len_bytes : 4 * nj, hipMemcpyDeviceToHost, st));
    if (nj) HIPCHK(ctx, hipMemcpyAsync(slots, d + cp.o_slots, nj * size_t(SLOT), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    res.crcs = reinterpret_cast<const CrcOut*>(reinterpret_cast<const uint8_t*>(lens) + cp.o_crc_in_len);
    res.crc_ms = res.kernel_ms = 0.f;
    if (ctx->timing && np) HIPCHK(ctx, hipEventElapsedTime(&res.crc_ms, ctx->ev[8], ctx->ev[9]));
    if (ctx->timing && nj) HIPCHK(ctx, hipEventElapsedTime(&res.kernel_ms, ctx->ev[0], ctx->ev[1]));
    res.streams.assign(sections.size(), {});
    for (size_t i = 0; i < sections.size(); i++) {
        std::vector<uint8_t>& o = res.streams[i];
        uint8_t head[12];
        o.assign(head, head + stream_head(codec, sections[i].second, head));
        for (size_t k = cp.range[i].first; k < cp.range[i].second; k++) {
            if (lens[k] > (zs ? 3 + cp.jobs[k].len : SLOT)) return fail(ctx, PF_ERR_HIP, zs ? "zstd compress: block overflow" : "snappy compress: block overflow");
            const uint8_t* b = slots + k * size_t(SLOT);
            o.insert(o.end(), b, b + lens[k]);
        }
    }
    return PF_OK;
}

// pf_snappy_compress / pf_zstd_compress: one host buffer as one section. `name` prefixes the messages.
int compress_buffer(pf_ctx* ctx, int codec, const std::string& name, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    if (!ctx || (!src && n) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n > 0xffffffffull) return fail(ctx, PF_ERR_INVALID_ARG, name + ": buffer too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
    HIPCHK(ctx, ctx->d_enc.ensure(std::max<size_t>(n, 1)));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_enc.p, src, n, hipMemcpyHostToDevice, ctx->stream));
    CompressPlan cp;
    Compressed res;
    const int rc = compress_sections(ctx, static_cast<const uint8_t*>(ctx->d_enc.p), {{0, n}}, codec, false, nullptr, cp, res);
    if (rc) return rc;
    const std::vector<uint8_t>& s = res.streams[0];
    *out_len = s.size();
    if (s.size() > cap) return fail(ctx, PF_ERR_CAPACITY, name + ": destination too small");
    std::memcpy(dst, s.data(), s.size());
    return PF_OK;
}

// What one pf_encode_chunk carries from step to step beside the plan.
struct EncRun {
    pf_ctx* ctx;
    const pf_encode_column* col;
    bool on_device;
    EncPlan p;
    std::vector<uint8_t> hval;   // host copies of validity / offsets (page plan, definition levels)
    std::vector<int32_t> hoff;
    uint32_t hres[3] = {0, 0, 0};   // collide, dictionary entries, dictionary bytes
    float enc_ms = 0.f, snap_ms = 0.f, crc_ms = 0.f;
    std::vector<std::vector<uint8_t>> bodies;
    std::vector<uint8_t> hlv;       // hybrid runs: the pages' levels
    std::vector<uint8_t> all;       // UNCOMPRESSED: the sections as they lie in d_enc_sec
    std::vector<CrcOut> crcs;
    Compressed comp;
};

// 1. validate and plan: the checks that need no array, the host copies of validity / offsets, the plan
int enc_plan(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    const pf_encode_column* col = r.col;
    const char* why = "";
    if (const int rc = check_encode_args(col, &why)) return fail(ctx, rc, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
    const int64_t n = col->num_rows;
    const size_t vbytes = size_t((n + 7) / 8);
    if (col->max_def == 1 && col->validity) {
        r.hval.resize(vbytes);
        if (r.on_device) HIPCHK(ctx, hipMemcpy(r.hval.data(), col->validity, vbytes, hipMemcpyDeviceToHost));
        else std::memcpy(r.hval.data(), col->validity, vbytes);
    }
    if (col->physical_type == PF_BYTE_ARRAY && n > 0) {
        r.hoff.resize(size_t(n) + 1);
        if (r.on_device) HIPCHK(ctx, hipMemcpy(r.hoff.data(), col->offsets, 4 * (size_t(n) + 1), hipMemcpyDeviceToHost));
        else std::memcpy(r.hoff.data(), col->offsets, 4 * (size_t(n) + 1));
    }
    if (const int rc = plan_encode(col, r.hval, r.hoff, r.p, &why)) return fail(ctx, rc, why);
    return PF_OK;
}

// 2. ensure the arena, bind; 3. upload the host inputs
int enc_arena_upload(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    const pf_encode_column* col = r.col;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    size_t temp_bytes = 0;
    HIPCHK(ctx, enc_scan_temp(p.scan_elems, temp_bytes));
    layout_encode(p, temp_bytes);
    HIPCHK(ctx, ctx->d_enc.ensure(p.a_sz));
    uint8_t* A = static_cast<uint8_t*>(ctx->d_enc.p);
    bind_encode(p, A, col, r.on_device);
    if (r.on_device) return PF_OK;
    const size_t n = size_t(p.n);
    if (!p.str && n) HIPCHK(ctx, hipMemcpyAsync(A + p.reg[R_IN].off, col->values, n * p.w, hipMemcpyHostToDevice, st));
    if (p.has_val && p.vbytes) HIPCHK(ctx, hipMemcpyAsync(A + p.reg[R_VL].off, r.hval.data(), p.vbytes, hipMemcpyHostToDevice, st));
    if (p.str && n) {
        HIPCHK(ctx, hipMemcpyAsync(A + p.reg[R_OF].off, r.hoff.data(), 4 * (n + 1), hipMemcpyHostToDevice, st));
        if (col->chars_len) HIPCHK(ctx, hipMemcpyAsync(A + p.reg[R_CH].off, col->chars, size_t(col->chars_len), hipMemcpyHostToDevice, st));
    }
    return PF_OK;
}

// 4. dense values, PLAIN sizes, dictionary; the dictionary's three words come back under the first sync
int enc_dense_dictionary(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    const EncArgs& ea = p.ea;
    HIPCHK(ctx, hipMemsetAsync(ea.collide, 0, 256, st));
    if (p.str) HIPCHK(ctx, hipMemsetAsync(ea.vsz, 0, 4 * (size_t(p.n) + 1), st));
    EVREC(ctx, ctx->ev[2], st);
    if (p.n) HIPCHK(ctx, enc_dense(ea, p.temp, p.temp_bytes, st));
    if (p.str) HIPCHK(ctx, enc_plain_sizes(ea, p.m, p.temp, p.temp_bytes, st));
    if (p.want_dict) {
        HIPCHK(ctx, enc_dictionary(ea, p.m, p.w == 4 ? 32 : 64, p.temp, p.temp_bytes, st));
        EVREC(ctx, ctx->ev[3], st);
        HIPCHK(ctx, hipMemcpyAsync(&r.hres[0], ea.collide, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&r.hres[1], ea.did + p.m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&r.hres[2], ea.doff + p.m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&r.enc_ms, ctx->ev[2], ctx->ev[3]));
    }
    plan_values(p, r.hres[0], r.hres[1], r.hres[2]);
    return PF_OK;
}

// Hybrid streams' size pass (after the ids, which it reads): the streams' bytes in one D2H and one sync.
int enc_hybrid_size_pass(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    if (!p.delta) {
        // The dictionary page and the ids are written before the size pass, into the worst case plan_values reserved;
        // plan_sections stays inside it, so d_enc_sec is not grown (and nothing moves) again on this route
        HIPCHK(ctx, ctx->d_enc_sec.ensure(p.ub));
        p.ea.dict_out = static_cast<uint8_t*>(ctx->d_enc_sec.p) + p.o_dict;
    }
    EVREC(ctx, ctx->ev[6], st);
    if (p.dict) enc_dictionary_page_and_ids(p.ea, p.m, st);
    if (!p.hs.empty()) {
        HIPCHK(ctx, hipMemcpyAsync(const_cast<HybridStream*>(p.ha.streams), p.hs.data(), sizeof(HybridStream) * p.hs.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, enc_hybrid_sizes(p.ha, st));
    }
    EVREC(ctx, ctx->ev[7], st);
    if (!p.hs.empty()) HIPCHK(ctx, hipMemcpyAsync(p.hbytes.data(), p.ha.bytes, 4 * p.hs.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (ctx->timing) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
        r.enc_ms += ms;
    }
    return PF_OK;
}

// DELTA_* size pass -> scan -> page totals (one D2H, one sync)
int enc_delta_size_pass(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    const DeltaArgs& da = p.da;
    EVREC(ctx, ctx->ev[4], st);
    HIPCHK(ctx, hipMemcpyAsync(const_cast<DeltaStream*>(da.streams), p.dstreams.data(), sizeof(DeltaStream) * p.dstreams.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(const_cast<DeltaPage*>(da.pages), p.dpages.data(), sizeof(DeltaPage) * p.dpages.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(da.bytes + p.n_items, 0, 4, st));
    if (p.str) HIPCHK(ctx, enc_delta_prefix(p.ea, da, p.m, p.temp, p.temp_bytes, st));
    HIPCHK(ctx, enc_delta_sizes(da, p.temp, p.temp_bytes, st));
    p.htot.assign(p.dpages.size(), 0);
    HIPCHK(ctx, hipMemcpyAsync(p.htot.data(), da.totals, 4 * p.htot.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PF_OK;
}

// 6. the write pass over the planned sections
int enc_write_pass(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, ctx->d_enc_sec.ensure(p.vo));   // hybrid runs, not delta: within the worst case reserved before the size pass
    uint8_t* SEC = static_cast<uint8_t*>(ctx->d_enc_sec.p);
    if (p.delta) {
        p.da.out = SEC;
        HIPCHK(ctx, hipMemcpyAsync(const_cast<DeltaPage*>(p.da.pages), p.dpages.data(), sizeof(DeltaPage) * p.dpages.size(), hipMemcpyHostToDevice, st));
        enc_delta_write(p.ea, p.da, p.m, st);
    } else {   // RLE_DICTIONARY or PLAIN: the host knows every page's size (hybrid runs: after their size pass)
        p.ea.dict_out = SEC + p.o_dict;
        p.ea.vals_out = SEC;
        EVREC(ctx, ctx->ev[4], st);
        if (p.dict && !p.hyb) enc_dictionary_page_and_ids(p.ea, p.m, st);
        HIPCHK(ctx, hipMemcpyAsync(SEC + p.o_pages, p.ep.data(), sizeof(EncPage) * p.ep.size(), hipMemcpyHostToDevice, st));
        if (!(p.hyb && (p.dict || p.brle))) enc_pages(p.ea, reinterpret_cast<const EncPage*>(SEC + p.o_pages), int(p.ep.size()), st);
    }
    if (p.hyb && !p.hs.empty()) {
        p.ha.out = SEC;
        HIPCHK(ctx, hipMemcpyAsync(const_cast<HybridStream*>(p.ha.streams), p.hs.data(), sizeof(HybridStream) * p.hs.size(), hipMemcpyHostToDevice, st));
        enc_hybrid_write(p.ha, st);
    }
    HIPCHK(ctx, hipGetLastError());
    return PF_OK;
}

// Statistics and page index: the kernels run with the page kernels (their time is in encode_ms), the results come
// back in pinned memory with the synchronisation the bodies wait for anyway.
int enc_stats_index(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    if (p.run_stats) {
        if (!p.stiles.empty())
            HIPCHK(ctx, hipMemcpyAsync(const_cast<StatTile*>(p.sa.tiles), p.stiles.data(), sizeof(StatTile) * p.stiles.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(const_cast<uint32_t*>(p.sa.ptile), p.sptile.data(), 4 * p.sptile.size(), hipMemcpyHostToDevice, st));
        enc_stats(p.ea, p.sa, st);
        HIPCHK(ctx, hipGetLastError());
        if (p.want_index) {
            HIPCHK(ctx, hipMemcpyAsync(const_cast<uint32_t*>(p.xa.rows), p.px_in.data(), 8 * p.n_px, hipMemcpyHostToDevice, st));
            enc_pgindex(p.ea, p.xa, st);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    EVREC(ctx, ctx->ev[5], st);
    if (p.want_index) {   // one block, in pinned memory, under the synchronisation the bodies wait for
        HIPCHK(ctx, ctx->h_enc_px.ensure(p.px_bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_enc_px.p, p.xa.head, p.px_bytes, hipMemcpyDeviceToHost, st));
    }
    if (p.want_stats) {
        const size_t st_bytes = sizeof(StatPart) * p.n_se + (p.str ? size_t(ST_LIMIT) * p.n_se : 0);
        HIPCHK(ctx, ctx->h_enc_st.ensure(st_bytes));
        uint8_t* h = static_cast<uint8_t*>(ctx->h_enc_st.p);
        HIPCHK(ctx, hipMemcpyAsync(h, p.sa.out, sizeof(StatPart) * p.n_se, hipMemcpyDeviceToHost, st));
        if (p.str) HIPCHK(ctx, hipMemcpyAsync(h + sizeof(StatPart) * p.n_se, p.sa.bytes, size_t(ST_LIMIT) * p.n_se, hipMemcpyDeviceToHost, st));
    }
    return PF_OK;
}

// Bloom filter (bloom_bytes): zeroed and filled on the stream behind the page kernels, outside encode_ms (events of
// its own); the bitset comes back in pinned memory with the copy and synchronisation the bodies wait for anyway.
int enc_bloom_filter(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    if (!p.bloom) return PF_OK;
    HIPCHK(ctx, ctx->h_enc_bloom.ensure(p.bloom));
    EVREC(ctx, ctx->ev_bloom[0], st);
    HIPCHK(ctx, hipMemsetAsync(p.d_bloom, 0, p.bloom, st));
    enc_bloom(p.ea, p.m, reinterpret_cast<uint32_t*>(p.d_bloom), uint32_t(p.bloom), p.dict && ctx->opts.bloom_first, st);
    HIPCHK(ctx, hipGetLastError());
    EVREC(ctx, ctx->ev_bloom[1], st);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_enc_bloom.p, p.d_bloom, p.bloom, hipMemcpyDeviceToHost, st));
    return PF_OK;
}

// 7. compress (or copy the sections as they are), CRC pieces, the sync the bodies wait for
int enc_bodies(EncRun& r) {
    pf_ctx* ctx = r.ctx;
    EncPlan& p = r.p;
    hipStream_t st = ctx->stream;
    const uint8_t* SEC = static_cast<const uint8_t*>(ctx->d_enc_sec.p);
    const char* why = "";
    plan_crc_levels(p, SEC);
    r.hlv.resize(p.lv_total);
    if (p.compressed) {
        if (p.lv_total) HIPCHK(ctx, hipMemcpyAsync(r.hlv.data(), SEC + p.o_lv, p.lv_total, hipMemcpyDeviceToHost, st));
        if (const int rc = compress_sections(ctx, SEC, p.sections, p.codec, p.want_crc, &p.lv_pieces, p.comp, r.comp)) return rc;
        r.bodies.swap(r.comp.streams);
        r.snap_ms = r.comp.kernel_ms;
        r.crc_ms = r.comp.crc_ms;
        if (p.want_crc) r.crcs.assign(r.comp.crcs, r.comp.crcs + p.comp.np);
        return PF_OK;
    }
    if (p.want_crc) {   // the table and the results in d_enc_out, which an uncompressed chunk does not use otherwise
        if (const int rc = plan_section_pieces(p, SEC, &why)) return fail(ctx, rc, why);
        const size_t npc = p.sec_pieces.size();
        HIPCHK(ctx, ctx->d_enc_out.ensure(p.o_crc_res + sizeof(CrcOut) * npc));
        uint8_t* d = static_cast<uint8_t*>(ctx->d_enc_out.p);
        r.crcs.resize(npc);
        HIPCHK(ctx, hipMemcpyAsync(d, p.sec_pieces.data(), sizeof(CrcPiece) * npc, hipMemcpyHostToDevice, st));
        EVREC(ctx, ctx->ev[8], st);
        launch_enc_crc(reinterpret_cast<const CrcPiece*>(d), int(npc), reinterpret_cast<CrcOut*>(d + p.o_crc_res), st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev[9], st);
        HIPCHK(ctx, hipMemcpyAsync(r.crcs.data(), d + p.o_crc_res, sizeof(CrcOut) * npc, hipMemcpyDeviceToHost, st));
    }
    r.all.resize(p.vo);
    HIPCHK(ctx, hipMemcpyAsync(r.all.data(), SEC, p.vo, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (p.want_crc && ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&r.crc_ms, ctx->ev[8], ctx->ev[9]));
    if (p.lv_total) std::memcpy(r.hlv.data(), r.all.data() + p.o_lv, p.lv_total);
    for (const auto& sct : p.sections) r.bodies.emplace_back(r.all.begin() + sct.first, r.all.begin() + sct.first + sct.second);
    return PF_OK;
}

// 8. assemble: page headers + bodies into the context's vectors, then the event timers
int enc_assemble(EncRun& r, pf_encoded_chunk* out) {
    pf_ctx* ctx = r.ctx;
    const EncPlan& p = r.p;
    AssembleIn in{};
    in.hval = &r.hval;
    in.bodies = &r.bodies;
    in.hlv = r.hlv.data();
    in.crcs = r.crcs.data();
    in.crc_first_lv = p.compressed ? p.comp.jobs.size() : p.sections.size();
    in.hst = p.want_stats ? static_cast<const StatPart*>(ctx->h_enc_st.p) : nullptr;
    in.hsb = p.want_stats ? static_cast<const uint8_t*>(ctx->h_enc_st.p) + sizeof(StatPart) * p.n_se : nullptr;
    in.px = p.want_index ? static_cast<const uint8_t*>(ctx->h_enc_px.p) : nullptr;
    in.bloom = p.bloom ? static_cast<const uint8_t*>(ctx->h_enc_bloom.p) : nullptr;
    AssembledChunk ac{&ctx->h_enc, &ctx->h_enc_stat, &ctx->h_enc_pgoff, &ctx->h_enc_pgrow, &ctx->h_enc_pgsize};
    const char* why = "";
    if (const int rc = assemble_chunk(p, in, ac, out, &why)) return fail(ctx, rc, why);
    if (ctx->timing) {   // the page kernels' events have completed (the stream was synchronised since)
        float pg_ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&pg_ms, ctx->ev[4], ctx->ev[5]));
        r.enc_ms += pg_ms + r.crc_ms;
    }
    out->snappy_ms = r.snap_ms;
    out->encode_ms = r.enc_ms;
    if (p.bloom && ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&out->bloom_ms, ctx->ev_bloom[0], ctx->ev_bloom[1]));
    return PF_OK;
}

}  // namespace

extern "C" int pf_snappy_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    return compress_buffer(ctx, PF_CODEC_SNAPPY, "snappy", src, n, dst, cap, out_len);
}

extern "C" int pf_zstd_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    return compress_buffer(ctx, PF_CODEC_ZSTD, "zstd", src, n, dst, cap, out_len);
}

extern "C" int pf_encode_chunk(pf_ctx* ctx, const pf_encode_column* col, int on_device, pf_encoded_chunk* out) {
    if (!ctx || !col || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    EncRun r{ctx, col, on_device != 0};
    const char* why = "";
    int rc = enc_plan(r);                                    // 1. validate and plan
    if (!rc) rc = enc_arena_upload(r);                       // 2. ensure the arena, bind  3. upload
    if (!rc) rc = enc_dense_dictionary(r);                   // 4. dense / dictionary, sync
    if (!rc && r.p.hyb) rc = enc_hybrid_size_pass(r);        // 5. size pass, sync
    if (!rc && r.p.delta) rc = enc_delta_size_pass(r);
    if (!rc && (rc = plan_sections(r.p, &why))) return fail(ctx, rc, why);
    if (!rc) rc = enc_write_pass(r);                         // 6. write pass, statistics, page index, Bloom filter
    if (!rc) rc = enc_stats_index(r);
    if (!rc) rc = enc_bloom_filter(r);
    if (!rc) rc = enc_bodies(r);                             // 7. compress, CRC, sync
    if (!rc) rc = enc_assemble(r, out);                      // 8. assemble
    return rc;
}
