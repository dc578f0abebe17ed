// pf_runtime.hip — context, arenas and kernel orchestration behind include/pfloor.h.
//
// One pf_ctx per GPU (one HIP stream, growable HBM arenas, pinned staging). A decode batch is
// any set of column chunks (a row group's selected columns, or several row groups). The host
// planner (pf_plan.cpp, no HIP calls) turns the descriptors into flat DevChunk / DevPage /
// SnappyJob tables, launch lists and arena sizes; this file grows the arenas to those sizes, has
// the planner bind its offsets to them, uploads the tables in one copy, and enqueues
//   k_snappy / k_zstd / k_lz4 -> k_ba (dictionaries) -> k_delta -> k_count -> k_ba (PLAIN pages) -> k_scan -> k_flat -> k_decode
// on the context stream. Nothing synchronises until pf_wait, which hands what came down to the host-only result
// side (pf_result.cpp: side-table layouts, the rerun decision, pf_column_info). The context itself is pf_ctx.h; the
// write path is a unit of its own, pf_enc_runtime.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "pf_ctx.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "pf_plan.h"
#include "pf_snappy_par.h"
#include "pfloor.h"

using namespace pf;

static_assert(sizeof(Int2) == sizeof(int2) && alignof(Int2) <= alignof(int2), "the planner's pairs are the kernels' int2");

namespace {

thread_local std::string g_err;

// Copies between pinned host pages and device memory by a kernel on the decode stream: two ranges
// of 8-byte words, grid-stride. The batch's metadata upload and its results download were SDMA /
// blit copies on the stream (PF_ZC=0): config 1 0.41 -> 0.39 ms, the others unchanged.
// (An upload stream of its own, event-joined, made every config slower: SF1 3.13 -> 4.4 ms.)
__global__ __launch_bounds__(256) void k_copy_words(uint64_t* __restrict__ d0, const uint64_t* __restrict__ s0, uint32_t n0,
                                                    uint64_t* __restrict__ d1, const uint64_t* __restrict__ s1, uint32_t n1) {
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n0 + n1; i += stride) {
        if (i < n0) d0[i] = s0[i];
        else d1[i - n0] = s1[i - n0];
    }
}
static_assert(sizeof(DevChunkResult) % 8 == 0 && sizeof(DevChunk) % 8 == 0, "k_copy_words moves 8-byte words");
// The batch's metadata upload (pinned host words -> device) and the zeroing of its validity arena and
// window hand-over words in one launch (round 5: two hipMemsetAsync fills were two more dependent
// launches at the head of every batch's chain). z0 / z1: 8-byte aligned, nz0 / nz1 bytes.
__global__ __launch_bounds__(256) void k_upload(uint64_t* __restrict__ d, const uint64_t* __restrict__ s, uint32_t n,
                                                uint8_t* __restrict__ z0, uint32_t nz0, uint8_t* __restrict__ z1, uint32_t nz1) {
    const uint32_t stride = gridDim.x * 256u;
    const uint32_t w0 = (nz0 + 7u) / 8u, w1 = (nz1 + 7u) / 8u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n + w0 + w1; i += stride) {
        if (i < n) { d[i] = s[i]; continue; }
        const bool first = i < n + w0;
        uint8_t* z = first ? z0 : z1;
        const uint32_t w = first ? i - n : i - n - w0, nz = first ? nz0 : nz1;
        if (8u * w + 8u <= nz) reinterpret_cast<uint64_t*>(z)[w] = 0;
        else for (uint32_t b = 8u * w; b < nz; b++) z[b] = 0;
    }
}
inline void copy_words(void* d0, const void* s0, size_t b0, void* d1, const void* s1, size_t b1, hipStream_t st) {
    const uint32_t n0 = uint32_t(b0 / 8), n1 = uint32_t(b1 / 8);
    const uint32_t grid = std::max(1u, std::min(1024u, (n0 + n1 + 255u) / 256u));
    hipLaunchKernelGGL(k_copy_words, dim3(grid), dim3(256), 0, st, static_cast<uint64_t*>(d0), static_cast<const uint64_t*>(s0), n0,
                       static_cast<uint64_t*>(d1), static_cast<const uint64_t*>(s1), n1);
}

// A decoded batch into pinned host memory by a kernel writing through the pages' device address
// (round 6): the SDMA engines move one direction at a time on this link -- an SDMA H2D and an SDMA D2H
// together make 57 GB/s, an SDMA H2D beside this kernel's D2H 86 GB/s (profiles/r06_e2e/duplex.txt) --
// so the next batch's H2D (pf_decode_row_group's SDMA copy) runs under this batch's download. Up to
// three ranges (the output arenas), 16-byte chunks grid-stride, the ranges' last < 16 bytes by block 0.
struct DlRange {
    uint8_t* d;
    const uint8_t* s;
    uint64_t n;
};
__global__ __launch_bounds__(256) void k_download(DlRange r0, DlRange r1, DlRange r2) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint64_t c0 = r0.n >> 4, c1 = r1.n >> 4, c2 = r2.n >> 4;
    const uint64_t stride = uint64_t(gridDim.x) * 256u;
    for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < c0 + c1 + c2; i += stride) {
        const DlRange& r = i < c0 ? r0 : (i < c0 + c1 ? r1 : r2);
        const uint64_t j = i < c0 ? i : (i < c0 + c1 ? i - c0 : i - c0 - c1);
        reinterpret_cast<u4*>(r.d)[j] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(r.s) + j);
    }
    if (blockIdx.x == 0 && threadIdx.x < 48) {
        const DlRange& r = threadIdx.x < 16 ? r0 : (threadIdx.x < 32 ? r1 : r2);
        const uint64_t b = (r.n & ~uint64_t(15)) + (threadIdx.x & 15u);
        if (b < r.n) r.d[b] = r.s[b];
    }
}

}  // namespace

namespace pf {
int fail(pf_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    g_err = msg;
    return code;
}
}  // namespace pf

namespace {

// k_count / k_decode blocks when no page is known to need them: both stride over their whole list,
// and nearly every page was taken by another kernel (k_count_flat, the flat kernels)
constexpr int COUNT_IDLE_GRID = 64;
constexpr int DECODE_IDLE_GRID = 32;

// Enqueue the kernels of the planned batch (metadata already on device).
int enqueue_kernels(pf_ctx* ctx) {
    hipStream_t st = ctx->stream;
    const BatchPlan& p = ctx->plan;
    uint8_t* meta = static_cast<uint8_t*>(ctx->d_meta.p);
    DevChunk* d_chunks = reinterpret_cast<DevChunk*>(meta + p.off_chunks);
    DevPage* d_pages = reinterpret_cast<DevPage*>(meta + p.off_pages);
    SnappyJob* d_jobs = reinterpret_cast<SnappyJob*>(meta + p.off_jobs);
    DevChunkResult* d_res = reinterpret_cast<DevChunkResult*>(meta + p.off_res);
    auto list = [&](ListId l) { return reinterpret_cast<int*>(meta + p.off_lists) + p.list_base[l]; };
    auto pairs = [&](ListId l) { return reinterpret_cast<const int2*>(list(l)); };
    auto len = [&](ListId l) { return int(p.lists[l].size()); };
    const int n_jobs = int(p.jobs.size()), n_nest = len(L_NEST), n_nseg = len(L_NSEG) / 2;
    unsigned long long* used = reinterpret_cast<unsigned long long*>(meta + p.meta_bytes - 256);
    const int2* d_pieces = reinterpret_cast<const int2*>(meta + p.off_pieces);
    uint32_t* d_splits = reinterpret_cast<uint32_t*>(meta + p.off_splits);
    int* d_fallback = reinterpret_cast<int*>(meta + p.off_fallback);
    const int2* d_wins = reinterpret_cast<const int2*>(meta + p.off_wins);

    // diagnostics build only (bench analysis, results are wrong): stages left out of every batch, so a
    // step's time without them shows what they cost under load
#ifdef PF_DIAG
    const unsigned skip = ctx->opts.debug_skip;
#else
    constexpr unsigned skip = 0;
#endif
    if (!ctx->meta_by_kernel) {   // (the zero-copy upload, k_upload, zeroes them)
        if (p.bits_bytes) HIPCHK(ctx, hipMemsetAsync(ctx->d_bits.p, 0, p.bits_bytes, st));
        if (p.npub_bytes) HIPCHK(ctx, hipMemsetAsync(static_cast<uint8_t*>(ctx->d_scratch.p) + p.off_npub, 0, p.npub_bytes, st));
    }
    EVREC(ctx, ctx->ev[1], st);
    // single-literal pages in place, PLAIN fixed-width pages straight into the column (pf_snappy_head.hip)
    if (!(skip & 1u)) launch_snappy_head(d_jobs, n_jobs, d_pages, d_chunks, d_fallback, d_res, st);
    if (!(skip & 1u)) launch_snappy_litcopy(d_jobs, list(L_DJOBS), len(L_DJOBS), d_fallback, st);
    if (!(skip & 1u)) launch_snappy_parse(d_jobs, n_jobs, d_wins, int(p.snap.wins.size()), p.snap.d_win, p.snap.d_ent,
                        p.snap.d_lane_out, d_splits, d_fallback, p.snap.max_snap_win, st);
    EVREC(ctx, ctx->ev[2], st);
    if (!(skip & 2u))
        launch_snappy_exec(d_jobs, n_jobs, d_pieces, int(p.snap.pieces.size()), d_splits, d_fallback, d_res, ctx->opts.exec, st);
    // ZSTD pages (a batch without one enqueues nothing here)
    launch_zstd(reinterpret_cast<ZstdJob*>(meta + p.off_zjobs), list(L_ZSTD), int(p.zjobs.size()),
                static_cast<uint8_t*>(ctx->d_scratch.p) + p.off_zlit, p.zlit_stride, d_res, st);
    // LZ4_RAW pages (likewise)
    launch_lz4(reinterpret_cast<Lz4Job*>(meta + p.off_ljobs), list(L_LZ4), int(p.ljobs.size()), d_res, st);
    EVREC(ctx, ctx->ev[3], st);
    BaJob* d_bajobs = reinterpret_cast<BaJob*>(meta + p.off_bajobs);
    const int2* d_batiles = reinterpret_cast<const int2*>(meta + p.off_batiles);
    const int n_ba = int(p.bajobs.size()), n_bt = int(p.ba_tiles.size());
    if (!(skip & 4u)) launch_ba(d_bajobs, p.n_ba_dict, d_batiles, p.n_ba_dict_tiles, d_res, st, p.ba_short_dict && ctx->opts.ba_fused);
    EVREC(ctx, ctx->ev[4], st);
    launch_delta(d_chunks, d_pages, list(L_DELTA), len(L_DELTA), p.max_dbp_nwin, d_res, st);
    EVREC(ctx, ctx->ev[5], st);
    if (!(skip & 8u)) launch_runs(d_chunks, d_pages, list(L_RUNS), len(L_RUNS), d_res, st);
    NullCaps ncaps = p.null_caps;
    if (ctx->opts.null_dcap) ncaps.dcap = ctx->opts.null_dcap;
    if (!(skip & 8u)) launch_lvl(d_chunks, d_pages, list(L_LVL), len(L_LVL), d_res, st, ctx->opts.page_null, ncaps);
    launch_dlen(d_chunks, d_pages, list(L_DLEN), len(L_DLEN), d_res, st);
    EVREC(ctx, ctx->ev[6], st);
    launch_nest_lvl(d_chunks, d_pages, list(L_NEST), n_nest, p.max_nwin, d_res, st, ctx->opts.nest_timeout);
    if (!(skip & 16u)) {
        launch_count_flat(d_chunks, d_pages, list(L_COUNT), len(L_COUNT), p.n_count_flat, pairs(L_CDICT), len(L_CDICT) / 2,
                          d_res, d_bajobs, st);
        launch_count(d_chunks, d_pages, list(L_COUNT), len(L_COUNT), d_res, d_bajobs, st, COUNT_IDLE_GRID);
    }
    launch_nest_count(d_chunks, d_pages, list(L_NEST), n_nest, pairs(L_NSEG), n_nseg, d_res, st);
    if (!(skip & 4u))
        launch_ba(d_bajobs + p.n_ba_dict, n_ba - p.n_ba_dict, d_batiles + p.n_ba_dict_tiles, n_bt - p.n_ba_dict_tiles,
                  d_res, st, p.ba_short_data && ctx->opts.ba_fused);
    EVREC(ctx, ctx->ev[7], st);
    launch_scan(d_chunks, d_pages, list(L_SCAN), len(L_SCAN), d_res, static_cast<uint8_t*>(ctx->d_chars.p),
                ctx->d_chars.cap, used, st);
    EVREC(ctx, ctx->ev[8], st);
    if (!(skip & 32u))
        launch_flat(d_chunks, d_pages, list(L_FLAT), p.n_flat_fixed, p.n_flat_all, p.n_null4, p.n_null8,
                    reinterpret_cast<int*>(meta + p.off_nfbq), pairs(L_CDICT), ctx->opts.flat_dstr ? len(L_CDICT) / 2 : 0, d_res, st,
                    ncaps, ctx->opts.null_stagger);
    // kept-dictionary chunks: indices, dictionary offsets and chars (nothing for a batch without one)
    const int n_keeps = int(p.keeps.size());
    if (n_keeps > 0 && !(skip & 32u))
        launch_flat_ids(d_chunks, d_pages, pairs(L_IDS), len(L_IDS) / 2, reinterpret_cast<DevKeep*>(meta + p.off_keeps), n_keeps,
                        reinterpret_cast<const int*>(meta + p.off_keepof), d_res, static_cast<uint8_t*>(ctx->d_chars.p),
                        ctx->d_chars.cap, used, st);
    EVREC(ctx, ctx->ev[9], st);
    if (!(skip & 64u)) launch_decode(d_chunks, d_pages, list(L_DECODE), len(L_DECODE), p.n_decode_first, d_res, st, DECODE_IDLE_GRID);
    launch_nest_decode(d_chunks, d_pages, pairs(L_NSEG), n_nseg, d_res, st);
    launch_dba_chars(d_chunks, d_pages, list(L_DBA), len(L_DBA), d_res, st);
    EVREC(ctx, ctx->ev[10], st);
    const WinLayout& wl = ctx->win_lay;
    const bool windowed = !ctx->wins.empty();
    DevWinRes* d_wres = windowed ? reinterpret_cast<DevWinRes*>(static_cast<uint8_t*>(ctx->d_win.p) + wl.res_off) : nullptr;
    if (windowed) {   // row windows: after every decode stage, so a chars rerun trims again
        EVREC(ctx, ctx->ev_win[0], st);
        launch_window(d_chunks, d_res, static_cast<DevWin*>(ctx->d_win.p), d_wres, int(ctx->wins.size()), ctx->win_grid,
                      static_cast<const uint8_t*>(ctx->d_chars.p), static_cast<uint8_t*>(ctx->d_wchars.p), ctx->twin.out,
                      ctx->twin.bits, n_keeps > 0 ? reinterpret_cast<const int*>(meta + p.off_keepof) : nullptr,
                      n_keeps > 0 ? reinterpret_cast<const DevKeep*>(meta + p.off_keeps) : nullptr, st);
        EVREC(ctx, ctx->ev_win[1], st);
        HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->h_win.p) + wl.res_off, d_wres, wl.res_bytes, hipMemcpyDeviceToHost, st));
    }
    if (ctx->filtered()) {   // the row filter: after the windows, so it sees their rows and a chars rerun filters again
        EVREC(ctx, ctx->ev_sel[0], st);
        launch_filter(d_chunks, d_res, d_wres, ctx->sel, ctx->sel_dict, ctx->n_chunks, ctx->sel_lay.grid, static_cast<const uint8_t*>(ctx->d_chars.p),
                      static_cast<uint8_t*>(ctx->d_wchars.p), ctx->twin.out, ctx->twin.bits, st);
        EVREC(ctx, ctx->ev_sel[1], st);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_sel.p, ctx->d_sel.p, ctx->sel_lay.o_up, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipGetLastError());
    if (n_keeps > 0)   // the kept dictionaries' device-written fields (chars base and size)
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_keep.p, meta + p.off_keeps, sizeof(DevKeep) * size_t(n_keeps), hipMemcpyDeviceToHost, st));
    // results + device-written chunk fields (chars base) back to pinned host memory
    const ResLayout& rl = ctx->res_lay;
    if (ctx->zc && ctx->h_res.d) {
        copy_words(ctx->h_res.d, meta + p.off_res, rl.res_bytes, static_cast<uint8_t*>(ctx->h_res.d) + rl.chunks_off, d_chunks,
                   rl.chunks_bytes, st);
    } else {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_res.p, meta + p.off_res, rl.res_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->h_res.p) + rl.chunks_off, d_chunks, rl.chunks_bytes,
                                   hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_done, st));
    return PF_OK;
}

// Upload metadata tables (results zeroed, arena counter zeroed).
int upload_meta(pf_ctx* ctx) {
    const BatchPlan& p = ctx->plan;
    uint8_t* h = static_cast<uint8_t*>(ctx->h_meta.p);
    auto put = [&](size_t off, const auto& v) { if (!v.empty()) std::memcpy(h + off, v.data(), sizeof(v[0]) * v.size()); };
    std::memset(h, 0, p.meta_bytes);
    put(p.off_chunks, p.chunks);
    put(p.off_pages, p.pages);
    put(p.off_jobs, p.jobs);
    put(p.off_zjobs, p.zjobs);
    put(p.off_ljobs, p.ljobs);
    put(p.off_pieces, p.snap.pieces);
    std::memset(h + p.off_splits, 0xff, sizeof(uint32_t) * p.snap.n_splits);
    put(p.off_wins, p.snap.wins);
    put(p.off_bajobs, p.bajobs);
    put(p.off_batiles, p.ba_tiles);
    if (!p.keeps.empty()) {
        put(p.off_keeps, p.dkeeps);
        put(p.off_keepof, p.keep_of);
    }
    for (int l = 0; l < N_LISTS; l++) put(p.off_lists + sizeof(int) * p.list_base[l], p.lists[l]);
    {   // diagnostics: force_serial = k sends every k-th Snappy job to the serial kernel (tests of
        // k_snappy_serial's grid-stride over many jobs; valid streams never fall back)
        const int k = ctx->opts.force_serial;
        int* fbh = reinterpret_cast<int*>(h + p.off_fallback);
        if (k > 0)
            for (size_t j = 0; j < p.jobs.size(); j++)
                if (int(j % size_t(k)) == k - 1) fbh[j] = FB_SERIAL;
        // force_redo = k: the block-parallel executor rejects every k-th job (after k_snappy_head), so
        // direct pages are also decoded through the redo path (tests)
        const int kr = ctx->opts.force_redo;
        SnappyJob* jh = reinterpret_cast<SnappyJob*>(h + p.off_jobs);
        if (kr > 0)
            for (size_t j = 0; j < p.jobs.size(); j++)
                if (int(j % size_t(kr)) == kr - 1) jh[j].dflags |= 1u;
    }
    DevChunkResult* r = reinterpret_cast<DevChunkResult*>(h + p.off_res);
    for (int c = 0; c < p.n_chunks; c++) {
        r[c].status = int32_t(p.host_status[c]);
        r[c].err_page = -1;
        const DevChunk& ck = p.chunks[c];
        if (!ck.needs_count) {   // flat fixed width: slots = rows = entries (host-known)
            r[c].num_slots = ck.num_entries;
            r[c].num_rows = ck.num_entries;
        }
    }
    // k_upload counts in 32 bits: an arena of 4 GiB or more takes the copy path (its zero fills below)
    const bool small = p.meta_bytes / 8 < (1ull << 31) && p.bits_bytes < (1ull << 31) && p.npub_bytes < (1ull << 31);
    ctx->meta_by_kernel = ctx->zc && ctx->h_meta.d && small;
    if (ctx->meta_by_kernel) {   // enqueue_kernels follows at once on the same stream
        const uint32_t n = uint32_t(p.meta_bytes / 8), nz0 = uint32_t(p.bits_bytes), nz1 = uint32_t(p.npub_bytes);
        const uint32_t grid = std::max(1u, std::min(1024u, (n + (nz0 + 7u) / 8u + (nz1 + 7u) / 8u + 255u) / 256u));
        hipLaunchKernelGGL(k_upload, dim3(grid), dim3(256), 0, ctx->stream, static_cast<uint64_t*>(ctx->d_meta.p),
                           static_cast<const uint64_t*>(ctx->h_meta.d), n, static_cast<uint8_t*>(ctx->d_bits.p), nz0,
                           static_cast<uint8_t*>(ctx->d_scratch.p) + p.off_npub, nz1);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_meta.p, h, p.meta_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return PF_OK;
}

// Start the copy of the batch's host bytes into d_in.
int input_to_device(pf_ctx* ctx, const uint8_t* bytes, size_t n_bytes) {
    HIPCHK(ctx, ctx->d_in.ensure(n_bytes));
    // pinned pages with a 16-byte aligned device address: read by a kernel (k_download's loop), so the
    // link runs both ways at once beside the downloads (an SDMA H2D waited behind them, r06 trace)
    void* hd = nullptr;
    if (ctx->opts.h2d_kernel && hipHostGetDevicePointer(&hd, const_cast<uint8_t*>(bytes), 0) == hipSuccess && hd &&
        (reinterpret_cast<uintptr_t>(hd) & 15u) == 0) {
        const DlRange r0{static_cast<uint8_t*>(ctx->d_in.p), static_cast<const uint8_t*>(hd), uint64_t(n_bytes)};
        const DlRange rz{nullptr, nullptr, 0};
        hipLaunchKernelGGL(k_download, dim3(ctx->opts.h2d_grid), dim3(256), 0, ctx->stream, r0, rz, rz);
        HIPCHK(ctx, hipGetLastError());
    } else {
        (void)hipGetLastError();
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_in.p, bytes, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return PF_OK;
}

}  // namespace


// The write path (pf_encode_chunk, pf_snappy_compress, pf_zstd_compress) is pf_enc_runtime.hip, planned by pf_enc_plan.cpp.

extern "C" {

int pf_abi_version(void) { return PF_ABI_VERSION; }

const char* pf_last_error(pf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int pf_device_count(int* count) {
    if (!count) return fail(nullptr, PF_ERR_INVALID_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, PF_ERR_HIP, hipGetErrorString(e)); }
    *count = n;
    return PF_OK;
}

namespace {
#ifdef PF_DIAG
// Diagnostics build only: the options from the environment (PfOpts, pf_internal.h).
void opts_from_env(pf::PfOpts& o) {
    auto on = [](const char* name, bool dflt) { const char* e = std::getenv(name); return e ? e[0] == '1' : dflt; };
    auto num = [](const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    o.exec = num("PF_EXEC", o.exec);
    o.ba_fused = on("PF_BA_FUSED", o.ba_fused);
    o.page_null = on("PF_PAGE_NULL", o.page_null);
    o.nest_timeout = on("PF_DEBUG_NEST_TIMEOUT", o.nest_timeout);
    o.null_dcap = uint32_t(std::max(0, num("PF_NULL_DCAP", 0))) & ~15u;
    o.null_stagger = num("PF_DEBUG_NULL_STAGGER", o.null_stagger);
    if (const char* e = std::getenv("PF_DEBUG_SKIP")) {
        const char* names[] = {"parse", "exec", "ba", "levels", "count", "flat", "decode"};
        for (int i = 0; i < 7; i++)
            if (std::strstr(e, names[i])) o.debug_skip |= 1u << i;
    }
    o.force_serial = num("PF_DEBUG_FORCE_SERIAL", o.force_serial);
    o.force_redo = num("PF_DEBUG_FORCE_REDO", o.force_redo);
    o.zc = on("PF_ZC", o.zc);
    o.dl_kernel = on("PF_DL_KERNEL", o.dl_kernel);
    o.dl_stream = on("PF_DL_STREAM", o.dl_stream);
    o.h2d_kernel = on("PF_H2D_KERNEL", o.h2d_kernel);
    o.h2d_grid = std::max(1, num("PF_H2D_GRID", o.h2d_grid));
    o.dl_prio = on("PF_DL_PRIO", o.dl_prio);
    o.debug_plan = on("PF_DEBUG_PLAN", o.debug_plan);
    if (const char* e = std::getenv("PF_NEST_SEG")) {
        o.nest_seg = std::atoll(e);
        o.nest_seg_set = true;
    }
    o.dbp_par = on("PF_DBP_PAR", o.dbp_par);
    o.bloom_first = on("PF_BLOOM_FIRST", o.bloom_first);
    o.flat_dstr = on("PF_FLAT_DSTR", o.flat_dstr);
    const int fb = num("PF_FIX_BLK", 8192);
    o.fix_shift = fb >= 16384 ? 2 : (fb >= 8192 ? 1 : 0);
}
#endif

int ctx_init(pf_ctx* ctx, pf_ctx* peer) {
#ifdef PF_DIAG
    opts_from_env(ctx->opts);
#endif
    HIPCHK(nullptr, hipSetDevice(ctx->device));
    if (peer) {
        ctx->streams = peer->streams;
    } else {
        ctx->streams = std::make_shared<Streams>();
        ctx->streams->device = ctx->device;
        HIPCHK(nullptr, hipStreamCreateWithFlags(&ctx->streams->stream, hipStreamNonBlocking));
    }
    ctx->stream = ctx->streams->stream;
    ctx->zc = ctx->opts.zc;
    HIPCHK(nullptr, hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming));
    HIPCHK(nullptr, hipEventCreateWithFlags(&ctx->ev_copy, hipEventDisableTiming));
    HIPCHK(nullptr, hipEventCreateWithFlags(&ctx->ev_dl, hipEventDisableTiming));
    for (auto& e : ctx->ev) HIPCHK(nullptr, hipEventCreate(&e));
    for (auto& e : ctx->ev_bloom) HIPCHK(nullptr, hipEventCreate(&e));
    for (auto& e : ctx->ev_win) HIPCHK(nullptr, hipEventCreate(&e));
    for (auto& e : ctx->ev_sel) HIPCHK(nullptr, hipEventCreate(&e));
    return PF_OK;
}

int ctx_create(int device, pf_ctx* peer, pf_ctx** out) {
    pf_ctx* ctx = new pf_ctx();
    ctx->device = device;
    const int rc = ctx_init(ctx, peer);
    if (rc != PF_OK) {   // release whatever streams / events were created before the failure
        const std::string msg = g_err;
        pf_ctx_destroy(ctx);
        g_err = msg;
        return rc;
    }
    *out = ctx;
    return PF_OK;
}
}  // namespace

int pf_ctx_create(int device, pf_ctx** out) {
    if (!out) return fail(nullptr, PF_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(nullptr, PF_ERR_INVALID_ARG, "no such HIP device");
    return ctx_create(device, nullptr, out);
}

int pf_ctx_create_shared(pf_ctx* peer, pf_ctx** out) {
    if (!out || !peer) return fail(nullptr, PF_ERR_INVALID_ARG, "null arg");
    *out = nullptr;
    return ctx_create(peer->device, peer, out);
}

int pf_ctx_set_timing(pf_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, PF_ERR_INVALID_ARG, "null ctx");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "decode in flight");
    ctx->timing = on != 0;
    ctx->timing_valid = false;
    return PF_OK;
}

int pf_ctx_destroy(pf_ctx* ctx) {
    if (!ctx) return PF_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);   // this context's work and any peer's ahead of it
    if (ctx->copies_pending) (void)hipEventSynchronize(ctx->ev_copy);   // (a download on the copy stream)
    for (DevBuf* b : {&ctx->d_in, &ctx->d_scratch, &ctx->d_out, &ctx->d_bits, &ctx->d_chars, &ctx->d_meta, &ctx->d_tokmap,
                      &ctx->d_scan_in, &ctx->d_scan, &ctx->d_enc, &ctx->d_enc_sec, &ctx->d_enc_out, &ctx->d_win, &ctx->d_wout,
                      &ctx->d_wbits, &ctx->d_wchars, &ctx->d_sel})
        b->release();
    ctx->h_win.release();
    ctx->h_sel.release();
    ctx->h_meta.release();
    ctx->h_res.release();
    ctx->h_enc_slots.release();
    ctx->h_enc_st.release();
    ctx->h_enc_px.release();
    ctx->h_enc_bloom.release();
    ctx->h_keep.release();
    for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_bloom) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_win) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev_sel) if (e) (void)hipEventDestroy(e);
    if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
    if (ctx->ev_copy) (void)hipEventDestroy(ctx->ev_copy);
    if (ctx->ev_dl) (void)hipEventDestroy(ctx->ev_dl);
    ctx->streams.reset();   // destroys the streams when no other context shares them
    delete ctx;
    return PF_OK;
}

int pf_host_alloc(pf_ctx* ctx, size_t bytes, void** out) {
    if (!out) return fail(ctx, PF_ERR_INVALID_ARG, "null out");
    if (ctx) (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault));
    return PF_OK;
}

int pf_host_free(pf_ctx* ctx, void* ptr) {
    if (ptr) HIPCHK(ctx, hipHostFree(ptr));
    return PF_OK;
}

int pf_device_alloc(pf_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(out, bytes + 256));   // slack: 16-byte staging loads may read past the end
    return PF_OK;
}

int pf_device_free(pf_ctx* ctx, void* ptr) {
    if (ptr) HIPCHK(ctx, hipFree(ptr));
    return PF_OK;
}

int pf_memcpy_h2d(pf_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return fail(ctx, PF_ERR_INVALID_ARG, "null ctx");
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PF_OK;
}

}  // extern "C"

namespace {
// The filter stage's buffer for the planned batch (laid out by layout_filter), its tables uploaded.
int bind_filter(pf_ctx* ctx) {
    const SelLayout& l = ctx->sel_lay = layout_filter(ctx->plan, ctx->filt, ctx->wins);
    HIPCHK(ctx, ctx->d_sel.ensure(l.total));
    HIPCHK(ctx, ctx->h_sel.ensure(l.up_end));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_sel.p);
    fill_filter(l, ctx->filt, h);
    HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->d_sel.p) + l.o_up, h + l.o_up, l.up_end - l.o_up, hipMemcpyHostToDevice,
                               ctx->stream));
    ctx->sel = bind_sel(l, ctx->filt, reinterpret_cast<uintptr_t>(ctx->d_sel.p));
    ctx->sel_dict = SelDictBufs{};   // (its metadata pointers: enqueue_batch, once d_meta is sized)
    return PF_OK;
}

// Plan, upload and enqueue one batch; ctx->wins lists the chunks to be windowed.
int enqueue_batch(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const uint8_t* bytes, size_t n_bytes,
                  int bytes_on_device) {
    const bool windowed = !ctx->wins.empty(), twins = ctx->twins();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // diagnostics: PF_DEBUG_PLAN=1 prints the host time of each phase (microseconds)
    const bool dbg_plan = ctx->opts.debug_plan;
    using clk = std::chrono::steady_clock;
    clk::time_point tp[7];
    int ntp = 0;
    auto mark = [&]() { if (dbg_plan) tp[ntp++] = clk::now(); };
    mark();
    BatchPlan& p = ctx->plan;
    ctx->n_chunks = n_chunks;
    ctx->info.assign(n_chunks, pf_column_info{});
    ctx->dinfo.assign(n_chunks, pf_dict_info{});
    ctx->reruns = 0;
    ctx->timing_valid = false;
    // stage "h2d" (ev[0] -> ev[1]): the input copy when there is one, the metadata upload and the
    // memsets; for device-resident input it starts at the metadata upload (not before the host plan)
    const bool input_h2d = !bytes_on_device && n_bytes;
    const uint8_t* d_bytes = bytes;
    if (input_h2d) {
        EVREC(ctx, ctx->ev[0], st);
        const int rc = input_to_device(ctx, bytes, n_bytes);
        if (rc) return rc;
        d_bytes = static_cast<const uint8_t*>(ctx->d_in.p);
    }
    mark();
    plan_batch(cds, n_chunks, n_bytes, ctx->opts, p, ctx->keep_flags.empty() ? nullptr : ctx->keep_flags.data());
    mark();
    // ---- arenas ----
    const ArenaNeeds need = arena_needs(p, ctx->chars_need, twins);
    if (ctx->copies_pending) {
        if (arenas_grow(need, ArenaCaps{ctx->d_out.cap, ctx->d_bits.cap, ctx->d_chars.cap, ctx->d_wout.cap, ctx->d_wbits.cap,
                                        ctx->d_wchars.cap}, twins))
            HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));   // a growing output arena must not be freed under a pending D2H copy
        else
            HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_copy, 0));   // (a download on the copy stream reads the arenas)
    }
    ctx->copies_pending = false;
    HIPCHK(ctx, ctx->d_scratch.ensure(std::max<size_t>(p.scratch_bytes, 1)));
    HIPCHK(ctx, ctx->d_out.ensure(std::max<size_t>(need.out, 1)));
    HIPCHK(ctx, ctx->d_bits.ensure(need.bits));
    HIPCHK(ctx, ctx->d_chars.ensure(need.chars));
    ctx->twin = TwinDelta{};
    if (twins) {   // the twins: the decode arenas' sizes, so a chunk keeps its offsets
        HIPCHK(ctx, ctx->d_wout.ensure(ctx->d_out.cap));
        HIPCHK(ctx, ctx->d_wbits.ensure(ctx->d_bits.cap));
        HIPCHK(ctx, ctx->d_wchars.ensure(ctx->d_chars.cap));
        ctx->twin.out = static_cast<uint8_t*>(ctx->d_wout.p) - static_cast<uint8_t*>(ctx->d_out.p);
        ctx->twin.bits = static_cast<uint8_t*>(ctx->d_wbits.p) - static_cast<uint8_t*>(ctx->d_bits.p);
    }
    if (windowed) {
        const WinLayout& wl = ctx->win_lay = win_layout(int(ctx->wins.size()));
        HIPCHK(ctx, ctx->d_win.ensure(wl.total));
        HIPCHK(ctx, ctx->h_win.ensure(wl.total));
        std::memcpy(ctx->h_win.p, ctx->wins.data(), wl.wins_bytes);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_win.p, ctx->h_win.p, wl.wins_bytes, hipMemcpyHostToDevice, st));
        ctx->win_grid = win_grid(p, ctx->wins);
    }
    if (ctx->filtered()) {
        plan_filter_dict(p, ctx->filt);   // which predicates are on chunks the plan keeps
        const int rc = bind_filter(ctx);
        if (rc) return rc;
    }
    HIPCHK(ctx, ctx->d_tokmap.ensure(p.snap.tokmap_bytes));
    HIPCHK(ctx, ctx->d_meta.ensure(p.meta_bytes));
    if (ctx->filtered() && !p.keeps.empty()) {
        const uint8_t* meta = static_cast<const uint8_t*>(ctx->d_meta.p);
        ctx->sel_dict = bind_sel_dict(ctx->sel_lay, ctx->filt, reinterpret_cast<uintptr_t>(ctx->d_sel.p),
                                      reinterpret_cast<const DevKeep*>(meta + p.off_keeps),
                                      reinterpret_cast<const int32_t*>(meta + p.off_keepof));
    }
    HIPCHK(ctx, ctx->h_meta.ensure(p.meta_bytes));
    ctx->res_lay = res_layout(n_chunks);
    HIPCHK(ctx, ctx->h_res.ensure(ctx->res_lay.total));
    if (!p.keeps.empty()) HIPCHK(ctx, ctx->h_keep.ensure(sizeof(DevKeep) * p.keeps.size()));
    mark();
    auto addr = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
    bind_batch(p, ArenaBases{addr(d_bytes), addr(ctx->d_scratch.p), addr(ctx->d_out.p), addr(ctx->d_bits.p), addr(ctx->d_meta.p),
                             addr(ctx->d_tokmap.p)});
    mark();
    if (!input_h2d) EVREC(ctx, ctx->ev[0], st);
    int rc = upload_meta(ctx);
    if (rc) return rc;
    mark();
    rc = enqueue_kernels(ctx);
    if (rc) return rc;
    mark();
    if (dbg_plan) {
        auto us = [&](int a, int b) { return long(std::chrono::duration_cast<std::chrono::microseconds>(tp[b] - tp[a]).count()); };
        std::fprintf(stderr, "[pf plan] chunks %d pages %zu jobs %zu wins %zu | h2d %ld plan %ld arenas %ld bind %ld upload %ld launch %ld us\n",
                     n_chunks, p.pages.size(), p.jobs.size(), p.snap.wins.size(), us(0, 1), us(1, 2), us(2, 3), us(3, 4),
                     us(4, 5), us(5, 6));
    }
    ctx->pending = true;
    ctx->tables_from_decode = true;
    return PF_OK;
}

// pf_decode_row_group (windows == nullptr), pf_decode_row_group_rows and pf_decode_row_group_filter (n_preds > 0).
int decode_batch(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const pf_row_window* windows, const pf_predicate* preds,
                 int n_preds, const uint8_t* bytes, size_t n_bytes, int bytes_on_device, const uint8_t* keep = nullptr) {
    if (!ctx) return fail(nullptr, PF_ERR_INVALID_ARG, "null ctx");
    if (n_chunks < 0 || (n_chunks > 0 && (!cds || !bytes))) return fail(ctx, PF_ERR_INVALID_ARG, "bad arguments");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    ctx->keep_flags.clear();
    if (keep && n_chunks > 0) ctx->keep_flags.assign(keep, keep + n_chunks);   // (copied, like the descriptors)
    for (int c = 0; windows && c < n_chunks; c++)
        if (windows[c].skip_rows < 0 || windows[c].take_rows < -1)
            return fail(ctx, PF_ERR_INVALID_ARG, "row window: negative skip_rows, or take_rows below -1");
    ctx->wins.clear();
    ctx->filt.preds.clear();
    ctx->filt.blob.clear();
    ctx->filt.dicts.clear();
    ctx->filt.dict_of.clear();
    if (n_preds != 0) {   // (a predicate error leaves the lists cleared, like an enqueue error below)
        const char* why = "";
        const int rc = plan_filter(cds, n_chunks, preds, n_preds, ctx->filt, &why);
        if (rc) return fail(ctx, rc, why);
    }
    for (int c = 0; windows && c < n_chunks; c++)
        if (windows[c].skip_rows != 0 || windows[c].take_rows != -1)
            ctx->wins.push_back(DevWin{c, 0, windows[c].skip_rows, windows[c].take_rows});
    const int rc = enqueue_batch(ctx, cds, n_chunks, bytes, n_bytes, bytes_on_device);
    if (rc) {   // nothing windowed or filtered is pending: the batch-copy gates must not answer for this call
        ctx->wins.clear();
        ctx->filt.preds.clear();
        ctx->filt.blob.clear();
    }
    return rc;
}
}  // namespace

extern "C" {

int pf_decode_row_group(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const uint8_t* bytes, size_t n_bytes,
                        int bytes_on_device) {
    return decode_batch(ctx, cds, n_chunks, nullptr, nullptr, 0, bytes, n_bytes, bytes_on_device);
}

int pf_decode_row_group_dict(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const uint8_t* keep, const uint8_t* bytes,
                             size_t n_bytes, int bytes_on_device) {
    return decode_batch(ctx, cds, n_chunks, nullptr, nullptr, 0, bytes, n_bytes, bytes_on_device, keep);
}

int pf_decode_row_group_dict_filter(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const uint8_t* keep,
                                    const pf_row_window* windows, const pf_predicate* preds, int n_preds, const uint8_t* bytes,
                                    size_t n_bytes, int bytes_on_device) {
    return decode_batch(ctx, cds, n_chunks, windows, preds, n_preds, bytes, n_bytes, bytes_on_device, keep);
}

int pf_decode_row_group_rows(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const pf_row_window* windows,
                             const uint8_t* bytes, size_t n_bytes, int bytes_on_device) {
    return decode_batch(ctx, cds, n_chunks, windows, nullptr, 0, bytes, n_bytes, bytes_on_device);
}

int pf_decode_row_group_filter(pf_ctx* ctx, const pf_chunk_desc* cds, int n_chunks, const pf_row_window* windows,
                               const pf_predicate* preds, int n_preds, const uint8_t* bytes, size_t n_bytes, int bytes_on_device) {
    return decode_batch(ctx, cds, n_chunks, windows, preds, n_preds, bytes, n_bytes, bytes_on_device);
}

int pf_selection_info_get(pf_ctx* ctx, pf_selection_info* out) {
    if (!ctx || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode || !ctx->filtered()) return fail(ctx, PF_ERR_STATE, "the last decode had no row filter");
    *out = ctx->sel_info;
    return PF_OK;
}

int pf_copy_selection(pf_ctx* ctx, int32_t* rows, size_t cap_bytes) {
    if (!ctx || (!rows && cap_bytes)) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode || !ctx->filtered()) return fail(ctx, PF_ERR_STATE, "the last decode had no row filter");
    const size_t n = 4 * size_t(ctx->sel_info.rows_selected);
    if (n > cap_bytes) return fail(ctx, PF_ERR_CAPACITY, "selection buffer too small");
    if (!n) return PF_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(rows, ctx->sel_info.d_rows, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    return PF_OK;
}

// Diagnostics (not part of pfloor.h): the filter stage of the last finished decode. *ms: time of its kernels (HIP events;
// 0 when the decode had no predicates or stage timing is off; not a stage of pf_last_timing).
int pf_debug_filter(pf_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    *ms = 0;
    if (!ctx->timing_valid || !ctx->timing || !ctx->filtered()) return PF_OK;
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev_sel[0], ctx->ev_sel[1]));
    return PF_OK;
}

// Diagnostics (not part of pfloor.h): the window stage of the last finished decode. *ms: time of its kernels (HIP
// events; 0 when the decode had no window or stage timing is off; not a stage of pf_last_timing, whose stages are
// the same with and without windows). *reruns: how often pf_wait ran the batch again for a chars overflow (0 or 1).
int pf_debug_window(pf_ctx* ctx, float* ms, int* reruns) {
    if (!ctx || !ms || !reruns) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    *ms = 0;
    *reruns = ctx->reruns;
    if (!ctx->timing_valid || !ctx->timing || ctx->wins.empty()) return PF_OK;
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev_win[0], ctx->ev_win[1]));
    return PF_OK;
}

int pf_wait(pf_ctx* ctx) {
    if (!ctx) return fail(nullptr, PF_ERR_INVALID_ARG, "null ctx");
    if (!ctx->pending) return fail(ctx, PF_ERR_STATE, "nothing to wait for");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (;;) {
        hipError_t e = hipEventSynchronize(ctx->ev_done);
        if (e != hipSuccess) { ctx->pending = false; return fail(ctx, PF_ERR_HIP, std::string("decode: ") + hipGetErrorString(e)); }
        const uint8_t* hres = static_cast<const uint8_t*>(ctx->h_res.p);
        const DevChunkResult* r = reinterpret_cast<const DevChunkResult*>(hres);
        // chars arena overflow: grow to the exact need and run the batch once more
        const CharsOverflow ov = chars_overflow(ctx->plan, r);
        if (ov.rerun && ctx->reruns == 0) {
            ctx->reruns++;
            ctx->chars_need = size_t(ov.need) + (1u << 20);
            HIPCHK(ctx, ctx->d_chars.ensure(ctx->chars_need));
            if (ctx->twins()) HIPCHK(ctx, ctx->d_wchars.ensure(ctx->d_chars.cap));
            int rc = upload_meta(ctx);
            if (rc) { ctx->pending = false; return rc; }
            rc = enqueue_kernels(ctx);
            if (rc) { ctx->pending = false; return rc; }
            continue;
        }
        const uint8_t* hwin = static_cast<const uint8_t*>(ctx->h_win.p);
        const uint8_t* hsel = static_cast<const uint8_t*>(ctx->h_sel.p);
        const bool filtered = ctx->filtered();
        BatchResults br{};
        br.res = r;
        br.dev_chunks = reinterpret_cast<const DevChunk*>(hres + ctx->res_lay.chunks_off);
        br.wins = ctx->wins.data();
        br.n_wins = ctx->wins.size();
        br.wres = br.n_wins ? reinterpret_cast<const DevWinRes*>(hwin + ctx->win_lay.res_off) : nullptr;
        br.twin = ctx->twin;
        br.sel_head = filtered ? reinterpret_cast<const DevSelHead*>(hsel + ctx->sel_lay.o_head) : nullptr;
        br.sel_chunks = filtered ? reinterpret_cast<const DevSelChunk*>(hsel + ctx->sel_lay.o_sc) : nullptr;
        br.sel_rows = ctx->sel.rows;
        br.keeps = ctx->plan.keeps.empty() ? nullptr : static_cast<const DevKeep*>(ctx->h_keep.p);
        const FirstError fe = assemble_info(ctx->plan, br, ctx->info.data(), &ctx->sel_info, ctx->dinfo.data());
        if (fe.code != PF_OK) fail(ctx, fe.code, fe.msg);
        ctx->pending = false;
        ctx->timing_valid = true;
        return fe.code;
    }
}

int pf_column_info_get(pf_ctx* ctx, int chunk, pf_column_info* out) {
    if (!ctx || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    *out = ctx->info[chunk];
    return PF_OK;
}

namespace {
// Chunk i's arrays against the caller's buffers: the call's checks, capacities last (nothing is enqueued).
int check_copy(pf_ctx* ctx, int chunk, const pf_column_out* o, CopyItem items[8]) {
    if (!ctx || !o) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    const pf_column_info& ci = ctx->info[chunk];
    if (ci.status != 0) return fail(ctx, ci.status, "chunk failed to decode");
    copy_items(ci, *o, items);
    for (int k = 0; k < 8; k++)
        if (items[k].wanted() && items[k].n > items[k].cap) return fail(ctx, PF_ERR_CAPACITY, "output buffer too small");
    return PF_OK;
}
// Enqueue the D2H copies of chunk i's arrays on the context stream (no synchronisation).
int enqueue_copy(pf_ctx* ctx, int chunk, const pf_column_out* o) {
    CopyItem items[8];
    const int rc = check_copy(ctx, chunk, o, items);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (const CopyItem& it : items)
        if (it.wanted() && it.n) HIPCHK(ctx, hipMemcpyAsync(it.dst, it.src, it.n, hipMemcpyDeviceToHost, ctx->stream));
    return PF_OK;
}
}  // namespace

int pf_copy_column(pf_ctx* ctx, int chunk, const pf_column_out* o) {
    const int rc = enqueue_copy(ctx, chunk, o);
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    return PF_OK;
}

int pf_copy_columns_async(pf_ctx* ctx, int n, const int* chunks, const pf_column_out* outs) {
    if (!ctx || n < 0 || (n > 0 && (!chunks || !outs))) return fail(ctx, PF_ERR_INVALID_ARG, "bad arguments");
    for (int i = 0; i < n; i++) {   // capacities first: nothing is enqueued if any buffer is too small
        CopyItem items[8];
        const int rc = check_copy(ctx, chunks[i], &outs[i], items);
        if (rc) return rc;
    }
    for (int i = 0; i < n; i++) {
        const int rc = enqueue_copy(ctx, chunks[i], &outs[i]);
        if (rc) return rc;
    }
    if (n > 0) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
        ctx->copies_pending = true;
    }
    return PF_OK;
}

namespace {
// Host layout of pf_copy_batch_async for the last decode (pf_result.h).
BatchLayout last_layout(const pf_ctx* ctx) { return batch_layout(ctx->plan, ctx->info, ctx->d_chars.p, &ctx->dinfo); }
}  // namespace

int pf_batch_bytes(pf_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    *bytes = last_layout(ctx).total;
    return PF_OK;
}

int pf_copy_batch_async(pf_ctx* ctx, void* host, size_t cap) {
    if (!ctx || (!host && cap)) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    const BatchLayout b = last_layout(ctx);
    if (b.total > cap) return fail(ctx, PF_ERR_CAPACITY, "batch buffer too small (pf_batch_bytes)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint8_t* h = static_cast<uint8_t*>(host);
    // pinned pages with a device address: k_download; otherwise (or PF_DL_KERNEL=0) SDMA copies
    void* hd = nullptr;
    if (ctx->opts.dl_kernel && (b.out || b.bits || b.chars)) {
        if (hipHostGetDevicePointer(&hd, host, 0) != hipSuccess || !hd || (reinterpret_cast<uintptr_t>(hd) & 15u) != 0) {
            (void)hipGetLastError();   // (not a mapped pinned buffer: the copy path)
            hd = nullptr;
        }
    }
    hipStream_t cs = ctx->stream;
    if (ctx->opts.dl_stream) {   // the download on the copy stream, after this context's decode
        {
            std::lock_guard<std::mutex> lk(ctx->streams->mu);
            if (!ctx->streams->copy_stream) {
                int least = 0, greatest = 0;
                if (ctx->opts.dl_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
                    HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->streams->copy_stream, hipStreamNonBlocking, greatest));
                else
                    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->streams->copy_stream, hipStreamNonBlocking));
            }
        }
        cs = ctx->streams->copy_stream;
        HIPCHK(ctx, hipEventRecord(ctx->ev_dl, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(cs, ctx->ev_dl, 0));
    }
    if (hd) {
        uint8_t* hdev = static_cast<uint8_t*>(hd);
        const DlRange r0{hdev, static_cast<const uint8_t*>(ctx->d_out.p), b.out};
        const DlRange r1{hdev + b.bits_off, static_cast<const uint8_t*>(ctx->d_bits.p), b.bits};
        const DlRange r2{hdev + b.chars_off, static_cast<const uint8_t*>(ctx->d_chars.p), b.chars};
        hipLaunchKernelGGL(k_download, dim3(256), dim3(256), 0, cs, r0, r1, r2);
        HIPCHK(ctx, hipGetLastError());
    } else {
        if (b.out) HIPCHK(ctx, hipMemcpyAsync(h, ctx->d_out.p, b.out, hipMemcpyDeviceToHost, cs));
        if (b.bits) HIPCHK(ctx, hipMemcpyAsync(h + b.bits_off, ctx->d_bits.p, b.bits, hipMemcpyDeviceToHost, cs));
        if (b.chars) HIPCHK(ctx, hipMemcpyAsync(h + b.chars_off, ctx->d_chars.p, b.chars, hipMemcpyDeviceToHost, cs));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_copy, cs));
    ctx->copies_pending = true;
    return PF_OK;
}

int pf_column_info_host(pf_ctx* ctx, int chunk, const void* host, pf_column_info* out) {
    if (!ctx || !out || !host) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    *out = rebase_info(last_layout(ctx), ArenaPtrs{ctx->d_out.p, ctx->d_bits.p, ctx->d_chars.p}, host, ctx->info[chunk]);
    return PF_OK;
}

int pf_dict_info_get(pf_ctx* ctx, int chunk, pf_dict_info* out) {
    if (!ctx || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    *out = ctx->dinfo[chunk];
    return PF_OK;
}

int pf_dict_info_host(pf_ctx* ctx, int chunk, const void* host, pf_dict_info* out) {
    if (!ctx || !out || !host) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    *out = rebase_dict(last_layout(ctx), ArenaPtrs{ctx->d_out.p, ctx->d_bits.p, ctx->d_chars.p}, host, ctx->dinfo[chunk]);
    return PF_OK;
}

int pf_copy_dictionary(pf_ctx* ctx, int chunk, const pf_column_out* o) {
    if (!ctx || !o) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    const pf_dict_info& di = ctx->dinfo[chunk];
    if (!di.kept) return fail(ctx, PF_ERR_STATE, "the chunk's dictionary was not kept");
    if (ctx->info[chunk].status != 0) return fail(ctx, ctx->info[chunk].status, "chunk failed to decode");
    CopyItem items[3];
    dict_copy_items(di, *o, items);
    for (const CopyItem& it : items)
        if (it.wanted() && it.n > it.cap) return fail(ctx, PF_ERR_CAPACITY, "dictionary buffer too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (const CopyItem& it : items)
        if (it.wanted() && it.n) HIPCHK(ctx, hipMemcpyAsync(it.dst, it.src, it.n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    return PF_OK;
}

int pf_sync(pf_ctx* ctx) {
    if (!ctx) return fail(nullptr, PF_ERR_INVALID_ARG, "null ctx");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));   // this context's copies only
    ctx->copies_pending = false;
    return PF_OK;
}

namespace {
// The head of a one-shot call (Snappy, ZSTD, LZ4, page scan): the arenas may be reallocated below, so this context's pending
// copies out of them finish first. drop_batch: d_meta will hold this call's layout, the last decode's tables are gone.
int begin_oneshot(pf_ctx* ctx, bool drop_batch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
    if (drop_batch) {
        ctx->n_chunks = 0;
        ctx->info.clear();
        ctx->dinfo.clear();
        ctx->tables_from_decode = false;
    }
    return PF_OK;
}
}  // namespace

int pf_snappy_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    if (!ctx || (!src && n) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    uint64_t ulen = 0;
    size_t p = 0;
    for (int sh = 0;; sh += 7) {
        if (p >= n || sh > 28) return fail(ctx, PF_ERR_CORRUPT_PAGE, "snappy: bad length preamble");
        uint8_t c = src[p++];
        ulen |= uint64_t(c & 0x7f) << sh;
        if (!(c & 0x80)) break;
    }
    *out_len = size_t(ulen);
    if (ulen > cap) return fail(ctx, PF_ERR_CAPACITY, "snappy: destination too small");
    if (n > 0xffffffffull || ulen > 0xffffffffull) return fail(ctx, PF_ERR_INVALID_ARG, "snappy: buffer too large");
    if (const int rc = begin_oneshot(ctx, true)) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, ctx->d_in.ensure(std::max<size_t>(n, 1)));
    HIPCHK(ctx, ctx->d_scratch.ensure(std::max<size_t>(ulen, 1) + 16));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_in.p, src, n, hipMemcpyHostToDevice, st));
    SnappyJob job{};
    job.src = static_cast<const uint8_t*>(ctx->d_in.p);
    job.dst = static_cast<uint8_t*>(ctx->d_scratch.p);
    job.src_len = uint32_t(n);
    job.dst_len = uint32_t(ulen);
    std::vector<SnappyJob> jobs(1, job);
    SnappyPlan sp;
    plan_snappy(jobs, sp);
    HIPCHK(ctx, ctx->d_tokmap.ensure(sp.tokmap_bytes));
    bind_snappy(jobs, sp, reinterpret_cast<uintptr_t>(ctx->d_tokmap.p));
    ctx->d_last_win = sp.d_win;
    ctx->d_last_lane_out = sp.d_lane_out;
    size_t m = 0;
    auto take = [](size_t& cursor, size_t sz) { size_t o = align_up(cursor, 256); cursor = o + sz; return o; };
    size_t o_job = take(m, sizeof(SnappyJob)), o_pc = take(m, sizeof(int2) * sp.pieces.size());
    size_t o_sp = take(m, 4 * sp.pieces.size()), o_fb = take(m, 4), o_wn = take(m, sizeof(int2) * sp.wins.size());
    size_t o_res = take(m, sizeof(DevChunkResult));
    m = align_up(m, 256);
    HIPCHK(ctx, ctx->d_meta.ensure(m));
    HIPCHK(ctx, ctx->h_meta.ensure(m));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_meta.p);
    std::memset(h, 0, m);
    std::memcpy(h + o_job, jobs.data(), sizeof(SnappyJob));
    std::memcpy(h + o_pc, sp.pieces.data(), sizeof(int2) * sp.pieces.size());
    std::memset(h + o_sp, 0xff, 4 * sp.pieces.size());
    std::memcpy(h + o_wn, sp.wins.data(), sizeof(int2) * sp.wins.size());
    uint8_t* d = static_cast<uint8_t*>(ctx->d_meta.p);
    HIPCHK(ctx, hipMemcpyAsync(d, h, m, hipMemcpyHostToDevice, st));
    ctx->d_last_splits = reinterpret_cast<const uint32_t*>(d + o_sp);
    launch_snappy(reinterpret_cast<const SnappyJob*>(d + o_job), 1, reinterpret_cast<const int2*>(d + o_wn),
                  int(sp.wins.size()), sp.d_win, sp.d_ent, sp.d_lane_out, reinterpret_cast<const int2*>(d + o_pc),
                  int(sp.pieces.size()), reinterpret_cast<uint32_t*>(d + o_sp), reinterpret_cast<int*>(d + o_fb),
                  reinterpret_cast<DevChunkResult*>(d + o_res), int(jobs[0].n_win),
                  ctx->opts.exec, st);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, ctx->h_res.ensure(512));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_res.p, d + o_res, sizeof(DevChunkResult), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->h_res.p) + 256, d + o_fb, 4, hipMemcpyDeviceToHost, st));
    if (ulen) HIPCHK(ctx, hipMemcpyAsync(dst, ctx->d_scratch.p, ulen, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const DevChunkResult* r = static_cast<const DevChunkResult*>(ctx->h_res.p);
    if (r->status != 0) return fail(ctx, r->status, "snappy: corrupt input");
    return PF_OK;
}

// One buffer of ZSTD frames through k_zstd (pf_zstd.hip), as one job with room for cap bytes.
int pf_zstd_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    if (!ctx || (!src && n) || (!dst && cap) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n > (1ull << 30) || cap > (1ull << 30)) return fail(ctx, PF_ERR_INVALID_ARG, "zstd: buffer too large");
    *out_len = 0;
    if (const int rc = begin_oneshot(ctx, true)) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t stride = zstd_lit_stride(uint32_t(cap));
    const size_t o_lit = align_up(cap + 16, 256);
    HIPCHK(ctx, ctx->d_in.ensure(std::max<size_t>(n, 1)));
    HIPCHK(ctx, ctx->d_scratch.ensure(o_lit + stride));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_in.p, src, n, hipMemcpyHostToDevice, st));
    ZstdJob job{};
    job.src = static_cast<const uint8_t*>(ctx->d_in.p);
    job.dst = static_cast<uint8_t*>(ctx->d_scratch.p);
    job.src_len = uint32_t(n);
    job.dst_len = uint32_t(cap);
    const size_t o_res = 256, m = 512;
    HIPCHK(ctx, ctx->d_meta.ensure(m));
    HIPCHK(ctx, ctx->h_meta.ensure(m));
    HIPCHK(ctx, ctx->h_res.ensure(512));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_meta.p);
    std::memset(h, 0, m);
    std::memcpy(h, &job, sizeof job);
    uint8_t* d = static_cast<uint8_t*>(ctx->d_meta.p);
    HIPCHK(ctx, hipMemcpyAsync(d, h, m, hipMemcpyHostToDevice, st));
    launch_zstd(reinterpret_cast<ZstdJob*>(d), nullptr, 1, static_cast<uint8_t*>(ctx->d_scratch.p) + o_lit, stride,
                reinterpret_cast<DevChunkResult*>(d + o_res), st);
    HIPCHK(ctx, hipGetLastError());
    uint8_t* hr = static_cast<uint8_t*>(ctx->h_res.p);
    HIPCHK(ctx, hipMemcpyAsync(hr, d, m, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ZstdJob done;
    std::memcpy(&done, hr, sizeof done);
    const DevChunkResult* r = reinterpret_cast<const DevChunkResult*>(hr + o_res);
    if (r->status != 0) return fail(ctx, r->status, "zstd: corrupt input");
    if (done.produced) HIPCHK(ctx, hipMemcpy(dst, ctx->d_scratch.p, done.produced, hipMemcpyDeviceToHost));
    *out_len = done.produced;
    return PF_OK;
}

// One raw LZ4 block through k_lz4 (pf_lz4.hip), as one job that has to produce exactly size bytes.
int pf_lz4_decompress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t size, size_t* out_len) {
    if (!ctx || (!src && n) || (!dst && size) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n > (1ull << 30) || size > (1ull << 30)) return fail(ctx, PF_ERR_INVALID_ARG, "lz4: buffer too large");
    *out_len = 0;
    if (const int rc = begin_oneshot(ctx, true)) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, ctx->d_in.ensure(std::max<size_t>(n, 1)));
    HIPCHK(ctx, ctx->d_scratch.ensure(size + 16));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_in.p, src, n, hipMemcpyHostToDevice, st));
    Lz4Job job{};
    job.src = static_cast<const uint8_t*>(ctx->d_in.p);
    job.dst = static_cast<uint8_t*>(ctx->d_scratch.p);
    job.src_len = uint32_t(n);
    job.dst_len = uint32_t(size);
    const size_t o_res = 256, m = 512;
    HIPCHK(ctx, ctx->d_meta.ensure(m));
    HIPCHK(ctx, ctx->h_meta.ensure(m));
    HIPCHK(ctx, ctx->h_res.ensure(512));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_meta.p);
    std::memset(h, 0, m);
    std::memcpy(h, &job, sizeof job);
    uint8_t* d = static_cast<uint8_t*>(ctx->d_meta.p);
    HIPCHK(ctx, hipMemcpyAsync(d, h, m, hipMemcpyHostToDevice, st));
    launch_lz4(reinterpret_cast<Lz4Job*>(d), nullptr, 1, reinterpret_cast<DevChunkResult*>(d + o_res), st);
    HIPCHK(ctx, hipGetLastError());
    uint8_t* hr = static_cast<uint8_t*>(ctx->h_res.p);
    HIPCHK(ctx, hipMemcpyAsync(hr, d, m, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    Lz4Job done;
    std::memcpy(&done, hr, sizeof done);
    const DevChunkResult* r = reinterpret_cast<const DevChunkResult*>(hr + o_res);
    if (r->status != 0) return fail(ctx, r->status, "lz4: corrupt input");
    if (done.produced) HIPCHK(ctx, hipMemcpy(dst, ctx->d_scratch.p, done.produced, hipMemcpyDeviceToHost));
    *out_len = done.produced;
    return PF_OK;
}

// GPU page-header scan (pfloor.h): k_page_scan per chunk, then k_page_crc over the pages found.
int pf_scan_pages(pf_ctx* ctx, const pf_scan_chunk* chunks, int n_chunks, const uint8_t* bytes, size_t n_bytes,
                  int bytes_on_device, int verify_crc, pf_page_desc* pages_out, pf_scan_result* results) {
    if (!ctx || n_chunks < 0 || (n_chunks && (!chunks || !results || !pages_out)) || (!bytes && n_bytes))
        return fail(ctx, PF_ERR_INVALID_ARG, "scan: null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n_chunks == 0) return PF_OK;
    int64_t slots = 0;
    for (int c = 0; c < n_chunks; c++) {
        const pf_scan_chunk& k = chunks[c];
        if (k.page_base < 0 || k.page_cap < 0 || k.chunk_offset > n_bytes || k.chunk_size > n_bytes - k.chunk_offset)
            return fail(ctx, PF_ERR_INVALID_ARG, "scan: chunk " + std::to_string(c) + " outside the buffer / bad slots");
        slots = std::max<int64_t>(slots, int64_t(k.page_base) + k.page_cap);
    }
    if (slots > (int64_t(1) << 30)) return fail(ctx, PF_ERR_INVALID_ARG, "scan: too many page slots");
    if (const int rc = begin_oneshot(ctx, false)) return rc;   // (its tables are d_scan's: the last decode's stay)
    hipStream_t st = ctx->stream;
    const uint8_t* d_bytes = bytes;
    if (!bytes_on_device && n_bytes) {
        HIPCHK(ctx, ctx->d_scan_in.ensure(n_bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_scan_in.p, bytes, n_bytes, hipMemcpyHostToDevice, st));
        d_bytes = static_cast<const uint8_t*>(ctx->d_scan_in.p);
    }
    size_t m = 0;
    auto take = [](size_t& cursor, size_t sz) { size_t o = align_up(cursor, 256); cursor = o + sz; return o; };
    const size_t ns = size_t(std::max<int64_t>(slots, 1));
    const size_t o_ck = take(m, sizeof(ScanChunk) * n_chunks), o_pg = take(m, sizeof(pf_page_desc) * ns);
    const size_t o_crc = take(m, sizeof(ScanCrc) * ns), o_res = take(m, sizeof(ScanResult) * n_chunks);
    const size_t o_bad = take(m, 4 * size_t(n_chunks)), o_list = take(m, 4 * ns);
    m = align_up(m, 256);
    HIPCHK(ctx, ctx->d_scan.ensure(m));
    HIPCHK(ctx, ctx->h_meta.ensure(m));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_meta.p);
    uint8_t* d = static_cast<uint8_t*>(ctx->d_scan.p);
    ScanChunk* hc = reinterpret_cast<ScanChunk*>(h + o_ck);
    for (int c = 0; c < n_chunks; c++)
        hc[c] = ScanChunk{d_bytes + chunks[c].chunk_offset, chunks[c].chunk_size, chunks[c].num_values, chunks[c].page_base,
                          chunks[c].page_cap};
    int32_t* hbad = reinterpret_cast<int32_t*>(h + o_bad);
    for (int c = 0; c < n_chunks; c++) hbad[c] = INT32_MAX;
    HIPCHK(ctx, hipMemcpyAsync(d + o_ck, h + o_ck, o_list - o_ck, hipMemcpyHostToDevice, st));
    ScanResult* d_res = reinterpret_cast<ScanResult*>(d + o_res);
    ScanCrc* d_crc = reinterpret_cast<ScanCrc*>(d + o_crc);
    launch_page_scan(reinterpret_cast<const ScanChunk*>(d + o_ck), n_chunks, reinterpret_cast<pf_page_desc*>(d + o_pg),
                     d_crc, d_res, st);
    HIPCHK(ctx, hipGetLastError());
    ScanResult* hr = reinterpret_cast<ScanResult*>(h + o_res);
    HIPCHK(ctx, hipMemcpyAsync(hr, d_res, sizeof(ScanResult) * n_chunks, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (verify_crc) {
        int32_t* hl = reinterpret_cast<int32_t*>(h + o_list);
        int n = 0;
        for (int c = 0; c < n_chunks; c++)
            for (int i = 0; i < hr[c].n_pages; i++) hl[n++] = chunks[c].page_base + i;
        if (n) {
            HIPCHK(ctx, hipMemcpyAsync(d + o_list, hl, 4 * size_t(n), hipMemcpyHostToDevice, st));
            launch_page_crc(d_crc, reinterpret_cast<const int*>(d + o_list), n, d_res, reinterpret_cast<int32_t*>(d + o_bad), st);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(hr, d_res, sizeof(ScanResult) * n_chunks, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(hbad, d + o_bad, 4 * size_t(n_chunks), hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(pages_out, d + o_pg, sizeof(pf_page_desc) * size_t(slots), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    int rc = PF_OK;
    for (int c = 0; c < n_chunks; c++) {
        pf_scan_result& r = results[c];
        r.n_pages = hr[c].n_pages;
        r.status = hr[c].status;
        r.err_page = hr[c].err_page;
        r.crc_pages = hr[c].crc_pages;
        if (r.status == PF_OK && verify_crc && hbad[c] != INT32_MAX) {
            r.status = PF_ERR_CORRUPT_PAGE;
            r.err_page = hbad[c] - chunks[c].page_base;
        }
        if (r.status != PF_OK && rc == PF_OK) {
            rc = r.status;
            fail(ctx, rc, "scan: chunk " + std::to_string(c) + " page " + std::to_string(r.err_page) +
                              (hbad[c] != INT32_MAX && verify_crc ? ": CRC checksum verification failed" : ": corrupt page header"));
        }
    }
    return rc;
}

// Test hook: which path decoded the last pf_snappy_decompress (1 = serial fallback).
int pf_snappy_last_fallback(pf_ctx* ctx) {
    return ctx && ctx->h_res.p ? *reinterpret_cast<const int*>(static_cast<uint8_t*>(ctx->h_res.p) + 256) : -1;
}

// Diagnostics (not part of pfloor.h): the index tables of the last pf_snappy_decompress.
int pf_debug_snappy_tables(pf_ctx* ctx, uint32_t* splits, int n_splits, uint32_t* wins, int n_wins, uint32_t* lane_out,
                           uint32_t* tokmap) {
    if (!ctx || !ctx->d_last_splits) return fail(ctx, PF_ERR_STATE, "no snappy tables");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (splits) HIPCHK(ctx, hipMemcpy(splits, ctx->d_last_splits, 4 * size_t(n_splits), hipMemcpyDeviceToHost));
    if (wins) HIPCHK(ctx, hipMemcpy(wins, ctx->d_last_win, sizeof(SnapWin) * size_t(n_wins), hipMemcpyDeviceToHost));
    if (lane_out) HIPCHK(ctx, hipMemcpy(lane_out, ctx->d_last_lane_out, 256 * size_t(n_wins), hipMemcpyDeviceToHost));
    if (tokmap) HIPCHK(ctx, hipMemcpy(tokmap, ctx->d_tokmap.p, 1024 * size_t(n_wins), hipMemcpyDeviceToHost));
    return PF_OK;
}

// Diagnostics (not part of pfloor.h): per Snappy job of the last finished pf_decode_row_group,
// {fallback flag (FB_*), compressed length, decompressed length, chunk, page}. Returns the job count.
int pf_debug_snappy_fallback(pf_ctx* ctx, int* out, int n_jobs) {
    if (!ctx || !ctx->d_meta.p || !ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nj = int(ctx->plan.jobs.size());
    const int m = n_jobs < nj ? n_jobs : nj;
    if (out && m > 0) {
        std::vector<int> fb(size_t(m), 0);
        HIPCHK(ctx, hipMemcpy(fb.data(), static_cast<uint8_t*>(ctx->d_meta.p) + ctx->plan.off_fallback, 4 * size_t(m),
                              hipMemcpyDeviceToHost));
        for (int i = 0; i < m; i++) {
            const SnappyJob& jb = ctx->plan.jobs[size_t(i)];
            const int rec[5] = {fb[size_t(i)], int(jb.src_len), int(jb.dst_len), jb.chunk, jb.page};
            for (int q = 0; q < 5; q++) out[5 * i + q] = rec[q];
        }
    }
    return nj;
}

namespace {
// The first n_pages DevPage records of the last finished pf_decode_row_group as the device left
// them. Returns the batch's page count, or a negative pf_status.
int fetch_pages(pf_ctx* ctx, int n_pages, std::vector<DevPage>& pg) {
    if (!ctx || !ctx->d_meta.p || !ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int np = int(ctx->plan.pages.size());
    pg.resize(size_t(std::max(0, std::min(n_pages, np))));
    if (!pg.empty())
        HIPCHK(ctx, hipMemcpy(pg.data(), static_cast<uint8_t*>(ctx->d_meta.p) + ctx->plan.off_pages, sizeof(DevPage) * pg.size(),
                              hipMemcpyDeviceToHost));
    return np;
}
}  // namespace

// Diagnostics (not part of pfloor.h): per page of the last finished pf_decode_row_group, what
// k_snappy_head decided (DIRECT_NONE / DIRECT_VALUES / DIRECT_INPLACE). Returns the page count.
int pf_debug_page_direct(pf_ctx* ctx, int* out, int n_pages) {
    std::vector<DevPage> pg;
    const int np = fetch_pages(ctx, out ? n_pages : 0, pg);
    if (np >= 0) {
        const int m = int(pg.size());
        for (int i = 0; i < m; i++) out[i] = pg[size_t(i)].direct;
    }
    return np;
}

// Diagnostics (not part of pfloor.h): per page of the last finished pf_decode_row_group, which
// parallel paths took it: {direct (DIRECT_*), dbp_ok (1 = k_dbp_* decoded it, 2 = handed back to
// k_delta), seg_ok (1 = nested segment kernels, 2 = hand-over failed, decoded whole)}. Returns the
// page count; out holds 3 ints per page.
int pf_debug_page_paths(pf_ctx* ctx, int* out, int n_pages) {
    std::vector<DevPage> pg;
    const int np = fetch_pages(ctx, out ? n_pages : 0, pg);
    if (np >= 0) {
        const int m = int(pg.size());
        for (int i = 0; i < m; i++) {
            out[3 * i] = pg[size_t(i)].direct;
            out[3 * i + 1] = pg[size_t(i)].dbp_ok;
            out[3 * i + 2] = pg[size_t(i)].seg_ok;
        }
    }
    return np;
}

// Diagnostics (tests): the done flags of the last decode's pages (DONE_FIXED 1 / DONE_FLAT 2 /
// DONE_NULL 4 / DONE_DSTR 16 with DONE_FLAT: which kernel took the page; k_page_null and k_flat_null both set DONE_NULL, and only
// k_page_null's pages keep no level table (lvl = 0 in out[2 * i + 1])).
extern "C" int pf_debug_page_done(pf_ctx* ctx, int* out, int n_pages) {
    std::vector<DevPage> pg;
    const int np = fetch_pages(ctx, out ? n_pages : 0, pg);
    if (np >= 0) {
        const int m = int(pg.size());
        for (int i = 0; i < m; i++) {
            out[2 * i] = pg[size_t(i)].done;
            uint32_t lt1 = 0;   // k_lvl's "block table fits" word (k_flat_null ran on the page)
            if (pg[size_t(i)].lvltab) HIPCHK(ctx, hipMemcpy(&lt1, &pg[size_t(i)].lvltab->fit, 4, hipMemcpyDeviceToHost));
            out[2 * i + 1] = int(lt1);
        }
    }
    return np;
}

int pf_last_timing(pf_ctx* ctx, float* stage_ms, int n_stages, int* n_written) {
    if (!ctx || !stage_ms || n_stages < 0) return fail(ctx, PF_ERR_INVALID_ARG, "bad arg");
    if (!ctx->timing) return fail(ctx, PF_ERR_STATE, "stage timing is off (pf_ctx_set_timing)");
    if (!ctx->timing_valid) return fail(ctx, PF_ERR_STATE, "no finished decode");
    int k = 0;
    for (int i = 0; i + 1 < N_EVENTS && k < n_stages; i++, k++) {
        float ms = 0;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
        stage_ms[k] = ms;
    }
    if (n_written) *n_written = k;
    return PF_OK;
}

}  // extern "C"
