// pf_runtime.hip — context, arenas and kernel orchestration behind include/pfloor.h.
//
// One pf_ctx per GPU (one HIP stream, growable HBM arenas, pinned staging). A decode batch is
// any set of column chunks (a row group's selected columns, or several row groups). The host
// planner (pf_plan.cpp, no HIP calls) turns the descriptors into flat DevChunk / DevPage /
// SnappyJob tables, launch lists and arena sizes; this file grows the arenas to those sizes, has
// the planner bind its offsets to them, uploads the tables in one copy, and enqueues
//   k_snappy / k_zstd -> k_ba (dictionaries) -> k_delta -> k_count -> k_ba (PLAIN pages) -> k_scan -> k_flat -> k_decode
// on the context stream. Nothing synchronises until pf_wait.
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

#include "pf_crc.h"
#include "pf_encode.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "pf_plan.h"
#include "pf_snappy_par.h"
#include "pf_xxh64.h"
#include "pf_zstd_enc_core.h"
#include "pfloor.h"

using namespace pf;

static_assert(sizeof(Int2) == sizeof(int2) && alignof(Int2) <= alignof(int2), "the planner's pairs are the kernels' int2");

namespace {

thread_local std::string g_err;

int fail(pf_ctx* ctx, int code, const std::string& msg);

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = std::max<size_t>(n + n / 4, 1 << 20);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct HostBuf {
    void* p = nullptr;
    void* d = nullptr;   // the device's address of the pinned pages (kernels read / write them over PCIe)
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; d = nullptr; cap = 0; }
        size_t want = std::max<size_t>(n + n / 4, 1 << 16);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) {
            cap = want;
            if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) d = nullptr;
        }
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; d = nullptr; cap = 0; }
};

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

constexpr int N_EVENTS = 11;  // h2d, snappy parse, snappy exec, dict, delta, levels, count, scan, flat, decode

}  // namespace

// The HIP streams of a context. Shared by contexts made with pf_ctx_create_shared (the stream
// lives until the last of them is destroyed).
struct Streams {
    int device = 0;
    hipStream_t stream = nullptr;
    // pf_copy_batch_async's downloads (made on first use): the next batch's H2D and kernels on `stream`
    // (a twin context's, with its own arenas) run while this batch's columns go to the host
    hipStream_t copy_stream = nullptr;
    std::mutex mu;
    ~Streams() {
        (void)hipSetDevice(device);
        if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }
};

struct pf_ctx {
    int device = 0;
    pf::PfOpts opts;                       // defaults; the diagnostics build reads PF_* at creation
    std::shared_ptr<Streams> streams;
    hipStream_t stream = nullptr;          // = streams->stream
    bool zc = true;                        // metadata / results copied by k_copy_words (PF_ZC=0: SDMA copies)
    hipEvent_t ev[N_EVENTS] = {};
    // recorded after the last operation of this context's decode: pf_wait waits for it, not for the
    // stream, so a context sharing the stream can have the next batch enqueued behind this one
    hipEvent_t ev_done = nullptr;
    // recorded after the last enqueued D2H copy of this context's outputs: pf_copy_column / pf_sync
    // wait for it, not for the stream, so a peer's decode queued behind the copies keeps running
    hipEvent_t ev_copy = nullptr;          // after this context's last async copy (on whichever stream)
    hipEvent_t ev_dl = nullptr;            // the decode a download on the copy stream follows
    hipEvent_t ev_bloom[2] = {};           // pf_encode_chunk: around the Bloom filter's fill (pf_encoded_chunk.bloom_ms)
    bool timing = true;                    // per-stage events (pf_last_timing); pf_ctx_set_timing
    std::string err;
    DevBuf d_in, d_scratch, d_out, d_bits, d_chars, d_meta, d_tokmap;
    DevBuf d_scan_in, d_scan;              // pf_scan_pages: host chunk bytes, tables
    DevBuf d_enc, d_enc_sec, d_enc_out;    // pf_encode_chunk / pf_snappy_compress: work arena, values sections, slots
    std::vector<uint8_t> h_enc;            // the last encoded chunk (headers + bodies)
    std::vector<uint8_t> h_enc_stat;       // its chunk statistics (min ‖ max)
    HostBuf h_enc_st;                      // pf_encode_chunk: statistics results D2H
    HostBuf h_enc_bloom;                   // pf_encode_chunk: the Bloom filter's bitset D2H (pf_encoded_chunk.bloom)
    HostBuf h_meta, h_res;
    HostBuf h_enc_slots;                   // pf_encode_chunk / pf_snappy_compress: compressed slots D2H
    // last batch
    int n_chunks = 0;
    bool pending = false;
    bool copies_pending = false;           // pf_copy_columns_async enqueued, not yet pf_sync'ed
    bool tables_from_decode = false;       // d_meta layout (off_fallback) belongs to a pf_decode_row_group
    bool timing_valid = false;
    pf::BatchPlan plan;                    // the last pf_decode_row_group's tables, lists and layout
    // diagnostics: tables of the last pf_snappy_decompress (pf_debug_snappy_tables)
    const uint32_t* d_last_splits = nullptr;
    const SnapWin* d_last_win = nullptr;
    const uint32_t* d_last_lane_out = nullptr;
    std::vector<pf_column_info> info;
    bool meta_by_kernel = false;   // this batch's metadata went up by k_upload (which also zeroes bits / npub)
    uint64_t chars_need = 0;
    int reruns = 0;
    HostBuf h_enc_px;                      // pf_encode_chunk: the page index block D2H (pf_encoded_chunk.index_*)
    std::vector<int64_t> h_enc_pgoff, h_enc_pgrow;   // pf_encoded_chunk.page_offset / page_first_row
    std::vector<int32_t> h_enc_pgsize;               // pf_encoded_chunk.page_size
    // row windows (pf_decode_row_group_rows): the chunks whose window is not {0, -1}, their tables, and the twin output
    // arenas k_win_copy writes (allocated only for a batch that has such a window)
    std::vector<DevWin> wins;
    DevBuf d_win, d_wout, d_wbits, d_wchars;
    HostBuf h_win;                         // DevWin[n] up, DevWinRes[n] down
    int win_grid = 1;
    hipEvent_t ev_win[2] = {};
    // row filter (pf_decode_row_group_filter): the packed predicates (none: no filter stage), the stage's device buffer
    // and its pinned mirror: [DevSelHead | DevSelChunk[n]] comes down, [DevPred[] | blob | win_of[n]] goes up
    pf::FilterPlan filt;
    DevBuf d_sel;
    HostBuf h_sel;
    pf::SelBufs sel{};
    size_t sel_up_off = 0;                 // where the uploaded tables begin: the bytes before them come down
    int sel_grid = 1;
    hipEvent_t ev_sel[2] = {};
    pf_selection_info sel_info{};
    bool filtered() const { return !filt.preds.empty(); }
    bool twins() const { return !wins.empty() || filtered(); }   // the batch's results are not (all) in the decode arenas
};

namespace {

int fail(pf_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    g_err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, PF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// stage-timing event: only when the context has timing on (each record is a marker on the stream,
// ~7 us between kernels on MI355X, so the product path leaves them off)
#define EVREC(ctx, ev, st)                                 \
    do {                                                   \
        if ((ctx)->timing) HIPCHK(ctx, hipEventRecord(ev, st)); \
    } while (0)

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
                    reinterpret_cast<int*>(meta + p.off_nfbq), d_res, st, ncaps, ctx->opts.null_stagger);
    EVREC(ctx, ctx->ev[9], st);
    if (!(skip & 64u)) launch_decode(d_chunks, d_pages, list(L_DECODE), len(L_DECODE), p.n_decode_first, d_res, st, DECODE_IDLE_GRID);
    launch_nest_decode(d_chunks, d_pages, pairs(L_NSEG), n_nseg, d_res, st);
    launch_dba_chars(d_chunks, d_pages, list(L_DBA), len(L_DBA), d_res, st);
    EVREC(ctx, ctx->ev[10], st);
    if (!ctx->wins.empty()) {   // row windows: after every decode stage, so a chars rerun trims again
        const int nw = int(ctx->wins.size());
        const size_t res_off = align_up(sizeof(DevWin) * nw, 256);
        DevWin* d_wins = static_cast<DevWin*>(ctx->d_win.p);
        DevWinRes* d_wres = reinterpret_cast<DevWinRes*>(static_cast<uint8_t*>(ctx->d_win.p) + res_off);
        EVREC(ctx, ctx->ev_win[0], st);
        launch_window(d_chunks, d_res, d_wins, d_wres, nw, ctx->win_grid, static_cast<const uint8_t*>(ctx->d_chars.p),
                      static_cast<uint8_t*>(ctx->d_wchars.p),
                      static_cast<uint8_t*>(ctx->d_wout.p) - static_cast<uint8_t*>(ctx->d_out.p),
                      static_cast<uint8_t*>(ctx->d_wbits.p) - static_cast<uint8_t*>(ctx->d_bits.p), st);
        EVREC(ctx, ctx->ev_win[1], st);
        HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->h_win.p) + res_off, d_wres, sizeof(DevWinRes) * nw,
                                   hipMemcpyDeviceToHost, st));
    }
    if (ctx->filtered()) {   // the row filter: after the windows, so it sees their rows and a chars rerun filters again
        const DevWinRes* d_wres = ctx->wins.empty() ? nullptr : reinterpret_cast<const DevWinRes*>(
            static_cast<const uint8_t*>(ctx->d_win.p) + align_up(sizeof(DevWin) * ctx->wins.size(), 256));
        EVREC(ctx, ctx->ev_sel[0], st);
        launch_filter(d_chunks, d_res, d_wres, ctx->sel, ctx->n_chunks, ctx->sel_grid, static_cast<const uint8_t*>(ctx->d_chars.p),
                      static_cast<uint8_t*>(ctx->d_wchars.p),
                      static_cast<uint8_t*>(ctx->d_wout.p) - static_cast<uint8_t*>(ctx->d_out.p),
                      static_cast<uint8_t*>(ctx->d_wbits.p) - static_cast<uint8_t*>(ctx->d_bits.p), st);
        EVREC(ctx, ctx->ev_sel[1], st);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_sel.p, ctx->d_sel.p, ctx->sel_up_off, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipGetLastError());
    // results + device-written chunk fields (chars base) back to pinned host memory
    const size_t res_pad = align_up(sizeof(DevChunkResult) * ctx->n_chunks, 256);
    if (ctx->zc && ctx->h_res.d) {
        copy_words(ctx->h_res.d, meta + p.off_res, sizeof(DevChunkResult) * ctx->n_chunks,
                   static_cast<uint8_t*>(ctx->h_res.d) + res_pad, d_chunks, sizeof(DevChunk) * ctx->n_chunks, st);
    } else {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_res.p, meta + p.off_res, sizeof(DevChunkResult) * ctx->n_chunks,
                                   hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(static_cast<uint8_t*>(ctx->h_res.p) + res_pad, d_chunks, sizeof(DevChunk) * ctx->n_chunks,
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
    put(p.off_pieces, p.snap.pieces);
    std::memset(h + p.off_splits, 0xff, sizeof(uint32_t) * p.snap.n_splits);
    put(p.off_wins, p.snap.wins);
    put(p.off_bajobs, p.bajobs);
    put(p.off_batiles, p.ba_tiles);
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


// ---------------------------------------------------------------- write path (pf_encode.hip)
namespace {
size_t uvarint_len(uint64_t v) { size_t k = 1; while (v >= 0x80) { v >>= 7; k++; } return k; }
void put_uvarint(std::vector<uint8_t>& o, uint64_t v) {
    while (v >= 0x80) { o.push_back(uint8_t(v | 0x80)); v >>= 7; }
    o.push_back(uint8_t(v));
}

// Bytes the host puts in front of a section's jobs: Snappy's length varint, or ZSTD's frame header (and for
// a section of 0 bytes, which has no job, the one empty last raw block).
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

// Compress `sections` (device, each [off, off + len) of `base`) with `codec` (PF_CODEC_SNAPPY | PF_CODEC_ZSTD)
// into the slots of independent jobs of SC_BLOCK / ZC_BLOCK bytes; returns per section the host stream (Snappy:
// varint length + block outputs; ZSTD: frame header + the jobs' blocks) in `streams`.
// With `crc_out` (PF_ENCODE_PAGE_CRC): k_enc_crc right behind the compressor over every job's slot, in job
// order, then over `extra`; the results come back in the copy that brings the jobs' lengths.
int compress_sections(pf_ctx* ctx, const uint8_t* base, const std::vector<std::pair<uint64_t, uint64_t>>& sections,
                      std::vector<std::vector<uint8_t>>& streams, int codec, float* kernel_ms = nullptr,
                      const std::vector<CrcPiece>* extra = nullptr, std::vector<CrcOut>* crc_out = nullptr, float* crc_ms = nullptr) {
    hipStream_t st = ctx->stream;
    const bool zs = codec == PF_CODEC_ZSTD;
    const uint32_t JOB = zs ? ZC_BLOCK : SC_BLOCK, SLOT = zs ? ZC_SLOT : SC_SLOT;
    std::vector<CompJob> jobs;
    std::vector<std::pair<size_t, size_t>> range(sections.size());   // jobs of each section
    for (size_t i = 0; i < sections.size(); i++) {
        range[i].first = jobs.size();
        for (uint64_t o = 0; o < sections[i].second; o += JOB) {
            CompJob j{};
            j.src = base + sections[i].first + o;
            j.len = uint32_t(std::min<uint64_t>(JOB, sections[i].second - o));
            j.last = zs && o + j.len == sections[i].second;
            jobs.push_back(j);
        }
        range[i].second = jobs.size();
    }
    const size_t nj = jobs.size();
    size_t m = 0;
    auto take = [](size_t& cur, size_t sz) { size_t o = align_up(cur, 256); cur = o + sz; return o; };
    const size_t o_jobs = take(m, sizeof(CompJob) * std::max<size_t>(nj, 1));
    // the jobs' lengths and, behind them, the pieces' CRCs: one D2H
    const size_t np = crc_out ? nj + (extra ? extra->size() : 0) : 0;
    const size_t o_crc_in_len = align_up(4 * nj, 16);
    const size_t len_bytes = np ? o_crc_in_len + sizeof(CrcOut) * np : 4 * std::max<size_t>(nj, 1);
    const size_t o_len = take(m, len_bytes);
    const size_t o_pieces = take(m, sizeof(CrcPiece) * std::max<size_t>(np, 1));
    const size_t o_slots = take(m, size_t(SLOT) * std::max<size_t>(nj, 1));
    HIPCHK(ctx, ctx->d_enc_out.ensure(m));
    uint8_t* d = static_cast<uint8_t*>(ctx->d_enc_out.p);
    for (size_t k = 0; k < nj; k++) jobs[k].dst = d + o_slots + k * SLOT;
    // compressed lengths + slots come back into the context's pinned staging (no zero-fill, DMA speed)
    HIPCHK(ctx, ctx->h_enc_slots.ensure(align_up(len_bytes, 256) + nj * size_t(SLOT)));
    uint32_t* lens = static_cast<uint32_t*>(ctx->h_enc_slots.p);
    uint8_t* slots = static_cast<uint8_t*>(ctx->h_enc_slots.p) + align_up(len_bytes, 256);
    std::vector<CrcPiece> pieces(np);
    if (nj) {
        HIPCHK(ctx, hipMemcpyAsync(d + o_jobs, jobs.data(), sizeof(CompJob) * nj, hipMemcpyHostToDevice, st));
        EVREC(ctx, ctx->ev[0], st);
        (zs ? launch_zstd_compress : launch_snappy_compress)(reinterpret_cast<const CompJob*>(d + o_jobs), int(nj), reinterpret_cast<uint32_t*>(d + o_len), st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev[1], st);
    }
    if (np) {
        const uint32_t* d_len = reinterpret_cast<const uint32_t*>(d + o_len);
        for (size_t k = 0; k < nj; k++) pieces[k] = CrcPiece{jobs[k].dst, d_len + k, 0u, SLOT};
        for (size_t k = nj; k < np; k++) pieces[k] = (*extra)[k - nj];
        HIPCHK(ctx, hipMemcpyAsync(d + o_pieces, pieces.data(), sizeof(CrcPiece) * np, hipMemcpyHostToDevice, st));
        EVREC(ctx, ctx->ev[8], st);
        launch_enc_crc(reinterpret_cast<const CrcPiece*>(d + o_pieces), int(np), reinterpret_cast<CrcOut*>(d + o_len + o_crc_in_len), st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev[9], st);
    }
    if (nj || np) HIPCHK(ctx, hipMemcpyAsync(lens, d + o_len, np ? len_bytes : 4 * nj, hipMemcpyDeviceToHost, st));
    if (nj) HIPCHK(ctx, hipMemcpyAsync(slots, d + o_slots, nj * size_t(SLOT), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (crc_out) {
        const CrcOut* h = reinterpret_cast<const CrcOut*>(reinterpret_cast<const uint8_t*>(lens) + o_crc_in_len);
        crc_out->assign(h, h + np);
    }
    if (crc_ms) {
        *crc_ms = 0.f;
        if (ctx->timing && np) HIPCHK(ctx, hipEventElapsedTime(crc_ms, ctx->ev[8], ctx->ev[9]));
    }
    if (kernel_ms) {
        *kernel_ms = 0.f;
        if (ctx->timing && nj) HIPCHK(ctx, hipEventElapsedTime(kernel_ms, ctx->ev[0], ctx->ev[1]));
    }
    streams.assign(sections.size(), {});
    for (size_t i = 0; i < sections.size(); i++) {
        std::vector<uint8_t>& o = streams[i];
        uint8_t head[12];
        o.assign(head, head + stream_head(codec, sections[i].second, head));
        for (size_t k = range[i].first; k < range[i].second; k++) {
            if (lens[k] > (zs ? 3 + jobs[k].len : SLOT)) return fail(ctx, PF_ERR_HIP, zs ? "zstd compress: block overflow" : "snappy compress: block overflow");
            const uint8_t* b = slots + k * size_t(SLOT);
            o.insert(o.end(), b, b + lens[k]);
        }
    }
    return PF_OK;
}
}  // namespace

extern "C" int pf_snappy_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    if (!ctx || (!src && n) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n > 0xffffffffull) return fail(ctx, PF_ERR_INVALID_ARG, "snappy: buffer too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
    HIPCHK(ctx, ctx->d_enc.ensure(std::max<size_t>(n, 1)));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_enc.p, src, n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<std::vector<uint8_t>> streams;
    const int rc = compress_sections(ctx, static_cast<const uint8_t*>(ctx->d_enc.p), {{0, n}}, streams, PF_CODEC_SNAPPY);
    if (rc) return rc;
    *out_len = streams[0].size();
    if (streams[0].size() > cap) return fail(ctx, PF_ERR_CAPACITY, "snappy: destination too small");
    std::memcpy(dst, streams[0].data(), streams[0].size());
    return PF_OK;
}

extern "C" int pf_zstd_compress(pf_ctx* ctx, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
    if (!ctx || (!src && n) || !out_len) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    if (n > 0xffffffffull) return fail(ctx, PF_ERR_INVALID_ARG, "zstd: buffer too large");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
    HIPCHK(ctx, ctx->d_enc.ensure(std::max<size_t>(n, 1)));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->d_enc.p, src, n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<std::vector<uint8_t>> streams;
    const int rc = compress_sections(ctx, static_cast<const uint8_t*>(ctx->d_enc.p), {{0, n}}, streams, PF_CODEC_ZSTD);
    if (rc) return rc;
    *out_len = streams[0].size();
    if (streams[0].size() > cap) return fail(ctx, PF_ERR_CAPACITY, "zstd: destination too small");
    std::memcpy(dst, streams[0].data(), streams[0].size());
    return PF_OK;
}

extern "C" int pf_encode_chunk(pf_ctx* ctx, const pf_encode_column* col, int on_device, pf_encoded_chunk* out) {
    if (!ctx || !col || !out) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    const int pt = col->physical_type;
    if (pt != PF_BOOLEAN && pt != PF_INT32 && pt != PF_INT64 && pt != PF_FLOAT && pt != PF_DOUBLE && pt != PF_BYTE_ARRAY)
        return fail(ctx, PF_ERR_UNSUPPORTED_TYPE, "encode: unsupported physical type");
    const int64_t n = col->num_rows;
    if (n < 0 || n > 0x7ffffff0 || (col->max_def != 0 && col->max_def != 1)) return fail(ctx, PF_ERR_INVALID_ARG, "encode: bad shape");
    if (col->codec != PF_CODEC_SNAPPY && col->codec != PF_CODEC_ZSTD && col->codec != PF_CODEC_UNCOMPRESSED)
        return fail(ctx, PF_ERR_UNSUPPORTED_CODEC, "encode: codec must be SNAPPY, ZSTD or UNCOMPRESSED");
    const bool compressed = col->codec != PF_CODEC_UNCOMPRESSED;
    if (col->bloom_bytes != 0 && (col->bloom_bytes < 0 || !bloom_size_ok(uint64_t(col->bloom_bytes))))
        return fail(ctx, PF_ERR_INVALID_ARG, "encode: bloom_bytes must be a power of two in [32, 128 MiB]");
    const size_t bloom = pt == PF_BOOLEAN ? 0 : size_t(col->bloom_bytes);   // BOOLEAN: no filter (parquet-mr builds none)
    const bool str = pt == PF_BYTE_ARRAY;
    const bool want_index = (col->dictionary & PF_ENCODE_PAGE_INDEX) != 0;
    if (want_index && str && col->index_truncate != 0 && col->index_truncate != -1 &&
        (col->index_truncate < 1 || col->index_truncate > 2047))
        return fail(ctx, PF_ERR_INVALID_ARG, "encode: index_truncate must be 0, -1 or in [1, 2047]");
    const uint32_t px_trunc = col->index_truncate == -1 ? PX_NO_TRUNC : col->index_truncate == 0 ? 64u : uint32_t(col->index_truncate);
    if (n > 0 && (str ? (!col->offsets || (!col->chars && col->chars_len > 0) || col->chars_len < 0 || col->chars_len > 0x7fffffff)
                      : !col->values))
        return fail(ctx, PF_ERR_INVALID_ARG, "encode: missing input arrays");
    const int w = pt == PF_BOOLEAN ? 1 : type_width(pt, 0);
    int64_t page_rows = col->page_rows > 0 ? col->page_rows : 20000;
    page_rows = (page_rows + 7) / 8 * 8;   // definition levels of a page start on a validity byte
    // dictionary page limit (parquet.dictionary.page.size, 1 MiB); capped so a dictionary that passes it
    // always fits the 32-bit offsets of the dictionary kernels
    const int64_t dict_limit = std::min<int64_t>(col->dict_page_limit > 0 ? col->dict_page_limit : (1 << 20), 0x7fffffff);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;

    // host copies of validity / offsets (page plan, definition levels)
    const size_t vbytes = size_t((n + 7) / 8);
    std::vector<uint8_t> hval;
    std::vector<int32_t> hoff;
    const bool has_val = col->max_def == 1 && col->validity;
    if (has_val) {
        hval.resize(vbytes);
        if (on_device) HIPCHK(ctx, hipMemcpy(hval.data(), col->validity, vbytes, hipMemcpyDeviceToHost));
        else std::memcpy(hval.data(), col->validity, vbytes);
    }
    if (str && n > 0) {
        hoff.resize(size_t(n) + 1);
        if (on_device) HIPCHK(ctx, hipMemcpy(hoff.data(), col->offsets, 4 * (size_t(n) + 1), hipMemcpyDeviceToHost));
        else std::memcpy(hoff.data(), col->offsets, 4 * (size_t(n) + 1));
        for (int64_t r = 0; r < n; r++)
            if (hoff[r + 1] < hoff[r] || hoff[r] < 0 || hoff[r + 1] > col->chars_len)
                return fail(ctx, PF_ERR_INVALID_ARG, "encode: offsets out of order or outside chars");
    }
    auto present = [&](int64_t r) { return !has_val || ((hval[size_t(r >> 3)] >> (r & 7)) & 1); };
    // page plan: rows, present values, PLAIN byte sizes
    struct PagePlanE { int64_t r0, r1; uint32_t d0, cnt; uint64_t plain; };
    std::vector<PagePlanE> pp;
    uint32_t m = 0;
    for (int64_t r0 = 0; r0 < n || (n == 0 && pp.empty()); r0 += page_rows) {
        PagePlanE p{r0, std::min(n, r0 + page_rows), m, 0, 0};
        for (int64_t r = p.r0; r < p.r1; r++)
            if (present(r)) {
                p.cnt++;
                if (str) p.plain += 4 + uint64_t(hoff[r + 1] - hoff[r]);
            }
        if (!str) p.plain = pt == PF_BOOLEAN ? (p.cnt + 7) / 8 : uint64_t(p.cnt) * w;
        m += p.cnt;
        pp.push_back(p);
        if (n == 0) break;
    }
    // DELTA_* fallback (PF_ENCODE_DELTA_FALLBACK): one stream per integer page, two (prefix lengths,
    // suffix lengths) per string page; an item of the size table is a stream header or a 128-delta block
    const bool delta_bit = (col->dictionary & PF_ENCODE_DELTA_FALLBACK) && (pt == PF_INT32 || pt == PF_INT64 || str);
    std::vector<DeltaStream> dstreams;
    std::vector<DeltaPage> dpages;
    uint32_t n_items = 0;
    if (delta_bit) {
        for (size_t i = 0; i < pp.size(); i++) {
            const PagePlanE& p = pp[i];
            const uint32_t ns = str ? 2u : 1u, blocks = p.cnt > 1 ? (p.cnt - 1 + 127) / 128 : 0u;
            // worst case of the values section (every block: zigzag(min) + widths + full-width values)
            const uint64_t worst = ns * (25ull + blocks * 14ull + uint64_t(p.cnt) * (str ? 4 : w)) + (str ? p.plain : 0);
            if (worst > 0x7fffffffull) return fail(ctx, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
            dpages.push_back(DeltaPage{0, p.d0, p.cnt, uint32_t(dstreams.size()), ns});
            for (uint32_t k = 0; k < ns; k++) {
                dstreams.push_back(DeltaStream{nullptr, uint32_t(str ? 4 : w), p.cnt, uint32_t(i), n_items});
                n_items += 1 + blocks;
            }
        }
        dstreams.push_back(DeltaStream{nullptr, 0, 0, 0, n_items});
    }
    // parquet-mr's hybrid runs (PF_ENCODE_HYBRID_RUNS): a page has a stream of levels (OPTIONAL) and one of
    // ids or BOOLEAN values
    const bool hyb = (col->dictionary & PF_ENCODE_HYBRID_RUNS) != 0;
    const size_t n_hs_max = hyb ? 2 * pp.size() : 0;
    // statistics (PF_ENCODE_STATISTICS): a workgroup per (page, tile of ST_TILE present values)
    const bool want_stats = (col->dictionary & PF_ENCODE_STATISTICS) != 0;
    const bool want_crc = (col->dictionary & PF_ENCODE_PAGE_CRC) != 0;
    const bool run_stats = want_stats || want_index;   // the page index is built from the statistics kernels' page results
    std::vector<StatTile> stiles;
    std::vector<uint32_t> sptile;
    if (run_stats) {
        for (size_t i = 0; i < pp.size(); i++) {
            sptile.push_back(uint32_t(stiles.size()));
            for (uint32_t o = 0; o < pp[i].cnt; o += ST_TILE)
                stiles.push_back(StatTile{uint32_t(i), pp[i].d0 + o, std::min(ST_TILE, pp[i].cnt - o), 0u});
        }
        sptile.push_back(uint32_t(stiles.size()));
    }
    const size_t n_se = run_stats ? pp.size() + 1 : 0;   // statistics entries: the pages, then the chunk
    // page index (PF_ENCODE_PAGE_INDEX): the pages' rows and present values go up, one block comes back:
    // head | null_counts | offsets | null_pages | values (the worst case: every entry as long as it can get)
    const size_t n_px = want_index ? pp.size() : 0;
    const uint64_t px_entry = !str ? uint64_t(w) : px_trunc == PX_NO_TRUNC ? uint64_t(ST_LIMIT) / 2 : uint64_t(px_trunc);
    const uint64_t px_cap = 2 * px_entry * n_px;
    if (px_cap > 0x40000000ull) return fail(ctx, PF_ERR_INVALID_ARG, "encode: page index values over 1 GiB (fewer pages or a shorter index_truncate)");
    const size_t px_nc = sizeof(PgIndexHead), px_off = px_nc + 8 * n_px, px_np = px_off + 4 * (2 * n_px + 1), px_val = px_np + n_px;
    const size_t px_bytes = want_index ? px_val + size_t(px_cap) : 0;

    // ---- device arena ----
    size_t a_sz = 0;
    auto take = [](size_t& cur, size_t sz) { size_t o = align_up(cur, 256); cur = o + std::max<size_t>(sz, 1); return o; };
    const size_t N1 = size_t(n) + 1;
    const size_t o_in = take(a_sz, str ? 0 : size_t(n) * w), o_vl = take(a_sz, vbytes);
    const size_t o_of = take(a_sz, str ? 4 * N1 : 0), o_ch = take(a_sz, str ? size_t(col->chars_len) : 0);
    const size_t o_flag = take(a_sz, 4 * N1), o_pos = take(a_sz, 4 * N1), o_dense = take(a_sz, size_t(n) * w);
    const size_t o_dsrc = take(a_sz, str ? 4 * N1 : 0), o_dlen = take(a_sz, str ? 4 * N1 : 0);
    const size_t o_vsz = take(a_sz, str ? 4 * N1 : 0), o_vpre = take(a_sz, str ? 4 * N1 : 0);
    const size_t o_key = take(a_sz, 8 * N1), o_skey = take(a_sz, 8 * N1), o_didx = take(a_sz, 4 * N1), o_sidx = take(a_sz, 4 * N1);
    const size_t o_hp = take(a_sz, 4 * N1), o_head = take(a_sz, 4 * N1), o_mark = take(a_sz, 4 * N1), o_did = take(a_sz, 4 * N1);
    const size_t o_dsz = take(a_sz, 4 * N1), o_doff = take(a_sz, 4 * N1), o_ids = take(a_sz, 4 * N1), o_col = take(a_sz, 256);
    // DELTA_* tables (only with the bit set): string prefix / suffix lengths and positions, streams, pages,
    // item bytes and offsets, block minima and widths, page totals
    const size_t NI1 = delta_bit ? size_t(n_items) + 1 : 0;
    const size_t o_pfx = take(a_sz, delta_bit && str ? 4 * N1 : 0), o_sfx = take(a_sz, delta_bit && str ? 4 * N1 : 0);
    const size_t o_spre = take(a_sz, delta_bit && str ? 4 * N1 : 0);
    const size_t o_dstr = take(a_sz, sizeof(DeltaStream) * dstreams.size()), o_dpg = take(a_sz, sizeof(DeltaPage) * dpages.size());
    const size_t o_dby = take(a_sz, 4 * NI1), o_dof = take(a_sz, 4 * NI1), o_dmin = take(a_sz, 8 * NI1), o_dwd = take(a_sz, 4 * NI1);
    const size_t o_dtot = take(a_sz, 4 * dpages.size());
    const size_t o_hstr = take(a_sz, sizeof(HybridStream) * n_hs_max), o_hby = take(a_sz, 4 * n_hs_max);
    const size_t o_stt = take(a_sz, sizeof(StatTile) * stiles.size()), o_stp = take(a_sz, 4 * sptile.size());
    const size_t o_spart = take(a_sz, sizeof(StatPart) * stiles.size()), o_swin = take(a_sz, str ? 8 * stiles.size() : 0);
    const size_t o_sout = take(a_sz, sizeof(StatPart) * n_se), o_sbytes = take(a_sz, str ? size_t(ST_LIMIT) * n_se : 0);
    const size_t o_xin = take(a_sz, 8 * n_px), o_xnn = take(a_sz, 4 * n_px), o_xout = take(a_sz, px_bytes);
    size_t temp_bytes = 0;
    HIPCHK(ctx, enc_scan_temp(std::max(N1, NI1), temp_bytes));   // the scans over rows, dense values and delta items
    const size_t o_temp = take(a_sz, temp_bytes);
    const size_t o_bloom = bloom ? take(a_sz, bloom) : 0;
    HIPCHK(ctx, ctx->d_enc.ensure(a_sz));
    uint8_t* A = static_cast<uint8_t*>(ctx->d_enc.p);
    EncArgs ea{};
    ea.ptype = pt; ea.width = w; ea.n = n;
    if (on_device) {
        ea.values = static_cast<const uint8_t*>(col->values);
        ea.validity = has_val ? col->validity : nullptr;
        ea.offsets = col->offsets;
        ea.chars = col->chars;
    } else {
        if (!str && n) HIPCHK(ctx, hipMemcpyAsync(A + o_in, col->values, size_t(n) * w, hipMemcpyHostToDevice, st));
        if (has_val && vbytes) HIPCHK(ctx, hipMemcpyAsync(A + o_vl, hval.data(), vbytes, hipMemcpyHostToDevice, st));
        if (str && n) {
            HIPCHK(ctx, hipMemcpyAsync(A + o_of, hoff.data(), 4 * N1, hipMemcpyHostToDevice, st));
            if (col->chars_len) HIPCHK(ctx, hipMemcpyAsync(A + o_ch, col->chars, size_t(col->chars_len), hipMemcpyHostToDevice, st));
        }
        ea.values = A + o_in;
        ea.validity = has_val ? A + o_vl : nullptr;
        ea.offsets = reinterpret_cast<const int32_t*>(A + o_of);
        ea.chars = A + o_ch;
    }
    ea.flag = reinterpret_cast<uint32_t*>(A + o_flag); ea.pos = reinterpret_cast<uint32_t*>(A + o_pos);
    ea.dense = A + o_dense;
    ea.dsrc = reinterpret_cast<uint32_t*>(A + o_dsrc); ea.dlen = reinterpret_cast<uint32_t*>(A + o_dlen);
    ea.vsz = reinterpret_cast<uint32_t*>(A + o_vsz); ea.vpre = reinterpret_cast<uint32_t*>(A + o_vpre);
    ea.key = reinterpret_cast<uint64_t*>(A + o_key); ea.skey = reinterpret_cast<uint64_t*>(A + o_skey);
    ea.didx = reinterpret_cast<uint32_t*>(A + o_didx); ea.sidx = reinterpret_cast<uint32_t*>(A + o_sidx);
    ea.headpos = reinterpret_cast<uint32_t*>(A + o_hp); ea.head = reinterpret_cast<uint32_t*>(A + o_head);
    ea.mark = reinterpret_cast<uint32_t*>(A + o_mark); ea.did = reinterpret_cast<uint32_t*>(A + o_did);
    ea.dsz = reinterpret_cast<uint32_t*>(A + o_dsz); ea.doff = reinterpret_cast<uint32_t*>(A + o_doff);
    ea.ids = reinterpret_cast<uint32_t*>(A + o_ids); ea.collide = reinterpret_cast<uint32_t*>(A + o_col);
    void* temp = A + o_temp;

    HIPCHK(ctx, hipMemsetAsync(A + o_col, 0, 256, st));
    if (str) HIPCHK(ctx, hipMemsetAsync(ea.vsz, 0, 4 * N1, st));
    EVREC(ctx, ctx->ev[2], st);
    if (n) HIPCHK(ctx, enc_dense(ea, temp, temp_bytes, st));
    if (str) HIPCHK(ctx, enc_plain_sizes(ea, m, temp, temp_bytes, st));
    // The device sums dictionary bytes in 32 bits: a BYTE_ARRAY column whose dictionary could reach 4 GiB
    // (all values distinct: 4 m + chars) is written PLAIN (conservative: such a dictionary is over any
    // page limit unless most values repeat; parity with parquet-mr's writer is unpinned).
    const bool dict_fits32 = !str || 4ull * uint64_t(m) + uint64_t(col->chars_len) < (1ull << 32);
    const bool dict_bit = (col->dictionary & PF_ENCODE_DICTIONARY) != 0;
    const bool want_dict = dict_bit && pt != PF_BOOLEAN && m > 0 && dict_fits32;
    uint32_t hres[3] = {0, 0, 0};   // collide, dictionary entries, dictionary bytes
    float enc_ms = 0.f;
    if (want_dict) {
        HIPCHK(ctx, enc_dictionary(ea, m, w == 4 ? 32 : 64, temp, temp_bytes, st));
        EVREC(ctx, ctx->ev[3], st);
        HIPCHK(ctx, hipMemcpyAsync(&hres[0], ea.collide, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&hres[1], ea.did + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&hres[2], ea.doff + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&enc_ms, ctx->ev[2], ctx->ev[3]));
    }
    int fallback = 0;
    if (dict_bit && pt == PF_BOOLEAN) fallback = 3;
    else if (want_dict && hres[0]) fallback = 2;
    else if (dict_bit && pt != PF_BOOLEAN && m > 0 && !dict_fits32) fallback = 1;
    else if (want_dict && (str ? int64_t(hres[2]) : int64_t(hres[1]) * w) > dict_limit) fallback = 1;   // fixed: D * w on the host
    const bool dict = want_dict && fallback == 0;
    const uint32_t D = dict ? hres[1] : 0, dict_bytes = dict ? (str ? hres[2] : hres[1] * uint32_t(w)) : 0;
    uint32_t bw = 1;
    while (D > 1 && (uint64_t(1) << bw) < D) bw++;
    if (hyb && D == 1) bw = 0;   // parquet-mr's getWidthFromMaxInt(D - 1)
    const bool brle = hyb && pt == PF_BOOLEAN;   // parquet-mr v2 writes BOOLEAN with the RLE encoding

    // ---- values sections: [dictionary page | page 0 | page 1 | ...] in d_enc_out's front ----
    const bool delta = delta_bit && !dict;   // the chunk is not dictionary-encoded: DELTA_* pages
    const int data_enc = dict ? PF_ENC_RLE_DICTIONARY : delta ? (str ? PF_ENC_DELTA_BYTE_ARRAY : PF_ENC_DELTA_BINARY_PACKED)
                              : brle ? PF_ENC_RLE : PF_ENC_PLAIN;
    std::vector<EncPage> ep(delta ? 0 : pp.size());
    std::vector<std::pair<uint64_t, uint64_t>> sections;
    size_t vo = 0;
    const size_t o_dict = take(vo, dict_bytes);
    if (dict) sections.push_back({o_dict, dict_bytes});
    // Hybrid streams: size pass (after the ids, which it reads) -> the streams' bytes in one D2H and one sync ->
    // the host sizes the sections and the levels -> write pass over the same grid.
    std::vector<HybridStream> hs;
    std::vector<uint32_t> hbytes;
    std::vector<int> lv_of(pp.size(), -1), vs_of(pp.size(), -1);   // a page's level / value stream
    std::vector<size_t> lv_off(pp.size(), 0);                       // a page's levels in hlv
    size_t o_lv = 0, lv_total = 0;
    HybridArgs ha{};
    auto hybrid_sizes = [&]() -> int {
        for (size_t i = 0; i < pp.size() && col->max_def == 1; i++) {
            lv_of[i] = int(hs.size());
            hs.push_back(HybridStream{ea.validity, 0, HY_VALIDITY, uint32_t(pp[i].r0), uint32_t(pp[i].r1 - pp[i].r0), 1,
                                      HY_PREFIX_NONE, uint32_t(i)});
        }
        for (size_t i = 0; i < pp.size() && (dict || brle); i++) {
            vs_of[i] = int(hs.size());
            hs.push_back(dict ? HybridStream{reinterpret_cast<const uint8_t*>(ea.ids), 0, HY_IDS, pp[i].d0, pp[i].cnt, bw,
                                             HY_PREFIX_WIDTH, uint32_t(i)}
                              : HybridStream{ea.dense, 0, HY_BOOL, pp[i].d0, pp[i].cnt, 1, HY_PREFIX_LENGTH, uint32_t(i)});
        }
        ha.streams = reinterpret_cast<const HybridStream*>(A + o_hstr);
        ha.n_streams = uint32_t(hs.size());
        ha.bytes = reinterpret_cast<uint32_t*>(A + o_hby);
        hbytes.assign(hs.size(), 0);
        EVREC(ctx, ctx->ev[6], st);
        if (dict) enc_dictionary_page_and_ids(ea, m, st);
        if (!hs.empty()) {
            HIPCHK(ctx, hipMemcpyAsync(A + o_hstr, hs.data(), sizeof(HybridStream) * hs.size(), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, enc_hybrid_sizes(ha, st));
        }
        EVREC(ctx, ctx->ev[7], st);
        if (!hs.empty()) HIPCHK(ctx, hipMemcpyAsync(hbytes.data(), ha.bytes, 4 * hs.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->timing) {
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
            enc_ms += ms;
        }
        return PF_OK;
    };
    auto place_levels = [&](size_t& cur) {   // the pages' levels, back to back behind the values sections
        for (size_t i = 0; i < pp.size(); i++)
            if (lv_of[i] >= 0) { lv_off[i] = lv_total; lv_total += hbytes[size_t(lv_of[i])]; }
        o_lv = take(cur, lv_total);
        for (size_t i = 0; i < pp.size(); i++)
            if (lv_of[i] >= 0) hs[size_t(lv_of[i])].out_off = o_lv + lv_off[i];
    };
    auto hybrid_write = [&](uint8_t* out) -> int {
        if (hs.empty()) return PF_OK;
        ha.out = out;
        HIPCHK(ctx, hipMemcpyAsync(A + o_hstr, hs.data(), sizeof(HybridStream) * hs.size(), hipMemcpyHostToDevice, st));
        enc_hybrid_write(ha, st);
        return PF_OK;
    };
    // Statistics: the kernels run with the page kernels (their time is in encode_ms), the results come back in
    // pinned memory with the synchronisation the bodies wait for anyway.
    const size_t st_bytes = sizeof(StatPart) * n_se + (str ? size_t(ST_LIMIT) * n_se : 0);
    std::vector<uint32_t> px_in;   // rows of every page, then its present values (alive until the synchronisation: the upload reads it)
    auto stats_launch = [&]() -> int {
        if (!run_stats) return PF_OK;
        StatArgs sa{};
        sa.tiles = reinterpret_cast<const StatTile*>(A + o_stt); sa.ptile = reinterpret_cast<const uint32_t*>(A + o_stp);
        sa.n_tiles = uint32_t(stiles.size()); sa.n_pages = uint32_t(pp.size());
        sa.part = reinterpret_cast<StatPart*>(A + o_spart); sa.win = reinterpret_cast<uint32_t*>(A + o_swin);
        sa.out = reinterpret_cast<StatPart*>(A + o_sout); sa.bytes = A + o_sbytes;
        if (!stiles.empty())
            HIPCHK(ctx, hipMemcpyAsync(A + o_stt, stiles.data(), sizeof(StatTile) * stiles.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(A + o_stp, sptile.data(), 4 * sptile.size(), hipMemcpyHostToDevice, st));
        enc_stats(ea, sa, st);
        HIPCHK(ctx, hipGetLastError());
        if (want_index) {
            px_in.resize(2 * n_px);
            for (size_t i = 0; i < n_px; i++) { px_in[i] = uint32_t(pp[i].r1 - pp[i].r0); px_in[n_px + i] = pp[i].cnt; }
            HIPCHK(ctx, hipMemcpyAsync(A + o_xin, px_in.data(), 8 * n_px, hipMemcpyHostToDevice, st));
            PgIndexArgs xa{};
            xa.pages = sa.out;
            xa.rows = reinterpret_cast<const uint32_t*>(A + o_xin); xa.cnt = xa.rows + n_px;
            xa.n_pages = uint32_t(n_px); xa.trunc = px_trunc; xa.value_cap = uint32_t(px_cap);
            xa.nn = reinterpret_cast<uint32_t*>(A + o_xnn);
            xa.head = reinterpret_cast<PgIndexHead*>(A + o_xout);
            xa.null_counts = reinterpret_cast<long long*>(A + o_xout + px_nc);
            xa.off = reinterpret_cast<uint32_t*>(A + o_xout + px_off);
            xa.null_pages = A + o_xout + px_np;
            xa.values = A + o_xout + px_val;
            enc_pgindex(ea, xa, st);
            HIPCHK(ctx, hipGetLastError());
        }
        return PF_OK;
    };
    auto stats_fetch = [&]() -> int {
        if (want_index) {   // one block, in pinned memory, under the synchronisation the bodies wait for
            HIPCHK(ctx, ctx->h_enc_px.ensure(px_bytes));
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_enc_px.p, A + o_xout, px_bytes, hipMemcpyDeviceToHost, st));
        }
        if (!want_stats) return PF_OK;
        HIPCHK(ctx, ctx->h_enc_st.ensure(st_bytes));
        uint8_t* h = static_cast<uint8_t*>(ctx->h_enc_st.p);
        HIPCHK(ctx, hipMemcpyAsync(h, A + o_sout, sizeof(StatPart) * n_se, hipMemcpyDeviceToHost, st));
        if (str) HIPCHK(ctx, hipMemcpyAsync(h + sizeof(StatPart) * n_se, A + o_sbytes, size_t(ST_LIMIT) * n_se, hipMemcpyDeviceToHost, st));
        return PF_OK;
    };
    // Bloom filter (bloom_bytes): zeroed and filled on the stream behind the page kernels, outside encode_ms (events of
    // its own); the bitset comes back in pinned memory with the copy and synchronisation the bodies wait for anyway.
    auto bloom_launch = [&]() -> int {
        if (!bloom) return PF_OK;
        HIPCHK(ctx, ctx->h_enc_bloom.ensure(bloom));
        EVREC(ctx, ctx->ev_bloom[0], st);
        HIPCHK(ctx, hipMemsetAsync(A + o_bloom, 0, bloom, st));
        enc_bloom(ea, m, reinterpret_cast<uint32_t*>(A + o_bloom), uint32_t(bloom), dict && ctx->opts.bloom_first, st);
        HIPCHK(ctx, hipGetLastError());
        EVREC(ctx, ctx->ev_bloom[1], st);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_enc_bloom.p, A + o_bloom, bloom, hipMemcpyDeviceToHost, st));
        return PF_OK;
    };
    if (hyb && delta) {
        const int rc = hybrid_sizes();
        if (rc) return rc;
    }
    if (delta) {
        // size pass -> scan -> page totals (one D2H, one sync) -> sections -> write pass
        DeltaArgs da{};
        da.streams = reinterpret_cast<const DeltaStream*>(A + o_dstr);
        da.pages = reinterpret_cast<const DeltaPage*>(A + o_dpg);
        da.n_streams = uint32_t(dstreams.size() - 1); da.n_pages = uint32_t(dpages.size()); da.n_items = n_items;
        da.bytes = reinterpret_cast<uint32_t*>(A + o_dby); da.off = reinterpret_cast<uint32_t*>(A + o_dof);
        da.minv = reinterpret_cast<long long*>(A + o_dmin); da.widths = reinterpret_cast<uint32_t*>(A + o_dwd);
        da.totals = reinterpret_cast<uint32_t*>(A + o_dtot);
        if (str) {
            da.pfx = reinterpret_cast<uint32_t*>(A + o_pfx); da.sfx = reinterpret_cast<uint32_t*>(A + o_sfx);
            da.spre = reinterpret_cast<uint32_t*>(A + o_spre);
        }
        for (size_t s = 0; s + 1 < dstreams.size(); s++) {
            const DeltaPage& p = dpages[dstreams[s].page];
            dstreams[s].src = !str ? ea.dense + uint64_t(p.d0) * uint32_t(w)
                                   : reinterpret_cast<const uint8_t*>((s - p.s0 == 0 ? da.pfx : da.sfx) + p.d0);
        }
        EVREC(ctx, ctx->ev[4], st);
        HIPCHK(ctx, hipMemcpyAsync(A + o_dstr, dstreams.data(), sizeof(DeltaStream) * dstreams.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(A + o_dpg, dpages.data(), sizeof(DeltaPage) * dpages.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(da.bytes + n_items, 0, 4, st));
        if (str) HIPCHK(ctx, enc_delta_prefix(ea, da, m, temp, temp_bytes, st));
        HIPCHK(ctx, enc_delta_sizes(da, temp, temp_bytes, st));
        std::vector<uint32_t> htot(dpages.size());
        HIPCHK(ctx, hipMemcpyAsync(htot.data(), da.totals, 4 * htot.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (size_t i = 0; i < dpages.size(); i++) {
            if (htot[i] > 0x7fffffffu) return fail(ctx, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
            dpages[i].out_off = take(vo, htot[i]);
            sections.push_back({dpages[i].out_off, htot[i]});
        }
        if (hyb) place_levels(vo);
        HIPCHK(ctx, ctx->d_enc_sec.ensure(vo));
        da.out = static_cast<uint8_t*>(ctx->d_enc_sec.p);
        HIPCHK(ctx, hipMemcpyAsync(A + o_dpg, dpages.data(), sizeof(DeltaPage) * dpages.size(), hipMemcpyHostToDevice, st));
        enc_delta_write(ea, da, m, st);
        if (hyb) {
            const int rc = hybrid_write(da.out);
            if (rc) return rc;
        }
        HIPCHK(ctx, hipGetLastError());
        if (const int rc = stats_launch()) return rc;
        EVREC(ctx, ctx->ev[5], st);
        if (const int rc = stats_fetch()) return rc;
        if (const int rc = bloom_launch()) return rc;
    }
    uint8_t* SEC = static_cast<uint8_t*>(ctx->d_enc_sec.p);
    if (!delta) {   // RLE_DICTIONARY or PLAIN: the host knows every page's size (hybrid runs: after their size pass)
        if (hyb) {
            // The dictionary page and the ids are written before the size pass: room for the worst case of
            // every section (an element is at most a 5-byte varint and the value, or a header and a group)
            auto worst = [](uint64_t cnt, uint32_t b) { return (cnt / 8 + 1) * std::max<uint64_t>(b + 1, 5 + (b + 7) / 8); };
            size_t ub = vo + 512 + sizeof(EncPage) * pp.size();
            for (const PagePlanE& p : pp)
                ub += 256 + size_t(dict ? 1 + worst(p.cnt, bw) : brle ? 4 + worst(p.cnt, 1) : p.plain) +
                      size_t(col->max_def == 1 ? worst(uint64_t(p.r1 - p.r0), 1) : 0);
            HIPCHK(ctx, ctx->d_enc_sec.ensure(ub));
            ea.dict_out = static_cast<uint8_t*>(ctx->d_enc_sec.p) + o_dict;
            const int rc = hybrid_sizes();
            if (rc) return rc;
        }
        for (size_t i = 0; i < pp.size(); i++) {
            const PagePlanE& p = pp[i];
            uint64_t bytes;
            if (vs_of[i] >= 0) {   // width byte or 4-byte length, then the stream
                const uint64_t pre = dict ? 1 : 4;
                bytes = pre + hbytes[size_t(vs_of[i])];
                ep[i] = EncPage{0, p.d0, p.cnt, dict ? 1u : 0u, bw};
                ep[i].out_off = take(vo, bytes);
                hs[size_t(vs_of[i])].out_off = ep[i].out_off + pre;
                sections.push_back({ep[i].out_off, bytes});
                continue;
            }
            if (dict) {
                const uint64_t groups = (p.cnt + 7) / 8;
                bytes = p.cnt ? 1 + uvarint_len((groups << 1) | 1) + groups * bw : 1;
            } else {
                bytes = p.plain;
            }
            ep[i] = EncPage{0, p.d0, p.cnt, dict ? 1u : 0u, bw};
            ep[i].out_off = take(vo, bytes);
            sections.push_back({ep[i].out_off, bytes});
        }
        if (hyb) place_levels(vo);
        const size_t o_pages = take(vo, sizeof(EncPage) * ep.size());
        HIPCHK(ctx, ctx->d_enc_sec.ensure(vo));   // hybrid runs: within the worst case reserved above, nothing moves
        SEC = static_cast<uint8_t*>(ctx->d_enc_sec.p);
        ea.dict_out = SEC + o_dict;
        ea.vals_out = SEC;
        EVREC(ctx, ctx->ev[4], st);
        if (dict && !hyb) enc_dictionary_page_and_ids(ea, m, st);
        HIPCHK(ctx, hipMemcpyAsync(SEC + o_pages, ep.data(), sizeof(EncPage) * ep.size(), hipMemcpyHostToDevice, st));
        if (!(hyb && (dict || brle))) enc_pages(ea, reinterpret_cast<const EncPage*>(SEC + o_pages), int(ep.size()), st);
        if (hyb) {
            const int rc = hybrid_write(SEC);
            if (rc) return rc;
        }
        HIPCHK(ctx, hipGetLastError());
        if (const int rc = stats_launch()) return rc;
        EVREC(ctx, ctx->ev[5], st);
        if (const int rc = stats_fetch()) return rc;
        if (const int rc = bloom_launch()) return rc;
    }
    std::vector<std::vector<uint8_t>> bodies;
    std::vector<uint8_t> hlv(lv_total);   // hybrid runs: the pages' levels
    float snap_ms = 0.f, crc_ms = 0.f;
    // Page CRCs (PF_ENCODE_PAGE_CRC): the pieces of the pages that lie in device memory -- the compression jobs'
    // slots (SNAPPY, ZSTD; compress_sections lists them) or the sections themselves, and the levels: the stream the GPU
    // encoded (hybrid runs), or the whole validity bytes of the page's rows, which the one bit-packed run repeats
    // -- go through k_enc_crc; `crcs` holds the jobs (SNAPPY, ZSTD) or sections first, then the levels.
    std::vector<CrcPiece> lv_pieces;
    std::vector<CrcOut> crcs;
    std::vector<int> lv_piece(pp.size(), -1);   // the page's whole level stream
    std::vector<int> vb_piece(pp.size(), -1);   // the whole bytes of its bit-packed run, between header and last partial byte
    if (want_crc)
        for (size_t i = 0; i < pp.size(); i++) {
            if (lv_of[i] >= 0) {
                const uint32_t nb = hbytes[size_t(lv_of[i])];
                lv_piece[i] = int(lv_pieces.size());
                lv_pieces.push_back(CrcPiece{SEC + o_lv + lv_off[i], nullptr, nb, nb});
            } else if (has_val && pp[i].r1 - pp[i].r0 >= 8) {   // (pages start on a validity byte)
                const uint32_t nb = uint32_t((pp[i].r1 - pp[i].r0) / 8);
                vb_piece[i] = int(lv_pieces.size());
                lv_pieces.push_back(CrcPiece{ea.validity + pp[i].r0 / 8, nullptr, nb, nb});
            }
        }
    size_t crc_first_lv = 0;   // index of the first level stream in crcs
    if (compressed) {
        if (lv_total) HIPCHK(ctx, hipMemcpyAsync(hlv.data(), SEC + o_lv, lv_total, hipMemcpyDeviceToHost, st));
        const int rc = compress_sections(ctx, SEC, sections, bodies, col->codec, &snap_ms, &lv_pieces, want_crc ? &crcs : nullptr, &crc_ms);
        if (rc) return rc;
        if (want_crc) crc_first_lv = crcs.size() - lv_pieces.size();
    } else {
        std::vector<CrcPiece> pieces;   // (alive until the synchronisation below: the upload reads it)
        if (want_crc) {   // the table and the results in d_enc_out, which an uncompressed chunk does not use otherwise
            for (const auto& sct : sections) {
                if (sct.second > 0xffffffffull) return fail(ctx, PF_ERR_INVALID_ARG, "encode: data page over 2 GiB");
                pieces.push_back(CrcPiece{SEC + sct.first, nullptr, uint32_t(sct.second), uint32_t(sct.second)});
            }
            crc_first_lv = pieces.size();
            pieces.insert(pieces.end(), lv_pieces.begin(), lv_pieces.end());
            const size_t npc = pieces.size(), o_res = align_up(sizeof(CrcPiece) * npc, 256);
            HIPCHK(ctx, ctx->d_enc_out.ensure(o_res + sizeof(CrcOut) * npc));
            uint8_t* d = static_cast<uint8_t*>(ctx->d_enc_out.p);
            crcs.resize(npc);
            HIPCHK(ctx, hipMemcpyAsync(d, pieces.data(), sizeof(CrcPiece) * npc, hipMemcpyHostToDevice, st));
            EVREC(ctx, ctx->ev[8], st);
            launch_enc_crc(reinterpret_cast<const CrcPiece*>(d), int(npc), reinterpret_cast<CrcOut*>(d + o_res), st);
            HIPCHK(ctx, hipGetLastError());
            EVREC(ctx, ctx->ev[9], st);
            HIPCHK(ctx, hipMemcpyAsync(crcs.data(), d + o_res, sizeof(CrcOut) * npc, hipMemcpyDeviceToHost, st));
        }
        std::vector<uint8_t> all(vo);
        HIPCHK(ctx, hipMemcpyAsync(all.data(), SEC, vo, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (want_crc && ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&crc_ms, ctx->ev[8], ctx->ev[9]));
        if (lv_total) std::memcpy(hlv.data(), all.data() + o_lv, lv_total);
        for (const auto& sct : sections) bodies.emplace_back(all.begin() + sct.first, all.begin() + sct.first + sct.second);
    }

    // ---- page headers + bodies ----
    std::vector<uint8_t>& o = ctx->h_enc;
    o.clear();
    int64_t unc = 0;
    size_t bi = 0;
    // CRC of a page: its pieces folded in stored order (pf_crc.h); the bytes the host generates itself (the
    // length varint or the frame header, a bit-packed level run built from hval) are fed bytewise.
    size_t crc_job = 0;   // SNAPPY, ZSTD: the next job in crcs
    bool crc_bad = false;
    auto page_crc = [&](size_t sec, size_t page, const std::vector<uint8_t>& def) {
        uint32_t raw = 0;
        uint64_t len = 0;
        auto piece = [&](const CrcOut& c) { raw = crc_combine_pow(raw, c.raw, c.x8len); len += c.len; };
        if (page != size_t(-1) && lv_piece[page] >= 0) {
            piece(crcs[crc_first_lv + size_t(lv_piece[page])]);
        } else if (page != size_t(-1) && vb_piece[page] >= 0) {   // run header ‖ whole validity bytes (device) ‖ last partial byte
            const CrcOut& c = crcs[crc_first_lv + size_t(vb_piece[page])];
            const size_t groups = size_t(pp[page].r1 - pp[page].r0 + 7) / 8, hdr = def.size() - groups;
            raw = crc_raw_bytes(raw, def.data(), hdr);
            len += hdr;
            piece(c);
            raw = crc_raw_bytes(raw, def.data() + hdr + c.len, def.size() - hdr - c.len);
            len += def.size() - hdr - c.len;
        } else {
            raw = crc_raw_bytes(raw, def.data(), def.size());
            len += def.size();
        }
        if (compressed) {
            uint8_t head[12];
            const size_t vl = stream_head(col->codec, sections[sec].second, head);
            raw = crc_raw_bytes(raw, bodies[sec].data(), vl);
            len += vl;
            const uint32_t job = col->codec == PF_CODEC_ZSTD ? ZC_BLOCK : SC_BLOCK;
            for (uint64_t o = 0; o < sections[sec].second; o += job) piece(crcs[crc_job++]);
        } else {
            piece(crcs[sec]);
        }
        if (len != def.size() + bodies[sec].size()) crc_bad = true;   // the pieces are not the page
        return crc_finish(raw, len);
    };
    // Statistics of entry e (a page, or pp.size(): the chunk) from the kernels' results
    const StatPart* hst = want_stats ? static_cast<const StatPart*>(ctx->h_enc_st.p) : nullptr;
    const uint8_t* hsb = want_stats ? static_cast<const uint8_t*>(ctx->h_enc_st.p) + sizeof(StatPart) * n_se : nullptr;
    auto stats_of = [&](size_t e, int64_t nulls) {
        StatsOut so;
        if (!want_stats || hst[e].any == 2) return so;   // over the size limit: no struct at all
        so.present = true;
        so.null_count = nulls;
        if (hst[e].any != 1) return so;
        so.has_min_max = true;
        if (str) {
            const char* b = reinterpret_cast<const char*>(hsb + e * size_t(ST_LIMIT));
            so.min.assign(b, hst[e].mnl);
            so.max.assign(b + hst[e].mnl, hst[e].mxl);
        } else {   // PLAIN: little-endian, w bytes (BOOLEAN: one byte)
            so.min.assign(reinterpret_cast<const char*>(&hst[e].mn), size_t(w));
            so.max.assign(reinterpret_cast<const char*>(&hst[e].mx), size_t(w));
        }
        so.legacy = !str || so.min == so.max;   // parquet-mr: the legacy fields only where the signed order is the type's
        return so;
    };
    out->dictionary_page_offset = -1;
    if (dict) {
        PageHeaderOut h;
        h.page_type = PF_PAGE_DICTIONARY;
        h.uncompressed_size = int32_t(dict_bytes);
        h.compressed_size = int32_t(bodies[0].size());
        h.num_values = int32_t(D);
        h.encoding = PF_ENC_PLAIN;   // parquet-mr PARQUET_2_0: dictionary page PLAIN, data pages RLE_DICTIONARY
        if (want_crc) { h.has_crc = true; h.crc = page_crc(0, size_t(-1), {}); }
        out->dictionary_page_offset = 0;
        const size_t h0 = o.size();
        write_page_header(o, h);
        unc += int64_t(o.size() - h0) + dict_bytes;
        o.insert(o.end(), bodies[0].begin(), bodies[0].end());
        bi = 1;
    }
    out->data_page_offset = int64_t(o.size());
    ctx->h_enc_pgoff.assign(n_px, 0);
    ctx->h_enc_pgrow.assign(n_px, 0);
    ctx->h_enc_pgsize.assign(n_px, 0);
    for (size_t i = 0; i < pp.size(); i++, bi++) {
        const PagePlanE& p = pp[i];
        const int64_t rows = p.r1 - p.r0;
        std::vector<uint8_t> def;
        if (lv_of[i] >= 0) {       // hybrid runs: the stream the GPU encoded from the validity bits
            def.assign(hlv.begin() + lv_off[i], hlv.begin() + lv_off[i] + hbytes[size_t(lv_of[i])]);
        } else if (col->max_def == 1) {   // RLE/bit-packed hybrid, bit width 1: one bit-packed run = the validity bits
            const uint64_t groups = uint64_t(rows + 7) / 8;
            put_uvarint(def, (groups << 1) | 1);
            for (uint64_t g = 0; g < groups; g++) {
                uint8_t b = has_val ? hval[size_t(p.r0 / 8 + g)] : 0xff;
                const int64_t left = rows - int64_t(g) * 8;
                if (left < 8) b &= uint8_t((1u << left) - 1u);
                def.push_back(b);
            }
            if (rows == 0) def.clear();
        }
        PageHeaderOut h;
        h.page_type = PF_PAGE_DATA_V2;
        h.uncompressed_size = int32_t(def.size() + sections[bi].second);
        h.compressed_size = int32_t(def.size() + bodies[bi].size());
        h.num_values = int32_t(rows);
        h.num_nulls = int32_t(rows - p.cnt);
        h.num_rows = int32_t(rows);
        h.encoding = data_enc;
        h.def_bytes = int32_t(def.size());
        h.is_compressed = compressed;
        if (want_crc) { h.has_crc = true; h.crc = page_crc(bi, i, def); }
        h.stats = stats_of(i, rows - p.cnt);
        const size_t h0 = o.size();
        write_page_header(o, h);
        unc += int64_t(o.size() - h0) + h.uncompressed_size;
        o.insert(o.end(), def.begin(), def.end());
        o.insert(o.end(), bodies[bi].begin(), bodies[bi].end());
        if (want_index) {   // the OffsetIndex entry: the host knows where it put the page
            ctx->h_enc_pgoff[i] = int64_t(h0);
            ctx->h_enc_pgsize[i] = int32_t(o.size() - h0);
            ctx->h_enc_pgrow[i] = p.r0;
        }
    }
    if (crc_bad) return fail(ctx, PF_ERR_HIP, "encode: the CRC pieces of a page do not add up to its size");
    out->stats_flags = 0;
    out->stat_min_len = out->stat_max_len = 0;
    out->null_count = 0;
    out->stat_min = out->stat_max = nullptr;
    if (want_stats) {
        const StatsOut so = stats_of(pp.size(), n - int64_t(m));
        std::vector<uint8_t>& hb = ctx->h_enc_stat;
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
    out->bytes = o.data();
    out->size = int64_t(o.size());
    out->total_uncompressed_size = unc;
    out->num_values = n;
    out->n_data_pages = int32_t(pp.size());
    out->dict_entries = int32_t(D);
    out->data_encoding = data_enc;
    out->fallback = fallback;
    out->codec = col->codec;
    if (ctx->timing) {   // the page kernels' events have completed (the stream was synchronised since)
        float pg_ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&pg_ms, ctx->ev[4], ctx->ev[5]));
        enc_ms += pg_ms + crc_ms;
    }
    out->snappy_ms = snap_ms;
    out->encode_ms = enc_ms;
    out->bloom = bloom ? static_cast<const uint8_t*>(ctx->h_enc_bloom.p) : nullptr;
    out->bloom_len = int32_t(bloom);
    out->bloom_ms = 0.f;
    if (bloom && ctx->timing) HIPCHK(ctx, hipEventElapsedTime(&out->bloom_ms, ctx->ev_bloom[0], ctx->ev_bloom[1]));
    out->index_pages = 0;
    out->page_offset = nullptr; out->page_size = nullptr; out->page_first_row = nullptr;
    out->column_index = 0; out->boundary_order = 0;
    out->index_null_pages = nullptr; out->index_null_counts = nullptr;
    out->index_values = nullptr; out->index_value_off = nullptr;
    if (want_index) {
        const uint8_t* h = static_cast<const uint8_t*>(ctx->h_enc_px.p);
        const PgIndexHead* hd = reinterpret_cast<const PgIndexHead*>(h);
        if (hd->value_bytes > px_cap && hd->valid) return fail(ctx, PF_ERR_HIP, "encode: the page index values exceed their block");
        out->index_pages = int32_t(n_px);
        out->page_offset = ctx->h_enc_pgoff.data();
        out->page_size = ctx->h_enc_pgsize.data();
        out->page_first_row = ctx->h_enc_pgrow.data();
        out->column_index = hd->valid ? 1 : 0;
        out->boundary_order = hd->valid ? int32_t(hd->order) : 0;
        out->index_null_pages = h + px_np;
        out->index_null_counts = reinterpret_cast<const int64_t*>(h + px_nc);
        if (hd->valid) {
            out->index_values = h + px_val;
            out->index_value_off = reinterpret_cast<const uint32_t*>(h + px_off);
        }
    }
    out->snappy_in = 0;
    out->snappy_out = 0;
    if (compressed)
        for (size_t i = 0; i < sections.size(); i++) {
            out->snappy_in += int64_t(sections[i].second);
            out->snappy_out += int64_t(bodies[i].size());
        }
    return PF_OK;
}

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
// The filter stage's buffer for the planned batch: sized from the host's row counts, its tables uploaded.
int bind_filter(pf_ctx* ctx) {
    const BatchPlan& p = ctx->plan;
    const FilterPlan& f = ctx->filt;
    const size_t nc = size_t(ctx->n_chunks), np = f.preds.size();
    std::vector<int32_t> win_of(nc, -1);
    for (size_t i = 0; i < ctx->wins.size(); i++) win_of[size_t(ctx->wins[i].chunk)] = int32_t(i);
    // rows_in is the first predicate chunk's row count after its window: at most take rows, or the chunk's entries
    // (a predicate chunk is flat: rows = entries)
    const int c0 = f.preds[0].chunk;
    int64_t rows_cap = p.chunks[size_t(c0)].num_entries;
    if (win_of[size_t(c0)] >= 0 && ctx->wins[size_t(win_of[size_t(c0)])].take >= 0)
        rows_cap = std::min<int64_t>(rows_cap, ctx->wins[size_t(win_of[size_t(c0)])].take);
    rows_cap = std::max<int64_t>(rows_cap, 0);
    const size_t tiles = std::max<size_t>(1, (size_t(rows_cap) + SEL_TILE - 1) / SEL_TILE);
    size_t m = 0;
    auto take = [&](size_t n) { const size_t o = align_up(m, 256); m = o + n; return o; };
    const size_t o_head = take(sizeof(DevSelHead)), o_sc = take(sizeof(DevSelChunk) * nc);
    const size_t o_up = take(0), o_preds = take(sizeof(DevPred) * np), o_blob = take(f.blob.size()), o_winof = take(4 * nc);
    const size_t up_end = m;
    const size_t o_mask = take(8 * tiles * (SEL_TILE / 64)), o_tc = take(4 * tiles), o_tb = take(4 * tiles);
    const size_t o_rows = take(4 * tiles * SEL_TILE), o_bs = take(4 * tiles * nc), o_bb = take(4 * tiles * nc), o_bt = take(8 * nc);
    HIPCHK(ctx, ctx->d_sel.ensure(m));
    HIPCHK(ctx, ctx->h_sel.ensure(up_end));
    uint8_t* h = static_cast<uint8_t*>(ctx->h_sel.p);
    uint8_t* d = static_cast<uint8_t*>(ctx->d_sel.p);
    std::memset(h, 0, up_end);
    std::memcpy(h + o_preds, f.preds.data(), sizeof(DevPred) * np);
    if (!f.blob.empty()) std::memcpy(h + o_blob, f.blob.data(), f.blob.size());
    std::memcpy(h + o_winof, win_of.data(), 4 * nc);
    HIPCHK(ctx, hipMemcpyAsync(d + o_up, h + o_up, up_end - o_up, hipMemcpyHostToDevice, ctx->stream));
    SelBufs& s = ctx->sel;
    s.head = reinterpret_cast<DevSelHead*>(d + o_head);
    s.sc = reinterpret_cast<DevSelChunk*>(d + o_sc);
    s.preds = reinterpret_cast<const DevPred*>(d + o_preds);
    s.blob = d + o_blob;
    s.win_of = reinterpret_cast<const int32_t*>(d + o_winof);
    s.mask = reinterpret_cast<uint64_t*>(d + o_mask);
    s.tile_count = reinterpret_cast<uint32_t*>(d + o_tc);
    s.tile_base = reinterpret_cast<uint32_t*>(d + o_tb);
    s.rows = reinterpret_cast<int32_t*>(d + o_rows);
    s.ba_sum = reinterpret_cast<uint32_t*>(d + o_bs);
    s.ba_base = reinterpret_cast<uint32_t*>(d + o_bb);
    s.ba_total = reinterpret_cast<int64_t*>(d + o_bt);
    s.rows_cap = rows_cap;
    s.tiles_cap = int64_t(tiles);
    s.n_preds = int32_t(np);
    ctx->sel_up_off = o_up;
    ctx->sel_grid = int(std::min<size_t>(tiles, 256));
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
    plan_batch(cds, n_chunks, n_bytes, ctx->opts, p);
    mark();
    // ---- arenas ----
    const size_t chars_cap = std::max<size_t>(size_t(2 * p.chars_hint) + (16u << 20), ctx->chars_need);
    // (the window kernels read validity bits in 8-byte words: room for the last one)
    const size_t bits_cap = std::max<size_t>(p.bits_bytes, 1) + (twins ? 8 : 0);
    if (ctx->copies_pending) {
        if (p.out_bytes > ctx->d_out.cap || bits_cap > ctx->d_bits.cap || chars_cap > ctx->d_chars.cap ||
            (twins && (ctx->d_out.cap > ctx->d_wout.cap || ctx->d_bits.cap > ctx->d_wbits.cap || ctx->d_chars.cap > ctx->d_wchars.cap)))
            HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));   // a growing output arena must not be freed under a pending D2H copy
        else
            HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_copy, 0));   // (a download on the copy stream reads the arenas)
    }
    ctx->copies_pending = false;
    HIPCHK(ctx, ctx->d_scratch.ensure(std::max<size_t>(p.scratch_bytes, 1)));
    HIPCHK(ctx, ctx->d_out.ensure(std::max<size_t>(p.out_bytes, 1)));
    HIPCHK(ctx, ctx->d_bits.ensure(bits_cap));
    HIPCHK(ctx, ctx->d_chars.ensure(chars_cap));
    if (twins) {   // the twins: the decode arenas' sizes, so a chunk keeps its offsets
        HIPCHK(ctx, ctx->d_wout.ensure(ctx->d_out.cap));
        HIPCHK(ctx, ctx->d_wbits.ensure(ctx->d_bits.cap));
        HIPCHK(ctx, ctx->d_wchars.ensure(ctx->d_chars.cap));
    }
    if (windowed) {
        const int nw = int(ctx->wins.size());
        const size_t tab = align_up(sizeof(DevWin) * nw, 256) + sizeof(DevWinRes) * nw;
        HIPCHK(ctx, ctx->d_win.ensure(tab));
        HIPCHK(ctx, ctx->h_win.ensure(tab));
        std::memcpy(ctx->h_win.p, ctx->wins.data(), sizeof(DevWin) * nw);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_win.p, ctx->h_win.p, sizeof(DevWin) * nw, hipMemcpyHostToDevice, st));
        uint64_t tiles = 1;   // k_win_copy's workgroups per chunk stride over its tiles: a bound from the host's counts
        for (const DevWin& w : ctx->wins) {
            const DevChunk& ck = p.chunks[size_t(w.chunk)];
            const uint64_t n = ck.max_rep == 0 && w.take >= 0 ? uint64_t(w.take) : uint64_t(ck.num_entries);
            tiles = std::max<uint64_t>(tiles, n * uint64_t(std::max(ck.width, 8)) / WIN_TILE + 8);
        }
        ctx->win_grid = int(std::min<uint64_t>(tiles, 512));
    }
    if (ctx->filtered()) {
        const int rc = bind_filter(ctx);
        if (rc) return rc;
    }
    HIPCHK(ctx, ctx->d_tokmap.ensure(p.snap.tokmap_bytes));
    HIPCHK(ctx, ctx->d_meta.ensure(p.meta_bytes));
    HIPCHK(ctx, ctx->h_meta.ensure(p.meta_bytes));
    HIPCHK(ctx, ctx->h_res.ensure(align_up(sizeof(DevChunkResult) * n_chunks, 256) + sizeof(DevChunk) * n_chunks + 256));
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
                 int n_preds, const uint8_t* bytes, size_t n_bytes, int bytes_on_device) {
    if (!ctx) return fail(nullptr, PF_ERR_INVALID_ARG, "null ctx");
    if (n_chunks < 0 || (n_chunks > 0 && (!cds || !bytes))) return fail(ctx, PF_ERR_INVALID_ARG, "bad arguments");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "previous decode not waited for");
    for (int c = 0; windows && c < n_chunks; c++)
        if (windows[c].skip_rows < 0 || windows[c].take_rows < -1)
            return fail(ctx, PF_ERR_INVALID_ARG, "row window: negative skip_rows, or take_rows below -1");
    ctx->wins.clear();
    ctx->filt.preds.clear();
    ctx->filt.blob.clear();
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
        const DevChunkResult* r = static_cast<const DevChunkResult*>(ctx->h_res.p);
        const DevChunk* dc = reinterpret_cast<const DevChunk*>(static_cast<uint8_t*>(ctx->h_res.p) +
                                                               align_up(sizeof(DevChunkResult) * ctx->n_chunks, 256));
        // chars arena overflow: grow to the exact need and run the batch once more
        uint64_t need = 0;
        bool overflow = false;
        for (int c = 0; c < ctx->n_chunks; c++) {
            if (ctx->plan.chunks[c].ptype == PF_BYTE_ARRAY) need += align_up(uint64_t(std::max<int64_t>(r[c].num_chars, 0)), 256);
            if (r[c].status == PF_ERR_CAPACITY && ctx->plan.chunks[c].ptype == PF_BYTE_ARRAY && r[c].num_chars <= 0x7fffffff)
                overflow = true;
        }
        if (overflow && ctx->reruns == 0) {
            ctx->reruns++;
            ctx->chars_need = size_t(need) + (1u << 20);
            HIPCHK(ctx, ctx->d_chars.ensure(ctx->chars_need));
            if (ctx->twins()) HIPCHK(ctx, ctx->d_wchars.ensure(ctx->d_chars.cap));
            int rc = upload_meta(ctx);
            if (rc) { ctx->pending = false; return rc; }
            rc = enqueue_kernels(ctx);
            if (rc) { ctx->pending = false; return rc; }
            continue;
        }
        int first_err = PF_OK;
        size_t wi = 0;
        const DevWinRes* wr = ctx->wins.empty() ? nullptr : reinterpret_cast<const DevWinRes*>(
            static_cast<const uint8_t*>(ctx->h_win.p) + align_up(sizeof(DevWin) * ctx->wins.size(), 256));
        for (int c = 0; c < ctx->n_chunks; c++) {
            pf_column_info& ci = ctx->info[c];
            const DevChunk& ck = ctx->plan.chunks[c];
            ci.num_entries = ck.num_entries;
            ci.num_slots = r[c].num_slots;
            ci.num_values = r[c].num_values;
            ci.num_rows = r[c].num_rows;
            ci.num_chars = ck.ptype == PF_BYTE_ARRAY ? r[c].num_chars : 0;
            ci.width = ck.width;
            ci.status = r[c].status;
            ci.d_values = ck.values;
            ci.d_validity = ck.validity;
            ci.d_offsets = ck.offsets;
            ci.d_chars = dc[c].chars;
            ci.d_list_offsets = ck.list_offsets;
            ci.d_list_validity = ck.list_validity;
            ci.d_def_levels = ck.def_levels;
            ci.d_rep_levels = ck.rep_levels;
            if (wi < ctx->wins.size() && ctx->wins[wi].chunk == c) {   // the window's view (chunks ascend in wins)
                const DevWinRes& w = wr[wi++];
                if (ci.status == 0 && w.status != 0) ci.status = w.status;
                else if (ci.status == 0 && !w.identity) {
                    const ptrdiff_t od = static_cast<uint8_t*>(ctx->d_wout.p) - static_cast<uint8_t*>(ctx->d_out.p);
                    const ptrdiff_t bd = static_cast<uint8_t*>(ctx->d_wbits.p) - static_cast<uint8_t*>(ctx->d_bits.p);
                    auto tw = [](auto* q, ptrdiff_t d) { return q ? reinterpret_cast<decltype(q)>(reinterpret_cast<uint8_t*>(q) + d) : nullptr; };
                    ci.num_entries = w.n_entries;
                    ci.num_slots = w.n_slots;
                    ci.num_values = w.n_values;
                    ci.num_rows = w.n_rows;
                    ci.num_chars = ck.ptype == PF_BYTE_ARRAY ? w.n_chars : 0;
                    ci.d_values = tw(ck.values, od);
                    ci.d_validity = tw(ck.validity, bd);
                    ci.d_offsets = tw(ck.offsets, od);
                    ci.d_chars = w.chars_dst;
                    ci.d_list_offsets = tw(ck.list_offsets, od);
                    ci.d_list_validity = tw(ck.list_validity, bd);
                    ci.d_def_levels = tw(ck.def_levels, od);
                    ci.d_rep_levels = tw(ck.rep_levels, od);
                }
            }
            if (ctx->filtered()) {   // the selection's view
                const DevSelHead& sh = *static_cast<const DevSelHead*>(ctx->h_sel.p);
                const DevSelChunk& sc = reinterpret_cast<const DevSelChunk*>(static_cast<const uint8_t*>(ctx->h_sel.p) +
                                                                            align_up(sizeof(DevSelHead), 256))[c];
                if (ci.status == 0 && sc.status != 0) ci.status = sc.status;   // (its own, or a predicate chunk's)
                else if (ci.status == 0) {
                    ci.num_entries = ci.num_slots = ci.num_rows = sh.rows_selected;
                    ci.num_values = sc.n_values;
                    ci.num_chars = ck.ptype == PF_BYTE_ARRAY ? sc.n_chars : 0;
                    ci.d_values = sc.o_values;
                    ci.d_validity = sc.o_validity;
                    ci.d_offsets = sc.o_offsets;
                    ci.d_chars = sc.o_chars;
                }
                if (c == 0) {
                    ctx->sel_info = pf_selection_info{};
                    ctx->sel_info.rows_in = sh.rows_in;
                    ctx->sel_info.rows_selected = sh.rows_selected;
                    ctx->sel_info.d_rows = ctx->sel.rows;
                    ctx->sel_info.status = sh.status;
                }
            }
            if (ci.status != 0 && first_err == PF_OK) {
                first_err = ci.status;
                char buf[160];
                std::snprintf(buf, sizeof buf, "chunk %d: decode failed (status %d, page %d)", c, ci.status, r[c].err_page);
                fail(ctx, first_err, buf);
            }
        }
        ctx->pending = false;
        ctx->timing_valid = true;
        return first_err;
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
// Enqueue the D2H copies of chunk i's arrays on the context stream (no synchronisation).
int enqueue_copy(pf_ctx* ctx, int chunk, const pf_column_out* o) {
    if (!ctx || !o) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (chunk < 0 || chunk >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
    const pf_column_info& ci = ctx->info[chunk];
    if (ci.status != 0) return fail(ctx, ci.status, "chunk failed to decode");
    struct Item { void* dst; size_t cap; const void* src; size_t n; };
    Item items[8] = {
        {o->values, o->values_cap, ci.d_values, size_t(ci.num_slots) * size_t(ci.width)},
        {o->validity, o->validity_cap, ci.d_validity, size_t((ci.num_slots + 7) / 8)},
        {o->offsets, o->offsets_cap, ci.d_offsets, ci.d_offsets ? 4 * size_t(ci.num_slots + 1) : 0},
        {o->chars, o->chars_cap, ci.d_chars, size_t(ci.num_chars)},
        {o->list_offsets, o->list_offsets_cap, ci.d_list_offsets, ci.d_list_offsets ? 4 * size_t(ci.num_rows + 1) : 0},
        {o->list_validity, o->list_validity_cap, ci.d_list_validity, size_t((ci.num_rows + 7) / 8)},
        {o->def_levels, o->def_levels_cap, ci.d_def_levels, size_t(ci.num_entries)},
        {o->rep_levels, o->rep_levels_cap, ci.d_rep_levels, size_t(ci.num_entries)},
    };
    for (const Item& it : items)
        if (it.dst && it.src && it.n > it.cap) return fail(ctx, PF_ERR_CAPACITY, "output buffer too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (const Item& it : items)
        if (it.dst && it.src && it.n) HIPCHK(ctx, hipMemcpyAsync(it.dst, it.src, it.n, hipMemcpyDeviceToHost, ctx->stream));
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
        if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
        const int c = chunks[i];
        if (c < 0 || c >= ctx->n_chunks) return fail(ctx, PF_ERR_INVALID_ARG, "chunk index out of range");
        const pf_column_info& ci = ctx->info[c];
        if (ci.status != 0) return fail(ctx, ci.status, "chunk failed to decode");
        const pf_column_out& o = outs[i];
        const size_t need[8] = {size_t(ci.num_slots) * size_t(ci.width), size_t((ci.num_slots + 7) / 8),
                                ci.d_offsets ? 4 * size_t(ci.num_slots + 1) : 0, size_t(ci.num_chars),
                                ci.d_list_offsets ? 4 * size_t(ci.num_rows + 1) : 0, size_t((ci.num_rows + 7) / 8),
                                size_t(ci.num_entries), size_t(ci.num_entries)};
        const void* dst[8] = {o.values, o.validity, o.offsets, o.chars, o.list_offsets, o.list_validity, o.def_levels,
                              o.rep_levels};
        const void* src[8] = {ci.d_values, ci.d_validity, ci.d_offsets, ci.d_chars, ci.d_list_offsets, ci.d_list_validity,
                              ci.d_def_levels, ci.d_rep_levels};
        const size_t cap[8] = {o.values_cap, o.validity_cap, o.offsets_cap, o.chars_cap, o.list_offsets_cap,
                               o.list_validity_cap, o.def_levels_cap, o.rep_levels_cap};
        for (int k = 0; k < 8; k++)
            if (dst[k] && src[k] && need[k] > cap[k]) return fail(ctx, PF_ERR_CAPACITY, "output buffer too small");
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
// Host layout of pf_copy_batch_async: [out arena | bits arena | chars arena], each 256-B aligned.
struct BatchLayout { size_t out, bits_off, bits, chars_off, chars, total; };
BatchLayout batch_layout(const pf_ctx* ctx) {
    BatchLayout b{};
    b.out = ctx->plan.out_bytes;
    b.bits_off = align_up(b.out, 256);
    b.bits = ctx->plan.bits_bytes;
    b.chars_off = align_up(b.bits_off + b.bits, 256);
    const uint8_t* c0 = static_cast<const uint8_t*>(ctx->d_chars.p);
    size_t hi = 0, bound = 0;
    for (int c = 0; c < ctx->n_chunks && c < int(ctx->info.size()); c++) {
        const pf_column_info& ci = ctx->info[c];
        if (ci.d_chars && ci.num_chars > 0) {
            hi = std::max(hi, size_t(static_cast<const uint8_t*>(ci.d_chars) - c0) + size_t(ci.num_chars));
            bound += align_up(size_t(ci.num_chars), 256);
        }
    }
    b.chars = hi;   // bytes copied: the arena's used extent (depends on the order k_scan placed the chunks)
    // buffer size: an order-independent bound, so equal batches always need equal buffers
    b.total = b.chars_off + std::max(hi, bound);
    return b;
}
}  // namespace

int pf_batch_bytes(pf_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    *bytes = batch_layout(ctx).total;
    return PF_OK;
}

int pf_copy_batch_async(pf_ctx* ctx, void* host, size_t cap) {
    if (!ctx || (!host && cap)) return fail(ctx, PF_ERR_INVALID_ARG, "null arg");
    if (ctx->pending) return fail(ctx, PF_ERR_STATE, "call pf_wait first");
    if (!ctx->tables_from_decode) return fail(ctx, PF_ERR_STATE, "no finished decode");
    if (ctx->twins()) return fail(ctx, PF_ERR_STATE, "the last decode had row windows or a row filter: no batch copy");
    const BatchLayout b = batch_layout(ctx);
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
    const BatchLayout b = batch_layout(ctx);
    const uint8_t* h = static_cast<const uint8_t*>(host);
    auto rebase = [&](const void* p) -> const void* {
        if (!p) return nullptr;
        const uint8_t* q = static_cast<const uint8_t*>(p);
        const uint8_t* o = static_cast<const uint8_t*>(ctx->d_out.p);
        const uint8_t* v = static_cast<const uint8_t*>(ctx->d_bits.p);
        const uint8_t* c = static_cast<const uint8_t*>(ctx->d_chars.p);
        if (q >= o && q <= o + b.out) return h + (q - o);
        if (q >= v && q <= v + b.bits) return h + b.bits_off + (q - v);
        if (q >= c && q <= c + b.chars) return h + b.chars_off + (q - c);
        return nullptr;
    };
    pf_column_info ci = ctx->info[chunk];
    ci.d_values = rebase(ci.d_values);
    ci.d_validity = static_cast<const uint8_t*>(rebase(ci.d_validity));
    ci.d_offsets = static_cast<const int32_t*>(rebase(ci.d_offsets));
    ci.d_chars = static_cast<const uint8_t*>(rebase(ci.d_chars));
    ci.d_list_offsets = static_cast<const int32_t*>(rebase(ci.d_list_offsets));
    ci.d_list_validity = static_cast<const uint8_t*>(rebase(ci.d_list_validity));
    ci.d_def_levels = static_cast<const uint8_t*>(rebase(ci.d_def_levels));
    ci.d_rep_levels = static_cast<const uint8_t*>(rebase(ci.d_rep_levels));
    *out = ci;
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
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));   // arenas may be reallocated below
    ctx->copies_pending = false;
    ctx->n_chunks = 0;
    ctx->info.clear();
    ctx->tables_from_decode = false;   // d_meta now holds this call's layout
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
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));   // arenas may be reallocated below
    ctx->copies_pending = false;
    ctx->n_chunks = 0;
    ctx->info.clear();
    ctx->tables_from_decode = false;   // d_meta now holds this call's layout
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
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->copies_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_copy));
    ctx->copies_pending = false;
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
// DONE_NULL 4: which kernel took the page; k_page_null and k_flat_null both set DONE_NULL, and only
// k_page_null's pages keep no level table (lvl = 0 in out[2 * i + 1])).
extern "C" int pf_debug_page_done(pf_ctx* ctx, int* out, int n_pages) {
    std::vector<DevPage> pg;
    const int np = fetch_pages(ctx, out ? n_pages : 0, pg);
    if (np >= 0) {
        const int m = int(pg.size());
        for (int i = 0; i < m; i++) {
            out[2 * i] = pg[size_t(i)].done;
            uint32_t lt1 = 0;   // k_lvl's "block table fits" word (k_flat_null ran on the page)
            if (pg[size_t(i)].lvltab) HIPCHK(ctx, hipMemcpy(&lt1, pg[size_t(i)].lvltab + 1, 4, hipMemcpyDeviceToHost));
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
