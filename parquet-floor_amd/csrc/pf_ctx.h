// pf_ctx.h — the context behind include/pfloor.h, shared by the runtime's translation units
// (pf_runtime.hip: decode, scan, copies, life cycle; pf_enc_runtime.hip: the write path). Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "pf_launch.h"
#include "pf_plan.h"
#include "pf_result.h"
#include "pfloor.h"

namespace pf {

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

constexpr int N_EVENTS = 11;  // h2d, snappy parse, snappy exec, dict, delta, levels, count, scan, flat, decode

// Records `msg` as the context's (and the thread's) last error and returns `code`. Defined in pf_runtime.hip.
int fail(pf_ctx* ctx, int code, const std::string& msg);

}  // namespace pf

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
    hipEvent_t ev[pf::N_EVENTS] = {};
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
    pf::DevBuf d_in, d_scratch, d_out, d_bits, d_chars, d_meta, d_tokmap;
    pf::DevBuf d_scan_in, d_scan;          // pf_scan_pages: host chunk bytes, tables
    pf::DevBuf d_enc, d_enc_sec, d_enc_out;   // pf_encode_chunk / pf_snappy_compress: work arena, values sections, slots
    std::vector<uint8_t> h_enc;            // the last encoded chunk (headers + bodies)
    std::vector<uint8_t> h_enc_stat;       // its chunk statistics (min ‖ max)
    pf::HostBuf h_enc_st;                  // pf_encode_chunk: statistics results D2H
    pf::HostBuf h_enc_bloom;               // pf_encode_chunk: the Bloom filter's bitset D2H (pf_encoded_chunk.bloom)
    pf::HostBuf h_meta, h_res;
    pf::HostBuf h_enc_slots;               // pf_encode_chunk / pf_snappy_compress: compressed slots D2H
    // last batch
    int n_chunks = 0;
    bool pending = false;
    bool copies_pending = false;           // pf_copy_columns_async enqueued, not yet pf_sync'ed
    bool tables_from_decode = false;       // d_meta layout (off_fallback) belongs to a pf_decode_row_group
    bool timing_valid = false;
    pf::BatchPlan plan;                    // the last pf_decode_row_group's tables, lists and layout
    // diagnostics: tables of the last pf_snappy_decompress (pf_debug_snappy_tables)
    const uint32_t* d_last_splits = nullptr;
    const pf::SnapWin* d_last_win = nullptr;
    const uint32_t* d_last_lane_out = nullptr;
    std::vector<pf_column_info> info;
    // kept dictionaries (pf_decode_row_group_dict): the call's flags (empty: none), every chunk's pf_dict_info after
    // pf_wait, and the pinned mirror the DevKeep table comes down into
    std::vector<uint8_t> keep_flags;
    std::vector<pf_dict_info> dinfo;
    pf::HostBuf h_keep;
    bool meta_by_kernel = false;   // this batch's metadata went up by k_upload (which also zeroes bits / npub)
    uint64_t chars_need = 0;
    int reruns = 0;
    pf::HostBuf h_enc_px;                  // pf_encode_chunk: the page index block D2H (pf_encoded_chunk.index_*)
    std::vector<int64_t> h_enc_pgoff, h_enc_pgrow;   // pf_encoded_chunk.page_offset / page_first_row
    std::vector<int32_t> h_enc_pgsize;               // pf_encoded_chunk.page_size
    // row windows (pf_decode_row_group_rows): the chunks whose window is not {0, -1}, their tables, and the twin output
    // arenas k_win_copy writes (allocated only for a batch that has such a window)
    std::vector<pf::DevWin> wins;
    pf::DevBuf d_win, d_wout, d_wbits, d_wchars;
    pf::HostBuf h_win;                     // DevWin[n] up, DevWinRes[n] down
    int win_grid = 1;
    // this batch's side-table layouts (pf_result.h), each computed once in enqueue_batch and read by enqueue_kernels
    // and pf_wait; the twin deltas from where the arenas were bound
    pf::ResLayout res_lay{};
    pf::WinLayout win_lay{};
    pf::SelLayout sel_lay;
    pf::TwinDelta twin;
    hipEvent_t ev_win[2] = {};
    // row filter (pf_decode_row_group_filter): the packed predicates (none: no filter stage), the stage's device buffer
    // and its pinned mirror: [DevSelHead | DevSelChunk[n]] comes down, [DevPred[] | blob | win_of[n]] goes up
    pf::FilterPlan filt;
    pf::DevBuf d_sel;
    pf::HostBuf h_sel;
    pf::SelBufs sel{};
    pf::SelDictBufs sel_dict{};             // predicates on kept chunks (pf_decode_row_group_dict_filter), and the keep tables
    hipEvent_t ev_sel[2] = {};
    pf_selection_info sel_info{};
    bool filtered() const { return !filt.preds.empty(); }
    bool twins() const { return !wins.empty() || filtered(); }   // the batch's results are not (all) in the decode arenas
};

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return pf::fail(ctx, PF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// stage-timing event: only when the context has timing on (each record is a marker on the stream,
// ~7 us between kernels on MI355X, so the product path leaves them off)
#define EVREC(ctx, ev, st)                                 \
    do {                                                   \
        if ((ctx)->timing) HIPCHK(ctx, hipEventRecord(ev, st)); \
    } while (0)
