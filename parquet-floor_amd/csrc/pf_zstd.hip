// pf_zstd.hip — ZSTD page decompression on gfx950 (wave64), over the decode core of pf_zstd_core.h.
//
// Blocks of a frame depend on each other (repeat offsets, reused tables, output position), so one
// 256-thread workgroup takes a page and its blocks in order; workgroups stride over the jobs. Every
// decision that can refuse a page -- headers, tables, bit streams, sequence bounds -- is the core's,
// the same code the host model runs; the kernel adds only who does what:
//  * thread 0 reads the headers and builds the Huffman table while thread 64 (another wave) reads
//    the sequences header and builds the three FSE tables;
//  * the 1 or 4 Huffman streams are decoded by lanes 0..3 of wave 0 in lockstep (one instruction
//    stream, four bit readers) into this workgroup's literal area, while thread 64 decodes the first
//    batch of sequences;
//  * sequences are decoded ZB at a time into LDS with their literal and output positions (running
//    sums of the decoding thread, which has to walk them in order anyway);
//  * a batch's literal runs, and its matches whose source ends before the batch's first output
//    byte, are copied by 16 groups of 16 lanes at once; the matches that read the batch's own
//    output follow in sequence order, each by all 256 threads with a barrier after it.
// LDS: the core's Tables (16.3 KiB) + the batch (5 KiB) + control: under 22 KiB, 7 workgroups per
// CU by LDS. Output goes to the page's scratch body, where the Snappy kernels put theirs.
#include <hip/hip_runtime.h>

#include "pf_device.h"
#include "pf_launch.h"
#include "pf_zstd_core.h"

namespace pf {

using namespace zstd;

constexpr int ZT = 256;            // threads
constexpr uint32_t ZB = 256;       // sequences per batch
constexpr int ZSEQ_TID = WAVE;     // the thread that decodes sequences (lane 0 of wave 1)
constexpr uint32_t ZDEP = 1u << 31;

struct ZSeq {
    uint32_t out, lit, ll, ml, off;   // ml: ZDEP set = the match reads this batch's output
};

struct ZCtl {
    int err;
    uint32_t ip, op, f0;   // input / output position, first output byte of the frame
    uint32_t state;        // frame step: 0 a frame begins, 1 input used up, 2 a skippable frame
    uint32_t huf_used, nb;
    uint32_t tail_lit, tail_out, tail_n, block_out;
    FrameHdr fh;
    BlockHdr bh;
    LitHdr lh;
    LitStreams ls;
    SeqHdr sh;
};

// One compressed block at p (bh.size bytes) to dst + op. Every thread calls it; C.block_out holds
// what it produced, C.err is set when it is refused.
__device__ void zstd_block(const uint8_t* p, const BlockHdr& bh, uint8_t* dst, uint32_t op, uint32_t f0, uint32_t dst_len,
                           uint8_t* lit, Tables& T, ZCtl& C, ZSeq* sq) {
    const int tid = threadIdx.x;
    const uint32_t left = dst_len - op;
    if (tid == 0 && !lit_header(p, bh.size, left < Z_BLOCK_MAX ? left : Z_BLOCK_MAX, T.huf_ok != 0, C.lh)) C.err = 1;
    __syncthreads();
    const LitHdr lh = C.lh;
    int err = C.err;
    __syncthreads();
    if (err) return;

    // ---- tables: Huffman by thread 0, sequences by thread 64 ----
    SeqDec d{};
    if (tid == 0 && lh.type >= 2) {
        uint32_t used = 0;
        bool ok = true;
        if (lh.type == 2) {
            ok = huf_read(p + lh.hdr, lh.csize, T, used);
            if (ok) { T.huf_ok = 1; T.huf_pairs = huf_pairs_for(lh.regen, lh.csize); }
        }
        ok = ok && lit_streams(p + lh.hdr + used, lh.csize - used, lh, C.ls);
        C.huf_used = used;
        if (!ok) C.err = 1;
    }
    if (tid == ZSEQ_TID) {
        const uint8_t* sp = p + lh.total;
        const uint32_t sn = bh.size - lh.total;
        if (!seq_header(sp, sn, T, C.sh)) C.err = 1;
        else if (C.sh.nseq && !seq_init(d, T, sp + C.sh.bits_off, sn - C.sh.bits_off)) C.err = 1;
    }
    __syncthreads();
    err = C.err;
    const uint32_t nseq = C.sh.nseq, used = C.huf_used;
    __syncthreads();
    if (err) return;

    // ---- literal streams (lanes 0..3) beside the first batch of sequences (thread 64) ----
    if (lh.type >= 2 && tid < int(lh.streams)) {
        const uint32_t so = C.ls.off[tid], sl = C.ls.len[tid], oo = C.ls.out[tid], cnt = C.ls.cnt[tid];
        if (!huf_stream(T.huf, T.huf_log, p + lh.hdr + used + so, sl, so, C.ls.strict != 0, T.huf_pairs != 0, lit + oo, cnt)) C.err = 1;
    }
    uint32_t lp = 0, bo = 0, done = 0;   // thread 64: literals used, block output, sequences decoded
    auto decode_batch = [&]() {
        uint32_t nb = nseq - done < ZB ? nseq - done : ZB;
        const uint32_t batch_start = bo;
        bool ok = true;
        for (uint32_t i = 0; i < nb; i++) {
            Seq s;
            if (!seq_next(d, T, done + i + 1 == nseq, s) || !seq_check(s, lh.regen - lp, bo, op - f0, left - bo)) {
                ok = false;
                nb = i;
                break;
            }
            const uint32_t mo = bo + s.ll;
            const bool dep = uint64_t(mo) + s.ml > uint64_t(batch_start) + s.off;
            sq[i] = ZSeq{op + bo, lp, s.ll, s.ml | (dep ? ZDEP : 0u), s.off};
            lp += s.ll;
            bo += s.ll + s.ml;
        }
        done += nb;
        C.nb = nb;
        if (ok && done == nseq) {
            const uint32_t tail = lh.regen - lp;
            ok = tail_check(tail, bo, left - bo);
            C.tail_lit = lp; C.tail_out = op + bo; C.tail_n = tail; C.block_out = bo + tail;
        }
        if (!ok) C.err = 1;
    };
    if (tid == ZSEQ_TID) decode_batch();

    const uint8_t* lits = lh.type >= 2 ? lit : p + lh.hdr;
    const bool rle = lh.type == 1;
    const uint8_t rle_byte = rle ? p[lh.hdr] : uint8_t(0);
    const uint32_t g = uint32_t(tid) >> 4, l = uint32_t(tid) & 15u;
    uint32_t done_all = 0;
    for (;;) {
        __syncthreads();   // the batch is in LDS (first time: the literals are in their area)
        err = C.err;
        const uint32_t nb = C.nb;
        if (err) break;
        // literal runs, and matches that read only what lies before the batch
        for (uint32_t i = g; i < nb; i += ZT / 16) {
            const ZSeq s = sq[i];
            for (uint32_t j = l; j < s.ll; j += 16) dst[s.out + j] = rle ? rle_byte : lits[s.lit + j];
            if (!(s.ml & ZDEP)) {
                const uint32_t mo = s.out + s.ll;
                for (uint32_t j = l; j < s.ml; j += 16) dst[mo + j] = dst[mo - s.off + j];
            }
        }
        __syncthreads();
        // matches that read the batch's own output, in order
        for (uint32_t i = 0; i < nb; i++) {
            const ZSeq s = sq[i];
            if (!(s.ml & ZDEP)) continue;
            const uint32_t ml = s.ml & ~ZDEP, mo = s.out + s.ll;
            // byte j of an overlapping match repeats the off bytes before it, which are complete
            for (uint32_t j = uint32_t(tid); j < ml; j += ZT) dst[mo + j] = dst[mo - s.off + (s.off < ml ? j % s.off : j)];
            __syncthreads();
        }
        __syncthreads();   // every thread is done with the batch before thread 64 overwrites it
        done_all += nb;
        if (done_all >= nseq) break;
        if (tid == ZSEQ_TID) decode_batch();
    }
    if (!err) {   // the literals after the last sequence
        const uint32_t tl = C.tail_lit, to = C.tail_out, tn = C.tail_n;
        for (uint32_t j = uint32_t(tid); j < tn; j += ZT) dst[to + j] = rle ? rle_byte : lits[tl + j];
    }
    __syncthreads();
}

__global__ __launch_bounds__(ZT) void k_zstd(ZstdJob* __restrict__ jobs, const int* __restrict__ order, int n_jobs,
                                             uint8_t* __restrict__ lit_area, uint32_t lit_stride, DevChunkResult* res) {
    __shared__ Tables T;
    __shared__ ZSeq sq[ZB];
    __shared__ ZCtl C;
    const int tid = threadIdx.x;
    uint8_t* lit = lit_area + size_t(blockIdx.x) * lit_stride;
    for (int k = blockIdx.x; k < n_jobs; k += gridDim.x) {
        const int j = order ? order[k] : k;
        const ZstdJob job = jobs[j];
        const uint8_t* src = job.src;
        uint8_t* dst = job.dst;
        if (tid == 0) { C.err = 0; C.ip = 0; C.op = 0; C.f0 = 0; C.nb = 0; }
        __syncthreads();
        int err = 0;
        for (;;) {   // frames
            if (tid == 0) {
                if (C.ip >= job.src_len) C.state = 1;
                else if (!frame_header(src + C.ip, job.src_len - C.ip, C.fh)) C.err = 1;
                else {
                    C.ip += C.fh.hdr;
                    C.state = C.fh.skippable ? 2 : 0;
                    if (!C.fh.skippable) { frame_begin(T); C.f0 = C.op; }
                }
            }
            __syncthreads();
            err = C.err;
            const uint32_t state = C.state;
            __syncthreads();
            if (err || state == 1) break;
            if (state == 2) continue;
            for (;;) {   // blocks
                if (tid == 0) {
                    if (!block_header(src + C.ip, job.src_len - C.ip, C.fh, job.dst_len - C.op, C.bh)) C.err = 1;
                    else C.ip += 3;
                }
                __syncthreads();
                err = C.err;
                const BlockHdr bh = C.bh;
                const uint32_t ip = C.ip, op = C.op, f0 = C.f0;
                __syncthreads();
                if (err) break;
                uint32_t produced = bh.size;
                if (bh.type == 0) {
                    for (uint32_t i = uint32_t(tid); i < bh.size; i += ZT) dst[op + i] = src[ip + i];
                } else if (bh.type == 1) {
                    const uint8_t b = src[ip];
                    for (uint32_t i = uint32_t(tid); i < bh.size; i += ZT) dst[op + i] = b;
                } else {
                    zstd_block(src + ip, bh, dst, op, f0, job.dst_len, lit, T, C, sq);
                    err = C.err;
                    produced = C.block_out;
                }
                __syncthreads();   // the block's bytes are visible to the next block's matches
                if (err) break;
                if (tid == 0) { C.ip = ip + bh.src; C.op = op + produced; }
                if (bh.last) break;
            }
            if (err) break;
            if (tid == 0) {   // frame end
                if (C.fh.has_fcs && uint64_t(C.op - C.f0) != C.fh.fcs) C.err = 1;
                if (C.fh.checksum) {   // consumed, not verified
                    if (job.src_len - C.ip < 4) C.err = 1;
                    else C.ip += 4;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const bool bad = C.err || (job.exact && C.op != job.dst_len);
            jobs[j].produced = bad ? 0u : C.op;
            if (bad) set_status(res, job.chunk, ST_CORRUPT, job.page);
        }
        __syncthreads();
    }
}

void launch_zstd(ZstdJob* d_jobs, const int* d_order, int n_jobs, uint8_t* d_lit, uint32_t lit_stride, DevChunkResult* d_res,
                 hipStream_t s) {
    if (n_jobs > 0)
        hipLaunchKernelGGL(k_zstd, dim3(n_jobs < ZSTD_GRID ? n_jobs : ZSTD_GRID), dim3(ZT), 0, s, d_jobs, d_order, n_jobs, d_lit,
                           lit_stride, d_res);
}

}  // namespace pf
