// pf_lz4.hip — LZ4_RAW page decompression on gfx950 (wave64), over the decode core of pf_lz4_core.h.
//
// The sequences of a block depend on each other through positions only, so one 256-thread workgroup
// takes a page; workgroups stride over the jobs in dispatch order. Every decision that can refuse a
// page is the core's next_seq, the same code the host model runs; the kernel adds only who does what:
//  * all threads stage LZ4_WINDOW bytes of the input in LDS, 16 bytes a lane, from the 16-byte
//    aligned address at or below the next token;
//  * thread 0 walks the tokens through the core, reading the window (a byte outside it -- a field
//    that straddles the window's end, an offset behind a long literal run -- is read from global
//    memory), and writes up to LZ4_BATCH sequences with their output positions into LDS. A batch
//    ends when it is full or the next token lies outside the window; it holds at least one sequence;
//  * a batch's literal runs (read from the input stream itself), and its matches whose source ends
//    before the batch's first output byte, are copied by 16 groups of 16 lanes at once; runs and
//    such matches of LZ_LONG bytes or more are left to a pass of all 256 threads;
//  * the matches that read the batch's own output follow in sequence order, each by all 256 threads
//    with a barrier after it. A match with off < ml reads dst[mo - off + j % off].
// Every loop is bounded by src_len or dst_len: a sequence consumes at least one input byte.
// LDS: the window (8 KiB) + the batch (5 KiB) + control: 13.3 KiB, 12 workgroups per CU by LDS.
// Output goes to the page's scratch body, where the Snappy and ZSTD kernels put theirs.
#include <hip/hip_runtime.h>

#include "pf_device.h"
#include "pf_launch.h"
#include "pf_lz4_core.h"

namespace pf {

using namespace lz4;

constexpr int LT = 256;              // threads
constexpr uint32_t LZ_LONG = 1024;   // a run or match this long is copied by the whole workgroup
constexpr uint32_t LDEP = 1u << 31;

struct LSeq {
    uint32_t out, lit, ll, ml, off;   // ml: LDEP set = the match reads this batch's output
};

struct LCtl {
    int err;
    uint32_t ip, op;          // input / output position of the next sequence
    uint32_t nb, nlong, last;
};

// Byte i of the stream: from the LDS window [lo, lo + LZ4_WINDOW) (lo wraps below 0 by up to 15),
// else from global memory. The core asks for bytes below src_len only.
struct WinReader {
    const uint8_t* win;
    const uint8_t* src;
    uint32_t lo;
    __device__ uint32_t operator()(uint32_t i) const {
        const uint32_t d = i - lo;
        return d < LZ4_WINDOW ? win[d] : src[i];
    }
};

__global__ __launch_bounds__(LT) void k_lz4(Lz4Job* __restrict__ jobs, const int* __restrict__ order, int n_jobs,
                                            DevChunkResult* res) {
    __shared__ __attribute__((aligned(16))) uint8_t win[LZ4_WINDOW];
    __shared__ LSeq sq[LZ4_BATCH];
    __shared__ LCtl C;
    const int tid = threadIdx.x;
    const uint32_t g = uint32_t(tid) >> 4, l = uint32_t(tid) & 15u;
    for (int k = blockIdx.x; k < n_jobs; k += gridDim.x) {
        const int j = order ? order[k] : k;
        const Lz4Job job = jobs[j];
        const uint8_t* src = job.src;
        uint8_t* dst = job.dst;
        const uint32_t n = job.src_len, size = job.dst_len;
        if (tid == 0) { C.err = 0; C.ip = 0; C.op = 0; C.nb = 0; C.nlong = 0; C.last = 0; }
        __syncthreads();
        for (;;) {
            // ---- the window at the next token ----
            const uint32_t ip0 = C.ip;
            const uint32_t lo = ip0 - uint32_t((reinterpret_cast<uintptr_t>(src) + ip0) & 15u);
            for (uint32_t q = uint32_t(tid); q < LZ4_WINDOW / 16; q += LT) {
                const int64_t pos = int64_t(int32_t(lo)) + 16 * int64_t(q);   // lo >= -15
                if (pos >= int64_t(n)) break;
                if (pos >= 0 && pos + 16 <= int64_t(n)) {
                    *reinterpret_cast<uint4*>(win + 16 * q) = *reinterpret_cast<const uint4*>(src + pos);
                } else {
                    for (int b = 0; b < 16; b++)
                        if (pos + b >= 0 && pos + b < int64_t(n)) win[16 * q + uint32_t(b)] = src[pos + b];
                }
            }
            __syncthreads();
            // ---- thread 0 walks a batch ----
            if (tid == 0) {
                const WinReader rd{win, src, lo};
                uint32_t ip = ip0, op = C.op, nb = 0, nlong = 0, last = 0;
                const uint32_t batch_start = op;
                bool ok = true;
                while (nb < LZ4_BATCH && ip - lo < LZ4_WINDOW) {
                    Seq s;
                    if (!next_seq(rd, n, size, ip, op, s)) { ok = false; break; }
                    const uint32_t mo = op + s.ll;
                    const bool dep = uint64_t(mo) + s.ml > uint64_t(batch_start) + s.off;
                    nlong += s.ll >= LZ_LONG || (!dep && s.ml >= LZ_LONG);
                    sq[nb++] = LSeq{op, s.lit, s.ll, s.ml | (dep ? LDEP : 0u), s.off};
                    op = mo + s.ml;
                    if (s.last) { last = 1; break; }
                }
                C.ip = ip; C.op = op; C.nb = nb; C.nlong = nlong; C.last = last;
                if (!ok) C.err = 1;
            }
            __syncthreads();
            const int err = C.err;
            const uint32_t nb = C.nb, nlong = C.nlong, last = C.last;
            if (err) break;
            // ---- literal runs, and matches that read only what lies before the batch ----
            for (uint32_t i = g; i < nb; i += LT / 16) {
                const LSeq s = sq[i];
                if (s.ll < LZ_LONG)
                    for (uint32_t b = l; b < s.ll; b += 16) dst[s.out + b] = src[s.lit + b];
                if (!(s.ml & LDEP) && s.ml < LZ_LONG) {
                    const uint32_t mo = s.out + s.ll;
                    for (uint32_t b = l; b < s.ml; b += 16) dst[mo + b] = dst[mo - s.off + b];
                }
            }
            if (nlong) {
                for (uint32_t i = 0; i < nb; i++) {
                    const LSeq s = sq[i];
                    if (s.ll >= LZ_LONG)
                        for (uint32_t b = uint32_t(tid); b < s.ll; b += LT) dst[s.out + b] = src[s.lit + b];
                    if (!(s.ml & LDEP) && s.ml >= LZ_LONG) {
                        const uint32_t mo = s.out + s.ll;
                        for (uint32_t b = uint32_t(tid); b < s.ml; b += LT) dst[mo + b] = dst[mo - s.off + b];
                    }
                }
            }
            __syncthreads();
            // ---- matches that read the batch's own output, in order ----
            for (uint32_t i = 0; i < nb; i++) {
                const LSeq s = sq[i];
                if (!(s.ml & LDEP)) continue;
                const uint32_t ml = s.ml & ~LDEP, mo = s.out + s.ll;
                // byte b of an overlapping match repeats the off bytes before it, which are complete
                for (uint32_t b = uint32_t(tid); b < ml; b += LT) dst[mo + b] = dst[mo - s.off + (s.off < ml ? b % s.off : b)];
                __syncthreads();
            }
            __syncthreads();   // every thread is done with the batch and the window before they are overwritten
            if (last) break;
        }
        __syncthreads();
        if (tid == 0) {
            const bool bad = C.err != 0;
            jobs[j].produced = bad ? 0u : C.op;
            if (bad) set_status(res, job.chunk, ST_CORRUPT, job.page);
        }
        __syncthreads();
    }
}

void launch_lz4(Lz4Job* d_jobs, const int* d_order, int n_jobs, DevChunkResult* d_res, hipStream_t s) {
    if (n_jobs > 0)
        hipLaunchKernelGGL(k_lz4, dim3(n_jobs < LZ4_GRID ? n_jobs : LZ4_GRID), dim3(LT), 0, s, d_jobs, d_order, n_jobs, d_res);
}

}  // namespace pf
