// pf_zstd_enc.hip — ZSTD compression of the write path (PF_CODEC_ZSTD): k_zstd_compress, one wave per
// job of <= ZC_BLOCK bytes, one job = one complete block (3-byte header included) in its slot.
//
// The format work is pf_zstd_enc_core.h, shared with the host model (compress_host), which emits the
// same bytes. What is here is who runs it:
//   1. match finding, k_snappy_compress's: the job staged in LDS, a 4096-entry table of the last
//      position (+1) of each 4-byte prefix hash, 64 positions a step looked up against the table as it
//      stood before the step, the first matching lane starts a match (extended 64 bytes per ballot, never
//      split, passed over when it stays below ZE_MIN_MATCH), later matching lanes past its end follow in
//      the same step. Instead of tokens the wave appends {literal length, match length, offset} records
//      and the literal bytes to LDS. The table is
//      updated with an LDS atomic max, so two positions of one hash in a step leave the later one
//      whichever lane goes first (the host model takes them in order);
//   2. literals: histogram by LDS atomic adds, a rank sort of the present symbols over the lanes, the
//      code lengths and the tree description by one lane, then per stream every lane takes a run of
//      consecutive symbols, the sums of their code lengths place the runs, and the codes are ORed
//      into LDS dwords (the last symbol lowest: the decoder reads backward);
//   3. sequences: every lane computes the codes of its sequences, three lanes walk one FSE state chain
//      each (one instruction stream over three tables), the bit sums of runs of consecutive sequences
//      place the runs, and all lanes OR their fields into the section (21.6 -> 13.6 ms per SF1 row group
//      against one lane writing the whole section);
//   4. block type from the sizes, the chosen form assembled in LDS and copied to the slot.
// LDS areas that are dead after a phase are used again (EncWork). Every store is a vector store or an
// LDS operation; the atomics are LDS OR / add / max, whose results do not depend on lane order.
#include <hip/hip_runtime.h>

#include "pf_encode.h"
#include "pf_zstd_enc_core.h"

namespace pf {

using namespace zstd;

static_assert(ZC_BLOCK == ZE_BLOCK, "the runtime's job size is the core's");
static_assert(sizeof(EncWork) <= 160u * 1024 / 3, "three workgroups per CU");

__global__ __launch_bounds__(64) void k_zstd_compress(const ZstdCJob* __restrict__ jobs, uint32_t* __restrict__ out_len) {
    __shared__ __attribute__((aligned(16))) EncWork W;
    const ZstdCJob job = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x, len = job.len;
    uint8_t* buf = ew_buf(W);
    uint8_t* lit = ew_lit(W);
    uint8_t* dst = job.dst;
    if (len == 0 || len > ZC_BLOCK) {   // (the runtime makes no such job)
        if (lane == 0) { block_header_put(dst, job.last, 0, 0); out_len[blockIdx.x] = 3; }
        return;
    }
    const uint8_t b0 = job.src[0];
    bool differs = false;
    for (uint32_t i = lane; i < len + 16; i += 64) {
        const uint8_t v = i < len ? job.src[i] : uint8_t(0);
        buf[i] = v;
        differs |= i < len && v != b0;
    }
    if (!__ballot(differs)) {   // RLE block
        if (lane == 0) { block_header_put(dst, job.last, 1, len); dst[3] = b0; out_len[blockIdx.x] = 4; }
        return;
    }
    for (uint32_t i = lane; i < (1u << ZE_HBITS); i += 64) W.tab[i] = 0;
    if (lane < 3) fse_enc_predefined(lane == 0 ? K_LL : lane == 1 ? K_OF : K_ML, lane == 0 ? W.fll : lane == 1 ? W.fof : W.fml, ew_fs(W, int(lane)));
    __syncthreads();

    // ---- 1. matches ----
    uint32_t ip = 0, lt = 0, nseq = 0, nlit = 0;
    while (ip + 4 <= len) {
        const uint32_t q = ip + lane;
        const bool valid = q + 4 <= len;
        const uint32_t v = valid ? ze_ld32(buf, q) : 0u;
        const uint32_t h = ze_hash(v);
        const uint32_t c = valid ? W.tab[h] : 0u;
        const bool m = valid && c != 0 && ze_ld32(buf, c - 1) == v;
        const unsigned long long mask = __ballot(m);
        if (!mask) {
            if (valid) atomicMax(&W.tab[h], q + 1);
            ip += 64;
            continue;
        }
        unsigned long long mk = mask;
        uint32_t e = ip;
        while (mk) {
            const uint32_t f = uint32_t(__ffsll(mk) - 1);
            const uint32_t qf = ip + f;
            const uint32_t cand = uint32_t(__builtin_amdgcn_readlane(int(c), int(f))) - 1u;
            uint32_t L = 4;
            for (;;) {   // extend the match 64 bytes per step
                const uint32_t x = qf + L + lane, y = cand + L + lane;
                const bool eq = x < len && buf[x] == buf[y];
                const unsigned long long ne = __ballot(!eq);
                if (!ne) { L += 64; continue; }
                L += uint32_t(__ffsll(ne) - 1);
                break;
            }
            if (L < ZE_MIN_MATCH) { mk &= mk - 1; continue; }   // not worth a sequence
            const uint32_t ll = qf - lt;
            for (uint32_t j = lane; j < ll; j += 64) lit[nlit + j] = buf[lt + j];
            if (lane == 0) {   // nseq < ZE_SEQ_MAX: matches are >= ZE_MIN_MATCH bytes and do not overlap
                W.sll[nseq] = uint16_t(ll);
                W.sml[nseq] = uint16_t(L);
                W.sof[nseq] = uint16_t(qf - cand);
            }
            nlit += ll;
            nseq++;
            e = qf + L;
            lt = e;
            mk = e - ip >= 64 ? 0ull : (mk & ~((1ull << (e - ip)) - 1ull));
        }
        if (e == ip) e = ip + 64;                           // every match of the step was too short
        if (valid && q < e) atomicMax(&W.tab[h], q + 1);   // positions passed by this step's matches
        ip = e;
    }
    for (uint32_t j = lane; j < len - lt; j += 64) lit[nlit + j] = buf[lt + j];
    nlit += len - lt;
    __syncthreads();   // the table is dead: its area is the sequences section and the Huffman work now

    // ---- 2. literals ----
    HufWork& H = ew_huf(W);
    for (uint32_t s = lane; s < 256; s += 64) H.hist[s] = 0;
    if (lane == 0) { W.nseq = nseq; W.nlit = nlit; H.ndist = 0; }
    __syncthreads();
    huf_hist(W, lane, 64);
    __syncthreads();
    huf_sort(W, lane, 64);
    __syncthreads();
    if (lane == 0) { huf_build(W); lit_streams_plan(W); }
    __syncthreads();
    huf_count_bits(W, lane, 64);
    __syncthreads();

    // ---- 3. sequences, 4. the block ----
#ifdef PF_ZE_SERIAL_SEQ   // A/B build: the whole section by one lane
    if (lane == 0) {
        lit_plan(W, 64);
        W.seq_bytes = seq_encode(W, ew_seq(W), ZE_SEQ_CAP);
        block_plan(W, len, false);
    }
    __syncthreads();
#else
    if (lane == 0) { lit_plan(W, 64); W.reps = 0; }
    for (uint32_t i = lane; i < ZE_SEQ_CAP / 4; i += 64) W.tab[i] = 0;
    __syncthreads();
    seq_codes(W, lane, 64);
    __syncthreads();
    if (lane < 3 && nseq) seq_chain(W, lane);   // three lanes, one chain each, one instruction stream
    __syncthreads();
    seq_count(W, lane, 64);
    __syncthreads();
    if (lane == 0) seq_head(W, ew_seq(W), ZE_SEQ_CAP, 64);
    __syncthreads();
    seq_put(W, W.tab, lane, 64);
    __syncthreads();
    if (lane == 0) block_plan(W, len, false);
    __syncthreads();
#endif
    const uint32_t bsize = W.bsize;
    if (W.btype == 0) {   // raw (bsize = len)
        for (uint32_t i = lane; i < len; i += 64) dst[3 + i] = job.src[i];
        if (lane == 0) { block_header_put(dst, job.last, 0, len); out_len[blockIdx.x] = 3 + len; }
        return;
    }
    // compressed, bsize < len: assembled over the job's bytes, which nothing reads any more
    uint32_t* out32 = W.amem;
    for (uint32_t i = lane; i < (ZE_BLOCK + 16) / 4; i += 64) out32[i] = 0;
    __syncthreads();
    if (lane == 0) lit_write_head(W, buf, 0, W.lp.bit0);
    __syncthreads();
    if (W.lp.type == 2) huf_put(W, out32, W.lp.bit0, lane, 64);
    __syncthreads();
    if (W.lp.type == 0)
        for (uint32_t i = lane; i < nlit; i += 64) buf[W.lp.hdr + i] = lit[i];
    const uint8_t* sq = ew_seq(W);
    for (uint32_t i = lane; i < W.seq_bytes; i += 64) buf[W.lp.total + i] = sq[i];
    __syncthreads();
    for (uint32_t i = lane; i < bsize; i += 64) dst[3 + i] = buf[i];
    if (lane == 0) { block_header_put(dst, job.last, 2, bsize); out_len[blockIdx.x] = 3 + bsize; }
}

void launch_zstd_compress(const ZstdCJob* d_jobs, int n_jobs, uint32_t* d_out_len, hipStream_t st) {
    if (n_jobs > 0) hipLaunchKernelGGL(k_zstd_compress, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_out_len);
}

}  // namespace pf
