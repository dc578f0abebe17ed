// pf_flat_count.hip — the count side of the flat fast path (max_rep == 0): what the flat kernels
// (pf_flat.hip, pf_flat_dstr.hip, pf_flat_null.hip) need known about a page before they decode it.
//   k_runs         per dictionary page: the id run table, walked once for all of the page's blocks,
//                  and whether every level is present
//   k_count_dict   per (page, block) of dictionary BYTE_ARRAY pages: the block's chars
//   k_count_flat   per all-present BYTE_ARRAY page: counts, chars bases of the blocks; PLAIN pages
//                  hand their value chain to the k_ba walk (pf_ba.hip)
//   k_debug_walk   (diagnostics build) wave_walk_runs against a one-lane reference walk
#include <hip/hip_runtime.h>

#include "pf_flat.h"
#include "pf_launch.h"

namespace pf {

// One 128-thread workgroup per dictionary data page of a flat chunk: walks the page's
// dictionary-id run headers ONCE (wave 1) and checks whether every definition level is present
// (wave 0), so that k_flat's blocks of the page load a ready run table instead of each walking
// the headers from the page start.
__global__ __launch_bounds__(128) void k_runs(const DevChunk* __restrict__ chunks, DevPage* pages,
                                              const int* __restrict__ list, DevChunkResult* res) {
    __shared__ Run R[RUN_CAP];
    __shared__ int s_allp, s_nr, s_res;
    __shared__ uint32_t s_cov;
    const int pi = list[blockIdx.x];
    DevPage& pg = pages[pi];
    IdRunTab* T = pg.runtab;
    if (!T) return;
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    Sections s;
    if (res[pg.chunk].status != 0 || !page_sections(pg, ck, s) || s.val_n == 0 || s.val[0] > 32) {
        if (tid == 0) T->all_present = 0;
        return;
    }
    const uint32_t ne = uint32_t(pg.num_values);
    const int id_bw = int(s.val[0]);
    if (tid == 0) {
        s_allp = ck.max_def == 0 ? 1 : (s.def_rle ? all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)) : 0);
    } else if (tid >= 64) {   // wave 1: the id runs, discovered wave-parallel
        __shared__ RunWalk s_st;
        int nr = 0;
        uint32_t cov = 0;
        const int rr = wave_walk_runs(s.val + 1, s.val_n - 1, id_bw, 0, ne, R, RUN_CAP, nr, cov, s_st, RunWalk{0, 0});
        if (tid == 64) { s_res = rr; s_nr = nr; s_cov = cov; }
    }
    __syncthreads();
    const int nr = s_nr;
    if (s_res == 2) {   // too many runs for the table: blocks walk themselves
        if (tid == 0) { T->valid = 0; T->all_present = 0; }
        return;
    }
    for (int i = tid; i < nr; i += 128) {
        T->fp(i) = R[i].first | (R[i].packed << 31);
        T->data(i) = R[i].data;
    }
    if (tid == 0) { T->nruns = uint32_t(nr); T->covered = s_cov; T->valid = 1u; T->all_present = s_allp ? 1u : 0u; }
}

// k_count_dict (round 5): the chars of one 4096-entry block of a flat dictionary BYTE_ARRAY page per
// workgroup -- the block's ids from the page's run table (k_runs), their dictionary lengths summed --
// into the page's per-block chars word bc[block]; k_count_flat scans those words into the blocks'
// chars bases and the page's chars. (Round 4 summed a page's blocks one after another in
// k_count_flat's one workgroup per page: SF1's pages of ~1M entries were 256 dependent rounds.)
__global__ __launch_bounds__(NT) void k_count_dict(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int2* __restrict__ blocks, DevChunkResult* res) {
    __shared__ Run R[RUN_CAP];
    __shared__ uint32_t s_len[DSTR_CAP];   // lengths of small dictionaries
    __shared__ unsigned long long s_acc;
    const int2 pb = blocks[blockIdx.x];
    DevPage& pg = pages[pb.x];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.ptype != 6 || !is_dict_enc(pg.encoding)) return;
    Sections s;
    if (!page_sections(pg, ck, s) || !count_dict_page(pg, ck, s)) return;
    const uint32_t ne = uint32_t(pg.num_values);
    const uint32_t b0 = uint32_t(pb.y) * FBLK;
    if (pb.y > 0 && b0 >= ne) return;
    const uint32_t b1 = min(ne, b0 + FBLK);
    const IdRunTab* T = pg.runtab;
    const uint32_t nr = T->nruns, cov = T->covered;
    for (uint32_t i = tid; i < nr; i += NT) R[i] = id_run(T, i, nr, cov);
    const bool lstage = ck.dict_n > 0 && ck.dict_n <= int64_t(DSTR_CAP);
    if (lstage)
        for (uint32_t i = tid; i < uint32_t(ck.dict_n); i += NT) s_len[i] = gptr(ck.dict_len)[i];
    if (tid == 0) s_acc = 0;
    __syncthreads();
    const uint8_t* ids = s.val + 1;
    const uint64_t ids_n = s.val_n - 1;
    const int id_bw = int(s.val[0]);
    constexpr int EPB = int(FBLK) / NT;   // entries of the block per thread
    int bad = 0;
    uint64_t acc = 0;
    // ids of the thread's EPB entries first (their loads in flight together), then the lengths
    uint32_t idk[EPB];
    int r = -1;
    #pragma unroll
    for (int k = 0; k < EPB; k++) {
        const uint32_t e = b0 + uint32_t(k) * NT + uint32_t(tid);
        idk[k] = 0xffffffffu;
        if (e >= b1) continue;
        if (r < 0) r = run_find(R, int(nr), e);
        while (e >= R[r].first + R[r].count) r++;
        const Run& Rr = R[r];
        uint32_t id = Rr.data;
        if (Rr.packed) {
            const uint64_t bit = uint64_t(Rr.data) + uint64_t(e - Rr.first) * uint64_t(id_bw);
            id = (bit >> 3) + 12 <= ids_n ? bits_fast(ids + (bit >> 3), uint32_t(bit & 7), id_bw)
                                          : bits_le(ids, ids_n, bit, id_bw);
        }
        if (int64_t(id) >= ck.dict_n) { bad = 1; continue; }
        idk[k] = id;
    }
    #pragma unroll
    for (int k = 0; k < EPB; k++)
        if (idk[k] != 0xffffffffu) acc += lstage ? s_len[idk[k]] : gptr(ck.dict_len)[idk[k]];
    if (acc) atomicAdd(&s_acc, (unsigned long long)acc);
    bad = __syncthreads_or(bad);
    if (tid == 0) flat_block_chars(pg)[pb.y] = bad ? BC_BAD : uint64_t(s_acc);
}

// k_count for flat BYTE_ARRAY pages whose levels are all present: slots = rows = values =
// entries; dictionary strings scan k_count_dict's per-block chars (k_flat's per-block chars bases,
// the page's chars); PLAIN pages hand their value chain to the k_ba walk. Marks the page counted
// (pg.counted) so k_count skips it; pages it leaves alone (nulls, corrupt) go through k_count.
__global__ __launch_bounds__(NT) void k_count_flat(const DevChunk* __restrict__ chunks, DevPage* pages,
                                                   const int* __restrict__ page_list, DevChunkResult* res,
                                                   BaJob* bajobs) {
    __shared__ int s_ok;
    __shared__ unsigned long long s_scan[NT / 64];
    const int pi = page_list[blockIdx.x];
    DevPage& pg = pages[pi];
    const DevChunk& ck = chunks[pg.chunk];
    const int tid = threadIdx.x;
    if (res[pg.chunk].status != 0 || ck.max_rep != 0 || ck.ptype != 6) return;
    Sections s;
    if (!page_sections(pg, ck, s)) return;
    const bool dict = is_dict_enc(pg.encoding);
    const uint32_t ne = uint32_t(pg.num_values);
    uint64_t total = 0;
    if (dict) {
        if (!count_dict_page(pg, ck, s)) return;
        // k_count_dict's block sums -> exclusive bases in place (a page of 1M entries: 256 words)
        uint64_t* bc = flat_block_chars(pg);
        const uint32_t nb = (ne + FBLK - 1) / FBLK;
        int bad = 0;
        for (uint32_t b = 0; b < nb; b += NT) {
            const uint32_t i = b + uint32_t(tid);
            uint64_t v = i < nb ? bc[i] : 0ull;
            if (v == BC_BAD) { bad = 1; v = 0; }
            uint64_t tot;
            const uint64_t ex = block_excl_scan64<NT>(v, s_scan, tot);
            if (i < nb) bc[i] = total + ex;
            total += tot;
        }
        if (__syncthreads_or(bad)) return;   // k_count reports the bad id
    } else {
        if (pg.encoding != 0 || pg.ba_job < 0) return;
        if (tid == 0)
            s_ok = ck.max_def == 0 ? 1
                                   : (s.def_rle ? all_present(s.def, s.def_n, bit_width(ck.max_def), ne, uint32_t(ck.max_def)) : 0);
        __syncthreads();
        if (!s_ok) return;
        if (tid == 0) {   // the value chain is walked by the k_ba_* kernels
            BaJob& J = bajobs[pg.ba_job];
            J.p = s.val;
            J.n = uint32_t(min<uint64_t>(s.val_n, J.n_cap));
            J.count = int64_t(ne);
            J.state = ne > 0 ? BA_OK : BA_SKIP;
        }
    }
    if (tid == 0) {
        pg.n_slots = int64_t(ne);
        pg.n_values = int64_t(ne);
        pg.n_rows = int64_t(ne);
        pg.n_chars = int64_t(total);
        pg.counted = 1;
    }
}

#ifdef PF_DIAG
// Diagnostics (tests/test_gpu_runs.py): walk_runs (one lane) and wave_walk_runs (one wave) over the
// same stream; out = {ret, nruns, covered, pos, first, runs[cap] x 4} for each.
// walk_runs is the reference: the run walk's contract (RunWalk, pf_pages.h) header by header.
__device__ int walk_runs(const uint8_t* p, uint64_t n, int bw, uint32_t lo, uint32_t limit, Run* runs, int cap,
                         int& nruns, uint32_t& covered, RunWalk& st) {
    nruns = 0;
    covered = st.first;
    while (st.first < limit) {
        uint64_t pos = st.pos, h;
        if (!uvarint(p, n, pos, h)) return 1;
        Run r;
        uint64_t cnt;
        if (h & 1) {
            cnt = (h >> 1) * 8;
            const uint64_t nb = (h >> 1) * uint64_t(bw);
            r.data = uint32_t(pos * 8);
            r.packed = 1;
            pos += nb < n - pos ? nb : n - pos;   // truncated to what is left (zero-padded)
        } else {
            cnt = h >> 1;
            const int nbv = (bw + 7) >> 3;
            if (pos + nbv > n) return 1;
            uint32_t v = 0;
            for (int b = 0; b < nbv; b++) v |= uint32_t(p[pos + b]) << (8 * b);
            pos += nbv;
            r.data = v;
            r.packed = 0;
        }
        if (cnt == 0) { st.pos = pos; continue; }
        const uint32_t c = uint32_t(cnt < uint64_t(limit - st.first) ? cnt : uint64_t(limit - st.first));
        if (st.first + c > lo) {
            if (nruns == cap) return 2;
            r.first = st.first;
            r.count = c;
            runs[nruns++] = r;
            covered = st.first + c;
        } else {
            covered = st.first + c;
        }
        st.pos = pos;
        st.first += c;
    }
    return 0;
}

__global__ __launch_bounds__(64) void k_debug_walk(const uint8_t* p, uint64_t n, int bw, uint32_t lo, uint32_t limit, int cap,
                                                    uint32_t pos0, uint32_t first0, uint32_t* out) {
    __shared__ Run R[RUN_CAP];
    __shared__ int s_nr;
    __shared__ uint32_t s_cov;
    __shared__ RunWalk s_st;
    const int tid = threadIdx.x;
    uint32_t* o1 = out;
    uint32_t* o2 = out + 5 + 4 * cap;
    if (tid == 0) {
        RunWalk st{pos0, first0};
        int nr = 0;
        uint32_t cov = 0;
        const int r = walk_runs(p, n, bw, lo, limit, R, cap, nr, cov, st);
        o1[0] = uint32_t(r); o1[1] = uint32_t(nr); o1[2] = cov; o1[3] = uint32_t(st.pos); o1[4] = st.first;
        for (int i = 0; i < nr; i++) { o1[5 + 4 * i] = R[i].first; o1[6 + 4 * i] = R[i].count; o1[7 + 4 * i] = R[i].data; o1[8 + 4 * i] = R[i].packed; }
        s_st = RunWalk{pos0, first0};
    }
    __syncthreads();
    const int r = wave_walk_runs(p, n, bw, lo, limit, R, cap, s_nr, s_cov, s_st, RunWalk{pos0, first0});
    __syncthreads();
    if (tid == 0) {
        o2[0] = uint32_t(r); o2[1] = uint32_t(s_nr); o2[2] = s_cov; o2[3] = uint32_t(s_st.pos); o2[4] = s_st.first;
    }
    for (int i = tid; i < s_nr; i += 64) { o2[5 + 4 * i] = R[i].first; o2[6 + 4 * i] = R[i].count; o2[7 + 4 * i] = R[i].data; o2[8 + 4 * i] = R[i].packed; }
}

extern "C" int pf_debug_walk_runs(const uint8_t* stream, uint64_t n, int bw, uint32_t lo, uint32_t limit, int cap,
                                  uint32_t pos0, uint32_t first0, uint32_t* out) {
    if (cap > int(RUN_CAP) || cap < 0) return -1;
    uint8_t* d = nullptr;
    uint32_t* o = nullptr;
    const size_t ob = 4 * size_t(2 * (5 + 4 * cap));
    if (hipMalloc(&d, n + 64) != hipSuccess) return -1;
    if (hipMalloc(&o, ob) != hipSuccess) { (void)hipFree(d); return -1; }
    int rc = 0;
    if (hipMemset(d, 0, n + 64) != hipSuccess || hipMemcpy(d, stream, n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(o, 0, ob) != hipSuccess)
        rc = -1;
    if (!rc) {
        hipLaunchKernelGGL(k_debug_walk, dim3(1), dim3(64), 0, 0, d, n, bw, lo, limit, cap, pos0, first0, o);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, o, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    }
    (void)hipFree(d);
    (void)hipFree(o);
    return rc;
}
#endif  // PF_DIAG

// ---- launchers -------------------------------------------------------------------------------
// The flat half of the count stage; launch_count (pf_decode.hip) follows it on the stream.
void launch_count_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int n_flat, const int2* d_dblk,
                       int n_dblk, DevChunkResult* d_res, BaJob* d_bajobs, hipStream_t st) {
    // d_list: the count list of n pages, whose first n_flat are the flat BYTE_ARRAY pages (k_count_flat's
    // grid; none: no launch). d_dblk: (page, block) pairs of the flat dictionary BYTE_ARRAY pages
    // (k_count_dict, before k_count_flat)
    if (n <= 0) return;
    if (n_dblk > 0) hipLaunchKernelGGL(k_count_dict, dim3(n_dblk), dim3(NT), 0, st, d_chunks, d_pages, d_dblk, d_res);
    if (n_flat > 0) hipLaunchKernelGGL(k_count_flat, dim3(n_flat), dim3(NT), 0, st, d_chunks, d_pages, d_list, d_res, d_bajobs);
}
void launch_runs(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res,
                 hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs, dim3(n), dim3(128), 0, st, d_chunks, d_pages, d_list, d_res);
}

}  // namespace pf
