// pf_window.hip — the row-window stage of pf_decode_row_group_rows (gfx950, wave64): after a batch is decoded, the
// chunks that carry a window are cut to its rows on the device, into twin output arenas, so only those rows cross the
// link. Trimming in place is not possible: the parallel forward moves of one array overlap.
//   k_win_bounds  one workgroup per windowed chunk: the window's entry, slot and chars ranges and its num_values
//   k_win_copy    grid over (tile, chunk): byte copies with a realigned source, funnel-shifted validity bits,
//                 rebased offsets
// Nothing here uses atomics: every count is a reduction in a fixed order.
#include "pf_launch.h"

namespace pf {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int WB = 256;                       // threads of both kernels
constexpr uint32_t WIN_BOUNDS_TILE = 4 * WB;  // repetition levels one k_win_bounds round counts

__device__ __forceinline__ void win_fail(DevWinRes* o, int32_t status) {
    if (threadIdx.x == 0) {
        *o = DevWinRes{};
        o->status = status;
    }
}

// The window's ranges. Flat chunk: entries = slots = rows. max_rep = 1: slots from list_offsets; the entry range runs
// from the skip-th entry with rep == 0 to the (skip + take)-th (or the chunk's end), found by a workgroup-wide count:
// ballot and popcount per wave over tiles of 1024 entries with a carry, the lane whose bit is the k-th set one reports
// its index. Every branch before a barrier is uniform over the workgroup.
__global__ __launch_bounds__(WB) void k_win_bounds(const DevChunk* __restrict__ chunks, const DevChunkResult* __restrict__ res,
                                                   const DevWin* __restrict__ wins, DevWinRes* __restrict__ out,
                                                   const uint8_t* chars_base, uint8_t* wchars_base) {
    const DevWin w = wins[blockIdx.x];
    const DevChunk& ck = chunks[w.chunk];
    const DevChunkResult& r = res[w.chunk];
    DevWinRes* o = &out[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int64_t s_pos[2];
    __shared__ uint32_t s_cnt[4];
    __shared__ unsigned long long s_sum[4];

    if (r.status != 0) { win_fail(o, r.status); return; }
    const int64_t rows = r.num_rows, entries = ck.num_entries;
    const int64_t skip = w.skip;
    if (skip < 0 || skip > rows || w.take < -1 || (w.take >= 0 && w.take > rows - skip)) { win_fail(o, PF_ERR_INVALID_ARG); return; }
    const int64_t take = w.take < 0 ? rows - skip : w.take;
    if (ck.max_rep >= 1 && entries > 0 && ck.rep_levels && ck.rep_levels[0] != 0) { win_fail(o, PF_ERR_CORRUPT_PAGE); return; }
    if (skip == 0 && take == rows) {
        if (tid == 0) { *o = DevWinRes{}; o->identity = 1; }
        return;
    }
    if (ck.max_rep > 1 || (ck.max_rep == 1 && (!ck.list_offsets || !ck.rep_levels))) { win_fail(o, PF_ERR_UNSUPPORTED_TYPE); return; }

    int64_t e0 = skip, e1 = skip + take, s0 = skip, s1 = skip + take;
    if (ck.max_rep == 1) {
        s0 = ck.list_offsets[skip];
        s1 = ck.list_offsets[skip + take];
        const int64_t tgt0 = skip, tgt1 = skip + take;   // index among the entries with rep == 0; == rows: the end
        if (tid == 0) { s_pos[0] = entries; s_pos[1] = entries; }
        __syncthreads();
        const uint8_t* __restrict__ rep = ck.rep_levels;
        int64_t carry = 0;
        for (int64_t base = 0; base < entries; base += WIN_BOUNDS_TILE) {
            uint64_t m[4];
            uint32_t c = 0;
            #pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t i = base + wave * 256 + k * 64 + lane;
                const bool z = i < entries && rep[i] == 0;
                m[k] = __ballot(z);
                c += uint32_t(__popcll(m[k]));
            }
            if (lane == 0) s_cnt[wave] = c;
            __syncthreads();
            uint32_t before = 0, total = 0;
            #pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t v = s_cnt[i];
                before += i < wave ? v : 0u;
                total += v;
            }
            const int64_t wstart = carry + before;
            #pragma unroll
            for (int t = 0; t < 2; t++) {
                const int64_t k = t ? tgt1 : tgt0;
                if (k >= wstart && k < wstart + c) {   // wave-uniform
                    uint32_t rel = uint32_t(k - wstart);
                    bool found = false;
                    #pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t pc = uint32_t(__popcll(m[q]));
                        if (!found && rel < pc) {
                            const uint64_t below = m[q] & ((1ull << lane) - 1ull);
                            if (((m[q] >> lane) & 1ull) && uint32_t(__popcll(below)) == rel)
                                s_pos[t] = base + wave * 256 + q * 64 + lane;
                            found = true;
                        }
                        if (!found) rel -= pc;
                    }
                }
            }
            carry += total;
            __syncthreads();
            if (carry > tgt1) break;   // both found
        }
        e0 = s_pos[0];
        e1 = s_pos[1];
    }
    const DevWinRes zero{};
    int64_t c0 = 0, c1 = 0;
    const bool ba = ck.ptype == PF_BYTE_ARRAY && ck.offsets && ck.chars;
    if (s0 < 0 || s0 > s1 || s1 > r.num_slots || e0 > e1 || e1 > entries) { win_fail(o, PF_ERR_CORRUPT_PAGE); return; }
    if (ba) {
        c0 = ck.offsets[s0];
        c1 = ck.offsets[s1];
        if (c0 < 0 || c0 > c1 || c1 > r.num_chars) { win_fail(o, PF_ERR_CORRUPT_PAGE); return; }
    }
    // num_values: the present slots of the window
    unsigned long long nv = (unsigned long long)(s1 - s0);
    if (ck.max_def > 0 && ck.validity) {
        const uint64_t* __restrict__ v = reinterpret_cast<const uint64_t*>(ck.validity);
        unsigned long long sum = 0;
        const int64_t w1 = (s1 + 63) >> 6;
        for (int64_t wi = (s0 >> 6) + tid; wi < w1; wi += WB) {
            uint64_t x = v[wi];
            const int64_t lo = wi << 6;
            if (lo < s0) x &= ~0ull << (s0 - lo);
            if (lo + 64 > s1) x &= ~0ull >> (lo + 64 - s1);
            sum += (unsigned long long)__popcll(x);
        }
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        nv = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    }
    if (tid == 0) {
        DevWinRes x = zero;
        x.e0 = e0; x.n_entries = e1 - e0;
        x.s0 = s0; x.n_slots = s1 - s0;
        x.c0 = c0; x.n_chars = c1 - c0;
        x.n_values = int64_t(nv);
        x.n_rows = take;
        if (ba) {
            x.chars_src = ck.chars;
            x.chars_dst = wchars_base + (ck.chars - chars_base);
        }
        *o = x;
    }
}

// ---- k_win_copy ----------------------------------------------------------------------------------------------------

// One tile of a byte copy: dst (16-byte aligned: the twin arrays start where the decode arena's do, 256-byte aligned)
// takes 16 bytes per lane; the source starts anywhere (skip * width), so a lane reads the two aligned 16-byte blocks
// its bytes lie in and shifts (the misalignment is uniform over the workgroup). The last 16..31 bytes go byte by byte,
// so no load touches a block without a byte of the range.
__device__ __forceinline__ void copy_tile(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t n, int64_t tile) {
    const int64_t off = tile * WIN_TILE + int64_t(threadIdx.x) * 16;
    if (off >= n) return;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src) + uintptr_t(off);
    const uint32_t m = uint32_t(sa & 15u);
    if (m == 0 ? off + 16 <= n : off + 32 <= n) {
        const u4* b = reinterpret_cast<const u4*>(sa - m);
        u4 lo = b[0], x = lo;
        if (m) {
            const u4 hi = b[1];
            uint32_t a0, a1, a2, a3, a4;
            switch (m >> 2) {
                case 0: a0 = lo.x; a1 = lo.y; a2 = lo.z; a3 = lo.w; a4 = hi.x; break;
                case 1: a0 = lo.y; a1 = lo.z; a2 = lo.w; a3 = hi.x; a4 = hi.y; break;
                case 2: a0 = lo.z; a1 = lo.w; a2 = hi.x; a3 = hi.y; a4 = hi.z; break;
                default: a0 = lo.w; a1 = hi.x; a2 = hi.y; a3 = hi.z; a4 = hi.w; break;
            }
            const uint32_t sh = (m & 3u) * 8u;   // (a funnel shift by 0 returns the low word)
            x.x = __funnelshift_r(a0, a1, sh);
            x.y = __funnelshift_r(a1, a2, sh);
            x.z = __funnelshift_r(a2, a3, sh);
            x.w = __funnelshift_r(a3, a4, sh);
        }
        *reinterpret_cast<u4*>(dst + off) = x;
    } else {
        const int64_t end = off + 16 < n ? off + 16 : n;
        for (int64_t i = off; i < end; i++) dst[i] = src[i];
    }
}

// One tile of rebased offsets: dst[i] = src[i] - src[0], i < n; four per lane, one 16-byte store.
__device__ __forceinline__ void offsets_tile(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int64_t n, int64_t tile) {
    const int64_t i0 = tile * (WIN_TILE / 4) + int64_t(threadIdx.x) * 4;
    if (i0 >= n) return;
    const int32_t first = src[0];
    int32_t v[4];
    #pragma unroll
    for (int k = 0; k < 4; k++) v[k] = i0 + k < n ? src[i0 + k] - first : 0;
    if (i0 + 4 <= n) {
        *reinterpret_cast<int4*>(dst + i0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        #pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + k < n) dst[i0 + k] = v[k];
    }
}

// One tile of validity bits: output word j is source bits [b0 + 64 j, b0 + 64 j + 64), read as two words; the final
// word is masked to nbits, and of it only the bytes of ceil(nbits / 8) are written.
__device__ __forceinline__ void bits_tile(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t b0, int64_t nbits,
                                          int64_t tile) {
    const uint64_t* __restrict__ v = reinterpret_cast<const uint64_t*>(src);
    const int64_t nbytes = (nbits + 7) >> 3;
    const uint32_t sh = uint32_t(b0 & 63);
    #pragma unroll
    for (int h = 0; h < 2; h++) {
        const int64_t j = tile * (WIN_TILE / 8) + h * WB + threadIdx.x;
        if (8 * j >= nbytes) continue;
        const int64_t first = b0 + 64 * j, rem = nbits - 64 * j;
        const int64_t last = rem < 64 ? b0 + nbits - 1 : first + 63;
        const int64_t sw = first >> 6;
        uint64_t x = v[sw];
        if (sh) {
            const uint64_t hi = (last >> 6) > sw ? v[sw + 1] : 0ull;
            x = (x >> sh) | (hi << (64u - sh));
        }
        if (rem < 64) x &= (1ull << rem) - 1ull;
        if (8 * j + 8 <= nbytes) {
            reinterpret_cast<uint64_t*>(dst)[j] = x;
        } else {
            for (int64_t b = 8 * j; b < nbytes; b++) dst[b] = uint8_t(x >> (8 * (b - 8 * j)));
        }
    }
}

__device__ __forceinline__ int64_t tiles_of(int64_t bytes) { return (bytes + WIN_TILE - 1) / WIN_TILE; }

template <typename T>
__device__ __forceinline__ T* twin(const T* p, int64_t delta) {
    return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + uintptr_t(delta));
}

// Grid (tiles, windowed chunk). A chunk's arrays are laid end to end in tiles of WIN_TILE output bytes; the workgroups
// of its row stride over them (the sizes are known only on the device, so the host sizes the grid from capacities).
__global__ __launch_bounds__(WB) void k_win_copy(const DevChunk* __restrict__ chunks, const DevWin* __restrict__ wins,
                                                 const DevWinRes* __restrict__ wres, int64_t out_delta, int64_t bits_delta,
                                                 const int32_t* __restrict__ keep_of, const DevKeep* __restrict__ keeps) {
    const DevWinRes r = wres[blockIdx.y];
    if (r.status != 0 || r.identity) return;
    const DevChunk& ck = chunks[wins[blockIdx.y].chunk];
    const int64_t skip = wins[blockIdx.y].skip;
    // a kept chunk's values are its indices, index_width bytes a slot (ck.width is its dictionary's entry width); it
    // has no offsets and no chars, and its dictionary stays where it is
    const int32_t kp = keep_of ? keep_of[wins[blockIdx.y].chunk] : -1;
    const int64_t width = kp >= 0 ? keeps[kp].index_width : ck.width;
    const int64_t nb_val = ck.values && width > 0 ? r.n_slots * width : 0;
    const int64_t nb_def = ck.def_levels ? r.n_entries : 0, nb_rep = ck.rep_levels ? r.n_entries : 0;
    const int64_t nb_chr = r.chars_src ? r.n_chars : 0;
    const int64_t nb_off = ck.offsets ? 4 * (r.n_slots + 1) : 0, nb_lof = ck.list_offsets ? 4 * (r.n_rows + 1) : 0;
    const int64_t nb_vld = ck.validity ? (r.n_slots + 7) >> 3 : 0, nb_lvl = ck.list_validity ? (r.n_rows + 7) >> 3 : 0;
    const int64_t t0 = tiles_of(nb_val), t1 = t0 + tiles_of(nb_def), t2 = t1 + tiles_of(nb_rep), t3 = t2 + tiles_of(nb_chr),
                  t4 = t3 + tiles_of(nb_off), t5 = t4 + tiles_of(nb_lof), t6 = t5 + tiles_of(nb_vld), t7 = t6 + tiles_of(nb_lvl);
    for (int64_t g = blockIdx.x; g < t7; g += gridDim.x) {
        if (g < t0) copy_tile(twin(ck.values, out_delta), ck.values + r.s0 * width, nb_val, g);
        else if (g < t1) copy_tile(twin(ck.def_levels, out_delta), ck.def_levels + r.e0, nb_def, g - t0);
        else if (g < t2) copy_tile(twin(ck.rep_levels, out_delta), ck.rep_levels + r.e0, nb_rep, g - t1);
        else if (g < t3) copy_tile(r.chars_dst, r.chars_src + r.c0, nb_chr, g - t2);
        else if (g < t4) offsets_tile(twin(ck.offsets, out_delta), ck.offsets + r.s0, r.n_slots + 1, g - t3);
        else if (g < t5) offsets_tile(twin(ck.list_offsets, out_delta), ck.list_offsets + skip, r.n_rows + 1, g - t4);
        else if (g < t6) bits_tile(twin(ck.validity, bits_delta), ck.validity, r.s0, r.n_slots, g - t5);
        else bits_tile(twin(ck.list_validity, bits_delta), ck.list_validity, skip, r.n_rows, g - t6);
    }
}

}  // namespace

void launch_window(const DevChunk* d_chunks, const DevChunkResult* d_res, const DevWin* d_wins, DevWinRes* d_wres, int n_wins,
                   int copy_grid, const uint8_t* chars_base, uint8_t* wchars_base, int64_t out_delta, int64_t bits_delta,
                   const int* d_keep_of, const DevKeep* d_keeps, hipStream_t st) {
    if (n_wins <= 0) return;
    hipLaunchKernelGGL(k_win_bounds, dim3(n_wins), dim3(WB), 0, st, d_chunks, d_res, d_wins, d_wres, chars_base, wchars_base);
    hipLaunchKernelGGL(k_win_copy, dim3(copy_grid < 1 ? 1 : copy_grid, n_wins), dim3(WB), 0, st, d_chunks, d_wins, d_wres,
                       out_delta, bits_delta, d_keep_of, d_keeps);
}

}  // namespace pf
