// pf_filter.hip — the filter stage of pf_decode_row_group_filter (gfx950, wave64): after a batch is decoded and windowed,
// a conjunction of predicates is evaluated over its rows and every chunk is compacted to the matching rows on the
// device, into the arena that does not hold its input, so only those rows and their row numbers cross the link.
//   k_sel_prep    one workgroup: where each chunk's input lies and its output goes, rows_in, the stage's statuses
//   k_sel_mask    grid over row tiles: one lane per row evaluates every predicate; ballots give the mask words
//   k_sel_scan    exclusive scan of per-tile counts in rounds of 256 with a carry (selected rows; BYTE_ARRAY chars)
//   k_sel_rows    the selected row numbers, by rank within the mask words
//   k_sel_gather  grid (output tile, chunk): values and validity bits through the row numbers; BYTE_ARRAY lengths
//   k_sel_chars   grid (output tile, chunk): the new offsets and the chars (long values by a whole wave)
//   k_sel_fin     one workgroup per chunk: num_values and num_chars of the selection
// Nothing here uses atomics: every count is a reduction in a fixed order. Sizes only the device knows (rows_in,
// rows_selected) meet grids sized from the host's capacities; a workgroup past them leaves at once, uniformly.
#include "pf_launch.h"
#include "pf_sel.h"

namespace pf {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint64_t ul2 __attribute__((ext_vector_type(2)));

constexpr int SEL_RPT = int(SEL_TILE / SB);       // consecutive rows per thread of the length scan

template <typename T>
__device__ __forceinline__ T* twin(T* p, int64_t delta) {
    return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + uintptr_t(delta)) : nullptr;
}

__device__ __forceinline__ int64_t tiles_of(int64_t rows) { return (rows + SEL_TILE - 1) / SEL_TILE; }

// Inclusive scan over the wave.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

// ---- k_sel_prep ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB) void k_sel_prep(const DevChunk* __restrict__ chunks, const DevChunkResult* __restrict__ res,
                                                 const DevWinRes* __restrict__ wres, SelBufs f, int n_chunks,
                                                 const uint8_t* chars_base, uint8_t* wchars_base, int64_t out_delta,
                                                 int64_t bits_delta, const int32_t* __restrict__ keep_of,
                                                 const DevKeep* __restrict__ keeps) {
    __shared__ int32_t s_status;
    __shared__ int64_t s_rows;
    const int tid = threadIdx.x;
    for (int c = tid; c < n_chunks; c += SB) {
        const DevChunk& ck = chunks[c];
        const DevChunkResult& r = res[c];
        DevSelChunk x{};
        // a kept chunk (pf_filter_dict.hip) is a fixed-width column of its indices: no offsets and no chars of its own
        const int32_t kp = keep_of ? keep_of[c] : -1;
        x.width = kp >= 0 ? keeps[kp].index_width : ck.width;
        x.ptype = ck.ptype;
        x.max_def = ck.max_def;
        int32_t st = r.status;
        int64_t rows = r.num_rows;
        const int wi = f.win_of[c];
        bool moved = false;   // the window stage left the chunk in the twins
        DevWinRes w{};
        if (st == 0 && wi >= 0) {
            w = wres[wi];
            if (w.status != 0) st = w.status;
            else if (!w.identity) { moved = true; rows = w.n_rows; }
        }
        if (st == 0 && ck.max_rep > 0) st = PF_ERR_UNSUPPORTED_TYPE;
        if (st == 0 && !moved) {
            x.values = ck.values; x.validity = ck.validity; x.offsets = ck.offsets; x.chars = ck.chars;
            x.o_values = twin(ck.values, out_delta); x.o_validity = twin(ck.validity, bits_delta);
            x.o_offsets = twin(ck.offsets, out_delta);
            x.o_chars = ck.chars ? wchars_base + (ck.chars - chars_base) : nullptr;
        } else if (st == 0) {
            x.values = twin(ck.values, out_delta); x.validity = twin(ck.validity, bits_delta);
            x.offsets = twin(ck.offsets, out_delta); x.chars = w.chars_dst;
            x.o_values = ck.values; x.o_validity = ck.validity; x.o_offsets = ck.offsets;
            x.o_chars = const_cast<uint8_t*>(w.chars_src);
        }
        if (kp >= 0) { x.offsets = nullptr; x.chars = nullptr; x.o_offsets = nullptr; x.o_chars = nullptr; }
        x.n_rows = rows;
        x.status = st;
        f.sc[c] = x;
    }
    __syncthreads();
    if (tid == 0) {   // (at most PF_MAX_PREDICATES entries)
        int32_t hs = 0;
        const int64_t rows_in = f.n_preds > 0 ? f.sc[f.preds[0].chunk].n_rows : 0;
        for (int i = 0; i < f.n_preds; i++) {
            const int32_t s = f.sc[f.preds[i].chunk].status;
            if (s != 0 && hs == 0) hs = s;
        }
        for (int i = 0; i < f.n_preds && hs == 0; i++)
            if (f.sc[f.preds[i].chunk].n_rows != rows_in) hs = PF_ERR_INVALID_ARG;
        // (rows_cap: what the host sized the mask and the row numbers for)
        if (hs == 0 && (rows_in < 0 || rows_in > 0x7fffffffll || rows_in > f.rows_cap)) hs = PF_ERR_INVALID_ARG;
        DevSelHead h{};
        h.rows_in = hs == 0 ? rows_in : 0;
        h.status = hs;
        *f.head = h;
        s_status = hs;
        s_rows = rows_in;
    }
    __syncthreads();
    const int32_t hs = s_status;
    const int64_t rows_in = s_rows;
    for (int c = tid; c < n_chunks; c += SB) {
        const int32_t st = f.sc[c].status;
        if (hs != 0) { if (st == 0) f.sc[c].status = hs; }
        else if (st == 0 && f.sc[c].n_rows != rows_in) f.sc[c].status = PF_ERR_INVALID_ARG;
    }
}

// ---- k_sel_mask ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB) void k_sel_mask(SelBufs f) {
    const int64_t rows_in = f.head->rows_in;   // 0 when the stage failed
    const int64_t tile = blockIdx.x, base = tile * SEL_TILE;
    if (base >= rows_in) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ uint32_t s_cnt[4];
    uint32_t cnt = 0;
    #pragma unroll 1
    for (int k = 0; k < SEL_WPW; k++) {
        const int word = wave * SEL_WPW + k;
        const int64_t r = base + word * 64 + lane;
        bool m = r < rows_in;
        for (int i = 0; i < f.n_preds; i++)
            if (m) m = eval_row(f.preds[i], f.sc[f.preds[i].chunk], r, f.blob);
        const uint64_t w = __ballot(m);
        if (lane == 0) f.mask[tile * SEL_WORDS + word] = w;
        cnt += uint32_t(__popcll(w));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) f.tile_count[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---- k_sel_scan ----------------------------------------------------------------------------------------------------

// Workgroup b scans in[b * stride ...] over the tiles of rows_in (by_selected = 0) or of rows_selected into out, and
// writes the sum to totals[b]. With sc set, only BYTE_ARRAY chunks that stand are scanned.
__global__ __launch_bounds__(SB) void k_sel_scan(const uint32_t* in, uint32_t* out, int64_t stride, const DevSelHead* head,
                                                 int by_selected, const DevSelChunk* sc, int64_t* totals) {
    const int b = blockIdx.x;
    if (sc && (sc[b].status != 0 || sc[b].ptype != PF_BYTE_ARRAY || !sc[b].o_offsets)) return;   // (kept: no chars)
    const int64_t n = tiles_of(by_selected ? head->rows_selected : head->rows_in);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    in += b * stride;
    out += b * stride;
    __shared__ uint32_t s_w[4];
    uint64_t carry = 0;
    for (int64_t base = 0; base < n; base += SB) {
        const int64_t i = base + tid;
        const uint32_t v = i < n ? in[i] : 0u;
        const uint32_t x = wave_scan(v, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        #pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t t = s_w[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (i < n) out[i] = uint32_t(carry) + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) totals[b] = int64_t(carry);
}

// ---- k_sel_rows ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB) void k_sel_rows(SelBufs f) {
    const int64_t rows_in = f.head->rows_in;
    const int64_t tile = blockIdx.x, base = tile * SEL_TILE;
    if (base >= rows_in) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t* __restrict__ m = f.mask + tile * SEL_WORDS;
    uint32_t pre = f.tile_base[tile];
    for (int w = 0; w < wave * SEL_WPW; w++) pre += uint32_t(__popcll(m[w]));   // (wave-uniform)
    #pragma unroll 1
    for (int k = 0; k < SEL_WPW; k++) {
        const int word = wave * SEL_WPW + k;
        const uint64_t x = m[word];
        if ((x >> lane) & 1ull) f.rows[pre + uint32_t(__popcll(x & ((1ull << lane) - 1ull)))] = int32_t(base + word * 64 + lane);
        pre += uint32_t(__popcll(x));
    }
}

// ---- k_sel_gather --------------------------------------------------------------------------------------------------

// nj output rows from j0 on: dst[j] = src[rows[j]]. Widths 1, 2, 4 and 8: every lane gathers 16 output bytes and stores
// them at once (the outputs start 256-byte aligned and j0 is a multiple of SEL_TILE); the rows past the last whole
// group go one by one. Other widths (INT96, FIXED_LEN_BYTE_ARRAY): one lane per output dword or byte, so the stores
// are coalesced whatever the width.
__device__ __forceinline__ void gather_values(const DevSelChunk& c, const int32_t* __restrict__ rows, int64_t j0, int nj) {
    const int tid = threadIdx.x;
    const int32_t* __restrict__ rj = rows + j0;
    if (c.width == 4) {
        const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(c.values);
        uint32_t* d = reinterpret_cast<uint32_t*>(c.o_values) + j0;
        for (int i = tid * 4; i < nj; i += SB * 4) {
            if (i + 4 <= nj) {
                const int4 r = *reinterpret_cast<const int4*>(rj + i);
                u4 v;
                v.x = s[r.x]; v.y = s[r.y]; v.z = s[r.z]; v.w = s[r.w];
                *reinterpret_cast<u4*>(d + i) = v;
            } else {
                for (int k = i; k < nj; k++) d[k] = s[rj[k]];
            }
        }
    } else if (c.width == 8) {
        const uint64_t* __restrict__ s = reinterpret_cast<const uint64_t*>(c.values);
        uint64_t* d = reinterpret_cast<uint64_t*>(c.o_values) + j0;
        for (int i = tid * 2; i < nj; i += SB * 2) {
            if (i + 2 <= nj) {
                const int2 r = *reinterpret_cast<const int2*>(rj + i);
                ul2 v;
                v.x = s[r.x]; v.y = s[r.y];
                *reinterpret_cast<ul2*>(d + i) = v;
            } else {
                d[i] = s[rj[i]];
            }
        }
    } else if (c.width == 1) {
        const uint8_t* __restrict__ s = c.values;
        uint8_t* d = c.o_values + j0;
        for (int i = tid * 16; i < nj; i += SB * 16) {
            if (i + 16 <= nj) {
                uint32_t v[4];
                #pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int4 r = *reinterpret_cast<const int4*>(rj + i + 4 * q);
                    v[q] = uint32_t(s[r.x]) | uint32_t(s[r.y]) << 8 | uint32_t(s[r.z]) << 16 | uint32_t(s[r.w]) << 24;
                }
                u4 o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                *reinterpret_cast<u4*>(d + i) = o;
            } else {
                for (int k = i; k < nj; k++) d[k] = s[rj[k]];
            }
        }
    } else if (c.width == 2) {   // (2-byte dictionary indices, FIXED_LEN_BYTE_ARRAY(2))
        const uint16_t* __restrict__ s = reinterpret_cast<const uint16_t*>(c.values);
        uint16_t* d = reinterpret_cast<uint16_t*>(c.o_values) + j0;
        for (int i = tid * 8; i < nj; i += SB * 8) {
            if (i + 8 <= nj) {
                uint32_t v[4];
                #pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int4 r = *reinterpret_cast<const int4*>(rj + i + 4 * q);
                    v[2 * q] = uint32_t(s[r.x]) | uint32_t(s[r.y]) << 16;
                    v[2 * q + 1] = uint32_t(s[r.z]) | uint32_t(s[r.w]) << 16;
                }
                u4 o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                *reinterpret_cast<u4*>(d + i) = o;
            } else {
                for (int k = i; k < nj; k++) d[k] = s[rj[k]];
            }
        }
    } else if ((c.width & 3) == 0) {
        const uint32_t wq = uint32_t(c.width) >> 2;
        const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(c.values);
        uint32_t* d = reinterpret_cast<uint32_t*>(c.o_values) + j0 * wq;
        const uint32_t total = uint32_t(nj) * wq;
        for (uint32_t b = tid; b < total; b += SB) {
            const uint32_t row = b / wq, k = b - row * wq;
            d[b] = s[int64_t(rj[row]) * wq + k];
        }
    } else {
        const uint32_t wb = uint32_t(c.width);
        uint8_t* d = c.o_values + j0 * wb;
        const uint64_t total = uint64_t(nj) * wb;
        for (uint64_t b = tid; b < total; b += SB) {
            const uint64_t row = b / wb, k = b - row * wb;
            d[b] = c.values[int64_t(rj[row]) * wb + k];
        }
    }
}

// Grid (tiles, chunk). The workgroups of a chunk stride over its output tiles of SEL_TILE rows.
// (amdgpu_waves_per_eu: the width-2 case must not cost the other widths a wave per SIMD; 80 VGPRs, no scratch)
__global__ __launch_bounds__(SB) __attribute__((amdgpu_waves_per_eu(6))) void k_sel_gather(SelBufs f) {
    const DevSelChunk c = f.sc[blockIdx.y];
    if (c.status != 0) return;
    const int64_t nsel = f.head->rows_selected, ntiles = tiles_of(nsel);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ rows = f.rows;
    const bool ba = c.ptype == PF_BYTE_ARRAY && c.offsets && c.o_offsets;
    __shared__ uint32_t s_w[4];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t j0 = t * SEL_TILE;
        const int nj = int(nsel - j0 < int64_t(SEL_TILE) ? nsel - j0 : int64_t(SEL_TILE));
        if (c.values && c.o_values && c.width > 0) gather_values(c, rows, j0, nj);
        if (c.validity && c.o_validity) {
            // lane j tests source bit rows[j]; a ballot is one output word, its tail zero. No two waves share a word.
            const int64_t nbytes = (nsel + 7) >> 3;
            #pragma unroll 1
            for (int k = 0; k < SEL_WPW; k++) {
                const int word = wave * SEL_WPW + k;
                const int j = word * 64 + lane;
                bool bit = false;
                if (j < nj) {
                    const int32_t r = rows[j0 + j];
                    bit = (c.validity[r >> 3] >> (r & 7)) & 1;
                }
                const uint64_t w = __ballot(bit);
                if (lane == 0 && word * 64 < nj) {
                    const int64_t gw = j0 / 64 + word;
                    if (8 * gw + 8 <= nbytes) reinterpret_cast<uint64_t*>(c.o_validity)[gw] = w;
                    else for (int64_t b = 8 * gw; b < nbytes; b++) c.o_validity[b] = uint8_t(w >> (8 * (b - 8 * gw)));
                }
            }
        }
        if (ba) {
            // the lengths of the tile's values, scanned within the tile: o_offsets[j] = the chars before value j in
            // its tile (k_sel_chars adds the tile's base), and the tile's sum
            uint32_t len[SEL_RPT], sum = 0;
            #pragma unroll
            for (int q = 0; q < SEL_RPT; q++) {
                const int j = tid * SEL_RPT + q;
                len[q] = 0;
                if (j < nj) {
                    const int32_t r = rows[j0 + j];
                    len[q] = uint32_t(c.offsets[r + 1] - c.offsets[r]);
                }
                sum += len[q];
            }
            const uint32_t x = wave_scan(sum, lane);
            if (lane == 63) s_w[wave] = x;
            __syncthreads();
            uint32_t before = 0, total = 0;
            #pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t v = s_w[w];
                before += w < wave ? v : 0u;
                total += v;
            }
            uint32_t at = before + x - sum;
            #pragma unroll
            for (int q = 0; q < SEL_RPT; q++) {
                const int j = tid * SEL_RPT + q;
                if (j < nj) c.o_offsets[j0 + j] = int32_t(at);
                at += len[q];
            }
            if (tid == 0) f.ba_sum[blockIdx.y * f.tiles_cap + t] = total;
            __syncthreads();
        }
    }
}

// ---- k_sel_chars ---------------------------------------------------------------------------------------------------

// Grid (tiles, chunk), BYTE_ARRAY chunks. Lane j finishes offsets[j] and copies its value when that is short; a value
// of more than SEL_LONG bytes is handed to the whole wave, 64 bytes a round.
__global__ __launch_bounds__(SB) void k_sel_chars(SelBufs f) {
    const DevSelChunk c = f.sc[blockIdx.y];
    if (c.status != 0 || c.ptype != PF_BYTE_ARRAY || !c.offsets || !c.o_offsets) return;
    const int64_t nsel = f.head->rows_selected, ntiles = tiles_of(nsel);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0) c.o_offsets[nsel] = int32_t(f.ba_total[blockIdx.y]);   // (nsel = 0: offsets = {0})
    const int32_t* __restrict__ rows = f.rows;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t j0 = t * SEL_TILE;
        const int nj = int(nsel - j0 < int64_t(SEL_TILE) ? nsel - j0 : int64_t(SEL_TILE));
        const uint32_t tb = f.ba_base[blockIdx.y * f.tiles_cap + t];
        #pragma unroll 1
        for (int k = 0; k < SEL_WPW; k++) {
            const int j = (wave * SEL_WPW + k) * 64 + lane;
            uint32_t len = 0, src = 0, dst = 0;
            if (j < nj) {
                const int32_t r = rows[j0 + j];
                src = uint32_t(c.offsets[r]);
                len = uint32_t(c.offsets[r + 1]) - src;
                dst = uint32_t(c.o_offsets[j0 + j]) + tb;
                c.o_offsets[j0 + j] = int32_t(dst);
            }
            if (len <= SEL_LONG)
                for (uint32_t b = 0; b < len; b++) c.o_chars[dst + b] = c.chars[src + b];
            uint64_t big = __ballot(len > SEL_LONG);
            while (big) {   // (wave-uniform)
                const int l = __ffsll((unsigned long long)big) - 1;
                big &= big - 1;
                const uint32_t s = __shfl(src, l, 64), n = __shfl(len, l, 64), d = __shfl(dst, l, 64);
                for (uint32_t b = lane; b < n; b += 64) c.o_chars[d + b] = c.chars[s + b];
            }
        }
    }
}

// ---- k_sel_fin -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB) void k_sel_fin(SelBufs f) {
    DevSelChunk* o = &f.sc[blockIdx.x];
    const DevSelChunk c = *o;
    if (c.status != 0) return;
    const int64_t nsel = f.head->rows_selected;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ unsigned long long s_sum[4];
    unsigned long long nv = (unsigned long long)nsel;
    if (c.max_def > 0 && c.o_validity) {   // the present rows of the selection (tail bits are zero)
        const int64_t nbytes = (nsel + 7) >> 3, nwords = nbytes >> 3;
        const uint64_t* __restrict__ v = reinterpret_cast<const uint64_t*>(c.o_validity);
        unsigned long long sum = 0;
        for (int64_t i = tid; i < nwords; i += SB) sum += (unsigned long long)__popcll(v[i]);
        if (tid == 0)
            for (int64_t b = nwords * 8; b < nbytes; b++) sum += (unsigned long long)__popc(uint32_t(c.o_validity[b]));
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        nv = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    }
    if (tid == 0) {
        o->n_values = int64_t(nv);
        o->n_chars = c.ptype == PF_BYTE_ARRAY && c.o_offsets ? f.ba_total[blockIdx.x] : 0;
    }
}

}  // namespace

void launch_filter(const DevChunk* d_chunks, const DevChunkResult* d_res, const DevWinRes* d_wres, const SelBufs& f,
                   const SelDictBufs& fd, int n_chunks, int gather_grid, const uint8_t* chars_base, uint8_t* wchars_base,
                   int64_t out_delta, int64_t bits_delta, hipStream_t st) {
    if (f.n_preds <= 0 || n_chunks <= 0) return;
    const dim3 tiles(unsigned(f.tiles_cap < 1 ? 1 : f.tiles_cap)), per_chunk(unsigned(gather_grid < 1 ? 1 : gather_grid), unsigned(n_chunks));
    hipLaunchKernelGGL(k_sel_prep, dim3(1), dim3(SB), 0, st, d_chunks, d_res, d_wres, f, n_chunks, chars_base, wchars_base, out_delta,
                       bits_delta, fd.keep_of, fd.keeps);
    // predicates on kept chunks: matched once per dictionary entry, then looked up per row (pf_filter_dict.hip)
    if (fd.n_recs > 0) launch_sel_dict(f, fd, tiles.x, st);
    else hipLaunchKernelGGL(k_sel_mask, tiles, dim3(SB), 0, st, f);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(SB), 0, st, f.tile_count, f.tile_base, int64_t(0), f.head, 0,
                       static_cast<const DevSelChunk*>(nullptr), &f.head->rows_selected);
    hipLaunchKernelGGL(k_sel_rows, tiles, dim3(SB), 0, st, f);
    hipLaunchKernelGGL(k_sel_gather, per_chunk, dim3(SB), 0, st, f);
    hipLaunchKernelGGL(k_sel_scan, dim3(unsigned(n_chunks)), dim3(SB), 0, st, f.ba_sum, f.ba_base, f.tiles_cap, f.head, 1, f.sc,
                       f.ba_total);
    hipLaunchKernelGGL(k_sel_chars, per_chunk, dim3(SB), 0, st, f);
    hipLaunchKernelGGL(k_sel_fin, dim3(unsigned(n_chunks)), dim3(SB), 0, st, f);
}

}  // namespace pf
