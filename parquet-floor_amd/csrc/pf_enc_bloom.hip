// pf_enc_bloom.hip — the split-block Bloom filter of a column chunk (pf_encode_column.bloom_bytes),
// gfx950. Over the dense values pf_encode_chunk already holds in HBM (EncArgs::dense, or dsrc / dlen + chars):
// null rows are not among them, so they are never inserted.
//
//   k_enc_bloom   one lane per dense value: XXH64 (seed 0) of its PLAIN bytes -- the closed form for 4- and 8-byte
//                 values, the general function for strings (a serial chain per value, so a value is one lane's) --
//                 then the hash's block and its eight words, one bit each, set with atomicOr (relaxed, agent scope,
//                 no return value) in the zeroed filter. With `first_only` (the chunk ended dictionary-encoded) only
//                 the first occurrence of every value (EncArgs::mark) is hashed: the same set of values, D hashes
//                 instead of m.
// OR is commutative and idempotent: the filter depends on the set of values and its size alone, not on the order
// workgroups run in nor on how the chunk is encoded.
#include <hip/hip_runtime.h>

#include "pf_encode.h"
#include "pf_xxh64.h"

namespace pf {

namespace {
constexpr int BL_NT = 256;
}

__global__ __launch_bounds__(BL_NT) void k_enc_bloom(EncArgs a, uint32_t m, uint32_t* __restrict__ filter, uint32_t n_blocks,
                                                     int first_only) {
    const uint64_t d = uint64_t(blockIdx.x) * BL_NT + threadIdx.x;
    if (d >= m) return;
    if (first_only && !a.mark[d]) return;
    uint64_t h;
    if (a.ptype == PF_BYTE_ARRAY) h = xxh64(a.chars + a.dsrc[d], a.dlen[d], 0);
    else if (a.width == 4) h = xxh64_u32(reinterpret_cast<const uint32_t*>(a.dense)[d], 0);
    else h = xxh64_u64(reinterpret_cast<const uint64_t*>(a.dense)[d], 0);
    uint32_t* blk = filter + uint64_t(bloom_block(h, n_blocks)) * 8u;
    #pragma unroll
    for (int i = 0; i < 8; i++)
        (void)__hip_atomic_fetch_or(blk + i, bloom_mask(h, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `filter`: bloom_bytes zeroed bytes (a power of two >= 32). Fixed-width values of 4 or 8 bytes, or strings.
void enc_bloom(const EncArgs& a, uint32_t m, uint32_t* filter, uint32_t bloom_bytes, bool first_only, hipStream_t st) {
    if (!m) return;
    hipLaunchKernelGGL(k_enc_bloom, dim3((m + BL_NT - 1) / BL_NT), dim3(BL_NT), 0, st, a, m, filter, bloom_bytes / 32u,
                       first_only ? 1 : 0);
}

}  // namespace pf
