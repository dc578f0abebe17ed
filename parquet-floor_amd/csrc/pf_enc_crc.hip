// pf_enc_crc.hip — write side of PageHeader.crc (PF_ENCODE_PAGE_CRC), gfx950.
//
// The stored bytes of a page are pieces that already lie in HBM when pf_encode_chunk has encoded them: the
// level stream, the values section (UNCOMPRESSED) or the outputs of its 8 KiB compression jobs, each in a
// slot of its own with its length in device memory. CRC-32 is linear (pf_crc.h), so
//   k_enc_crc   one 256-thread workgroup per piece: each thread takes a contiguous segment, computes its raw
//               CRC (zero init, table in LDS), shifts it to its place in the piece by a multiplication with
//               x^(8 * bytes after it) mod P, and the XOR of all of them (shuffles, then LDS) is the piece's
//               raw CRC; with it go the piece's length and x^(8 * length) mod P, which makes the host's fold
//               of a page's pieces one multiplication per piece.
// The method is k_page_crc's (pf_scan.hip), which verifies what this writes.
#include <hip/hip_runtime.h>

#include "pf_crc.h"
#include "pf_encode.h"

namespace pf {

namespace {
constexpr int CRC_NT = 256;
}

__global__ __launch_bounds__(CRC_NT) void k_enc_crc(const CrcPiece* __restrict__ pieces, CrcOut* __restrict__ out) {
    __shared__ uint32_t table[256];
    __shared__ uint32_t x2n[32];
    __shared__ uint32_t red[CRC_NT / 64];
    const CrcPiece pc = pieces[blockIdx.x];
    const int tid = threadIdx.x;
    {
        uint32_t c = uint32_t(tid);
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        table[tid] = c;
    }
    if (tid == 0) crc_x2n_table(x2n);
    __syncthreads();
    // a job's length is where the compressor left it; never past the piece's capacity
    const uint32_t len = min(pc.len_ptr ? *pc.len_ptr : pc.len, pc.cap);
    const uint32_t seg = (len + CRC_NT - 1) / CRC_NT;
    const uint32_t b0 = min(len, uint32_t(tid) * seg), b1 = min(len, b0 + seg);
    const uint8_t* g = pc.ptr;
    uint32_t c = 0;   // raw CRC (zero init, no final xor): linear in the data
    for (uint32_t i = b0; i < b1; i++) c = table[(c ^ g[i]) & 0xffu] ^ (c >> 8);
    uint32_t part = b1 > b0 ? crc_mulmod(crc_x8n(len - b1, x2n), c) : 0u;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part ^= uint32_t(__shfl_xor(part, d, 64));
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        uint32_t raw = 0;
        for (int w = 0; w < CRC_NT / 64; w++) raw ^= red[w];
        out[blockIdx.x] = CrcOut{raw, len, crc_x8n(len, x2n), 0u};
    }
}

void launch_enc_crc(const CrcPiece* d_pieces, int n_pieces, CrcOut* d_out, hipStream_t st) {
    if (n_pieces > 0) hipLaunchKernelGGL(k_enc_crc, dim3(n_pieces), dim3(CRC_NT), 0, st, d_pieces, d_out);
}

}  // namespace pf
