// pf_encode.h — launchers of the write path (pf_encode.hip, pf_enc_*.hip <-> pf_enc_runtime.hip). Their
// tables are plain data in pf_enc_tables.h, which the host planner shares. Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_enc_tables.h"
#include "pfloor.h"

namespace pf {

// ---- DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY pages (pf_enc_delta.hip) ----
hipError_t enc_delta_prefix(const EncArgs& a, const DeltaArgs& t, uint32_t m, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t enc_delta_sizes(const DeltaArgs& t, void* temp, size_t temp_bytes, hipStream_t st);
void enc_delta_write(const EncArgs& a, const DeltaArgs& t, uint32_t m, hipStream_t st);

// ---- RLE / bit-packed hybrid streams in parquet-mr's run shape (pf_enc_hybrid.hip) ----
hipError_t enc_hybrid_sizes(const HybridArgs& t, hipStream_t st);
void enc_hybrid_write(const HybridArgs& t, hipStream_t st);

// ---- page and chunk statistics (pf_enc_stats.hip; PF_ENCODE_STATISTICS) ----
void enc_stats(const EncArgs& a, const StatArgs& s, hipStream_t st);

// ---- page index (pf_enc_pgindex.hip; PF_ENCODE_PAGE_INDEX) ----
void enc_pgindex(const EncArgs& a, const PgIndexArgs& x, hipStream_t st);

// ---- page CRCs (pf_enc_crc.hip; PF_ENCODE_PAGE_CRC) ----
void launch_enc_crc(const CrcPiece* d_pieces, int n_pieces, CrcOut* d_out, hipStream_t st);

// ---- split-block Bloom filter (pf_enc_bloom.hip; pf_encode_column.bloom_bytes) ----
// `filter`: bloom_bytes zeroed bytes, a power of two >= 32. first_only: hash only the dense values with mark set
// (a dictionary-encoded chunk's first occurrences).
void enc_bloom(const EncArgs& a, uint32_t m, uint32_t* filter, uint32_t bloom_bytes, bool first_only, hipStream_t st);

hipError_t enc_scan_temp(size_t n, size_t& bytes);
hipError_t enc_dense(const EncArgs& a, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t enc_plain_sizes(const EncArgs& a, uint32_t m, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t enc_dictionary(const EncArgs& a, uint32_t m, int key_bits, void* temp, size_t temp_bytes, hipStream_t st);
void enc_dictionary_page_and_ids(const EncArgs& a, uint32_t m, hipStream_t st);
void enc_pages(const EncArgs& a, const EncPage* d_pages, int n_pages, hipStream_t st);
void launch_snappy_compress(const SnapCJob* d_jobs, int n_jobs, uint32_t* d_out_len, hipStream_t st);
void launch_zstd_compress(const ZstdCJob* d_jobs, int n_jobs, uint32_t* d_out_len, hipStream_t st);

}  // namespace pf
