// pf_enc_plan.h — host-only planning of one chunk's encode (pf_enc_plan.cpp), the write side's pf_plan.h.
// Plain C++: no HIP call, no context; it reads the pf_encode_column fields and the host copies of validity
// and offsets the runtime makes anyway, so every decision of pf_encode_chunk that is not a launch can be
// checked without a GPU (tests/native/pf_enc_plan_check.cpp). The steps, split where the host has to wait
// for the device (pf_enc_runtime.hip runs what lies between them):
//
//   plan_encode     arguments -> settings, page plan, delta / statistics / page-index tables
//   layout_encode   the work arena as named regions (after enc_scan_temp, a HIP call, gave temp_bytes)
//   bind_encode     regions -> EncArgs, DeltaArgs, StatArgs, PgIndexArgs, HybridArgs
//   plan_values     the dictionary's three words -> fallback, dict, bit width, encoding, hybrid streams
//   plan_sections   the size pass's bytes -> values sections, EncPage entries, levels' placement
//   plan_crc_levels the level pieces of the page CRCs
//   plan_compress   sections -> compression jobs, slots and the one block that comes back (bind_compress: pointers)
//   assemble_chunk  bodies, levels, CRC pieces, statistics -> page headers + bodies and pf_encoded_chunk
//
// A step that fails returns the status code and sets *why to the text of pf_last_error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "pf_enc_tables.h"
#include "pf_plan.h"
#include "pfloor.h"

namespace pf {

size_t uvarint_len(uint64_t v);
void put_uvarint(std::vector<uint8_t>& o, uint64_t v);
// Bytes the host puts in front of a section's jobs: Snappy's length varint, or ZSTD's frame header (and for
// a section of 0 bytes, which has no job, the one empty last raw block).
size_t stream_head(int codec, uint64_t n, uint8_t* o /* 12 bytes */);

// Upper bound of a hybrid stream of `cnt` entries at bit width `bw` (an element is at most a 5-byte varint
// and the value, or a header and a group): what the non-delta hybrid route reserves before the size pass.
uint64_t hybrid_worst(uint64_t cnt, uint32_t bw);

// A data page: rows [r0, r1), dense (present) values [d0, d0 + cnt), PLAIN bytes of its values section.
struct EncPagePlan {
    int64_t r0, r1;
    uint32_t d0, cnt;
    uint64_t plain;
};

// The regions of the work arena (d_enc), in the order they lie in it.
enum EncRegion {
    R_IN, R_VL, R_OF, R_CH,                                    // host inputs: values, validity, offsets, chars
    R_FLAG, R_POS, R_DENSE, R_DSRC, R_DLEN, R_VSZ, R_VPRE,
    R_KEY, R_SKEY, R_DIDX, R_SIDX, R_HP, R_HEAD, R_MARK, R_DID, R_DSZ, R_DOFF, R_IDS, R_COL,
    R_PFX, R_SFX, R_SPRE, R_DSTR, R_DPG, R_DBY, R_DOF, R_DMIN, R_DWD, R_DTOT,   // DELTA_*
    R_HSTR, R_HBY,                                             // hybrid streams and their bytes
    R_STT, R_STP, R_SPART, R_SWIN, R_SOUT, R_SBYTES,           // statistics
    R_XIN, R_XNN, R_XOUT,                                      // page index
    R_TEMP, R_BLOOM,
    N_ENC_REGIONS
};
struct Region {
    size_t off = 0, size = 0;   // size 0: absent (only R_BLOOM); a region a route does not use has size 1
};

// Compression of a set of sections: jobs of SC_BLOCK / ZC_BLOCK bytes, their slots in d_enc_out, and the
// block [lengths | CrcOut[]] one D2H brings back.
struct CompressPlan {
    int codec = 0;
    uint32_t JOB = 0, SLOT = 0;
    std::vector<CompJob> jobs;                         // len / last planned, src / dst bound
    std::vector<uint64_t> src_off;                     // a job's input, relative to the sections' base
    std::vector<std::pair<size_t, size_t>> range;      // jobs of each section
    size_t np = 0;                                     // CRC pieces: the jobs, then the caller's extra ones
    size_t o_jobs = 0, o_len = 0, o_pieces = 0, o_slots = 0, arena = 0;
    size_t o_crc_in_len = 0, len_bytes = 0;            // CrcOut[np] at o_len + o_crc_in_len; bytes of the one D2H
    std::vector<CrcPiece> pieces;                      // bound; alive until the synchronisation its upload waits for
};
void plan_compress(const std::vector<std::pair<uint64_t, uint64_t>>& sections, int codec, bool want_crc, size_t n_extra,
                   CompressPlan& cp);
void bind_compress(CompressPlan& cp, const uint8_t* base, uint8_t* arena, const std::vector<CrcPiece>* extra);

struct EncPlan {
    // ---- plan_encode: settings ----
    int pt = 0, w = 0, max_def = 0, codec = 0, bits = 0;
    int64_t n = 0, page_rows = 0, dict_limit = 0, chars_len = 0;
    bool compressed = false, str = false, has_val = false;
    bool dict_bit = false, delta_bit = false, hyb = false, want_stats = false, want_crc = false, want_index = false;
    bool run_stats = false, dict_fits32 = true;
    uint32_t px_trunc = 0;
    size_t bloom = 0, vbytes = 0;
    // page plan and tables
    std::vector<EncPagePlan> pp;
    uint32_t m = 0;                        // present values
    std::vector<DeltaStream> dstreams;     // + the sentinel (item0 = n_items); src bound
    std::vector<DeltaPage> dpages;
    uint32_t n_items = 0;
    size_t n_hs_max = 0;
    std::vector<StatTile> stiles;
    std::vector<uint32_t> sptile;
    size_t n_se = 0;                       // statistics entries: the pages, then the chunk
    size_t n_px = 0, px_nc = 0, px_off = 0, px_np = 0, px_val = 0, px_bytes = 0;
    uint64_t px_cap = 0;
    std::vector<uint32_t> px_in;           // rows of every page, then its present values (uploaded)
    size_t scan_elems = 0;                 // elements of the longest scan: what enc_scan_temp is asked for
    // ---- layout_encode ----
    Region reg[N_ENC_REGIONS];
    size_t a_sz = 0, temp_bytes = 0;
    // ---- bind_encode ----
    EncArgs ea{};
    DeltaArgs da{};
    StatArgs sa{};
    PgIndexArgs xa{};
    HybridArgs ha{};
    void* temp = nullptr;
    uint8_t* d_bloom = nullptr;
    // ---- plan_values ----
    bool want_dict = false, dict = false, brle = false, delta = false;
    int fallback = 0, data_enc = 0;
    uint32_t D = 0, dict_bytes = 0, bw = 1;
    std::vector<HybridStream> hs;          // uploaded twice: for the size pass, and with out_off for the write pass
    std::vector<int> lv_of, vs_of;         // a page's level / value stream (-1: none)
    size_t ub = 0;                         // hybrid, not delta: what d_enc_sec reserves before the size pass
    // ---- the size passes' results (D2H targets) ----
    std::vector<uint32_t> hbytes;          // bytes of every hybrid stream
    std::vector<uint32_t> htot;            // bytes of every delta page's values section
    // ---- plan_sections ----
    std::vector<std::pair<uint64_t, uint64_t>> sections;   // [dictionary page | page 0 | page 1 | ...]: (offset, bytes) in d_enc_sec
    std::vector<EncPage> ep;
    std::vector<size_t> lv_off;            // a page's levels, relative to o_lv
    size_t o_dict = 0, o_lv = 0, lv_total = 0, o_pages = 0, vo = 0;
    // ---- plan_crc_levels ----
    std::vector<CrcPiece> lv_pieces;
    std::vector<int> lv_piece;             // the page's whole level stream
    std::vector<int> vb_piece;             // the whole bytes of its bit-packed run, between header and last partial byte
    // ---- compression / CRC tables (alive until the synchronisation their uploads wait for) ----
    CompressPlan comp;
    std::vector<CrcPiece> sec_pieces;      // UNCOMPRESSED: the sections, then the levels
    size_t o_crc_res = 0;                  // ... and where their CrcOut[] lie in d_enc_out
};

// The argument checks that need neither validity nor offsets (the runtime makes its host copies after them).
int check_encode_args(const pf_encode_column* col, const char** why);
int plan_encode(const pf_encode_column* col, const std::vector<uint8_t>& hval, const std::vector<int32_t>& hoff, EncPlan& p,
                const char** why);
void layout_encode(EncPlan& p, size_t temp_bytes);
// `arena`: where the regions lie; the input pointers of `col` are used as they are when on_device.
void bind_encode(EncPlan& p, uint8_t* arena, const pf_encode_column* col, bool on_device);
// collide, D, dict_bytes_dev: the three words the dictionary kernels leave (ignored unless p.want_dict).
void plan_values(EncPlan& p, uint32_t collide, uint32_t D, uint32_t dict_bytes_dev);
int plan_sections(EncPlan& p, const char** why);
void plan_crc_levels(EncPlan& p, const uint8_t* sec);
// UNCOMPRESSED with page CRCs: the sections and the levels as pieces of `sec`.
int plan_section_pieces(EncPlan& p, const uint8_t* sec, const char** why);

// What the device sent back, and where the assembled chunk goes (vectors the caller owns: pf_encoded_chunk
// points into them).
struct AssembleIn {
    const std::vector<uint8_t>* hval;
    const std::vector<std::vector<uint8_t>>* bodies;   // per section, as stored
    const uint8_t* hlv;                                // lv_total bytes of hybrid levels
    const CrcOut* crcs;                                // jobs (SNAPPY, ZSTD) or sections first, then the levels
    size_t crc_first_lv;
    const StatPart* hst;                               // n_se results, or nullptr
    const uint8_t* hsb;                                // strings: n_se x ST_LIMIT
    const uint8_t* px;                                 // the page index block, or nullptr
    const uint8_t* bloom;                              // the filter's bitset, or nullptr
};
struct AssembledChunk {
    std::vector<uint8_t>* bytes;
    std::vector<uint8_t>* stat;
    std::vector<int64_t>* pgoff;
    std::vector<int64_t>* pgrow;
    std::vector<int32_t>* pgsize;
};
// Fills every field of `out` but the event timers (snappy_ms, encode_ms, bloom_ms are set to 0).
int assemble_chunk(const EncPlan& p, const AssembleIn& in, AssembledChunk& ac, pf_encoded_chunk* out, const char** why);

}  // namespace pf
