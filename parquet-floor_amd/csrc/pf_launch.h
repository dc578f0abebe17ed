// pf_launch.h — the kernel launchers the runtime (pf_runtime.hip) calls. Included by every file
// that defines one, so a definition that drifts from its prototype does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include "pf_internal.h"
#include "pfloor.h"

namespace pf {

// pf_snappy.hip (launch_snappy_serial), pf_snappy_parse.hip (launch_snappy_parse), pf_snappy_exec.hip
// (launch_snappy_exec, launch_snappy), pf_snappy_exec2.hip (launch_snappy_exec2, diagnostics build)
void launch_snappy_serial(const SnappyJob* d_jobs, int n_jobs, const int* d_fallback, DevChunkResult* d_res, hipStream_t s);
void launch_snappy_parse(const SnappyJob* d_jobs, int n_jobs, const int2* d_wins, int n_wins, SnapWin* d_win, SnapEnt* d_ent,
                         uint32_t* d_lane_out, uint32_t* d_splits, int* d_fb, int max_nwin, hipStream_t s);
void launch_snappy_exec(const SnappyJob* d_jobs, int n_jobs, const int2* d_pieces, int n_pieces, uint32_t* d_splits, int* d_fb,
                        DevChunkResult* d_res, int exec, hipStream_t s);
void launch_snappy(const SnappyJob* d_jobs, int n_jobs, const int2* d_wins, int n_wins, SnapWin* d_win, SnapEnt* d_ent,
                   uint32_t* d_lane_out, const int2* d_pieces, int n_pieces, uint32_t* d_splits, int* d_fb,
                   DevChunkResult* d_res, int max_nwin, int exec, hipStream_t s);
#ifdef PF_DIAG
void launch_snappy_exec2(const SnappyJob* d_jobs, int n_jobs, const int2* d_pieces, int n_pieces, const uint32_t* d_splits,
                         int* d_fb, hipStream_t s);
#endif

// pf_zstd.hip
void launch_zstd(ZstdJob* d_jobs, const int* d_order, int n_jobs, uint8_t* d_lit, uint32_t lit_stride, DevChunkResult* d_res,
                 hipStream_t s);

// pf_lz4.hip
void launch_lz4(Lz4Job* d_jobs, const int* d_order, int n_jobs, DevChunkResult* d_res, hipStream_t s);

// pf_snappy_head.hip
void launch_snappy_head(SnappyJob* d_jobs, int n_jobs, DevPage* d_pages, const DevChunk* d_chunks, int* d_fb,
                        const DevChunkResult* d_res, hipStream_t st);
void launch_snappy_litcopy(const SnappyJob* d_jobs, const int* d_list, int n, const int* d_fb, hipStream_t st);

// pf_ba.hip
void launch_ba(BaJob* d_jobs, int n_jobs, const int2* d_tiles, int n_tiles, DevChunkResult* d_res, hipStream_t st,
               bool short_values);

// pf_flat_count.hip
void launch_runs(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, hipStream_t st);
void launch_count_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int n_flat, const int2* d_dblk,
                       int n_dblk, DevChunkResult* d_res, BaJob* d_bajobs, hipStream_t st);

// pf_flat_null.hip (launch_flat_null: called by launch_flat, first in the flat stage)
void launch_lvl(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, hipStream_t st,
                bool page_null, NullCaps nc);
void launch_flat_null(const DevChunk* d_chunks, DevPage* d_pages, const int2* blocks, int n4, int n8, int* d_fbq,
                      DevChunkResult* d_res, hipStream_t st, NullCaps nc, int stagger);

// pf_flat_dstr.hip (called by launch_flat, between k_flat_fixed and k_flat_all)
void launch_flat_dstr(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_dblk, int n_dblk, DevChunkResult* d_res,
                      hipStream_t st);

// pf_flat_ids.hip: kept-dictionary chunks (pf_decode_row_group_dict), at the end of the flat stage
void launch_flat_ids(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_blocks, int n_blocks, DevKeep* d_keeps, int n_keeps,
                     const int* d_keep_of, DevChunkResult* d_res, uint8_t* chars_arena, uint64_t arena_cap,
                     unsigned long long* arena_used, hipStream_t st);

// pf_flat.hip: the flat stage (what the runtime calls)
void launch_flat(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int nfix, int n, int n4, int n8, int* d_fbq,
                 const int2* d_dblk, int n_dblk, DevChunkResult* d_res, hipStream_t st, NullCaps nc, int stagger);

// pf_decode.hip
void launch_nest_lvl(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int max_nwin, DevChunkResult* d_res,
                     hipStream_t st, bool force_timeout);
void launch_count(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, BaJob* d_bajobs,
                  hipStream_t st, int idle_grid);
void launch_nest_count(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, const int2* d_segs, int n_segs,
                       DevChunkResult* d_res, hipStream_t st);
void launch_scan(DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, uint8_t* arena,
                 uint64_t cap, unsigned long long* used, hipStream_t st);
void launch_decode(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int n_first, DevChunkResult* d_res,
                   hipStream_t st, int idle_grid);
void launch_nest_decode(const DevChunk* d_chunks, DevPage* d_pages, const int2* d_segs, int n_segs, DevChunkResult* d_res,
                        hipStream_t st);

// pf_delta.hip
void launch_delta(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, int max_dbp_nwin, DevChunkResult* d_res,
                  hipStream_t st);
void launch_dlen(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, hipStream_t st);
void launch_dba_chars(const DevChunk* d_chunks, DevPage* d_pages, const int* d_list, int n, DevChunkResult* d_res, hipStream_t st);

// pf_window.hip: out_delta / bits_delta = twin arena base - decode arena base (bytes)
void launch_window(const DevChunk* d_chunks, const DevChunkResult* d_res, const DevWin* d_wins, DevWinRes* d_wres, int n_wins,
                   int copy_grid, const uint8_t* chars_base, uint8_t* wchars_base, int64_t out_delta, int64_t bits_delta,
                   const int* d_keep_of, const DevKeep* d_keeps, hipStream_t st);   // (the kept-dictionary tables, or null)

// pf_filter.hip: the filter stage's launch (SelBufs, SelDictBufs: pf_internal.h, laid out and bound by pf_result.cpp)
void launch_filter(const DevChunk* d_chunks, const DevChunkResult* d_res, const DevWinRes* d_wres, const SelBufs& f,
                   const SelDictBufs& fd, int n_chunks, int gather_grid, const uint8_t* chars_base, uint8_t* wchars_base,
                   int64_t out_delta, int64_t bits_delta, hipStream_t st);

// pf_filter_dict.hip: k_sel_dict and the mask pass that reads its bitmaps (called by launch_filter in place of k_sel_mask
// when a predicate is on a kept chunk)
void launch_sel_dict(const SelBufs& f, const SelDictBufs& fd, unsigned row_tiles, hipStream_t st);

// pf_scan.hip
void launch_page_scan(const ScanChunk* d_chunks, int n_chunks, pf_page_desc* d_pages, ScanCrc* d_crcs, ScanResult* d_res,
                      hipStream_t s);
void launch_page_crc(const ScanCrc* d_crcs, const int* d_list, int n, ScanResult* d_res, int32_t* d_bad, hipStream_t s);

}  // namespace pf
