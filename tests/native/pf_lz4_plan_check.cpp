// pf_lz4_plan_check — the host planner (csrc/pf_plan.cpp) on LZ4_RAW chunks, without a GPU: hand-made
// descriptors, bound to made-up arena addresses. Built by tests/test_lz4_plan.py with g++ under
// AddressSanitizer + UBSan.
//  * an LZ4_RAW chunk gets one job per compressed page; the page bodies are aligned, disjoint and
//    inside the scratch arena, the jobs point into the input and the scratch arena, L_LZ4 is a
//    permutation of the jobs ordered by compressed bytes;
//  * more jobs than k_lz4 has workgroups plan like any other number;
//  * in a batch that mixes LZ4_RAW, ZSTD, Snappy and uncompressed chunks each job list holds only
//    its codec, and the Snappy and ZSTD side is that of the batch without the LZ4_RAW chunk;
//  * v2 pages with is_compressed = 0 get no job, nor does a page of no bytes on either side; a
//    page of bytes that has to produce none gets one;
//  * GZIP and the Hadoop-framed LZ4 (codec 5) still fail with -4 and take nothing with them.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_plan.h"

using namespace pf;

namespace {
int g_fail = 0;
void check(bool ok, const char* fmt, ...) {
    if (ok) return;
    g_fail++;
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}

const ArenaBases BASES{0x10000000100ull, 0x20000000100ull, 0x30000000100ull, 0x40000000100ull, 0x50000000100ull, 0x60000000100ull};

struct Chunk {
    pf_chunk_desc d{};
    std::vector<pf_page_desc> pages;
};
Chunk chunk(int ptype, int max_def, int codec) {
    Chunk c;
    c.d.physical_type = ptype; c.d.max_def = max_def; c.d.codec = codec;
    return c;
}
pf_page_desc page(int type, int nv, uint32_t comp, uint32_t uncomp, int is_compressed = 1, int def_bytes = 0) {
    pf_page_desc d{};
    d.page_type = type; d.encoding = PF_ENC_PLAIN; d.def_encoding = PF_ENC_RLE; d.rep_encoding = PF_ENC_RLE;
    d.num_values = nv; d.compressed_size = comp; d.uncompressed_size = uncomp; d.num_nulls = -1;
    d.is_compressed = is_compressed; d.def_bytes = def_bytes;
    return d;
}
std::vector<pf_chunk_desc> layout(std::vector<Chunk>& cs, size_t& n_bytes) {
    std::vector<pf_chunk_desc> out;
    uint64_t off = 0;
    for (Chunk& c : cs) {
        uint64_t in = 0;
        for (pf_page_desc& pd : c.pages) { pd.offset = in + 40; in = pd.offset + pd.compressed_size; }
        c.d.n_pages = int(c.pages.size());
        c.d.pages = c.pages.data();
        c.d.chunk_offset = off;
        c.d.chunk_size = in;
        off += align_up(in, 256);
        out.push_back(c.d);
    }
    n_bytes = off;
    return out;
}
void plan(std::vector<Chunk>& cs, BatchPlan& p, size_t& n_bytes) {
    const std::vector<pf_chunk_desc> cds = layout(cs, n_bytes);
    plan_batch(cds.data(), int(cds.size()), n_bytes, PfOpts{}, p);
    bind_batch(p, BASES);
}

struct Region {
    uint64_t off, len;
};
void check_lz4(const BatchPlan& p, size_t n_bytes, const char* name) {
    std::vector<Region> rs;
    for (size_t i = 0; i < p.pages.size(); i++)
        if (p.pplan[i].scratch_off != NO_OFF) {
            check(p.pplan[i].scratch_off % 16 == 0, "%s: page %zu body not 16-byte aligned", name, i);
            rs.push_back(Region{p.pplan[i].scratch_off, p.pages[i].body_len});
        }
    if (uint64_t(p.zstd_grid) * p.zlit_stride) rs.push_back(Region{p.off_zlit, uint64_t(p.zstd_grid) * p.zlit_stride});
    if (p.npub_bytes) rs.push_back(Region{p.off_npub, p.npub_bytes});
    for (size_t a = 0; a < rs.size(); a++) {
        check(rs[a].off + rs[a].len <= p.scratch_bytes, "%s: region %zu outside the scratch arena", name, a);
        for (size_t b = a + 1; b < rs.size(); b++)
            check(rs[a].off + rs[a].len <= rs[b].off || rs[b].off + rs[b].len <= rs[a].off || !rs[a].len || !rs[b].len,
                  "%s: regions %zu and %zu overlap", name, a, b);
    }
    std::vector<char> seen(p.ljobs.size(), 0);
    check(p.lists[L_LZ4].size() == p.ljobs.size(), "%s: L_LZ4 length", name);
    for (size_t k = 0; k < p.lists[L_LZ4].size(); k++) {
        const int j = p.lists[L_LZ4][k];
        const bool in_range = j >= 0 && size_t(j) < p.ljobs.size();
        check(in_range && !seen[size_t(in_range ? j : 0)], "%s: L_LZ4 is not a permutation", name);
        if (!in_range) continue;
        seen[size_t(j)] = 1;
        if (k) check(p.ljobs[size_t(p.lists[L_LZ4][k - 1])].src_len >= p.ljobs[size_t(j)].src_len, "%s: dispatch order", name);
    }
    std::vector<char> has_job(p.pages.size(), 0);
    for (const Lz4Job& jb : p.ljobs) {
        const DevPage& pg = p.pages[size_t(jb.page)];
        const uintptr_t s = reinterpret_cast<uintptr_t>(jb.src), d = reinterpret_cast<uintptr_t>(jb.dst);
        check(s >= BASES.in && s + jb.src_len <= BASES.in + n_bytes, "%s: job source outside the input", name);
        check(d >= BASES.scratch && d + jb.dst_len <= BASES.scratch + p.scratch_bytes, "%s: job destination outside scratch", name);
        check(jb.dst == pg.body && jb.dst_len == pg.body_len && (pg.flags & PG_COMPRESSED), "%s: job and page disagree", name);
        check(p.chunks[size_t(jb.chunk)].codec == PF_CODEC_LZ4_RAW && pg.chunk == jb.chunk, "%s: job of a chunk that is not LZ4_RAW", name);
        check(jb.src_len || jb.dst_len, "%s: a job without bytes on either side", name);
        check(!has_job[size_t(jb.page)], "%s: two jobs of one page", name);
        has_job[size_t(jb.page)] = 1;
    }
    for (size_t i = 0; i < p.pages.size(); i++) {   // every compressed page of an LZ4_RAW chunk that has bytes has its job
        const DevPage& pg = p.pages[i];
        if (p.chunks[size_t(pg.chunk)].codec != PF_CODEC_LZ4_RAW) continue;
        if (!(pg.flags & PG_COMPRESSED)) check(!has_job[i], "%s: stored page %zu has a job", name, i);
        if ((pg.flags & PG_COMPRESSED) && pg.body_len) check(bool(has_job[i]), "%s: compressed page %zu has no job", name, i);
    }
    for (const SnappyJob& jb : p.jobs) check(p.chunks[size_t(jb.chunk)].codec == PF_CODEC_SNAPPY, "%s: Snappy job of another codec", name);
    for (const ZstdJob& jb : p.zjobs) check(p.chunks[size_t(jb.chunk)].codec == PF_CODEC_ZSTD, "%s: ZSTD job of another codec", name);
    check(p.off_ljobs % 256 == 0 && p.off_ljobs + sizeof(Lz4Job) * p.ljobs.size() <= p.meta_bytes - 256, "%s: jobs outside the metadata block", name);
    check(p.off_ljobs >= p.off_zjobs + sizeof(ZstdJob) * p.zjobs.size(), "%s: LZ4 jobs over the ZSTD jobs", name);
    check(p.list_base[N_LISTS] - p.list_base[L_LZ4] == p.ljobs.size(), "%s: L_LZ4 is not the last list of the block", name);
}

Chunk coded_chunk(int codec) {   // dictionary page, v1 page, v2 pages compressed and stored, a 400 KB page
    Chunk c = chunk(PF_INT64, 1, codec);
    c.pages.push_back(page(PF_PAGE_DICTIONARY, 100, 300, 800));
    c.pages.push_back(page(PF_PAGE_DATA, 1000, 777, 8013));
    c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 900, 8010, 1, 10));
    c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 8010, 8010, 0, 10));
    c.pages.push_back(page(PF_PAGE_DATA, 50000, 123457, 400013));
    return c;
}
Chunk snappy_chunk(int nv) {
    Chunk c = chunk(PF_INT32, 0, PF_CODEC_SNAPPY);
    c.pages.push_back(page(PF_PAGE_DATA, nv, 3u * uint32_t(nv), 4u * uint32_t(nv)));
    c.pages.push_back(page(PF_PAGE_DATA, nv, 5u * uint32_t(nv), 4u * uint32_t(nv)));
    return c;
}
Chunk plain_chunk() {
    Chunk c = chunk(PF_DOUBLE, 0, PF_CODEC_UNCOMPRESSED);
    c.pages.push_back(page(PF_PAGE_DATA, 3000, 24000, 24000));
    return c;
}
}  // namespace

int main() {
    size_t n = 0;
    {   // one LZ4_RAW chunk
        std::vector<Chunk> cs{coded_chunk(PF_CODEC_LZ4_RAW)};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0, "lz4 chunk does not plan: %lld", (long long)p.host_status[0]);
        check(p.ljobs.size() == 4 && p.jobs.empty() && p.zjobs.empty(), "lz4 chunk: %zu lz4 jobs, %zu snappy jobs, %zu zstd jobs",
              p.ljobs.size(), p.jobs.size(), p.zjobs.size());
        if (p.host_status[0] == 0 && p.ljobs.size() == 4) {
            check(!(p.pages[3].flags & PG_COMPRESSED) && p.pplan[3].scratch_off == NO_OFF && p.pages[3].body_len == 8000, "stored v2 page");
            check(p.pages[2].body_len == 8000 && p.ljobs[2].src_len == 890 && p.ljobs[2].dst_len == 8000, "v2 level bytes stay outside the block");
            check(p.ljobs[1].src_len == 777 && p.ljobs[1].dst_len == 8013, "v1 page: the whole body is the block");
            check(p.lists[L_LZ4].size() == 4 && p.lists[L_LZ4][0] == 3, "largest page first");
            check(p.zstd_grid == 0 && p.zlit_stride == 0, "an LZ4 batch has no ZSTD literal area");
        }
        check_lz4(p, n, "lz4");
    }
    {   // more jobs than workgroups
        Chunk c = chunk(PF_INT32, 0, PF_CODEC_LZ4_RAW);
        for (int i = 0; i < LZ4_GRID + 90; i++) c.pages.push_back(page(PF_PAGE_DATA, 500, 600 + uint32_t(i % 7), 2000));
        std::vector<Chunk> cs{c};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0 && p.ljobs.size() == size_t(LZ4_GRID + 90), "many: %zu jobs", p.ljobs.size());
        check_lz4(p, n, "many");
    }
    {   // mixed batch against the same batch without the LZ4_RAW chunk
        std::vector<Chunk> with{snappy_chunk(5000), coded_chunk(PF_CODEC_LZ4_RAW), coded_chunk(PF_CODEC_ZSTD), plain_chunk(), snappy_chunk(70000)};
        std::vector<Chunk> without{snappy_chunk(5000), coded_chunk(PF_CODEC_ZSTD), plain_chunk(), snappy_chunk(70000)};
        BatchPlan a, b;
        size_t na = 0, nb = 0;
        plan(with, a, na);
        plan(without, b, nb);
        for (size_t c = 0; c < with.size(); c++) check(a.host_status[c] == 0, "mixed: chunk %zu does not plan", c);
        check_lz4(a, na, "mixed");
        check_lz4(b, nb, "no lz4");
        check(a.ljobs.size() == 4 && a.zjobs.size() == 4 && a.jobs.size() == 4, "mixed: %zu / %zu / %zu jobs", a.ljobs.size(), a.zjobs.size(), a.jobs.size());
        check(b.ljobs.empty() && b.lists[L_LZ4].empty(), "no lz4: a job");
        check(a.jobs.size() == b.jobs.size() && a.snap.n_splits == b.snap.n_splits && a.snap.wins.size() == b.snap.wins.size() &&
                  a.snap.pieces.size() == b.snap.pieces.size() && a.snap.tokmap_bytes == b.snap.tokmap_bytes, "mixed: Snappy tables changed");
        check(a.zjobs.size() == b.zjobs.size() && a.zstd_grid == b.zstd_grid && a.zlit_stride == b.zlit_stride && a.lists[L_ZSTD] == b.lists[L_ZSTD],
              "mixed: ZSTD side changed");
        check(a.lists[L_DJOBS] == b.lists[L_DJOBS], "mixed: litcopy list changed");
    }
    {   // pages without bytes: 0 -> 0 gets no job (an all-null v2 page flagged compressed), n -> 0 gets one
        Chunk c = chunk(PF_INT32, 1, PF_CODEC_LZ4_RAW);
        c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 10, 10, 1, 10));     // levels only on both sides
        c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 11, 10, 1, 10));     // one byte (`00`) that produces none
        c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 500, 4010, 1, 10));
        c.pages[0].num_nulls = c.pages[1].num_nulls = 1000;
        std::vector<Chunk> cs{c};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0, "empty pages: %lld", (long long)p.host_status[0]);
        check(p.ljobs.size() == 2, "empty pages: %zu jobs", p.ljobs.size());
        if (p.ljobs.size() == 2) {
            check(p.ljobs[0].page == 1 && p.ljobs[0].src_len == 1 && p.ljobs[0].dst_len == 0, "empty pages: the 1 -> 0 job");
            check(p.ljobs[1].page == 2 && p.ljobs[1].src_len == 490 && p.ljobs[1].dst_len == 4000, "empty pages: the data job");
        }
        check_lz4(p, n, "empty pages");
    }
    for (int codec : {int(PF_CODEC_GZIP), int(PF_CODEC_LZ4), int(PF_CODEC_LZO), int(PF_CODEC_BROTLI)}) {   // still refused, taking nothing with them
        std::vector<Chunk> cs{coded_chunk(codec), coded_chunk(PF_CODEC_LZ4_RAW)};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == PF_ERR_UNSUPPORTED_CODEC && p.host_status[1] == 0, "codec %d: %lld %lld", codec, (long long)p.host_status[0],
              (long long)p.host_status[1]);
        check(p.ljobs.size() == 4 && p.jobs.empty() && p.zjobs.empty() && p.pages.size() == 5, "codec %d: jobs or pages of the refused chunk", codec);
        check_lz4(p, n, "refused codec");
    }
    {   // a chunk that fails after its jobs were made loses them
        Chunk bad = coded_chunk(PF_CODEC_LZ4_RAW);
        bad.pages.push_back(page(PF_PAGE_DATA, -5, 10, 10));
        std::vector<Chunk> cs{coded_chunk(PF_CODEC_LZ4_RAW), bad};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0 && p.host_status[1] == PF_ERR_CORRUPT_PAGE && p.ljobs.size() == 4, "failed chunk keeps jobs");
        check_lz4(p, n, "failed chunk");
    }
    std::printf("lz4 plan check: failures %d\n", g_fail);
    return g_fail ? 1 : 0;
}
