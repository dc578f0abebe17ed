// pf_zstd_plan_check — the host planner (csrc/pf_plan.cpp) on ZSTD chunks, without a GPU: hand-made
// descriptors, bound to made-up arena addresses. Built by tests/test_zstd_plan.py with g++ under
// AddressSanitizer + UBSan.
//  * a ZSTD chunk's regions (page bodies, literal areas) are aligned, disjoint and inside the arenas,
//    its jobs point into the input and the scratch arena;
//  * the literal areas are per resident workgroup: min(jobs, ZSTD_GRID) of them, not one per page;
//  * a batch that mixes ZSTD, Snappy and uncompressed chunks has the Snappy tables of the batch
//    without the ZSTD chunk; a batch without ZSTD has no ZSTD job and no literal area;
//  * v2 pages with is_compressed = 0 get no job; a GZIP chunk still fails with -4.
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
void check_zstd(const BatchPlan& p, size_t n_bytes, const char* name) {
    std::vector<Region> rs;
    for (size_t i = 0; i < p.pages.size(); i++)
        if (p.pplan[i].scratch_off != NO_OFF) {
            check(p.pplan[i].scratch_off % 16 == 0, "%s: page %zu body not 16-byte aligned", name, i);
            rs.push_back(Region{p.pplan[i].scratch_off, p.pages[i].body_len});
        }
    const uint64_t lit_bytes = uint64_t(p.zstd_grid) * p.zlit_stride;
    check(p.zstd_grid == std::min<size_t>(p.zjobs.size(), size_t(ZSTD_GRID)), "%s: grid %u for %zu jobs", name, p.zstd_grid, p.zjobs.size());
    if (lit_bytes) {
        check(p.off_zlit % 256 == 0 && p.zlit_stride % 256 == 0, "%s: literal areas not 256-byte aligned", name);
        rs.push_back(Region{p.off_zlit, lit_bytes});
    }
    if (p.npub_bytes) rs.push_back(Region{p.off_npub, p.npub_bytes});
    for (size_t a = 0; a < rs.size(); a++) {
        check(rs[a].off + rs[a].len <= p.scratch_bytes, "%s: region %zu outside the scratch arena", name, a);
        for (size_t b = a + 1; b < rs.size(); b++)
            check(rs[a].off + rs[a].len <= rs[b].off || rs[b].off + rs[b].len <= rs[a].off || !rs[a].len || !rs[b].len,
                  "%s: regions %zu and %zu overlap", name, a, b);
    }
    uint32_t max_dst = 0;
    std::vector<char> seen(p.zjobs.size(), 0);
    check(p.lists[L_ZSTD].size() == p.zjobs.size(), "%s: L_ZSTD length", name);
    for (size_t k = 0; k < p.lists[L_ZSTD].size(); k++) {
        const int j = p.lists[L_ZSTD][k];
        check(j >= 0 && size_t(j) < p.zjobs.size() && !seen[size_t(j)], "%s: L_ZSTD is not a permutation", name);
        if (j >= 0 && size_t(j) < seen.size()) seen[size_t(j)] = 1;
        if (k) check(p.zjobs[size_t(p.lists[L_ZSTD][k - 1])].src_len >= p.zjobs[size_t(j)].src_len, "%s: dispatch order", name);
    }
    for (const ZstdJob& jb : p.zjobs) {
        const DevPage& pg = p.pages[size_t(jb.page)];
        const uintptr_t s = reinterpret_cast<uintptr_t>(jb.src), d = reinterpret_cast<uintptr_t>(jb.dst);
        check(s >= BASES.in && s + jb.src_len <= BASES.in + n_bytes, "%s: job source outside the input", name);
        check(d >= BASES.scratch && d + jb.dst_len <= BASES.scratch + p.scratch_bytes, "%s: job destination outside scratch", name);
        check(jb.dst == pg.body && jb.dst_len == pg.body_len && (pg.flags & PG_COMPRESSED) && jb.exact == 1, "%s: job and page disagree", name);
        check(p.chunks[size_t(jb.chunk)].codec == PF_CODEC_ZSTD && pg.chunk == jb.chunk, "%s: job of a chunk that is not ZSTD", name);
        max_dst = std::max(max_dst, jb.dst_len);
    }
    if (lit_bytes) check(p.zlit_stride >= std::min<uint32_t>(max_dst, ZSTD_LIT_MAX), "%s: literal area below a block's literals", name);
    for (const SnappyJob& jb : p.jobs) check(p.chunks[size_t(jb.chunk)].codec == PF_CODEC_SNAPPY, "%s: Snappy job of another codec", name);
    check(p.off_zjobs + sizeof(ZstdJob) * p.zjobs.size() <= p.meta_bytes - 256, "%s: jobs outside the metadata block", name);
}

Chunk zstd_chunk() {   // dictionary page, v1 page, v2 pages compressed and stored, a 400 KB page
    Chunk c = chunk(PF_INT64, 1, PF_CODEC_ZSTD);
    c.pages.push_back(page(PF_PAGE_DICTIONARY, 100, 300, 800));
    c.pages.push_back(page(PF_PAGE_DATA, 1000, 777, 8013));
    c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 900, 8010, 1, 10));
    c.pages.push_back(page(PF_PAGE_DATA_V2, 1000, 8010, 8010, 0, 10));
    c.pages.push_back(page(PF_PAGE_DATA, 50000, 123457, 400013));
    c.pages[1].encoding = c.pages[2].encoding = c.pages[3].encoding = c.pages[4].encoding = PF_ENC_PLAIN;
    return c;
}
Chunk snappy_chunk(int nv) {
    Chunk c = chunk(PF_INT32, 0, PF_CODEC_SNAPPY);
    c.pages.push_back(page(PF_PAGE_DATA, nv, 3u * uint32_t(nv), 4u * uint32_t(nv)));
    c.pages.push_back(page(PF_PAGE_DATA, nv, 5u * uint32_t(nv), 4u * uint32_t(nv)));   // did not compress: litcopy candidate
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
    {   // one ZSTD chunk
        std::vector<Chunk> cs{zstd_chunk()};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0, "zstd chunk does not plan: %lld", (long long)p.host_status[0]);
        check(p.zjobs.size() == 4 && p.jobs.empty(), "zstd chunk: %zu zstd jobs, %zu snappy jobs", p.zjobs.size(), p.jobs.size());
        check(!(p.pages[3].flags & PG_COMPRESSED) && p.pplan[3].scratch_off == NO_OFF && p.pages[3].body_len == 8000, "stored v2 page");
        check(p.pages[2].body_len == 8000 && p.zjobs[2].src_len == 890 && p.zjobs[2].dst_len == 8000, "v2 level bytes stay outside the frame");
        check(p.zlit_stride >= ZSTD_LIT_MAX && p.zlit_stride <= ZSTD_LIT_MAX + 512, "literal area of a large page: %u", p.zlit_stride);
        check(p.lists[L_ZSTD][0] == 3, "largest page first");
        check_zstd(p, n, "zstd");
    }
    {   // more jobs than workgroups: the areas stop at ZSTD_GRID, and small pages get small areas
        Chunk c = chunk(PF_INT32, 0, PF_CODEC_ZSTD);
        for (int i = 0; i < ZSTD_GRID + 90; i++) c.pages.push_back(page(PF_PAGE_DATA, 500, 600 + uint32_t(i % 7), 2000));
        std::vector<Chunk> cs{c};
        BatchPlan p;
        plan(cs, p, n);
        check(p.zjobs.size() == size_t(ZSTD_GRID + 90) && p.zstd_grid == uint32_t(ZSTD_GRID), "grid cap");
        check(p.zlit_stride >= 2000 && p.zlit_stride <= 2000 + 512, "small pages, small areas: %u", p.zlit_stride);
        check_zstd(p, n, "many");
    }
    {   // mixed batch against the same batch without the ZSTD chunk
        std::vector<Chunk> with{snappy_chunk(5000), zstd_chunk(), plain_chunk(), snappy_chunk(70000)};
        std::vector<Chunk> without{snappy_chunk(5000), plain_chunk(), snappy_chunk(70000)};
        BatchPlan a, b;
        size_t na = 0, nb = 0;
        plan(with, a, na);
        plan(without, b, nb);
        for (size_t c = 0; c < with.size(); c++) check(a.host_status[c] == 0, "mixed: chunk %zu does not plan", c);
        check_zstd(a, na, "mixed");
        check_zstd(b, nb, "no zstd");
        check(b.zjobs.empty() && b.zstd_grid == 0 && b.zlit_stride == 0 && b.lists[L_ZSTD].empty(), "no zstd: a job or an area");
        check(a.jobs.size() == b.jobs.size() && a.snap.n_splits == b.snap.n_splits && a.snap.wins.size() == b.snap.wins.size() &&
                  a.snap.pieces.size() == b.snap.pieces.size() && a.snap.tokmap_bytes == b.snap.tokmap_bytes &&
                  a.snap.max_snap_win == b.snap.max_snap_win, "mixed: Snappy tables changed");
        for (size_t j = 0; j < a.jobs.size() && j < b.jobs.size(); j++) {
            const SnappyJob &x = a.jobs[j], &y = b.jobs[j];
            check(x.src_len == y.src_len && x.dst_len == y.dst_len && x.n_win == y.n_win && x.n_pieces == y.n_pieces &&
                      x.win_base == y.win_base && x.split_base == y.split_base && x.dflags == y.dflags, "mixed: Snappy job %zu changed", j);
        }
        check(a.lists[L_DJOBS] == b.lists[L_DJOBS], "mixed: litcopy list changed");
        check(std::memcmp(a.snap.pieces.data(), b.snap.pieces.data(), sizeof(Int2) * std::min(a.snap.pieces.size(), b.snap.pieces.size())) == 0,
              "mixed: piece order changed");
    }
    {   // GZIP is still refused, and takes nothing with it
        Chunk g = zstd_chunk();
        g.d.codec = PF_CODEC_GZIP;
        std::vector<Chunk> cs{g, zstd_chunk()};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == PF_ERR_UNSUPPORTED_CODEC && p.host_status[1] == 0, "gzip: %lld %lld", (long long)p.host_status[0],
              (long long)p.host_status[1]);
        check(p.zjobs.size() == 4, "gzip: jobs");
        check_zstd(p, n, "gzip");
    }
    {   // a chunk that fails after its jobs were made loses them
        Chunk bad = zstd_chunk();
        bad.pages.push_back(page(PF_PAGE_DATA, -5, 10, 10));
        std::vector<Chunk> cs{zstd_chunk(), bad};
        BatchPlan p;
        plan(cs, p, n);
        check(p.host_status[0] == 0 && p.host_status[1] == PF_ERR_CORRUPT_PAGE && p.zjobs.size() == 4, "failed chunk keeps jobs");
        check_zstd(p, n, "failed chunk");
    }
    std::printf("zstd plan check: failures %d\n", g_fail);
    return g_fail ? 1 : 0;
}
