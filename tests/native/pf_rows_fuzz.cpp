// Sanitizer driver for pf_file_chunk_desc_rows (csrc/pf_file.cpp): the OffsetIndex and the page headers at the
// locations it gives are untrusted input. Built with -fsanitize=address,undefined by tests/test_row_window_cpu.py.
// For every column of the fixture and a few row ranges it runs the call over
//   every prefix of the chunk's OffsetIndex (the index length the footer states, shortened),
//   every single-byte change (all 255 other values) of the OffsetIndex,
//   every single-byte change of the selected pages' headers and of the dictionary page's header,
//   every prefix of those headers, two ways: the index rewritten in the file so that the location's
//   compressed_page_size (for the dictionary header: the first location's offset, hence dict_size) ends the header
//   after k bytes, through the call; and pf::read_page_header on a heap copy of exactly k bytes, whose red zone
//   catches a read past the length even where the call's own buffer goes on,
// and accepts any status: the run passes when no sanitizer reports.
//   pf_rows_fuzz FIXTURE TMPDIR
// pf_file.cpp is included, not linked: the driver shortens oi_length in the parsed footer and reopens the file handle
// after each byte written, neither of which the C ABI offers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pf_file.cpp"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> b;
    FILE* f = std::fopen(path, "rb");
    if (!f) return b;
    std::fseek(f, 0, SEEK_END);
    b.resize(size_t(std::ftell(f)));
    std::fseek(f, 0, SEEK_SET);
    if (!b.empty() && std::fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
    std::fclose(f);
    return b;
}

static long g_calls = 0, g_ok = 0;

// The call under test, and a touch of everything it returned.
static int call(pf_file* f, int col, int64_t lo, int64_t hi) {
    pf_chunk_desc d;
    pf_chunk_rows r;
    const int rc = pf_file_chunk_desc_rows(f, 0, col, lo, hi, 256, &d, &r);
    g_calls++;
    if (rc == PF_OK) {
        g_ok++;
        uint64_t sum = uint64_t(r.first_row + r.skip_rows + r.take_rows) + r.dict_size + r.data_size;
        for (int i = 0; i < d.n_pages; i++) sum += d.pages[i].offset + d.pages[i].compressed_size;
        if (sum == 0x5a5a5a5a5a5a5a5aull) std::puts("");
    }
    return rc;
}

static bool put_bytes(const std::string& path, pf_file* f, uint64_t at, const uint8_t* v, size_t n) {
    FILE* w = std::fopen(path.c_str(), "r+b");
    if (!w) return false;
    std::fseek(w, long(at), SEEK_SET);
    const bool ok = std::fwrite(v, 1, n, w) == n;
    std::fclose(w);
    std::fclose(f->fp);   // (a stdio read buffer may hold the old byte)
    f->fp = std::fopen(path.c_str(), "rb");
    return ok && f->fp;
}
static bool put_byte(const std::string& path, pf_file* f, uint64_t at, uint8_t v) { return put_bytes(path, f, at, &v, 1); }

// Thrift compact integers: zigzag, a varint, and a varint padded with continuation bytes to n bytes (readers take
// it; it lets a smaller value overwrite a larger one in place). Empty when v does not fit n bytes.
static uint64_t zz(int64_t v) { return (uint64_t(v) << 1) ^ uint64_t(v >> 63); }
static std::vector<uint8_t> varint(uint64_t v) {
    std::vector<uint8_t> b;
    for (; v >= 0x80; v >>= 7) b.push_back(uint8_t(v) | 0x80);
    b.push_back(uint8_t(v));
    return b;
}
static std::vector<uint8_t> padded(uint64_t v, size_t n) {
    std::vector<uint8_t> b(n);
    for (size_t i = 0; i < n; i++, v >>= 7) b[i] = uint8_t(v & 0x7f) | (i + 1 < n ? 0x80 : 0);
    return v ? std::vector<uint8_t>() : b;
}

// Where a PageLocation's fields lie in the file: the index holds "0x16 offset 0x15 compressed_page_size ..." per
// location (field ids by delta). Returns false when the bytes are not found as written.
struct LocBytes { uint64_t off_at, off_len, cps_at, cps_len; };
static bool find_location(const std::vector<uint8_t>& file, uint64_t oi_off, uint64_t oi_len, const pf_page_location& L,
                          LocBytes& out) {
    std::vector<uint8_t> pat{0x16};
    const std::vector<uint8_t> o = varint(zz(L.offset)), c = varint(zz(L.compressed_page_size));
    pat.insert(pat.end(), o.begin(), o.end());
    pat.push_back(0x15);
    pat.insert(pat.end(), c.begin(), c.end());
    for (uint64_t i = oi_off; i + pat.size() <= oi_off + oi_len; i++)
        if (std::memcmp(file.data() + i, pat.data(), pat.size()) == 0) {
            out = LocBytes{i + 1, o.size(), i + 2 + o.size(), c.size()};
            return true;
        }
    return false;
}

static long g_direct = 0;

// pf::read_page_header over every prefix of a header, each in a heap block of its own length.
static void direct_prefixes(const uint8_t* head, uint64_t len) {
    for (uint64_t k = 0; k <= len; k++) {
        std::vector<uint8_t> c(head, head + k);
        pf_page_desc pd;
        try {
            const size_t h = pf::read_page_header(c.data(), size_t(k), pd);
            if (h > k) { std::fprintf(stderr, "header length %zu past its %llu bytes\n", h, (unsigned long long)k); std::exit(3); }
        } catch (const std::exception&) {
        }
        g_direct++;
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: pf_rows_fuzz FIXTURE TMPDIR\n"); return 2; }
    const std::vector<uint8_t> orig = slurp(argv[1]);
    if (orig.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const std::string path = std::string(argv[2]) + "/rows_fuzz.parquet";
    {
        FILE* w = std::fopen(path.c_str(), "wb");
        if (!w || std::fwrite(orig.data(), 1, orig.size(), w) != orig.size()) return 2;
        std::fclose(w);
    }
    pf_file* f = nullptr;
    if (pf_file_open(path.c_str(), &f) != PF_OK) { std::fprintf(stderr, "open: %s\n", pf_file_last_error()); return 2; }
    int nc = 0;
    int64_t rows = 0;
    pf_file_num_columns(f, &nc);
    pf_file_row_group_rows(f, 0, &rows);
    const int64_t ranges[][2] = {{0, rows}, {rows / 3, rows / 3 + 100}, {rows - 1, rows}, {0, 0}};
    for (int col = 0; col < nc; col++) {
        pf::ChunkMeta& m = f->meta.row_groups[0].columns[size_t(col)];
        const int64_t oi_off = m.oi_offset, oi_len = m.oi_length;
        if (oi_off < 0) { std::fprintf(stderr, "column %d has no OffsetIndex\n", col); return 2; }
        for (size_t ri = 0; ri < sizeof ranges / sizeof ranges[0]; ri++) {
            const int64_t* rg = ranges[ri];
            if (call(f, col, rg[0], rg[1]) != PF_OK) { std::fprintf(stderr, "baseline: %s\n", pf_file_last_error()); return 2; }
            // the headers this range selects: [file offset, length)
            struct Head { uint64_t at, len; int page; };   // page: index of its location, -1 the dictionary page
            std::vector<Head> heads;
            std::vector<pf_page_location> all_locs;
            uint64_t chunk_start = 0, chunk_size = 0;
            pf_file_chunk_range(f, 0, col, &chunk_start, &chunk_size);
            {
                pf_chunk_desc d;
                pf_chunk_rows r;
                pf_file_chunk_desc_rows(f, 0, col, rg[0], rg[1], 0, &d, &r);
                std::vector<pf_page_location> locs(4096);
                int n = 0;
                pf_file_offset_index(f, 0, col, locs.data(), int(locs.size()), &n);
                int k = 0;
                if (r.dict_size) { heads.push_back({r.dict_start, d.pages[0].offset, -1}); k = 1; }
                for (int p = 0; p < r.n_data_pages; p++) {
                    const uint64_t at = uint64_t(locs[size_t(r.first_page + p)].offset);
                    heads.push_back({at, d.pages[k + p].offset - (r.dict_size + (at - r.data_start)), r.first_page + p});
                }
                all_locs.assign(locs.begin(), locs.begin() + n);
            }
            for (int64_t k = 0; k <= oi_len; k++) {   // prefixes of the index
                m.oi_length = k;
                call(f, col, rg[0], rg[1]);
            }
            m.oi_length = oi_len;
            auto bytes = [&](uint64_t at, uint64_t n) {
                for (uint64_t i = at; i < at + n; i++) {
                    for (int v = 0; v < 256; v++) {
                        if (uint8_t(v) == orig[i]) continue;
                        if (!put_byte(path, f, i, uint8_t(v))) return false;
                        call(f, col, rg[0], rg[1]);
                    }
                    if (!put_byte(path, f, i, orig[i])) return false;
                }
                return true;
            };
            if (ri == 1) {   // (the index does not depend on the range: its bytes once per column)
                if (!bytes(uint64_t(oi_off), uint64_t(oi_len))) return 2;
            }
            if (ri != 0)   // (the headers the narrow ranges select; the whole chunk's would only repeat the same code)
                for (const auto& h : heads)
                    if (!bytes(h.at, h.len)) return 2;
            // prefixes of the headers: the index says the header's range ends after k bytes (k = its length: the
            // body is cut off instead)
            for (const auto& h : heads) {
                direct_prefixes(orig.data() + h.at, h.len);
                LocBytes lb;
                if (!find_location(orig, uint64_t(oi_off), uint64_t(oi_len), all_locs[size_t(h.page < 0 ? 0 : h.page)], lb)) {
                    std::fprintf(stderr, "column %d: page location bytes not found in the index\n", col);
                    return 2;
                }
                const uint64_t at = h.page < 0 ? lb.off_at : lb.cps_at, len = h.page < 0 ? lb.off_len : lb.cps_len;
                // a call that fails leaves the array of the last call that succeeded where it is (read below: a freed
                // or rewritten array is a report or a mismatch)
                pf_chunk_desc kept;
                pf_chunk_rows kr;
                if (pf_file_chunk_desc_rows(f, 0, col, rg[0], rg[1], 256, &kept, &kr) != PF_OK) return 2;
                std::vector<pf_page_desc> kept_pages(kept.pages, kept.pages + kept.n_pages);
                for (uint64_t k = 0; k <= h.len; k++) {
                    const std::vector<uint8_t> v = padded(zz(int64_t(h.page < 0 ? chunk_start + k : k)), size_t(len));
                    if (v.empty()) { std::fprintf(stderr, "column %d: %llu does not fit the index field\n", col, (unsigned long long)k); return 2; }
                    if (!put_bytes(path, f, at, v.data(), v.size())) return 2;
                    const int rc = call(f, col, rg[0], rg[1]);
                    if (rc == PF_OK && h.page >= 0 && k < h.len) { std::fprintf(stderr, "column %d: a header cut to %llu bytes was accepted\n", col, (unsigned long long)k); return 3; }
                    if (rc != PF_OK && std::memcmp(kept.pages, kept_pages.data(), sizeof(pf_page_desc) * kept_pages.size()) != 0) {
                        std::fprintf(stderr, "column %d: a failed call changed the earlier descriptor's pages\n", col);
                        return 3;
                    }
                    if (rc == PF_OK) {   // (a success swapped a new array in: that one is the kept one now)
                        if (pf_file_chunk_desc_rows(f, 0, col, rg[0], rg[1], 256, &kept, &kr) != PF_OK) return 2;
                        kept_pages.assign(kept.pages, kept.pages + kept.n_pages);
                    }
                }
                if (!put_bytes(path, f, at, orig.data() + at, size_t(len))) return 2;
            }
            if (call(f, col, rg[0], rg[1]) != PF_OK) { std::fprintf(stderr, "restored file fails: %s\n", pf_file_last_error()); return 2; }
        }
    }
    pf_file_close(f);
    std::printf("calls %ld ok %ld direct %ld\n", g_calls, g_ok, g_direct);
    return 0;
}
