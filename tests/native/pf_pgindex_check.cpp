// pf_pgindex_check — the page index parsers of csrc/pf_meta.cpp (parse_column_index, parse_offset_index) over a
// file of structs, built by tests/test_write_pgindex_cpu.py with g++ under AddressSanitizer + UBSan.
//
//   pf_pgindex_check <cases>
//
// cases: per case  u32 kind (0 ColumnIndex, 1 OffsetIndex), u32 n, n bytes (little endian)
// Every struct is parsed as it is (it must be accepted), then every proper prefix of it and every change of one
// byte to each of the 255 other values. Each parse reads a heap block of exactly the struct's size, so a read
// past it is a sanitizer report. A damaged struct is either refused (MetaError) or accepted with lists that are
// consistent with each other; anything else counts as a failure. Prints "valid N accepted A refused R failures F".
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pf_host.h"

static bool read_all(const char* path, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(size_t(n));
    const bool ok = n == 0 || std::fread(out.data(), 1, size_t(n), f) == size_t(n);
    std::fclose(f);
    return ok;
}

static size_t accepted = 0, refused = 0, failures = 0;

// 1 accepted and consistent, 0 refused, -1 accepted but inconsistent
static int parse(uint32_t kind, const uint8_t* bytes, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);   // exact size
    std::memcpy(p.get(), bytes, n);
    try {
        if (kind == 0) {
            pf::ColumnIndexMeta ci;
            pf::parse_column_index(p.get(), n, ci);
            const size_t np = ci.null_pages.size();
            if (ci.value_off.size() != 2 * np + 1 || ci.value_off[0] != 0 || ci.value_off.back() != ci.values.size()) return -1;
            for (size_t i = 0; i + 1 < ci.value_off.size(); i++)
                if (ci.value_off[i] > ci.value_off[i + 1]) return -1;
            if (ci.has_null_counts && ci.null_counts.size() != np) return -1;
            if (ci.boundary_order < 0 || ci.boundary_order > 2 || ci.values.size() > n) return -1;
        } else {
            std::vector<pf_page_location> locs;
            pf::parse_offset_index(p.get(), n, locs);
            if (locs.size() > n) return -1;
            for (const pf_page_location& l : locs)
                if (l.offset < 0 || l.compressed_page_size < 0 || l.first_row_index < 0) return -1;
        }
    } catch (const pf::MetaError&) {
        return 0;
    }
    return 1;
}

static void damaged(uint32_t kind, const uint8_t* bytes, size_t n) {
    const int r = parse(kind, bytes, n);
    if (r > 0) accepted++;
    else if (r == 0) refused++;
    else failures++;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: pf_pgindex_check <cases>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    size_t at = 0, valid = 0;
    while (at + 8 <= in.size()) {
        uint32_t kind, n;
        std::memcpy(&kind, &in[at], 4);
        std::memcpy(&n, &in[at + 4], 4);
        at += 8;
        if (n > in.size() - at || kind > 1) { std::fprintf(stderr, "bad case file\n"); return 2; }
        std::vector<uint8_t> s(in.begin() + long(at), in.begin() + long(at + n));
        at += n;
        if (parse(kind, s.data(), s.size()) != 1) {
            std::fprintf(stderr, "case %zu: the undamaged struct was not accepted\n", valid);
            failures++;
        }
        valid++;
        for (size_t k = 0; k < s.size(); k++) {   // every proper prefix: the STOP byte is gone, so none is a struct
            if (parse(kind, s.data(), k) != 0) {
                std::fprintf(stderr, "case %zu: prefix of %zu bytes accepted\n", valid - 1, k);
                failures++;
            } else {
                refused++;
            }
        }
        for (size_t k = 0; k < s.size(); k++) {
            const uint8_t keep = s[k];
            for (int v = 0; v < 256; v++) {
                if (v == keep) continue;
                s[k] = uint8_t(v);
                damaged(kind, s.data(), s.size());
            }
            s[k] = keep;
        }
    }
    std::printf("valid %zu accepted %zu refused %zu failures %zu\n", valid, accepted, refused, failures);
    return failures ? 1 : 0;
}
