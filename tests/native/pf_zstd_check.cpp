// pf_zstd_check — the host model of the ZSTD decode core (csrc/pf_zstd_core.h) over a file of cases,
// built by tests/test_zstd_core.py with g++ under AddressSanitizer + UBSan.
//
//   pf_zstd_check <cases> <results>
//
// cases:   per case  u32 n, u32 expected, n bytes (little endian)
// results: per case  i32 status, u32 len, len bytes
// A case is decoded into a heap block of exactly `expected` bytes (so a write past it is an ASan
// report); status is 0 when the core accepts the frames and they produce exactly `expected` bytes
// (len = expected, the bytes follow), else -2 (len = 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pf_zstd_core.h"

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

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: pf_zstd_check <cases> <results>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    auto T = std::make_unique<pf::zstd::Tables>();
    std::vector<uint8_t> lit(pf::zstd::Z_BLOCK_MAX);
    size_t at = 0, cases = 0, accepted = 0;
    while (at + 8 <= in.size()) {
        uint32_t n, expected;
        std::memcpy(&n, &in[at], 4);
        std::memcpy(&expected, &in[at + 4], 4);
        at += 8;
        if (n > in.size() - at) { std::fprintf(stderr, "truncated case file\n"); return 2; }
        // exact-size heap copies: an overrun of source or destination is a sanitizer report
        std::unique_ptr<uint8_t[]> src(new uint8_t[n ? n : 1]), dst(new uint8_t[expected ? expected : 1]);
        std::memcpy(src.get(), in.data() + at, n);
        at += n;
        size_t produced = 0;
        int32_t st = pf::zstd::decompress_host(src.get(), n, dst.get(), expected, &produced, *T, lit.data());
        if (st == 0 && produced != expected) st = pf::zstd::Z_CORRUPT;
        const uint32_t len = st == 0 ? expected : 0;
        std::fwrite(&st, 4, 1, out);
        std::fwrite(&len, 4, 1, out);
        if (len) std::fwrite(dst.get(), 1, len, out);
        cases++;
        accepted += st == 0;
    }
    std::fclose(out);
    std::printf("cases %zu accepted %zu\n", cases, accepted);
    return 0;
}
