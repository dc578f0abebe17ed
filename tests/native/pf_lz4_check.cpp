// pf_lz4_check — the host model of the LZ4 decode core (csrc/pf_lz4_core.h) over a file of cases,
// built by tests/lz4_blocks.py with g++ under AddressSanitizer + UBSan.
//
//   pf_lz4_check <cases> <results>
//
// cases:   per case  u32 n, u32 expected, n bytes (little endian)
// results: per case  i32 status, u32 len, len bytes
// A case is decoded from a heap block of exactly n bytes into one of exactly `expected` bytes (so a
// read or write past either is an ASan report); status is 0 when the core accepts the block and it
// produces exactly `expected` bytes (len = expected, the bytes follow), else -2 (len = 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pf_lz4_core.h"

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
    if (argc != 3) { std::fprintf(stderr, "usage: pf_lz4_check <cases> <results>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    size_t at = 0, cases = 0, accepted = 0;
    while (at + 8 <= in.size()) {
        uint32_t n, expected;
        std::memcpy(&n, &in[at], 4);
        std::memcpy(&expected, &in[at + 4], 4);
        at += 8;
        if (n > in.size() - at) { std::fprintf(stderr, "truncated case file\n"); return 2; }
        // exact-size heap copies: an overrun of source or destination is a sanitizer report
        // (n = 0 / expected = 0: a block of no bytes, so that any access at all is one)
        std::unique_ptr<uint8_t[]> src(new uint8_t[n]), dst(new uint8_t[expected]);
        if (n) std::memcpy(src.get(), in.data() + at, n);
        at += n;
        const int32_t st = pf::lz4::decompress_host(src.get(), n, dst.get(), expected);
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
