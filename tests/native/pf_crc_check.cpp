// The host fold of page CRCs (csrc/pf_crc.h: crc_combine, crc_combine_pow, crc_raw_bytes, crc_finish) against a
// plain bytewise CRC-32: the raw CRCs of pieces, folded in order, are the CRC of their concatenation, at the
// lengths around the compressor's 8 KiB jobs. Built with -fsanitize=address,undefined by
// tests/test_write_stats_cpu.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pf_crc.h"

namespace {
int failures = 0;

// CRC-32 as zlib computes it, bit by bit, and its raw form (zero init, no final xor)
uint32_t crc_bits(const uint8_t* p, size_t n, uint32_t init, uint32_t fin) {
    uint32_t c = init;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return c ^ fin;
}
uint32_t crc32_plain(const std::vector<uint8_t>& v) { return crc_bits(v.data(), v.size(), 0xffffffffu, 0xffffffffu); }
uint32_t raw_plain(const std::vector<uint8_t>& v) { return crc_bits(v.data(), v.size(), 0u, 0u); }

void expect(bool ok, const char* what, size_t a, size_t b, size_t c) {
    if (ok) return;
    failures++;
    std::printf("FAIL %s (%zu, %zu, %zu)\n", what, a, b, c);
}

std::vector<uint8_t> bytes(std::mt19937& g, size_t n) {
    std::vector<uint8_t> v(n);
    for (auto& b : v) b = uint8_t(g());
    return v;
}
}  // namespace

int main() {
    std::mt19937 g(12345);
    const size_t lens[] = {0, 1, 8191, 8192, 8193};
    expect(crc32_plain({'1', '2', '3', '4', '5', '6', '7', '8', '9'}) == 0xcbf43926u, "the check value of CRC-32", 0, 0, 0);
    expect(pf::crc_finish(0, 0) == 0, "an empty page has CRC 0", 0, 0, 0);
    uint32_t x2n[32];
    pf::crc_x2n_table(x2n);
    int checks = 0;
    for (size_t la : lens)
        for (size_t lb : lens) {
            const std::vector<uint8_t> a = bytes(g, la), b = bytes(g, lb);
            std::vector<uint8_t> ab = a;
            ab.insert(ab.end(), b.begin(), b.end());
            const uint32_t ra = raw_plain(a), rb = raw_plain(b);
            expect(pf::crc_raw_bytes(0, a.data(), a.size()) == ra, "crc_raw_bytes", la, 0, 0);
            expect(pf::crc_raw_bytes(ra, b.data(), b.size()) == raw_plain(ab), "crc_raw_bytes continues", la, lb, 0);
            expect(pf::crc_combine(ra, rb, lb) == raw_plain(ab), "crc_combine", la, lb, 0);
            expect(pf::crc_combine_pow(ra, rb, pf::crc_x8n(lb, x2n)) == raw_plain(ab), "crc_combine_pow", la, lb, 0);
            expect(pf::crc_finish(pf::crc_combine(ra, rb, lb), la + lb) == crc32_plain(ab), "crc_finish", la, lb, 0);
            checks += 5;
            for (size_t lc : lens) {   // three pieces: host bytes, then two device pieces, as a page's levels ‖ varint ‖ jobs
                const std::vector<uint8_t> c = bytes(g, lc);
                std::vector<uint8_t> abc = ab;
                abc.insert(abc.end(), c.begin(), c.end());
                uint32_t raw = pf::crc_raw_bytes(0, a.data(), a.size());
                raw = pf::crc_combine(raw, rb, lb);
                raw = pf::crc_combine(raw, raw_plain(c), lc);
                expect(pf::crc_finish(raw, la + lb + lc) == crc32_plain(abc), "three-piece fold", la, lb, lc);
                checks++;
            }
        }
    // a long tail: every bit of the length takes part in x^(8 n)
    {
        const std::vector<uint8_t> a = bytes(g, 3), b(size_t(1) << 20, 0);
        std::vector<uint8_t> ab = a;
        ab.insert(ab.end(), b.begin(), b.end());
        expect(pf::crc_combine(raw_plain(a), 0u, b.size()) == raw_plain(ab), "crc_combine over 1 MiB of zeros", 3, b.size(), 0);
        checks++;
    }
    std::printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
