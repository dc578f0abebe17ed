// pf_fix_ids_check — fix_ids8 (csrc/pf_fix_ids.h, the id unpack of k_flat_fixed's eight-a-thread body) against a plain
// per-entry reference, on the host. Built by tests/test_fix_ids_cpu.py with -fsanitize=address,undefined and run directly.
//
// A case is a list of runs (RLE or bit-packed at width bw) with a run table in k_runs' row format. A packed run's ids
// may start at any bit (a table row is a bit offset), which is how every first-bit shift 0..7 of a group is met at every
// width. The id section lies `mis` bytes into a heap block of exactly mis + ids_n bytes whose start is word aligned, and
// the word loader aborts on a word that is not wholly inside the section: a read outside it fails the run twice over.
// Every group start e0 (a multiple of 8) with n = 1..8 is compared with the reference when the routine calls the group
// fast, and whether it does so is compared with the rule written out here: one run, and RLE / width 0, or n == 8,
// bw <= 16 and the words inside the section.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pf_fix_ids.h"

namespace {

struct RunSpec {
    uint32_t count;
    bool packed;
    uint32_t shift;   // packed: the bit of its first byte at which the run's first id starts
};

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

struct Case {
    std::vector<uint32_t> rt;
    std::vector<uint8_t> stream;
    std::vector<uint32_t> want;
    std::vector<uint32_t> run_of;   // run index of every value
    uint32_t total = 0;
};

uint32_t bit_at(const std::vector<uint8_t>& s, uint64_t bit) {
    const uint64_t by = bit >> 3;
    return by < s.size() ? (s[by] >> (bit & 7)) & 1u : 0u;
}

// `tail`: bytes after the last run's last id byte
Case build(const std::vector<RunSpec>& runs, int bw, uint32_t tail) {
    Case c;
    const uint32_t vmask = bw >= 32 ? 0xffffffffu : ((1u << bw) - 1u);
    uint32_t first = 0;
    for (const RunSpec& r : runs) {
        for (uint32_t g = 1 + rnd() % 3; g > 0; g--) c.stream.push_back(uint8_t(rnd()));   // where a header would be
        c.rt.push_back(first | (r.packed ? 0x80000000u : 0u));
        if (r.packed) {
            c.rt.push_back(uint32_t(c.stream.size() * 8) + r.shift);
            const uint64_t bits = uint64_t(r.shift) + uint64_t(r.count) * uint64_t(bw);
            for (uint64_t b = 0; b < (bits + 7) / 8; b++) c.stream.push_back(uint8_t(rnd()));
        } else {
            const uint32_t v = rnd() & vmask;
            c.rt.push_back(v);
            for (int b = 0; b < (bw + 7) / 8; b++) c.stream.push_back(uint8_t(v >> (8 * b)));
        }
        first += r.count;
    }
    c.total = first;
    for (uint32_t t = 0; t < tail; t++) c.stream.push_back(uint8_t(rnd()));
    for (size_t i = 0; i < runs.size(); i++)
        for (uint32_t k = 0; k < runs[i].count; k++) {
            uint32_t v = c.rt[2 * i + 1];
            if (runs[i].packed) {
                v = 0;
                for (int b = 0; b < bw; b++) v |= bit_at(c.stream, uint64_t(c.rt[2 * i + 1]) + uint64_t(k) * bw + b) << b;
            }
            c.want.push_back(v);
            c.run_of.push_back(uint32_t(i));
        }
    return c;
}

long g_cases = 0, g_groups = 0, g_fast = 0, g_fail = 0;

struct Frame {   // the words a caller may read: those wholly inside [mis, mis + n)
    const uint8_t* base;
    uint32_t mis;
    uint64_t n;
    uint32_t operator()(uint32_t o) const {
        if ((o & 3u) || o < mis || uint64_t(o) + 4u > uint64_t(mis) + n) {
            fprintf(stderr, "word at %u read outside the section [%u, %llu)\n", o, mis, (unsigned long long)(mis + n));
            abort();
        }
        uint32_t x;
        memcpy(&x, base + o, 4);
        return x;
    }
};

void fail(const char* what, int bw, uint32_t mis, uint32_t e0, uint32_t n, uint32_t k, uint32_t got, uint32_t want) {
    if (g_fail++ < 20) fprintf(stderr, "%s: bw %d mis %u e0 %u n %u k %u: got %u, want %u\n", what, bw, mis, e0, n, k, got, want);
}

void check(const Case& c, const std::vector<RunSpec>& runs, int bw, uint32_t mis) {
    g_cases++;
    const uint64_t ids_n = c.stream.size();
    uint8_t* block = static_cast<uint8_t*>(malloc(mis + ids_n + (mis + ids_n == 0)));   // (malloc: 16-byte aligned)
    for (uint32_t i = 0; i < mis; i++) block[i] = uint8_t(rnd() | 1u);
    if (ids_n) memcpy(block + mis, c.stream.data(), ids_n);
    const Frame F{block, mis, ids_n};
    const uint32_t nr = uint32_t(c.rt.size() / 2);
    const pf::FixRowsRt R{c.rt.data(), nr, c.total};
    for (uint32_t e0 = 0; e0 < c.total; e0 += 8) {
        const uint32_t full = c.total - e0 < 8 ? c.total - e0 : 8;
        for (uint32_t n = 1; n <= full; n++) {
            uint32_t id[8];
            for (uint32_t& x : id) x = 0xdeadbeefu;
            const bool fast = pf::fix_ids8(R, nr, e0, n, bw, mis, ids_n, F, id);
            g_groups++;
            // the rule, written out
            const uint32_t r = c.run_of[e0];
            bool want_fast = c.run_of[e0 + n - 1] == r;
            if (want_fast && runs[r].packed && bw != 0) {
                const uint64_t bit = uint64_t(c.rt[2 * r + 1]) + uint64_t(e0 - (c.rt[2 * r] & 0x7fffffffu)) * bw;
                const uint64_t o4 = ((bit >> 3) + mis) & ~3ull;
                const uint64_t last = (bit + 8ull * bw - 1) >> 3;   // last id byte of the group
                want_fast = n == 8 && bw <= 16 && o4 >= mis && o4 + 4ull * pf::fix_ndw(bw) <= mis + ids_n;
                // the words of the load hold every id byte of the group
                if (want_fast && last + mis >= o4 + 4ull * pf::fix_ndw(bw)) fail("group wider than its words", bw, mis, e0, n, 0, 0, 0);
            }
            if (fast != want_fast) fail("fast", bw, mis, e0, n, 0, fast, want_fast);
            if (!fast) {
                for (uint32_t x : id) if (x != 0xdeadbeefu) fail("id touched", bw, mis, e0, n, 0, x, 0xdeadbeefu);
                continue;
            }
            g_fast++;
            for (uint32_t k = 0; k < n; k++)
                if (id[k] != c.want[e0 + k]) fail("id", bw, mis, e0, n, k, id[k], c.want[e0 + k]);
        }
    }
    free(block);
}

}  // namespace

int main() {
    for (int bw = 0; bw <= 32; bw++) {
        for (uint32_t shift = 0; shift < 8; shift++) {
            std::vector<std::vector<RunSpec>> layouts;
            layouts.push_back({{40, true, shift}});                              // nr = 1, packed
            layouts.push_back({{40, false, 0}});                                 // nr = 1, RLE
            // a boundary at every split 1..7 of a group, between packed -> packed, packed -> RLE, RLE -> packed
            for (uint32_t j = 1; j < 8; j++) {
                layouts.push_back({{8 + j, true, shift}, {24 - j, true, (shift + 3) & 7}});
                layouts.push_back({{8 + j, true, shift}, {24 - j, false, 0}});
                layouts.push_back({{8 + j, false, 0}, {24 - j, true, shift}});
            }
            for (size_t li = 0; li < layouts.size(); li++)
                for (uint32_t mis = 0; mis < 4; mis++)
                    check(build(layouts[li], bw, (uint32_t(li) + mis + shift) % 25), layouts[li], bw, mis);
        }
        // the section ends 0..24 bytes after the last group's last id byte
        for (uint32_t tail = 0; tail <= 24; tail++) {
            const std::vector<RunSpec> l = {{3, false, 0}, {29, true, tail & 7}};
            check(build(l, bw, tail), l, bw, tail & 3);
            const std::vector<RunSpec> m = {{16, true, 0}};
            check(build(m, bw, tail), m, bw, (tail >> 2) & 3);
        }
        {   // nr = RUN_CAP: one-group packed runs and RLE runs of 1, 3, 8 and 13 values in turn
            std::vector<RunSpec> l;
            const uint32_t rl[4] = {1, 3, 8, 13};
            for (int i = 0; i < pf::RUN_CAP; i++) l.push_back(i % 2 ? RunSpec{8, true, 0} : RunSpec{rl[(i / 2) % 4], false, 0});
            check(build(l, bw, 5), l, bw, uint32_t(bw) & 3);
        }
    }
    // random run lists
    for (int it = 0; it < 600; it++) {
        const int bw = int(rnd() % 33);
        std::vector<RunSpec> runs;
        for (uint32_t k = 1 + rnd() % 12; k > 0; k--) runs.push_back({1 + rnd() % 40, bool(rnd() & 1), rnd() % 8});
        check(build(runs, bw, rnd() % 25), runs, bw, rnd() % 4);
    }
    printf("cases %ld groups %ld fast %ld failures %ld\n", g_cases, g_groups, g_fast, g_fail);
    return g_fail ? 1 : 0;
}
