// pf_dstr_ids_check — dstr_ids16 (csrc/pf_dstr_ids.h, the id unpack of k_flat_dstr) against a plain per-entry
// reference, on the host. Built by tests/test_dstr_ids_cpu.py with -fsanitize=address,undefined and run directly.
//
// A case is a list of runs over `total` values (RLE or bit-packed at width bw), laid out as a hybrid stream's
// payloads: each run's bytes follow a header-sized gap, a packed run holds whole groups of 8 values. The run table
// is built in k_runs' row format straight from the list. The stream is then read through a frame that starts
// `shift` bytes before it (the kernel's stage starts at an aligned address before the first id byte), holds exactly
// the words the contract allows to be loaded, and is zero past the stream's end. Every 16-value group start e0 in
// [0, total), aligned or not, with n = min(16, total - e0) and with shorter n, is compared entry by entry.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pf_dstr_ids.h"

namespace {

struct RunSpec {
    uint32_t count;
    bool packed;
};

struct Case {
    std::vector<uint32_t> rt;        // table rows
    std::vector<uint8_t> stream;
    std::vector<uint32_t> want;      // reference ids, by the per-entry walk below
    uint32_t total = 0;
};

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

// One bit of a little-endian (LSB-first) stream; bits past its end are zero.
uint32_t bit_at(const std::vector<uint8_t>& s, uint64_t bit) {
    const uint64_t by = bit >> 3;
    return by < s.size() ? (s[by] >> (bit & 7)) & 1u : 0u;
}

// `cut`: bytes dropped from the stream's end (a truncated final packed run reads zeros there).
Case build(const std::vector<RunSpec>& runs, int bw, uint32_t cut) {
    Case c;
    const uint32_t vmask = bw >= 32 ? 0xffffffffu : ((1u << bw) - 1u);
    uint32_t first = 0;
    std::vector<uint32_t> data;   // per run: RLE value or bit offset
    for (const RunSpec& r : runs) {
        for (uint32_t g = 1 + rnd() % 3; g > 0; g--) c.stream.push_back(uint8_t(rnd()));   // where a header would be
        c.rt.push_back(first | (r.packed ? 0x80000000u : 0u));
        if (r.packed) {
            c.rt.push_back(uint32_t(c.stream.size() * 8));
            const uint32_t groups = (r.count + 7) / 8;
            for (uint32_t b = 0; b < groups * uint32_t(bw); b++) c.stream.push_back(uint8_t(rnd()));
        } else {
            const uint32_t v = rnd() & vmask;
            c.rt.push_back(v);
            for (int b = 0; b < (bw + 7) / 8; b++) c.stream.push_back(uint8_t(v >> (8 * b)));
        }
        first += r.count;
    }
    c.total = first;
    if (cut > c.stream.size()) cut = uint32_t(c.stream.size());
    c.stream.resize(c.stream.size() - cut);
    // the reference: entry by entry, run by linear search, value bit by bit
    uint32_t e = 0;
    for (size_t i = 0; i < runs.size(); i++) {
        for (uint32_t k = 0; k < runs[i].count; k++, e++) {
            uint32_t v = c.rt[2 * i + 1];
            if (runs[i].packed) {
                v = 0;
                for (int b = 0; b < bw; b++) v |= bit_at(c.stream, uint64_t(c.rt[2 * i + 1]) + uint64_t(k) * bw + b) << b;
            }
            c.want.push_back(v);
        }
    }
    return c;
}

long g_cases = 0, g_groups = 0, g_fail = 0;

// The frame a caller may read: words [w_lo, w_hi] only, everything else aborts the program.
struct Frame {
    std::vector<uint32_t> w;
    uint32_t operator()(uint32_t i) const {
        if (i >= w.size()) {
            fprintf(stderr, "word %u read outside the frame of %zu words\n", i, w.size());
            abort();
        }
        return w[i];
    }
};

void check(const Case& c, int bw, uint32_t shift) {
    g_cases++;
    Frame F;
    // shift bytes of other data, the stream, zeros up to the word after the last one that holds a stream bit
    std::vector<uint8_t> fb;
    for (uint32_t i = 0; i < shift; i++) fb.push_back(uint8_t(rnd() | 1u));
    fb.insert(fb.end(), c.stream.begin(), c.stream.end());
    // a truncated run's values lie past the stream: its words must be loadable as zeros
    uint64_t last_bit = uint64_t(fb.size()) * 8;
    for (size_t i = 0; 2 * i < c.rt.size(); i++)
        if (c.rt[2 * i] >> 31) {
            const uint32_t first = c.rt[2 * i] & 0x7fffffffu;
            const uint32_t end = 2 * i + 2 < c.rt.size() ? (c.rt[2 * i + 2] & 0x7fffffffu) : c.total;
            const uint64_t b = uint64_t(shift) * 8 + c.rt[2 * i + 1] + uint64_t(end - first) * bw;
            if (b > last_bit) last_bit = b;
        }
    const size_t words = size_t((last_bit + 31) / 32) + 1;   // + the word after (W(w + 1))
    F.w.assign(words, 0u);
    for (size_t i = 0; i < fb.size(); i++) F.w[i / 4] |= uint32_t(fb[i]) << (8 * (i % 4));
    const uint32_t nr = uint32_t(c.rt.size() / 2);
    for (uint32_t e0 = 0; e0 < c.total; e0++) {
        const uint32_t full = c.total - e0 < 16 ? c.total - e0 : 16;
        for (uint32_t n : {full, full / 2, 1u, 0u}) {
            uint32_t id[16];
            for (uint32_t& x : id) x = 0xdeadbeefu;
            pf::dstr_ids16(c.rt.data(), nr, c.total, e0, n, bw, int64_t(shift) * 8, F, id);
            g_groups++;
            for (uint32_t k = 0; k < 16; k++) {
                const uint32_t want = k < n ? c.want[e0 + k] : 0u;
                if (id[k] != want) {
                    if (g_fail++ < 20)
                        fprintf(stderr, "bw %d shift %u e0 %u n %u k %u: got %u, want %u\n", bw, shift, e0, n, k, id[k], want);
                }
            }
        }
    }
    // a group past the covered values gives zeros and reads nothing
    uint32_t id[16];
    pf::dstr_ids16(c.rt.data(), nr, c.total, c.total, 16, bw, int64_t(shift) * 8, F, id);
    for (uint32_t k = 0; k < 16; k++)
        if (id[k] != 0) g_fail++;
}

}  // namespace

int main() {
    for (int bw = 0; bw <= 32; bw++) {
        std::vector<std::vector<RunSpec>> layouts;
        layouts.push_back({{200, true}});                          // all bit-packed
        layouts.push_back({{64, true}, {64, true}, {40, true}});
        layouts.push_back({{200, false}});                         // all RLE
        layouts.push_back({{9, false}, {100, false}, {8, false}, {23, false}});
        {   // alternating 8-value RLE / 8-value packed runs, both phases
            std::vector<RunSpec> a, b;
            for (int i = 0; i < 12; i++) { a.push_back({8, i % 2 == 0}); b.push_back({8, i % 2 == 1}); }
            layouts.push_back(a);
            layouts.push_back(b);
        }
        // a boundary at every position within the 16 (groups start at every e0, so every phase is met
        // as well), between every pair of kinds; then two boundaries inside one group
        for (uint32_t j = 1; j < 16; j++)
            for (int kinds = 0; kinds < 4; kinds++)
                layouts.push_back({{j, bool(kinds & 1)}, {32 - j, bool(kinds & 2)}});
        for (uint32_t j = 1; j < 14; j += 3)
            for (int kinds = 0; kinds < 8; kinds++)
                layouts.push_back({{16 + j, bool(kinds & 1)}, {2, bool(kinds & 2)}, {1, bool(kinds & 4)}, {30, bool(kinds & 1)}});
        // a last partial group: totals that are no multiple of 8 or 16, packed and RLE tails
        layouts.push_back({{16, true}, {5, true}});
        layouts.push_back({{24, false}, {3, true}});
        layouts.push_back({{17, true}, {1, false}});
        layouts.push_back({{1, true}});
        for (size_t li = 0; li < layouts.size(); li++) {
            for (uint32_t shift : {0u, 1u, 3u, 15u}) {
                const Case c = build(layouts[li], bw, 0);
                check(c, bw, shift);
            }
            // the stream ends inside the last packed run
            const Case t = build(layouts[li], bw, 1 + rnd() % 5);
            check(t, bw, 2);
        }
    }
    // random run lists
    for (int it = 0; it < 400; it++) {
        const int bw = int(rnd() % 33);
        std::vector<RunSpec> runs;
        for (uint32_t k = 1 + rnd() % 12; k > 0; k--) runs.push_back({1 + rnd() % 40, bool(rnd() & 1)});
        check(build(runs, bw, rnd() % 3 == 0 ? rnd() % 4 : 0), bw, rnd() % 16);
    }
    printf("cases %ld groups %ld failures %ld\n", g_cases, g_groups, g_fail);
    return g_fail ? 1 : 0;
}
