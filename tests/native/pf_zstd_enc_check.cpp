// pf_zstd_enc_check — the host model of the ZSTD encode core (csrc/pf_zstd_enc_core.h) over a file of
// inputs, built by tests/zstd_enc_cases.py with g++ (under AddressSanitizer + UBSan for the CPU tests).
//
//   pf_zstd_enc_check <cases> <results>
//
// cases:   per case  u32 kind, u32 n, n bytes (little endian); kind 1 (one job, handed to the block assembler
//          with literals and sequences of the test's own, which must regenerate the n bytes) goes on with
//          u32 nlit, nlit bytes, u32 nseq, nseq x (u16 literal length, u16 match length, u16 offset)
// results: per case  i32 status, u32 len, u32 repeat codes, u32 blocks raw, rle, compressed, len bytes
// Every input is compressed twice into heap blocks of exactly the size bound (frame header + 3 bytes per
// job + the input), so a write past it is a sanitizer report, and the frame goes through the project's
// own decompress_host. status: 0, 1 the two runs differ, 2 decompress_host refuses the frame or returns
// other bytes, 3 compress_host reports the bound as too small.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pf_zstd_enc_core.h"

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
    namespace Z = pf::zstd;
    if (argc != 3) { std::fprintf(stderr, "usage: pf_zstd_enc_check <cases> <results>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    auto W = std::make_unique<Z::EncWork>();
    auto T = std::make_unique<Z::Tables>();
    std::vector<uint8_t> lit(Z::Z_BLOCK_MAX);
    Z::EncFseScratch hand_scratch;
    size_t at = 0, cases = 0, good = 0;
    while (at + 8 <= in.size()) {
        uint32_t kind, n;
        std::memcpy(&kind, &in[at], 4);
        std::memcpy(&n, &in[at + 4], 4);
        at += 8;
        if (n > in.size() - at || (kind == 1 && (n == 0 || n > Z::ZE_BLOCK))) { std::fprintf(stderr, "bad case file\n"); return 2; }
        const size_t jobs = (size_t(n) + Z::ZE_BLOCK - 1) / Z::ZE_BLOCK;
        const size_t bound = 9 + 3 * (jobs ? jobs : 1) + n;
        // exact-size heap copies: an overrun of source or destination is a sanitizer report
        std::unique_ptr<uint8_t[]> src(new uint8_t[n ? n : 1]), a(new uint8_t[bound]), b(new uint8_t[bound]), back(new uint8_t[n ? n : 1]);
        std::memcpy(src.get(), in.data() + at, n);
        at += n;
        Z::EncStats st{};
        size_t la = 0, lb = 0, produced = 0;
        int32_t status = 0;
        if (kind == 1) {   // the assembler alone: frame header + one block
            uint32_t nlit, nseq;
            std::memcpy(&nlit, &in[at], 4);
            if (nlit > Z::ZE_BLOCK) { std::fprintf(stderr, "bad case file\n"); return 2; }
            std::memcpy(Z::ew_lit(*W), &in[at + 4], nlit);
            std::memcpy(&nseq, &in[at + 4 + nlit], 4);
            if (nseq > Z::ZE_SEQ_MAX) { std::fprintf(stderr, "bad case file\n"); return 2; }
            at += 8 + nlit;
            for (uint32_t i = 0; i < nseq; i++, at += 6) {
                std::memcpy(&W->sll[i], &in[at], 2);
                std::memcpy(&W->sml[i], &in[at + 2], 2);
                std::memcpy(&W->sof[i], &in[at + 4], 2);
            }
            W->nlit = nlit;
            W->nseq = nseq;
            Z::fse_enc_predefined(Z::K_LL, W->fll, hand_scratch);
            Z::fse_enc_predefined(Z::K_OF, W->fof, hand_scratch);
            Z::fse_enc_predefined(Z::K_ML, W->fml, hand_scratch);
            la = Z::frame_header_put(n, a.get());
            la += Z::assemble_host(*W, src.get(), n, true, false, a.get() + la, &st);
            std::memcpy(b.get(), a.get(), la);
            lb = la;
        } else if (Z::compress_host(src.get(), n, a.get(), bound, &la, *W, &st) != Z::Z_OK) status = 3;
        if (!status && kind != 1 && (Z::compress_host(src.get(), n, b.get(), bound, &lb, *W) != Z::Z_OK || la != lb || std::memcmp(a.get(), b.get(), la) != 0))
            status = 1;
        if (!status && (Z::decompress_host(a.get(), la, back.get(), n, &produced, *T, lit.data()) != Z::Z_OK || produced != n ||
                        std::memcmp(back.get(), src.get(), n) != 0))
            status = 2;
        const uint32_t len = status == 3 ? 0 : uint32_t(la);
        const uint32_t extra[4] = {uint32_t(st.rep_codes), uint32_t(st.blocks_raw), uint32_t(st.blocks_rle), uint32_t(st.blocks_compressed)};
        std::fwrite(&status, 4, 1, out);
        std::fwrite(&len, 4, 1, out);
        std::fwrite(extra, 4, 4, out);
        if (len) std::fwrite(a.get(), 1, len, out);
        cases++;
        good += status == 0;
    }
    std::fclose(out);
    std::printf("cases %zu good %zu\n", cases, good);
    return 0;
}
