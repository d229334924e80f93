// AddressSanitizer + UBSan over the text statistics' host statement (ts_host of td_textstats_args.h, which td_text_stats_host is) and
// over the kernels' window walk as the CPU model runs it (tests/twin/textstats_model.cpp): both look three bytes in front of a position,
// two behind it and back to a line's last visible character, inside the document only: this is where a read past a document's or the
// text's end would show.  Random texts of an alphabet that makes events dense, each in a heap buffer of exactly its size, with offsets
// in a heap buffer of exactly theirs, cut into documents at random positions; the model at tile sizes 64 and 256 and every base shift
// must give the host statement's rows.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/textstats_asan.cpp tests/twin/textstats_model.cpp tokendagger_amd/csrc/td_tables.cpp \
//       tokendagger_amd/csrc/td_regex.cpp -o /tmp/td_textstats_asan && /tmp/td_textstats_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" int textstats_host(const uint8_t* text, const int64_t* off, int64_t n_docs, int groups, int64_t* stats, int64_t* totals);
extern "C" int textstats_model(const uint8_t* text, const int64_t* off, int64_t n_docs, int groups, int tile, int shift, int64_t* stats,
                               int64_t* totals, int64_t* info);

namespace {

const char* kAlphabet[] = {" ", "\n", "\r", ".", "#", "{", "-", "\xE2\x80\xA2", "\xE2\x80\xA6", "\xE3\x80\x82", "\xE2\x80\x9D", "a", "A", "9",
                           "\xC3\xA9", "\xE4\xB8\xAD", "\xCC\x81", "\x80", "\xE2"};
constexpr int kSyms = sizeof kAlphabet / sizeof kAlphabet[0], kCols = 21;

uint64_t g_state = 88172645463325252ull;
uint32_t rnd(uint32_t n) {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)((g_state >> 11) % n);
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 4000;
    long long calls = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<uint8_t> s;
        const int syms = (int)rnd(r % 50 == 0 ? 700 : 70);
        for (int i = 0; i < syms; ++i) {
            const char* a = kAlphabet[rnd(kSyms)];
            s.insert(s.end(), a, a + strlen(a));
        }
        const int64_t n = (int64_t)s.size(), n_docs = 1 + rnd(7);
        uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
        if (n) memcpy(text, s.data(), (size_t)n);
        int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
        off[0] = 0;
        off[n_docs] = n;
        for (int64_t d = 1; d < n_docs; ++d) off[d] = rnd((uint32_t)n + 1);
        for (int64_t d = 1; d < n_docs; ++d)  // (sorted: an insertion sort over at most six entries)
            for (int64_t e = d; e > 1 && off[e - 1] > off[e]; --e) { const int64_t x = off[e]; off[e] = off[e - 1]; off[e - 1] = x; }
        int64_t* want = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs * kCols));
        int64_t* got = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs * kCols));
        int64_t wt[kCols], gt[kCols], info[4];
        for (int groups = 1; groups <= 3; ++groups) {
            if (textstats_host(text, off, n_docs, groups, want, wt) != 0) abort();
            ++calls;
            for (int tile = 64; tile <= 256; tile *= 4) {
                const int shift = (int)rnd(16);
                if (textstats_model(text, off, n_docs, groups, tile, shift, got, gt, info) != 0) abort();
                ++calls;
                if (memcmp(want, got, sizeof(int64_t) * (size_t)(n_docs * kCols)) || memcmp(wt, gt, sizeof wt)) {
                    fprintf(stderr, "the model differs from the host statement: round %d groups %d tile %d shift %d\n", r, groups, tile, shift);
                    return 1;
                }
            }
        }
        free(got);
        free(want);
        free(off);
        free(text);
    }
    printf("textstats_asan: %lld calls, no report\n", calls);
    return 0;
}
