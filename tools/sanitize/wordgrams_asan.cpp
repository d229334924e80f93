// AddressSanitizer + UBSan over the word n-gram repetition host statement (wg_host of td_wordgrams_args.h, which td_word_ngrams_host
// is): it cuts a document into words, sorts the occurrences of every n by their words' bytes and compares neighbours: this is where a read
// past a document's or the text's end would show.  Random texts of an alphabet that makes short words and repeated n-grams dense, each in
// a heap buffer of exactly its size, with offsets in a heap buffer of exactly theirs, cut into documents at random positions; the columns
// must add up (both groups the two single ones side by side, duplicates and word characters within their bounds).  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/wordgrams_asan.cpp -o /tmp/td_wordgrams_asan && /tmp/td_wordgrams_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "td_wordgrams_args.h"

namespace {

const char* kAlphabet[] = {"a", "b", " ", " ", "\n", "\xC3\xA9", "\t", "ab"};
constexpr int kSyms = sizeof kAlphabet / sizeof kAlphabet[0], kCols = td::WG_COLS;

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
        int64_t* rows[4];
        int64_t tot[4][kCols];
        for (int groups = 1; groups <= 3; ++groups) {
            rows[groups] = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs * kCols));
            if (td::wg_host(text, off, n_docs, groups, rows[groups], tot[groups]) != 0) abort();
            ++calls;
        }
        for (int64_t i = 0; i < n_docs * kCols; ++i) {
            const int64_t c = i % kCols, both = rows[3][i], *row = rows[3] + i - c;
            const bool top = td::wg_col_is_max((int)c), dup = c >= td::WG_DUP5_CHARS;
            if (both != (c < 3 ? rows[1][i] : rows[1][i] + rows[2][i]) || both < 0 || (c < 3 && rows[2][i] != both) ||
                (dup && both > row[td::WG_WORD_CHARS]) || (top && both > row[(c - 3) % 2 ? td::WG_WORD_CHARS : td::WG_WORDS]) ||
                row[td::WG_WORD_CHARS] > row[td::WG_CHARS] || row[td::WG_CHARS] > off[i / kCols + 1] - off[i / kCols]) {
                fprintf(stderr, "the columns do not add up: round %d entry %lld\n", r, (long long)i);
                return 1;
            }
        }
        for (int groups = 1; groups <= 3; ++groups) free(rows[groups]);
        free(off);
        free(text);
    }
    printf("wordgrams_asan: %lld calls, no report\n", calls);
    return 0;
}
