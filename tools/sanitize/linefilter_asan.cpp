// AddressSanitizer + UBSan over the host statement of the line filter (td_line_filter_host is lf_host of td_linefilter_args.h, which
// compiles without HIP's runtime).  It compares phrases forward from every byte and reads two bytes in front of a line's last non-space
// byte: this is where a read past a document's or the text's end, or in front of a line's start, would show.  Every string of length
// <= 5 over the 8 bytes at which the rule changes, each in a heap buffer of exactly its size, as one document and as every split into
// two documents, into an output of exactly the bytes needed (one byte less must be refused); the results of a split must be those of
// its halves.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/linefilter_asan.cpp -o /tmp/td_linefilter_asan && /tmp/td_linefilter_asan
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "td_linefilter_args.h"

using namespace td;

namespace {

const uint8_t kBytes[8] = {'a', 'A', ' ', '\n', '.', 0xE2, 0x80, 0x9D};

td_line_rules rules() {
    td_line_rules r;
    memset(&r, 0, sizeof r);
    r.min_words = 1;
    r.max_word_bytes = 3;
    r.flags = TD_LF_NEED_TERMINAL;
    r.n_phrases = 3;
    const char* p[3] = {"aa", "a.", "\xE2\x80\x9D"};
    for (int j = 0; j < 3; ++j) {
        r.phrases[j].len = (uint8_t)strlen(p[j]);
        r.phrases[j].kind = j == 0 ? TD_LF_PHRASE_DROP_LINE : TD_LF_PHRASE_COUNT_DOC;
        memcpy(r.phrases[j].bytes, p[j], strlen(p[j]));
    }
    return r;
}

struct Result {
    std::vector<uint8_t> out;
    int64_t ooff[3], stats[2][LF_COLS], totals[LF_COLS];
};

// one call on heap buffers of exactly the sizes the call may touch
Result run(const td_line_rules& r, const uint8_t* s, int n, int cut) {
    const int n_docs = cut < 0 ? 1 : 2;
    uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
    for (int i = 0; i < n; ++i) text[i] = s[i];
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
    off[0] = 0;
    if (cut >= 0) off[1] = cut;
    off[n_docs] = n;
    Result res;
    int64_t need = -1;
    if (lf_host(text, off, n_docs, &r, nullptr, 0, nullptr, &res.stats[0][0], nullptr, &need) != LF_HOST_OK || need < 0 || need > n) abort();
    uint8_t* out = need ? (uint8_t*)malloc((size_t)need) : nullptr;
    if (need && lf_host(text, off, n_docs, &r, out, need - 1, res.ooff, &res.stats[0][0], res.totals, nullptr) != LF_HOST_CAPACITY) abort();
    if (lf_host(text, off, n_docs, &r, out, need, res.ooff, &res.stats[0][0], res.totals, nullptr) != LF_HOST_OK) abort();
    res.out.assign(out, out + need);
    free(out);
    free(off);
    free(text);
    return res;
}

}  // namespace

int main() {
    const td_line_rules r = rules();
    if (!lf_rules_ok(&r)) abort();
    long long calls = 0;
    uint8_t s[5];
    for (int n = 0; n <= 5; ++n) {
        int total = 1;
        for (int i = 0; i < n; ++i) total *= 8;
        for (int code = 0; code < total; ++code) {
            int c = code;
            for (int i = 0; i < n; ++i) { s[i] = kBytes[c % 8]; c /= 8; }
            run(r, s, n, -1);
            ++calls;
            for (int cut = 0; cut <= n; ++cut) {
                const Result both = run(r, s, n, cut), left = run(r, s, cut, -1), right = run(r, s + cut, n - cut, -1);
                calls += 3;
                std::vector<uint8_t> cat = left.out;
                cat.insert(cat.end(), right.out.begin(), right.out.end());
                bool same = both.out == cat && both.ooff[1] == (int64_t)left.out.size() && both.ooff[2] == (int64_t)cat.size();
                for (int k = 0; k < LF_COLS; ++k)
                    same = same && both.stats[0][k] == left.stats[0][k] && both.stats[1][k] == right.stats[0][k] &&
                           both.totals[k] == left.totals[k] + right.totals[k];
                if (!same) {
                    fprintf(stderr, "a split differs from its halves: n %d code %d cut %d\n", n, code, cut);
                    return 1;
                }
            }
        }
    }
    printf("linefilter_asan: %lld calls, no report\n", calls);
    return 0;
}
