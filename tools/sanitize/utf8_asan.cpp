// AddressSanitizer + UBSan over the host statement of the UTF-8 repair (td_utf8_host is u8_host of td_utf8_args.h, which compiles
// without HIP's runtime).  It looks three bytes to either side of a position: this is where a read past a document's or the text's end
// would show.  Every string of length <= 4 over the 25 bytes at which the rule changes, each in a heap buffer of exactly its size, as
// one document and as every split into two documents, under both policies, into an output of exactly the bytes needed; the results of a
// split must be those of its halves.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc tools/sanitize/utf8_asan.cpp -o /tmp/td_utf8_asan && /tmp/td_utf8_asan
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "td_utf8_args.h"

using namespace td;

namespace {

const uint8_t kBytes[25] = {0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF,
                            0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF};

struct Result {
    std::vector<uint8_t> out;
    int64_t ooff[3], first[2], nbad[2], counts[8];
    uint8_t flags[2];
};

// one call on heap buffers of exactly the sizes the call may touch
Result run(const uint8_t* s, int n, int cut, int policy) {
    const int n_docs = cut < 0 ? 1 : 2;
    uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
    for (int i = 0; i < n; ++i) text[i] = s[i];
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
    off[0] = 0;
    if (cut >= 0) off[1] = cut;
    off[n_docs] = n;
    Result r;
    if (u8_host(text, off, n_docs, policy, nullptr, 0, nullptr, nullptr, nullptr, nullptr, r.counts) != U8_HOST_OK) abort();
    const int64_t need = r.counts[0];
    uint8_t* out = need ? (uint8_t*)malloc((size_t)need) : nullptr;
    if (need && u8_host(text, off, n_docs, policy, out, need - 1, r.ooff, r.flags, r.first, r.nbad, r.counts) != U8_HOST_CAPACITY) abort();
    if (u8_host(text, off, n_docs, policy, out, need, r.ooff, r.flags, r.first, r.nbad, r.counts) != U8_HOST_OK) abort();
    r.out.assign(out, out + need);
    free(out);
    free(off);
    free(text);
    return r;
}

}  // namespace

int main() {
    long long calls = 0;
    uint8_t s[4];
    int idx[4];
    for (int n = 0; n <= 4; ++n) {
        int total = 1;
        for (int i = 0; i < n; ++i) total *= 25;
        for (int code = 0; code < total; ++code) {
            int c = code;
            for (int i = 0; i < n; ++i) { idx[i] = c % 25; c /= 25; s[i] = kBytes[idx[i]]; }
            for (int policy = 0; policy < 2; ++policy) {
                run(s, n, -1, policy);
                ++calls;
                for (int cut = 0; cut <= n; ++cut) {
                    const Result both = run(s, n, cut, policy), left = run(s, cut, -1, policy), right = run(s + cut, n - cut, -1, policy);
                    calls += 3;
                    std::vector<uint8_t> cat = left.out;
                    cat.insert(cat.end(), right.out.begin(), right.out.end());
                    if (both.out != cat || both.ooff[1] != (int64_t)left.out.size() || both.flags[0] != left.flags[0] ||
                        both.flags[1] != right.flags[0] || both.first[0] != left.first[0] || both.first[1] != right.first[0] ||
                        both.nbad[0] != left.nbad[0] || both.nbad[1] != right.nbad[0]) {
                        fprintf(stderr, "a split differs from its halves: n %d code %d cut %d policy %d\n", n, code, cut, policy);
                        return 1;
                    }
                }
            }
        }
    }
    printf("utf8_asan: %lld calls, no report\n", calls);
    return 0;
}
