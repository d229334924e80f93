// AddressSanitizer + UBSan over the host statement of the address mask (td_mask_addresses_host is ma_host of td_mask_args.h, which
// compiles without HIP's runtime).  A decision walks back from an '@' and forward from an '@' or a digit: this is where a read past a
// document's or the text's end, or in front of its start, would show, and where a match that overlapped another would make the copy in
// front of it negative.  Every string of length <= 6 over the 6 bytes at which the rule changes, each in a heap buffer of exactly its size,
// as one document and as every split into two documents, into an output of exactly the bytes needed (one byte less must be refused); the
// results of a split must be those of its halves.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/mask_asan.cpp -o /tmp/td_mask_asan && /tmp/td_mask_asan
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "td_mask_args.h"

using namespace td;

namespace {

const uint8_t kBytes[6] = {'a', '1', '.', '@', '-', ' '};

td_mask_rules rules() {
    td_mask_rules r;
    memset(&r, 0, sizeof r);
    r.flags = TD_MA_EMAILS | TD_MA_IPS | TD_MA_KEEP_PRIVATE_IPS;
    r.n_emails = 3;
    r.n_ips = 2;
    const char* e[3] = {"", "<mail>", "a-placeholder-of-thirty-two-bytes"};
    for (int j = 0; j < 3; ++j) {
        r.emails[j].len = (uint8_t)(strlen(e[j]) < 32 ? strlen(e[j]) : 32);
        memcpy(r.emails[j].bytes, e[j], r.emails[j].len);
    }
    r.ips[0].len = 1;
    r.ips[0].bytes[0] = 'I';
    r.ips[1].len = 9;
    memcpy(r.ips[1].bytes, "<an IPv4>", 9);
    return r;
}

struct Result {
    std::vector<uint8_t> out;
    int64_t ooff[3], stats[2][MA_COLS], totals[MA_COLS];
};

// one call on heap buffers of exactly the sizes the call may touch
Result run(const td_mask_rules& r, const uint8_t* s, int n, int cut) {
    const int n_docs = cut < 0 ? 1 : 2;
    uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
    for (int i = 0; i < n; ++i) text[i] = s[i];
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
    off[0] = 0;
    if (cut >= 0) off[1] = cut;
    off[n_docs] = n;
    Result res;
    int64_t need = -1;
    if (ma_host(text, off, n_docs, &r, nullptr, 0, nullptr, &res.stats[0][0], nullptr, &need) != MA_HOST_OK || need < 0) abort();
    uint8_t* out = need ? (uint8_t*)malloc((size_t)need) : nullptr;
    if (need && ma_host(text, off, n_docs, &r, out, need - 1, res.ooff, &res.stats[0][0], res.totals, nullptr) != MA_HOST_CAPACITY) abort();
    if (ma_host(text, off, n_docs, &r, out, need, res.ooff, &res.stats[0][0], res.totals, nullptr) != MA_HOST_OK) abort();
    res.out.assign(out, out + need);
    free(out);
    free(off);
    free(text);
    return res;
}

}  // namespace

int main() {
    const td_mask_rules r = rules();
    if (!ma_rules_ok(&r)) abort();
    long long calls = 0, matches = 0;
    uint8_t s[6];
    for (int n = 0; n <= 6; ++n) {
        int total = 1;
        for (int i = 0; i < n; ++i) total *= 6;
        for (int code = 0; code < total; ++code) {
            int c = code;
            for (int i = 0; i < n; ++i) { s[i] = kBytes[c % 6]; c /= 6; }
            matches += run(r, s, n, -1).totals[MA_EMAILS];
            ++calls;
            for (int cut = 0; cut <= n; ++cut) {
                const Result both = run(r, s, n, cut), left = run(r, s, cut, -1), right = run(r, s + cut, n - cut, -1);
                calls += 3;
                std::vector<uint8_t> cat = left.out;
                cat.insert(cat.end(), right.out.begin(), right.out.end());
                bool same = both.out == cat && both.ooff[1] == (int64_t)left.out.size() && both.ooff[2] == (int64_t)cat.size();
                for (int k = 0; k < MA_COLS; ++k)
                    same = same && both.stats[0][k] == left.stats[0][k] && both.stats[1][k] == right.stats[0][k] &&
                           both.totals[k] == left.totals[k] + right.totals[k];
                if (!same) {
                    fprintf(stderr, "a split differs from its halves: n %d code %d cut %d\n", n, code, cut);
                    return 1;
                }
            }
        }
    }
    // what six bytes cannot hold: a quad, kept and replaced, at both ends of a buffer of exactly its size
    const char* quads[4] = {"1.1.1.1", "10.1.1.1", "1.1.1.1.", "a@a.aa 1.1.1.11"};
    for (const char* q : quads) matches += run(r, (const uint8_t*)q, (int)strlen(q), -1).totals[MA_IPS];
    if (matches < 4) abort();  // ("a@a.aa" and the quads did match)
    printf("mask_asan: %lld calls, no report\n", calls);
    return 0;
}
