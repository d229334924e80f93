// AddressSanitizer + UBSan over the host statement of the bag models and the model's builder (td_bag_classify_host is bag_host of
// td_bag_args.h, td_bag_model_create uploads what bag_build_dict and bag_build_tree make; all compile without HIP's runtime).  A token
// walks to its document's end, a character n-gram up to maxn characters of '<' + token + '>', a word n-gram N - 1 tokens on: this is
// where a read past a document's or the text's end would show; the builder writes a table, offsets and bytes into one blob of exactly
// its size.  Every string of length <= 6 over 5 bytes at which the rule changes, each in a heap buffer of exactly its size, as one
// document and as every split into two, under three models; a split's integer columns must be those of its halves.  Then every word is
// looked up in the built table as the kernels do it, and the tree is built for 2 .. 40 labels.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/bag_asan.cpp -o /tmp/td_bag_asan && /tmp/td_bag_asan
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "td_bag_args.h"

using namespace td;

namespace {

const uint8_t kBytes[5] = {'a', ' ', 0xC3, 0xA9, 0x00};

struct Model {  // everything on the heap, every part of exactly its size
    uint8_t* bytes;
    int64_t* off;
    float *in, *out;
    int64_t counts[3] = {5, 3, 1};
    td_bag_params p;
    BagWords w;
    Model(const std::vector<std::string>& e, td_bag_params params) : p(params) {
        size_t total = 0;
        for (const auto& s : e) total += s.size();
        bytes = (uint8_t*)malloc(total ? total : 1);
        off = (int64_t*)malloc(sizeof(int64_t) * (e.size() + 1));
        off[0] = 0;
        for (size_t i = 0; i < e.size(); ++i) {
            memcpy(bytes + off[i], e[i].data(), e[i].size());
            off[i + 1] = off[i] + (int64_t)e[i].size();
        }
        const size_t rows = e.size() + (size_t)p.bucket, n_out = (size_t)(p.loss == BAG_HS ? p.n_labels - 1 : p.n_labels);
        in = (float*)malloc(sizeof(float) * rows * p.dim);
        out = (float*)malloc(sizeof(float) * n_out * p.dim);
        for (size_t i = 0; i < rows * p.dim; ++i) in[i] = (float)((int)(i * 37 % 257) - 128) / 64.0f;
        for (size_t i = 0; i < n_out * p.dim; ++i) out[i] = (float)((int)(i * 53 % 257) - 128) / 64.0f;
        w = BagWords{bytes, off, (int64_t)e.size()};
    }
    ~Model() { free(bytes); free(off); free(in); free(out); }
};

struct Result {
    int64_t stats[2][BAG_COLS], totals[BAG_COLS];
};

Result run(const Model& m, const uint8_t* s, int n, int cut, int flags) {
    const int n_docs = cut < 0 ? 1 : 2;
    uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
    for (int i = 0; i < n; ++i) text[i] = s[i];
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
    off[0] = 0;
    if (cut >= 0) off[1] = cut;
    off[n_docs] = n;
    int32_t* best = (int32_t*)malloc(sizeof(int32_t) * n_docs);
    float* bp = (float*)malloc(sizeof(float) * n_docs);
    float* probs = (float*)malloc(sizeof(float) * n_docs * m.p.n_labels);
    float* hid = (float*)malloc(sizeof(float) * n_docs * m.p.dim);
    Result r;
    int64_t pos = 0;
    if (bag_host(m.w, m.in, m.out, m.counts, &m.p, text, off, n_docs, flags, best, bp, probs, hid, &r.stats[0][0], r.totals, &pos) || pos != -1) abort();
    for (int d = 0; d < n_docs; ++d)
        if ((r.stats[d][BAG_FEATURES] == 0) != (best[d] == -1) || best[d] >= m.p.n_labels) abort();
    free(best); free(bp); free(probs); free(hid); free(off); free(text);
    return r;
}

}  // namespace

int main() {
    long long calls = 0, rows = 0;
    const std::vector<std::string> words = {"a", "aa", "\xC3\xA9", "a\xC3", "</s>", std::string(1025, 'a')};
    const td_bag_params params[3] = {{3, 3, 1, 3, 1, BAG_HS, 5}, {2, 2, 0, 0, 3, BAG_SOFTMAX, 4}, {5, 3, 2, 8, 5, BAG_OVA, 1}};
    for (const td_bag_params& p : params) {
        Model m(words, p);
        uint8_t s[6];
        for (int flags = 0; flags < 2; ++flags)
            for (int n = 0; n <= 6; ++n) {
                int total = 1;
                for (int i = 0; i < n; ++i) total *= 5;
                for (int code = 0; code < total; ++code) {
                    int c = code;
                    for (int i = 0; i < n; ++i) { s[i] = kBytes[c % 5]; c /= 5; }
                    rows += run(m, s, n, -1, flags).totals[BAG_FEATURES];
                    ++calls;
                    for (int cut = 0; cut <= n; cut += 1 + (n > 4)) {
                        const Result both = run(m, s, n, cut, flags), left = run(m, s, cut, -1, flags), right = run(m, s + cut, n - cut, -1, flags);
                        calls += 3;
                        for (int k = 0; k < BAG_COLS; ++k)
                            if (both.stats[0][k] != left.stats[0][k] || both.stats[1][k] != right.stats[0][k]) {
                                fprintf(stderr, "a split differs from its halves: n %d code %d cut %d column %d\n", n, code, cut, k);
                                return 1;
                            }
                    }
                }
            }
        // the dictionary as the kernels read it: every word of at most 1024 bytes is found where its hash says, by its bytes
        std::vector<uint32_t> blob;
        const BagDict D = bag_build_dict(m.w, blob);
        if (blob.size() != D.blob_words) abort();
        for (int64_t e = 0; e < m.w.n; ++e) {
            const uint8_t* wb = m.bytes + m.off[e];
            const int len = (int)(m.off[e + 1] - m.off[e]);
            if (len > BAG_TOKEN_BYTES) continue;
            uint32_t h = BAG_HASH_INIT;
            for (int i = 0; i < len; ++i) h = bag_step(h, wb[i]);
            if (bag_lookup(D, [wb](int j) { return wb[j]; }, len, h) != (int32_t)e) abort();
            if (bag_lookup(D, [wb](int j) { return (uint8_t)(wb[j] ^ 1); }, len, h) >= 0) abort();  // (the same hash, other bytes)
        }
    }
    for (int L = 2; L <= 40; ++L) {
        std::vector<int64_t> counts((size_t)L);
        for (int i = 0; i < L; ++i) counts[i] = (L - i) / 3 + 1;
        std::vector<uint32_t> off, path;
        const int depth = bag_build_tree(counts.data(), L, off, path);
        if (depth < 1 || off.size() != (size_t)L + 1 || off[L] != path.size()) abort();
        for (uint32_t e : path)
            if ((int)(e >> 1) >= L - 1) abort();
    }
    if (rows < 1000) abort();
    printf("bag_asan: %lld calls, no report\n", calls);
    return 0;
}
