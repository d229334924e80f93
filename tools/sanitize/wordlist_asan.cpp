// AddressSanitizer + UBSan over the host statement of the word-list matches and the set's builder (td_word_matches_host is wl_host of
// td_wordlist_args.h, td_word_set_create uploads what wl_build makes; both compile without HIP's runtime).  A start walks up to 64 bytes
// forward and looks one byte back and one byte behind an occurrence: this is where a read past a document's or the text's end, or in
// front of its start, would show; the builder writes a table, offsets, bytes and groups into one blob of exactly its size.  Every string
// of length <= 6 over 5 bytes at which the rule changes, each in a heap buffer of exactly its size, as one document and as every split
// into two; the results of a split must be those of its halves.  Then every bad list, and a probe of the built table for every entry, as
// the kernels do it.  CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       -Itokendagger_amd/csrc -Iinclude tools/sanitize/wordlist_asan.cpp -o /tmp/td_wordlist_asan && /tmp/td_wordlist_asan
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "td_wordlist_args.h"

using namespace td;

namespace {

const uint8_t kBytes[5] = {'a', 'B', ' ', '+', 0xC3};

struct Heap {  // a list on the heap, every part of exactly its size
    uint8_t* bytes;
    int64_t* off;
    int32_t* groups;
    WlList list;
    Heap(const std::vector<std::string>& e, const std::vector<int>& g, int flags) {
        size_t total = 0;
        for (const auto& s : e) total += s.size();
        bytes = (uint8_t*)malloc(total ? total : 1);
        off = (int64_t*)malloc(sizeof(int64_t) * (e.size() + 1));
        groups = g.empty() ? nullptr : (int32_t*)malloc(sizeof(int32_t) * e.size());
        off[0] = 0;
        for (size_t i = 0; i < e.size(); ++i) {
            memcpy(bytes + off[i], e[i].data(), e[i].size());
            off[i + 1] = off[i] + (int64_t)e[i].size();
            if (groups) groups[i] = g[i];
        }
        list = WlList{bytes, off, groups, (int64_t)e.size(), flags};
    }
    ~Heap() { free(bytes); free(off); free(groups); }
};

struct Result {
    int64_t stats[2][WL_COLS], totals[WL_COLS];
    std::vector<int64_t> hits;
};

Result run(const WlList& l, const uint8_t* s, int n, int cut) {
    const int n_docs = cut < 0 ? 1 : 2;
    uint8_t* text = n ? (uint8_t*)malloc((size_t)n) : nullptr;
    for (int i = 0; i < n; ++i) text[i] = s[i];
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_docs + 1));
    off[0] = 0;
    if (cut >= 0) off[1] = cut;
    off[n_docs] = n;
    Result r;
    r.hits.resize((size_t)l.n);
    int64_t pos = 0;
    if (wl_host(l, text, off, n_docs, &r.stats[0][0], r.totals, r.hits.data(), &pos) || pos != -1) abort();
    free(off);
    free(text);
    return r;
}

int bad_at(const std::vector<std::string>& e, const std::vector<int>& g, int flags) {
    Heap h(e, g, flags);
    int64_t pos = -7;
    if (!wl_list_check(h.list, &pos)) abort();
    return (int)pos;
}

}  // namespace

int main() {
    long long calls = 0, found = 0;
    for (int flags = 0; flags < 4; ++flags) {
        const bool fold = flags & WL_FOLD;
        Heap h({"a", fold ? "ab" : "aB", "b a", "+", std::string(fold ? "b" : "B") + "\xC3", std::string(64, 'a')}, {0, 1, 2, 63, 5, 6}, flags);
        uint8_t s[6];
        for (int n = 0; n <= 6; ++n) {
            int total = 1;
            for (int i = 0; i < n; ++i) total *= 5;
            for (int code = 0; code < total; ++code) {
                int c = code;
                for (int i = 0; i < n; ++i) { s[i] = kBytes[c % 5]; c /= 5; }
                found += run(h.list, s, n, -1).totals[WL_HITS];
                ++calls;
                for (int cut = 0; cut <= n; ++cut) {
                    const Result both = run(h.list, s, n, cut), left = run(h.list, s, cut, -1), right = run(h.list, s + cut, n - cut, -1);
                    calls += 3;
                    bool same = true;
                    for (int k = 0; k < WL_COLS; ++k) same = same && both.stats[0][k] == left.stats[0][k] && both.stats[1][k] == right.stats[0][k];
                    for (size_t e = 0; e < both.hits.size(); ++e) same = same && both.hits[e] == left.hits[e] + right.hits[e];
                    if (!same) {
                        fprintf(stderr, "a split differs from its halves: flags %d n %d code %d cut %d\n", flags, n, code, cut);
                        return 1;
                    }
                }
            }
        }
        // the set as the kernels read it: every entry is found where its hash says, by its bytes, and the 64-byte one at a text's end
        std::vector<uint32_t> words;
        const WlSet S = wl_build(h.list, words);
        if (words.size() != S.blob_words || S.max_len != 64 || !wl_fits_lds(S)) abort();
        const uint8_t* pool = (const uint8_t*)(words.data() + S.bytes_at);
        for (uint32_t e = 0; e < S.n_entries; ++e) {
            const uint32_t o = words[S.off_at + e], len = words[S.off_at + e + 1] - o;
            uint32_t hsh = WL_HASH_INIT;
            for (uint32_t i = 0; i < len; ++i) hsh = wl_step(hsh, pool[o + i]);
            const uint32_t x = wl_finish(hsh, (int)len);
            uint32_t at = x & S.slot_mask;
            while (words[at] && words[at] != wl_slot_word(x, e)) at = (at + 1) & S.slot_mask;
            if (!words[at] || ((const uint8_t*)(words.data() + S.groups_at))[e] != (uint8_t)h.groups[e]) abort();
        }
        const std::string longest(64, fold ? 'A' : 'a');
        if (run(h.list, (const uint8_t*)longest.data(), 64, -1).stats[0][WL_HIT_BYTES] < 64) abort();
    }
    if (bad_at({"a", "", "c"}, {}, 0) != 1 || bad_at({"a", std::string(65, 'x')}, {}, 0) != 1 || bad_at({"a", "b"}, {0, 64}, 0) != 1 ||
        bad_at({"a", "B"}, {}, WL_FOLD) != 1 || bad_at({"a", "b", "a", "b"}, {}, 0) != 2 || bad_at({"a"}, {}, 4) != -1 || bad_at({}, {}, 0) != -1)
        abort();
    if (found < 1000) abort();
    printf("wordlist_asan: %lld calls, no report\n", calls);
    return 0;
}
