// Bag models (td_bag.hip): the rule, stated once.  The host statement (bag_host, which td_bag_classify_host is), the model's builder
// (bag_check, bag_build_dict, bag_build_tree, which td_bag_model_create uploads) and the kernels compile what is here: the columns and
// limits, the delimiters, the hash, the character and word n-gram walks, the dictionary's table word and the kernels' arguments.  The
// rule is the contract in include/tokendagger_hip.h.  Compiles on the host without HIP's runtime (tools/sanitize/bag_asan.cpp).
//
// A token is decided from its own bytes and the two beside it, inside one document: whoever holds its first byte decides it.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tokendagger_hip.h"
#include "td_rewrite_args.h"

namespace td {

constexpr int BAG_COLS = TD_BAG_COLS;
enum { BAG_TOKENS = 0, BAG_IN_VOCAB, BAG_FEATURES, BAG_LONG };
constexpr int BAG_TOKEN_BYTES = TD_BAG_TOKEN_BYTES;
constexpr int BAG_SOFTMAX = TD_BAG_SOFTMAX, BAG_OVA = TD_BAG_OVA, BAG_HS = TD_BAG_HS;
constexpr int BAG_EOS = TD_BAG_EOS;
constexpr int BAG_MAX_DIM = 512, BAG_MAX_LABELS = 4096, BAG_MAX_N = 8, BAG_MAX_WORD_NGRAMS = 5;
constexpr int64_t BAG_MAX_WORDS = 1ll << 26;
static_assert(BAG_COLS == 4, "td_bag_reset: a column is the index's low bits");

__host__ __device__ inline bool bag_call_flags_ok(int flags) { return (flags & ~BAG_EOS) == 0; }

// ---- the rule of one byte, the hash ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool bag_delim(uint32_t c) { return c == 0x20u || (c - 9u) <= 4u || c == 0u; }
__host__ __device__ inline bool bag_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }
constexpr uint32_t BAG_HASH_INIT = 2166136261u;
__host__ __device__ inline uint32_t bag_step(uint32_t h, uint32_t c) { return (h ^ (uint32_t)(int32_t)(int8_t)(uint8_t)c) * 16777619u; }
__host__ __device__ inline uint64_t bag_sext(uint32_t h) { return (uint64_t)(int64_t)(int32_t)h; }
// "</s>": its bytes and its hash
__host__ __device__ inline uint32_t bag_eos_byte(int k) { return k == 0 ? '<' : k == 1 ? '/' : k == 2 ? 's' : '>'; }
__host__ __device__ inline uint32_t bag_eos_hash() {
    uint32_t h = BAG_HASH_INIT;
    for (int k = 0; k < 4; ++k) h = bag_step(h, bag_eos_byte(k));
    return h;
}

// The character n-grams that begin at position i of s = '<' + token + '>' (s(k): byte k, n_s: its length): emit(hash) in the order of n.
template <class Byte, class Emit>
__host__ __device__ inline void bag_chargrams_at(Byte s, int n_s, int i, int minn, int maxn, Emit emit) {
    if (bag_cont(s(i))) return;
    uint32_t h = BAG_HASH_INIT;
    int j = i;
    for (int n = 1; n <= maxn && j < n_s; ++n) {
        h = bag_step(h, s(j++));
        while (j < n_s && bag_cont(s(j))) h = bag_step(h, s(j++));
        if (n >= minn && !(n == 1 && (i == 0 || j == n_s))) emit(h);
    }
}
// The word n-grams that begin at token i of a document's m tokens (H(k): hash k): emit(h), 64 bits, in the order of j.
template <class Hash, class Emit>
__host__ __device__ inline void bag_wordgrams_at(Hash H, int64_t m, int64_t i, int N, Emit emit) {
    uint64_t h = bag_sext(H(i));
    for (int64_t j = i + 1; j < m && j < i + N; ++j) {
        h = h * 116049371ull + bag_sext(H(j));
        emit(h);
    }
}

// ---- the dictionary's table -------------------------------------------------------------------------------------------------------------------
// blob: 32-bit words: slots table words, then n + 1 byte offsets of the words, then the words' bytes (padded to a word).  A table word is
// the hash's bits above idx_bits with their lowest bit set (never 0: an empty slot is 0) above the word's index.  A lookup starts at slot
// h & slot_mask and walks on until it meets an empty slot; at most half the slots are taken.  The bytes decide, never the hash.
struct BagDict {
    const uint32_t* blob;
    uint32_t slot_mask, off_at, bytes_at, idx_bits;
    uint64_t blob_words;
};
__host__ __device__ inline uint32_t bag_tag(uint32_t h, uint32_t idx_bits) { return (h >> idx_bits) | 1u; }
__host__ __device__ inline uint32_t bag_slot_word(uint32_t h, uint32_t idx_bits, uint32_t w) { return bag_tag(h, idx_bits) << idx_bits | w; }
// the word whose bytes are t(0 .. L - 1), with hash h, or -1
template <class Byte>
__host__ __device__ inline int32_t bag_lookup(const BagDict& D, Byte t, int L, uint32_t h) {
    const uint32_t tag = bag_tag(h, D.idx_bits), idx_mask = (1u << D.idx_bits) - 1u;
    const uint8_t* pool = reinterpret_cast<const uint8_t*>(D.blob + D.bytes_at);
    for (uint32_t at = h & D.slot_mask;; at = (at + 1) & D.slot_mask) {
        const uint32_t v = D.blob[at];
        if (!v) return -1;
        if ((v >> D.idx_bits) != tag) continue;
        const uint32_t w = v & idx_mask, o = D.blob[D.off_at + w];
        if (D.blob[D.off_at + w + 1] - o != (uint32_t)L) continue;
        bool same = true;
        for (int j = 0; j < L && same; ++j) same = pool[o + j] == t(j);
        if (same) return (int32_t)w;
    }
}

// ---- the model as the kernels get it, by value --------------------------------------------------------------------------------------------
struct BagModel {
    BagDict dict;
    const float* win;         // [nwords + bucket][dimp]: the input matrix, a row padded to 16 bytes
    const float* wo_t;        // [dim][lpad]: the output layer transposed, n_out columns padded to lpad
    const uint32_t* hs_off;   // TD_BAG_HS: [n_labels + 1], a label's entries of hs_path
    const uint32_t* hs_path;  //            node << 1 | code, leaf to root
    int64_t nwords, bucket;
    int32_t dim, dimp, n_labels, n_out, lpad, minn, maxn, word_ngrams, loss, eos_idx;
};

struct BagWords {  // a dictionary as the caller gives it
    const uint8_t* bytes;
    const int64_t* off;  // [n + 1], from 0
    int64_t n;
};

// The model's checks.  0, or 1 with *pos the lowest word that is empty, holds a delimiter or equals an earlier word; -1 where no word
// is to blame (a parameter, a null pointer, offsets that do not start at 0, more than 2^31 bytes of words, label counts that
// increase).  order: the words sorted by (length, bytes), for the host statement.
inline int bag_check(const BagWords& w, const td_bag_params* p, const float* input, const float* output, const int64_t* label_counts,
                     int64_t* pos, std::vector<uint32_t>* order = nullptr) {
    if (pos) *pos = -1;
    if (!p || !input || !output || w.n < 0 || w.n > BAG_MAX_WORDS || !w.off || w.off[0] != 0 || (w.n > 0 && !w.bytes)) return 1;
    if (p->dim < 1 || p->dim > BAG_MAX_DIM || p->n_labels < 1 || p->n_labels > BAG_MAX_LABELS) return 1;
    if (p->loss != BAG_SOFTMAX && p->loss != BAG_OVA && p->loss != BAG_HS) return 1;
    if (p->loss == BAG_HS && (p->n_labels < 2 || !label_counts)) return 1;
    if (p->minn < 0 || p->maxn > BAG_MAX_N || p->minn > p->maxn || (p->minn == 0 && p->maxn != 0)) return 1;
    if (p->word_ngrams < 1 || p->word_ngrams > BAG_MAX_WORD_NGRAMS || p->bucket < 0 || p->bucket > (1ll << 31)) return 1;
    if (p->bucket == 0 && (p->maxn != 0 || p->word_ngrams != 1)) return 1;
    if (w.n + p->bucket < 1) return 1;
    if (p->loss == BAG_HS)
        for (int l = 1; l < p->n_labels; ++l)
            if (label_counts[l] > label_counts[l - 1] || label_counts[l] < 0) return 1;
    int64_t bad = w.n;
    for (int64_t e = 0; e < w.n && bad == w.n; ++e) {
        const int64_t len = w.off[e + 1] - w.off[e];
        if (len < 1) bad = e;
        for (int64_t i = 0; bad == w.n && i < len; ++i)
            if (bag_delim(w.bytes[w.off[e] + i])) bad = e;
    }
    if (bad == w.n && w.off[w.n] > (1ll << 31)) return 1;
    std::vector<uint32_t> ord((size_t)bad);
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
    const auto len_of = [&](uint32_t e) { return w.off[e + 1] - w.off[e]; };
    const auto cmp = [&](uint32_t x, uint32_t y) { return memcmp(w.bytes + w.off[x], w.bytes + w.off[y], (size_t)len_of(x)); };  // (equal lengths)
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
        if (len_of(x) != len_of(y)) return len_of(x) < len_of(y);
        const int c = cmp(x, y);
        return c != 0 ? c < 0 : x < y;
    });
    for (size_t i = 1; i < ord.size(); ++i)
        if (len_of(ord[i]) == len_of(ord[i - 1]) && cmp(ord[i], ord[i - 1]) == 0) bad = std::min<int64_t>(bad, ord[i]);
    if (bad < w.n) {
        if (pos) *pos = bad;
        return 1;
    }
    if (order) order->swap(ord);
    return 0;
}

// the word that equals key[0, len), by bisection over the sorted order, or -1 (the host statement's lookup: no hash)
inline int64_t bag_find(const BagWords& w, const std::vector<uint32_t>& order, const uint8_t* key, int64_t len) {
    const auto it = std::lower_bound(order.begin(), order.end(), 0u, [&](uint32_t e, uint32_t) {
        const int64_t le = w.off[e + 1] - w.off[e];
        return le != len ? le < len : memcmp(w.bytes + w.off[e], key, (size_t)len) < 0;
    });
    if (it == order.end() || w.off[*it + 1] - w.off[*it] != len || memcmp(w.bytes + w.off[*it], key, (size_t)len) != 0) return -1;
    return *it;
}

// A checked dictionary -> the blob and its description (blob points into `words`, which the caller keeps or uploads).
inline BagDict bag_build_dict(const BagWords& w, std::vector<uint32_t>& words) {
    BagDict d;
    memset(&d, 0, sizeof d);
    const uint64_t n = (uint64_t)w.n, total = (uint64_t)w.off[n];
    uint64_t slots = 16;
    while (slots < 2 * n) slots <<= 1;
    d.idx_bits = 1;
    while ((1ull << d.idx_bits) < n) ++d.idx_bits;
    d.slot_mask = (uint32_t)(slots - 1);
    d.off_at = (uint32_t)slots;
    d.bytes_at = (uint32_t)(slots + n + 1);
    d.blob_words = slots + n + 1 + (total + 3) / 4;
    words.assign((size_t)d.blob_words, 0u);
    if (total) memcpy(words.data() + d.bytes_at, w.bytes, (size_t)total);
    for (uint64_t e = 0; e <= n; ++e) words[d.off_at + e] = (uint32_t)w.off[e];
    for (uint64_t e = 0; e < n; ++e) {
        const uint8_t* p = w.bytes + w.off[e];
        const int64_t len = w.off[e + 1] - w.off[e];
        if (len > BAG_TOKEN_BYTES) continue;  // (never matches: no token is that long)
        uint32_t h = BAG_HASH_INIT;
        for (int64_t i = 0; i < len; ++i) h = bag_step(h, p[i]);
        uint32_t at = h & d.slot_mask;
        while (words[at]) at = (at + 1) & d.slot_mask;
        words[at] = bag_slot_word(h, d.idx_bits, (uint32_t)e);
    }
    d.blob = words.data();
    return d;
}

// fastText's buildTree over non-increasing counts: off[n_labels + 1] and path (node << 1 | code, leaf to root).  Returns the longest path.
inline int bag_build_tree(const int64_t* counts, int L, std::vector<uint32_t>& off, std::vector<uint32_t>& path) {
    struct Node {
        int32_t parent;
        int64_t count;
        bool binary;
    };
    std::vector<Node> tree((size_t)2 * L, Node{-1, 1000000000000000ll, false});
    for (int i = 0; i < L; ++i) tree[i].count = counts[i];
    int leaf = L - 1, node = L;
    for (int i = L; i < 2 * L - 1; ++i) {
        int mini[2];
        for (int j = 0; j < 2; ++j) {
            if (leaf >= 0 && tree[leaf].count < tree[node].count) mini[j] = leaf--;
            else mini[j] = node++;
        }
        tree[i].count = tree[mini[0]].count + tree[mini[1]].count;
        tree[mini[0]].parent = tree[mini[1]].parent = i;
        tree[mini[1]].binary = true;
    }
    off.assign((size_t)L + 1, 0u);
    path.clear();
    int depth = 0;
    for (int i = 0; i < L; ++i) {
        for (int j = i; tree[j].parent != -1; j = tree[j].parent) path.push_back((uint32_t)(tree[j].parent - L) << 1 | (tree[j].binary ? 1u : 0u));
        off[i + 1] = (uint32_t)path.size();
        depth = std::max(depth, (int)(off[i + 1] - off[i]));
    }
    return depth;
}

// ---- the host statement (td_bag_classify_host) --------------------------------------------------------------------------------------------
// Documents one by one, tokens one by one, rows one by one; sums and the output layer in double.  probs, hidden and totals may be null.
// Argument errors write nothing; *pos as bag_check.
inline int bag_host(const BagWords& w, const float* input, const float* output, const int64_t* label_counts, const td_bag_params* p,
                    const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int flags, int32_t* best, float* best_prob, float* probs,
                    float* hidden, int64_t* stats, int64_t* totals, int64_t* pos) {
    std::vector<uint32_t> order;
    if (bag_check(w, p, input, output, label_counts, pos, &order)) return 1;
    if (n_docs < 0 || !doc_off || !bag_call_flags_ok(flags) || (n_docs > 0 && (!stats || !best || !best_prob)) ||
        !rewrite_offsets_ok(doc_off, n_docs) || (doc_off[n_docs] > 0 && !text))
        return 1;
    const int dim = p->dim, L = p->n_labels, n_out = p->loss == BAG_HS ? L - 1 : L;
    const uint8_t eos[4] = {'<', '/', 's', '>'};
    const int64_t eos_idx = bag_find(w, order, eos, 4);
    std::vector<uint32_t> hs_off, hs_path;
    if (p->loss == BAG_HS) bag_build_tree(label_counts, L, hs_off, hs_path);
    int64_t tot[BAG_COLS] = {0, 0, 0, 0};
    std::vector<int64_t> rows;
    std::vector<uint32_t> H;
    std::vector<double> sum((size_t)dim), f((size_t)n_out), pr((size_t)L);
    std::vector<float> hid((size_t)dim);
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t ds = doc_off[d], de = doc_off[d + 1];
        int64_t in_vocab = 0, n_long = 0;
        rows.clear();
        H.clear();
        for (int64_t q = ds; q < de;) {
            if (bag_delim(text[q])) {
                ++q;
                continue;
            }
            int64_t e = q;
            while (e < de && !bag_delim(text[e])) ++e;
            const int64_t len = e - q;
            const uint8_t* tk = text + q;
            q = e;
            if (len > BAG_TOKEN_BYTES) {
                ++n_long;
                continue;
            }
            uint32_t h = BAG_HASH_INIT;
            for (int64_t i = 0; i < len; ++i) h = bag_step(h, tk[i]);
            H.push_back(h);
            const int64_t wi = bag_find(w, order, tk, len);
            if (wi >= 0) {
                rows.push_back(wi);
                ++in_vocab;
            }
            if (p->maxn > 0 && !(len == 4 && memcmp(tk, eos, 4) == 0)) {
                const int n_s = (int)len + 2;
                const auto s = [&](int k) -> uint32_t { return k == 0 ? '<' : k == n_s - 1 ? '>' : tk[k - 1]; };
                for (int i = 0; i < n_s; ++i)
                    bag_chargrams_at(s, n_s, i, p->minn, p->maxn, [&](uint32_t g) { rows.push_back(w.n + (int64_t)(g % (uint64_t)p->bucket)); });
            }
        }
        if (flags & BAG_EOS) {
            H.push_back(bag_eos_hash());
            if (eos_idx >= 0) {
                rows.push_back(eos_idx);
                ++in_vocab;
            }
        }
        const int64_t m = (int64_t)H.size();
        if (p->word_ngrams > 1)
            for (int64_t i = 0; i < m; ++i)
                bag_wordgrams_at([&](int64_t k) { return H[(size_t)k]; }, m, i, p->word_ngrams,
                                 [&](uint64_t g) { rows.push_back(w.n + (int64_t)(g % (uint64_t)p->bucket)); });
        const int64_t n = (int64_t)rows.size();
        const int64_t row[BAG_COLS] = {m, in_vocab, n, n_long};
        memcpy(stats + d * BAG_COLS, row, sizeof row);
        for (int c = 0; c < BAG_COLS; ++c) tot[c] += row[c];
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int64_t r : rows)
            for (int c = 0; c < dim; ++c) sum[c] += (double)input[r * dim + c];
        for (int c = 0; c < dim; ++c) hid[c] = n ? (float)sum[c] / (float)n : 0.0f;
        if (hidden) memcpy(hidden + d * dim, hid.data(), sizeof(float) * (size_t)dim);
        std::fill(pr.begin(), pr.end(), 0.0);
        int b = -1;
        if (n) {
            for (int l = 0; l < n_out; ++l) {
                double acc = 0;
                for (int c = 0; c < dim; ++c) acc += (double)output[(int64_t)l * dim + c] * (double)hid[c];
                f[l] = acc;
            }
            if (p->loss == BAG_SOFTMAX) {
                double mx = f[0], z = 0;
                for (int l = 1; l < L; ++l) mx = std::max(mx, f[l]);
                for (int l = 0; l < L; ++l) z += exp(f[l] - mx);
                for (int l = 0; l < L; ++l) pr[l] = exp(f[l] - mx) / z;
            } else if (p->loss == BAG_OVA) {
                for (int l = 0; l < L; ++l) pr[l] = 1.0 / (1.0 + exp(-f[l]));
            } else {
                for (int l = 0; l < L; ++l) {
                    double lp = 0;
                    for (uint32_t k = hs_off[l]; k < hs_off[l + 1]; ++k) {
                        const double x = (hs_path[k] & 1u) ? f[hs_path[k] >> 1] : -f[hs_path[k] >> 1];  // log s(x)
                        lp += x < 0 ? x - log1p(exp(x)) : -log1p(exp(-x));
                    }
                    pr[l] = exp(lp);
                }
            }
            b = 0;
            for (int l = 1; l < L; ++l)
                if ((float)pr[l] > (float)pr[b]) b = l;
        }
        best[d] = b;
        best_prob[d] = b < 0 ? 0.0f : (float)pr[b];
        if (probs)
            for (int l = 0; l < L; ++l) probs[d * L + l] = (float)pr[l];
    }
    if (totals) memcpy(totals, tot, sizeof tot);
    return 0;
}

// ---- the kernels' arguments ---------------------------------------------------------------------------------------------------------------
// A kept token's record: where it lies, its hash and its word (or -1).
struct BagRec {
    uint64_t start_len;  // start << 11 | len
    uint32_t hash;
    int32_t word;
};
static_assert(sizeof(BagRec) == 16 && BAG_TOKEN_BYTES < (1 << 11), "a record is one 16-byte store");

constexpr int BAG_CHUNK = 256;  // units (a document's tokens, then its EOS) a wavefront of td_bag_features takes: fixed, so that the order of
                               // every sum is the text's and the model's alone
enum { BAG_H_RECS = 0, BAG_H_WORDS = 2 };  // BagArgs::bhead: the call's records

struct BagArgs : RewriteArgs {  // (flags, out, out_capacity, out_doc_off and counts are not used; tile_base: the tiles' records)
    BagModel m;
    int call_flags;
    BagRec* rec;                  // [max_recs]
    long long* first;             // [n_docs + 1]: the records in front of a document
    float* hsum;                  // [n_docs][dimp]: the rows' sums
    float* part;                  // [chunks][2][dimp]: what a chunk adds to the documents that reach beyond it
    unsigned long long* bhead;    // [BAG_H_WORDS]
    int64_t max_recs;
    int32_t* best;
    float* best_prob;
    float* probs;                 // may be null
    float* hidden;                // may be null
    unsigned long long* stats;    // [n_docs][BAG_COLS]
    unsigned long long* totals;   // [BAG_COLS], may be null
};

}  // namespace td
