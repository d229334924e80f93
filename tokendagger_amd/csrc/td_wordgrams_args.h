// Per-document word n-gram repetition statistics (td_wordgrams.hip): what the kernels, the host library (td_api_wordgrams.cpp) and the
// stand-alone sanitizer program (tools/sanitize/wordgrams_asan.cpp) share: the columns, the rule of one byte, a word's record, the keys,
// the host statement and the kernels' arguments.  The rule is the contract in include/tokendagger_hip.h.
//
// A word is one more kind of td_repetition's unit: a maximal run of content bytes inside one document, content being a function of the
// byte alone (not a space).  Its hash across windows, wavefronts and tiles is the same segmented scan (RpElem, rp_combine, rp_append of
// td_repetition_args.h).
#pragma once
#include "td_repetition_args.h"

namespace td {

constexpr int WG_COLS = 15;  // TD_WG_COLS
enum { WG_WORDS = 0, WG_WORD_CHARS, WG_CHARS, WG_TOP2_COUNT, WG_TOP2_CHARS, WG_DUP5_CHARS = 9 };  // TOPn: 3 + 2 (n - 2), + 1; DUPn: 9 + n - 5
constexpr int WG_TOP = 1, WG_DUP = 2;  // TD_WG_TOP, TD_WG_DUP
constexpr int WG_NO_LDS = 1;           // TD_WG_NO_LDS
constexpr int WG_TOP_LO = 2, WG_TOP_HI = 4, WG_DUP_LO = 5, WG_DUP_HI = 10;
// A document of at most this many words is resolved by one workgroup in LDS: a table of twice as many slots (a 32-bit word and a 32-bit
// count each), the words' hashes, an occurrence's slot and its flag are 27 KB, so five workgroups share a CU's 160 KB (five wavefronts a
// SIMD): the work waits on LDS atomics and on the text behind L2, which more resident wavefronts hide.  (2048 would leave two.)
constexpr int WG_LDS_WORDS = 1024;
TD_HD bool wg_groups_ok(int groups) { return groups != 0 && (groups & ~(WG_TOP | WG_DUP)) == 0; }
TD_HD bool wg_flags_ok(int flags) { return (flags & ~WG_NO_LDS) == 0; }
TD_HD bool wg_asked(int groups, int n) { return n <= WG_TOP_HI ? (groups & WG_TOP) != 0 : (groups & WG_DUP) != 0; }
TD_HD int wg_col(int n) { return n <= WG_TOP_HI ? WG_TOP2_COUNT + 2 * (n - WG_TOP_LO) : WG_DUP5_CHARS + (n - WG_DUP_LO); }
TD_HD bool wg_col_is_max(int c) { return c >= WG_TOP2_COUNT && c < WG_DUP5_CHARS; }  // totals: the maximum, not the sum

// ---- the rule of one byte -------------------------------------------------------------------------------------------------------------------
TD_HD bool wg_is_space(uint32_t x) { return x == 0x20u || (x - 0x09u) <= 4u; }  // what Python's bytes.split() splits on

// ---- a word's record ------------------------------------------------------------------------------------------------------------------------
// 16 bytes a word, in text order: the finalised hash, and the start (40 bits) with the length (24 bits, saturating: a longer word's end
// is found in the text).  Two words are equal when their bytes are; the hash and the length only say early that they are not.
struct WgWord {
    uint64_t h, sl;
};
constexpr int WG_LEN_BITS = 24;
constexpr uint64_t WG_LEN_SAT = (1ull << WG_LEN_BITS) - 1;
TD_HD WgWord wg_word(uint64_t h, int64_t start, int64_t len) {
    return WgWord{rp_key(h, 0, 0, len), ((uint64_t)start << WG_LEN_BITS) | ((uint64_t)len < WG_LEN_SAT ? (uint64_t)len : WG_LEN_SAT)};
}
TD_HD int64_t wg_start(const WgWord& w) { return (int64_t)(w.sl >> WG_LEN_BITS); }
// the key of the n-gram of the words whose hashes are hw(0) .. hw(n - 1), in the document `doc`
template <class H>
TD_HD uint64_t wg_key(H hw, int n, int64_t doc) {
    uint64_t z = 0;
    for (int j = 0; j < n; ++j) z = z * RP_MUL + hw(j);
    return rp_key(z, doc, 0, n);
}
// The global table's word: 23 bits of tag (never 0: an empty slot is the word 0) above the rank of the first word of the occurrence that
// claimed the slot (ranks are below 2^40: a word has a byte).  Beside it the slot's count, 64 bits.
TD_HD uint64_t wg_slot_word(uint64_t key, int64_t rank) { return rp_word(key, 0, rank); }
// max_words == 0: a word every four bytes of text and one a document (a text of shorter words is told its need: TD_E_CAPACITY)
inline int64_t wg_default_words(int64_t n_bytes, int64_t n_docs) { return n_bytes / 4 + n_docs + 1024; }

// ---- the host statement (td_word_ngrams_host) -----------------------------------------------------------------------------------------------
// Documents one by one: the words, then for each n the occurrences sorted by their words' lengths and bytes; a run of equal neighbours is
// one n-gram and its length the count.  No hash.  Argument errors write nothing.  Returns 0, or 1 for bad arguments.
inline int wg_host(const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!doc_off || n_docs < 0 || (n_docs > 0 && !stats) || !wg_groups_ok(groups) || !rewrite_offsets_ok(doc_off, n_docs)) return 1;
    if (doc_off[n_docs] > 0 && !text) return 1;
    int64_t tot[WG_COLS] = {0};
    struct Word { int64_t start, len, chars; };
    std::vector<Word> words;
    std::vector<int64_t> occ, count;
    std::vector<uint8_t> dup;
    for (int64_t d = 0; d < n_docs; ++d) {
        int64_t* row = stats + d * WG_COLS;
        for (int c = 0; c < WG_COLS; ++c) row[c] = 0;
        words.clear();
        Word w = {-1, 0, 0};
        for (int64_t p = doc_off[d]; p < doc_off[d + 1]; ++p) {
            const uint32_t x = text[p];
            row[WG_CHARS] += rp_is_char(x);
            if (!wg_is_space(x)) {
                if (w.start < 0) w = {p, 0, 0};
                w.len += 1;
                w.chars += rp_is_char(x);
            }
            if (w.start >= 0 && (wg_is_space(x) || p + 1 == doc_off[d + 1])) {
                words.push_back(w);
                row[WG_WORD_CHARS] += w.chars;
                w.start = -1;
            }
        }
        const int64_t W = row[WG_WORDS] = (int64_t)words.size();
        for (int n = WG_TOP_LO; n <= WG_DUP_HI; ++n) {
            if (!wg_asked(groups, n) || W < n) continue;
            const int64_t occs = W - n + 1;
            const auto cmp = [&](int64_t a, int64_t b) {  // < 0, 0, > 0
                for (int j = 0; j < n; ++j) {
                    const Word &u = words[(size_t)(a + j)], &v = words[(size_t)(b + j)];
                    if (u.len != v.len) return u.len < v.len ? -1 : 1;
                    if (const int r = memcmp(text + u.start, text + v.start, (size_t)u.len)) return r;
                }
                return 0;
            };
            occ.resize((size_t)occs);
            count.assign((size_t)occs, 0);
            for (int64_t i = 0; i < occs; ++i) occ[(size_t)i] = i;
            std::sort(occ.begin(), occ.end(), [&](int64_t a, int64_t b) { return cmp(a, b) < 0; });
            for (int64_t i = 0, j; i < occs; i = j) {
                for (j = i + 1; j < occs && cmp(occ[(size_t)i], occ[(size_t)j]) == 0; ++j) {}
                for (int64_t k = i; k < j; ++k) count[(size_t)occ[(size_t)k]] = j - i;
            }
            if (n <= WG_TOP_HI) {
                int64_t best = 0, best_chars = 0;
                for (int64_t i = 0; i < occs; ++i) {
                    int64_t chars = 0;
                    for (int j = 0; j < n; ++j) chars += words[(size_t)(i + j)].chars;
                    if (count[(size_t)i] > best || (count[(size_t)i] == best && chars > best_chars)) best = count[(size_t)i], best_chars = chars;
                }
                row[wg_col(n)] = best;
                row[wg_col(n) + 1] = best_chars;
            } else {
                dup.assign((size_t)W, 0);
                for (int64_t i = 0; i < occs; ++i)
                    if (count[(size_t)i] >= 2)
                        for (int j = 0; j < n; ++j) dup[(size_t)(i + j)] = 1;
                for (int64_t j = 0; j < W; ++j)
                    if (dup[(size_t)j]) row[wg_col(n)] += words[(size_t)j].chars;
            }
        }
        for (int c = 0; c < WG_COLS; ++c) tot[c] = wg_col_is_max(c) ? std::max(tot[c], row[c]) : tot[c] + row[c];
    }
    if (totals) memcpy(totals, tot, sizeof tot);
    return 0;
}

// ---- the kernels' arguments -----------------------------------------------------------------------------------------------------------------
// head (RewriteArgs) as td_repetition's: RP_H_UNITS the words the call holds, RP_H_MASK the global table's slots - 1 (td_wg_long).
// RpArgs: groups, max_units (the words the records have room for), stats, totals, carry ([tiles][2]: the open word's element, and
// {-1, word ends, 1, word characters}, an element whose combine adds), table (the global table's words).
enum { WG_L_DOCS = 0, WG_L_WORDS = 1, WG_L_HEAD = 2 };  // long: the documents of the global path and their words
struct WgArgs : RpArgs {
    int wflags;                     // TD_WG_NO_LDS
    int n;                          // td_wg_insert, td_wg_count, td_wg_cover: the n of this round
    WgWord* rec;                    // [max_units]
    unsigned long long* cum;        // [max_units + 1]: the word characters in front of word r
    long long* first_word;          // [n_docs + 1]: the rank of a document's first word
    unsigned long long* cnt;        // [slots]: the global table's counts
    unsigned long long* occ;        // [max_units]: an occurrence's slot, then its n-gram's count
    uint8_t* flag;                  // [max_units]: the occurrence's n-gram occurs twice
    long long* long_doc;            // [n_docs + 1]: the documents of the global path
    long long* long_first;          // [n_docs + 1]: their words in front of each, then all of them
    unsigned long long* lhead;      // [WG_L_HEAD]
};

}  // namespace td
