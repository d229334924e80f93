// Word-list matches (td_wordlist.hip): the rule, stated once.  The host statement (wl_host, which td_word_matches_host is), the set's
// builder (wl_build, which td_word_set_create uploads) and the kernels compile what is here: the columns, flags and limits, the byte
// classes, the fold, the hash, the table's word, the set's checks and the kernels' arguments.  The rule is the contract in
// include/tokendagger_hip.h.  Compiles on the host without HIP's runtime (tools/sanitize/wordlist_asan.cpp).
//
// An occurrence is decided from its own bytes and the two beside it, inside one document: whoever holds its first byte decides it, and
// nothing is carried from one piece of the text to the next.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tokendagger_hip.h"
#include "td_rewrite_args.h"

namespace td {

constexpr int WL_COLS = TD_WL_COLS;
enum { WL_HITS = 0, WL_GROUPS, WL_FIRST_HIT, WL_HIT_BYTES };
constexpr int WL_FOLD = TD_WL_FOLD_ASCII, WL_ANYWHERE = TD_WL_ANYWHERE;  // the set's flags
constexpr int WL_NO_LDS = TD_WL_NO_LDS;                                  // the device call's flag
constexpr int WL_ENTRY_BYTES = TD_WL_ENTRY_BYTES, WL_MAX_ENTRIES = TD_WL_MAX_ENTRIES, WL_MAX_GROUP = 63;
static_assert(WL_ENTRY_BYTES == 64, "the set's lengths are one 64-bit bitmap");
static_assert(WL_MAX_ENTRIES < (1 << 16), "an entry's index is the low half of a table word");

// The LDS budget of a resident set.  td_wl_tiles keeps, whatever the set: the tile's table of documents (RC_LDS_DOCS * 4 = 17 408 B), the
// tile's bytes with their halo (16 + 4096 + 64 + 16 = 4 192 B), a list of WL_LIST start positions (4 096 B), the sums of the tile's first
// 32 documents (32 * 4 * 8 = 1 024 B), 64 counters of a small set's entries (512 B) and some hundred bytes of scan words and bitmaps:
// 27.4 KB.  A CU has 160 KB; four workgroups of 40 960 B leave 40 960 - 27 400 = 13 560 B, so the set's blob (table, offsets, bytes,
// groups) may take 13 KiB.  Gopher's eight stop words are 132 B, a block list of 400 entries of nine bytes 4 096 + 1 604 + 3 600 + 400 =
// 9.7 KB.
constexpr int WL_LDS_BYTES = 13 * 1024;
constexpr int WL_LIST = 2048;  // starts taken from a tile in one sweep; a tile of more (runs of punctuation) takes two sweeps

__host__ __device__ inline bool wl_flags_ok(int flags) { return (flags & ~(WL_FOLD | WL_ANYWHERE)) == 0; }
__host__ __device__ inline bool wl_call_flags_ok(int flags) { return (flags & ~WL_NO_LDS) == 0; }

// ---- the rule of one byte -----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool wl_word(uint32_t c) { return c >= 0x80u || (c - '0') <= 9u || ((c | 0x20u) - 'a') <= 25u || c == '_'; }
__host__ __device__ inline uint32_t wl_fold(uint32_t c, bool fold) { return fold && (c - 'A') <= 25u ? c | 0x20u : c; }

// ---- the hash: FNV-1a over the folded bytes, a byte at a time from a start; finished with the length ----------------------------------------
constexpr uint32_t WL_HASH_INIT = 2166136261u;
__host__ __device__ inline uint32_t wl_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }
__host__ __device__ inline uint32_t wl_finish(uint32_t h, int len) {
    uint32_t x = h ^ ((uint32_t)len * 0x9E3779B9u);
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    x *= 0x297A2D39u;
    x ^= x >> 15;
    return x;
}
// The table's word: the hash's high half with bit 0 set (never 0: an empty slot is 0) above the entry's index.  A lookup starts at
// slot x & mask and walks on until it meets an empty slot; at most half the slots are taken.
__host__ __device__ inline uint32_t wl_tag(uint32_t x) { return (x >> 16) | 1u; }
__host__ __device__ inline uint32_t wl_slot_word(uint32_t x, uint32_t entry) { return wl_tag(x) << 16 | entry; }

// ---- the set ---------------------------------------------------------------------------------------------------------------------------------
// What the kernels get of a set, by value.  blob: 32-bit words: slots table words, then n + 1 byte offsets of the entries, then the
// entries' bytes (padded to a word), then a group byte an entry (padded to a word).
struct WlSet {
    const uint32_t* blob;
    uint32_t blob_words, slot_mask, off_at, bytes_at, groups_at;  // the parts' first words
    uint32_t n_entries, max_len, flags;
    uint64_t lengths;    // bit L - 1: an entry of L bytes exists
    uint32_t first[8];   // bit c: an entry begins with byte c
};

struct WlList {  // a list as the caller gives it
    const uint8_t* bytes;
    const int64_t* off;     // [n + 1], from 0
    const int32_t* groups;  // [n] or null: all 0
    int64_t n;
    int flags;
};

__host__ __device__ inline bool wl_same(const uint8_t* x, const uint8_t* y, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (x[i] != y[i]) return false;
    return true;
}

// The list's checks.  0, or 1 with *pos the lowest entry that is empty, longer than 64 bytes, of a group outside 0 .. 63, holds an ASCII
// upper-case byte under WL_FOLD, or equals an earlier entry; -1 where no entry is to blame (the count, the flags, a null pointer,
// offsets that do not start at 0).  order: the entries sorted by (length, bytes), for the host statement.
inline int wl_list_check(const WlList& l, int64_t* pos, std::vector<uint32_t>* order = nullptr) {
    if (pos) *pos = -1;
    if (l.n < 1 || l.n > WL_MAX_ENTRIES || !wl_flags_ok(l.flags) || !l.off || !l.bytes || l.off[0] != 0) return 1;
    int64_t bad = l.n;
    for (int64_t e = 0; e < l.n && bad == l.n; ++e) {
        const int64_t len = l.off[e + 1] - l.off[e];
        if (len < 1 || len > WL_ENTRY_BYTES || (l.groups && (l.groups[e] < 0 || l.groups[e] > WL_MAX_GROUP))) bad = e;
        for (int64_t i = 0; bad == l.n && (l.flags & WL_FOLD) && i < len; ++i)
            if ((uint32_t)(l.bytes[l.off[e] + i] - 'A') <= 25u) bad = e;
    }
    std::vector<uint32_t> ord((size_t)bad);  // (the entries in front of the first bad one: their lengths are known to be good)
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
    const auto len_of = [&](uint32_t e) { return l.off[e + 1] - l.off[e]; };
    const auto cmp = [&](uint32_t x, uint32_t y) { return memcmp(l.bytes + l.off[x], l.bytes + l.off[y], (size_t)len_of(x)); };  // (equal lengths)
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
        if (len_of(x) != len_of(y)) return len_of(x) < len_of(y);
        const int c = cmp(x, y);
        return c != 0 ? c < 0 : x < y;
    });
    for (size_t i = 1; i < ord.size(); ++i)
        if (len_of(ord[i]) == len_of(ord[i - 1]) && cmp(ord[i], ord[i - 1]) == 0) bad = std::min<int64_t>(bad, ord[i]);
    if (bad < l.n) {
        if (pos) *pos = bad;
        return 1;
    }
    if (order) order->swap(ord);
    return 0;
}

// A checked list -> the blob and its description (blob points into `words`, which the caller keeps or uploads).
inline WlSet wl_build(const WlList& l, std::vector<uint32_t>& words) {
    WlSet s;
    memset(&s, 0, sizeof s);
    const uint32_t n = (uint32_t)l.n, total = (uint32_t)l.off[n];
    uint32_t slots = 16;
    while (slots < 2 * n) slots <<= 1;
    s.slot_mask = slots - 1;
    s.off_at = slots;
    s.bytes_at = s.off_at + n + 1;
    s.groups_at = s.bytes_at + (total + 3) / 4;
    s.blob_words = s.groups_at + (n + 3) / 4;
    s.n_entries = n;
    s.flags = (uint32_t)l.flags;
    words.assign(s.blob_words, 0u);
    uint8_t* bytes = (uint8_t*)(words.data() + s.bytes_at);
    uint8_t* groups = (uint8_t*)(words.data() + s.groups_at);
    memcpy(bytes, l.bytes, total);
    for (uint32_t e = 0; e <= n; ++e) words[s.off_at + e] = (uint32_t)l.off[e];
    for (uint32_t e = 0; e < n; ++e) {
        const int len = (int)(l.off[e + 1] - l.off[e]);
        groups[e] = (uint8_t)(l.groups ? l.groups[e] : 0);
        s.max_len = std::max<uint32_t>(s.max_len, (uint32_t)len);
        s.lengths |= 1ull << (len - 1);
        const uint8_t* p = l.bytes + l.off[e];
        s.first[p[0] >> 5] |= 1u << (p[0] & 31);
        uint32_t h = WL_HASH_INIT;
        for (int i = 0; i < len; ++i) h = wl_step(h, p[i]);
        const uint32_t x = wl_finish(h, len);
        uint32_t at = x & s.slot_mask;
        while (words[at]) at = (at + 1) & s.slot_mask;
        words[at] = wl_slot_word(x, e);
    }
    s.blob = words.data();
    return s;
}
inline bool wl_fits_lds(const WlSet& s) { return (size_t)s.blob_words * 4 <= (size_t)WL_LDS_BYTES; }

// ---- the host statement (td_word_matches_host) ---------------------------------------------------------------------------------------------
// Documents one by one, starts one by one, and at a start every length the list has: the folded bytes are looked up in the entries
// sorted by (length, bytes).  No hash.  totals and entry_hits may be null.  Argument errors write nothing; *pos as wl_list_check.
inline int wl_host(const WlList& l, const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int64_t* stats, int64_t* totals,
                   int64_t* entry_hits, int64_t* pos) {
    std::vector<uint32_t> order;
    if (wl_list_check(l, pos, &order)) return 1;
    if (n_docs < 0 || !doc_off || (n_docs > 0 && !stats) || !rewrite_offsets_ok(doc_off, n_docs) || (doc_off[n_docs] > 0 && !text)) return 1;
    const bool fold = (l.flags & WL_FOLD) != 0, anywhere = (l.flags & WL_ANYWHERE) != 0;
    uint64_t lengths = 0;
    for (int64_t e = 0; e < l.n; ++e) lengths |= 1ull << (l.off[e + 1] - l.off[e] - 1);
    int64_t tot[WL_COLS] = {0, 0, 0, 0};
    if (entry_hits) memset(entry_hits, 0, sizeof(int64_t) * (size_t)l.n);
    uint8_t key[WL_ENTRY_BYTES];
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t ds = doc_off[d], de = doc_off[d + 1];
        uint64_t hits = 0, groups = 0, hit_bytes = 0;
        int64_t first = -1;
        for (int64_t p = ds; p < de; ++p) {
            if (!anywhere && p > ds && wl_word(text[p - 1])) continue;
            for (int len = 1; len <= WL_ENTRY_BYTES && p + len <= de; ++len) {
                key[len - 1] = (uint8_t)wl_fold(text[p + len - 1], fold);
                if (!((lengths >> (len - 1)) & 1) || (!anywhere && p + len < de && wl_word(text[p + len]))) continue;
                const auto it = std::lower_bound(order.begin(), order.end(), 0u, [&](uint32_t e, uint32_t) {
                    const int64_t le = l.off[e + 1] - l.off[e];
                    return le != len ? le < len : memcmp(l.bytes + l.off[e], key, (size_t)len) < 0;
                });
                if (it == order.end() || l.off[*it + 1] - l.off[*it] != len || !wl_same(l.bytes + l.off[*it], key, len)) continue;
                ++hits;
                groups |= 1ull << (l.groups ? l.groups[*it] : 0);
                hit_bytes += (uint64_t)len;
                if (first < 0) first = p - ds;
                if (entry_hits) ++entry_hits[*it];
            }
        }
        const int64_t row[WL_COLS] = {(int64_t)hits, (int64_t)groups, first, (int64_t)hit_bytes};
        memcpy(stats + d * WL_COLS, row, sizeof row);
        tot[WL_HITS] += row[WL_HITS];
        tot[WL_GROUPS] |= row[WL_GROUPS];
        tot[WL_FIRST_HIT] += hits > 0;
        tot[WL_HIT_BYTES] += row[WL_HIT_BYTES];
    }
    if (totals) memcpy(totals, tot, sizeof tot);
    return 0;
}

// ---- the kernels' arguments ---------------------------------------------------------------------------------------------------------------
struct WlArgs : RewriteArgs {  // (flags, out, out_capacity, out_doc_off, counts and tile_base are not used)
    WlSet set;
    unsigned long long* stats;       // [n_docs][WL_COLS]
    unsigned long long* totals;      // [WL_COLS], may be null
    unsigned long long* entry_hits;  // [set.n_entries], may be null
};

}  // namespace td
