// Per-document duplicate-line and duplicate-paragraph statistics (td_repetition.hip): what the kernels, the host library
// (td_api_repetition.cpp) and the stand-alone sanitizer program (tools/sanitize/repetition_asan.cpp) share: the columns, the rule of one
// byte, the scan's element and its combine, the hash family's constants, the table's word, the host statement and the kernels'
// arguments.  The rule is the contract in include/tokendagger_hip.h.
//
// Both kinds of unit are one thing: a maximal run of CONTENT bytes inside one document.  For lines every byte but LF is content.  For
// paragraphs an LF is content too when the bytes on both sides of it are non-LF bytes of the same document: a single LF inside a
// paragraph belongs to it, leading and trailing ones and runs of two or more do not.  So whether a byte is content, and whether a unit
// ends at it, is decided by the byte and three neighbours (rp_byte); which unit it belongs to is a segmented scan (RpElem, rp_combine).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "td_common.h"
#include "td_rewrite_args.h"

namespace td {

constexpr int RP_COLS = 12;  // TD_RP_COLS
enum { RP_UNITS = 0, RP_BYTES, RP_CHARS, RP_DUP_UNITS, RP_DUP_BYTES, RP_DUP_CHARS, RP_KIND_COLS };  // a kind's columns; paragraphs: + 6
constexpr int RP_LINES = 1, RP_PARAS = 2;  // TD_RP_LINES, TD_RP_PARAS; a kind k (0 lines, 1 paragraphs) is the group 1 << k
constexpr int64_t RP_MAX_BYTES = 1ll << 40;  // a unit's start is 40 bits of the table's word
TD_HD bool rp_groups_ok(int groups) { return groups != 0 && (groups & ~(RP_LINES | RP_PARAS)) == 0; }
TD_HD bool rp_is_char(uint32_t x) { return (x & 0xC0u) != 0x80u; }

// ---- the rule of one byte -------------------------------------------------------------------------------------------------------------------
// x: byte p of the document [ds, de).  prev_lf: p == ds or text[p - 1] is LF; next_lf: p + 1 == de or text[p + 1] is LF; next2_lf:
// p + 2 >= de or text[p + 2] is LF.
enum { RP_CONTENT = 1, RP_END = 2 };  // bits of a kind's answer: the byte is content of a unit; a unit ends with it
TD_HD int rp_byte(int kind, uint32_t x, bool prev_lf, bool next_lf, bool next2_lf) {
    const bool lf = x == 0x0A;
    if (kind == 0) return lf ? 0 : RP_CONTENT | (next_lf ? RP_END : 0);
    if (lf) return !prev_lf && !next_lf ? RP_CONTENT : 0;
    return RP_CONTENT | (next_lf && next2_lf ? RP_END : 0);
}
// whether a unit of `kind` that reaches up to e (its last byte, a non-LF byte, is e - 1) ends there, in a document that ends at de >= e
TD_HD bool rp_ends_at(int kind, const uint8_t* text, int64_t e, int64_t de) {
    if (e == de) return true;
    if (text[e] != 0x0A) return false;
    return kind == 0 || e + 1 == de || text[e + 1] == 0x0A;
}

struct RpCursor {  // the document that holds the current byte
    int64_t D, ds, de;
};
// (p is below doc_off[n_docs]: a document that holds it follows; empty ones are stepped over)
TD_HD void rp_advance(const int64_t* doc_off, int64_t p, RpCursor& c) {
    while (p >= c.de) {
        ++c.D;
        c.ds = c.de;
        c.de = doc_off[c.D + 1];
    }
}

// ---- the scan -------------------------------------------------------------------------------------------------------------------------------
// What a stretch of bytes leaves behind for one kind: s the start of the unit that is open at its end, where the stretch holds one
// (the byte behind its last delimiter; a document's first byte is one) or -1; h, pw, c: the polynomial hash of the content bytes since,
// the multiplier's power of their count, the characters among them.
struct RpElem {
    int64_t s;
    uint64_t h, pw, c;
};
constexpr uint64_t RP_MUL = 0x9E3779B97F4A7C15ull;  // the polynomial's multiplier modulo 2^64 (odd)
constexpr uint64_t RP_MIX_DOC = 0xC2B2AE3D27D4EB4Full, RP_MIX_LEN = 0x165667B19E3779F9ull, RP_MIX_KIND = 0x27D4EB2F165667C5ull;
TD_HD RpElem rp_identity() { return RpElem{-1, 0, 1, 0}; }
TD_HD RpElem rp_open(int64_t s) { return RpElem{s, 0, 1, 0}; }  // behind a delimiter: a unit may begin at s
TD_HD RpElem rp_combine(const RpElem& a, const RpElem& b) {      // a in front of b; associative
    if (b.s >= 0) return b;
    return RpElem{a.s, a.h * b.pw + b.h, a.pw * b.pw, a.c + b.c};
}
TD_HD void rp_append(RpElem& e, uint32_t x) {  // a content byte behind e
    e.h = e.h * RP_MUL + (x + 1);
    e.pw *= RP_MUL;
    e.c += rp_is_char(x);
}
// the key of a unit: its hash, finalised (splitmix64's mix), with its document, kind and length mixed in
TD_HD uint64_t rp_key(uint64_t h, int64_t doc, int kind, int64_t len) {
    uint64_t z = h ^ ((uint64_t)doc * RP_MIX_DOC) ^ ((uint64_t)len * RP_MIX_LEN) ^ (kind ? RP_MIX_KIND : 0);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The table's word, all a prober needs of a resident unit: 23 bits of tag (never 0: an empty slot is the word 0), the kind, the unit's
// start.  Its length, its document and its bytes are checked against the text and the prober's own.
constexpr int RP_START_BITS = 40;
TD_HD uint64_t rp_word(uint64_t key, int kind, int64_t start) {
    return (((key >> (RP_START_BITS + 1)) | 1ull) << (RP_START_BITS + 1)) | ((uint64_t)kind << RP_START_BITS) | (uint64_t)start;
}
// slots of a table for n units: a power of two, at least 2 n
TD_HD uint64_t rp_slots(int64_t n) {
    uint64_t s = 64;
    while (s < 2 * (uint64_t)n) s <<= 1;
    return s;
}
// max_units == 0: a unit every 16 bytes of text and one a document (a text of shorter units is told its need: TD_E_CAPACITY)
inline int64_t rp_default_units(int64_t n_bytes, int64_t n_docs) { return n_bytes / 16 + n_docs + 1024; }

// ---- the host statement (td_repetition_host) ------------------------------------------------------------------------------------------------
// Documents one by one: the units by rp_byte, then sorted by length and bytes; a unit that equals the one before it is a duplicate.  No
// hash.  Argument errors write nothing.  Returns 0, or 1 for bad arguments.
inline int rp_host(const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!doc_off || n_docs < 0 || (n_docs > 0 && !stats) || !rp_groups_ok(groups) || !rewrite_offsets_ok(doc_off, n_docs)) return 1;
    if (doc_off[n_docs] > 0 && !text) return 1;
    int64_t tot[RP_COLS] = {0};
    struct Unit { int64_t start, len, chars; };
    std::vector<Unit> units;
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t ds = doc_off[d], de = doc_off[d + 1];
        int64_t* row = stats + d * RP_COLS;
        for (int c = 0; c < RP_COLS; ++c) row[c] = 0;
        for (int kind = 0; kind < 2; ++kind) {
            if (!(groups & (1 << kind))) continue;
            int64_t* col = row + kind * RP_KIND_COLS;
            units.clear();
            Unit u = {-1, 0, 0};
            for (int64_t p = ds; p < de; ++p) {
                const uint32_t x = text[p];
                const int r = rp_byte(kind, x, p == ds || text[p - 1] == 0x0A, p + 1 == de || text[p + 1] == 0x0A, p + 2 >= de || text[p + 2] == 0x0A);
                if (!(r & RP_CONTENT)) continue;
                if (u.start < 0) u = {p, 0, 0};
                u.len += 1;
                u.chars += rp_is_char(x);
                if (r & RP_END) {
                    units.push_back(u);
                    u.start = -1;
                }
            }
            std::sort(units.begin(), units.end(), [&](const Unit& a, const Unit& b) {
                if (a.len != b.len) return a.len < b.len;
                return memcmp(text + a.start, text + b.start, (size_t)a.len) < 0;
            });
            for (size_t i = 0; i < units.size(); ++i) {
                const Unit& v = units[i];
                col[RP_UNITS] += 1;
                col[RP_BYTES] += v.len;
                col[RP_CHARS] += v.chars;
                if (i > 0 && units[i - 1].len == v.len && memcmp(text + units[i - 1].start, text + v.start, (size_t)v.len) == 0) {
                    col[RP_DUP_UNITS] += 1;
                    col[RP_DUP_BYTES] += v.len;
                    col[RP_DUP_CHARS] += v.chars;
                }
            }
        }
        for (int c = 0; c < RP_COLS; ++c) tot[c] += row[c];
    }
    if (totals) memcpy(totals, tot, sizeof tot);
    return 0;
}

// ---- the kernels' arguments -----------------------------------------------------------------------------------------------------------------
// head (RewriteArgs): RW_H_BAD and RW_H_FULL as in every text pass; RP_H_UNITS the units the call holds, RP_H_MASK the table's slots - 1
enum { RP_H_UNITS = 2, RP_H_MASK = 3 };
struct RpArgs : RewriteArgs {   // (flags, out, out_capacity, out_doc_off, counts and tile_base are not used)
    int groups;
    int64_t max_units;
    unsigned long long* stats;   // [n_docs][RP_COLS] int64
    unsigned long long* totals;  // [RP_COLS] or null
    RpElem* carry;               // [tiles][2]: a tile's elements, then their inclusive prefixes
    unsigned long long* table;   // [rp_slots(max_units)]
};

}  // namespace td
