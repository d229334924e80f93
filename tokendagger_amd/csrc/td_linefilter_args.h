// Line filtering (td_linefilter.hip): the rule, stated once.  The host statement (lf_host, which td_line_filter_host is) and the kernels
// compile what is here: the byte classes, the summary of a piece of a line with its append and its combine, a phrase's occurrence, the
// terminal mark and the decision.  Compiles on the host without HIP's runtime (tools/sanitize/linefilter_asan.cpp).
//
// A BREAK lies in front of byte p when p is 0, a document's start or the byte behind an LF: the lines are the non-empty ranges between
// two breaks, and a line's LAST byte is the one with p + 1 at a document's end or text[p] an LF.  A PIECE is a range with no break
// inside; what the rule needs of a line is a function of its piece's summary, and summaries combine.
#pragma once
#include <string.h>

#include "../../include/tokendagger_hip.h"
#include "td_rewrite_args.h"

namespace td {

constexpr int LF_COLS = TD_LF_COLS;
enum { LF_LINES = 0, LF_KEPT_LINES, LF_KEPT_BYTES, LF_FAIL_WORDS, LF_FAIL_TERMINAL, LF_FAIL_LONG_WORD, LF_FAIL_PHRASE, LF_DOC_HITS };
enum { LF_F_WORDS = 1, LF_F_TERMINAL = 2, LF_F_LONG = 4, LF_F_PHRASE = 8 };  // what lf_decide returns: 0 is KEPT
enum { LF_HOST_OK = 0, LF_HOST_INVALID = 1, LF_HOST_CAPACITY = 2 };

__host__ __device__ inline bool lf_space(uint32_t c) { return c == 0x20 || (c >= 0x09 && c <= 0x0D); }
__host__ __device__ inline uint32_t lf_lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }

inline bool lf_rules_ok(const td_line_rules* r) {
    if (!r || r->min_words < 0 || r->max_word_bytes < 0 || (r->flags & ~TD_LF_NEED_TERMINAL) || r->n_phrases < 0 ||
        r->n_phrases > TD_LF_MAX_PHRASES)
        return false;
    for (int j = 0; j < r->n_phrases; ++j) {
        const td_line_phrase& p = r->phrases[j];
        if (p.len < 1 || p.len > TD_LF_PHRASE_BYTES || (p.kind != TD_LF_PHRASE_DROP_LINE && p.kind != TD_LF_PHRASE_COUNT_DOC)) return false;
        for (int k = 0; k < p.len; ++k)
            if (p.bytes[k] == 0x0A || (p.bytes[k] >= 'A' && p.bytes[k] <= 'Z')) return false;
    }
    return true;
}

// A piece's summary.  T: int32_t inside a tile (positions from the tile's base), int64_t across tiles (positions in the text).
template <class T>
struct LfPiece {
    T len;    // bytes
    T lead;   // the leading run of non-space bytes (len: the piece is all non-space)
    T trail;  // the trailing run
    T words;  // word starts: non-space bytes with a space or the piece's start in front of them
    T wmax;   // the longest run of non-space bytes
    T last;   // the position of the last non-space byte, -1: none
    T drop;   // a drop-line phrase starts in it
};
template <class T>
__host__ __device__ inline LfPiece<T> lf_empty() { return LfPiece<T>{0, 0, 0, 0, 0, -1, 0}; }

// the byte at position p behind the piece
template <class T>
__host__ __device__ inline void lf_append(LfPiece<T>& a, bool space, bool drop, T p) {
    if (space) {
        a.trail = 0;
    } else {
        if (a.trail == 0) ++a.words;
        if (a.lead == a.len) ++a.lead;
        ++a.trail;
        a.wmax = a.wmax > a.trail ? a.wmax : a.trail;
        a.last = p;
    }
    ++a.len;
    a.drop |= (T)drop;
}

// a, then b: the trailing run meets the leading one, and one word start is taken back
template <class T>
__host__ __device__ inline LfPiece<T> lf_join(const LfPiece<T>& a, const LfPiece<T>& b) {
    LfPiece<T> r;
    const bool meet = a.trail > 0 && b.lead > 0;
    const T mid = a.trail + b.lead, m = a.wmax > b.wmax ? a.wmax : b.wmax;
    r.len = a.len + b.len;
    r.lead = a.lead == a.len ? a.len + b.lead : a.lead;
    r.trail = b.trail == b.len ? b.len + a.trail : b.trail;
    r.words = a.words + b.words - (meet ? 1 : 0);
    r.wmax = meet && mid > m ? mid : m;
    r.last = b.last >= 0 ? b.last : a.last;
    r.drop = a.drop | b.drop;
    return r;
}

// A byte range's element: head, the piece in front of its first break; tail, the piece behind its last one (brk 0: head is all of it).
template <class T>
struct LfElem {
    LfPiece<T> head, tail;
    T brk;
};
template <class T>
__host__ __device__ inline LfElem<T> lf_identity() { return LfElem<T>{lf_empty<T>(), lf_empty<T>(), 0}; }
template <class T>
__host__ __device__ inline LfElem<T> lf_combine(const LfElem<T>& a, const LfElem<T>& b) {
    LfElem<T> r;
    r.brk = a.brk | b.brk;
    r.head = a.brk ? a.head : lf_join(a.head, b.head);
    r.tail = b.brk ? b.tail : a.brk ? lf_join(a.tail, b.head) : lf_empty<T>();
    return r;
}
// the piece that is still open at the range's end
template <class T>
__host__ __device__ inline LfPiece<T> lf_open(const LfElem<T>& e) {
    LfPiece<T> r = e.head;
    if (e.brk) r = e.tail;
    return r;
}

__host__ __device__ inline LfPiece<int64_t> lf_widen(const LfPiece<int32_t>& a, int64_t base) {
    return LfPiece<int64_t>{a.len, a.lead, a.trail, a.words, a.wmax, a.last < 0 ? -1 : base + a.last, a.drop};
}

// phrase[0, len) occurs at text + i: the bytes up to the document's end de, ASCII upper case folded
__host__ __device__ inline bool lf_occurs(const uint8_t* text, int64_t i, int64_t de, const uint8_t* phrase, int len) {
    if (i + len > de) return false;
    for (int k = 0; k < len; ++k)
        if (lf_lower(text[i + k]) != phrase[k]) return false;
    return true;
}

// the line [ls, ..) whose last non-space byte is at q (-1: none) ends in a terminal mark whose bytes all lie in the line
__host__ __device__ inline bool lf_terminal(const uint8_t* text, int64_t ls, int64_t q) {
    if (q < ls) return false;
    const uint32_t c = text[q];
    if (c == '.' || c == '!' || c == '?' || c == '"') return true;
    if (q - 2 < ls) return false;
    const uint32_t x = (uint32_t)text[q - 2] << 16 | (uint32_t)text[q - 1] << 8 | c;
    return x == 0xE2809D || x == 0xE38082 || x == 0xEFBC81 || x == 0xEFBC9F;
}

// the rules a line fails, from its piece and its start: 0 is KEPT
__host__ __device__ inline int lf_decide(int64_t min_words, int64_t max_word_bytes, int flags, const uint8_t* text, const LfPiece<int64_t>& l,
                                         int64_t ls) {
    int f = 0;
    if (l.words < min_words) f |= LF_F_WORDS;
    if ((flags & TD_LF_NEED_TERMINAL) && !lf_terminal(text, ls, l.last)) f |= LF_F_TERMINAL;
    if (max_word_bytes > 0 && l.wmax > max_word_bytes) f |= LF_F_LONG;
    if (l.drop) f |= LF_F_PHRASE;
    return f;
}

// a decided line of len bytes into a row of LF_COLS sums
template <class S>
__host__ __device__ inline void lf_count(S* row, int fail, int64_t len) {
    row[LF_LINES] += 1;
    if (!fail) {
        row[LF_KEPT_LINES] += 1;
        row[LF_KEPT_BYTES] += (S)len;
    }
    row[LF_FAIL_WORDS] += (fail & LF_F_WORDS) != 0;
    row[LF_FAIL_TERMINAL] += (fail & LF_F_TERMINAL) != 0;
    row[LF_FAIL_LONG_WORD] += (fail & LF_F_LONG) != 0;
    row[LF_FAIL_PHRASE] += (fail & LF_F_PHRASE) != 0;
}

// The contract's executable statement: a document, a line, a byte at a time.  out, out_doc_offsets and totals may be null; with out
// null nothing is held against out_capacity.  Argument errors and an output that does not fit write nothing but *need (may be null).
inline int lf_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_line_rules* rules, uint8_t* out,
                   int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals, int64_t* need) {
    if (n_docs < 0 || !doc_offsets || out_capacity < 0 || !lf_rules_ok(rules) || !rewrite_offsets_ok(doc_offsets, n_docs) ||
        (n_docs > 0 && !stats) || (doc_offsets[n_docs] > 0 && !text) || rewrite_overlap(text, doc_offsets[n_docs], out, out_capacity))
        return LF_HOST_INVALID;
    for (int pass = 0; pass < 2; ++pass) {  // 0: the size; 1: the results
        int64_t opos = 0;
        for (int64_t d = 0; d < n_docs; ++d) {
            const int64_t ds = doc_offsets[d], de = doc_offsets[d + 1];
            int64_t row[LF_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (pass && out_doc_offsets) out_doc_offsets[d] = opos;
            for (int64_t ls = ds; ls < de;) {
                LfPiece<int64_t> l = lf_empty<int64_t>();
                int64_t p = ls;
                for (bool last = false; !last; ++p) {
                    bool drop = false;
                    for (int j = 0; j < rules->n_phrases; ++j) {
                        const td_line_phrase& ph = rules->phrases[j];
                        if (!lf_occurs(text, p, de, ph.bytes, ph.len)) continue;
                        if (ph.kind == TD_LF_PHRASE_DROP_LINE) drop = true;
                        else ++row[LF_DOC_HITS];
                    }
                    lf_append(l, lf_space(text[p]), drop, p);
                    last = text[p] == 0x0A || p + 1 == de;
                }
                const int fail = lf_decide(rules->min_words, rules->max_word_bytes, rules->flags, text, l, ls);
                lf_count(row, fail, p - ls);
                if (!fail) {
                    if (pass && out) memcpy(out + opos, text + ls, (size_t)(p - ls));
                    opos += p - ls;
                }
                ls = p;
            }
            if (pass) {
                for (int c = 0; c < LF_COLS; ++c) {
                    stats[d * LF_COLS + c] = row[c];
                    if (totals) totals[c] += row[c];
                }
            }
        }
        if (!pass) {
            if (need) *need = opos;
            if (out && opos > out_capacity) return LF_HOST_CAPACITY;
            if (totals) memset(totals, 0, sizeof(int64_t) * LF_COLS);
        } else if (out_doc_offsets) {
            out_doc_offsets[n_docs] = opos;
        }
    }
    return LF_HOST_OK;
}

// ---- the kernels' arguments ---------------------------------------------------------------------------------------------------------------
struct LfArgs : RewriteArgs {  // (flags: not used; counts[0]: the output's bytes, the rest 0)
    td_line_rules rules;
    unsigned long long* stats;   // [n_docs][LF_COLS]
    unsigned long long* totals;  // [LF_COLS], may be null
    LfElem<int64_t>* elems;      // [tiles]: the tiles' elements (td_lf_carry)
    LfPiece<int64_t>* carry;     // [2 * tiles]: the open piece that ends in front of the tile, the one that begins behind it (td_lf_prefix)
    uint16_t* masks;             // [256 * tiles]: a window's kept bytes, bit k: byte k of the window
};

}  // namespace td
