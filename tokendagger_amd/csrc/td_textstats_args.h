// Per-document text statistics (td_textstats.hip): what the kernels, the host library (td_api_textstats.cpp), the CPU model
// (tests/twin/textstats_model.cpp) and the stand-alone sanitizer program (tools/sanitize/textstats_asan.cpp) share: the columns, the
// rule of one byte (ts_step), a window's classes and its walk, the host statement, and what the pass adds to the text passes'
// arguments (td_rewrite_args.h).  The rule is the contract in include/tokendagger_hip.h.
//
// Everything is decided looking backwards.  A byte has the value classify_at gives it inside its document (class + F_CONT); an event is
// counted at one byte: a character at its first byte, a word at its first character, a word with a letter at its first letter, a
// word's length at the first space behind it or at the document's last byte, a line at its LF or at the document's last byte when that
// is no LF, a bullet at the line's first visible character.  What such a byte needs to know of the text in front of it is four "last
// position before me" values (TsLane): the last LF, the last space byte, the last visible byte, the last letter byte, each of no use
// when it lies in front of the document (compared with ds where it is used, never reset).
#pragma once
#include <string.h>

#include "td_common.h"
#include "td_rewrite_args.h"

#if defined(__clang__)
#define TS_UNROLL _Pragma("unroll")
#else
#define TS_UNROLL _Pragma("GCC unroll 16")
#endif

namespace td {

constexpr int TS_COLS = 21;  // TD_TS_COLS
enum {
    TS_BYTES = 0, TS_CHARS, TS_UPPER, TS_LOWER, TS_LETTER_OTHER, TS_MARK, TS_NUMBER, TS_SPACE, TS_NON_ASCII, TS_WORDS, TS_WORDS_ALPHA,
    TS_WORD_MAX, TS_LINES, TS_LINES_BLANK, TS_LINE_MAX, TS_END_TERMINAL, TS_END_ELLIPSIS, TS_START_BULLET, TS_HASHES, TS_ELLIPSES, TS_CURLY
};
constexpr int TS_LOCAL = 1, TS_RUNS = 2;  // TD_TS_LOCAL, TD_TS_RUNS
constexpr uint32_t TS_RUNS_COLS = (1u << TS_WORDS_ALPHA) | (1u << TS_WORD_MAX) | (1u << TS_LINES_BLANK) | (1u << TS_LINE_MAX) |
                                  (1u << TS_END_TERMINAL) | (1u << TS_END_ELLIPSIS) | (1u << TS_START_BULLET);
constexpr uint32_t TS_LOCAL_COLS = ((1u << TS_COLS) - 1) & ~TS_RUNS_COLS;
constexpr uint32_t TS_MAX_COLS = (1u << TS_WORD_MAX) | (1u << TS_LINE_MAX);  // kept by maxima; every other column is a sum
TD_HD bool ts_groups_ok(int groups) { return groups != 0 && (groups & ~(TS_LOCAL | TS_RUNS)) == 0; }
TD_HD bool ts_is_max(int c) { return (TS_MAX_COLS >> c) & 1u; }

// the last LF, space byte, visible byte and letter byte in front of the current byte (-1: none in the text)
struct TsLane {
    int64_t lf, sp, vis, let;
    bool prev_space;  // the byte in front of the current one is a space byte of the same document
};
// a lane's sums for the document it is in (n[TS_WORD_MAX] and n[TS_LINE_MAX] are not used) and its two maxima
struct TsAcc {
    uint32_t n[TS_COLS];
    int64_t wmax, lmax;
};
TD_HD int64_t ts_acc_col(const TsAcc& A, int c) { return c == TS_WORD_MAX ? A.wmax : c == TS_LINE_MAX ? A.lmax : (int64_t)A.n[c]; }
TD_HD int64_t ts_max(int64_t x, int64_t y) { return x > y ? x : y; }

// ---- the class of a byte inside its document [ds, de) ---------------------------------------------------------------------------------------
struct TsSrc {  // classify_at's view of one document: nothing in front of ds or behind de exists
    const uint8_t* text;
    int64_t lo, hi;
    TD_HD uint32_t byte(int64_t i) const { return text[i]; }
    TD_HD bool doc(int64_t) const { return false; }
};
TD_HD uint32_t ts_class(const Tables& T, const uint8_t* ascii, const uint8_t* text, int64_t p, uint32_t x, int64_t ds, int64_t de) {
    return x < 0x80 ? ascii[x] : classify_at(T, TsSrc{text, ds, de}, p);
}

// ---- the rule of one byte -------------------------------------------------------------------------------------------------------------------
// Byte p of the document [ds, de): x its value, v its class + F_CONT.  L: the lane's look-back in front of p, moved behind it here.
// Reads text at p - 3 .. p + 2 and at the line's last visible character, inside the document only.
template <int G>
TD_HD void ts_step(const uint8_t* text, int64_t p, uint32_t x, uint32_t v, int64_t ds, int64_t de, TsLane& L, TsAcc& A) {
    const uint32_t cls = v & CLS_MASK;
    const bool start = !(v & F_CONT), space = in_set(M_S, cls), letter = in_set(M_L, cls);
    const bool last = p + 1 == de, after_space = p == ds || L.prev_space, lf = x == 0x0A;
    if (G & TS_LOCAL) {
        if (start) {
            A.n[TS_CHARS] += 1;
            A.n[TS_UPPER] += cls == C_UP;
            A.n[TS_LOWER] += cls == C_LW;
            A.n[TS_LETTER_OTHER] += cls == C_LB;
            A.n[TS_MARK] += cls == C_MK;
            A.n[TS_NUMBER] += cls == C_NUM;
            A.n[TS_SPACE] += space;
            A.n[TS_NON_ASCII] += x >= 0x80;
            A.n[TS_WORDS] += !space && after_space;
            if (x == 0xE2 && p + 3 <= de && text[p + 1] == 0x80 && text[p + 2] == 0xA6) A.n[TS_ELLIPSES] += 1;
        }
        A.n[TS_HASHES] += x == '#';
        A.n[TS_CURLY] += x == '{' || x == '}';
        // a run of three or more dots, at its third
        if (x == '.' && p - 2 >= ds && text[p - 1] == '.' && text[p - 2] == '.' && !(p - 3 >= ds && text[p - 3] == '.')) A.n[TS_ELLIPSES] += 1;
        A.n[TS_LINES] += lf || last;
    }
    if (G & TS_RUNS) {
        const int64_t ls = ts_max(L.lf + 1, ds), ws = ts_max(L.sp + 1, ds);  // where the line and (p no space) the word begin
        if (start && !space) {
            if (L.vis < ls) {  // the line's first visible character
                bool bullet = x == '-' || x == '*';
                if (x == 0xE2 && p + 3 <= de) {
                    const uint32_t b1 = text[p + 1], b2 = text[p + 2];
                    bullet = (b1 == 0x80 && (b2 == 0xA2 || b2 == 0xA3)) || (b1 == 0x97 && b2 == 0xA6);
                }
                A.n[TS_START_BULLET] += bullet;
            }
            A.n[TS_WORDS_ALPHA] += letter && L.let < ws;  // the word's first letter
        }
        if (space && !after_space) A.wmax = ts_max(A.wmax, p - ws);  // a word ended in front of p
        if (!space && last) A.wmax = ts_max(A.wmax, de - ws);
        if (space) L.sp = p;
        else L.vis = p;
        if (letter) L.let = p;
        if (lf || last) {  // a line ends: at the LF, or behind the document's last byte
            A.lmax = ts_max(A.lmax, (lf ? p : de) - ls);
            if (L.vis < ls) {
                A.n[TS_LINES_BLANK] += 1;
            } else {
                const int64_t q = L.vis;  // the last byte of the line's last visible character
                const uint32_t y = text[q];
                bool term = y == '.' || y == '!' || y == '?' || y == '"';
                bool ell = y == '.' && q - 2 >= ls && text[q - 1] == '.' && text[q - 2] == '.';
                if (y >= 0x80 && q - 2 >= ds) {  // (a lead at q - 2 with its two bytes inside the document is one character)
                    const uint32_t c0 = text[q - 2], c1 = text[q - 1];
                    term = (c0 == 0xE2 && c1 == 0x80 && y == 0x9D) || (c0 == 0xE3 && c1 == 0x80 && y == 0x82) ||
                           (c0 == 0xEF && c1 == 0xBC && (y == 0x81 || y == 0x9F));
                    ell = c0 == 0xE2 && c1 == 0x80 && y == 0xA6;
                }
                A.n[TS_END_TERMINAL] += term;
                A.n[TS_END_ELLIPSIS] += ell;
            }
            if (lf) L.lf = p;
        }
    }
    L.prev_space = space;
}

// ---- a window: 16 bytes at b0 (16-byte aligned address), of which [b, we) lie in the text ---------------------------------------------------
struct TsCursor {  // the document that holds the current byte
    int64_t D, ds, de;
};
// (p is below doc_off[n_docs]: a document that holds it follows; empty ones are stepped over)
TD_HD bool ts_advance(const int64_t* doc_off, int64_t p, TsCursor& c) {
    if (p < c.de) return false;
    do {
        ++c.D;
        c.ds = c.de;
        c.de = doc_off[c.D + 1];
    } while (p >= c.de);
    return true;
}
TD_HD uint32_t ts_get(const uint32_t w[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
TD_HD bool ts_window_ascii(const uint32_t w[4]) { return ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) == 0; }

// the window's bytes into w (zero outside [b, we)): the model's and the sanitizer program's load; the kernels load 16 bytes at once
TD_HD void ts_load_bytes(const uint8_t* text, int64_t b0, int64_t b, int64_t we, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int64_t p = b; p < we; ++p) w[(p - b0) >> 2] |= (uint32_t)text[p] << (8 * ((p - b0) & 3));
}

// The classes of the window's bytes into c, and into S the last LF, space byte, visible byte and letter byte of the window (-1: none).
// cur: the document of b, by value; not looked at when the window has no byte >= 0x80 (an ASCII byte's class needs no document).
TD_HD void ts_window_classes(const Tables& T, const uint8_t* ascii, const uint8_t* text, const int64_t* doc_off, int64_t b0, int64_t b,
                             int64_t we, const uint32_t w[4], TsCursor cur, uint32_t c[4], TsLane& S) {
    const bool plain = ts_window_ascii(w);
    c[0] = c[1] = c[2] = c[3] = 0;
    S.lf = S.sp = S.vis = S.let = -1;
TS_UNROLL
    for (int k = 0; k < 16; ++k) {
        const int64_t p = b0 + k;
        if (p < b || p >= we) continue;
        const uint32_t x = ts_get(w, k);
        uint32_t v;
        if (plain) {
            v = ascii[x];
        } else {
            ts_advance(doc_off, p, cur);
            v = ts_class(T, ascii, text, p, x, cur.ds, cur.de);
        }
        c[k >> 2] |= v << (8 * (k & 3));
        if (in_set(M_S, v & CLS_MASK)) S.sp = p;
        else S.vis = p;
        if (in_set(M_L, v & CLS_MASK)) S.let = p;
        if (x == 0x0A) S.lf = p;
    }
}

// The walk: cur the document of b (moved on), L the look-back in front of b with prev_space set, A the lane's sums for cur.D.  When the
// document changes, flush(D, A) takes the sums of the document left behind; the caller takes what is in A at the end, for cur.D.
template <int G, class Flush>
TD_HD void ts_window_walk(const uint8_t* text, const int64_t* doc_off, int64_t b0, int64_t b, int64_t we, const uint32_t w[4],
                          const uint32_t c[4], TsCursor& cur, TsLane& L, TsAcc& A, Flush flush) {
TS_UNROLL
    for (int k = 0; k < 16; ++k) {
        const int64_t p = b0 + k;
        if (p < b || p >= we) continue;
        if (p >= cur.de) {
            flush(cur.D, A);
            memset(&A, 0, sizeof A);
            ts_advance(doc_off, p, cur);
        }
        ts_step<G>(text, p, ts_get(w, k), ts_get(c, k), cur.ds, cur.de, L, A);
    }
}

// whether the byte in front of b is a space byte of b's document [ds, de)
TD_HD bool ts_space_before(const Tables& T, const uint8_t* ascii, const uint8_t* text, int64_t b, int64_t ds, int64_t de) {
    return b > ds && in_set(M_S, ts_class(T, ascii, text, b - 1, text[b - 1], ds, de) & CLS_MASK);
}

// ---- the host statement (td_text_stats_host) ------------------------------------------------------------------------------------------------
// Documents one by one, bytes one by one.  Here, and not in the host library, so that it compiles without HIP's runtime.  T: the class
// tables (td_tables.h: class_tables()).  Argument errors write nothing.  Returns 0, or 1 for bad arguments.
inline int ts_host(const Tables& T, const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!doc_off || n_docs < 0 || (n_docs > 0 && !stats) || !ts_groups_ok(groups) || !rewrite_offsets_ok(doc_off, n_docs)) return 1;
    if (doc_off[n_docs] > 0 && !text) return 1;
    int64_t tot[TS_COLS] = {0};
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t ds = doc_off[d], de = doc_off[d + 1];
        TsLane L = {-1, -1, -1, -1, false};
        TsAcc A;
        memset(&A, 0, sizeof A);
        for (int64_t p = ds; p < de; ++p) {
            const uint32_t x = text[p], v = ts_class(T, T.ascii_cls, text, p, x, ds, de);
            if (groups == TS_LOCAL) ts_step<TS_LOCAL>(text, p, x, v, ds, de, L, A);
            else if (groups == TS_RUNS) ts_step<TS_RUNS>(text, p, x, v, ds, de, L, A);
            else ts_step<TS_LOCAL | TS_RUNS>(text, p, x, v, ds, de, L, A);
        }
        for (int c = 0; c < TS_COLS; ++c) {
            const int64_t v = c == TS_BYTES ? ((groups & TS_LOCAL) ? de - ds : 0) : ts_acc_col(A, c);
            stats[d * TS_COLS + c] = v;
            tot[c] = ts_is_max(c) ? ts_max(tot[c], v) : tot[c] + v;
        }
    }
    if (totals) memcpy(totals, tot, sizeof tot);
    return 0;
}

// ---- the kernels' arguments -----------------------------------------------------------------------------------------------------------------
struct TsArgs : RewriteArgs {   // (flags, out, out_capacity, out_doc_off, counts and tile_base are not used)
    const uint8_t* ascii_cls;   // the handle's class tables (Tables)
    const uint16_t* ucls1;
    const uint8_t* ucls2;
    int groups;
    unsigned long long* stats;   // [n_docs][TS_COLS] int64
    unsigned long long* totals;  // [TS_COLS] or null
    long long* carry;            // [tiles][4] (TS_RUNS): a tile's last LF, space, visible and letter byte or -1, then their inclusive prefix maxima
};
TD_HD Tables ts_tables(const uint8_t* ascii_cls, const uint16_t* ucls1, const uint8_t* ucls2) {
    Tables T = {};
    T.ascii_cls = ascii_cls;
    T.ucls1 = ucls1;
    T.ucls2 = ucls2;
    return T;
}

}  // namespace td
