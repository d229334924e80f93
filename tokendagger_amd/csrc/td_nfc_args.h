// Unicode NFC normalisation (td_nfc.hip): what the kernels, the host library (td_api_nfc.cpp) and the CPU model
// (tests/twin/nfc_model.cpp) share: the table lookup, the UTF-8 unit decoder, the quick check, the segment scan and the segment
// normaliser, and what the pass adds to the rewrites' arguments (td_rewrite_args.h).  The rule is the contract in
// include/tokendagger_hip.h; the tables are generated/unicode_nfc.inc (tools/gen_unicode_nfc.py).
#pragma once
#include "generated/unicode_nfc.inc"  // (the constants; the tables themselves where TD_NFC_TABLE is defined)
#include "td_rewrite_args.h"

namespace td {

constexpr uint32_t NFC_LEAD_MIN = 0xCC;        // the UTF-8 lead byte of U+0300, the lowest code point that is no boundary

struct NfcTables {
    const uint8_t* s1;        // [TD_NFC_N_STAGE1]  block of code point >> TD_NFC_SHIFT, for code points below TD_NFC_CP_LIMIT
    const uint16_t* s2;       // [TD_NFC_N_STAGE2]  ccc | Quick_Check << 8 | has-decomposition << 10
    const uint32_t* dec_key;  // [TD_NFC_N_DEC]     code points, sorted
    const uint16_t* dec_off;  // [TD_NFC_N_DEC]     offset into dec_cps | length - 1 << 12
    const uint32_t* dec_cps;  // [TD_NFC_N_DEC_CPS]
    const uint32_t* pair_a;   // [TD_NFC_N_PAIR]    (a, b) -> c, sorted by (a, b)
    const uint32_t* pair_b;
    const uint32_t* pair_c;
};

constexpr uint32_t NFC_P_DEC = 1u << 10;
constexpr uint32_t NFC_P_BOUNDARY_MASK = 0x3FF;  // ccc == 0 and Quick_Check == Yes <=> (prop & mask) == 0
constexpr uint32_t NFC_S_BASE = 0xAC00, NFC_L_BASE = 0x1100, NFC_V_BASE = 0x1161, NFC_T_BASE = 0x11A7;
constexpr uint32_t NFC_L_COUNT = 19, NFC_V_COUNT = 21, NFC_T_COUNT = 28, NFC_N_COUNT = NFC_V_COUNT * NFC_T_COUNT,
                   NFC_S_COUNT = NFC_L_COUNT * NFC_N_COUNT;

__host__ __device__ inline uint32_t nfc_prop(const NfcTables& T, uint32_t cp) {
    if (cp >= TD_NFC_CP_LIMIT) return 0;  // (nothing from there on has a property)
    return T.s2[((uint32_t)T.s1[cp >> TD_NFC_SHIFT] << TD_NFC_SHIFT) | (cp & ((1u << TD_NFC_SHIFT) - 1))];
}
__host__ __device__ inline uint32_t nfc_ccc(uint32_t prop) { return prop & 255; }
__host__ __device__ inline uint32_t nfc_qc(uint32_t prop) { return (prop >> 8) & 3; }
__host__ __device__ inline bool nfc_boundary_prop(uint32_t prop) { return (prop & NFC_P_BOUNDARY_MASK) == 0; }

// ---- units -----------------------------------------------------------------------------------------------------------------------------
// The unit at text[p], p < end (the document's end): the length 1 .. 4 of the well-formed UTF-8 sequence (Unicode Table 3-7) that starts
// there and ends at or below `end`, with its code point in cp, or 0: byte p alone is an opaque unit.
__host__ __device__ inline int nfc_unit(const uint8_t* text, int64_t p, int64_t end, uint32_t& cp) {
    const uint32_t b0 = text[p];
    if (b0 < 0x80) { cp = b0; return 1; }
    if (b0 < 0xC2 || b0 > 0xF4) return 0;
    const int len = b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
    if (p + len > end) return 0;
    const uint32_t b1 = text[p + 1];
    const uint32_t lo = b0 == 0xE0 ? 0xA0 : b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xED ? 0x9F : b0 == 0xF4 ? 0x8F : 0xBF;
    if (b1 < lo || b1 > hi) return 0;
    if (len == 2) { cp = (b0 & 0x1F) << 6 | (b1 & 0x3F); return 2; }
    const uint32_t b2 = text[p + 2];
    if ((b2 & 0xC0) != 0x80) return 0;
    if (len == 3) { cp = (b0 & 0x0F) << 12 | (b1 & 0x3F) << 6 | (b2 & 0x3F); return 3; }
    const uint32_t b3 = text[p + 3];
    if ((b3 & 0xC0) != 0x80) return 0;
    cp = (b0 & 0x07) << 18 | (b1 & 0x3F) << 12 | (b2 & 0x3F) << 6 | (b3 & 0x3F);
    return 4;
}

// Whether a unit starts at byte p of the document [ds, de), ds <= p < de; if none does, `next` is the end of the code point that covers
// p.  A byte that is no continuation byte always starts one; a continuation byte does unless one of the three bytes in front of it, inside
// the document, leads a well-formed sequence that reaches over it.  So the units are fixed by at most three bytes of context.
__host__ __device__ inline bool nfc_unit_starts(const uint8_t* text, int64_t p, int64_t ds, int64_t de, int64_t& next) {
    if ((text[p] & 0xC0) != 0x80) return true;
    for (int j = 1; j <= 3 && p - j >= ds; ++j) {
        if ((text[p - j] & 0xC0) == 0x80) continue;
        uint32_t cp;
        const int len = nfc_unit(text, p - j, de, cp);
        if (len > j) { next = p - j + len; return false; }
        return true;
    }
    return true;
}

// The ccc of the unit that ends at p, a unit's start with ds < p (0: an opaque unit or a starter).
__host__ __device__ inline uint32_t nfc_ccc_before(const NfcTables& T, const uint8_t* text, int64_t p, int64_t ds, int64_t de) {
    if ((text[p - 1] & 0xC0) != 0x80) return 0;  // ASCII, or a lead byte cut short
    for (int j = 2; j <= 4 && p - j >= ds; ++j) {
        if ((text[p - j] & 0xC0) == 0x80) continue;
        uint32_t cp;
        return nfc_unit(text, p - j, de, cp) == j ? nfc_ccc(nfc_prop(T, cp)) : 0;
    }
    return 0;
}

// ---- quick check ------------------------------------------------------------------------------------------------------------------------
// The unit at p (a unit's start in [ds, de)) keeps its stretch from being proven NFC: a code point that is not Quick_Check Yes, or a
// non-starter whose ccc is below that of the code point in front of it.  Units led by a byte below NFC_LEAD_MIN never do.
__host__ __device__ inline bool nfc_unit_unproven(const NfcTables& T, const uint8_t* text, int64_t p, int64_t ds, int64_t de) {
    uint32_t cp;
    if (text[p] < NFC_LEAD_MIN || !nfc_unit(text, p, de, cp)) return false;
    const uint32_t prop = nfc_prop(T, cp), c = nfc_ccc(prop);
    if (nfc_qc(prop)) return true;
    return c && p > ds && nfc_ccc_before(T, text, p, ds, de) > c;
}

// ---- segments --------------------------------------------------------------------------------------------------------------------------
struct NfcSeg {
    int64_t end;     // the next boundary (or de)
    int32_t cps;     // code points of the segment (an opaque first unit is none)
    bool proven;     // the segment is its own NFC by the quick check
    bool opaque;     // its first unit is an opaque byte
};

// The segment that starts at the boundary s of the document [ds, de), s < de.
__host__ __device__ inline NfcSeg nfc_seg_scan(const NfcTables& T, const uint8_t* text, int64_t s, int64_t de) {
    NfcSeg g;
    uint32_t cp, prev = 0;
    int len = nfc_unit(text, s, de, cp);
    g.opaque = len == 0;
    g.proven = true;
    g.cps = len ? 1 : 0;
    if (len && text[s] >= NFC_LEAD_MIN) {  // (the first unit of a document may be any code point)
        const uint32_t prop = nfc_prop(T, cp);
        g.proven = nfc_qc(prop) == 0;
        prev = nfc_ccc(prop);
    }
    int64_t q = s + (len ? len : 1);
    while (q < de && text[q] >= NFC_LEAD_MIN) {
        len = nfc_unit(text, q, de, cp);
        if (!len) break;
        const uint32_t prop = nfc_prop(T, cp);
        if (nfc_boundary_prop(prop)) break;
        const uint32_t c = nfc_ccc(prop);
        if (nfc_qc(prop) || (c && prev > c)) g.proven = false;
        prev = c;
        ++g.cps;
        q += len;
    }
    g.end = q;
    return g;
}

// The first boundary at or behind p in the document [ds, de), ds <= p <= de (de itself: the next document's start, or the text's end),
// or the first unit's start at or behind `stop` when no boundary lies in front of it: a lane looks no further than its own window, so a
// long segment costs the lanes it passes over sixteen bytes each and not its length.
__host__ __device__ inline int64_t nfc_boundary_from(const NfcTables& T, const uint8_t* text, int64_t p, int64_t ds, int64_t de, int64_t stop) {
    if (p >= de || p == ds) return p;
    int64_t q = p;
    if (!nfc_unit_starts(text, p, ds, de, q)) {
        if (q >= de) return de;
    }
    while (q < de && q < stop && text[q] >= NFC_LEAD_MIN) {
        uint32_t cp;
        const int len = nfc_unit(text, q, de, cp);
        if (!len || nfc_boundary_prop(nfc_prop(T, cp))) break;
        q += len;
    }
    return q;
}

// ---- the segment normaliser --------------------------------------------------------------------------------------------------------------
// A cursor over the canonical decomposition D of the code points of text[pos, end): the code point at pos (len bytes) decomposes to
// d0 .. d(n-1), `sub` is the element.  Every unit in the range is a well-formed code point.
struct NfcCur {
    int64_t pos;
    int32_t sub, n, len;
    uint32_t d0, d1, d2, d3;
};

__host__ __device__ inline void nfc_cur_load(const NfcTables& T, const uint8_t* text, int64_t end, NfcCur& c) {
    c.sub = 0;
    c.n = 0;
    if (c.pos >= end) return;
    uint32_t cp = 0;
    c.len = nfc_unit(text, c.pos, end, cp);
    c.n = 1;
    c.d0 = cp;
    if (cp - NFC_S_BASE < NFC_S_COUNT) {
        const uint32_t si = cp - NFC_S_BASE, t = si % NFC_T_COUNT;
        c.d0 = NFC_L_BASE + si / NFC_N_COUNT;
        c.d1 = NFC_V_BASE + (si % NFC_N_COUNT) / NFC_T_COUNT;
        c.d2 = NFC_T_BASE + t;
        c.n = t ? 3 : 2;
    } else if (cp >= 0xC0 && (nfc_prop(T, cp) & NFC_P_DEC)) {
        int lo = 0, hi = TD_NFC_N_DEC;  // the key is there
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (T.dec_key[mid] <= cp) lo = mid;
            else hi = mid;
        }
        const uint32_t* q = T.dec_cps + (T.dec_off[lo] & 0xFFF);
        c.n = (int32_t)(T.dec_off[lo] >> 12) + 1;
        c.d0 = q[0];
        if (c.n > 1) c.d1 = q[1];
        if (c.n > 2) c.d2 = q[2];
        if (c.n > 3) c.d3 = q[3];
    }
}
__host__ __device__ inline bool nfc_cur_done(const NfcCur& c) { return c.n == 0; }
__host__ __device__ inline uint32_t nfc_cur_get(const NfcCur& c) { return c.sub == 0 ? c.d0 : c.sub == 1 ? c.d1 : c.sub == 2 ? c.d2 : c.d3; }
__host__ __device__ inline void nfc_cur_next(const NfcTables& T, const uint8_t* text, int64_t end, NfcCur& c) {
    if (++c.sub < c.n) return;
    c.pos += c.len;
    nfc_cur_load(T, text, end, c);
}

// The primary composite of (a, b), or 0: Hangul L + V and LV + T by arithmetic, the rest by bisection over the sorted pairs.
__host__ __device__ inline uint32_t nfc_compose(const NfcTables& T, uint32_t a, uint32_t b) {
    if (a - NFC_L_BASE < NFC_L_COUNT && b - NFC_V_BASE < NFC_V_COUNT) return NFC_S_BASE + ((a - NFC_L_BASE) * NFC_V_COUNT + (b - NFC_V_BASE)) * NFC_T_COUNT;
    if (a - NFC_S_BASE < NFC_S_COUNT && (a - NFC_S_BASE) % NFC_T_COUNT == 0 && b - (NFC_T_BASE + 1) < NFC_T_COUNT - 1) return a + (b - NFC_T_BASE);
    int lo = 0, hi = TD_NFC_N_PAIR;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t ma = T.pair_a[mid], mb = T.pair_b[mid];
        if (ma == a && mb == b) return T.pair_c[mid];
        if (ma < a || (ma == a && mb < b)) lo = mid + 1;
        else hi = mid;
    }
    return 0;
}

template <class Put>
__host__ __device__ inline void nfc_put_cp(uint32_t cp, Put& put) {
    if (cp < 0x80) {
        put((uint8_t)cp);
    } else if (cp < 0x800) {
        put((uint8_t)(0xC0 | cp >> 6)); put((uint8_t)(0x80 | (cp & 0x3F)));
    } else if (cp < 0x10000) {
        put((uint8_t)(0xE0 | cp >> 12)); put((uint8_t)(0x80 | ((cp >> 6) & 0x3F))); put((uint8_t)(0x80 | (cp & 0x3F)));
    } else {
        put((uint8_t)(0xF0 | cp >> 18)); put((uint8_t)(0x80 | ((cp >> 12) & 0x3F))); put((uint8_t)(0x80 | ((cp >> 6) & 0x3F)));
        put((uint8_t)(0x80 | (cp & 0x3F)));
    }
}

// NFC of the segment text[s, e) (UAX #15: decompose, order, compose), its bytes handed to put(byte) one by one.  No scratch memory
// whatever the length: the segment is a row of CHAINS, a chain being a starter of D (none where the segment begins with marks)
// and what follows it up to the starter that does not compose with it.  A chain is walked twice: once to learn its composed
// starter, which is put first, and once more to put the marks that were kept.  The marks between two starters of D come out in
// canonical order by one sweep per distinct ccc value among them (at most 55), each sweep also finding the next value.
template <class Put>
__host__ __device__ inline void nfc_segment(const NfcTables& T, const uint8_t* text, int64_t s, int64_t e, bool opaque_first, Put& put) {
    if (opaque_first) put(text[s++]);
    NfcCur chain;
    chain.pos = s;
    nfc_cur_load(T, text, e, chain);
    while (!nfc_cur_done(chain)) {
        NfcCur cur = chain;
        for (int pass = 0; pass < 2; ++pass) {
            cur = chain;
            uint32_t S = nfc_cur_get(cur), last = 0;
            const bool has_s = nfc_ccc(nfc_prop(T, S)) == 0;
            bool kept = false;
            if (has_s) nfc_cur_next(T, text, e, cur);
            for (;;) {
                // the marks from cur to the next starter of D, in canonical order
                const NfcCur g0 = cur;
                uint32_t v = 0;
                for (;;) {
                    uint32_t nv = 256;
                    cur = g0;
                    while (!nfc_cur_done(cur)) {
                        const uint32_t m = nfc_cur_get(cur), cm = nfc_ccc(nfc_prop(T, m));
                        if (cm == 0) break;
                        if (cm == v) {
                            const uint32_t comp = has_s && last < cm ? nfc_compose(T, S, m) : 0;
                            if (comp) {
                                S = comp;
                            } else {
                                last = cm;
                                kept = true;
                                if (pass) nfc_put_cp(m, put);
                            }
                        } else if (cm > v && cm < nv) {
                            nv = cm;
                        }
                        nfc_cur_next(T, text, e, cur);
                    }
                    if (nv == 256) break;
                    v = nv;
                }
                if (nfc_cur_done(cur)) break;
                // a starter of D: it joins the chain when nothing was kept since the chain's starter and the two compose
                const uint32_t comp = has_s && last == 0 ? nfc_compose(T, S, nfc_cur_get(cur)) : 0;
                if (!comp) break;
                S = comp;
                nfc_cur_next(T, text, e, cur);
            }
            if (pass == 0 && has_s) nfc_put_cp(S, put);
            if (!kept) break;
        }
        chain = cur;
    }
}

// put(byte) for nfc_segment: counts, stores where out is not null, and compares with the segment's own bytes
struct NfcSink {
    uint8_t* out;         // where byte n goes, or null
    const uint8_t* cmp;   // the segment's input
    int64_t cmp_len;
    int64_t n;
    bool diff;
    __host__ __device__ inline void operator()(uint8_t b) {
        if (out) out[n] = b;
        if (n >= cmp_len || cmp[n] != b) diff = true;
        ++n;
    }
};

// A segment that is not proven through the normaliser: the bytes made (stored at out where it is not null); differs: they are not
// the segment's own.
__host__ __device__ inline int64_t nfc_rewrite(const NfcTables& T, const uint8_t* text, int64_t s, const NfcSeg& g, uint8_t* out, bool& differs) {
    NfcSink sink{out, text + s, g.end - s, 0, false};
    nfc_segment(T, text, s, g.end, g.opaque, sink);
    differs = sink.diff || sink.n != sink.cmp_len;
    return sink.n;
}

// ---- counts[8], and a lane's modes, under the pass's names (the statement below and the CPU model speak them) ------------------------------
enum { NFC_C_BYTES = RW_C_BYTES, NFC_C_WORDS = RW_C_WORDS, NFC_MEASURE = RW_MEASURE, NFC_SIZE = RW_SIZE, NFC_WRITE = RW_WRITE };
enum { NFC_C_UNPROVEN = 1, NFC_C_CHANGED = 2, NFC_C_SEGMENTS = 3, NFC_C_CPS = 4, NFC_C_OPAQUE = 5, NFC_C_LONGEST = 6 };

// ---- the kernels' arguments ---------------------------------------------------------------------------------------------------------------
struct NfcArgs : RewriteArgs {  // (flags: 0 where the document is proven NFC)
    uint8_t* changed;          // [n_docs] or null
};

// The bytes >= 0xCC of the window [b, we) (inside the text) for the check: D, ds, de are the lane's document (D < 0: none yet),
// doc_of(p) the last document that starts at or below p.
template <class DocOf>
__host__ __device__ inline void nfc_check_window(const NfcArgs& a, const NfcTables& T, int64_t b, int64_t we, int64_t& D, int64_t& ds, int64_t& de,
                                                  DocOf doc_of) {
    for (int64_t p = b; p < we; ++p) {
        if (a.text[p] < NFC_LEAD_MIN) continue;
        if (D < 0 || p < ds || p >= de) {  // (p is below doc_off[n_docs]: the last document that starts at or below p holds it)
            D = doc_of(p);
            ds = a.doc_off[D];
            de = a.doc_off[D + 1];
        }
        if (nfc_unit_unproven(T, a.text, p, ds, de)) a.flags[D] = 1;
    }
}

// ---- a lane of the normaliser -----------------------------------------------------------------------------------------------------------
struct NfcLaneStats {
    uint32_t segments, cps, opaque, longest;
};

// The segments that start in the window [b, we) of the text (b < we <= total).  ub(x): the first document of the tile's table that starts
// behind x, as an index of doc_off.  MEASURE: flags, changed and st.  WRITE: the bytes from out + opos on and the output offsets of
// the documents that start in the window.  Returns the bytes the window's segments make.
template <int MODE, class Ub>
__host__ __device__ inline int64_t nfc_lane(const NfcArgs& a, const NfcTables& T, int64_t b, int64_t we, int64_t total, Ub ub, int64_t opos,
                                            NfcLaneStats& st) {
    const uint8_t* text = a.text;
    int64_t D = ub(b) - 1, ds = a.doc_off[D], de = a.doc_off[D + 1];
    int64_t p = nfc_boundary_from(T, text, b, ds, de, we);  // (at or behind we: the window owns nothing)
    // WRITE: the documents that start in [b, we), in order; kd is the next of them
    int64_t kd = 0, next_start = INT64_MAX;
    if (MODE == NFC_WRITE) {
        kd = ub(b - 1);
        next_start = kd <= a.n_docs ? a.doc_off[kd] : INT64_MAX;
    }
    int64_t n = 0;
    while (p < we) {
        while (p >= de) {  // (p < total: a document that holds it follows; empty ones are stepped over)
            ++D;
            ds = de;
            de = a.doc_off[D + 1];
        }
        if (MODE == NFC_WRITE) {
            while (next_start == p) {
                a.out_doc_off[kd] = opos + n;
                ++kd;
                next_start = kd <= a.n_docs ? a.doc_off[kd] : INT64_MAX;
            }
        }
        const NfcSeg g = nfc_seg_scan(T, text, p, de);
        if (g.proven) {
            if (MODE == NFC_WRITE)
                for (int64_t q = p; q < g.end; ++q) a.out[opos + n + (q - p)] = text[q];
            n += g.end - p;
        } else {
            bool differs;
            n += nfc_rewrite(T, text, p, g, MODE == NFC_WRITE ? a.out + opos + n : nullptr, differs);
            if (MODE == NFC_MEASURE) {
                a.flags[D] = 1;
                if (differs && a.changed) a.changed[D] = 1;
                st.segments += 1;
                st.cps += (uint32_t)g.cps;
            }
        }
        if (MODE == NFC_MEASURE) {
            st.opaque += g.opaque;
            st.longest = st.longest > (uint32_t)g.cps ? st.longest : (uint32_t)g.cps;
        }
        p = g.end;
    }
    return n;
}

}  // namespace td
