// UTF-8 validation and repair (td_utf8.hip): what the kernels, the host library (td_api_utf8.cpp), the CPU model
// (tests/twin/utf8_model.cpp) and the stand-alone sanitizer program (tools/sanitize/utf8_asan.cpp) share: the unit rule (unit length,
// well-formedness, start test), the window screen, the lane walk, and what the pass adds to the rewrites' arguments
// (td_rewrite_args.h).  The rule is the contract in include/tokendagger_hip.h.
#pragma once
#include <string.h>

#include "td_rewrite_args.h"

namespace td {

constexpr int U8_REPLACE = 0, U8_IGNORE = 1;         // TD_UTF8_REPLACE, TD_UTF8_IGNORE

// ---- the unit rule -------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool u8_is_cont(uint32_t b) { return (b & 0xC0) == 0x80; }
__host__ __device__ inline bool u8_is_lead(uint32_t b) { return b >= 0xC2 && b <= 0xF4; }

// The unit that starts at text[p], p < de (the document's end): its length, and whether it is a well-formed sequence (Unicode Table 3-7)
// that ends inside the document.  Otherwise it is the maximal subpart: the lead byte plus the following bytes that still form a prefix
// of some well-formed sequence (the second byte held to the lead's own range), or a single byte that can start nothing.
__host__ __device__ inline int u8_unit(const uint8_t* text, int64_t p, int64_t de, bool& wf) {
    const uint32_t b0 = text[p];
    wf = b0 < 0x80;
    if (!u8_is_lead(b0)) return 1;
    const int need = b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
    const uint32_t lo = b0 == 0xE0 ? 0xA0 : b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xED ? 0x9F : b0 == 0xF4 ? 0x8F : 0xBF;
    if (p + 1 >= de || text[p + 1] < lo || text[p + 1] > hi) return 1;
    int len = 2;
    while (len < need && p + len < de && u8_is_cont(text[p + len])) ++len;
    wf = len == need;
    return len;
}

// The start of the unit that holds byte p of the document [ds, de), ds <= p < de.  A byte that is no continuation byte starts a unit; a
// continuation byte belongs to the unit of the nearest non-continuation byte among the three in front of it, inside the document, when
// that unit reaches over it, and starts a unit of its own otherwise.  So the units are fixed by at most three bytes of context.
__host__ __device__ inline int64_t u8_unit_start(const uint8_t* text, int64_t p, int64_t ds, int64_t de) {
    if (!u8_is_cont(text[p])) return p;
    for (int j = 1; j <= 3 && p - j >= ds; ++j) {
        if (u8_is_cont(text[p - j])) continue;
        bool wf;
        return u8_unit(text, p - j, de, wf) > j ? p - j : p;
    }
    return p;
}

// ---- the window screen ---------------------------------------------------------------------------------------------------------------------
// Bytes of a dword as SWAR lanes; a predicate is the top bit of its byte.
constexpr uint32_t U8_H = 0x80808080u, U8_L = 0x7F7F7F7Fu;
// the bytes of w at or above k (k > 0x80), given l = w & U8_L
__host__ __device__ inline uint32_t u8_ge(uint32_t w, uint32_t l, uint32_t k) { return (l + (0x100u - k) * 0x01010101u) & w & U8_H; }
// dword j of the byte stream moved n bytes towards its end: byte i of the result is byte i - n of (lo, hi), lo in front
__host__ __device__ inline uint32_t u8_back(uint32_t hi, uint32_t lo, int n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - 8 * n)); }

struct U8Masks {
    uint32_t cont, lead, ge_e0, ge_f0, bad, ge_a0, ge_90, eq_e0, eq_ed, eq_f0, eq_f4;
};

__host__ __device__ inline U8Masks u8_masks(uint32_t w) {
    const uint32_t l = w & U8_L;
    U8Masks m;
    const uint32_t ge_c0 = u8_ge(w, l, 0xC0), ge_c2 = u8_ge(w, l, 0xC2), ge_f5 = u8_ge(w, l, 0xF5);
    m.cont = w & U8_H & ~ge_c0;
    m.lead = ge_c2 & ~ge_f5;
    m.bad = (ge_c0 & ~ge_c2) | ge_f5;
    m.ge_e0 = u8_ge(w, l, 0xE0);
    m.ge_f0 = u8_ge(w, l, 0xF0);
    m.ge_a0 = u8_ge(w, l, 0xA0);
    m.ge_90 = u8_ge(w, l, 0x90);
    m.eq_e0 = m.ge_e0 & ~u8_ge(w, l, 0xE1);
    m.eq_ed = u8_ge(w, l, 0xED) & ~u8_ge(w, l, 0xEE);
    m.eq_f0 = m.ge_f0 & ~u8_ge(w, l, 0xF1);
    m.eq_f4 = u8_ge(w, l, 0xF4) & ~ge_f5;
    return m;
}

// Whether the window s[1 .. 4] (16 bytes), read as text with s[0] the four bytes in front of it and s[5] the four behind it, MAY hold
// a byte of an ill-formed subpart: the screen is exact on well-formed text (never set) and set whenever an ill-formed unit starts in
// the window or reaches into it.  An ill-formed unit that starts at p shows at one of p .. p + 3: a stray continuation byte or a byte
// that can start nothing at p itself, a lead byte at the first place where the byte it needs is missing.  So positions b .. b + 18
// are looked at, each with its three bytes in front.
//   g2(i)       byte i - 1 is a lead and byte i is in its second-byte range
//   taken(i)    byte i is consumed: g2(i), or a continuation byte behind g2(i - 1) with byte i - 2 >= E0, or a continuation byte behind a
//               continuation byte behind g2(i - 2) with byte i - 3 >= F0
//   error(i)    a lead in front without g2 | no continuation byte though byte i - 2 >= E0 or byte i - 3 >= F0 | C0, C1, F5 .. FF |
//               a continuation byte that is not taken
__host__ __device__ inline bool u8_window_suspect(const uint32_t s[6]) {
    U8Masks m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = u8_masks(s[k]);
    uint32_t g2[6];
    const U8Masks none = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const U8Masks& f = k ? m[k - 1] : none;  // (g2[0] is used from its byte 2 on: right with nothing in front of s[0])
        const uint32_t lo_a0 = u8_back(m[k].eq_e0, f.eq_e0, 1), hi_9f = u8_back(m[k].eq_ed, f.eq_ed, 1);
        const uint32_t lo_90 = u8_back(m[k].eq_f0, f.eq_f0, 1), hi_8f = u8_back(m[k].eq_f4, f.eq_f4, 1);
        const uint32_t viol = (lo_a0 & ~m[k].ge_a0) | (hi_9f & m[k].ge_a0) | (lo_90 & ~m[k].ge_90) | (hi_8f & m[k].ge_90);
        g2[k] = u8_back(m[k].lead, f.lead, 1) & m[k].cont & ~viol;
    }
    uint32_t err = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        const uint32_t lead1 = u8_back(m[k].lead, m[k - 1].lead, 1), cont1 = u8_back(m[k].cont, m[k - 1].cont, 1);
        const uint32_t e0_2 = u8_back(m[k].ge_e0, m[k - 1].ge_e0, 2), f0_3 = u8_back(m[k].ge_f0, m[k - 1].ge_f0, 3);
        const uint32_t g2_1 = u8_back(g2[k], g2[k - 1], 1), g2_2 = u8_back(g2[k], g2[k - 1], 2);
        const uint32_t taken = g2[k] | (m[k].cont & ((g2_1 & e0_2) | (cont1 & g2_2 & f0_3)));
        const uint32_t e = (lead1 & ~g2[k]) | (~m[k].cont & (e0_2 | f0_3)) | m[k].bad | (m[k].cont & ~taken);
        err |= k < 5 ? e : e & 0x00808080u;  // (behind the window: three bytes)
    }
    return (err & U8_H) != 0;
}

// ---- counts[8], and a lane's modes, under the pass's names (the statements below and the CPU model speak them) --------------------------------
enum { U8_C_BYTES = RW_C_BYTES, U8_C_WORDS = RW_C_WORDS, U8_MEASURE = RW_MEASURE, U8_SIZE = RW_SIZE, U8_WRITE = RW_WRITE };
enum { U8_C_DOCS = 1, U8_C_SUBPARTS = 2, U8_C_SUB_BYTES = 3, U8_C_BEGIN_CONT = 4, U8_C_END_LEAD = 5 };

// Whether the last unit of the document [ds, de), ds < de, is an ill-formed subpart led by a lead byte (C2 .. F4): a character cut short.
__host__ __device__ inline bool u8_ends_cut(const uint8_t* text, int64_t ds, int64_t de) {
    const int64_t q = u8_unit_start(text, de - 1, ds, de);
    bool wf;
    u8_unit(text, q, de, wf);
    return !wf && u8_is_lead(text[q]);
}

// ---- the host statement (td_utf8_host) -------------------------------------------------------------------------------------------------------
// Here, and not in the host library, so that it compiles without HIP's runtime (tools/sanitize/utf8_asan.cpp).
enum { U8_HOST_OK = 0, U8_HOST_INVALID = 1, U8_HOST_CAPACITY = 2 };

// Documents one by one, units one by one.  Argument errors write nothing; an output that does not fit writes counts[0] alone.
inline int u8_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int policy, uint8_t* out, int64_t out_capacity,
                   int64_t* out_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts) {
    if (!doc_offsets || !counts || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0) || (policy != U8_REPLACE && policy != U8_IGNORE))
        return U8_HOST_INVALID;
    if (!rewrite_offsets_ok(doc_offsets, n_docs)) return U8_HOST_INVALID;
    const int64_t total = doc_offsets[n_docs];
    if ((total > 0 && !text) || rewrite_overlap(text, total, out, out_capacity)) return U8_HOST_INVALID;
    int64_t c[U8_C_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int pass = out ? 0 : 1; pass < 2; ++pass) {  // with an output: the bytes needed first
        int64_t n = 0;
        for (int64_t d = 0; d < n_docs; ++d) {
            const int64_t ds = doc_offsets[d], de = doc_offsets[d + 1];
            int64_t first = -1, bad = 0, sub_bytes = 0;
            if (pass && out_doc_offsets) out_doc_offsets[d] = n;
            for (int64_t p = ds; p < de;) {
                bool wf;
                const int len = u8_unit(text, p, de, wf);
                if (wf) {
                    if (pass && out) memcpy(out + n, text + p, (size_t)len);
                    n += len;
                } else {
                    if (first < 0) first = p - ds;
                    ++bad;
                    sub_bytes += len;
                    if (policy == U8_REPLACE) {
                        if (pass && out) memcpy(out + n, "\xEF\xBF\xBD", 3);
                        n += 3;
                    }
                }
                p += len;
            }
            if (!pass) continue;
            if (flags) flags[d] = bad != 0;
            if (first_bad) first_bad[d] = first;
            if (n_bad) n_bad[d] = bad;
            c[U8_C_DOCS] += bad != 0;
            c[U8_C_SUBPARTS] += bad;
            c[U8_C_SUB_BYTES] += sub_bytes;
            if (ds < de) {
                c[U8_C_BEGIN_CONT] += u8_is_cont(text[ds]);
                c[U8_C_END_LEAD] += u8_ends_cut(text, ds, de);
            }
        }
        if (!pass && n > out_capacity) {
            counts[U8_C_BYTES] = n;
            return U8_HOST_CAPACITY;
        }
        c[U8_C_BYTES] = n;
    }
    if (out_doc_offsets) out_doc_offsets[n_docs] = c[U8_C_BYTES];
    memcpy(counts, c, sizeof c);
    return U8_HOST_OK;
}

// ---- the kernels' arguments ----------------------------------------------------------------------------------------------------------------
struct U8Args : RewriteArgs {  // (flags: 0 where the document is well-formed)
    int policy;                // U8_REPLACE or U8_IGNORE
    unsigned long long* first_bad;  // [n_docs] or null: int64, -1 (all ones) where the document is well-formed, kept by an unsigned minimum
    unsigned long long* n_bad;      // [n_docs] or null
    uint8_t* dirty;            // [windows] or null (the check): 1 where a unit near a document's edge makes a window's bytes ill-formed
};

// The windows of a text whose base lies `shift` bytes behind a 16-byte aligned address: window g is text[16 g - shift, 16 g - shift + 16).
__host__ __device__ inline int64_t u8_window_of(int64_t p, int shift) { return (p + shift) >> 4; }
__host__ __device__ inline int64_t u8_windows(int64_t total, int shift) { return (total + shift + 15) >> 4; }

// A document's edges, by the lane that has the document [ds, de): the units that start within three bytes of its start or its end are the
// ones the document's rule may see differently from the text's.  report(p, len): the ill-formed unit text[p, p + len).
// The document's rule and the text's differ only where the text's rule reaches over the boundary: a continuation byte at ds (the bytes
// behind it may be consumed by a lead in front of the document) or at de < total (a sequence of the document's last bytes may end behind
// it).  Every other document is left after those two bytes: what is ill-formed in it is ill-formed in the text and shows in the screen.
template <class Report>
__host__ __device__ inline void u8_doc_edges(const uint8_t* text, int64_t ds, int64_t de, int64_t total, Report report) {
    if (ds >= de || !(u8_is_cont(text[ds]) || (de < total && u8_is_cont(text[de])))) return;
    for (int64_t p = ds; p < de; ++p) {
        if (p >= ds + 3 && p < de - 3) { p = de - 4; continue; }
        if (u8_unit_start(text, p, ds, de) != p) continue;
        bool wf;
        const int len = u8_unit(text, p, de, wf);
        if (!wf) report(p, len);
    }
}

// ---- a lane of the repair ------------------------------------------------------------------------------------------------------------------
struct U8LaneStats {
    uint32_t subparts, sub_bytes;
};

// The BYTES of the window [b, we) of the text (b < we <= total): a byte of a well-formed unit is one byte of output, the first byte of
// an ill-formed subpart is EF BF BD or nothing, its other bytes are nothing.  So a window without a byte of a subpart is a copy.
// ub(x): the first document of the tile's table that starts behind x, as an index of doc_off.  MEASURE: flags, first_bad, n_bad and
// st, by the lane that has the subpart's first byte.  WRITE: the bytes from out + opos on and the output offsets of the documents that
// start in the window.  add(ptr, n), lower(ptr, v): an atomic sum and an atomic unsigned minimum.  Returns the bytes the window makes.
template <int MODE, class Ub, class Add, class Lower>
__host__ __device__ inline int64_t u8_lane(const U8Args& a, int64_t b, int64_t we, Ub ub, int64_t opos, U8LaneStats& st, Add add, Lower lower) {
    const uint8_t* text = a.text;
    int64_t D = ub(b) - 1, ds = a.doc_off[D], de = a.doc_off[D + 1];
    int64_t kd = 0, next_start = INT64_MAX;
    if (MODE == U8_WRITE) {
        kd = ub(b - 1);
        next_start = kd <= a.n_docs ? a.doc_off[kd] : INT64_MAX;
    }
    int64_t n = 0, unit_end = b;
    bool unit_wf = true;
    for (int64_t p = b; p < we; ++p) {
        while (p >= de) {  // (p < total: a document that holds it follows; empty ones are stepped over)
            ++D;
            ds = de;
            de = a.doc_off[D + 1];
        }
        if (MODE == U8_WRITE) {
            while (next_start == p) {
                a.out_doc_off[kd] = opos + n;
                ++kd;
                next_start = kd <= a.n_docs ? a.doc_off[kd] : INT64_MAX;
            }
        }
        if (p >= unit_end) {  // (behind a unit a unit starts; the window's first byte may lie inside one)
            const int64_t q = p == b ? u8_unit_start(text, p, ds, de) : p;
            const int len = u8_unit(text, q, de, unit_wf);
            unit_end = q + len;
            if (!unit_wf && q == p) {
                if (MODE == U8_MEASURE) {
                    a.flags[D] = 1;
                    if (a.first_bad) lower(a.first_bad + D, (unsigned long long)(p - ds));
                    if (a.n_bad) add(a.n_bad + D, 1ull);
                    st.subparts += 1;
                    st.sub_bytes += (uint32_t)len;
                }
                if (a.policy == U8_REPLACE) {
                    if (MODE == U8_WRITE) {
                        a.out[opos + n] = 0xEF;
                        a.out[opos + n + 1] = 0xBF;
                        a.out[opos + n + 2] = 0xBD;
                    }
                    n += 3;
                }
            }
        }
        if (unit_wf) {
            if (MODE == U8_WRITE) a.out[opos + n] = text[p];
            n += 1;
        }
    }
    return n;
}

// The units that start in the window [b, we) for the check: D, ds, de are the lane's document (D < 0: none yet), doc_of(p) the last
// document that starts at or below p.
template <class DocOf, class Lower>
__host__ __device__ inline void u8_check_window(const U8Args& a, int64_t b, int64_t we, int64_t& D, int64_t& ds, int64_t& de, DocOf doc_of, Lower lower) {
    for (int64_t p = b; p < we; ++p) {
        if (a.text[p] < 0x80) continue;
        if (D < 0 || p < ds || p >= de) {  // (p is below doc_off[n_docs]: the last document that starts at or below p holds it)
            D = doc_of(p);
            ds = a.doc_off[D];
            de = a.doc_off[D + 1];
        }
        if (u8_unit_start(a.text, p, ds, de) != p) continue;
        bool wf;
        u8_unit(a.text, p, de, wf);
        if (wf) continue;
        a.flags[D] = 1;
        if (a.first_bad) lower(a.first_bad + D, (unsigned long long)(p - ds));
    }
}

}  // namespace td
