// Address masking (td_mask.hip): the rule, stated once.  The host statement (ma_host, which td_mask_addresses_host is) and the kernels
// compile what is here: the byte classes, the decision on an '@', the decision on a digit that may begin an IPv4 address, the hash that
// picks the placeholder.  Compiles on the host without HIP's runtime (tools/sanitize/mask_asan.cpp).
//
// A decision reads the document [ds, de) only, and from its anchor at most 65 bytes back and 255 forward ('@'), 1 back and 17 forward
// (a digit).  Matches never overlap, so every anchor is decided on its own, by whoever needs it.
#pragma once
#include <string.h>

#include "../../include/tokendagger_hip.h"
#include "td_rewrite_args.h"

namespace td {

constexpr int MA_COLS = TD_MA_COLS;
enum { MA_EMAILS = 0, MA_IPS, MA_IPS_KEPT, MA_BYTES_OUT_OF, MA_BYTES_IN, MA_OUT_BYTES };
enum { MA_NONE = 0, MA_EMAIL = 1, MA_IP = 2, MA_IP_KEPT = 3 };  // what a decision returns
enum { MA_HOST_OK = 0, MA_HOST_INVALID = 1, MA_HOST_CAPACITY = 2 };
constexpr int MA_LOCAL_MAX = 64, MA_RUN_MAX = 254, MA_MATCH_MAX = 254, MA_MATCH_MIN = 6;  // "a@b.cd"; an IPv4 has 7 at the least

__host__ __device__ inline bool ma_digit(uint32_t c) { return c >= '0' && c <= '9'; }
__host__ __device__ inline bool ma_alpha(uint32_t c) { return (c | 0x20u) >= 'a' && (c | 0x20u) <= 'z'; }
__host__ __device__ inline bool ma_D(uint32_t c) { return ma_digit(c) || ma_alpha(c) || c == '.' || c == '-'; }
__host__ __device__ inline bool ma_L(uint32_t c) { return ma_D(c) || c == '_' || c == '%' || c == '+'; }

inline bool ma_rules_ok(const td_mask_rules* r) {
    if (!r || (r->flags & ~(TD_MA_EMAILS | TD_MA_IPS | TD_MA_KEEP_PRIVATE_IPS)) || r->n_emails < 0 || r->n_emails > TD_MA_MAX_LITERALS ||
        r->n_ips < 0 || r->n_ips > TD_MA_MAX_LITERALS || ((r->flags & TD_MA_EMAILS) && r->n_emails < 1) || ((r->flags & TD_MA_IPS) && r->n_ips < 1))
        return false;
    for (int j = 0; j < r->n_emails; ++j)
        if (r->emails[j].len > TD_MA_LITERAL_BYTES) return false;
    for (int j = 0; j < r->n_ips; ++j)
        if (r->ips[j].len > TD_MA_LITERAL_BYTES) return false;
    return true;
}

// the '@' at a of the document [ds, de): the match [ms, me) it is the middle of, or false
__host__ __device__ inline bool ma_email(const uint8_t* text, int64_t ds, int64_t de, int64_t a, int64_t& ms, int64_t& me) {
    int64_t ls = a;
    while (ls > ds && a - ls <= MA_LOCAL_MAX && ma_L(text[ls - 1])) --ls;  // (stops at 65: too long)
    const int64_t nl = a - ls;
    if (nl < 1 || nl > MA_LOCAL_MAX || text[ls] == '.' || text[a - 1] == '.' || (ls > ds && text[ls - 1] == '@')) return false;
    int64_t re = a + 1;
    while (re < de && re - (a + 1) <= MA_RUN_MAX && ma_D(text[re])) ++re;  // (stops at 255)
    const int64_t nr = re - (a + 1);
    if (nr < 1 || nr > MA_RUN_MAX || (re < de && text[re] == '@')) return false;
    const int64_t dend = text[re - 1] == '.' ? re - 1 : re;
    if (dend - ls > MA_MATCH_MAX) return false;
    int labels = 0;
    int64_t s = a + 1, last = s;
    for (int64_t p = s; p <= dend; ++p) {
        if (p < dend && text[p] != '.') continue;
        if (p - s < 1 || p - s > 63 || text[s] == '-' || text[p - 1] == '-') return false;
        ++labels;
        last = s;
        s = p + 1;
    }
    if (labels < 2 || dend - last < 2 || dend - last > 24) return false;
    for (int64_t p = last; p < dend; ++p)
        if (!ma_alpha(text[p])) return false;
    ms = ls;
    me = dend;
    return true;
}

// the digit at p of the document [ds, de): MA_IP or MA_IP_KEPT with the match [p, q), or MA_NONE
__host__ __device__ inline int ma_ipv4(const uint8_t* text, int64_t ds, int64_t de, int64_t p, int flags, int64_t& q) {
    if (p > ds && ma_L(text[p - 1])) return MA_NONE;
    int64_t x = p;
    uint32_t o0 = 0, o1 = 0;
    for (int i = 0; i < 4; ++i) {
        if (x >= de || !ma_digit(text[x])) return MA_NONE;
        const uint32_t first = text[x];
        uint32_t v = 0;
        int n = 0;
        for (; x < de && n < 4 && ma_digit(text[x]); ++x, ++n) v = v * 10 + (text[x] - '0');
        if (n > 3 || v > 255 || (n > 1 && first == '0')) return MA_NONE;
        if (i == 0) o0 = v;
        if (i == 1) o1 = v;
        if (i == 3) break;
        if (x >= de || text[x] != '.') return MA_NONE;
        ++x;
    }
    if (x < de) {
        uint32_t c = text[x];
        if (c == '.') c = x + 1 < de ? text[x + 1] : ' ';  // the dot is in L: only the byte behind it can let the match stand
        if (ma_L(c) || c == '@') return MA_NONE;
    }
    q = x;
    const bool priv = o0 == 0 || o0 == 10 || o0 == 127 || (o0 == 169 && o1 == 254) || (o0 == 172 && (o1 & 0xF0u) == 16) ||
                      (o0 == 192 && o1 == 168) || o0 >= 224;
    return priv && (flags & TD_MA_KEEP_PRIVATE_IPS) ? MA_IP_KEPT : MA_IP;
}

// the literal of n that replaces text[ms, me): FNV-1a-32 of the matched bytes (not walked where there is one literal)
__host__ __device__ inline int ma_pick(const uint8_t* text, int64_t ms, int64_t me, int n) {
    if (n < 2) return 0;
    uint32_t h = 2166136261u;
    for (int64_t p = ms; p < me; ++p) h = (h ^ text[p]) * 16777619u;
    return (int)(h % (uint32_t)n);
}

// The contract's executable statement: a document, an anchor at a time, in the anchors' order, which is the matches'.  out,
// out_doc_offsets and totals may be null; with out null nothing is held against out_capacity.  Argument errors and an output that does
// not fit write nothing but *need (may be null).
inline int ma_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_mask_rules* rules, uint8_t* out,
                   int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals, int64_t* need) {
    if (n_docs < 0 || !doc_offsets || out_capacity < 0 || !ma_rules_ok(rules) || !rewrite_offsets_ok(doc_offsets, n_docs) ||
        (n_docs > 0 && !stats) || (doc_offsets[n_docs] > 0 && !text) || rewrite_overlap(text, doc_offsets[n_docs], out, out_capacity))
        return MA_HOST_INVALID;
    for (int pass = 0; pass < 2; ++pass) {  // 0: the size; 1: the results
        int64_t opos = 0;
        for (int64_t d = 0; d < n_docs; ++d) {
            const int64_t ds = doc_offsets[d], de = doc_offsets[d + 1];
            int64_t row[MA_COLS] = {0, 0, 0, 0, 0, 0}, done = ds;  // done: the text in front of it is out
            const int64_t o0 = opos;
            if (pass && out_doc_offsets) out_doc_offsets[d] = opos;
            for (int64_t p = ds; p <= de; ++p) {
                int64_t ms = p, me = de;
                int kind = MA_NONE;
                if (p == de) ms = de;  // the rest of the document
                else if (text[p] == '@' && (rules->flags & TD_MA_EMAILS)) kind = ma_email(text, ds, de, p, ms, me) ? MA_EMAIL : MA_NONE;
                else if (ma_digit(text[p]) && (rules->flags & TD_MA_IPS)) kind = ma_ipv4(text, ds, de, p, rules->flags, me);
                if (kind == MA_IP_KEPT) ++row[MA_IPS_KEPT];
                if (p < de && kind != MA_EMAIL && kind != MA_IP) continue;
                if (pass && out) memcpy(out + opos, text + done, (size_t)(ms - done));
                opos += ms - done;
                done = ms;
                if (p == de) break;
                const td_mask_literal& lit = kind == MA_EMAIL ? rules->emails[ma_pick(text, ms, me, rules->n_emails)]
                                                              : rules->ips[ma_pick(text, ms, me, rules->n_ips)];
                if (pass && out) memcpy(out + opos, lit.bytes, lit.len);
                opos += lit.len;
                done = me;
                ++row[kind == MA_EMAIL ? MA_EMAILS : MA_IPS];
                row[MA_BYTES_OUT_OF] += me - ms;
                row[MA_BYTES_IN] += lit.len;
            }
            row[MA_OUT_BYTES] = opos - o0;
            if (pass) {
                for (int c = 0; c < MA_COLS; ++c) {
                    stats[d * MA_COLS + c] = row[c];
                    if (totals) totals[c] += row[c];
                }
            }
        }
        if (!pass) {
            if (need) *need = opos;
            if (out && opos > out_capacity) return MA_HOST_CAPACITY;
            if (totals) memset(totals, 0, sizeof(int64_t) * MA_COLS);
        } else if (out_doc_offsets) {
            out_doc_offsets[n_docs] = opos;
        }
    }
    return MA_HOST_OK;
}

// ---- the kernels' arguments ---------------------------------------------------------------------------------------------------------------
struct MaArgs : RewriteArgs {  // (flags: not used; counts[0]: the output's bytes, the rest 0)
    td_mask_rules rules;
    unsigned long long* stats;   // [n_docs][MA_COLS]
    unsigned long long* totals;  // [MA_COLS], may be null
    uint32_t* dirty;             // [tiles]: MEASURE found a match or a kept address in or astride the tile; WRITE copies any other tile
};

}  // namespace td
