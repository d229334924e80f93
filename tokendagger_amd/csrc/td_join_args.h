// The truncation rule of a field join (include/tokendagger_hip.h, td_join_spec), once: td_join_plan on the host and td_join_count /
// td_join_first on the device run this text.  No loop here depends on a length: TD_JOIN_SHRINK_LONGEST is in closed form.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TD_JOIN_HD __host__ __device__ __forceinline__
#else
#define TD_JOIN_HD inline
#endif

namespace td {

constexpr int JOIN_MAX_FIELDS = 8, JOIN_MAX_LITERAL = 16;
constexpr int JOIN_MAX_PARTS = 2 * JOIN_MAX_FIELDS + 1;  // before_0 body_0 ... before_{K-1} body_{K-1} tail

enum { JOIN_DROPPED = 0, JOIN_KEPT = 1, JOIN_TRUNCATED = 2 };

// What the rule needs of a td_join_spec (the host fills it from a checked spec: join_rule_of).
struct JoinRule {
    int32_t K;                         // fields, 1 .. 8
    int32_t longest;                   // TD_JOIN_SHRINK_LONGEST
    int32_t field_major;               // field f of example x is document f * n_ex + x, not x * K + f
    int32_t n_tail;
    int64_t max_total;                 // -1: no limit
    int64_t fixed;                     // sum n_before + n_tail
    int64_t max_len[JOIN_MAX_FIELDS];  // -1: no cap
    int32_t n_before[JOIN_MAX_FIELDS];
    int32_t order_pos[JOIN_MAX_FIELDS];  // the field's place among the shrinkable ones by (rank, index); -1: shrink_rank = 0
    uint32_t keep_tail;                // bit f: TD_JOIN_KEEP_TAIL
};

// L[f] -> the kept c[f] (f < K; the rest is left alone) and JOIN_DROPPED / JOIN_KEPT / JOIN_TRUNCATED.  Every loop has constant
// bounds and every array a constant index once unrolled: on the device L and c stay in registers.
TD_JOIN_HD int join_keep(const JoinRule& r, const int64_t (&L)[JOIN_MAX_FIELDS], int64_t (&c)[JOIN_MAX_FIELDS]) {
    int64_t need = r.fixed;
    bool cut_any = false;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f) {
        if (f >= r.K) continue;
        c[f] = r.max_len[f] >= 0 && L[f] > r.max_len[f] ? r.max_len[f] : L[f];
        cut_any |= c[f] < L[f];
        need += c[f];
    }
    if (r.max_total < 0 || need <= r.max_total) return cut_any ? JOIN_TRUNCATED : JOIN_KEPT;
    int64_t over = need - r.max_total;
    if (!r.longest) {
#pragma unroll
        for (int i = 0; i < JOIN_MAX_FIELDS; ++i) {
#pragma unroll
            for (int f = 0; f < JOIN_MAX_FIELDS; ++f) {
                if (f >= r.K || r.order_pos[f] != i) continue;
                const int64_t cut = c[f] < over ? c[f] : over;
                c[f] -= cut;
                over -= cut;
            }
        }
        return over > 0 ? JOIN_DROPPED : JOIN_TRUNCATED;
    }
    // One id at a time from the longest, ties to the highest index, ends with every shrinkable field above a level l cut to l
    // and the lowest-indexed of them one id longer.  B ids stay in the shrinkable fields; g(v) = sum min(c_f, v) is piecewise
    // linear with its bends at the c_f: p, the largest bend (or 0) with g(p) <= B, then l = p + (B - g(p)) / #{c_f > p}.
    int64_t S = 0;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f)
        if (f < r.K && r.order_pos[f] >= 0) S += c[f];
    if (over > S) return JOIN_DROPPED;
    const int64_t B = S - over;
    int64_t p = 0, gp = 0;
#pragma unroll
    for (int i = 0; i < JOIN_MAX_FIELDS; ++i) {
        if (i >= r.K || r.order_pos[i] < 0) continue;
        const int64_t v = c[i];
        int64_t g = 0;
#pragma unroll
        for (int f = 0; f < JOIN_MAX_FIELDS; ++f)
            if (f < r.K && r.order_pos[f] >= 0) g += c[f] < v ? c[f] : v;
        if (g <= B && v > p) { p = v; gp = g; }
    }
    int64_t above = 0;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f)
        if (f < r.K && r.order_pos[f] >= 0 && c[f] > p) ++above;
    if (above == 0) return JOIN_TRUNCATED;  // (B >= S: not reached with over > 0)
    const int64_t level = p + (B - gp) / above;
    int64_t extra = (B - gp) % above;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f) {
        if (f >= r.K || r.order_pos[f] < 0 || c[f] <= p) continue;
        c[f] = level + (extra > 0 ? 1 : 0);
        extra -= extra > 0 ? 1 : 0;
    }
    return JOIN_TRUNCATED;
}

// The document of field f of example x.
TD_JOIN_HD int64_t join_doc(const JoinRule& r, int64_t n_ex, int64_t x, int f) { return r.field_major ? (int64_t)f * n_ex + x : x * r.K + f; }

}  // namespace td
