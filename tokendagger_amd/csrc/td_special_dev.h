// Allowed special tokens on the device (td_special.hip): what the kernels and the CPU model (tests/twin/special_model.cpp) share: the
// table a call searches, the candidate test of a 32-byte word, the match of one position against the sorted literals, the document
// limit of a match, and the greedy walk through a cluster of hits.  Everything here is a function of its arguments alone: the kernels
// add the loads, the lists and the atomics around it.  The table itself is built by td_special_table.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

// The allowed special literals of a call, sorted bytewise (td_special.hip), and the two bitmaps of the cut search.
struct SpecialTable {
    const uint8_t* bytes;     // the literals, each dword-aligned and zero-padded to a multiple of 4 bytes
    const uint32_t* off;      // [n] byte offset of literal i (a multiple of 4)
    const uint32_t* len;      // [n] its length in bytes
    const int32_t* id;        // [n]
    const int32_t* parent;    // [n] the longest other literal that is a proper prefix of literal i, or -1
    const uint32_t* first2;   // [2048] bit (b0 << 8 | b1): a literal starts with these two bytes
    int64_t* cand_pos;        // [cand_cap] positions whose first two bytes start an allowed literal
    int32_t* cand_lit;        // [cand_cap] the literal matched there, or -1
    uint32_t* cand_count;
    uint32_t cand_cap;
    uint32_t* hitbits;        // [(n_text+31)/32] an allowed literal matches at this byte
    uint32_t* accbits;        // ... and is cut out (not inside a literal cut out in front of it)
    uint32_t n, maxlen;       // literals; bytes of the longest one.  n == 0: no cuts in this call
};

constexpr uint32_t SP_QWORDS = 12;              // dwords of text a match takes into registers
constexpr uint32_t SP_MAXLEN = 4 * SP_QWORDS;   // bytes of the longest literal the device search takes
constexpr uint32_t SP_FIRST2_WORDS = 2048;      // words of SpecialTable::first2: a bit per pair of bytes

// the lowest set bit of m != 0
__host__ __device__ __forceinline__ int sp_low_bit(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs(m) - 1;
#else
    return __builtin_ctz(m);
#endif
}

// first document start in (p, p + span], or p + span; never behind n
__host__ __device__ __forceinline__ int64_t sp_doc_limit(const uint32_t* docbits, int64_t n, int64_t p, int64_t span) {
    int64_t lim = p + span < n ? p + span : n;
    for (int64_t q = p + 1; q < lim;) {
        uint32_t m = docbits[q >> 5] >> (q & 31);
        if (m) { const int64_t f = q + sp_low_bit(m); return f < lim ? f : lim; }
        q = ((q >> 5) + 1) << 5;
    }
    return lim;
}

// index of the longest allowed literal that is a prefix of text[p, lim), or -1.  The text at p is taken into registers once
// (12 dwords: literals are at most SP_MAXLEN bytes), the literals are stored dword-aligned and zero-padded, and a comparison
// goes a dword at a time in byte order (a byte-by-byte walk through the 40-byte common prefix of a thousand reserved tokens
// was ~440 dependent loads per match).
__host__ __device__ __forceinline__ int sp_match(const SpecialTable& S, const uint8_t* text, int64_t p, int64_t lim) {
    const int64_t avail64 = lim - p;
    const uint32_t avail = avail64 > (int64_t)(4 * SP_QWORDS) ? 4 * SP_QWORDS : (uint32_t)avail64;
    uint32_t Q[SP_QWORDS];
#pragma unroll
    for (uint32_t k = 0; k < SP_QWORDS; ++k) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (4 * k + j < avail) w |= (uint32_t)text[p + 4 * k + j] << (24 - 8 * j);  // (byte order: a dword compare is a memcmp)
        Q[k] = w;
    }
    // literal i <= Q ?  (prefix: the literal is a prefix of Q)
    auto le = [&](int i, bool& prefix) {
        const uint32_t o = S.off[i], len = S.len[i];
        const uint32_t* lw = reinterpret_cast<const uint32_t*>(S.bytes + o);
        prefix = false;
        bool decided = false, res = false;
#pragma unroll
        for (uint32_t k = 0; k < SP_QWORDS; ++k) {
            if (!decided && 4 * k < len) {
                const uint32_t nb = len - 4 * k < 4u ? len - 4 * k : 4u;           // literal bytes in this dword
                const uint32_t mask = nb == 4u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (8 * nb));
                const uint32_t x = __builtin_bswap32(lw[k]) & mask, y = Q[k] & mask;
                if (x != y) { decided = true; res = x < y; }
                else if (4 * k + nb > avail) { decided = true; res = false; }      // Q ends inside the literal (its bytes read as 0): the literal is greater
            }
        }
        if (!decided) { prefix = len <= avail; return prefix; }
        // equal bytes up to a difference: when the difference lies behind the end of Q the literal is the greater one
        return res;
    };
    int lo = -1, hi = (int)S.n;  // literal[lo] <= Q < literal[hi]
    bool pre = false, lo_pre = false;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (le(mid, pre)) { lo = mid; lo_pre = pre; } else hi = mid;
    }
    int i = lo;
    while (i >= 0 && !lo_pre) {  // up the chain of prefixes: everything in [longest prefix literal, Q] starts with it
        i = S.parent[i];
        if (i >= 0) (void)le(i, lo_pre);
    }
    return i;
}

// a lane's 32 bytes at p0 as eight little-endian words and the byte behind them as the ninth, byte by byte (bytes at and behind n
// read as 0): the last words of a text and every word of a text that does not start on a 16-byte boundary
__host__ __device__ __forceinline__ void sp_words_bytewise(const uint8_t* text, int64_t n, int64_t p0, uint32_t (&tw)[9]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t x = 0;
        for (int j = 0; j < 4; ++j)
            if (p0 + 4 * k + j < n) x |= (uint32_t)text[p0 + 4 * k + j] << (8 * j);
        tw[k] = x;
    }
    tw[8] = p0 + 32 < n ? (uint32_t)text[p0 + 32] : 0u;
}

// bit k: position p0 + k < n starts with two bytes some allowed literal starts with (first2: 1-byte literals have all b1 set)
__host__ __device__ __forceinline__ uint32_t sp_word_candidates(const uint32_t (&tw)[9], const uint32_t* first2, int64_t p0, int64_t n) {
    uint32_t cand = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const uint32_t b0 = (tw[k >> 2] >> (8 * (k & 3))) & 0xFFu, b1 = (tw[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
        const uint32_t key = (b0 << 8) | b1;
        if (p0 + k < n && ((first2[key >> 5] >> (key & 31)) & 1u)) cand |= 1u << k;
    }
    return cand;
}

// first hit in [q, lim), or lim
__host__ __device__ __forceinline__ int64_t sp_next_hit(const uint32_t* hitbits, int64_t q, int64_t lim) {
    while (q < lim) {
        const uint32_t m = hitbits[q >> 5] >> (q & 31);
        if (m) { const int64_t f = q + sp_low_bit(m); return f < lim ? f : lim; }
        q = ((q >> 5) + 1) << 5;
    }
    return lim;
}

// Hits further apart than a literal is long cannot touch, so a hit without another one in the maxlen - 1 bytes in front of it is
// accepted for sure: it is the head of its cluster
__host__ __device__ __forceinline__ bool sp_is_head(const SpecialTable& S, int64_t p) {
    const int64_t back = (int64_t)S.maxlen - 1;  // a literal that starts further back ends in front of the hit
    const int64_t lo = p - back > 0 ? p - back : 0;
    return !(sp_next_hit(S.hitbits, lo, p) < p);
}

// greedy left-to-right from the head p of a cluster, i its literal: accept(cur) for every hit that is cut out, rematch(cur) -> the
// literal of a later hit of the cluster.  A hit inside an accepted literal is dropped.
template <class Accept, class Rematch>
__host__ __device__ __forceinline__ void sp_cluster_walk(const SpecialTable& S, int64_t n, int64_t p, int i, Accept accept, Rematch rematch) {
    const int64_t back = (int64_t)S.maxlen - 1;
    int64_t cur = p;
    for (;;) {  // cur is accepted, i its literal
        accept(cur);
        const int64_t end = cur + (int64_t)S.len[i];
        // hits inside the literal are dropped; the next one at or behind its end is accepted if it belongs to this cluster
        int64_t last = cur, q = cur + 1;
        bool more = false;
        for (;;) {
            const int64_t lim = last + back + 1 < n ? last + back + 1 : n;
            const int64_t f = sp_next_hit(S.hitbits, q, lim);
            if (f >= lim) break;  // the cluster ends: the next hit is a head of its own
            last = f;
            if (f >= end) { cur = f; more = true; break; }
            q = f + 1;
        }
        if (!more) break;
        i = rematch(cur);
    }
}

}  // namespace td
