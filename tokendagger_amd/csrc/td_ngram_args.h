// N-gram matches (td_ngrams.hip): what the kernel, the host library (td_api_ngram.cpp) and the CPU model (tests/twin/ngram_model.cpp)
// share: the kernel's arguments, its constants, the window hash, the table's slot layout and its probe rule.  The rule is the contract in
// include/tokendagger_hip.h.
//
// The hash only FINDS a candidate: ng_probe reports a pattern after its ids were compared with the window's and found equal, so the
// result is a function of the inputs alone, whatever the hash, the table size and tag_mask are.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace td {

constexpr int NG_THREADS = 256;      // lanes of a workgroup (td_rows_common.h's RC_THREADS)
constexpr int NG_TILE = 4096;        // start positions (and output slots) of a workgroup's tile, sixteen a lane (RC_TILE)
constexpr int NG_PER = 16;
constexpr int NG_MAX_LEN = 64;       // TD_NGRAM_MAX_LEN
constexpr int NG_MAX_LENGTHS = 8;    // TD_NGRAM_MAX_LENGTHS
constexpr int NG_HALO = NG_MAX_LEN - 1;  // ids a window reaches behind its tile, and starts in front of a tile that reach into it
constexpr int NG_FRONT = NG_MAX_LEN;     // ids kept in front of the tile in LDS (NG_HALO, rounded to an int4)
constexpr int NG_SPAN = NG_FRONT + NG_TILE;            // starts a tile looks at: the halo's and its own
constexpr int NG_LDS_IDS = NG_FRONT + NG_TILE + NG_MAX_LEN;  // ids a tile holds: [t0 - 64, t0 + 4096 + 64); the last is read by no window
constexpr int64_t NG_MAX_PATS = 1ll << 24;
constexpr int64_t NG_MAX_IDS = 1ll << 28;
static_assert(NG_TILE == NG_PER * NG_THREADS && NG_FRONT % NG_PER == 0 && NG_FRONT >= NG_HALO, "sixteen starts a lane, whole runs in the halo");

// ---- the window hash: a polynomial in NG_BASE modulo 2^32 over the window's ids, first id at the highest power ---------------------
constexpr uint32_t NG_BASE = 0x9E3779B1u;

// ids[0 .. k) through get(j)
template <class Get>
__host__ __device__ inline uint32_t ng_hash_full(Get get, int k) {
    uint32_t h = 0;
    for (int j = 0; j < k; ++j) h = h * NG_BASE + (uint32_t)get(j);
    return h;
}

// NG_BASE^k: what the id that leaves a window of k ids was multiplied with, times NG_BASE
__host__ __device__ inline uint32_t ng_base_pow(int k) {
    uint32_t p = 1;
    for (int j = 0; j < k; ++j) p *= NG_BASE;
    return p;
}

// the hash of the window one position further: `out` leaves in front, `in` enters behind; base_k = ng_base_pow(k)
__host__ __device__ inline uint32_t ng_hash_roll(uint32_t h, int32_t out, int32_t in, uint32_t base_k) {
    return h * NG_BASE - (uint32_t)out * base_k + (uint32_t)in;
}

// The finished hash of a window of k ids (keyed with the length: the table holds every length), a bijection of h for every k:
// its low bits choose the slot, all of it is the slot's tag.
__host__ __device__ inline uint32_t ng_finish(uint32_t h, int k) {
    uint32_t x = h + (uint32_t)k * 0x7FEB352Du;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// ---- the table: open addressing, linear probing, 2^slot_bits slots, at least twice the distinct patterns --------------------------
struct NgSlot {
    uint32_t tag;   // ng_finish of the pattern
    uint32_t pat1;  // the distinct pattern's index + 1; 0: nobody sits here
};
static_assert(sizeof(NgSlot) == 8, "a slot is one 8-byte load");

// the tag bits a lookup compares before it compares ids: the top `bits` of the tag, all 32 with bits = 0 (the low ones chose the slot)
__host__ __device__ inline uint32_t ng_tag_mask(int bits) { return bits <= 0 || bits >= 32 ? 0xFFFFFFFFu : ~0u << (32 - bits); }

// What every lookup reads.  Immutable once built; a set's copy lives on its device.
struct NgTable {
    const NgSlot* slots;      // [slot_mask + 1]
    const int32_t* pat_ids;   // the distinct patterns' ids, flat
    const uint32_t* pat_off;  // [n_distinct + 1] into pat_ids
    const uint32_t* pat_orig; // [n_distinct]: the lowest index of the sequence in the caller's list
    uint32_t slot_mask;
    uint32_t max_probe;       // the longest distance between a pattern's first slot and its own, at build time: no lookup walks further
    int32_t n_lengths;
    uint64_t lengths8;        // the distinct lengths, ascending, a byte each (a kernel argument indexed by a register would live in scratch)
    __host__ __device__ int length(int l) const { return (int)((lengths8 >> (8 * l)) & 0xFFu); }
};

// One slot of a lookup's walk: the window win(0 .. k) with the finished hash x meets slot s.  NG_STOP: the slot is empty, the window is
// no pattern; NG_NEXT: somebody else sits here, the walk goes on; else the distinct pattern equal to the window (its ids were compared).
// failed (may be null): tag matches whose ids differed, for the model.
enum { NG_STOP = -1, NG_NEXT = -2 };
template <class Win>
__host__ __device__ inline int32_t ng_slot_step(const NgTable& T, NgSlot s, uint32_t x, int k, uint32_t tag_mask, Win win, long long* failed = nullptr) {
    if (s.pat1 == 0) return NG_STOP;
    if ((s.tag ^ x) & tag_mask) return NG_NEXT;
    const uint32_t lo = T.pat_off[s.pat1 - 1], hi = T.pat_off[s.pat1];
    bool same = hi - lo == (uint32_t)k;
    for (int j = 0; same && j < k; ++j) same = T.pat_ids[lo + j] == win(j);
    if (same) return (int32_t)(s.pat1 - 1);
    if (failed) ++*failed;
    return NG_NEXT;
}

// The probe rule: slots x, x + 1, ... (masked) until ng_slot_step says NG_STOP or finds the pattern, at most max_probe + 1 of them:
// the loop ends there whatever the data is.  The kernel walks sixteen windows a lane side by side by the same rule (td_ngrams.hip).
template <class Win>
__host__ __device__ inline int32_t ng_probe(const NgTable& T, uint32_t x, int k, uint32_t tag_mask, Win win, long long* failed = nullptr) {
    for (uint32_t d = 0; d <= T.max_probe; ++d) {
        const int32_t r = ng_slot_step(T, T.slots[(x + d) & T.slot_mask], x, k, tag_mask, win, failed);
        if (r != NG_NEXT) return r;
    }
    return -1;
}

// ---- the kernel's arguments ------------------------------------------------------------------------------------------------------------
enum { NG_H_BAD = 0, NG_H_WORDS = 2 };  // NgramArgs::head: 2^62 - the lowest document with bad offsets (0: none), kept by an atomic maximum

struct NgramArgs {
    const int32_t* ids;        // [n_tokens]
    int64_t n_tokens;
    const int64_t* tok_off;    // [n_docs + 1]
    int64_t n_docs;
    NgTable tab;
    uint32_t tag_mask;
    int32_t ignore;
    uint8_t* cover;                    // [total] or null
    int32_t* labels;                   // [total] or null, in place
    unsigned long long* doc_stats;     // [n_docs][2]: the caller's, or the handle's own when the caller has none
    unsigned long long* pat_counts;    // [n_pats] or null
    unsigned long long* counts;        // [4]
    unsigned long long* head;          // [NG_H_WORDS], zeroed before the launches; the outputs are zeroed by td_ng_clear
    int* err;
    long long* err_pos;
};

}  // namespace td
