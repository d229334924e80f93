// MinHash signatures and LSH band keys (td_minhash.hip): what the kernels, the host library (td_api_minhash.cpp) and the CPU model
// (tests/twin/minhash_model.cpp) share: the permutation family, the band fold, the kernels' arguments and the tile constants.  The rule
// is the contract in include/tokendagger_hip.h; the shingle hash is td_ngram_args.h's window hash, the project's only one.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_ngram_args.h"

namespace td {

constexpr int MH_THREADS = 256;          // lanes of a workgroup (RC_THREADS, NG_THREADS)
constexpr int MH_TILE = 4096;            // starts of a workgroup's tile, sixteen a lane in the hash phase (RC_TILE, NG_TILE)
constexpr int MH_PER = 16;
constexpr int MH_MAX_K = NG_MAX_LEN;     // the n-gram halo serves: a window reaches at most 63 ids behind its tile
constexpr int MH_LDS_IDS = MH_TILE + MH_MAX_K;  // ids a tile holds: [t0, t0 + 4096 + 64); a window belongs to the tile of its start
constexpr int MH_WAVE_STARTS = MH_TILE / (MH_THREADS / 64);  // the starts whose minima one wavefront takes: the ones its lanes hashed
constexpr int MH_CHUNK = 64;             // permutations a wavefront holds at a time, one a lane
constexpr int MH_MAX_PERM = 1024;
static_assert(MH_THREADS == NG_THREADS && MH_TILE == NG_TILE && MH_PER == NG_PER, "the n-gram tile's shape");
static_assert(MH_WAVE_STARTS == 64 * MH_PER, "a wavefront reads back the hashes its own lanes wrote");

// ---- the permutation family: multiply-add-shift over 64 bits, strongly universal for 32-bit keys --------------------------------------
constexpr uint64_t MH_GOLDEN = 0x9E3779B97F4A7C15ull;

// the splitmix64 finaliser
__host__ __device__ inline uint64_t mh_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

struct MhParam {  // one 16-byte load
    uint64_t a;   // odd
    uint64_t b;
};
static_assert(sizeof(MhParam) == 16, "a lane loads its permutation at once");

__host__ __device__ inline MhParam mh_param(uint64_t seed, int64_t j) {
    return MhParam{mh_mix64(seed + (2 * (uint64_t)j + 1) * MH_GOLDEN) | 1ull, mh_mix64(seed + (2 * (uint64_t)j + 2) * MH_GOLDEN)};
}

// h_j(x): the upper half of a * x + b modulo 2^64
__host__ __device__ inline uint32_t mh_hash(MhParam p, uint32_t x) { return (uint32_t)((p.a * (uint64_t)x + p.b) >> 32); }

// the finished hash of a shingle of len ids (len = k, or the length of a document shorter than k)
template <class Get>
__host__ __device__ inline uint32_t mh_shingle(Get get, int len) { return ng_finish(ng_hash_full(get, len), len); }

// key[d][b]: the fold of sig[d][b * rows .. (b + 1) * rows)
__host__ __device__ inline uint64_t mh_band_key(const uint32_t* sig_row, int64_t b, int64_t rows) {
    uint64_t h = mh_mix64((uint64_t)b + 1);
    for (int64_t j = b * rows; j < (b + 1) * rows; ++j) h = mh_mix64(h ^ (uint64_t)sig_row[j]);
    return h;
}

// the shingles of a document of L ids
__host__ __device__ inline int64_t mh_shingles(int64_t L, int k) { return L >= k ? L - k + 1 : L > 0 ? 1 : 0; }

// ---- the kernels' arguments ----------------------------------------------------------------------------------------------------------
// MhashArgs::head, zeroed before the launches: 2^62 - the lowest document with bad offsets (0: none), kept by an atomic maximum; the
// documents without an id and the ones of 1 .. k - 1 ids (td_mh_docs counts them, td_mh_clear hands them to counts)
enum { MH_H_BAD = 0, MH_H_EMPTY = 1, MH_H_SHORT = 2, MH_H_WORDS = 4 };

struct MhashArgs {
    const int32_t* ids;        // [n_tokens]
    int64_t n_tokens;
    const int64_t* tok_off;    // [n_docs + 1]
    int64_t n_docs;
    const MhParam* params;     // [num_perm], the handle's table for (seed, num_perm)
    int32_t k;
    int32_t num_perm;
    int32_t bands;             // 0: no keys
    int32_t rows;
    uint32_t* sig;                     // [n_docs][num_perm]
    unsigned long long* band_keys;     // [n_docs][bands] or null
    unsigned long long* counts;        // [4]
    unsigned long long* head;          // [MH_H_WORDS]
    int* err;
    long long* err_pos;
};

}  // namespace td
