// CPU model of td_minhash.hip's decomposition over tokendagger_amd/csrc/td_minhash_args.h (the family, the fold and the window hash
// are the kernel's own): tiles that hold the 64 ids behind them and nothing in front, every shingle attributed to the tile of its
// start, the window hash rolled over runs of sixteen starts whatever document they lie in (and held against the recomputed one), a
// wavefront's quarter of the tile, the documents' offsets relative to the tile and clamped as the kernel's table clamps them, ONE run
// of valid starts per (document, wavefront), chunks of 64 permutations, and a minimum merged into the document's row at the end of
// every (document, wavefront, chunk) run.  The tile size is an argument.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_minhash_args.h"

using namespace td;

// stats[6]: tiles, windows hashed in the hash phase, merges (one atomicMin wave-instruction each), the most documents a tile met,
// (document, wavefront) runs, shingles of documents shorter than k.
// Returns 0, 1 for bad arguments, 2 when a rolled hash differed from the recomputed one.
extern "C" int minhash_model(const int32_t* ids, const int64_t* tok_off, int64_t n_docs, int tile, int k, int num_perm, uint64_t seed, int bands,
                             int rows, uint32_t* sig, uint64_t* keys, int64_t* counts, int64_t* stats) {
    if (tile < 4 * MH_PER || tile % (4 * MH_PER) || k < 1 || k > MH_MAX_K || num_perm < 1 || num_perm > MH_MAX_PERM) return 1;
    if (bands < 0 || (bands > 0 && (rows < 1 || (int64_t)bands * rows > num_perm))) return 1;
    const int64_t total = tok_off[n_docs];
    const int32_t off_lo = -MH_MAX_K, off_hi = tile + MH_MAX_K + 1, wave_starts = tile / 4;
    std::vector<MhParam> par((size_t)num_perm);
    for (int j = 0; j < num_perm; ++j) par[(size_t)j] = mh_param(seed, j);
    memset(stats, 0, 6 * sizeof(int64_t));
    memset(counts, 0, 4 * sizeof(int64_t));
    for (int64_t i = 0; i < n_docs * num_perm; ++i) sig[i] = 0xFFFFFFFFu;
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t L = tok_off[d + 1] - tok_off[d];
        counts[1] += L == 0;
        counts[2] += L > 0 && L < k;
    }
    const uint32_t bk = ng_base_pow(k);
    std::vector<int32_t> lds((size_t)tile + MH_MAX_K);
    std::vector<uint32_t> x((size_t)tile);
    for (int64_t t0 = 0; t0 < total; t0 += tile) {
        ++stats[0];
        const int64_t s1 = std::min<int64_t>(t0 + tile, total);
        for (size_t j = 0; j < lds.size(); ++j) lds[j] = t0 + (int64_t)j < total ? ids[t0 + (int64_t)j] : -1;
        // hash: runs of sixteen starts
        uint32_t h = 0;
        for (int j = 0; j < tile; ++j) {
            if (j % MH_PER == 0) h = ng_hash_full([&](int i) { return lds[(size_t)(j + i)]; }, k);
            else h = ng_hash_roll(h, lds[(size_t)(j - 1)], lds[(size_t)(j - 1 + k)], bk);
            if (h != ng_hash_full([&](int i) { return lds[(size_t)(j + i)]; }, k)) return 2;
            x[(size_t)j] = ng_finish(h, k);
            ++stats[1];
        }
        // the tile's documents: k0 the last with tok_off <= t0, nk the ones that start below s1
        const int64_t k0 = (std::upper_bound(tok_off, tok_off + n_docs, t0) - tok_off) - 1;
        const int64_t nk = (std::upper_bound(tok_off, tok_off + n_docs, s1 - 1) - tok_off) - k0;
        stats[3] = std::max(stats[3], nk);
        const auto rel = [&](int64_t i) {
            const int64_t r = tok_off[k0 + i] - t0;
            return (int32_t)std::min<int64_t>(std::max<int64_t>(r, off_lo), off_hi);
        };
        for (int wv = 0; wv < 4; ++wv) {
            const int32_t r0 = wave_starts * wv, r1 = (int32_t)std::min<int64_t>(s1 - t0, r0 + wave_starts);
            if (r0 >= r1) continue;
            int64_t i0 = 0;  // the last document with rel <= r0
            while (i0 + 1 < nk && rel(i0 + 1) <= r0) ++i0;
            for (int j0 = 0; j0 < num_perm; j0 += MH_CHUNK) {
                for (int64_t i = i0; i < nk; ++i) {
                    const int32_t da = rel(i);
                    if (da >= r1) break;
                    const int32_t de = rel(i + 1), L = de - da;
                    if (L == 0) continue;
                    int32_t lo, hi;
                    uint32_t xs = 0;
                    if (L >= k) {
                        lo = std::max(da, r0);
                        hi = std::min(de - k + 1, r1);
                        if (lo >= hi) continue;
                    } else {
                        if (da < r0) continue;
                        xs = mh_shingle([&](int c) { return lds[(size_t)(da + c)]; }, L);
                        lo = da;
                        hi = da + 1;
                    }
                    if (j0 == 0) {
                        counts[0] += hi - lo;
                        ++stats[4];
                        stats[5] += L < k;
                    }
                    ++stats[2];
                    for (int j = j0; j < std::min(j0 + MH_CHUNK, num_perm); ++j) {  // a lane a permutation
                        uint32_t m = 0xFFFFFFFFu;
                        for (int32_t q = lo; q < hi; ++q) m = std::min(m, mh_hash(par[(size_t)j], L >= k ? x[(size_t)q] : xs));
                        uint32_t& w = sig[(k0 + i) * num_perm + j];
                        w = std::min(w, m);
                    }
                }
            }
        }
    }
    for (int64_t d = 0; d < n_docs; ++d)
        for (int b = 0; b < bands; ++b) keys[d * bands + b] = mh_band_key(sig + d * num_perm, b, rows);
    return 0;
}
