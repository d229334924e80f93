// N-gram matches (td_ngram_matches*, td_encode_batch_ngram_matches): ids + per-document token offsets + a set of id sequences ->
// which ids lie inside an occurrence of a listed sequence (cover, labels), and how many occurrences start in every document, of every
// pattern and in all.  The rule is the contract in include/tokendagger_hip.h; td_ngram_args.h has the hash, the table and the probe.
//
// An occurrence is at most 64 ids long, so what a tile needs from its neighbours is bounded: the 63 ids behind it (windows that start
// in the tile) and the starts of the 63 positions in front of it (occurrences that reach into the tile).  Both are read again by the
// tile itself; nothing is carried from tile to tile and no workgroup waits for another.
//
//   td_ng_docs     a lane a document: the offsets checks.  The lowest bad document is kept in head; every later kernel returns when
//                  there is one, td_ng_tiles raises it: nothing is written then.
//   td_ng_clear    zeroes doc_stats, counts and (without TD_NGRAM_ACCUMULATE) pattern_counts
//   td_ng_tiles    a workgroup a tile of 4096 positions [t0, t0 + 4096), sixteen consecutive starts a lane:
//     load         ids [t0 - 64, t0 + 4096 + 64) into LDS by int4, padded (a lane's run starts 17 words behind its neighbour's)
//     locate       the tile's documents by td_rows_common.h's locator (group_last_le, tile_table, a lane's last_le; runs of empty
//                  documents that overflow the table: last_le_global over the offsets).  A start's room = the ids from it to its
//                  document's end, at most 64, as a byte in LDS; 0 in front of the first id and behind the last.
//     hash, look up  per length of the set: one full window hash a lane, fifteen rolls; the sixteen finished hashes, then the walks of
//                  the starts with room side by side: a step loads the next slot of every start that still walks (up to sixteen
//                  independent 8-byte loads in flight a lane) and ng_slot_step decides each; at most max_probe + 1 steps.  Lanes
//                  0 - 3 do the same afterwards for the starts in front of the tile whose windows reach into it.
//     reach, cover the longest match at every start as a byte in LDS; a lane's furthest reach, the exclusive maximum over the lanes
//                  (wave_incl_scan, the wavefronts' through LDS) seeded with the furthest reach of the starts in front of the tile;
//                  covered(i) = the running maximum exceeds i.
//     write        cover: sixteen bytes a lane; labels: the flags through LDS, four ids a lane and step, an int4 of ignore_index
//                  where all four are covered, single dwords for the covered ones elsewhere.  Uncovered slots are not stored to.
//     count        occurrences only of the starts in [t0, t0 + 4096).  A lane adds its documents' (occurrences, covered ids) to the
//                  tile's per-document words in LDS; one pair of global adds per (document, tile) afterwards.  pattern_counts: an
//                  add an occurrence.
//   td_ng_finish   a lane a document: documents with an occurrence -> counts[2]
//
// Nothing outside ids[0, total), tok_off[0, n_docs] and the set's arrays is read: a slot index is masked, a pattern index comes
// from a slot the host wrote.
#include <hip/hip_runtime.h>

#include "td_ngrams.h"
#include "td_rows_common.h"

namespace td {

namespace {

static_assert(NG_THREADS == RC_THREADS && NG_TILE == RC_TILE, "the row kernels' launch shape");
constexpr int NG_MAX_GRID = 1 << 20;
constexpr int NG_LDS_WORDS = NG_LDS_IDS + (NG_LDS_IDS >> 4) + 1;
constexpr int32_t NG_END_HI = NG_SPAN + NG_MAX_LEN + 1;  // a document's end, from the tile's first start: clamped above every window's end
constexpr long long NG_BAD_TOP = 1ll << 62;

__device__ __forceinline__ int ng_idx(int j) { return j + (j >> 4); }

__device__ __forceinline__ void ng_add(unsigned long long* p, unsigned long long n) {
    __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t ng_total(const NgramArgs& a) { return a.tok_off[a.n_docs]; }

__global__ __launch_bounds__(NG_THREADS) void td_ng_docs(const NgramArgs a) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.tok_off[0] != 0) atomicMax(&a.head[NG_H_BAD], (unsigned long long)NG_BAD_TOP);
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_tokens) atomicMax(&a.head[NG_H_BAD], (unsigned long long)(NG_BAD_TOP - d));
    }
}

__global__ __launch_bounds__(NG_THREADS) void td_ng_clear(const NgramArgs a, int64_t n_pats, int zero_pats) {
    if (a.head[NG_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid < 4) a.counts[gid] = 0;
    for (int64_t i = gid; i < 2 * a.n_docs; i += step) a.doc_stats[i] = 0;
    if (a.pat_counts && zero_pats)
        for (int64_t i = gid; i < n_pats; i += step) a.pat_counts[i] = 0;
}

// The sixteen starts at LDS positions [jb, jb + 16) (position 0 = id t0 - NG_FRONT), every length of the set: s_ko[pos] = the longest
// match at the start | its matches << 8.  s_room, s_ko: the lane's own sixteen entries are read and written, nobody else's.
template <bool MAIN>
__device__ __forceinline__ void ng_run(const NgramArgs& a, const int32_t* s_ids, const uint32_t* s_room, uint16_t* s_ko, int jb) {
    const uint4 rw = *reinterpret_cast<const uint4*>(s_room + (jb >> 2));
    const uint32_t room[4] = {rw.x, rw.y, rw.z, rw.w};
    if ((room[0] | room[1] | room[2] | room[3]) == 0) return;  // (in front of the first id, behind the last)
    for (int l = 0; l < a.tab.n_lengths; ++l) {
        const int k = a.tab.length(l);
        const uint32_t bk = ng_base_pow(k);
        uint32_t fit = 0;
#pragma unroll
        for (int i = 0; i < NG_PER; ++i) fit |= ((room[i >> 2] >> (8 * (i & 3))) & 0xFFu) >= (uint32_t)k ? 1u << i : 0u;
        if constexpr (!MAIN) {  // a start in front of the tile matters only when its window reaches into the tile
            const int first = NG_FRONT - k + 1 - jb;  // the lane's first such start
            fit &= first <= 0 ? 0xFFFFu : first >= NG_PER ? 0u : 0xFFFFu << first;
        }
        if (!fit) continue;
        uint32_t h = ng_hash_full([&](int j) { return s_ids[ng_idx(jb + j)]; }, k);
        uint32_t x[NG_PER];
#pragma unroll
        for (int i = 0; i < NG_PER; ++i) {
            if (i) h = ng_hash_roll(h, s_ids[ng_idx(jb + i - 1)], s_ids[ng_idx(jb + i - 1 + k)], bk);
            x[i] = ng_finish(h, k);
        }
        // the sixteen walks side by side: every step loads the next slot of every start that still walks (independent loads, one
        // latency a step for all of them), at most max_probe + 1 steps
        uint32_t alive = fit;
        for (uint32_t d = 0; d <= a.tab.max_probe && alive; ++d) {
            NgSlot sl[NG_PER];
#pragma unroll
            for (int i = 0; i < NG_PER; ++i) {
                sl[i] = NgSlot{0, 0};
                if ((alive >> i) & 1u) sl[i] = a.tab.slots[(x[i] + d) & a.tab.slot_mask];
            }
#pragma unroll
            for (int i = 0; i < NG_PER; ++i) {
                if (!((alive >> i) & 1u)) continue;
                const int32_t p = ng_slot_step(a.tab, sl[i], x[i], k, a.tag_mask, [&](int j) { return s_ids[ng_idx(jb + i + j)]; });
                if (p == NG_NEXT) continue;
                alive &= ~(1u << i);
                if (p < 0) continue;
                s_ko[jb + i] = (uint16_t)(((s_ko[jb + i] & 0xFF00u) + 0x100u) | (uint32_t)k);  // (lengths ascend: k is the longest so far)
                if constexpr (MAIN)
                    if (a.pat_counts) ng_add(a.pat_counts + a.tab.pat_orig[p], 1ull);
            }
        }
    }
}

__global__ __launch_bounds__(NG_THREADS) void td_ng_tiles(const NgramArgs a) {
    __shared__ int32_t s_ids[NG_LDS_WORDS];
    __shared__ int32_t s_off[RC_LDS_DOCS];   // tok_off[k0 + i] - s0, clamped to [0, NG_END_HI]
    __shared__ uint32_t s_acc[RC_LDS_DOCS];  // document k0 + i in this tile: occurrences << 13 | covered ids (at most 8 * 4096, 4096)
    __shared__ alignas(16) uint32_t s_room[NG_SPAN / 4]; // a byte a start: its room; afterwards a byte a position: covered
    __shared__ alignas(16) uint16_t s_ko[NG_SPAN];     // a start's longest match | its matches << 8
    __shared__ int32_t s_wave[NG_THREADS / 64];
    __shared__ int32_t s_seed;
    __shared__ long long s_red[NG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (const unsigned long long bad = a.head[NG_H_BAD]) {
        if (blockIdx.x == 0 && tid == 0) rows_raise(a, TD_E_INVALID, (int64_t)(NG_BAD_TOP - (long long)bad));
        return;
    }
    const int64_t total = ng_total(a), ntiles = (total + NG_TILE - 1) / NG_TILE;
    const bool ids16 = (((uintptr_t)a.ids) & 15) == 0;
    const auto off_of = [off = a.tok_off](int64_t k) { return off[k]; };
    for (int i = tid; i < RC_LDS_DOCS; i += NG_THREADS) s_acc[i] = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * NG_TILE, base = t0 - NG_FRONT;
        const int64_t s0 = base > 0 ? base : 0;                          // the first start looked at
        const int64_t s1 = t0 + NG_TILE < total ? t0 + NG_TILE : total;  // behind the last
        __syncthreads();  // (the tile before is stored, its tables are read)
        for (int r = tid; r < NG_LDS_IDS / 4; r += NG_THREADS) {
            const int64_t p = base + 4 * r;
            int32_t v[4];
            if (p >= 0 && p + 4 <= total && ids16) {
                const int4 q = *reinterpret_cast<const int4*>(a.ids + p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = p + c >= 0 && p + c < total ? a.ids[p + c] : -1;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) s_ids[ng_idx(4 * r + c)] = v[c];
        }
        // ---- the tile's documents: tok_off[0] = 0 <= s0 < s1 <= total = tok_off[n_docs] -------------------------------------------------
        bool lds;
        const int64_t k0 = group_last_le(off_of, 0, a.n_docs, s0);
        int64_t nk = tile_table(s_off, off_of, k0, a.n_docs, s0, 0, NG_END_HI, (int32_t)(s1 - s0), lds);
        if (!lds) nk = group_last_le(off_of, k0, a.n_docs, s1 - 1) - k0 + 1;
        // ---- room: the lane's sixteen starts, and the halo's by lanes 0 - 3 ------------------------------------------------------------
        const auto fill_room = [&](int jb) {
            uint32_t w[4] = {0, 0, 0, 0};
            int64_t end = -1;  // the starts below it are in one document
#pragma unroll
            for (int i = 0; i < NG_PER; ++i) {
                const int64_t q = base + jb + i;
                if (q < s0 || q >= s1) continue;
                if (q >= end) {
                    if (lds) end = s0 + s_off[last_le(s_off, (int)nk, (int32_t)(q - s0)) + 1];
                    else end = a.tok_off[k0 + last_le_global([off = a.tok_off + k0](int64_t x) { return off[x]; }, 0, nk, q) + 1];
                }
                const int64_t room = end - q < NG_MAX_LEN ? end - q : NG_MAX_LEN;
                w[i >> 2] |= (uint32_t)room << (8 * (i & 3));
            }
            *reinterpret_cast<uint4*>(s_room + (jb >> 2)) = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint4*>(s_ko + jb) = make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(s_ko + jb + 8) = make_uint4(0, 0, 0, 0);
        };
        fill_room(NG_FRONT + NG_PER * tid);
        if (tid < NG_FRONT / NG_PER) fill_room(NG_PER * tid);
        __syncthreads();  // (the ids are in LDS; a lane's room and matches are its own)
        // ---- hash and look up -------------------------------------------------------------------------------------------------------------
        const int jb = NG_FRONT + NG_PER * tid;
        ng_run<true>(a, s_ids, s_room, s_ko, jb);
        if (tid < NG_FRONT / NG_PER) ng_run<false>(a, s_ids, s_room, s_ko, NG_PER * tid);
        __syncthreads();
        // ---- reach: in LDS positions, 0 = none ----------------------------------------------------------------------------------------------
        if (wv == 0) {
            const int k = s_ko[lane] & 0xFF;
            int32_t r = k ? lane + k : 0;
            for (int d = 32; d >= 1; d >>= 1) r = max(r, __shfl_xor(r, d));
            if (lane == 0) s_seed = r;
        }
        const int64_t p0 = t0 + NG_PER * tid;
        const int nv = total - p0 >= NG_PER ? NG_PER : total - p0 > 0 ? (int)(total - p0) : 0;  // positions of the lane below total
        int32_t mine = 0;
        for (int i = 0; i < nv; ++i) {
            const int k = s_ko[jb + i] & 0xFF;
            if (k) mine = max(mine, jb + i + k);
        }
        const int32_t incl = wave_incl_scan(mine, lane, [](int32_t x, int32_t y) { return max(x, y); });
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        int32_t run = s_seed;
        for (int w = 0; w < wv; ++w) run = max(run, s_wave[w]);
        const int32_t prev = __shfl_up(incl, 1);
        if (lane) run = max(run, prev);
        // ---- the walk: covered positions, the documents' sums ------------------------------------------------------------------------------
        uint32_t cb = 0, n_occ = 0, n_cov = 0, d_occ = 0, d_cov = 0;
        int64_t end = -1, doc = -1;
        const auto doc_flush = [&] {
            if (doc < 0 || (d_occ | d_cov) == 0) return;
            if (lds) {
                atomicAdd(&s_acc[doc - k0], d_occ << 13 | d_cov);
            } else {
                if (d_occ) ng_add(a.doc_stats + 2 * doc, d_occ);
                if (d_cov) ng_add(a.doc_stats + 2 * doc + 1, d_cov);
            }
        };
        for (int i = 0; i < nv; ++i) {
            const int64_t q = p0 + i;
            if (q >= end) {
                doc_flush();
                d_occ = d_cov = 0;
                if (lds) doc = k0 + last_le(s_off, (int)nk, (int32_t)(q - s0));
                else doc = k0 + last_le_global([off = a.tok_off + k0](int64_t x) { return off[x]; }, 0, nk, q);
                end = lds ? s0 + s_off[doc - k0 + 1] : a.tok_off[doc + 1];
            }
            const uint32_t ko = s_ko[jb + i];
            if (ko & 0xFFu) run = max(run, (int32_t)(jb + i + (ko & 0xFFu)));
            const uint32_t cov = run > jb + i ? 1u : 0u;
            cb |= cov << i;
            d_cov += cov;
            d_occ += ko >> 8;
            n_cov += cov;
            n_occ += ko >> 8;
        }
        doc_flush();
        uint32_t cw[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t n4 = (cb >> (4 * c)) & 15u;
            cw[c] = (n4 & 1u) | (n4 & 2u) << 7 | (n4 & 4u) << 14 | (n4 & 8u) << 21;
        }
        *reinterpret_cast<uint4*>(s_room + (jb >> 2)) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
        if (a.cover && nv > 0) {
            uint8_t* cp = a.cover + p0;
            if (nv == NG_PER && (((uintptr_t)cp) & 15) == 0) {
                *reinterpret_cast<uint4*>(cp) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
            } else {
                for (int i = 0; i < nv; ++i) cp[i] = (cb >> i) & 1u;
            }
        }
        const long long sums = block_sum((long long)n_occ << 32 | n_cov, s_red);  // (and the flags and the documents' words are in LDS)
        if (tid == 0) {
            if (sums >> 32) ng_add(a.counts + 0, (unsigned long long)(sums >> 32));
            if (sums & 0xFFFFFFFFll) ng_add(a.counts + 1, (unsigned long long)(sums & 0xFFFFFFFFll));
        }
        if (a.labels) {
            const bool out16 = (((uintptr_t)a.labels) & 15) == 0;
            const int32_t ig = a.ignore;
            for (int r = tid; r < NG_TILE / 4; r += NG_THREADS) {
                const int64_t p = t0 + 4 * r;
                if (p >= total) break;
                const uint32_t f = s_room[NG_FRONT / 4 + r];
                if (f == 0x01010101u && p + 4 <= total && out16) {
                    *reinterpret_cast<int4*>(a.labels + p) = make_int4(ig, ig, ig, ig);
                } else if (f) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((f >> (8 * c)) & 1u && p + c < total) a.labels[p + c] = ig;
                }
            }
        }
        if (lds) {
            for (int i = tid; i < (int)nk; i += NG_THREADS) {
                const uint32_t v = s_acc[i];
                if (v == 0) continue;
                s_acc[i] = 0;
                if (v >> 13) ng_add(a.doc_stats + 2 * (k0 + i), v >> 13);
                if (v & 0x1FFFu) ng_add(a.doc_stats + 2 * (k0 + i) + 1, v & 0x1FFFu);
            }
        }
    }
}

__global__ __launch_bounds__(NG_THREADS) void td_ng_finish(const NgramArgs a) {
    __shared__ long long s_red[NG_THREADS / 64];
    if (a.head[NG_H_BAD]) return;
    long long n = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x)
        n += a.doc_stats[2 * d] != 0;
    n = block_sum(n, s_red);
    if (threadIdx.x == 0 && n) ng_add(a.counts + 2, (unsigned long long)n);
}

}  // namespace

hipError_t launch_ngram_matches(const NgramArgs& a, int64_t n_pats, bool zero_pat_counts, hipStream_t stream) {
    const auto grid_of = [](int64_t n, int64_t per, int64_t most) {
        const int64_t g = (n + per - 1) / per;
        return (unsigned)(g < 1 ? 1 : g < most ? g : most);
    };
    const unsigned g_docs = grid_of(a.n_docs + 1, NG_THREADS, 4096);
    const int64_t zero = a.pat_counts && zero_pat_counts && n_pats > 2 * a.n_docs ? n_pats : 2 * a.n_docs;
    hipError_t e;
    hipLaunchKernelGGL(td_ng_docs, dim3(g_docs), dim3(NG_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_ng_clear, dim3(grid_of(zero, NG_THREADS, 4096)), dim3(NG_THREADS), 0, stream, a, n_pats, zero_pat_counts ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_ng_tiles, dim3(grid_of(a.n_tokens, NG_TILE, NG_MAX_GRID)), dim3(NG_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_ng_finish, dim3(g_docs), dim3(NG_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
