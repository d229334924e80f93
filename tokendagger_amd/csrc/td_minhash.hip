// MinHash signatures and LSH band keys (td_minhash*, td_encode_batch_minhash): ids + per-document token offsets -> sig[d][j], the
// minimum over the document's shingles of the j-th permutation of the shingle's hash, and key[d][b], the fold of a band of sig[d].  The
// rule is the contract in include/tokendagger_hip.h; td_minhash_args.h has the family and the fold, td_ngram_args.h the window hash.
//
// A shingle is at most 64 ids long and belongs to the tile of its start, so a tile needs the 63 ids behind it and nothing in front:
// they are read again by the tile itself, nothing is carried from tile to tile and no workgroup waits for another.
//
//   td_mh_params   a lane a permutation: (a_j, b_j) into the handle's table, only when the seed or num_perm change
//   td_mh_docs     a lane a document: the offsets checks.  The lowest bad document is kept in head; every later kernel returns when
//                  there is one, td_mh_tiles raises it: nothing is written then.  Also the documents without an id and the short ones.
//   td_mh_clear    sig to all ones, counts to {0, documents without an id, short documents, 0}
//   td_mh_tiles    a workgroup a tile of 4096 starts [t0, t0 + 4096):
//     load         ids [t0, t0 + 4096 + 64) into LDS by int4, padded (a lane's run starts 17 words behind its neighbour's)
//     locate       the tile's documents by td_rows_common.h's locator (group_last_le, tile_table); runs of empty documents that
//                  overflow the table: the offsets themselves, bisected by last_le_global
//     hash         sixteen consecutive starts a lane: one full window hash, fifteen rolls, the sixteen finished hashes x into LDS,
//                  whatever document they lie in (a window across a boundary is hashed and never read)
//     minima       the roles turn: a LANE IS A PERMUTATION.  A wavefront takes the 1024 starts its own lanes hashed and, per chunk of
//                  64 permutations, holds (a_j, b_j) of permutation j = chunk + lane in four registers (one 16-byte load a chunk and
//                  tile).  The valid starts of a document inside a tile are ONE run [lo, hi) — its full windows, or its first position
//                  when it is shorter than k — so the wavefront walks its documents, reads every x of the run from LDS at an address
//                  all lanes share (a broadcast, four x a read) and keeps the running minimum of h_j(x) in one register.  Per
//                  (shingle, permutation): a 64-bit multiply-add, a 32-bit multiply-add and a minimum; no cross-lane step, no LDS
//                  atomic, no slots that a tile could have too few of.
//     merge        the end of a (document, wavefront, chunk) run is one global atomicMin wave-instruction over 64 consecutive words
//                  of the document's row: 256 contiguous bytes.  A minimum does not depend on the order of its operands.
//     count        the shingles hashed, through block_sum and one add a tile
//   td_mh_finish   behind the tiles in stream order, a lane a (document, band): the fold.  Launched only when keys are wanted.
//
// Nothing outside ids[0, total), tok_off[0, n_docs] and params[0, num_perm) is read.
#include <hip/hip_runtime.h>

#include "td_minhash.h"
#include "td_rows_common.h"

namespace td {

namespace {

static_assert(MH_THREADS == RC_THREADS && MH_TILE == RC_TILE, "the row kernels' launch shape");
constexpr int MH_MAX_GRID = 1 << 20;
constexpr int MH_LDS_WORDS = MH_LDS_IDS + (MH_LDS_IDS >> 4) + 1;
constexpr int32_t MH_OFF_LO = -MH_MAX_K;             // a document's start, from the tile's first start: clamped to where every length is >= k
constexpr int32_t MH_OFF_HI = MH_TILE + MH_MAX_K + 1;  // a document's end: clamped above every window's end
constexpr long long MH_BAD_TOP = 1ll << 62;

__device__ __forceinline__ int mh_idx(int j) { return j + (j >> 4); }

__device__ __forceinline__ void mh_add(unsigned long long* p, unsigned long long n) {
    __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The handle's table: a lane a permutation (launched only when the seed or num_perm differ from the table's)
__global__ __launch_bounds__(MH_THREADS) void td_mh_params(MhParam* table, uint64_t seed, int num_perm) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < num_perm) table[j] = mh_param(seed, j);
}

__global__ __launch_bounds__(MH_THREADS) void td_mh_docs(const MhashArgs a) {
    __shared__ long long s_red[MH_THREADS / 64];
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.tok_off[0] != 0) atomicMax(&a.head[MH_H_BAD], (unsigned long long)MH_BAD_TOP);
    long long n_empty = 0, n_short = 0;
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_tokens) atomicMax(&a.head[MH_H_BAD], (unsigned long long)(MH_BAD_TOP - d));
        n_empty += hi == lo;
        n_short += hi > lo && hi - lo < a.k;
    }
    n_empty = block_sum(n_empty, s_red);
    n_short = block_sum(n_short, s_red);
    if (threadIdx.x == 0) {
        if (n_empty) mh_add(a.head + MH_H_EMPTY, (unsigned long long)n_empty);
        if (n_short) mh_add(a.head + MH_H_SHORT, (unsigned long long)n_short);
    }
}

__global__ __launch_bounds__(MH_THREADS) void td_mh_clear(const MhashArgs a) {
    if (a.head[MH_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid == 0) {
        a.counts[0] = 0;
        a.counts[1] = a.head[MH_H_EMPTY];
        a.counts[2] = a.head[MH_H_SHORT];
        a.counts[3] = 0;
    }
    // sig: the words in front of the first 16-byte boundary, the int4s, the words behind the last
    const int64_t n = a.n_docs * a.num_perm;
    int64_t front = (int64_t)(((16 - (((uintptr_t)a.sig) & 15)) & 15) / 4);
    front = front < n ? front : n;
    const int64_t n4 = (n - front) / 4;
    uint4* q = reinterpret_cast<uint4*>(a.sig + front);
    for (int64_t i = gid; i < front; i += step) a.sig[i] = ~0u;
    for (int64_t i = gid; i < n4; i += step) q[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (int64_t i = front + 4 * n4 + gid; i < n; i += step) a.sig[i] = ~0u;
}

__global__ __launch_bounds__(MH_THREADS) void td_mh_tiles(const MhashArgs a) {
    __shared__ int32_t s_ids[MH_LDS_WORDS];
    __shared__ int32_t s_off[RC_LDS_DOCS];        // tok_off[k0 + i] - t0, clamped to [MH_OFF_LO, MH_OFF_HI]
    __shared__ alignas(16) uint32_t s_x[MH_TILE];  // the finished hash of the window at every start
    __shared__ long long s_red[MH_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (const unsigned long long bad = a.head[MH_H_BAD]) {
        if (blockIdx.x == 0 && tid == 0) rows_raise(a, TD_E_INVALID, (int64_t)(MH_BAD_TOP - (long long)bad));
        return;
    }
    const int64_t total = a.tok_off[a.n_docs], ntiles = (total + MH_TILE - 1) / MH_TILE;
    const bool ids16 = (((uintptr_t)a.ids) & 15) == 0;
    const int k = a.k, num_perm = a.num_perm;
    const uint32_t bk = ng_base_pow(k);
    const auto off_of = [off = a.tok_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * MH_TILE;
        const int64_t s1 = t0 + MH_TILE < total ? t0 + MH_TILE : total;  // behind the tile's last start
        __syncthreads();  // (the tile before has read its tables)
        for (int r = tid; r < MH_LDS_IDS / 4; r += MH_THREADS) {
            const int64_t p = t0 + 4 * r;
            int32_t v[4];
            if (p + 4 <= total && ids16) {
                const int4 q = *reinterpret_cast<const int4*>(a.ids + p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = p + c < total ? a.ids[p + c] : -1;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) s_ids[mh_idx(4 * r + c)] = v[c];
        }
        // ---- the tile's documents: tok_off[0] = 0 <= t0 < s1 <= total = tok_off[n_docs] ---------------------------------------------------
        bool lds;
        const int64_t k0 = group_last_le(off_of, 0, a.n_docs, t0);
        int64_t nk = tile_table(s_off, off_of, k0, a.n_docs, t0, MH_OFF_LO, MH_OFF_HI, (int32_t)(s1 - t0), lds);
        if (!lds) nk = group_last_le(off_of, k0, a.n_docs, s1 - 1) - k0 + 1;
        __syncthreads();  // (the ids are in LDS)
        // ---- hash: a lane's sixteen starts ------------------------------------------------------------------------------------------------
        {
            const int jb = MH_PER * tid;
            uint32_t h = ng_hash_full([&](int j) { return s_ids[mh_idx(jb + j)]; }, k);
            uint32_t x[MH_PER];
#pragma unroll
            for (int i = 0; i < MH_PER; ++i) {
                if (i) h = ng_hash_roll(h, s_ids[mh_idx(jb + i - 1)], s_ids[mh_idx(jb + i - 1 + k)], bk);
                x[i] = ng_finish(h, k);
            }
#pragma unroll
            for (int c = 0; c < MH_PER / 4; ++c)
                *reinterpret_cast<uint4*>(s_x + jb + 4 * c) = make_uint4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
        }
        __syncthreads();
        // ---- minima: a lane a permutation, the wavefront over its 1024 starts' documents ---------------------------------------------------
        const int32_t r0 = MH_WAVE_STARTS * __builtin_amdgcn_readfirstlane(wv);  // (scalar: the walk's loops are the wavefront's, not a lane's)
        const int32_t r1 = s1 - t0 < r0 + MH_WAVE_STARTS ? (int32_t)(s1 - t0) : r0 + MH_WAVE_STARTS;
        uint32_t n_sh = 0;  // (the same in every lane of the wavefront)
        // rel(i): tok_off[k0 + i] - t0, clamped, for 0 <= i <= nk; the same in every lane
        const auto walk = [&](auto rel) {
            const int64_t i0 = last_le_global(rel, 0, nk, r0);
            for (int j0 = 0; j0 < num_perm; j0 += MH_CHUNK) {
                const int j = j0 + lane;
                const bool active = j < num_perm;
                const MhParam p = active ? a.params[j] : MhParam{1, 0};
                for (int64_t i = i0; i < nk; ++i) {
                    const int32_t da = rel(i);
                    if (da >= r1) break;
                    const int32_t de = rel(i + 1), L = de - da;
                    if (L == 0) continue;
                    uint32_t m = ~0u, n;
                    if (L >= k) {  // the full windows that start in [r0, r1)
                        const int32_t lo = da > r0 ? da : r0, hi = de - k + 1 < r1 ? de - k + 1 : r1;
                        if (lo >= hi) continue;
                        int32_t q = lo;
                        for (; q < hi && (q & 3); ++q) m = min(m, mh_hash(p, s_x[q]));
                        for (; q + 4 <= hi; q += 4) {
                            const uint4 v = reinterpret_cast<const uint4*>(s_x)[q >> 2];
                            m = min(min(m, mh_hash(p, v.x)), min(mh_hash(p, v.y), min(mh_hash(p, v.z), mh_hash(p, v.w))));
                        }
                        for (; q < hi; ++q) m = min(m, mh_hash(p, s_x[q]));
                        n = (uint32_t)(hi - lo);
                    } else {  // shorter than k: the whole document, where it starts (da >= 0: not clamped)
                        if (da < r0) continue;
                        m = mh_hash(p, mh_shingle([&](int c) { return s_ids[mh_idx(da + c)]; }, L));
                        n = 1;
                    }
                    if (j0 == 0) n_sh += n;
                    if (active) atomicMin(a.sig + (k0 + i) * num_perm + j, m);
                }
            }
        };
        if (r0 < r1) {
            if (lds) {
                walk([&](int64_t i) { return __builtin_amdgcn_readfirstlane(s_off[i]); });
            } else {
                walk([&, off = a.tok_off + k0](int64_t i) {
                    const int64_t r = off[i] - t0;
                    return __builtin_amdgcn_readfirstlane(r < MH_OFF_LO ? MH_OFF_LO : r > MH_OFF_HI ? MH_OFF_HI : (int32_t)r);
                });
            }
        }
        const long long sh = block_sum(lane == 0 ? (long long)n_sh : 0, s_red);
        if (tid == 0 && sh) mh_add(a.counts + 0, (unsigned long long)sh);
    }
}

__global__ __launch_bounds__(MH_THREADS) void td_mh_finish(const MhashArgs a) {
    if (a.head[MH_H_BAD]) return;
    const int64_t n = a.n_docs * a.bands;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = i / a.bands, b = i - d * a.bands;
        a.band_keys[i] = mh_band_key(a.sig + d * a.num_perm, b, a.rows);
    }
}

}  // namespace

hipError_t launch_minhash_params(MhParam* table, uint64_t seed, int num_perm, hipStream_t stream) {
    hipLaunchKernelGGL(td_mh_params, dim3((unsigned)((num_perm + MH_THREADS - 1) / MH_THREADS)), dim3(MH_THREADS), 0, stream, table, seed, num_perm);
    return hipGetLastError();
}

hipError_t launch_minhash(const MhashArgs& a, hipStream_t stream) {
    const auto grid_of = [](int64_t n, int64_t per, int64_t most) {
        const int64_t g = (n + per - 1) / per;
        return (unsigned)(g < 1 ? 1 : g < most ? g : most);
    };
    hipError_t e;
    hipLaunchKernelGGL(td_mh_docs, dim3(grid_of(a.n_docs + 1, MH_THREADS, 4096)), dim3(MH_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_mh_clear, dim3(grid_of(a.n_docs * a.num_perm, 4 * MH_THREADS, 8192)), dim3(MH_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_mh_tiles, dim3(grid_of(a.n_tokens, MH_TILE, MH_MAX_GRID)), dim3(MH_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.bands > 0) {
        hipLaunchKernelGGL(td_mh_finish, dim3(grid_of(a.n_docs * a.bands, MH_THREADS, 4096)), dim3(MH_THREADS), 0, stream, a);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace td
