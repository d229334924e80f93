// Token counts (td_token_counts*, td_encode_batch_token_counts): ids (or any int32 stream aligned with them) [+ per-document token
// offsets + a group per document] -> counts[group * n_bins + value], 64-bit, and info[4] = counted / negative / too large / in a
// document of a bad group.  A histogram of up to 2^28 bins: no LDS holds it, and the values are skewed (one id is a sixth of an
// English corpus), so adding every id to global memory runs at the rate of ONE word's atomics.  One kernel:
//
//   td_cnt_tiles    at most CNT_MAX_GRID workgroups stride over tiles of CNT_TILE positions (absolute multiples of the tile, so a
//                   lane's four ids are one int4 wherever the caller's pointer is 16-byte aligned; dwords otherwise and at the
//                   ends of the visited range).  A lane loads its sixteen ids first and counts them afterwards.
//     table         every workgroup keeps 2^seat_bits seats (key, count) in LDS, key = group * n_bins + value.  A key tries two
//                   seats, cnt_seat(key) and that ^ 1: a plain read finds a seat it already holds, a compare-and-swap on the key
//                   takes an empty one, then one LDS add on the count.  Before that, a wavefront whose 64 lanes hold ONE key
//                   (padding, a run of one id) adds 64 by one lane.
//     conflict      a key that finds both seats held by others goes to global memory, but not alone: the wavefront's lanes with
//                   the same key are found by ballot and ONE lane adds their number.  Policy: first come, first seated, until
//                   the next flush; nothing is evicted in between.  The worst order is a tile of cold ids that takes the hot
//                   id's two seats first: the hot id then costs one global atomic per wavefront step (64 ids) until the flush, at
//                   most CNT_FLUSH_TILES tiles later, clears the table and the next tile's ids are seated by their frequency again.
//     flush         behind every flush_tiles tiles (CNT_FLUSH_TILES; TD_OPT_COUNTS_FLUSH_TILES shrinks it for tests) and behind the last: occupied seats only, one 64-bit add each, seat cleared.
//                   A 32-bit seat counter therefore never exceeds CNT_FLUSH_TILES * CNT_TILE = 2^18.
//     groups        <true>: the tile's documents by td_rows_common.h's locator (group_last_le for the first, tile_table for the
//                   offsets behind it, a lane's last_le), their groups into LDS beside the offsets; a tile inside one document
//                   resolves its group once; a tile whose documents overflow the table (thousands of empty ones) finds its last
//                   by a second group_last_le and bisects over the offsets themselves (last_le_global).
//     offsets       <true>: every workgroup checks a slice of tok_off for a decrease before its tiles
//   Nothing outside ids[0, n_tokens), tok_off[0, n_docs] and doc_group[0, n_docs) is read and nothing outside counts / info is
//   written, whatever the offsets and the values are: a position is visited only inside [max(lo, 0), min(hi, n_tokens)), a key is
//   made only of 0 <= value < n_bins and 0 <= group < n_groups.
#include <hip/hip_runtime.h>

#include "td_counts.h"
#include "td_rows_common.h"

namespace td {

namespace {

static_assert(CNT_THREADS == RC_THREADS && CNT_TILE == RC_TILE && CNT_MAX_GRID <= RC_MAX_GRID, "the row kernels' launch shape");
constexpr int CNT_ITERS = CNT_TILE / (4 * CNT_THREADS);

__device__ __forceinline__ void cnt_global_add(const CountsArgs& a, int32_t key, unsigned long long n) {
    __hip_atomic_fetch_add(a.counts + key, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// occupied seats to counts, and every seat empty again; by the whole workgroup, barriers on both sides
__device__ __forceinline__ void cnt_flush(const CountsArgs& a, int32_t* s_key, uint32_t* s_cnt, int seats) {
    __syncthreads();
    for (int s = threadIdx.x; s < seats; s += CNT_THREADS) {
        const int32_t k = s_key[s];
        if (k != CNT_EMPTY) {
            cnt_global_add(a, k, (unsigned long long)s_cnt[s]);
            s_key[s] = CNT_EMPTY;
            s_cnt[s] = 0;
        }
    }
    __syncthreads();
}

// true: `key` sits (or now sits) in seat s
__device__ __forceinline__ bool cnt_take(int32_t* s_key, uint32_t s, int32_t key) {
    int32_t k = s_key[s];
    if (k == CNT_EMPTY) {
        k = atomicCAS(&s_key[s], CNT_EMPTY, key);
        if (k == CNT_EMPTY) return true;
    }
    return k == key;
}

// One step of a wavefront, in uniform control flow: every lane brings a key or CNT_EMPTY (nothing to count).
__device__ __forceinline__ void cnt_step(const CountsArgs& a, int32_t* s_key, uint32_t* s_cnt, int32_t key, int lane) {
    const int32_t first = __builtin_amdgcn_readfirstlane(key);
    if (__all(key == first)) {  // one key in all 64 lanes (or none at all)
        if (first == CNT_EMPTY) return;
        uint32_t s = cnt_seat(first, a.seat_bits);
        bool seated = false;
        if (lane == 0) {
            seated = cnt_take(s_key, s, first);
            if (!seated) seated = cnt_take(s_key, s ^= 1u, first);
            if (seated) atomicAdd(&s_cnt[s], 64u);
            else cnt_global_add(a, first, 64ull);
        }
        return;
    }
    int32_t pend = CNT_EMPTY;
    if (key != CNT_EMPTY) {
        uint32_t s = cnt_seat(key, a.seat_bits);
        bool seated = cnt_take(s_key, s, key);
        if (!seated) seated = cnt_take(s_key, s ^= 1u, key);
        if (seated) atomicAdd(&s_cnt[s], 1u);
        else pend = key;
    }
    // equal keys of the wavefront reach global memory as one add
    for (unsigned long long m = __ballot(pend != CNT_EMPTY); m != 0; m = __ballot(pend != CNT_EMPTY)) {
        const int leader = __ffsll((long long)m) - 1;
        const int32_t k = __shfl(pend, leader);
        const bool same = pend == k;
        const unsigned long long n = (unsigned long long)__popcll(__ballot(same));
        if (lane == leader) cnt_global_add(a, k, n);
        if (same) pend = CNT_EMPTY;
    }
}

template <bool GROUPS>
__global__ __launch_bounds__(CNT_THREADS) void td_cnt_tiles(const CountsArgs a) {
    __shared__ int32_t s_key[CNT_SEATS];
    __shared__ uint32_t s_cnt[CNT_SEATS];
    __shared__ long long s_red[CNT_THREADS / 64];
    __shared__ int32_t s_off[GROUPS ? RC_LDS_DOCS : 1];  // tok_off[k0 + i] - s0, clamped to [0, CNT_TILE + 1]
    __shared__ int32_t s_grp[GROUPS ? RC_LDS_DOCS : 1];  // doc_group[k0 + i]
    const int tid = threadIdx.x, lane = tid & 63;
    const int seats = 1 << a.seat_bits;
    for (int s = tid; s < seats; s += CNT_THREADS) {
        s_key[s] = CNT_EMPTY;
        s_cnt[s] = 0;
    }
    // the visited positions [lo, hi), inside the buffer whatever the offsets say
    int64_t lo = 0, hi = a.n_tokens;
    if constexpr (GROUPS) {  // (one group: tok_off is null, every position of the buffer is visited)
        lo = a.tok_off[0];
        hi = a.tok_off[a.n_docs];
        if (lo < 0 || hi < lo || hi > a.n_tokens) {
            if (tid == 0) rows_raise(a, TD_E_INVALID, lo < 0 ? 0 : a.n_docs);
            lo = lo < 0 ? 0 : lo;
            hi = hi > a.n_tokens ? a.n_tokens : hi;
            hi = hi < lo ? lo : hi;
        }
    }
    const bool aligned = (((uintptr_t)a.ids) & 15) == 0;
    const int32_t n_bins = (int32_t)a.n_bins;
    long long n_counted = 0, n_negative = 0, n_large = 0, n_badgroup = 0;
    int since_flush = 0;
    [[maybe_unused]] const auto off_of = [off = a.tok_off](int64_t k) { return off[k]; };
    if constexpr (GROUPS) {
        // offsets that decrease are met here, by the grid as a whole: the searches below stay inside [0, n_docs] on any offsets, but
        // which document they find is only defined on sorted ones
        for (int64_t d = (int64_t)blockIdx.x * CNT_THREADS + tid; d < a.n_docs; d += (int64_t)gridDim.x * CNT_THREADS)
            if (a.tok_off[d + 1] < a.tok_off[d]) rows_raise(a, TD_E_INVALID, d);
    }
    __syncthreads();
    const int64_t stop = lo < hi ? hi : 0;  // (nothing visited: no tile, and no document is looked for)
    for (int64_t tile = lo / CNT_TILE + blockIdx.x; tile * CNT_TILE < stop; tile += gridDim.x) {
        const int64_t t0 = tile * CNT_TILE;
        const int64_t s0 = t0 > lo ? t0 : lo;
        const int64_t s1 = t0 + CNT_TILE < hi ? t0 + CNT_TILE : hi;
        // the ids first: four loads in flight a lane
        int32_t v[CNT_ITERS][4];
        uint32_t valid = 0;
#pragma unroll
        for (int it = 0; it < CNT_ITERS; ++it) {
            const int64_t j0 = t0 + (int64_t)it * 4 * CNT_THREADS + 4 * tid;
            if (aligned && j0 >= s0 && j0 + 4 <= s1) {
                const int4 x = *reinterpret_cast<const int4*>(a.ids + j0);
                v[it][0] = x.x; v[it][1] = x.y; v[it][2] = x.z; v[it][3] = x.w;
                valid |= 15u << (4 * it);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[it][q] = 0;
                    if (j0 + q >= s0 && j0 + q < s1) {
                        v[it][q] = a.ids[j0 + q];
                        valid |= 1u << (4 * it + q);
                    }
                }
            }
        }
        // the tile's documents
        [[maybe_unused]] int64_t k0 = 0, nk = 1;
        [[maybe_unused]] bool lds = true, one = true;
        [[maybe_unused]] int32_t g_one = 0;
        if constexpr (GROUPS) {
            __syncthreads();  // (the previous tile's readers of s_off and s_grp are done)
            k0 = group_last_le(off_of, 0, a.n_docs, s0);  // tok_off[0] = lo <= s0 < hi = tok_off[n_docs]
            nk = tile_table(s_off, off_of, k0, a.n_docs, s0, 0, CNT_TILE + 1, (int32_t)(s1 - s0), lds);
            if (!lds) nk = group_last_le(off_of, k0, a.n_docs, s1 - 1) - k0 + 1;
            one = nk <= 1;
            if (one) {
                g_one = a.doc_group[k0];
            } else if (lds) {
                for (int i = tid; i < (int)nk; i += CNT_THREADS) s_grp[i] = a.doc_group[k0 + i];
                __syncthreads();
            }
        }
#pragma unroll
        for (int it = 0; it < CNT_ITERS; ++it) {
            const int64_t j0 = t0 + (int64_t)it * 4 * CNT_THREADS + 4 * tid;
            [[maybe_unused]] int64_t end = one ? s1 : j0;  // the positions below it are in the document of group g (resolved when passed)
            [[maybe_unused]] int32_t g = g_one;
            [[maybe_unused]] int64_t doc = k0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int32_t key = CNT_EMPTY;
                if (valid >> (4 * it + q) & 1u) {
                    const int64_t j = j0 + q;
                    bool bad = false;
                    if constexpr (GROUPS) {
                        if (j >= end) {
                            if (lds) {
                                const int64_t i = last_le(s_off, nk, (int32_t)(j - s0));
                                end = s0 + s_off[i + 1];
                                g = s_grp[i];
                                doc = k0 + i;
                            } else {
                                const int64_t i = last_le_global([off = a.tok_off + k0](int64_t x) { return off[x]; }, 0, nk, j);
                                end = a.tok_off[k0 + i + 1];
                                g = a.doc_group[k0 + i];
                                doc = k0 + i;
                            }
                        }
                        bad = g < 0 || g >= a.n_groups;
                        if (bad) rows_raise(a, TD_E_INVALID, doc);
                    }
                    const int32_t x = v[it][q];
                    if (bad) ++n_badgroup;
                    else if (x < 0) ++n_negative;
                    else if (x >= n_bins) ++n_large;
                    else {
                        ++n_counted;
                        key = GROUPS ? g * n_bins + x : x;
                    }
                }
                cnt_step(a, s_key, s_cnt, key, lane);
            }
        }
        if (++since_flush >= a.flush_tiles) {
            cnt_flush(a, s_key, s_cnt, seats);
            since_flush = 0;
        }
    }
    if (since_flush) cnt_flush(a, s_key, s_cnt, seats);
    n_counted = block_sum(n_counted, s_red);
    n_negative = block_sum(n_negative, s_red);
    n_large = block_sum(n_large, s_red);
    n_badgroup = block_sum(n_badgroup, s_red);
    if (tid == 0) {
        if (n_counted) __hip_atomic_fetch_add(a.info + CNT_I_COUNTED, (unsigned long long)n_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_negative) __hip_atomic_fetch_add(a.info + CNT_I_NEGATIVE, (unsigned long long)n_negative, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_large) __hip_atomic_fetch_add(a.info + CNT_I_TOO_LARGE, (unsigned long long)n_large, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_badgroup) __hip_atomic_fetch_add(a.info + CNT_I_BAD_GROUP, (unsigned long long)n_badgroup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

hipError_t launch_token_counts(const CountsArgs& a, hipStream_t stream) {
    const int grid = cnt_grid(a.n_tokens);
    if (a.doc_group) hipLaunchKernelGGL(td_cnt_tiles<true>, dim3(grid), dim3(CNT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(td_cnt_tiles<false>, dim3(grid), dim3(CNT_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
