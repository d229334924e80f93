// Device helpers and launch constants the row layouts (td_rows.hip, td_pack.hip, td_windows.hip) and the document selection
// (td_select.hip) share: each of the four finds a slot's document through its own key, by the one tile locator here (workgroup
// search, LDS table, lane bisection), and all of them store, sum, scan, divide and raise errors the same way; td_labels.hip takes
// the wavefront scan.  Device code only: the host library sees td_rows.h, td_pack.h, td_windows.h and td_select.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_common.h"

namespace td {

constexpr int RC_THREADS = 256;    // lanes of a workgroup, in every kernel of the four files
constexpr int RC_TILE = 4096;      // output slots a workgroup writes per tile (four int4 stores a lane)
constexpr int RC_MAX_GRID = 2048;  // slot kernels stride over tiles with at most this many workgroups

// The pair form of a slot kernel (td_*_rows_labeled*): the kernel is instantiated for the arguments WITH the label stream (RowsLabArgs,
// PackLabArgs, WindowLabArgs: LabArgs, td_rows_lab.h), LAB = has_lab<A>.  A slot's source index is resolved once and moves both streams: ids -> out, lab.src -> lab.dst.
// The one-stream instantiation reads none of it and compiles to what the kernel was without it.

// The first error of a call wins.  A: RowsArgs or WindowArgs (err, err_pos in the handle's control block).
template <class A>
__device__ __forceinline__ void rows_raise(const A& a, int code, int64_t pos) {
    if (atomicCAS(a.err, 0, code) == 0) *a.err_pos = pos;
}

// ids[src] with 0 <= src < n_tokens checked: offsets that are not non-decreasing (CONCAT, PAD) raise here, and nothing outside
// the buffer is read; td_win_slots runs on checked offsets only, there this is a second fence, not a path.
template <class A>
__device__ __forceinline__ int32_t rows_load1(const A& a, int64_t src) {
    if (src >= 0 && src < a.n_tokens) return a.ids[src];
    rows_raise(a, TD_E_INVALID, src);
    return a.pad;
}

template <class A, class = void>
constexpr bool has_lab = false;
template <class A>
constexpr bool has_lab<A, decltype((void)A::lab)> = true;

// Both streams at src (checked once, like rows_load1): the id returned, the label into `lab`.
template <class A>
__device__ __forceinline__ int32_t rows_load1_pair(const A& a, int64_t src, int32_t& lab) {
    if (src >= 0 && src < a.n_tokens) {
        lab = a.lab.src[src];
        return a.ids[src];
    }
    rows_raise(a, TD_E_INVALID, src);
    lab = a.lab.pad;
    return a.pad;
}

// p[src .. src + 3] as four dwords: the sources sit at a per-document shift, misaligned three times out of four
__device__ __forceinline__ void rows_get4(const int32_t* p, int64_t src, int32_t v[4]) {
    p += src;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
}

// slots [j0, j0 + 4) below `end`; int4 when aligned (j0 is a multiple of 4)
__device__ __forceinline__ void rows_put4(int32_t* p, int64_t j0, int64_t end, const int32_t v[4]) {
    if (j0 + 4 <= end && (((uintptr_t)p) & 15) == 0) {
        *reinterpret_cast<int4*>(p + j0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        for (int q = 0; q < 4; ++q)
            if (j0 + q < end) p[j0 + q] = v[q];
    }
}

// the label slots, in the pair form only
template <class A>
__device__ __forceinline__ void lab_put4(const A& a, int64_t j0, int64_t end, const int32_t v[4]) {
    if constexpr (has_lab<A>) rows_put4(a.lab.dst, j0, end, v);
}

// x / d for 0 <= x < 2^63 by the multiplier the host computed, magic = floor((2^64 - 1) / d): the estimate is low by at most one
__device__ __forceinline__ int64_t div_magic(int64_t x, int64_t d, unsigned long long magic) {
    const unsigned long long D = (unsigned long long)d;
    unsigned long long q = __umul64hi((unsigned long long)x, magic);
    unsigned long long r = (unsigned long long)x - q * D;
    for (int f = 0; f < 2 && r >= D; ++f) { ++q; r -= D; }
    return (int64_t)q;
}

// The sum (the maximum, of values >= 0) over the workgroup's RC_THREADS lanes, in every lane; s_red: RC_THREADS / 64 words of LDS.
__device__ __forceinline__ long long block_sum(long long v, long long* s_red) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < RC_THREADS / 64; ++w) r += s_red[w];
    __syncthreads();
    return r;
}

__device__ __forceinline__ long long block_max(long long v, long long* s_red) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (long long)__shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < RC_THREADS / 64; ++w) r = max(r, s_red[w]);
    __syncthreads();
    return r;
}

// The inclusive scan of v over a wavefront's 64 lanes: lane l gets op(... op(op(v_0, v_1), v_2) ..., v_l); op(earlier, later), associative.
template <class T, class Op>
__device__ __forceinline__ T wave_incl_scan(T v, int lane, Op op) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}

// the exclusive scan of `sum` over the workgroup's RC_THREADS lanes, and its total; s_wave: RC_THREADS / 64 words of LDS
__device__ __forceinline__ long long block_excl(long long sum, long long* s_wave, long long& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long incl = wave_incl_scan(sum, lane, [](long long x, long long y) { return x + y; });
    __syncthreads();  // (the readers of an earlier call are done)
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int w = 0; w < RC_THREADS / 64; ++w) {
        if (w < wv) before += s_wave[w];
        total += s_wave[w];
    }
    return before + incl - sum;
}

// ---- finding an output slot's document ------------------------------------------------------------------------------------------
// Every slot kernel maps a tile of output slots back to the documents (segments, rows, kept entries) that fill it, through a
// non-decreasing key with a sentinel entry behind the last document: one workgroup search for the tile's first document, the
// keys of the tile's documents into LDS, one bisection a lane.  The keys are callables taken by value; everything inlines.

constexpr int RC_LDS_DOCS = 4352;    // keys of a tile's documents kept in LDS; more (runs of empty documents): the caller's fallback
constexpr int RC_SCAN_CHUNK = 1024;  // documents (entries) per workgroup of a count / chunks / first scan, four a lane
static_assert(RC_TILE == 16 * RC_THREADS && RC_SCAN_CHUNK == 4 * RC_THREADS, "four int4 stores, four scan entries a lane");
static_assert(RC_LDS_DOCS % RC_THREADS == 0, "tile_table fills whole steps of RC_THREADS entries");

// The last index in [lo, hi) whose key is <= x, given key(lo) <= x and key non-decreasing: RC_THREADS probes a step, by the whole
// workgroup.  lo, hi and the trip count are the same in every lane, so every lane reaches every barrier; lane 0's probe is lo
// itself (known), and no lane reads outside [lo, hi).
template <class Key>
__device__ __forceinline__ int64_t group_last_le(Key key, int64_t lo, int64_t hi, int64_t x) {
    const int tid = threadIdx.x;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + RC_THREADS - 1) / RC_THREADS;
        const int64_t q = lo + (int64_t)tid * step;
        const int c = __syncthreads_count(tid > 0 && q < hi && key(q) <= x);
        hi = hi < lo + (int64_t)(c + 1) * step ? hi : lo + (int64_t)(c + 1) * step;
        lo += (int64_t)c * step;
    }
    return lo;
}

// s_tab[i] = key(d0 + i) - origin clamped to [v_lo, v_hi] (behind d_last, the sentinel: v_hi), RC_THREADS entries a step, until
// a step holds an entry at or above `limit` (v_lo < limit <= v_hi).  Returns the entries below `limit`, n: s_tab[0, n] is
// valid, s_tab[n] the first at or above it.  fits: false when RC_LDS_DOCS entries held none, s_tab is then of no use.
// By the whole workgroup; the caller puts a barrier between the table's last readers and this call.
template <class Key>
__device__ __forceinline__ int tile_table(int32_t* s_tab, Key key, int64_t d0, int64_t d_last, int64_t origin, int32_t v_lo,
                                          int32_t v_hi, int32_t limit, bool& fits) {
    int n = 0;
    fits = false;
    // (kept rolled: with the 17 steps unrolled td_rows_concat<RowsArgs> compiles to 81 VGPRs and 5 waves a SIMD instead of 79 and 6)
#pragma unroll 1
    for (int c0 = 0; c0 < RC_LDS_DOCS; c0 += RC_THREADS) {
        const int64_t d = d0 + c0 + threadIdx.x;
        int32_t v = v_hi;
        if (d <= d_last) {
            const int64_t r = key(d) - origin;
            v = r < v_lo ? v_lo : r > v_hi ? v_hi : (int32_t)r;
        }
        s_tab[c0 + threadIdx.x] = v;
        const int c = __syncthreads_count(v < limit);
        n += c;
        if (c < RC_THREADS) {
            fits = true;
            break;
        }
    }
    return n;
}

// For a caller whose table always fits (it says why beside the call).
template <class Key>
__device__ __forceinline__ int tile_table(int32_t* s_tab, Key key, int64_t d0, int64_t d_last, int64_t origin, int32_t v_lo,
                                          int32_t v_hi, int32_t limit) {
    [[maybe_unused]] bool fits;
    return tile_table(s_tab, key, d0, d_last, origin, v_lo, v_hi, limit, fits);
}

// The last index in [0, n) with tab[i] <= x, given tab[0] <= x (n < 1: 0): a lane's own bisection, over an LDS table.  The index
// has the type of n (td_sel_slots counts its documents in 64 bits; compiled with a 32-bit index here it is allotted ten VGPRs more).
template <class T, class I>
__device__ __forceinline__ I last_le(const T* tab, I n, T x) {
    I lo = 0, hi = n;
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (tab[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same over [lo, hi) of a key in global memory.
template <class Key>
__device__ __forceinline__ int64_t last_le_global(Key key, int64_t lo, int64_t hi, int64_t x) {
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// N interleaved streams of chunk sums, cs[N * c + s] for c < nch, to their exclusive prefixes in place, by ONE workgroup: four
// chunks a lane, the carry across passes of 4 * RC_THREADS chunks.  carry[s]: stream s's total.  s_wave: as block_excl.
template <int N>
__device__ __forceinline__ void chunks_excl_scan(unsigned long long* cs, int64_t nch, long long* s_wave, long long (&carry)[N]) {
    const int tid = threadIdx.x;
    for (int s = 0; s < N; ++s) carry[s] = 0;
    for (int64_t base = 0; base < nch; base += 4 * RC_THREADS) {
        long long v[N][4], run[N];
        for (int s = 0; s < N; ++s) {
            long long sum = 0, total;
            for (int q = 0; q < 4; ++q) {
                const int64_t c = base + tid * 4 + q;
                v[s][q] = c < nch ? (long long)cs[N * c + s] : 0;
                sum += v[s][q];
            }
            run[s] = carry[s] + block_excl(sum, s_wave, total);
            carry[s] += total;
        }
        for (int q = 0; q < 4; ++q) {
            const int64_t c = base + tid * 4 + q;
            for (int s = 0; s < N; ++s) {
                if (c < nch) cs[N * c + s] = (unsigned long long)run[s];
                run[s] += v[s][q];
            }
        }
    }
}

}  // namespace td
