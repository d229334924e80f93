// Device helpers and launch constants the row layouts (td_rows.hip, td_pack.hip, td_windows.hip) and the document selection
// (td_select.hip) share: each of the four finds a slot's document in its own way, and all of them store, sum, scan, divide and
// raise errors the same way.  Device code only: the host library sees td_rows.h, td_pack.h, td_windows.h and td_select.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_common.h"

namespace td {

constexpr int RC_THREADS = 256;    // lanes of a workgroup, in every kernel of the three files
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

// the exclusive scan of `sum` over the workgroup's RC_THREADS lanes, and its total; s_wave: RC_THREADS / 64 words of LDS
__device__ __forceinline__ long long block_excl(long long sum, long long* s_wave, long long& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long incl = sum;
    for (int dd = 1; dd < 64; dd <<= 1) {
        const long long o = __shfl_up(incl, dd);
        if (lane >= dd) incl += o;
    }
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

}  // namespace td
