// The segmented scan of td_repetition.hip's units, for the kernels that share it (td_repetition.hip, td_wordgrams.hip): the scan of RpElem
// over a workgroup's lanes, the tiles of a call, the one-workgroup prefix over the tiles' elements with the capacity check, and the
// comparison of two byte ranges.  Device only; moved here from td_repetition.hip unchanged.
#pragma once
#include "td_repetition_args.h"
#include "td_rewrite_common.h"

namespace td {

namespace {

constexpr int RP_WAVES = RW_THREADS / 64;

__device__ __forceinline__ RpElem rp_shfl_up(const RpElem& e, int d) {
    return RpElem{(int64_t)__shfl_up((long long)e.s, d), (uint64_t)__shfl_up((unsigned long long)e.h, d),
                  (uint64_t)__shfl_up((unsigned long long)e.pw, d), (uint64_t)__shfl_up((unsigned long long)e.c, d)};
}

// e[kind] of the workgroup's lanes, in lane order, to what the lanes in front of each combine to (the identity in front of the first);
// all[kind]: all of them combined.  s_wave: 2 * RP_WAVES elements of LDS.
__device__ __forceinline__ void rp_block_excl(RpElem (&e)[2], RpElem* s_wave, RpElem (&all)[2]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    RpElem incl[2];
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
        RpElem v = e[kind];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const RpElem o = rp_shfl_up(v, d);
            if (lane >= d) v = rp_combine(o, v);
        }
        incl[kind] = v;
    }
    __syncthreads();  // (the readers of an earlier call are done)
    if (lane == 63) {
        s_wave[2 * wv] = incl[0];
        s_wave[2 * wv + 1] = incl[1];
    }
    __syncthreads();
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
        RpElem before = rp_identity();
        all[kind] = rp_identity();
        for (int x = 0; x < RP_WAVES; ++x) {
            const RpElem sw = s_wave[2 * x + kind];
            if (x < wv) before = rp_combine(before, sw);
            all[kind] = rp_combine(all[kind], sw);
        }
        const RpElem up = rp_shfl_up(incl[kind], 1);
        e[kind] = lane > 0 ? rp_combine(before, up) : before;
    }
}

__device__ __forceinline__ int64_t rp_tiles(const RpArgs& a, int64_t& total, int& shift) {
    total = a.doc_off[a.n_docs];
    shift = (int)(((uintptr_t)a.text) & 15);
    return total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
}

__global__ __launch_bounds__(RW_THREADS) void td_rp_prefix(const RpArgs a) {
    __shared__ RpElem s_wave[2 * RP_WAVES];
    if (a.head[RW_H_BAD]) return;
    int64_t total;
    int shift;
    const int64_t ntiles = rp_tiles(a, total, shift);
    const int64_t per = (ntiles + RW_THREADS - 1) / RW_THREADS;
    const int64_t t0 = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    RpElem T[2] = {rp_identity(), rp_identity()}, all[2];
#pragma unroll 4
    for (int64_t t = t0; t < t1; ++t) {
        T[0] = rp_combine(T[0], a.carry[2 * t]);
        T[1] = rp_combine(T[1], a.carry[2 * t + 1]);
    }
    rp_block_excl(T, s_wave, all);
#pragma unroll 4
    for (int64_t t = t0; t < t1; ++t) {
        a.carry[2 * t] = T[0] = rp_combine(T[0], a.carry[2 * t]);
        a.carry[2 * t + 1] = T[1] = rp_combine(T[1], a.carry[2 * t + 1]);
    }
    if (threadIdx.x == 0) {
        const long long need = (long long)a.head[RP_H_UNITS];
        if (need > a.max_units) {
            a.head[RW_H_FULL] = 1;
            rows_raise(a, TD_E_CAPACITY, need);
        } else {
            a.head[RP_H_MASK] = rp_slots(need) - 1;
        }
    }
}

__device__ __forceinline__ bool rp_equal(const uint8_t* x, const uint8_t* y, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t u, v;
        __builtin_memcpy(&u, x + i, 8);
        __builtin_memcpy(&v, y + i, 8);
        if (u != v) return false;
    }
    for (; i < n; ++i)
        if (x[i] != y[i]) return false;
    return true;
}

}  // namespace

}  // namespace td
