// Device pieces of the segmented scan of token lengths that td_offsets.hip (the starts written out) and td_ranges.hip (the starts
// kept in registers) share: the run, its operator, the wavefront scan and the lowest-index rule of a bad id.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_common.h"

namespace td {

struct Seg {  // a run of the segmented scan: f = a document starts inside it, s = sum since its last document start
    uint32_t f;
    unsigned long long s;
};
__device__ __forceinline__ Seg seg_op(Seg x, Seg y) { return Seg{x.f | y.f, y.f ? y.s : x.s + y.s}; }

// 64-lane inclusive segmented scan
__device__ __forceinline__ Seg wave_scan(Seg x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t f = __shfl_up(x.f, d);
        const unsigned long long s = __shfl_up(x.s, d);
        if (lane >= d) x = seg_op(Seg{f, s}, x);
    }
    return x;
}

// An id that is no token, at index i: the lowest index wins (as td_decode_len; absorb_ctl turns the maximum back).  A: err, err_pos.
template <class A>
__device__ __forceinline__ void off_bad_token(const A& a, int64_t i) {
    const int was = atomicCAS(a.err, 0, TD_E_BAD_TOKEN);
    if (was == 0 || was == TD_E_BAD_TOKEN)
        atomicMax(reinterpret_cast<unsigned long long*>(a.err_pos), (unsigned long long)(0x7FFFFFFFFFFFFFFFll - i));
}

// The byte length of an id, 0 for one outside the vocabulary.  A: len_off, max_id.
template <class A>
__device__ __forceinline__ uint32_t tok_len(const A& a, int32_t id) {
    return (id >= 0 && id <= a.max_id) ? a.len_off[id + 1] - a.len_off[id] : 0u;
}

}  // namespace td
