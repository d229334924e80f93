// UTF-8 validation and repair (td_utf8_check_device, td_utf8_device and what ends in them): text + document offsets -> flags[d] (0:
// well-formed), first_bad[d], n_bad[d], and the repaired text + its document offsets.  The rule is the contract in
// include/tokendagger_hip.h; td_utf8_args.h has the unit rule, the window screen and the lane walk, which the host statement
// (td_utf8_host) and the CPU model compile too.  No table: everything is compares on bytes.
//
// The windows, the tiles, the kernels of a call and their order are the rewrites' frame (td_rewrite_common.h); this file has the pass.
// Two facts keep the documents off the fast path:
//   - a unit is fixed by three bytes in front of it and three behind it, so a unit at least three bytes away from both ends of its
//     document is what it would be were the whole text one document;
//   - the window screen (u8_window_suspect: SWAR over the window's four dwords, the dword in front and the dword behind, in registers)
//     is never set on well-formed text and always set where a byte of the window belongs to an ill-formed subpart of the text.
// So a lane a document looks at its document's first byte and at the byte behind its last: only where one of them is a continuation
// byte can the document's rule differ from the text's, and then the units within three bytes of the document's ends are taken by the
// document's rule (at most six).  A window finds its documents only when the screen is set.  A window with no byte >= 0x80 is skipped
// after four ORs.
//
//   td_utf8_prepare  (the reset) a lane a document: flags 0, first_bad -1, n_bad 0, counts 0, then the document's edges.  The check
//                    reports them at once (flags, first_bad: its own document's entries); the repair marks the windows that hold their
//                    bytes in `dirty`.
//   td_utf8_check    grid-stride over windows, four loads in flight a lane; a window the screen sets is walked by the document's rule
//                    (its documents by bisection): flags (a store) and first_bad (a minimum) are idempotent, so both paths may report.
//   U8Policy         the screen: a window that is neither suspect nor dirty is a copy and is not walked; windows at the text's ends are
//                    walked.  The walk: a lane has the BYTES of its window: a byte of a well-formed unit is a byte of output, the first
//                    byte of a subpart three bytes or none.  flags, first_bad, n_bad, counts[2] and counts[3] are made in MEASURE alone,
//                    by the lane that has the subpart's first byte.
//   td_utf8_sums     a lane a document: counts[1] from flags; for the repair counts[4] and counts[5] from the documents' first and last units
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read, nothing outside the outputs is written.  Sums, minima and
// stores of 1 only: the results do not depend on the order of the lanes.
#include <hip/hip_runtime.h>

#include "td_rewrite_common.h"
#include "td_utf8.h"

namespace td {

namespace {

struct U8Add {
    __device__ __forceinline__ void operator()(unsigned long long* p, unsigned long long n) const {
        __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct U8Lower {
    __device__ __forceinline__ void operator()(unsigned long long* p, unsigned long long v) const {
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__device__ __forceinline__ bool u8_ascii(uint4 v) { return ((v.x | v.y | v.z | v.w) & U8_H) == 0; }

// the screen of the window v at text + b, which has four bytes of the text in front of it and four behind it
__device__ __forceinline__ bool u8_suspect_at(const uint8_t* text, int64_t b, uint4 v) {
    const uint32_t s[6] = {*reinterpret_cast<const uint32_t*>(text + b - 4), v.x, v.y, v.z, v.w, *reinterpret_cast<const uint32_t*>(text + b + 16)};
    return u8_window_suspect(s);
}

__global__ __launch_bounds__(RW_THREADS) void td_utf8_docs(const U8Args a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_utf8_prepare(const U8Args a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t total = a.doc_off[a.n_docs];
    if (gid < RW_C_WORDS) a.counts[gid] = 0;
    for (int64_t d = gid; d < a.n_docs; d += step) {
        const int64_t ds = a.doc_off[d], de = a.doc_off[d + 1];
        unsigned long long first = ~0ull;
        bool ill = false;
        u8_doc_edges(a.text, ds, de, total, [&](int64_t p, int len) {
            if (a.dirty) {  // (the repair: the measure pass reports, each subpart by the one lane that has its first byte)
                a.dirty[u8_window_of(p, shift)] = 1;
                a.dirty[u8_window_of(p + len - 1, shift)] = 1;
            } else {
                ill = true;
                first = first < (unsigned long long)(p - ds) ? first : (unsigned long long)(p - ds);
            }
        });
        a.flags[d] = ill;
        if (a.first_bad) a.first_bad[d] = first;
        if (a.n_bad) a.n_bad[d] = 0;
    }
}

// ---- the check ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RW_THREADS) void td_utf8_check(const U8Args a) {
    if (rewrite_bad_offsets(a, true)) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t nwin = u8_windows(total, shift), step = (int64_t)gridDim.x * blockDim.x;
    int64_t D = -1, ds = 0, de = 0;
    const auto slow = [&](int64_t g) {
        const int64_t b = g * 16 - shift;
        u8_check_window(a, b < 0 ? 0 : b, b + 16 < total ? b + 16 : total, D, ds, de,
                        [&](int64_t p) { return last_le_global([off = a.doc_off](int64_t d) { return off[d]; }, 0, a.n_docs, p); }, U8Lower{});
    };
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // four windows a step while all four have four bytes of the text in front of them and four behind them
    for (; g * 16 - shift >= 4 && (g + 3 * step) * 16 - shift + 20 <= total; g += 4 * step) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint4*>(a.text + ((g + q * step) * 16 - shift));
        if (((v[0].x | v[0].y | v[0].z | v[0].w | v[1].x | v[1].y | v[1].z | v[1].w | v[2].x | v[2].y | v[2].z | v[2].w | v[3].x | v[3].y | v[3].z |
              v[3].w) & U8_H) == 0)
            continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!u8_ascii(v[q]) && u8_suspect_at(a.text, (g + q * step) * 16 - shift, v[q])) slow(g + q * step);
    }
    for (; g < nwin; g += step) {
        const int64_t b = g * 16 - shift;
        if (b >= 4 && b + 20 <= total) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
            if (u8_ascii(v) || !u8_suspect_at(a.text, b, v)) continue;
        }
        slow(g);
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_utf8_sums(const U8Args a) {
    __shared__ long long s_red[RW_THREADS / 64];
    if (a.head[RW_H_BAD]) return;
    const bool repair = a.dirty != nullptr;
    long long ill = 0, begins = 0, ends = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        ill += a.flags[d] != 0;
        const int64_t ds = a.doc_off[d], de = a.doc_off[d + 1];
        if (repair && ds < de) {
            begins += u8_is_cont(a.text[ds]);
            ends += u8_ends_cut(a.text, ds, de);
        }
    }
    ill = block_sum(ill, s_red);
    begins = block_sum(begins, s_red);
    ends = block_sum(ends, s_red);
    if (threadIdx.x == 0) {
        if (ill) U8Add{}(a.counts + U8_C_DOCS, (unsigned long long)ill);
        if (begins) U8Add{}(a.counts + U8_C_BEGIN_CONT, (unsigned long long)begins);
        if (ends) U8Add{}(a.counts + U8_C_END_LEAD, (unsigned long long)ends);
    }
}

// ---- the repair -----------------------------------------------------------------------------------------------------------------------
struct U8Policy {
    using Args = U8Args;
    using Stats = U8LaneStats;
    // a window none of whose bytes belongs to an ill-formed subpart: a copy, walked in neither phase.  Windows at the text's ends are walked.
    static __device__ __forceinline__ void screen(const U8Args& a, int64_t b0, int64_t b, int64_t, int64_t total, int64_t window, bool& fast, bool& plain) {
        if (b0 < 4 || b0 + 20 > total) return;
        const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
        plain = fast = u8_ascii(v) || (!u8_suspect_at(a.text, b, v) && !a.dirty[window]);
    }
    template <int MODE, class Ub>
    static __device__ __forceinline__ int64_t lane(const U8Args& a, int64_t b, int64_t we, int64_t, Ub ub, int64_t opos, U8LaneStats& st) {
        return u8_lane<MODE>(a, b, we, ub, opos, st, U8Add{}, U8Lower{});
    }
    static __device__ __forceinline__ void plain_window(U8LaneStats&) {}
    static __device__ __forceinline__ void flush(const U8Args& a, const U8LaneStats& st, long long* s_red) {
        const long long sub = block_sum(st.subparts, s_red), byt = block_sum(st.sub_bytes, s_red);
        if (threadIdx.x == 0) {
            if (sub) U8Add{}(a.counts + U8_C_SUBPARTS, (unsigned long long)sub);
            if (byt) U8Add{}(a.counts + U8_C_SUB_BYTES, (unsigned long long)byt);
        }
    }
};

template <int WRITE>
__global__ __launch_bounds__(RW_THREADS) void td_utf8_tiles(const U8Args a) {
    using P = U8Policy;
#include "td_rewrite_tiles_body.h"
}

__global__ __launch_bounds__(RW_THREADS) void td_utf8_scan(const U8Args a) { rewrite_scan(a); }

}  // namespace

hipError_t launch_utf8_check(const U8Args& a, hipStream_t stream) {
    return rewrite_launch_check(a, stream, td_utf8_docs, td_utf8_prepare, td_utf8_check, td_utf8_sums);
}

hipError_t launch_utf8(const U8Args& a, hipStream_t stream, int phases) {
    return rewrite_launch_phases(a, stream, phases, td_utf8_docs, td_utf8_prepare, td_utf8_tiles<0>, td_utf8_scan, td_utf8_sums, td_utf8_tiles<1>);
}

}  // namespace td
