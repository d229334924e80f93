// Unicode NFC normalisation (td_nfc_check_device, td_nfc_device and what ends in them): text + document offsets -> flags[d] (0: proven
// NFC) at read speed, and the normalised text + its document offsets.  The rule is the contract in include/tokendagger_hip.h;
// td_nfc_args.h has the lookup, the decoder, the quick check, the segment scan and the segment normaliser, which the host statement
// (td_nfc_host) and the CPU model compile too.  The tables (generated/unicode_nfc.inc, 55 KiB) are __device__ constants here: they are
// touched only behind a lead byte >= 0xCC and are left to L2, LDS holds none of them.
//
// The windows, the tiles, the kernels of a call and their order are the rewrites' frame (td_rewrite_common.h); this file has the pass:
//   td_nfc_clear    (the reset) flags, changed and counts to zero
//   td_nfc_check    grid-stride over windows, four loads in flight a lane.  A window none of whose bytes reaches 0xCC holds boundaries
//                   only and is proven by four integer operations a dword.  A byte >= 0xCC is decoded inside its document (found by
//                   bisection); a code point that is not Quick_Check Yes, or a non-starter below the ccc of the unit in front
//                   of it (decoded backwards: a unit is fixed by three bytes of context, so lane, step and workgroup seams do not matter),
//                   flags its document.
//   NfcPolicy       the screen: a window of bytes below 0xCC, begun and followed by a byte that is no continuation byte, is a copy.  The
//                   walk: a lane OWNS the segments that start in its window and walks each to its end, beyond the window too; a lane
//                   whose window holds no boundary owns nothing and looks no further than its window.  Proven segments count their
//                   length, the others go through the normaliser with a sink that only counts and compares.  A window of ASCII is not
//                   walked (sixteen segments of one code point); one of bytes below 0xCC is, for its opaque bytes.
//   td_nfc_sums     a lane a document: counts[1] and counts[2] from flags and changed
//
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read, nothing outside the outputs is written.
#include <hip/hip_runtime.h>

#include "td_nfc.h"
#include "td_rewrite_common.h"

namespace td {

namespace {

#define TD_NFC_TABLE(type, name, n) __device__ const type name[n]
#include "generated/unicode_nfc.inc"
#undef TD_NFC_TABLE

__device__ __forceinline__ NfcTables nfc_tables() {
    return NfcTables{td_nfc_stage1, td_nfc_stage2, td_nfc_dec_key, td_nfc_dec_off, td_nfc_dec_cps, td_nfc_pair_a, td_nfc_pair_b, td_nfc_pair_c};
}

__device__ __forceinline__ void nfc_add(unsigned long long* p, unsigned long long n) {
    __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the bytes of a dword at or above 0xCC, as their top bits
__device__ __forceinline__ uint32_t nfc_hits(uint32_t w) { return ((w & 0x7F7F7F7Fu) + 0x34343434u) & w & 0x80808080u; }
__device__ __forceinline__ uint32_t nfc_hits(uint4 v) { return nfc_hits(v.x) | nfc_hits(v.y) | nfc_hits(v.z) | nfc_hits(v.w); }

__global__ __launch_bounds__(RW_THREADS) void td_nfc_docs(const NfcArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_nfc_clear(const NfcArgs a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid < RW_C_WORDS) a.counts[gid] = 0;
    for (int64_t d = gid; d < a.n_docs; d += step) {
        a.flags[d] = 0;
        if (a.changed) a.changed[d] = 0;
    }
}

// ---- the check ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RW_THREADS) void td_nfc_check(const NfcArgs a) {
    if (rewrite_bad_offsets(a, true)) return;
    const NfcTables T = nfc_tables();
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t nwin = (total + shift + 15) >> 4, step = (int64_t)gridDim.x * blockDim.x;
    int64_t D = -1, ds = 0, de = 0;
    const auto slow = [&](int64_t g) {
        const int64_t b = g * 16 - shift;
        nfc_check_window(a, T, b < 0 ? 0 : b, b + 16 < total ? b + 16 : total, D, ds, de,
                         [&](int64_t p) { return last_le_global([off = a.doc_off](int64_t d) { return off[d]; }, 0, a.n_docs, p); });
    };
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // four windows a step while all four lie inside the text (g >= 1: the first window may begin in front of it)
    for (; g >= 1 && (g + 3 * step) * 16 - shift + 16 <= total; g += 4 * step) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint4*>(a.text + ((g + q * step) * 16 - shift));
        if ((nfc_hits(v[0]) | nfc_hits(v[1]) | nfc_hits(v[2]) | nfc_hits(v[3])) == 0) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (nfc_hits(v[q])) slow(g + q * step);
    }
    for (; g < nwin; g += step) {
        const int64_t b = g * 16 - shift;
        if (b >= 0 && b + 16 <= total && nfc_hits(*reinterpret_cast<const uint4*>(a.text + b)) == 0) continue;
        slow(g);
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_nfc_sums(const NfcArgs a) {
    __shared__ long long s_red[RW_THREADS / 64];
    if (a.head[RW_H_BAD]) return;
    long long unproven = 0, changed = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        unproven += a.flags[d] != 0;
        if (a.changed) changed += a.changed[d] != 0;
    }
    unproven = block_sum(unproven, s_red);
    changed = block_sum(changed, s_red);
    if (threadIdx.x == 0) {
        if (unproven) nfc_add(a.counts + NFC_C_UNPROVEN, (unsigned long long)unproven);
        if (changed) nfc_add(a.counts + NFC_C_CHANGED, (unsigned long long)changed);
    }
}

// ---- the normaliser -------------------------------------------------------------------------------------------------------------------
struct NfcPolicy {
    using Args = NfcArgs;
    using Stats = NfcLaneStats;
    // a window of bytes below 0xCC, begun and followed by a byte that is no continuation byte: boundaries only, a copy
    // (PLAIN: ASCII alone, sixteen code points and no opaque byte; a fast window with a byte from 0x80 on is still a copy, but MEASURE
    // walks it for counts[5] and counts[6]: which of its bytes are opaque depends on the documents' ends too)
    static __device__ __forceinline__ void screen(const NfcArgs& a, int64_t b0, int64_t b, int64_t we, int64_t total, int64_t, bool& fast, bool& plain) {
        if (b0 < 0 || b0 + 16 > total) return;
        const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
        if (nfc_hits(v) == 0 && (a.text[b] & 0xC0) != 0x80) {
            fast = we == total || ((a.text[we] & 0xC0) != 0x80 && a.text[we] < NFC_LEAD_MIN);
            plain = fast && ((v.x | v.y | v.z | v.w) & 0x80808080u) == 0;
        }
    }
    template <int MODE, class Ub>
    static __device__ __forceinline__ int64_t lane(const NfcArgs& a, int64_t b, int64_t we, int64_t total, Ub ub, int64_t opos, NfcLaneStats& st) {
        return nfc_lane<MODE>(a, nfc_tables(), b, we, total, ub, opos, st);
    }
    static __device__ __forceinline__ void plain_window(NfcLaneStats& st) { st.longest = st.longest > 1 ? st.longest : 1; }
    static __device__ __forceinline__ void flush(const NfcArgs& a, const NfcLaneStats& st, long long* s_red) {
        const long long seg = block_sum(st.segments, s_red), cps = block_sum(st.cps, s_red), opq = block_sum(st.opaque, s_red);
        const long long lng = block_max(st.longest, s_red);
        if (threadIdx.x == 0) {
            if (seg) nfc_add(a.counts + NFC_C_SEGMENTS, (unsigned long long)seg);
            if (cps) nfc_add(a.counts + NFC_C_CPS, (unsigned long long)cps);
            if (opq) nfc_add(a.counts + NFC_C_OPAQUE, (unsigned long long)opq);
            if (lng) atomicMax(a.counts + NFC_C_LONGEST, (unsigned long long)lng);
        }
    }
};

template <int WRITE>
__global__ __launch_bounds__(RW_THREADS) void td_nfc_tiles(const NfcArgs a) {
    using P = NfcPolicy;
#include "td_rewrite_tiles_body.h"
}

__global__ __launch_bounds__(RW_THREADS) void td_nfc_scan(const NfcArgs a) { rewrite_scan(a); }

}  // namespace

hipError_t launch_nfc_check(const NfcArgs& a, hipStream_t stream) {
    return rewrite_launch_check(a, stream, td_nfc_docs, td_nfc_clear, td_nfc_check, td_nfc_sums);
}

hipError_t launch_nfc(const NfcArgs& a, hipStream_t stream, int phases) {
    return rewrite_launch_phases(a, stream, phases, td_nfc_docs, td_nfc_clear, td_nfc_tiles<0>, td_nfc_scan, td_nfc_sums, td_nfc_tiles<1>);
}

}  // namespace td
