// The text rewrites (td_nfc.hip, td_utf8.hip): the frame both passes' kernels are wrappers of.  Device only.
//
// The text is cut into WINDOWS of 16 bytes at 16-byte aligned ADDRESSES (the base pointer need not be aligned: the first window is short),
// a lane a window, 256 windows a tile.  A call is
//   docs      a lane a document: the offsets checks.  The lowest bad document is kept in head; every later kernel returns when there is
//             one, the next one raises it: nothing is written then.
//   reset     the pass's own (td_nfc_clear, td_utf8_prepare)
//   tiles<0>  (the tile loop is td_rewrite_tiles_body.h, included inside the pass's kernel: see there why)
//             MEASURE: a window the pass's screen calls plain is its own bytes and is not walked, any other goes through the pass's lane
//             walk.  The tile's bytes go to tile_base[t]; the pass's per-document results and counts are made here.
//   scan      one workgroup: tile_base to its exclusive prefixes, counts[0], TD_E_CAPACITY, the offsets of the documents that start at
//             the text's end.
//   sums      the pass's own
//   tiles<1>  WRITE: the lanes measure once more (sizes only), a workgroup scan places them, then they write: a tile of windows the
//             screen calls fast is one cooperative copy with 16-byte stores, any other tile is written lane by lane.  A document's
//             output offset is written by the lane that has its first byte.
// Measure and write are two walks, not one with staging in LDS: an output tile is up to three times its input, the copied case (all of
// real text but a few places) walks nothing twice but sixteen bytes' worth of compares, and nothing is carried from tile to tile.
//
// A pass is a POLICY P of compile-time hooks, what really differs between the two:
//   Args, Stats                                              the kernels' arguments (RewriteArgs and more), a lane's sums (zero at first)
//   screen(a, b0, b, we, total, window, fast, plain)         an owned window: fast: a copy in WRITE; plain: not walked in MEASURE
//   lane<MODE>(a, b, we, total, ub, opos, st) -> bytes       the walk over the window [b, we)
//   plain_window(st)                                         MEASURE, a window that was not walked
//   flush(a, st, s_red)                                      MEASURE, the workgroup's end: the lanes' sums into counts
#pragma once
#include <type_traits>

#include "td_rewrite_args.h"
#include "td_rows_common.h"

namespace td {

static_assert(RW_THREADS == RC_THREADS && RW_TILE == RC_TILE, "the row kernels' launch shape");
constexpr int RW_MAX_GRID = 1 << 20;
constexpr int32_t RW_OFF_LO = -8, RW_OFF_HI = RW_TILE + 8;
constexpr long long RW_BAD_TOP = 1ll << 62;

// gid, step: the lane's place in the grid and the grid's lanes, taken in the kernel itself (blockDim is one load only there)
__device__ __forceinline__ void rewrite_docs(const RewriteArgs& a, int64_t gid, int64_t step) {
    if (gid == 0 && a.doc_off[0] != 0) atomicMax(&a.head[RW_H_BAD], (unsigned long long)RW_BAD_TOP);
    for (int64_t d = gid; d < a.n_docs; d += step) {
        const int64_t lo = a.doc_off[d], hi = a.doc_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_bytes) atomicMax(&a.head[RW_H_BAD], (unsigned long long)(RW_BAD_TOP - d));
    }
}

// (for the kernels that come first behind the reset in a call)
__device__ __forceinline__ bool rewrite_bad_offsets(const RewriteArgs& a, bool raise) {
    const unsigned long long bad = a.head[RW_H_BAD];
    if (!bad) return false;
    if (raise && blockIdx.x == 0 && threadIdx.x == 0) rows_raise(a, TD_E_INVALID, (int64_t)(RW_BAD_TOP - (long long)bad));
    return true;
}

// dst[0, len) = src[0, len) by the whole workgroup: 16-byte stores at 16-byte aligned addresses of dst, the source as it lies
__device__ __forceinline__ void rewrite_group_copy(uint8_t* dst, const uint8_t* src, int64_t len) {
    const int tid = threadIdx.x;
    int64_t head = (int64_t)((16 - (((uintptr_t)dst) & 15)) & 15);
    head = head < len ? head : len;
    const int64_t n16 = (len - head) >> 4;
    if (tid < head) dst[tid] = src[tid];
    for (int64_t k = tid; k < n16; k += RW_THREADS) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * k, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
    }
    const int64_t tail = head + 16 * n16;
    if (tail + tid < len) dst[tail + tid] = src[tail + tid];
}

__device__ __forceinline__ void rewrite_scan(const RewriteArgs& a) {
    __shared__ long long s_wave[RW_THREADS / 64];
    if (a.head[RW_H_BAD]) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    long long carry[1];
    chunks_excl_scan<1>(a.tile_base, ntiles, s_wave, carry);
    const int64_t need = carry[0];
    if (threadIdx.x == 0) {
        a.counts[RW_C_BYTES] = (unsigned long long)need;
        if (need > a.out_capacity) {
            a.head[RW_H_FULL] = 1;
            rows_raise(a, TD_E_CAPACITY, need);
        }
    }
    if (need > a.out_capacity) return;
    // the documents that start at the text's end (the entry behind the last one among them): no window holds them
    for (int64_t d = a.n_docs - threadIdx.x; d >= 0 && a.doc_off[d] == total; d -= RW_THREADS) a.out_doc_off[d] = need;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------------
inline unsigned rewrite_grid(int64_t n, int64_t per, int64_t most) {
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g < most ? g : most);
}

template <class A>
hipError_t rewrite_launch(void (*kernel)(A), unsigned grid, const A& a, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(RW_THREADS), 0, stream, a);
    return hipGetLastError();
}

// the start of either sequence: docs, then reset
template <class A>
hipError_t rewrite_launch_start(const A& a, hipStream_t stream, void (*docs)(A), void (*reset)(A)) {
    const hipError_t e = rewrite_launch(docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream);
    return e != hipSuccess ? e : rewrite_launch(reset, rewrite_grid(a.n_docs + RW_C_WORDS, RW_THREADS, 4096), a, stream);
}

template <class A>
hipError_t rewrite_launch_check(const A& a, hipStream_t stream, void (*docs)(A), void (*reset)(A), void (*check)(A), void (*sums)(A)) {
    hipError_t e;
    if ((e = rewrite_launch_start(a, stream, docs, reset)) != hipSuccess) return e;
    // four windows a lane, and at most 2048 workgroups (eight a CU) that stride over the rest
    if ((e = rewrite_launch(check, rewrite_grid(a.n_bytes + 16, 4 * RW_TILE, 2048), a, stream)) != hipSuccess) return e;
    return rewrite_launch(sums, rewrite_grid(a.n_docs, RW_THREADS, 4096), a, stream);
}

template <class A>
hipError_t rewrite_launch_phases(const A& a, hipStream_t stream, int phases, void (*docs)(A), void (*reset)(A), void (*measure)(A),
                                 void (*scan)(A), void (*sums)(A), void (*write)(A)) {
    hipError_t e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if (phases & RW_RUN_MEASURE) {
        if ((e = rewrite_launch_start(a, stream, docs, reset)) != hipSuccess) return e;
        if ((e = rewrite_launch(measure, tiles, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(scan, 1, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(sums, rewrite_grid(a.n_docs, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    }
    return phases & RW_RUN_WRITE ? rewrite_launch(write, tiles, a, stream) : hipGetLastError();
}

}  // namespace td
