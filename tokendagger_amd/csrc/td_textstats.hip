// Per-document text statistics (td_text_stats_device and what ends in it): text + document offsets -> stats[n_docs][TS_COLS] and
// totals[TS_COLS].  The rule is the contract in include/tokendagger_hip.h; td_textstats_args.h has the rule of one byte, a window's
// classes and its walk, which the host statement (td_text_stats_host) and the CPU model compile too.
//
// The windows, the tiles, the offsets check and the tile's table of documents are the text passes' frame (td_rewrite_common.h,
// td_rows_common.h); this pass only reads the text.  A call is
//   td_ts_docs     the frame's offsets check
//   td_ts_reset    a lane an entry of stats: 0, BYTES under TS_LOCAL; totals 0
//   td_ts_carry    (TS_RUNS) a workgroup a tile: the tile's last LF, space byte, visible byte and letter byte, or -1, into carry[t]
//   td_ts_prefix   (TS_RUNS) ONE workgroup: carry to its inclusive prefix maxima over the tiles (the maximum counterpart of
//                  chunks_excl_scan: a tile a lane, the carry across sweeps of RW_THREADS tiles)
//   td_ts_tiles<G> a workgroup a tile: the lanes take their windows' classes, scan the four last positions across the workgroup behind
//                  carry[t - 1] (TS_RUNS), and walk.  A lane keeps the sums of the document it is in; at its window's end a wavefront
//                  whose lanes are all in one document reduces them by shuffles; what is left goes to a table in LDS (the tile's first
//                  TS_SLOTS documents), and from there, or at once for later documents, to stats by 64-bit adds and maxima.
//   td_ts_totals   a lane a document: the columns' sums and maxima into totals
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores (td_ts_reset), adds and maxima touch the outputs:
// the results do not depend on the order of the lanes.  A window with no byte >= 0x80 takes its classes from ascii_cls in LDS, without
// the UTF-8 decode and without its documents.
#include <hip/hip_runtime.h>

#include "td_rewrite_common.h"
#include "td_textstats.h"

namespace td {

namespace {

constexpr int TS_SLOTS = 32;  // documents of a tile whose sums meet in LDS

__device__ __forceinline__ void ts_global(unsigned long long* p, int c, unsigned long long v) {
    if (ts_is_max(c)) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the window at b0 into w: one 16-byte load where it lies in the text, byte by byte at the text's ends
__device__ __forceinline__ void ts_load(const uint8_t* text, int64_t b0, int64_t b, int64_t we, uint32_t w[4]) {
    if (b == b0 && we == b0 + 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + b0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (b0 + k >= b && b0 + k < we) w[k >> 2] |= (uint32_t)text[b0 + k] << (8 * (k & 3));
}

struct TsTile {  // a tile's place in the text
    int64_t base, t0, s1;  // 16-byte aligned start (may lie in front of the text), first and end byte
};
__device__ __forceinline__ TsTile ts_tile(int64_t t, int shift, int64_t total) {
    TsTile r;
    r.base = t * RW_TILE - shift;
    r.t0 = r.base < 0 ? 0 : r.base;
    r.s1 = r.base + RW_TILE < total ? r.base + RW_TILE : total;
    return r;
}

__global__ __launch_bounds__(RW_THREADS) void td_ts_docs(const TsArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_ts_reset(const TsArgs a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.totals && gid < TS_COLS) a.totals[gid] = 0;
    for (int64_t i = gid; i < a.n_docs * TS_COLS; i += step) {
        const int64_t d = i / TS_COLS;
        a.stats[i] = (a.groups & TS_LOCAL) && i - d * TS_COLS == TS_BYTES ? (unsigned long long)(a.doc_off[d + 1] - a.doc_off[d]) : 0ull;
    }
}

// The tile's table of documents, as the rewrites' tile loop builds it: kb the last document that starts in front of t0 (t0 == 0: the
// first), s_off[i] = doc_off[kb + i] - t0 clamped; lds: the table fits.  By the whole workgroup, between two barriers of the caller.
struct TsTable {
    int64_t kb, nk;
    bool lds;
};
template <class Off>
__device__ __forceinline__ TsTable ts_table(int32_t* s_off, Off off_of, int64_t n_docs, const TsTile& tl) {
    TsTable r;
    r.lds = true;
    r.kb = tl.t0 > 0 ? group_last_le(off_of, 0, n_docs, tl.t0 - 1) : 0;
    r.nk = tile_table(s_off, off_of, r.kb, n_docs, tl.t0, RW_OFF_LO, RW_OFF_HI, (int32_t)(tl.s1 - tl.t0), r.lds);
    if (!r.lds) r.nk = group_last_le(off_of, r.kb, n_docs, tl.s1 - 1) - r.kb + 1;
    return r;
}
// the document that holds byte x of the tile (t0 <= x < s1): the last one of the table that starts at or below x
__device__ __forceinline__ int64_t ts_doc_of(const TsArgs& a, const int32_t* s_off, const TsTable& tb, int64_t t0, int64_t x) {
    int64_t lo = 0, hi = tb.nk;  // the first entry of [0, nk] behind x lies in [lo, hi]
    const int64_t r = x - t0;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t rel = tb.lds ? (int64_t)s_off[mid] : a.doc_off[tb.kb + mid] - t0;
        if (rel > r) hi = mid;
        else lo = mid + 1;
    }
    return tb.kb + lo - 1;
}

// ---- TS_RUNS: the tiles' last positions, and their prefix maxima ------------------------------------------------------------------------
__global__ __launch_bounds__(RW_THREADS) void td_ts_carry(const TsArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ long long s_red[RW_THREADS / 64];
    __shared__ uint8_t s_ascii[128];
    if (a.head[RW_H_BAD]) return;
    const int tid = threadIdx.x;
    if (tid < 128) s_ascii[tid] = a.ascii_cls[tid];
    const Tables T = ts_tables(a.ascii_cls, a.ucls1, a.ucls2);
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TsTile tl = ts_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        uint32_t w[4] = {0, 0, 0, 0}, c[4];
        if (owns) ts_load(a.text, b0, b, we, w);
        const bool need = owns && !ts_window_ascii(w);
        TsTable tb = {0, 0, true};
        __syncthreads();  // (the tile before has read its table; s_ascii is written)
        if (__syncthreads_or(need)) {
            tb = ts_table(s_off, off_of, a.n_docs, tl);
            __syncthreads();
        }
        TsLane S = {-1, -1, -1, -1, false};
        if (owns) {
            TsCursor cur = {0, 0, 0};
            if (need) {
                cur.D = ts_doc_of(a, s_off, tb, tl.t0, b);
                cur.ds = a.doc_off[cur.D];
                cur.de = a.doc_off[cur.D + 1];
            }
            ts_window_classes(T, s_ascii, a.text, a.doc_off, b0, b, we, w, cur, c, S);
        }
        // (block_max is over values >= 0: a position as its distance from the tile's base + 1, 0: none)
        const long long lf = block_max(S.lf < 0 ? 0 : S.lf - tl.base + 1, s_red), sp = block_max(S.sp < 0 ? 0 : S.sp - tl.base + 1, s_red);
        const long long vis = block_max(S.vis < 0 ? 0 : S.vis - tl.base + 1, s_red), let = block_max(S.let < 0 ? 0 : S.let - tl.base + 1, s_red);
        if (tid == 0) {
            a.carry[4 * t + 0] = lf ? tl.base + lf - 1 : -1;
            a.carry[4 * t + 1] = sp ? tl.base + sp - 1 : -1;
            a.carry[4 * t + 2] = vis ? tl.base + vis - 1 : -1;
            a.carry[4 * t + 3] = let ? tl.base + let - 1 : -1;
        }
    }
}

// the exclusive maximum scan of v[0 .. 3] (each >= -1) over the workgroup's lanes, -1 in front of the first; all[k]: the maximum over all of them.
// s_wave: 4 * RW_THREADS / 64 words of LDS.
__device__ __forceinline__ void ts_block_excl_max(long long (&v)[4], long long* s_wave, long long (&all)[4]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long incl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) incl[k] = wave_incl_scan(v[k], lane, [](long long x, long long y) { return x > y ? x : y; });
    __syncthreads();  // (the readers of an earlier call are done)
    if (lane == 63)
        for (int k = 0; k < 4; ++k) s_wave[4 * wv + k] = incl[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long before = -1;
        all[k] = -1;
        for (int x = 0; x < RW_THREADS / 64; ++x) {
            const long long sw = s_wave[4 * x + k];
            if (x < wv) before = before > sw ? before : sw;
            all[k] = all[k] > sw ? all[k] : sw;
        }
        const long long up = __shfl_up(incl[k], 1);
        v[k] = lane > 0 && up > before ? up : before;
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_ts_prefix(const TsArgs a) {
    __shared__ long long s_wave[4 * RW_THREADS / 64];
    if (a.head[RW_H_BAD]) return;
    const int tid = threadIdx.x;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    long long carry[4] = {-1, -1, -1, -1};
    // a sweep is RW_THREADS tiles, a tile a lane; the loads of four sweeps are in flight at once
    for (int64_t base = 0; base < ntiles; base += 4 * RW_THREADS) {
        long long v[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t t = base + q * RW_THREADS + tid;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[q][k] = t < ntiles ? a.carry[4 * t + k] : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t t = base + q * RW_THREADS + tid;
            if (base + q * RW_THREADS >= ntiles) break;  // (the same in every lane)
            long long m[4] = {v[q][0], v[q][1], v[q][2], v[q][3]}, all[4];
            ts_block_excl_max(m, s_wave, all);  // m: the maximum over the lanes in front
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m[k] = m[k] > carry[k] ? m[k] : carry[k];
                m[k] = m[k] > v[q][k] ? m[k] : v[q][k];
                if (t < ntiles) a.carry[4 * t + k] = m[k];
                carry[k] = carry[k] > all[k] ? carry[k] : all[k];
            }
        }
    }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------------
// A's sums for document D: into the tile's table in LDS where D is among its first TS_SLOTS documents, to stats otherwise
__device__ __forceinline__ void ts_put(const TsArgs& a, unsigned long long* s_acc, int64_t kb, int64_t D, const TsAcc& A) {
    const int64_t slot = D - kb;
#pragma unroll
    for (int c = 1; c < TS_COLS; ++c) {
        const unsigned long long v = (unsigned long long)ts_acc_col(A, c);
        if (!v) continue;
        if (slot < TS_SLOTS) {
            if (ts_is_max(c)) atomicMax(&s_acc[slot * TS_COLS + c], v);
            else atomicAdd(&s_acc[slot * TS_COLS + c], v);
        } else {
            ts_global(a.stats + D * TS_COLS + c, c, v);
        }
    }
}

template <int G>
__global__ __launch_bounds__(RW_THREADS) void td_ts_tiles(const TsArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ unsigned long long s_acc[TS_SLOTS * TS_COLS];
    __shared__ long long s_wave[4 * RW_THREADS / 64];
    __shared__ uint8_t s_ascii[128];
    if (rewrite_bad_offsets(a, true)) return;
    const int tid = threadIdx.x;
    if (tid < 128) s_ascii[tid] = a.ascii_cls[tid];
    for (int i = tid; i < TS_SLOTS * TS_COLS; i += RW_THREADS) s_acc[i] = 0;
    const Tables T = ts_tables(a.ascii_cls, a.ucls1, a.ucls2);
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TsTile tl = ts_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        uint32_t w[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
        if (owns) ts_load(a.text, b0, b, we, w);
        __syncthreads();  // (the tile before has read its table and emptied s_acc; s_ascii and s_acc are written)
        const TsTable tb = ts_table(s_off, off_of, a.n_docs, tl);
        __syncthreads();
        TsCursor cur = {-1, 0, 0};
        TsLane S = {-1, -1, -1, -1, false};
        if (owns) {
            cur.D = ts_doc_of(a, s_off, tb, tl.t0, b);
            cur.ds = a.doc_off[cur.D];
            cur.de = a.doc_off[cur.D + 1];
            ts_window_classes(T, s_ascii, a.text, a.doc_off, b0, b, we, w, cur, c, S);
        }
        TsLane L = {-1, -1, -1, -1, false};
        if (G & TS_RUNS) {  // the last positions in front of the window: the lanes in front, behind them the tiles in front
            long long v[4] = {S.lf, S.sp, S.vis, S.let}, all[4];
            ts_block_excl_max(v, s_wave, all);
            if (t > 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long in = a.carry[4 * (t - 1) + k];
                    v[k] = v[k] > in ? v[k] : in;
                }
            }
            L.lf = v[0]; L.sp = v[1]; L.vis = v[2]; L.let = v[3];
        }
        TsAcc A;
        memset(&A, 0, sizeof A);
        if (owns) {
            L.prev_space = ts_space_before(T, s_ascii, a.text, b, cur.ds, cur.de);
            ts_window_walk<G>(a.text, a.doc_off, b0, b, we, w, c, cur, L, A, [&](int64_t D, const TsAcc& X) { ts_put(a, s_acc, tb.kb, D, X); });
        }
        // the lanes' sums for the documents they end in: a wavefront that ends in one document adds them up first
        const int64_t Dw = __shfl(cur.D, 0);
        if (__all(!owns || cur.D == Dw)) {
#pragma unroll
            for (int c2 = 1; c2 < TS_COLS; ++c2) {
                if (ts_is_max(c2)) continue;
                if (!((G & TS_LOCAL) && ((TS_LOCAL_COLS >> c2) & 1u)) && !((G & TS_RUNS) && ((TS_RUNS_COLS >> c2) & 1u))) continue;
                uint32_t s = A.n[c2];
                for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                A.n[c2] = s;
            }
            if (G & TS_RUNS) {
                for (int d = 32; d >= 1; d >>= 1) {
                    A.wmax = ts_max(A.wmax, (int64_t)__shfl_xor((long long)A.wmax, d));
                    A.lmax = ts_max(A.lmax, (int64_t)__shfl_xor((long long)A.lmax, d));
                }
            }
            if ((tid & 63) == 0 && owns) ts_put(a, s_acc, tb.kb, cur.D, A);
        } else if (owns) {
            ts_put(a, s_acc, tb.kb, cur.D, A);
        }
        __syncthreads();
        for (int i = tid; i < TS_SLOTS * TS_COLS; i += RW_THREADS) {
            const unsigned long long v = s_acc[i];
            if (!v) continue;
            const int slot = i / TS_COLS, col = i - slot * TS_COLS;
            ts_global(a.stats + (tb.kb + slot) * TS_COLS + col, col, v);
            s_acc[i] = 0;
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_ts_totals(const TsArgs a) {
    __shared__ long long s_red[RW_THREADS / 64];
    if (a.head[RW_H_BAD] || !a.totals) return;
    long long v[TS_COLS];
    for (int c = 0; c < TS_COLS; ++c) v[c] = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < TS_COLS; ++c) {
            const long long x = (long long)a.stats[d * TS_COLS + c];
            v[c] = ts_is_max(c) ? (v[c] > x ? v[c] : x) : v[c] + x;
        }
    }
#pragma unroll
    for (int c = 0; c < TS_COLS; ++c) {
        const long long r = ts_is_max(c) ? block_max(v[c], s_red) : block_sum(v[c], s_red);
        if (threadIdx.x == 0 && r) ts_global(a.totals + c, c, (unsigned long long)r);
    }
}

}  // namespace

hipError_t launch_textstats(const TsArgs& a, hipStream_t stream) {
    hipError_t e;
    if ((e = rewrite_launch(td_ts_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_ts_reset, rewrite_grid(a.n_docs * TS_COLS + TS_COLS, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if (a.groups & TS_RUNS) {
        if ((e = rewrite_launch(td_ts_carry, tiles, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_ts_prefix, 1, a, stream)) != hipSuccess) return e;
    }
    void (*walk)(TsArgs) = a.groups == TS_LOCAL ? td_ts_tiles<TS_LOCAL> : a.groups == TS_RUNS ? td_ts_tiles<TS_RUNS> : td_ts_tiles<TS_LOCAL | TS_RUNS>;
    if ((e = rewrite_launch(walk, tiles, a, stream)) != hipSuccess) return e;
    return rewrite_launch(td_ts_totals, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream);
}

}  // namespace td
