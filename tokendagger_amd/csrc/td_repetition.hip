// Per-document duplicate-line and duplicate-paragraph statistics (td_repetition_device and what ends in it): text + document offsets ->
// stats[n_docs][RP_COLS] and totals[RP_COLS].  The rule is the contract in include/tokendagger_hip.h; td_repetition_args.h has the rule
// of one byte, the scan's element and its combine, the hash family and the table's word, which the host statement compiles too.
//
// The windows, the tiles, the offsets check and the tile's table of documents are the text passes' frame (td_rewrite_common.h); this
// pass only reads the text.  A unit (a line, a paragraph) is a maximal run of content bytes inside a document; what a byte needs to know
// of the text in front of it is where its unit began and the unit's hash and characters so far, for either kind: RpElem, the element of
// a segmented scan whose combine is associative.  A call is
//   td_rp_docs       the frame's offsets check
//   td_rp_summary    a workgroup a tile: a lane folds its window's bytes into an element, the lanes' elements are combined in order
//                    (shuffles inside a wavefront, LDS across the four) into carry[t]; the unit ends of the tile are counted into head
//   td_rp_prefix     ONE workgroup: carry to its inclusive prefixes over the tiles.  A lane takes a CHUNK of ntiles / 256 consecutive
//                    tiles: it combines them, the workgroup scans the 256 chunk elements, the lane walks its chunk once more and writes.
//                    (No decoupled look-back: nothing here waits for another workgroup.)  Then the capacity: more units than max_units
//                    raise TD_E_CAPACITY; otherwise the call's table gets rp_slots(units) slots.
//   td_rp_reset      stats, totals and the table's slots to 0 (nothing when an error was raised)
//   td_rp_tiles<G>   a workgroup a tile: fold and exclusive scan as above, behind carry[t - 1]; a lane whose window holds a unit's last
//                    byte walks its window again from that prefix and, at the unit's end, looks the unit up in the table (rp_insert):
//                    an empty slot is claimed by one CAS of a word that holds all a later prober needs, a slot with the same tag and kind
//                    is compared (document, length, end, bytes) and probed past when it differs.  One claim per distinct unit, whatever
//                    the order.  The unit's count, bytes and characters go to its document's columns, and to the DUP columns when it
//                    CLAIMED (they hold the distinct units until td_rp_finish): by atomic adds in LDS for the tile's first RP_SLOTS
//                    documents, from there, or at once for later documents, to stats by 64-bit adds.
//   td_rp_finish     a lane a document: DUP = total - distinct; the columns' sums into totals
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores (td_rp_reset, td_rp_finish) and adds touch the
// outputs, and a unit is a duplicate or not by its bytes alone: the results do not depend on the order of the lanes or on the hash.
#include <hip/hip_runtime.h>

#include "td_repetition.h"
#include "td_repetition_scan.h"

namespace td {

namespace {

constexpr int RP_SLOTS = 32;  // documents of a tile whose sums meet in LDS

// a lane's window: its 16 bytes, and which of the 19 bytes from one in front of it to two behind it are LFs
struct RpWindow {
    uint64_t lo, hi;
    uint32_t lf;  // bit i: text[b0 - 1 + i] is an LF, or lies outside the text (inside the window: outside [b, we), 0)
};
__device__ __forceinline__ RpWindow rp_window(const uint8_t* text, int64_t b0, int64_t b, int64_t we, int64_t total) {
    uint32_t w[4];
    rw_load(text, b0, b, we, w);
    RpWindow r;
    r.lo = w[0] | ((uint64_t)w[1] << 32);
    r.hi = w[2] | ((uint64_t)w[3] << 32);
    r.lf = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) r.lf |= (uint32_t)(((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) == 0x0Au) << (k + 1);
    r.lf |= (uint32_t)(b0 - 1 < 0 || text[b0 - 1] == 0x0A);
    r.lf |= (uint32_t)(b0 + 16 >= total || text[b0 + 16] == 0x0A) << 17;
    r.lf |= (uint32_t)(b0 + 17 >= total || text[b0 + 17] == 0x0A) << 18;
    return r;
}

// The bytes [b, we) of the window at b0 behind E (either kind's element in front of b), cur the document of b; both are moved on.
// on_end(kind, p, E[kind], cur) where a unit of a kind of G ends with byte p.  The loop is kept rolled: the window is shifted, not indexed.
template <int G, class End>
__device__ __forceinline__ void rp_walk(const int64_t* doc_off, RpWindow W, int64_t b0, int64_t b, int64_t we, RpCursor& cur, RpElem (&E)[2], End on_end) {
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
        const int64_t p = b0 + k;
        const uint32_t x = (uint32_t)W.lo & 0xFFu, lf = W.lf;
        W.lo = (W.lo >> 8) | (W.hi << 56);
        W.hi >>= 8;
        W.lf >>= 1;
        if (p < b || p >= we) continue;
        rp_advance(doc_off, p, cur);
        if (p == cur.ds) E[0] = E[1] = rp_open(p);
        const bool prev_lf = p == cur.ds || (lf & 1u), next_lf = p + 1 == cur.de || (lf & 4u), next2_lf = p + 2 >= cur.de || (lf & 8u);
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            if (!(G & (1 << kind))) continue;
            const int r = rp_byte(kind, x, prev_lf, next_lf, next2_lf);
            if (r & RP_CONTENT) rp_append(E[kind], x);
            else E[kind] = rp_open(p + 1);
            if (r & RP_END) on_end(kind, p, E[kind], cur);
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_rp_docs(const RpArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// A lane's part of a tile: its window, its document, and the fold of its bytes from the identity into E; returns the unit ends in it.
struct RpLane {
    int64_t b0, b, we;
    bool owns;
    RpWindow W;
    RpCursor cur;  // the document of b
};
template <int G>
__device__ __forceinline__ int rp_lane(const RpArgs& a, int32_t* s_off, const RwTile& tl, int64_t total, RpLane& L, RwTable& tb, RpElem (&E)[2]) {
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    L.b0 = tl.base + 16 * (int64_t)threadIdx.x;
    L.b = L.b0 < 0 ? 0 : L.b0;
    L.we = L.b0 + 16 < total ? L.b0 + 16 : total;
    L.owns = L.b < L.we;
    L.W = RpWindow{0, 0, 0};
    if (L.owns) L.W = rp_window(a.text, L.b0, L.b, L.we, total);
    __syncthreads();  // (the tile before has read its table)
    tb = rw_table(s_off, off_of, a.n_docs, tl);
    __syncthreads();
    E[0] = E[1] = rp_identity();
    L.cur = RpCursor{-1, 0, 0};
    int ends = 0;
    if (L.owns) {
        L.cur.D = rw_doc_of(a.doc_off, s_off, tb, tl.t0, L.b);
        L.cur.ds = a.doc_off[L.cur.D];
        L.cur.de = a.doc_off[L.cur.D + 1];
        RpCursor c = L.cur;
        rp_walk<G>(a.doc_off, L.W, L.b0, L.b, L.we, c, E, [&](int, int64_t, const RpElem&, const RpCursor&) { ++ends; });
    }
    return ends;
}

template <int G>
__global__ __launch_bounds__(RW_THREADS) void td_rp_summary(const RpArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ RpElem s_wave[2 * RP_WAVES];
    __shared__ long long s_red[RP_WAVES];
    if (rewrite_bad_offsets(a, true)) return;
    int64_t total;
    int shift;
    const int64_t ntiles = rp_tiles(a, total, shift);
    long long units = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        RpLane L;
        RwTable tb;
        RpElem E[2], all[2];
        units += rp_lane<G>(a, s_off, tl, total, L, tb, E);
        rp_block_excl(E, s_wave, all);
        if (threadIdx.x == 0) {
            a.carry[2 * t] = all[0];
            a.carry[2 * t + 1] = all[1];
        }
    }
    units = block_sum(units, s_red);
    if (threadIdx.x == 0 && units) __hip_atomic_fetch_add(&a.head[RP_H_UNITS], (unsigned long long)units, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(RW_THREADS) void td_rp_reset(const RpArgs a) {
    if (a.head[RW_H_BAD] || a.head[RW_H_FULL]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.totals && gid < RP_COLS) a.totals[gid] = 0;
    for (int64_t i = gid; i < a.n_docs * RP_COLS; i += step) a.stats[i] = 0;
    const int64_t pairs = (int64_t)(a.head[RP_H_MASK] + 1) / 2;  // (the table is 16-byte aligned and has an even count of slots)
    for (int64_t i = gid; i < pairs; i += step) reinterpret_cast<ulonglong2*>(a.table)[i] = make_ulonglong2(0, 0);
}

// ---- the table --------------------------------------------------------------------------------------------------------------------------
// The unit text[start, start + len) of `kind` in the document c (ds <= start, start + len <= de), h its hash: true when it CLAIMED a slot
// (no unit of the same kind and bytes of its document was there before), false when one was.  The table has more slots than the call has
// units, so an empty one is met; the walk is bounded by the slots all the same.
__device__ __forceinline__ bool rp_insert(const RpArgs& a, uint64_t mask, int kind, const RpCursor& c, int64_t start, int64_t len, uint64_t h) {
    const uint64_t key = rp_key(h, c.D, kind, len), word = rp_word(key, kind, start);
    uint64_t slot = key & mask;
    for (uint64_t n = 0; n <= mask; ++n, slot = (slot + 1) & mask) {
        unsigned long long cur = __hip_atomic_load(&a.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&a.table[slot], 0ull, (unsigned long long)word);
            if (cur == 0) return true;
        }
        if ((cur ^ word) >> RP_START_BITS) continue;  // another tag or kind
        const int64_t rs = (int64_t)(cur & ((1ull << RP_START_BITS) - 1));
        if (rs < c.ds || rs + len > c.de || !rp_ends_at(kind, a.text, rs + len, c.de)) continue;  // another document, or longer
        if (rp_equal(a.text + rs, a.text + start, len)) return false;
    }
    return false;
}

// a unit of document D into its columns: the tile's table in LDS where D is among its first RP_SLOTS documents, stats otherwise
__device__ __forceinline__ void rp_add(const RpArgs& a, unsigned long long* s_acc, int64_t kb, int64_t D, int kind, int64_t len, uint64_t chars, bool claimed) {
    const int64_t slot = D - kb;
    const unsigned long long v[3] = {1ull, (unsigned long long)len, (unsigned long long)chars};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (i >= 3 && !claimed) break;
        const int col = kind * RP_KIND_COLS + i;
        if ((uint64_t)slot < (uint64_t)RP_SLOTS) atomicAdd(&s_acc[slot * RP_COLS + col], v[i % 3]);
        else __hip_atomic_fetch_add(a.stats + D * RP_COLS + col, v[i % 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int G>
__global__ __launch_bounds__(RW_THREADS) void td_rp_tiles(const RpArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ RpElem s_wave[2 * RP_WAVES];
    __shared__ unsigned long long s_acc[RP_SLOTS * RP_COLS];
    if (a.head[RW_H_BAD] || a.head[RW_H_FULL]) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < RP_SLOTS * RP_COLS; i += RW_THREADS) s_acc[i] = 0;
    int64_t total;
    int shift;
    const int64_t ntiles = rp_tiles(a, total, shift);
    const uint64_t mask = a.head[RP_H_MASK];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        RpLane L;
        RwTable tb;
        RpElem E[2], all[2];
        const int ends = rp_lane<G>(a, s_off, tl, total, L, tb, E);  // (its first barrier: the tile before has emptied s_acc)
        rp_block_excl(E, s_wave, all);
        if (L.owns && ends) {
            if (t > 0) {
                E[0] = rp_combine(a.carry[2 * (t - 1)], E[0]);
                E[1] = rp_combine(a.carry[2 * (t - 1) + 1], E[1]);
            }
            rp_walk<G>(a.doc_off, L.W, L.b0, L.b, L.we, L.cur, E, [&](int kind, int64_t p, const RpElem& R, const RpCursor& c) {
                if (R.s < c.ds || R.s > p) return;  // (a unit begins in its document, at or in front of its last byte)
                const int64_t len = p - R.s + 1;
                rp_add(a, s_acc, tb.kb, c.D, kind, len, R.c, rp_insert(a, mask, kind, c, R.s, len, R.h));
            });
        }
        __syncthreads();
        for (int i = tid; i < RP_SLOTS * RP_COLS; i += RW_THREADS) {
            const unsigned long long v = s_acc[i];
            if (!v) continue;
            __hip_atomic_fetch_add(a.stats + tb.kb * RP_COLS + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_acc[i] = 0;
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_rp_finish(const RpArgs a) {
    __shared__ long long s_red[RP_WAVES];
    if (a.head[RW_H_BAD] || a.head[RW_H_FULL]) return;
    long long v[RP_COLS];
    for (int c = 0; c < RP_COLS; ++c) v[c] = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long* row = a.stats + d * RP_COLS;
#pragma unroll
        for (int c = 0; c < RP_COLS; ++c) {
            const bool dup = c % RP_KIND_COLS >= RP_DUP_UNITS;
            const long long x = dup ? (long long)(row[c - RP_DUP_UNITS] - row[c]) : (long long)row[c];
            if (dup) row[c] = (unsigned long long)x;
            v[c] += x;
        }
    }
    if (!a.totals) return;
#pragma unroll
    for (int c = 0; c < RP_COLS; ++c) {
        const long long r = block_sum(v[c], s_red);
        if (threadIdx.x == 0 && r) __hip_atomic_fetch_add(a.totals + c, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

hipError_t launch_repetition(const RpArgs& a, hipStream_t stream) {
    hipError_t e;
    if ((e = rewrite_launch(td_rp_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    void (*summary)(RpArgs) = a.groups == RP_LINES ? td_rp_summary<RP_LINES> : a.groups == RP_PARAS ? td_rp_summary<RP_PARAS> : td_rp_summary<RP_LINES | RP_PARAS>;
    void (*walk)(RpArgs) = a.groups == RP_LINES ? td_rp_tiles<RP_LINES> : a.groups == RP_PARAS ? td_rp_tiles<RP_PARAS> : td_rp_tiles<RP_LINES | RP_PARAS>;
    if ((e = rewrite_launch(summary, tiles, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_rp_prefix, 1, a, stream)) != hipSuccess) return e;
    const int64_t words = std::max<int64_t>(a.n_docs * RP_COLS + RP_COLS, (int64_t)rp_slots(a.max_units) / 2);
    if ((e = rewrite_launch(td_rp_reset, rewrite_grid(words, 4 * RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(walk, tiles, a, stream)) != hipSuccess) return e;
    return rewrite_launch(td_rp_finish, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream);
}

}  // namespace td
