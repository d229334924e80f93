// Decode rows (td_decode_rows*, include/tokendagger_hip.h "decode rows"): ids in segments -> the segments' bytes, their byte
// offsets, the ids each consumed and info[4], with a skip set, a stop set and a rule for negative ids.  Whether an id is live depends
// on whether its segment has stopped in front of it, and that crosses tile edges: the tiles' byte counts are a small monoid (DcrAgg,
// td_decode_rows_args.h), not a sum.  Three launches, nothing waits for another workgroup:
//
//   td_dcr_table / td_dcr_mark   (only when the lists or flags differ from the previous call's) one word per id: byte length, stop
//                   bit, skip bit; the listed ids arrive in td_dcr_mark's arguments, DCR_MARK_IDS a launch.
//   td_dcr_sum      one workgroup per tile of DCR_TILE positions (absolute multiples of the tile), sixteen consecutive ids a lane
//                   (int4 loads where the pointer allows), ONE gather from the table per id: the tile's aggregate.  <PLAIN>
//                   (nothing listed, no flag): nothing stops, the aggregate is the byte sum and no segment is looked for.
//                   Also checks the offsets for a decrease, the grid as a whole, as td_cnt_tiles does.
//   td_dcr_scan     one workgroup: the aggregates to each tile's byte base and entering state, the total, TD_E_CAPACITY,
//                   out_offsets[n_segs], info[0]; a call that visits no position gets its offsets and seg_ids here.
//   td_dcr_emit     per tile, 512 lanes of eight ids: the ids again, the in-tile scan from the entering state, out_offsets / seg_ids of the segments that
//                   start in the tile, the bytes through an LDS window with 16-byte stores (as td_decode_copy: window passes while a
//                   tile's bytes exceed it, a shift when `out` is misaligned), info by block_sum and one atomic per word.
//
// Segments.  Offsets form: the tile's starts are the offsets in [s0, s1]: one workgroup search (group_last_le) for the first, then
// the offsets behind it are read in coalesced steps until one lies above s1, each setting a bit for its position in LDS; a second
// such loop writes out_offsets from the positions' byte prefixes (kept in LDS where a segment starts).  No per-position search: only the position where a segment stops or ends
// bisects for its index (last_le_global), once a segment.  However many empty segments start in a tile, the loop just gets longer.
// Rows form: arithmetic only (div_magic once a lane, then counting).
//
// Bounds.  A position is visited only inside [max(lo, 0), min(hi, n_tokens)); segment indices stay in [0, n_segs] on any offsets;
// a tile writes bytes only inside [base[t], base[t + 1]) and only when the total fits the capacity.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "td_decode_rows_args.h"
#include "td_offsets_dev.h"
#include "td_rows_common.h"

namespace td {

namespace {

static_assert(DCR_THREADS == RC_THREADS && DCR_TILE == RC_TILE && DCR_TILE == 16 * DCR_THREADS, "the row kernels' launch shape");
constexpr int DCR_PER = 16;  // consecutive positions a lane of td_dcr_sum
// td_dcr_emit takes the same tile with twice the lanes, eight positions each: a lane's tokens go into the window one after the
// other, byte by byte from the L2-resident store, and that chain is what the kernel waits for; measured on 110 M ids, 256 lanes of
// sixteen took 1.37 ms where td_decode_copy (1024 lanes of four) takes 0.89.
constexpr int DCR_EMIT_THREADS = 512;
constexpr int DCR_EMIT_PER = DCR_TILE / DCR_EMIT_THREADS;
static_assert(DCR_EMIT_PER == 8 && DCR_EMIT_THREADS % 64 == 0, "two int4 loads a lane");
static_assert(DCR_WIN >= (DCR_TILE + 1) * 4, "the byte prefixes of a tile's positions share the window's LDS");

__global__ __launch_bounds__(DCR_THREADS) void td_dcr_table(uint32_t* table, const uint32_t* tok_off, int32_t max_id) {
    for (int64_t id = (int64_t)blockIdx.x * DCR_THREADS + threadIdx.x; id <= max_id; id += (int64_t)gridDim.x * DCR_THREADS)
        table[id] = (tok_off[id + 1] - tok_off[id]) & DCR_LEN;
}

__global__ __launch_bounds__(DCR_THREADS) void td_dcr_mark(const DcrMarkArgs m) {
    const int i = threadIdx.x;
    if (i >= m.n) return;
    const int32_t id = m.ids[i];
    const uint32_t bits = ((m.bits[i] & 1) ? DCR_SKIP : 0u) | ((m.bits[i] & 2) ? DCR_STOP : 0u);
    if (id <= m.max_id) m.table[id] = ((bits & DCR_SKIP) ? 0u : (m.table[id] & DCR_LEN)) | bits;  // (the ids are unique: one writer)
    else m.hi[m.hi_at[i]] = DcrHi{id, bits};
}

// The rare path of an id above max_id: a listed one (models pad with n_vocab) has its bits, any other is no token.  Kept out of
// line: inlined sixteen times a lane, td_dcr_emit<false, false> is allotted 256 VGPRs.
__device__ __forceinline__ uint32_t dcr_entry_hi(const DcrHi* hi, int32_t n_hi, int32_t id) {
#pragma unroll 1
    for (int k = 0; k < n_hi; ++k)
        if (hi[k].id == id) return hi[k].bits;
    return DCR_BAD;
}

// Offsets form: position j is the last its segment consumes; the segment is the last of [from, to) whose offset is <= j (the
// empty ones in front of it share its offset).  Once a segment, out of line.
__device__ __noinline__ void dcr_seg_end(const int64_t* tok_off, long long* seg_ids, int64_t from, int64_t to, int64_t j) {
    const int64_t d = last_le_global([tok_off](int64_t x) { return tok_off[x]; }, from, to, j);
    const int64_t b = tok_off[d];
    if (b <= j) seg_ids[d] = j + 1 - b;
}

// What an id is: length, DCR_STOP, DCR_SKIP; DCR_BAD (0): no token.
template <bool PLAIN>
__device__ __forceinline__ uint32_t dcr_entry(const DecodeRowsArgs& a, int32_t id) {
    if (id >= 0 && id <= a.max_id) return a.table[id];
    if constexpr (PLAIN) return DCR_BAD;
    if (id < 0) return a.skip_negative ? DCR_SKIP : DCR_BAD;
    return a.n_hi ? dcr_entry_hi(a.hi, a.n_hi, id) : DCR_BAD;
}

// The visited positions [lo, hi), inside the buffer whatever the offsets say.  true: the offsets' ends are wrong.
template <bool ROWS>
__device__ __forceinline__ bool dcr_range(const DecodeRowsArgs& a, int64_t& lo, int64_t& hi, int64_t& bad_at) {
    if constexpr (ROWS) {
        lo = 0;
        hi = a.n_segs * a.row_stride;  // (<= n_tokens: the host has checked it)
        return false;
    }
    lo = a.tok_off[0];
    hi = a.tok_off[a.n_segs];
    if (lo < 0 || hi < lo || hi > a.n_tokens) {
        bad_at = lo < 0 ? 0 : a.n_segs;
        lo = lo < 0 ? 0 : lo;
        hi = hi > a.n_tokens ? a.n_tokens : hi;
        hi = hi < lo ? lo : hi;
        return true;
    }
    return false;
}

// a lane's PER ids at [j0, j0 + PER) inside [s0, s1); positions outside: 0 (never looked at)
template <int PER>
__device__ __forceinline__ void dcr_load(const DecodeRowsArgs& a, int64_t j0, int64_t s0, int64_t s1, int32_t (&v)[PER]) {
    const bool aligned = (((uintptr_t)a.ids) & 15) == 0;
#pragma unroll
    for (int g = 0; g < PER / 4; ++g) {
        const int64_t j = j0 + 4 * g;
        if (aligned && j >= s0 && j + 4 <= s1) {
            const int4 x = *reinterpret_cast<const int4*>(a.ids + j);
            v[4 * g] = x.x; v[4 * g + 1] = x.y; v[4 * g + 2] = x.z; v[4 * g + 3] = x.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[4 * g + q] = (j + q >= s0 && j + q < s1) ? a.ids[j + q] : 0;
        }
    }
}

// Offsets form: the segments whose offset lies in [s0, s1] are [d_first, d_end), a bit per start position into s_flag (bit
// DCR_TILE: s1 itself when the tile is full).  One workgroup search for d_first, then the offsets are read in steps of the
// workgroup's lanes until a step holds one above s1 (tile_table's way, without the table).  By the whole workgroup; barriers inside.
__device__ __forceinline__ void dcr_starts(const DecodeRowsArgs& a, int64_t s0, int64_t s1, int64_t lo, uint32_t* s_flag, int64_t& d_first,
                                           int64_t& d_end) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const auto off_of = [off = a.tok_off](int64_t k) { return off[k]; };
    for (int w = tid; w < DCR_TILE / 32 + 1; w += nt) s_flag[w] = 0;
    // tok_off[0] = lo <= s0: the first tile's starts begin with segment 0, a later tile's behind the last offset below s0
    d_first = s0 == lo ? 0 : group_last_le(off_of, 0, a.n_segs + 1, s0 - 1) + 1;
    __syncthreads();
    d_end = d_first;
    for (;;) {  // (d_end and the counts are the same in every lane)
        const int64_t d = d_end + tid;
        bool below = false;
        if (d <= a.n_segs) {
            const int64_t p = a.tok_off[d];
            below = p <= s1;
            if (below && p >= s0) atomicOr(&s_flag[(p - s0) >> 5], 1u << ((p - s0) & 31));
        }
        const int c = __syncthreads_count(below);
        d_end += c;
        if (c < nt) break;
    }
}

__device__ __forceinline__ bool dcr_flag(const uint32_t* s_flag, int64_t q) { return (s_flag[q >> 5] >> (q & 31)) & 1u; }

__device__ __forceinline__ DcrAgg dcr_shfl_up(const DcrAgg& v, int d) {
    DcrAgg o;
    o.a = __shfl_up(v.a, d);
    o.b = __shfl_up(v.b, d);
    const uint32_t fs = __shfl_up(v.f | (v.st << 1), d);
    o.f = fs & 1u;
    o.st = fs >> 1;
    return o;
}

// The aggregate of everything in front of this lane in the workgroup of NW wavefronts, and the workgroup's; s_wave: NW entries.
template <int NW>
__device__ __forceinline__ DcrAgg dcr_block_excl(const DcrAgg& mine, DcrAgg* s_wave, DcrAgg& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    DcrAgg incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const DcrAgg o = dcr_shfl_up(incl, d);
        if (lane >= d) incl = dcr_op(o, incl);
    }
    __syncthreads();  // (the readers of an earlier call are done)
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    DcrAgg before = dcr_identity();
    total = dcr_identity();
    for (int w = 0; w < NW; ++w) {
        if (w < wv) before = dcr_op(before, s_wave[w]);
        total = dcr_op(total, s_wave[w]);
    }
    DcrAgg ex = dcr_shfl_up(incl, 1);
    if (lane == 0) ex = dcr_identity();
    return dcr_op(before, ex);
}

// Rows form: a lane's row while it counts through its positions.
struct DcrRow {
    int64_t r;
    int64_t q;    // the position inside the row
    int64_t len;  // the row's length, clamped to [0, row_stride]
};
template <bool RAISE>
__device__ __forceinline__ int64_t dcr_row_len(const DecodeRowsArgs& a, int64_t r) {
    if (!a.seg_len || r >= a.n_segs) return a.row_stride;
    const int64_t n = a.seg_len[r];
    if (n < 0 || n > a.row_stride) {
        if constexpr (RAISE) rows_raise(a, TD_E_INVALID, r);
        return n < 0 ? 0 : a.row_stride;
    }
    return n;
}
template <bool RAISE>
__device__ __forceinline__ DcrRow dcr_row_at(const DecodeRowsArgs& a, int64_t p) {
    DcrRow w;
    w.r = div_magic(p, a.row_stride, a.stride_magic);
    w.q = p - w.r * a.row_stride;
    w.len = dcr_row_len<RAISE>(a, w.r);
    return w;
}
template <bool RAISE>
__device__ __forceinline__ void dcr_row_next(const DecodeRowsArgs& a, DcrRow& w) {
    if (++w.q == a.row_stride) {
        w.q = 0;
        ++w.r;
        w.len = dcr_row_len<RAISE>(a, w.r);
    }
}

template <bool ROWS, bool PLAIN>
__global__ __launch_bounds__(DCR_THREADS) void td_dcr_sum(const DecodeRowsArgs a) {
    __shared__ uint32_t s_flag[DCR_TILE / 32 + 1];
    __shared__ DcrAgg s_wave[DCR_THREADS / 64];
    const int tid = threadIdx.x;
    int64_t lo, hi, bad_at = 0;
    const bool bad_ends = dcr_range<ROWS>(a, lo, hi, bad_at);
    if constexpr (!ROWS) {
        if (bad_ends && blockIdx.x == 0 && tid == 0) rows_raise(a, TD_E_INVALID, bad_at);
        for (int64_t d = (int64_t)blockIdx.x * DCR_THREADS + tid; d < a.n_segs; d += (int64_t)gridDim.x * DCR_THREADS)
            if (a.tok_off[d + 1] < a.tok_off[d]) rows_raise(a, TD_E_INVALID, d);
    }
    if ((int64_t)blockIdx.x >= a.n_tiles) return;
    const int64_t t0 = (int64_t)blockIdx.x * DCR_TILE;
    const int64_t s0 = t0 > lo ? t0 : lo;
    const int64_t s1 = t0 + DCR_TILE < hi ? t0 + DCR_TILE : hi;
    if (s0 >= s1) {  // (the same in every lane)
        if (tid == 0) a.agg[blockIdx.x] = dcr_identity();
        return;
    }
    const int64_t j0 = t0 + (int64_t)DCR_PER * tid;
    int32_t v[DCR_PER];
    dcr_load<DCR_PER>(a, j0, s0, s1, v);
    if constexpr (!ROWS && !PLAIN) {
        int64_t d_first, d_end;
        dcr_starts(a, s0, s1, lo, s_flag, d_first, d_end);
    }
    [[maybe_unused]] DcrRow row{0, 0, 0};
    if constexpr (ROWS) row = dcr_row_at<false>(a, j0 < hi ? j0 : 0);
    DcrAgg g = dcr_identity();
#pragma unroll
    for (int k = 0; k < DCR_PER; ++k) {
        const int64_t j = j0 + k;
        if (j >= s0 && j < s1) {
            bool start = false, dead = false;
            if constexpr (ROWS) {
                start = row.q == 0;
                dead = row.q >= row.len;
            } else if constexpr (!PLAIN) {
                start = dcr_flag(s_flag, j - s0);
            }
            if (start) { g.f = 1; g.st = 0; }
            if (!dead && !g.st) {
                const uint32_t e = dcr_entry<PLAIN>(a, v[k]);
                if (g.f) g.b += e & DCR_LEN;
                else g.a += e & DCR_LEN;
                if constexpr (!PLAIN) g.st = e >> 31;
            }
        }
        if constexpr (ROWS) dcr_row_next<false>(a, row);
    }
    DcrAgg total;
    (void)dcr_block_excl<DCR_THREADS / 64>(g, s_wave, total);
    if (tid == 0) a.agg[blockIdx.x] = total;
}

template <bool ROWS>
__global__ __launch_bounds__(DCR_THREADS) void td_dcr_scan(const DecodeRowsArgs a) {
    __shared__ DcrAgg s_wave[DCR_THREADS / 64];
    const int tid = threadIdx.x;
    DcrAgg carry = dcr_identity();
    for (int64_t c0 = 0; c0 < a.n_tiles; c0 += 4 * DCR_THREADS) {
        DcrAgg x[4], g = dcr_identity(), total;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t c = c0 + 4 * tid + q;
            x[q] = c < a.n_tiles ? a.agg[c] : dcr_identity();
            g = dcr_op(g, x[q]);
        }
        DcrAgg run = dcr_op(carry, dcr_block_excl<DCR_THREADS / 64>(g, s_wave, total));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t c = c0 + 4 * tid + q;
            // (tile 0 is entered open; the first visited position is a start, so nothing depends on it)
            if (c < a.n_tiles) a.base[c] = dcr_bytes(run, false) | (dcr_leaves_stopped(run, false) ? DCR_BASE_STOPPED : 0ull);
            run = dcr_op(run, x[q]);
        }
        carry = dcr_op(carry, total);
    }
    const unsigned long long total = dcr_bytes(carry, false);
    if (tid == 0) {
        a.base[a.n_tiles] = total;
        a.out_offsets[a.n_segs] = (long long)total;
        a.info[DCR_I_BYTES] = total;
        if ((long long)total > a.out_cap) rows_raise(a, TD_E_CAPACITY, (int64_t)total);
    }
    int64_t lo, hi, bad_at = 0;
    (void)dcr_range<ROWS>(a, lo, hi, bad_at);
    if (lo >= hi)  // no position is visited, no tile writes: every segment is empty
        for (int64_t d = tid; d < a.n_segs; d += DCR_THREADS) {
            a.out_offsets[d] = 0;
            if (a.seg_ids) a.seg_ids[d] = 0;
        }
}

template <bool ROWS, bool PLAIN>
__global__ __launch_bounds__(DCR_EMIT_THREADS) __attribute__((amdgpu_waves_per_eu(6))) void td_dcr_emit(const DecodeRowsArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DCR_WIN];
    __shared__ uint32_t s_flag[DCR_TILE / 32 + 1];
    __shared__ DcrAgg s_wave[DCR_EMIT_THREADS / 64];
    __shared__ unsigned long long s_red[DCR_EMIT_THREADS / 64];
    uint32_t* const s_pre = reinterpret_cast<uint32_t*>(s_out);  // the byte prefix at a start position, until the window takes the LDS
    const int tid = threadIdx.x;
    int64_t lo, hi, bad_at = 0;
    (void)dcr_range<ROWS>(a, lo, hi, bad_at);
    const int64_t t0 = (int64_t)blockIdx.x * DCR_TILE;
    const int64_t s0 = t0 > lo ? t0 : lo;
    const int64_t s1 = t0 + DCR_TILE < hi ? t0 + DCR_TILE : hi;
    if (s0 >= s1) return;  // (the same in every lane)
    const unsigned long long bw = a.base[blockIdx.x];
    const bool in_stopped = (bw & DCR_BASE_STOPPED) != 0;
    const int64_t base = (int64_t)(bw & ~DCR_BASE_STOPPED);
    const int64_t base_next = (int64_t)(a.base[blockIdx.x + 1] & ~DCR_BASE_STOPPED);
    const bool fits = (int64_t)a.base[a.n_tiles] <= a.out_cap;
    const int64_t j0 = t0 + (int64_t)DCR_EMIT_PER * tid;
    int32_t v[DCR_EMIT_PER];
    dcr_load<DCR_EMIT_PER>(a, j0, s0, s1, v);
    [[maybe_unused]] int64_t d_first = 0, d_end = 0;
    if constexpr (!ROWS) dcr_starts(a, s0, s1, lo, s_flag, d_first, d_end);
    [[maybe_unused]] DcrRow row{0, 0, 0};
    if constexpr (ROWS) row = dcr_row_at<true>(a, j0 < hi ? j0 : 0);
    [[maybe_unused]] const DcrRow row0 = row;
    // the lane's aggregate: what the walk below does, without its effects
    uint32_t ent[DCR_EMIT_PER];
    DcrAgg g = dcr_identity();
#pragma unroll
    for (int k = 0; k < DCR_EMIT_PER; ++k) {
        const int64_t j = j0 + k;
        ent[k] = 0;
        if (j >= s0 && j < s1) {
            bool start, dead = false;
            if constexpr (ROWS) {
                start = row.q == 0;
                dead = row.q >= row.len;
            } else {
                start = dcr_flag(s_flag, j - s0);
            }
            if (start) { g.f = 1; g.st = 0; }
            if (!dead && !g.st) {
                const uint32_t e = dcr_entry<PLAIN>(a, v[k]);
                ent[k] = e;
                if (g.f) g.b += e & DCR_LEN;
                else g.a += e & DCR_LEN;
                if constexpr (!PLAIN) g.st = e >> 31;
            }
        }
        if constexpr (ROWS) dcr_row_next<false>(a, row);
    }
    DcrAgg total;
    const DcrAgg front = dcr_block_excl<DCR_EMIT_THREADS / 64>(g, s_wave, total);
    bool stopped = dcr_leaves_stopped(front, in_stopped);
    const uint32_t lane_at = (uint32_t)dcr_bytes(front, in_stopped);  // the lane's first byte, from the tile's
    uint32_t cbytes = (uint32_t)dcr_bytes(total, in_stopped);
    if ((int64_t)cbytes > base_next - base) cbytes = base_next > base ? (uint32_t)(base_next - base) : 0u;  // (a fence: the sums agree)
    // the walk: errors, the segments' ids, the byte prefixes at the starts, the counts
    uint32_t at = lane_at;
    uint32_t n_emitted = 0, n_skipped = 0, n_stopped = 0;
    if constexpr (ROWS) row = row0;
#pragma unroll
    for (int k = 0; k < DCR_EMIT_PER; ++k) {
        const int64_t j = j0 + k;
        if (j >= s0 && j < s1) {
            bool start, dead = false, last;
            if constexpr (ROWS) {
                start = row.q == 0;
                dead = row.q >= row.len;
                last = row.q + 1 == row.len;
                if (start) {
                    a.out_offsets[row.r] = base + at;
                    if (row.len == 0 && a.seg_ids) a.seg_ids[row.r] = 0;
                }
            } else {
                start = dcr_flag(s_flag, j - s0);
                last = j + 1 == hi || dcr_flag(s_flag, j + 1 - s0);
                if (start) s_pre[j - s0] = at;
            }
            if (start) stopped = false;
            uint32_t e = 0;
            const bool live = !dead && !stopped;
            if (live) {
                e = ent[k];
                const uint32_t len = e & DCR_LEN;
                if (len) ++n_emitted;
                else if (e & DCR_SKIP) ++n_skipped;
                else off_bad_token(a, j);
                at += len;
                if constexpr (!PLAIN) {
                    if (e >> 31) {
                        stopped = true;
                        ++n_stopped;
                    }
                }
                if (a.seg_ids && ((e >> 31) || last)) {  // the segment's ids end here: by its stop, or open at its last position
                    if constexpr (ROWS) {
                        a.seg_ids[row.r] = row.q + 1;
                    } else {
                        dcr_seg_end(a.tok_off, a.seg_ids, d_first > 0 ? d_first - 1 : 0, d_end < a.n_segs ? d_end : a.n_segs, j);
                    }
                }
            }
            ent[k] = live ? e : 0u;  // (what the copy below moves)
        }
        if constexpr (ROWS) dcr_row_next<true>(a, row);
    }
    if constexpr (!ROWS) {
        if (tid == 0) s_pre[s1 - s0] = cbytes;
        __syncthreads();
        for (int64_t d = d_first + tid; d < d_end; d += DCR_EMIT_THREADS) {
            const int64_t p = a.tok_off[d];
            if (p < s0 || p > s1 || (p == s1 && s1 != hi)) continue;  // (s1 itself: the next tile's, but for the last)
            a.out_offsets[d] = base + s_pre[p - s0];
            if (a.seg_ids && d < a.n_segs && a.tok_off[d + 1] == p) a.seg_ids[d] = 0;
        }
    }
    // the three counts as one sum: each is at most DCR_TILE, 16 bits apart they cannot meet
    unsigned long long n = (unsigned long long)n_emitted | ((unsigned long long)n_skipped << 16) | ((unsigned long long)n_stopped << 32);
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if ((tid & 63) == 0) s_red[tid >> 6] = n;
    __syncthreads();  // (and s_pre's readers are done)
    if (tid == 0) {
        n = 0;
        for (int w = 0; w < DCR_EMIT_THREADS / 64; ++w) n += s_red[w];
        if (n & 0xFFFF) __hip_atomic_fetch_add(a.info + DCR_I_EMITTED, n & 0xFFFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((n >> 16) & 0xFFFF) __hip_atomic_fetch_add(a.info + DCR_I_SKIPPED, (n >> 16) & 0xFFFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n >> 32) __hip_atomic_fetch_add(a.info + DCR_I_STOPPED, n >> 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!fits || !a.out) return;  // (TD_E_CAPACITY is td_dcr_scan's; the same in every lane)
    // the bytes: the lanes' tokens into the window, the window out with 16-byte stores
    constexpr uint32_t WIN = DCR_WIN - 16;  // the window is shifted so that LDS and global addresses agree mod 16
    for (uint32_t w0 = 0; w0 < cbytes; w0 += WIN) {
        const uint32_t wn = cbytes - w0 < WIN ? cbytes - w0 : WIN;
        uint8_t* dst = a.out + base + w0;
        const uint32_t shift = (uint32_t)(uintptr_t)dst & 15u;
        uint32_t l0 = lane_at;
#pragma unroll
        for (int k = 0; k < DCR_EMIT_PER; ++k) {
            const uint32_t len = ent[k] & DCR_LEN;
            if (len) {
                // the part of token k inside [w0, w0 + wn)
                const uint32_t b = l0 > w0 ? l0 : w0;
                const uint32_t e = l0 + len < w0 + wn ? l0 + len : w0 + wn;
                if (b < e) {
                    const uint8_t* src = a.src_bytes + a.src_off[v[k]];
                    for (uint32_t q = b; q < e; ++q) s_out[q - w0 + shift] = src[q - l0];
                }
                l0 += len;
            }
        }
        __syncthreads();
        uint32_t head = (16u - shift) & 15u;
        if (head > wn) head = wn;
        if ((uint32_t)tid < head) dst[tid] = s_out[shift + tid];
        const uint32_t nv = (wn - head) >> 4;
        for (uint32_t x = tid; x < nv; x += DCR_EMIT_THREADS)
            *reinterpret_cast<uint4*>(dst + head + 16 * x) = *reinterpret_cast<const uint4*>(s_out + shift + head + 16 * x);
        const uint32_t done = head + 16 * nv;
        if (done + (uint32_t)tid < wn) dst[done + tid] = s_out[shift + done + tid];
        __syncthreads();
    }
}

template <bool ROWS, bool PLAIN>
void dcr_launch(const DecodeRowsArgs& a, int phases, hipStream_t stream) {
    const unsigned tiles = (unsigned)a.n_tiles;
    if (phases & 1) {
        hipLaunchKernelGGL((td_dcr_sum<ROWS, PLAIN>), dim3(tiles ? tiles : 1u), dim3(DCR_THREADS), 0, stream, a);
        hipLaunchKernelGGL(td_dcr_scan<ROWS>, dim3(1), dim3(DCR_THREADS), 0, stream, a);
    }
    if ((phases & 2) && tiles) hipLaunchKernelGGL((td_dcr_emit<ROWS, PLAIN>), dim3(tiles), dim3(DCR_EMIT_THREADS), 0, stream, a);
}

}  // namespace

hipError_t launch_decode_rows_table(uint32_t* table, const uint32_t* tok_off, int32_t max_id, hipStream_t stream) {
    if (max_id < 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>(((int64_t)max_id + DCR_THREADS) / DCR_THREADS, RC_MAX_GRID);
    hipLaunchKernelGGL(td_dcr_table, dim3(grid), dim3(DCR_THREADS), 0, stream, table, tok_off, max_id);
    return hipGetLastError();
}

hipError_t launch_decode_rows_mark(const DcrMarkArgs& m, hipStream_t stream) {
    hipLaunchKernelGGL(td_dcr_mark, dim3(1), dim3(DCR_THREADS), 0, stream, m);
    return hipGetLastError();
}

hipError_t launch_decode_rows(const DecodeRowsArgs& a, bool plain, int phases, hipStream_t stream) {
    if (a.n_tiles < 0 || a.n_tiles > 0x7FFFFFF0ll) return hipErrorInvalidValue;
    if (a.row_stride > 0) {
        if (plain) dcr_launch<true, true>(a, phases, stream);
        else dcr_launch<true, false>(a, phases, stream);
    } else {
        if (plain) dcr_launch<false, true>(a, phases, stream);
        else dcr_launch<false, false>(a, phases, stream);
    }
    return hipGetLastError();
}

}  // namespace td
